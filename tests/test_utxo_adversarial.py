"""The HBM UTXO table and the block pass's duplicate guard (K10) under keys an attacker would choose: txids ground
so that many outpoints share one home slot (long probe chains, chains that wrap past the last slot, tombstones
in the middle of a chain, many lanes racing for one chain), outpoints that differ in one bit of one word, and
outpoints whose K10 fingerprints collide.

The keys are built on the CPU from Python mirrors of the table's two hash functions; every GPU test first checks
the mirrors against the device's own values (``utxo_debug_hashes``), so a changed hash fails these tests instead
of leaving them vacuous, and checks slot layouts against the raw table (``utxo_debug_slots``)."""
import functools
import random

import numpy as np
import pytest

from upow_amd.ledger.utxo import (MISSING, PAYLOAD_DTYPE, STAKE_EXCLUDE, STAKE_ONLY, UtxoIndex, make_payload,
                                  sort_order)

HOSTS = ['host', 'host-py']
BACKENDS = [*HOSTS, pytest.param('gpu', marks=pytest.mark.gpu)]
EMPTY, FULL, TOMB = 0, 1, 2
# csrc/utxo_dev.h UtxoSlot: key words, meta (state | index << 8 | tag << 16), owner fingerprint, padding
SLOT_DTYPE = np.dtype([('k', '<u4', (8,)), ('meta', '<u4'), ('fp', '<u4'), ('pad', '<u4', (2,))])
assert SLOT_DTYPE.itemsize == 48
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------
# mirrors of the device hashes (csrc/utxo_dev.h slot_hash, outpoint_fp) over packed 40-byte records

def _words(recs):
    return np.ascontiguousarray(recs[:, :32]).view('<u4').reshape(len(recs), 8)


def _index_byte(recs):
    return recs[:, 32].astype(np.uint32)


def slot_hash_np(k0, idx):
    h = k0.astype(np.uint32) ^ (np.asarray(idx, np.uint32) * np.uint32(0x9E3779B1))
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x2c1b3c6d)
    return h ^ (h >> np.uint32(12))


def home_np(recs, log2):
    return slot_hash_np(_words(recs)[:, 0], _index_byte(recs)) & np.uint32((1 << log2) - 1)


def _premix_np(k, idx):
    """outpoint_fp before its final mix, without the (k0 << 32 | k1) term when k has 6 columns (words 2..7)"""
    k = k.astype(np.uint64)
    w = k[:, -6:].T
    h = (w[0] << np.uint64(17)) ^ (w[1] * np.uint64(0x9E3779B97F4A7C15)) ^ (w[2] << np.uint64(7)) ^ \
        (w[3] << np.uint64(29)) ^ w[4] ^ (w[5] << np.uint64(41))
    h = h ^ (idx.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
    if k.shape[1] == 8:
        h = h ^ ((k[:, 0] << np.uint64(32)) | k[:, 1])
    return h


def fp_np(recs):
    h = _premix_np(_words(recs), _index_byte(recs))
    h = h ^ (h >> np.uint64(31))
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    return h ^ (h >> np.uint64(29))


def _assert_mirrors(L, recs, log2):
    """The device's own home slots and fingerprints of ``recs`` equal the mirrors'; returns the device values."""
    home, fp = L.utxo_debug_hashes(np.ascontiguousarray(recs), log2)
    assert home.dtype == np.uint32 and fp.dtype == np.uint64 and len(home) == len(fp) == len(recs)
    assert np.array_equal(home, home_np(recs, log2)) and np.array_equal(fp, fp_np(recs))
    return home, fp


# ---------------------------------------------------------------------------------------------------------
# key builders (CPU): packed records {txid 32 B, u32 index, u32 tag}

def _records(txids, idx, tag=0):
    recs = np.zeros((len(txids), 40), dtype=np.uint8)
    recs[:, :32] = txids
    recs[:, 32:36] = np.full(len(txids), idx, np.uint32).view(np.uint8).reshape(-1, 4)
    recs[:, 36:40] = np.full(len(txids), tag, np.uint32).view(np.uint8).reshape(-1, 4)
    return recs


def _with(recs, idx=None, tag=None):
    recs = np.array(recs, dtype=np.uint8).reshape(-1, 40)
    if idx is not None:
        recs[:, 32:36] = np.asarray(idx, np.uint32).reshape(-1, 1).view(np.uint8) if np.ndim(idx) else \
            np.full(len(recs), idx, np.uint32).view(np.uint8).reshape(-1, 4)
    if tag is not None:
        recs[:, 36:40] = np.asarray(tag, np.uint32).reshape(-1, 1).view(np.uint8) if np.ndim(tag) else \
            np.full(len(recs), tag, np.uint32).view(np.uint8).reshape(-1, 4)
    return recs


def _keys(recs):
    """packed records as the (txid hex, index) pairs of UtxoIndex's key API"""
    idx = np.ascontiguousarray(recs[:, 32:36]).view(np.uint32).ravel()
    return [(bytes(r[:32]).hex(), int(i)) for r, i in zip(recs, idx)]


def random_records(n, seed, idx=None):
    rng = np.random.default_rng(seed)
    recs = _records(rng.integers(0, 256, (n, 32), dtype=np.uint8), 0)
    return _with(recs, idx=rng.integers(0, 256, n, dtype=np.uint32) if idx is None else idx)


@functools.lru_cache(maxsize=None)
def _same_home(n, log2, slot, idx, seed):
    rng = np.random.default_rng(seed)
    found = np.zeros(0, np.uint32)
    while len(found) < n:  # ~2^log2 draws per key
        k0 = rng.integers(0, 1 << 32, size=64 << log2, dtype=np.uint32)
        hit = k0[(slot_hash_np(k0, idx & 0xff) & np.uint32((1 << log2) - 1)) == slot]
        found = np.unique(np.concatenate([found, hit]))
    found = rng.permutation(found)[:n]
    txids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    txids[:, :4] = found.astype('<u4').view(np.uint8).reshape(n, 4)
    return _records(txids, idx)


def same_home(n, log2, slot, idx, seed=0):
    """n distinct outpoints of index ``idx`` whose home slot in a 2^log2-slot table is ``slot``: the txid's first
    four bytes are drawn until the mirrored slot_hash lands there, the other 28 bytes are random."""
    return _same_home(n, log2, slot, idx, seed).copy()


def near_equal(rec):
    """For each txid word j in 1..7, a copy of ``rec`` with one bit of word j flipped: same home slot (word 0 and
    the index are kept), so one chain holds keys that differ in each word key_eq compares."""
    out = np.repeat(np.asarray(rec, np.uint8).reshape(1, 40), 7, axis=0)
    for j in range(1, 8):
        out[j - 1, 4 * j + (j % 4)] ^= np.uint8(1 << (j % 8))
    return out


def fp_collide(rec, d):
    """The outpoint with the same 64-bit K10 fingerprint as ``rec``: outpoint_fp XORs txid word 1 and word 6 into
    the same bits 0..31 before mixing, so XORing both with d (non-zero, 32 bits) cancels."""
    assert 0 < d < 1 << 32
    out = np.array(rec, dtype=np.uint8).reshape(40)
    x = np.frombuffer(int(d).to_bytes(4, 'little'), np.uint8)
    out[4:8] ^= x
    out[24:28] ^= x
    return out


def fp_zero(seed, idx=0):
    """An outpoint whose K10 fingerprint is 0: words 0 and 1 enter outpoint_fp as one plain 64-bit XOR term, so
    they can cancel the other words' terms, and the final mix maps 0 to 0."""
    rec = random_records(1, seed, idx=idx)
    rest = int(_premix_np(_words(rec)[:, 2:], _index_byte(rec))[0])
    rec[0, 0:4] = np.frombuffer((rest >> 32).to_bytes(4, 'little'), np.uint8)
    rec[0, 4:8] = np.frombuffer((rest & 0xFFFFFFFF).to_bytes(4, 'little'), np.uint8)
    return rec[0]


def test_key_builders():
    """The builders against the mirrors (the GPU tests check the mirrors against the device)."""
    recs = same_home(40, 8, 250, 3)
    assert len({bytes(r) for r in recs}) == 40 and (home_np(recs, 8) == 250).all() and (recs[:, 32] == 3).all()
    near = near_equal(recs[0])
    assert len({bytes(r) for r in near} | {bytes(recs[0])}) == 8 and (home_np(near, 8) == 250).all()
    diff = _words(near) ^ _words(recs[:1])
    assert [int(np.flatnonzero(d)[0]) for d in diff] == list(range(1, 8))  # word j alone, for j = 1..7
    assert all(bin(int(d.sum())).count('1') == 1 for d in diff)
    b = fp_collide(recs[0], 0x80000001)
    assert bytes(b) != bytes(recs[0]) and fp_np(np.stack([recs[0], b])).tolist() == [int(fp_np(recs[:1])[0])] * 2
    assert int(fp_np(fp_zero(5, 9).reshape(1, 40))[0]) == 0
    # the mirror of slot_hash / outpoint_fp on one hand-computed key: all-zero txid, index 1
    one = _records(np.zeros((1, 32), np.uint8), 1)
    h = 0x9E3779B1
    h ^= h >> 15
    h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
    h ^= h >> 12
    assert int(slot_hash_np(_words(one)[:, 0], _index_byte(one))[0]) == h
    f = 0xC2B2AE3D27D4EB4F
    f ^= f >> 31
    f = (f * 0xBF58476D1CE4E5B9) & M64
    f ^= f >> 29
    assert int(fp_np(one)[0]) == f


# ---------------------------------------------------------------------------------------------------------
# K10: duplicate inputs of one block. The oracle is exact (txid, index byte) equality.

def _filler(n, seed):
    return list(random_records(n, 1000 + seed))


def _pair(seed, d=0x5A5A0001):
    a = random_records(1, seed)[0]
    return a, fp_collide(a, d)


def _case_order(order):
    def build():
        a, b = _pair(11)
        recs = [{'A': a, 'B': b}[c] for c in order]
        return dict(recs=recs + _filler(50, 1), n_dup=len(order) - 2, same_fp=[list(range(len(order)))])
    return build


def _case_chain64():
    a = random_records(1, 12)[0]
    rng = random.Random(12)
    ds = rng.sample(range(1, 1 << 32), 63)
    group = [a] + [fp_collide(a, d) for d in ds]
    recs = group + group
    rng.shuffle(recs)
    return dict(recs=recs + _filler(50, 2), n_dup=64, same_fp=[list(range(128))])


def _case_triple():
    a = random_records(1, 13)[0]
    return dict(recs=[a, a, a] + _filler(50, 3), n_dup=2)


def _case_index_byte():
    a = random_records(1, 14, idx=7)
    f = _filler(50, 4)  # fourth distinct outpoint: not in the index (the dict backend looks up the whole index)
    return dict(recs=f[:3] + [a[0], _with(a, idx=7 + 256)[0]] + f[3:], n_dup=1)


def _case_index_differs():
    a = random_records(1, 15, idx=7)
    return dict(recs=[a[0], _with(a, idx=8)[0]] + _filler(50, 5), n_dup=0)


def _case_tag_only():
    a = random_records(1, 16)
    return dict(recs=[_with(a, tag=0)[0], _with(a, tag=3)[0]] + _filler(50, 6), n_dup=1)


def _case_across_blocks():
    a = random_records(1, 17)[0]
    f = _filler(340, 7)
    return dict(recs=[a] + f[:299] + [a] + f[299:], n_dup=1)  # positions 0 and 300: different 256-thread blocks


def _case_ends(n):
    def build():  # at 129 inputs the scratch table grows from 256 to 512 slots
        a = random_records(1, 18)[0]
        return dict(recs=[a] if n == 1 else [a] + _filler(n - 2, 8) + [a], n_dup=0 if n == 1 else 1)
    return build


def _case_big_amounts():
    a, b = _pair(19)
    c = random_records(1, 20)[0]
    return dict(recs=[a, b, c, b, a] + _filler(50, 9), n_dup=2, same_fp=[[0, 1, 3, 4]],
                amounts=[(1 << 63) - 1, 1 << 63, (1 << 64) - 1], out_amounts=[(1 << 63) - 1, 1 << 63, (1 << 64) - 1])


def _case_fp_zero():
    z = fp_zero(21)  # the scratch word of lane 0 must not read as an empty slot
    return dict(recs=[z, z] + _filler(50, 10), n_dup=1, fp_is_zero=[0, 1])


K10_CASES = {
    'AABB': _case_order('AABB'), 'ABB': _case_order('ABB'), 'BAB': _case_order('BAB'), 'BBA': _case_order('BBA'),
    'chain64': _case_chain64, 'triple': _case_triple, 'index_byte': _case_index_byte,
    'index_differs': _case_index_differs, 'tag_only': _case_tag_only, 'across_blocks': _case_across_blocks,
    'ends1': _case_ends(1), 'ends128': _case_ends(128), 'ends129': _case_ends(129),
    'big_amounts': _case_big_amounts, 'fp_zero': _case_fp_zero,
}


def _wrap64(x):
    return ((x + (1 << 63)) & M64) - (1 << 63)


@functools.lru_cache(maxsize=None)
def _k10_case(name):
    """The case's block (input records, tx segments, output amounts), the outpoints live in the index before it,
    and what the pass must return for it, worked out here with Python integers."""
    case = K10_CASES[name]()
    recs = np.stack(case['recs'])
    n = len(recs)
    rng = random.Random(name)
    key33 = [bytes(r[:33]) for r in recs]
    first = {}
    for pos, k in enumerate(key33):
        first.setdefault(k, pos)
    assert n - len(first) == case['n_dup']  # the oracle agrees with the case's stated count
    # of the distinct outpoints (first-seen order) every fifth is unknown and some sit in another table
    live, state = [], {}
    amounts = list(case.get('amounts', []))
    for j, (k, pos) in enumerate(first.items()):
        if j % 5 == 3:
            continue
        tag = 3 if j % 7 == 5 else 0
        amount = amounts[j] if j < len(amounts) else rng.randrange(1, 1 << 40)
        live.append(pos)
        state[k] = (tag, amount)
    live_recs = _with(recs[live], tag=[state[key33[p]][0] for p in live])
    live_pay = make_payload([state[key33[p]][1] for p in live], [bytes([42]) + rng.randbytes(32) for _ in live])
    in_start = [0]
    while in_start[-1] < n:
        in_start.append(min(n, in_start[-1] + rng.randint(1, 3)))
    n_tx = len(in_start) - 1
    out_start = [0]
    for _ in range(n_tx):
        out_start.append(out_start[-1] + rng.randint(1, 2))
    outs = [rng.randrange(1, 1 << 38) for _ in range(out_start[-1])]
    outs[:len(case.get('out_amounts', []))] = case.get('out_amounts', [])
    tags = [state.get(k, (MISSING, 0))[0] for k in key33]
    amt = [state.get(k, (MISSING, 0))[1] for k in key33]
    fee = [_wrap64(sum(amt[in_start[t]:in_start[t + 1]]) - sum(outs[out_start[t]:out_start[t + 1]]))
           for t in range(n_tx)]
    missing = [sum(1 for g in tags[in_start[t]:in_start[t + 1]] if g != 0) for t in range(n_tx)]
    return dict(case, recs=recs, key33=key33, live_recs=live_recs, live_pay=live_pay,
                block=(recs, np.array(in_start, np.int32), np.array(outs, np.uint64), np.array(out_start, np.int32)),
                tags=np.array(tags, np.uint8), amounts=amt, fee=np.array(fee, np.int64),
                missing=np.array(missing, np.uint32))


def _k10_index(backend, request=None):
    idx = UtxoIndex(backend=backend)
    if backend == 'gpu':
        request.getfixturevalue('gpu')
        from upow_amd.ledger.utxo import _GpuBackend
        idx.be = _GpuBackend(log2_cap=11)
    return idx


def _k10_pass(backend, name, request=None):
    case = _k10_case(name)
    idx = _k10_index(backend, request)
    idx.insert_records(case['live_recs'], case['live_pay'])
    assert idx.duplicates == 0 and len(idx) == len(case['live_recs'])
    return idx.block_inputs(*case['block'], 0)


@functools.lru_cache(maxsize=None)
def _k10_host_reference(name):
    return _k10_pass('host', name)


@pytest.mark.parametrize('name', list(K10_CASES))
@pytest.mark.parametrize('backend', BACKENDS)
def test_k10_duplicates(backend, name, request):
    case = _k10_case(name)
    recs, key33, n = case['recs'], case['key33'], len(case['recs'])
    fp = _assert_mirrors(request.getfixturevalue('gpu'), recs, 8)[1] if backend == 'gpu' else fp_np(recs)
    for group in case.get('same_fp', []):  # the engineered collisions are collisions, of distinct outpoints
        assert len({int(fp[p]) for p in group}) == 1 and len({key33[p] for p in group}) > 1
    assert all(int(fp[p]) == 0 for p in case.get('fp_is_zero', []))
    tags, pay, dup_of, fee, missing, n_dup = _k10_pass(backend, name, request)
    flagged = np.flatnonzero(dup_of)
    print(f'{name}/{backend}: n_in {n}, n_dup {n_dup} (expected {case["n_dup"]}), flagged {flagged.tolist()}')
    assert n_dup == case['n_dup'] == len(flagged)
    # every flagged position names a record with the same 33 key bytes; per outpoint one position is unflagged
    assert all(int(dup_of[p]) - 1 != p and key33[int(dup_of[p]) - 1] == key33[p] for p in flagged)
    unflagged = [key33[p] for p in range(n) if not dup_of[p]]
    assert len(unflagged) == len(set(unflagged)) == len(set(key33))
    # the rest of the pass, against the case's own arithmetic and byte for byte against the host backend
    assert np.array_equal(tags, case['tags'])
    assert [int(a) for a in pay['amount']] == case['amounts']
    assert np.array_equal(fee, case['fee']) and fee.dtype == np.int64
    assert np.array_equal(missing, case['missing'])
    ref = _k10_host_reference(name)
    got = (tags, pay, dup_of, fee, missing)
    for k in (0, 1, 3, 4):
        assert np.array_equal(np.asarray(ref[k]).view(np.uint8), np.asarray(got[k]).view(np.uint8)), k


# ---------------------------------------------------------------------------------------------------------
# engineered probe chains in the HBM table, through the raw handle API (no automatic rehash)

def _slots(L, h):
    s = np.frombuffer(L.utxo_debug_slots(h), dtype=SLOT_DTYPE)
    assert len(s) == L.utxo_capacity(h)
    return s


def _state(slots):
    return slots['meta'] & 3


def _full_slots(slots):
    return np.flatnonzero(_state(slots) == FULL).tolist()


def _slot_of(slots, rec):
    """the FULL slot holding outpoint ``rec`` (key words and index byte), or None"""
    hit = np.flatnonzero((_state(slots) == FULL) & (slots['k'] == _words(rec.reshape(1, 40))[0]).all(axis=1) &
                         (((slots['meta'] >> 8) & 0xff) == rec[32]))
    assert len(hit) <= 1
    return int(hit[0]) if len(hit) else None


def _owner(i):
    """address of owner i; its slot fingerprint (address bytes 1..4) is i"""
    return bytes([42 + (i & 1)]) + int(i).to_bytes(4, 'little') + bytes([i & 0xff] * 28)


def _payloads(n, first=0):
    """payload i: amount first + i and an address (hence an owner fingerprint) of its own"""
    return make_payload([first + i for i in range(n)], [_owner(first + i) for i in range(n)])


def _lookup(L, h, recs):
    tags, pay = L.utxo_lookup(h, np.ascontiguousarray(recs))
    return np.frombuffer(tags, np.uint8), np.frombuffer(pay, PAYLOAD_DTYPE)


def _insert(L, h, recs, pay):
    return L.utxo_insert(h, np.ascontiguousarray(recs), np.ascontiguousarray(pay).view(np.uint8))


def _dump(L, h):
    raw, p = L.utxo_dump_payload(h)
    r, p = np.frombuffer(raw, np.uint8).reshape(-1, 40), np.frombuffer(p, np.uint8).reshape(-1, 80)
    o = sort_order(r)
    return r[o].tobytes(), p[o].tobytes()


def _ring(first, n, cap):
    return sorted((first + i) % cap for i in range(n))


@pytest.fixture
def table(gpu):
    """``make(log2)`` gives a fresh table handle; all are destroyed after the test"""
    made = []

    def make(log2):
        made.append(gpu.utxo_create(log2))
        return made[-1]
    yield make
    for h in made:
        gpu.utxo_destroy(h)


@pytest.mark.gpu
def test_chain_wraps_past_the_last_slot(gpu, table):
    recs = _with(same_home(60, 8, 250, 5, seed=1), tag=np.arange(60) % 7)
    home, _ = _assert_mirrors(gpu, recs, 8)
    assert (home == 250).all()
    h = table(8)
    pay = _payloads(40)
    assert _insert(gpu, h, recs[:40], pay) == (0, 0)
    slots = _slots(gpu, h)
    assert _full_slots(slots) == _ring(250, 40, 256) and (_state(slots) != FULL).sum() == 216
    assert (_state(slots)[34:250] == EMPTY).all()
    tags, got = _lookup(gpu, h, recs)
    assert tags[:40].tolist() == (np.arange(40) % 7).tolist() and got[:40].tobytes() == pay.tobytes()
    assert (tags[40:] == MISSING).all() and got[40:].tobytes() == bytes(80 * 20)
    assert np.frombuffer(gpu.utxo_probe(h, recs), np.uint8).tolist() == tags.tolist()
    for i in (0, 5, 6, 39):  # the slot's key words, index, tag and owner fingerprint are the entry's own
        s = slots[_slot_of(slots, recs[i])]
        assert (int(s['meta']) >> 8) & 0xff == 5 and (int(s['meta']) >> 16) & 0xff == i % 7 and int(s['fp']) == i


@pytest.mark.gpu
def test_near_equal_keys_share_a_chain(gpu, table):
    base = same_home(1, 8, 77, 9, seed=2)
    recs = np.concatenate([base, near_equal(base[0])])
    home, _ = _assert_mirrors(gpu, recs, 8)
    assert (home == 77).all() and len({bytes(r) for r in recs}) == 8
    h = table(8)
    pay = _payloads(8, first=100)
    assert _insert(gpu, h, recs, pay) == (0, 0)
    assert _full_slots(_slots(gpu, h)) == list(range(77, 85))
    tags, got = _lookup(gpu, h, recs)
    assert (tags == 0).all() and got['amount'].tolist() == list(range(100, 108)) and got.tobytes() == pay.tobytes()
    for gone in (3, 7):  # a variant in the middle of the chain, then the one whose word 7 differs
        live = [i for i in range(8) if i not in (3, gone)]
        assert np.frombuffer(gpu.utxo_erase(h, _with(recs[gone:gone + 1], tag=MISSING)), np.uint8).tolist() == [1]
        tags, got = _lookup(gpu, h, recs)
        assert tags.tolist() == [0 if i in live else MISSING for i in range(8)]
        assert got['amount'][live].tolist() == [100 + i for i in live]


def _chain(gpu, table, n=30, home=100, idx=2, seed=3, spare=25):
    """An n-key chain in a 2^8 table whose slot order is the insertion order (one insert call per key): key i
    sits in slot home + i. Returns the handle, n + spare same-home records and the n payloads."""
    recs = same_home(n + spare, 8, home, idx, seed=seed)
    hm, _ = _assert_mirrors(gpu, recs, 8)
    assert (hm == home).all()
    h = table(8)
    pay = _payloads(n)
    for i in range(n):
        assert _insert(gpu, h, recs[i:i + 1], pay[i:i + 1]) == (0, 0)
    slots = _slots(gpu, h)
    assert _full_slots(slots) == list(range(home, home + n))
    assert (slots['k'][home:home + n] == _words(recs[:n])).all()
    assert slots['fp'][home:home + n].tolist() == list(range(n))
    return h, recs, pay


def _erase_5_to_9(gpu, h, recs):
    for i in range(5, 10):
        assert np.frombuffer(gpu.utxo_erase(h, _with(recs[i:i + 1], tag=MISSING)), np.uint8).tolist() == [1]
    slots = _slots(gpu, h)
    assert np.flatnonzero(_state(slots) == TOMB).tolist() == list(range(105, 110))
    assert _full_slots(slots) == [*range(100, 105), *range(110, 130)]
    return slots


@pytest.mark.gpu
def test_tombstones_in_the_middle_of_a_chain(gpu, table):
    h, recs, pay = _chain(gpu, table)
    _erase_5_to_9(gpu, h, recs)
    tags, got = _lookup(gpu, h, recs)
    live = [*range(5), *range(10, 30)]
    assert (tags[live] == 0).all() and got[live].tobytes() == pay[live].tobytes()  # also those behind the tombstones
    assert (tags[5:10] == MISSING).all() and (tags[30:] == MISSING).all() and got[5:10].tobytes() == bytes(400)
    assert np.frombuffer(gpu.utxo_erase(h, _with(recs[5:10], tag=MISSING)), np.uint8).tolist() == [0] * 5


@pytest.mark.gpu
def test_duplicate_behind_a_tombstone_is_found(gpu, table):
    """The insert must walk past the reusable slots 105..109 to see that key 20 is live in slot 120."""
    h, recs, pay = _chain(gpu, table)
    _erase_5_to_9(gpu, h, recs)
    before = _dump(gpu, h)
    assert _insert(gpu, h, _with(recs[20:21], tag=4), _payloads(1, first=7000)) == (0, 1)
    tags, got = _lookup(gpu, h, recs[20:21])
    assert tags.tolist() == [0] and got.tobytes() == pay[20:21].tobytes()
    slots = _slots(gpu, h)
    assert np.flatnonzero(_state(slots) == TOMB).tolist() == list(range(105, 110))
    assert _full_slots(slots) == [*range(100, 105), *range(110, 130)] and _slot_of(slots, recs[20]) == 120
    assert _dump(gpu, h) == before and len(before[0]) == 25 * 40


@pytest.mark.gpu
def test_insert_reuses_the_first_tombstone(gpu, table):
    h, recs, pay = _chain(gpu, table)
    _erase_5_to_9(gpu, h, recs)
    new_pay = _payloads(1, first=9000)
    assert _insert(gpu, h, _with(recs[30:31], tag=6), new_pay) == (0, 0)
    slots = _slots(gpu, h)
    assert _slot_of(slots, recs[30]) == 105 and _state(slots)[105] == FULL
    assert np.flatnonzero(_state(slots) == TOMB).tolist() == list(range(106, 110))
    assert int(slots['fp'][105]) == 9000 and (int(slots['meta'][105]) >> 16) & 0xff == 6
    tags, got = _lookup(gpu, h, recs[30:31])
    assert tags.tolist() == [6] and got.tobytes() == new_pay.tobytes()
    raw, p, total = gpu.utxo_address_scan(h, _owner(9000), 1 << 6)
    assert raw == _with(recs[30:31], tag=6).tobytes() and p == new_pay.tobytes() and total == 9000
    raw, p, total = gpu.utxo_address_scan(h, _owner(5), 0x7f)  # the slot's previous owner
    assert raw == b'' and p == b'' and total == 0
    raw, p, total = gpu.utxo_address_scan(h, _owner(4), 0x7f)  # a neighbour that is still live
    assert raw == recs[4:5].tobytes() and total == 4


@pytest.mark.gpu
def test_erase_races_on_one_chain(gpu, table):
    h, recs, _ = _chain(gpu, table)
    twice = _with(np.concatenate([recs[:30], recs[:30]]), tag=MISSING)
    out = np.frombuffer(gpu.utxo_erase(h, twice), np.uint8)
    assert (out[:30] + out[30:] == 1).all()  # exactly one copy of each key wins
    slots = _slots(gpu, h)
    assert _full_slots(slots) == [] and np.flatnonzero(_state(slots) == TOMB).tolist() == list(range(100, 130))
    assert (_lookup(gpu, h, recs)[0] == MISSING).all() and _dump(gpu, h) == (b'', b'')


def _check_contended(gpu, h, recs, pay):
    slots = _slots(gpu, h)
    full = _full_slots(slots)
    print(f'contention: {len(full)} of {len(recs)} entries in the table')
    assert full == _ring(1000, 400, 1024)
    tags, got = _lookup(gpu, h, recs)
    assert (tags == 1).all() and got.tobytes() == pay.tobytes()  # racing lanes did not cross payloads
    s = np.array([_slot_of(slots, r) for r in recs])
    assert sorted(s.tolist()) == full and slots['fp'][s].tolist() == list(range(400))


@functools.lru_cache(maxsize=None)
def _contended():
    return _with(same_home(400, 10, 1000, 0, seed=4), tag=1), _payloads(400)


@pytest.mark.gpu
def test_400_lanes_race_for_one_chain(gpu, table):
    """More same-home keys in one launch than a wave has lanes: every lane must still find a slot (a lane that
    loses a race lost it to an entry that now holds a slot, so it can lose at most capacity times)."""
    recs, pay = _contended()
    home, _ = _assert_mirrors(gpu, recs, 10)
    assert (home == 1000).all()
    h = table(10)
    res = _insert(gpu, h, recs, pay)
    print(f'contention: utxo_insert returned (no slot, duplicates) = {res}')
    assert res == (0, 0)
    _check_contended(gpu, h, recs, pay)
    h = table(10)  # the block path's form: queued insert, counters collected later
    gpu.utxo_apply_async(h, [(np.ascontiguousarray(recs), np.ascontiguousarray(pay).view(np.uint8))],
                         np.zeros((0, 40), np.uint8))
    res = gpu.utxo_apply_wait(h)
    print(f'contention: utxo_apply_wait returned (pending, no slot, duplicates, erased) = {res}')
    assert res == (True, 0, 0, 0)
    _check_contended(gpu, h, recs, pay)


@pytest.mark.gpu
def test_rehash_of_a_clustered_set(gpu, table):
    recs, pay = _contended()
    assert (_assert_mirrors(gpu, recs, 10)[0] == 1000).all()
    assert set(_assert_mirrors(gpu, recs, 11)[0].tolist()) <= {1000, 2024}
    h = table(10)
    for s in range(0, 400, 50):  # 50 lanes a launch: within what one wave settles alone
        assert _insert(gpu, h, recs[s:s + 50], pay[s:s + 50]) == (0, 0)
    before = _dump(gpu, h)
    o = sort_order(recs)
    assert before == (recs[o].tobytes(), pay[o].tobytes())
    for log2 in (11, 10):
        res = gpu.utxo_rehash(h, log2)
        print(f'rehash of 400 clustered entries to 2^{log2}: (moved, no slot) = {res}')
        assert res == (400, 0)
        assert gpu.utxo_capacity(h) == 1 << log2 and _dump(gpu, h) == before
    assert _full_slots(_slots(gpu, h)) == _ring(1000, 400, 1024)


# ---------------------------------------------------------------------------------------------------------
# model test: the HBM table against the host table over clustered and near-equal keys

class _CountRehash:
    """the native module, recording each rehash as (capacity before, capacity asked for)"""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        return getattr(self._L, name)

    def utxo_rehash(self, h, log2):
        self.calls.append((self._L.utxo_capacity(h), 1 << log2))
        return self._L.utxo_rehash(h, log2)


@pytest.mark.gpu
def test_gpu_table_agrees_with_host_on_clustered_keys(gpu):
    from upow_amd.ledger.utxo import _GpuBackend
    pool = np.concatenate([same_home(24, 8, 255, 1, seed=5), same_home(24, 8, 0, 1, seed=6),
                           same_home(24, 8, 131, 200, seed=7)])
    for base in (pool[3], pool[30], pool[60], random_records(1, 8)[0]):
        pool = np.concatenate([pool, near_equal(base)])
    pool = np.concatenate([pool, random_records(1, 8)])
    home, _ = _assert_mirrors(gpu, pool, 8)
    assert len(pool) == 101 and len({bytes(r[:33]) for r in pool}) == 101
    assert [int((home == s).sum()) >= 24 for s in (255, 0, 131)] == [True] * 3
    keys = _keys(pool)
    g, h = UtxoIndex(backend='gpu'), UtxoIndex(backend='host')
    g.be = _GpuBackend(log2_cap=8)
    g.be.L = counted = _CountRehash(g.be.L)
    rng = random.Random(9)
    owners = [_owner(o) for o in range(5)] + [bytes(range(64))]

    def batch(lo, hi):
        sel = rng.sample(range(len(pool)), rng.randint(lo, hi))  # no outpoint twice in one batch
        pay = make_payload([rng.randrange(1, 1 << 50) for _ in sel], [rng.choice(owners) for _ in sel],
                           [rng.random() < 0.3 for _ in sel])
        return sel, pay

    for step in range(60):
        op = rng.random()
        if op < 0.35:
            sel, pay = batch(5, 30 if step < 40 else 90)
            tag = rng.choice((0, 0, 1, 3, 6))
            for i in (g, h):
                i.insert([keys[k] for k in sel], tag, pay)
        elif op < 0.6:
            sel, _ = batch(5, 40)
            tag = rng.choice((None, None, 0, 3))
            assert (g.erase([keys[k] for k in sel], tag) == h.erase([keys[k] for k in sel], tag)).all()
        elif op < 0.75:
            sel, _ = batch(5, 60)
            tg, pg = g.lookup([keys[k] for k in sel])
            th, ph = h.lookup([keys[k] for k in sel])
            assert (tg == th).all() and pg.tobytes() == ph.tobytes()
        else:  # a block: its created outputs in, then its spent outputs (of any table) out
            sel, pay = batch(5, 30)
            tag = rng.choice((0, 0, 3))
            spent, _ = batch(5, 30)
            for i in (g, h):
                i.apply_block([(_with(pool[sel[:3]], tag=tag), pay[:3]), (_with(pool[sel[3:]], tag=tag), pay[3:])],
                              _with(pool[spent], tag=MISSING))
        assert (g.probe(keys) == h.probe(keys)).all(), step
        assert len(g) == len(h) and g.duplicates == h.duplicates, step
    print(f'model: rehashes (capacity before, after) = {counted.calls}, {len(g)} live, {g.duplicates} duplicates')
    assert any(a == b for a, b in counted.calls) and any(a < b for a, b in counted.calls)
    assert g.be.log2 > 8 and h.duplicates > 0
    rg, pg = g.records_payload()
    rh, ph = h.records_payload()
    assert len(rg) == len(g) and rg.tobytes() == rh.tobytes() and pg.tobytes() == ph.tobytes()
    for tag in (0, 1, 3, 6):
        assert g.set_hash(tag) == h.set_hash(tag)
    for o in owners:
        for sel in (0, STAKE_EXCLUDE, STAKE_ONLY):
            ag, ah = g.address_outputs(o, (0, 1, 3, 6), sel), h.address_outputs(o, (0, 1, 3, 6), sel)
            assert ag[0].tobytes() == ah[0].tobytes() and ag[1].tobytes() == ah[1].tobytes() and ag[2] == ah[2]
