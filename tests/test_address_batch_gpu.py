"""``utxo_address_scan_batch_kernel`` (K14 for many queries in one table pass) on small HBM tables: the cases
its fingerprint-run search, chunking, resize pass and per-query filters can get wrong, against the host table."""
import random
import struct

import numpy as np
import pytest

from upow_amd.ledger.utxo import (PAYLOAD_DTYPE, STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY, UtxoIndex, _GpuBackend,
                                  make_payload)

pytestmark = pytest.mark.gpu
ALL_TAGS = (0, 3, 5)


def _keys(n, seed):
    rng = random.Random(seed)
    return [(rng.randbytes(32).hex(), rng.randrange(0, 256)) for _ in range(n)]


def _pair(log2_cap):
    """The HBM table at 2^log2_cap slots (256 slots are one block of the scan, 4096 sixteen) and the host table."""
    g = UtxoIndex(backend='gpu')
    g.be = _GpuBackend(log2_cap=log2_cap)
    return g, UtxoIndex(backend='host')


def _addr(fp, rest_seed, length=33, first=42):
    """An address whose owner fingerprint (bytes 1..4, little endian) is ``fp``."""
    rest = random.Random(rest_seed).randbytes(length - 5)
    return bytes([first]) + struct.pack('<I', fp) + rest


def _colliders(fp):
    """Six owners with one fingerprint: they differ in byte 0, byte 5, byte 32 and the length only."""
    base = _addr(fp, 7)
    o_b0 = bytes([43]) + base[1:]
    o_b5 = base[:5] + bytes([base[5] ^ 0x55]) + base[6:]
    o_b32 = base[:32] + bytes([base[32] ^ 0x01])
    o_long = base + random.Random(8).randbytes(31)  # 64 bytes that start with the 33-byte owner's
    o_long2 = o_long[:40] + bytes([o_long[40] ^ 0x80]) + o_long[41:]
    return [base, o_b0, o_b5, o_b32, o_long, o_long2]


def _rows(owners, n, seed, stake_rate=0.0):
    """n outputs spread over ``owners`` in tables 0, 3 and 5: the key, owner, tag, amount and stake flag of each."""
    rng = random.Random(seed)
    keys = _keys(n, seed)
    own = [owners[k % len(owners)] for k in range(n)]  # every owner gets entries
    tags = [rng.choice(ALL_TAGS) for _ in keys]
    amounts = [rng.randrange(1, 1 << 44) for _ in keys]
    stake = [t == 0 and rng.random() < stake_rate for t in tags]
    return keys, own, tags, amounts, stake


def _fill(tables, owners, n, seed, stake_rate=0.0):
    """The outputs of ``_rows``, the same in every table of ``tables``."""
    keys, own, tags, amounts, stake = _rows(owners, n, seed, stake_rate)
    for t in ALL_TAGS:
        sel = [k for k in range(n) if tags[k] == t]
        pay = make_payload([amounts[k] for k in sel], [own[k] for k in sel], [stake[k] for k in sel])
        for idx in tables:
            idx.insert([keys[k] for k in sel], t, pay)
    want = {}
    for o, a in zip(own, amounts):
        c = want.setdefault(o, [0, 0])
        c[0] += 1
        c[1] += a
    return keys, want


def _check(g, h, queries, every_single=True):
    """The batch on the HBM table equals the host table's answers (and the HBM table's own single scans)."""
    got = g.address_outputs_many(queries)
    want = h.address_outputs_many(queries)
    assert len(got) == len(want) == len(queries)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], k
        if every_single:
            s = g.address_outputs(*queries[k])
            assert a[0].tobytes() == s[0].tobytes() and a[1].tobytes() == s[1].tobytes() and a[2] == s[2], k
    return got


@pytest.mark.parametrize('log2_cap,n', [(8, 120), (12, 1900)])
def test_fingerprint_collisions(gpu, log2_cap, n):
    g, h = _pair(log2_cap)
    owners = _colliders(0x5eed1234) + [_addr(0x01000000 + k, k) for k in range(4)]
    _, want = _fill((g, h), owners, n, 31)
    assert g.be.log2 == log2_cap
    got = _check(g, h, [(o, ALL_TAGS, STAKE_ANY) for o in owners])
    for o, r in zip(owners, got):  # exactly its own outpoints and sum
        assert (len(r[0]), r[2]) == tuple(want[o])
        assert all(bytes(p['addr'][:p['len']]) == o for p in r[1])


@pytest.mark.parametrize('log2_cap,n', [(8, 120), (12, 1900)])
@pytest.mark.parametrize('where', ['first', 'last', 'only'])
def test_run_boundaries(gpu, log2_cap, n, where):
    """The equal-fingerprint run at the start, at the end, and as the whole of the sorted query table."""
    g, h = _pair(log2_cap)
    fp = {'first': 0, 'last': 0xffffffff, 'only': 0x80000000}[where]
    run = _colliders(fp)
    others = [] if where == 'only' else [_addr(0x10000000 * k + 5, k) for k in range(1, 12)]
    _, want = _fill((g, h), run + others, n, 37)
    # queries for owners that are not in the table, next to the run in fingerprint order, find nothing
    ghosts = [] if where == 'only' else [_addr(1, 99), _addr(0xfffffffe, 98)]
    queries = [(o, ALL_TAGS, STAKE_ANY) for o in others[:5] + run + others[5:] + ghosts]
    got = _check(g, h, queries)
    for (o, _, _), r in zip(queries, got):
        assert (len(r[0]), r[2]) == tuple(want.get(o, (0, 0)))
    # a run of length one at either end of the table
    _check(g, h, [(run[0], (0,), STAKE_ANY)])


@pytest.mark.parametrize('q', [1024, 1025, 1027])  # the run of four: whole in one launch, split 3 + 1, split 1 + 3
def test_chunking(gpu, q):
    """More than 1024 distinct queries take a second launch; an equal-fingerprint run that straddles the
    boundary between the launches is answered in both."""
    g, h = _pair(12)
    run = _colliders(5000)[:4]
    fillers = [_addr(k, k) for k in range(q - 4)]  # fingerprints 0 .. q-5: sorted ahead of the run
    owners = run + fillers[::9]
    _, want = _fill((g, h), owners, 1900, 41)
    queries = [(o, ALL_TAGS, STAKE_ANY) for o in fillers[:100] + run + fillers[100:]]
    assert len(queries) == q
    got = _check(g, h, queries, every_single=False)
    for (o, _, _), r in zip(queries, got):
        assert (len(r[0]), r[2]) == tuple(want.get(o, (0, 0)))


def test_resize_pass(gpu):
    """More matches than the first pass's 4096-record buffer: all come back once, totals equal the sums."""
    g, h = _pair(12)
    owners = [_addr(77, 1), _addr(77, 2), _addr(78, 3)]
    keys, want = _fill((g, h), owners + [_addr(79, 4)], 5000 * 4 // 3 + 4, 43)
    assert sum(want[o][0] for o in owners) > 4096
    got = _check(g, h, [(o, ALL_TAGS, STAKE_ANY) for o in owners], every_single=False)
    seen = set()
    for o, r in zip(owners, got):
        assert (len(r[0]), r[2]) == tuple(want[o])
        seen.update(bytes(x) for x in r[0])
    assert len(seen) == sum(want[o][0] for o in owners)
    lens = np.array([33] * 3, dtype=np.uint32)
    addrs = np.zeros((3, 64), dtype=np.uint8)
    for k, o in enumerate(owners):
        addrs[k, :33] = np.frombuffer(o, dtype=np.uint8)
    mask = np.full(3, 0b101001, dtype=np.uint32)
    qidx, raw, pay, totals = gpu.utxo_address_scan_batch(g.be.h, addrs, lens, mask, np.zeros(3, dtype=np.uint32))
    assert len(qidx) == sum(want[o][0] for o in owners) and len(raw) == 40 * len(qidx)
    assert [int(t) for t in totals] == [want[o][1] for o in owners]


def test_per_query_filters(gpu):
    """One owner with entries in three tables and stake flags, asked under nine filters in one batch."""
    g, h = _pair(12)
    owner, other = _addr(9, 1), _addr(9, 2)
    _fill((g, h), [owner, other], 1500, 47, stake_rate=0.4)
    queries = [(owner, tags, sel) for tags in ((0,), (3,), (0, 5), ALL_TAGS) for sel in (STAKE_ANY, STAKE_EXCLUDE)]
    queries += [(owner, (0,), STAKE_ONLY), (other, (0,), STAKE_ONLY), (owner, (1, 2, 4, 6), STAKE_ANY)]
    got = _check(g, h, queries)
    for (o, tags, sel), r in zip(queries, got):
        tag = r[0][:, 36:40].copy().view('<u4').ravel()
        assert set(tag.tolist()) <= set(tags)
        staked = (r[1]['flags'] & 1).astype(bool) & (tag == 0)
        assert sel == STAKE_ANY or bool(staked.all() if sel == STAKE_ONLY else not staked.any())
    n = [len(r[0]) for r in got]
    assert n[0] > n[1] > 0 and n[8] > 0 and n[0] == n[1] + n[8] and n[10] == 0  # any = spendable + staked
    assert n[6] == n[0] + n[2] + (n[4] - n[0])  # all tables = table 0 + table 3 + table 5


def test_tombstones_and_rehash(gpu):
    """After erases, tombstoned slots reused by other owners and growth past 2^8 slots the batch still
    equals the host table."""
    g, h = _pair(8)
    owners = [bytes([42 + (o & 1)]) + bytes([o] * 32) for o in range(4)]
    queries = [(o, (0,), sel) for o in owners for sel in (STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY)]
    rng = np.random.default_rng(3)
    for round_ in range(6):
        keys = _keys(200, 1000 + round_)
        own = rng.integers(0, 4, len(keys))
        stake = (rng.random(len(keys)) < 0.3).tolist()
        pay = make_payload([int(a) for a in rng.integers(1, 10**6, len(keys))], [owners[o] for o in own], stake)
        for idx in (g, h):
            idx.insert(keys, 0, pay)
        gone = keys[::3]
        for idx in (g, h):
            idx.erase(gone)
        if round_ == 0:
            _check(g, h, queries)  # tombstones, before any reuse
        for idx in (g, h):
            idx.insert(gone[:20], 0, make_payload([11] * 20, [owners[1]] * 20))  # lands in tombstones
        if round_ == 0:
            _check(g, h, queries)
    assert g.be.log2 > 8
    _check(g, h, queries)


def test_binding_totals_and_arguments(gpu):
    g, h = _pair(12)
    owners = [_addr(3, 1), _addr(3, 2, length=64, first=7), _addr(4, 3)]
    _fill((g, h), owners[:2], 600, 53)
    qs = [owners[0], owners[2], owners[1], owners[0]]
    addrs = np.zeros((4, 64), dtype=np.uint8)
    for k, o in enumerate(qs):
        addrs[k, :len(o)] = np.frombuffer(o, dtype=np.uint8)
    lens = np.array([len(o) for o in qs], dtype=np.uint32)
    masks = np.array([0b101001, 0b101001, 0b1000, 0b1], dtype=np.uint32)
    sels = np.zeros(4, dtype=np.uint32)
    qidx, raw, pay, totals = gpu.utxo_address_scan_batch(g.be.h, addrs, lens, masks, sels)
    assert qidx.dtype == np.uint32 and totals.dtype == np.uint64 and len(totals) == 4
    pay = np.frombuffer(pay, dtype=PAYLOAD_DTYPE)
    recs = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 40)
    assert len(pay) == len(recs) == len(qidx) > 0
    for k in range(4):
        assert int(totals[k]) == int(pay['amount'][qidx == k].sum())
        assert all(bytes(p['addr'][:p['len']]) == qs[k] for p in pay[qidx == k])
    assert totals[1] == 0 and (qidx != 1).all() and totals[0] > totals[3] > 0 and totals[2] > 0
    # bytes after the stated length are not part of the query
    addrs[0, 33:] = 0xee
    again = gpu.utxo_address_scan_batch(g.be.h, addrs, lens, masks, sels)
    assert [int(t) for t in again[3]] == [int(t) for t in totals]
    # no queries: empty arrays; an address longer than 64 bytes: invalid_argument
    e = gpu.utxo_address_scan_batch(g.be.h, np.zeros((0, 64), np.uint8), *(np.zeros(0, np.uint32),) * 3)
    assert len(e[0]) == 0 and e[1] == b'' and e[2] == b'' and len(e[3]) == 0
    lens[2] = 65
    with pytest.raises(ValueError):
        gpu.utxo_address_scan_batch(g.be.h, addrs, lens, masks, sels)


def _single_owners():
    """Owners in the table and queries that must find nothing, at the edges where a batch of one could differ
    from a scan with the query in kernel arguments."""
    cs = _colliders(0x5eed1234)
    o64 = _addr(0x22222222, 11, length=64, first=7)
    # a 33-byte and two 64-byte owners, two more with the first one's fingerprint, and the fingerprints 0 and
    # 0xffffffff: the ends of the one-entry fingerprint table
    present = [cs[0], cs[1], cs[4], o64, _addr(0, 21), _addr(0xffffffff, 22)]
    present += [_addr(0x01000000 + k, k) for k in range(3)]
    # three absent owners with a present fingerprint, the 33-byte prefix of a present 64-byte owner, two ghosts
    absent = [cs[2], cs[3], cs[5], o64[:33], _addr(1, 99), _addr(0xfffffffe, 98)]
    return present, absent


def _expected(rows, addr, tags, sel):
    """(matches, amount sum) of one query, from the inserted rows themselves."""
    _, own, tg, amounts, stake = rows
    hit = [a for o, t, a, s in zip(own, tg, amounts, stake)
           if o == addr and t in tags and (sel == STAKE_ANY or s == (sel == STAKE_ONLY))]
    return len(hit), sum(hit)


def _pairs(raw, pay):
    """The (record, payload) pairs of a raw scan result, in an order of their own (the scan's is the atomics')."""
    return sorted((raw[40 * k:40 * k + 40], pay[80 * k:80 * k + 80]) for k in range(len(raw) // 40))


@pytest.mark.parametrize('log2_cap,n', [(8, 120), (12, 1900), (13, 4200)])
def test_single_is_batch_of_one(gpu, log2_cap, n):
    """``utxo_address_scan`` is ``utxo_address_scan_batch`` with one query: every case against the host table and
    the sums of the inserted rows. At 2^13 slots one owner holds all 4200 outputs, so the scan takes the resize
    pass (more than the first pass's 4096-record buffer)."""
    g, h = _pair(log2_cap)
    present, absent = _single_owners()
    if n > 4096:
        present, absent = present[:1], absent[:1]
    rows = _rows(present, n, 59, stake_rate=0.4)
    _fill((g, h), present, n, 59, stake_rate=0.4)
    if n > 4096:
        assert _expected(rows, present[0], ALL_TAGS, STAKE_ANY)[0] == n
    nowhere = (1, 2, 4, 6)  # tables that hold no owner
    for addr in present + absent:
        for tags in (ALL_TAGS, (0,), nowhere):
            for sel in (STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY):
                want = _expected(rows, addr, tags, sel)
                a, b = g.address_outputs(addr, tags, sel), h.address_outputs(addr, tags, sel)
                assert (len(b[0]), b[2]) == want  # the host table on its own gives what the rows say
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
                raw, pay, total = gpu.utxo_address_scan(g.be.h, addr, sum(1 << t for t in tags), sel)
                amounts = np.frombuffer(pay, dtype=PAYLOAD_DTYPE)['amount']
                assert (len(raw), len(amounts), total, int(amounts.sum())) == (40 * want[0], want[0], want[1], want[1])
                if addr in absent or tags == nowhere:
                    assert raw == b'' and pay == b'' and total == 0
    assert all(_expected(rows, present[0], (0,), sel)[0] > 0 for sel in (STAKE_EXCLUDE, STAKE_ONLY))
    # bytes past the stated length are no part of the query: the bytes form cannot carry any, a batch row can
    row = np.full((1, 64), 0xee, dtype=np.uint8)
    row[0, :33] = np.frombuffer(present[0], dtype=np.uint8)
    one = np.ones(1, dtype=np.uint32)
    qidx, raw_b, pay_b, totals = gpu.utxo_address_scan_batch(g.be.h, row, 33 * one, 0b101001 * one, 0 * one)
    raw, pay, total = gpu.utxo_address_scan(g.be.h, present[0], 0b101001)
    assert len(raw) > 0 and _pairs(raw_b, pay_b) == _pairs(raw, pay) and int(totals[0]) == total and not qidx.any()
    with pytest.raises(ValueError):
        gpu.utxo_address_scan(g.be.h, bytes(65), 1)
