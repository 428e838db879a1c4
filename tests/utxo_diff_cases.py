"""Case builders shared by tests/test_utxo_diff.py and tests/test_utxo_diff_gpu.py: record sets with planted, known
differences against an index's entries (``plant``), an independent oracle of the UTXO diff (``brute_diff``: dicts
over canonical entry bytes built with ``struct``; it does not call ``diff_of``), and comparisons of a ``UtxoDiff``
with either. Not a test file."""
import random
import struct
from types import SimpleNamespace

import numpy as np

from state_digest_cases import arrays, random_entries  # noqa: F401  (re-exported for the two test files)
from upow_amd.ledger.utxo import PAYLOAD_DTYPE

CHANGES = ('tag', 'flag', 'amount_bit0', 'amount_bit40', 'length', 'addr_first', 'addr_last', 'payload_off',
           'payload_on')
NOISE = ('past_length', 'flag_bit1', 'empty_payload')


def keys_of(recs):
    """The 33-byte outpoints (txid | index byte) of packed records; they sort like (txid, index)."""
    return [bytes(r[:33]) for r in np.asarray(recs, np.uint8).reshape(-1, 40)]


def entry_bytes(rec, p):
    """E of one entry from the definition; ``p`` is one payload record or None."""
    tag, flag, length, amount, addr = int(rec[36]), 0, 0, 0, b''
    if p is not None and int(p['len']) in (33, 64):
        length, flag, amount = int(p['len']), int(p['flags']) & 1, int(p['amount'])
        addr = bytes(p['addr'][:length])
    return struct.pack('<32sBBBBQ', bytes(rec[:32]), int(rec[32]), tag, flag, length, amount) + addr


def brute_diff(recs_o, pay_o, recs_i, pay_i, tags=None):
    """(missing, extra, changed) as sorted lists of 33-byte outpoints: of O, cut to ``tags``, against I. I's
    entries outside ``tags`` are never extra; one of them under an outpoint of O makes it changed."""
    inside = (lambda r: True) if tags is None else (lambda r: int(r[36]) in tags)
    index = {bytes(r[:33]): (entry_bytes(r, None if pay_i is None else pay_i[j]), inside(r))
             for j, r in enumerate(recs_i)}
    assert len(index) == len(recs_i)
    missing, changed, named = [], [], set()
    for j, r in enumerate(recs_o):
        if not inside(r):
            continue
        key = bytes(r[:33])
        if key not in index:
            missing.append(key)
            continue
        assert key not in named, 'O repeats a live outpoint'
        named.add(key)
        if index[key][0] != entry_bytes(r, None if pay_o is None else pay_o[j]):
            changed.append(key)
    extra = [k for k, (_, counted) in index.items() if counted and k not in named]
    return sorted(missing), sorted(extra), sorted(changed)


def plant(recs, pay, seed, k=3, kinds=None):
    """O made from I's arrays (recs, pay) with known edits: ``.recs``, ``.pay`` (shuffled), the expected
    ``.missing``, ``.extra``, ``.changed`` (sorted 33-byte outpoints) and ``.edits``: edit name -> outpoints.
    k entries are dropped (extra), k fresh ones added (missing), one fresh entry added that shares a kept entry's
    txid under the other of the indexes 0 and 255 (missing), k entries changed in exactly one field for each name
    in CHANGES, and k given each NOISE edit, which must not show. Every edit takes entries of its own; a set too
    small for all of them gets the ones it has entries for. ``kinds``: the names of the edits to make (default:
    all of CHANGES, NOISE, 'dropped', 'fresh' and 'sibling')."""
    rng = random.Random(seed)
    recs, pay = np.array(recs, dtype=np.uint8).reshape(-1, 40), np.array(pay, dtype=PAYLOAD_DTYPE)
    n = len(recs)
    order = list(range(n))
    rng.shuffle(order)
    full = [i for i in order if int(pay['len'][i]) in (33, 64)]
    bare = [i for i in order if int(pay['len'][i]) not in (33, 64)]
    edits = {name: [] for name in CHANGES + NOISE + ('dropped', 'fresh', 'sibling')}

    def take(pool, name):
        out = [pool.pop() for _ in range(min(k, len(pool)) if kinds is None or name in kinds else 0)]
        edits[name] = [bytes(recs[i, :33]) for i in out]
        return out

    for i in take(full, 'tag'):
        recs[i, 36] = (int(recs[i, 36]) + 1 + rng.randrange(6)) % 7
    for i in take(full, 'flag'):
        pay['flags'][i] ^= 1
    for i in take(full, 'amount_bit0'):
        pay['amount'][i] ^= np.uint64(1)
    for i in take(full, 'amount_bit40'):
        pay['amount'][i] ^= np.uint64(1 << 40)
    for i in take(full, 'length'):
        pay['len'][i] = 97 - int(pay['len'][i])  # 33 <-> 64
    for i in take(full, 'addr_first'):
        pay['addr'][i, 0] ^= 0x80
    for i in take(full, 'addr_last'):
        pay['addr'][i, int(pay['len'][i]) - 1] ^= 0x01
    for i in take(full, 'payload_off'):
        pay[i] = np.zeros(1, dtype=PAYLOAD_DTYPE)[0]
    for i in take(bare, 'payload_on'):
        pay['amount'][i], pay['len'][i] = 1 + rng.randrange(1 << 40), (33, 64)[rng.randrange(2)]
        pay['addr'][i, :int(pay['len'][i])] = np.frombuffer(rng.randbytes(int(pay['len'][i])), np.uint8)
    short = [i for i in full if int(pay['len'][i]) == 33]
    for i in take(short, 'past_length'):
        pay['addr'][i, 33 + rng.randrange(31)] ^= 0xff
    full = [i for i in full if bytes(recs[i, :33]) not in edits['past_length']]
    for i in take(full, 'flag_bit1'):
        pay['flags'][i] ^= 2
    for i in take(bare, 'empty_payload'):
        pay['amount'][i], pay['flags'][i], pay['len'][i] = 999, 1, 3
        pay['addr'][i, :3] = np.frombuffer(b'xyz', np.uint8)
    rest = full + bare
    dropped = take(rest, 'dropped')
    fresh_recs, fresh_pay = arrays(random_entries(k if kinds is None or 'fresh' in kinds else 0, seed + 100003))
    edits['fresh'] = keys_of(fresh_recs)
    if rest and (kinds is None or 'sibling' in kinds):  # a kept entry's txid under the other extreme index
        sib = recs[rest[0]].copy()
        sib[32] = 0 if int(sib[32]) else 255
        if bytes(sib[:33]) not in set(keys_of(recs)):
            fresh_recs = np.concatenate([fresh_recs, sib[None]])
            fresh_pay = np.concatenate([fresh_pay, pay[rest[0]:rest[0] + 1]])
            edits['sibling'] = [bytes(sib[:33])]
    keep = np.array(sorted(set(range(n)) - set(dropped)), dtype=np.intp)
    recs, pay = np.concatenate([recs[keep], fresh_recs]), np.concatenate([pay[keep], fresh_pay])
    shuffle = np.array(rng.sample(range(len(recs)), len(recs)), dtype=np.intp)
    return SimpleNamespace(recs=np.ascontiguousarray(recs[shuffle]), pay=np.ascontiguousarray(pay[shuffle]), edits=edits,
                           missing=sorted(edits['fresh'] + edits['sibling']), extra=sorted(edits['dropped']),
                           changed=sorted(key for name in CHANGES for key in edits[name]))


def check_lists(d, missing, extra, changed):
    """The diff ``d`` lists exactly these outpoints (sorted 33-byte keys), untruncated, with matching counts."""
    assert keys_of(d.missing[0]) == missing and keys_of(d.extra[0]) == extra
    assert keys_of(d.changed[0]) == changed == keys_of(d.changed[2])
    assert (d.n_missing, d.n_extra, d.n_changed) == (len(missing), len(extra), len(changed))
    assert not d.truncated and d.equal == (not missing and not extra and not changed)
    assert len(d.missing[1]) == len(missing) and len(d.extra[1]) == len(extra)
    assert len(d.changed[1]) == len(d.changed[3]) == len(changed)


def check_rows(d, recs_o, pay_o, recs_i, pay_i):
    """Every row of ``d`` is the record and payload its side holds for that outpoint (zeros where O has no
    payloads)."""
    zero = np.zeros(1, dtype=PAYLOAD_DTYPE)[0].tobytes()
    side_o = {bytes(r[:33]): (bytes(r), zero if pay_o is None else pay_o[j].tobytes()) for j, r in enumerate(recs_o)}
    side_i = {bytes(r[:33]): (bytes(r), pay_i[j].tobytes()) for j, r in enumerate(recs_i)}
    for (r, p), side in ((d.missing, side_o), (d.extra, side_i), (d.changed[:2], side_o), (d.changed[2:], side_i)):
        for j in range(len(r)):
            assert side[bytes(r[j, :33])] == (bytes(r[j]), p[j].tobytes())


def assert_same(d, ref):
    """Two diffs agree in every count and, list for list, in every byte."""
    for name in ('n_missing', 'n_extra', 'n_changed', 'compared', 'entries', 'truncated', 'equal'):
        assert getattr(d, name) == getattr(ref, name), name
    for got, want in zip(d.missing + d.extra + d.changed, ref.missing + ref.extra + ref.changed):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
