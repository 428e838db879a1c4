"""Case builders shared by tests/test_utxo_merkle.py and tests/test_utxo_merkle_gpu.py: a seeded random pool, the
hand-made entries that probe the sort and each entry length, an independent level-by-level tree, and the comparison
of a snapshot with the hashlib reference (``merkle_of`` / ``prove_of``). Not a test file."""
import hashlib

import numpy as np

from state_digest_cases import arrays, random_entries
from upow_amd.ledger import utxo_proof
from upow_amd.ledger.utxo import merkle_of, prove_of

SIZES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]

_ADDR33 = bytes([43]) + bytes(range(200, 232))
_ADDR64 = bytes(range(64, 128))


def pool(n=1000, seed=91):
    """n random entries as (records, payloads), read-only."""
    recs, pay = arrays(random_entries(n, seed))
    recs.setflags(write=False)
    pay.setflags(write=False)
    return recs, pay


def random_arrays(n, seed):
    """n random entries as (records, payloads) made with numpy alone (large n): every tag, the three entry lengths,
    the stake flag on some entries of tag 0; the 32 random txid bytes make the outpoints distinct."""
    from upow_amd.ledger.utxo import PAYLOAD_DTYPE
    rng = np.random.default_rng(seed)
    recs = np.zeros((n, 40), dtype=np.uint8)
    recs[:, :32] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    recs[:, 32] = rng.integers(0, 256, n, dtype=np.uint8)
    recs[:, 36] = rng.integers(0, 7, n, dtype=np.uint8)
    pay = np.zeros(n, dtype=PAYLOAD_DTYPE)
    length = rng.choice(np.array([0, 33, 64], dtype=np.uint32), n, p=[0.1, 0.6, 0.3])
    pay['len'] = length
    pay['amount'] = np.where(length > 0, rng.integers(1, 1 << 50, n, dtype=np.uint64), 0)
    pay['flags'] = (length > 0) & (recs[:, 36] == 0) & (rng.integers(0, 3, n) == 0)
    addr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    addr[np.arange(64)[None, :] >= length[:, None]] = 0
    pay['addr'] = addr
    return recs, pay


def _txid(base=0x40, **bytes_at):
    t = bytearray([base] * 32)
    for k, v in bytes_at.items():
        t[int(k[1:])] = v
    return bytes(t)


def sort_entries():
    """Hand-made entries (txid, index, tag, flags, amount, addr), in no particular order: each L (0 with and
    without payload bytes that do not count, 33, 64); txids equal except in the first byte, in the last byte, and
    in one byte of each 8-byte sort column; one txid with indexes 0, 1 and 255; one outpoint under two tags."""
    same = _txid(0x77)
    return [
        (_txid(b31=0x41), 3, 0, 0, 5, _ADDR33),           # differs in the last byte
        (_txid(b0=0x41), 3, 0, 0, 6, _ADDR64),            # differs in the first byte
        (_txid(), 3, 0, 1, 7, _ADDR33),
        (_txid(b3=0x3f), 3, 1, 0, 8, _ADDR64),            # one byte of column 4 (bytes 0..7)
        (_txid(b12=0x41), 3, 2, 0, 9, _ADDR33),           # column 3 (bytes 8..15)
        (_txid(b20=0x3f), 3, 3, 0, 10, _ADDR64),          # column 2 (bytes 16..23)
        (_txid(b27=0x80), 3, 4, 0, 11, _ADDR33),          # column 1 (bytes 24..31), a byte with the top bit set
        (same, 255, 0, 0, 12, _ADDR33),
        (same, 0, 0, 0, 13, _ADDR64),
        (same, 1, 5, 0, 14, b''),                         # L = 0
        (same, 2, 6, 1, 999, b'xyz'),                     # a length that does not count: L = 0, zero amount and flag
        (b'\xff' * 32, 9, 6, 0, 15, _ADDR33),
        (b'\xff' * 32, 9, 0, 0, 16, _ADDR64),             # the same outpoint under two tags
        (b'\x00' * 32, 0, 0, 0, 1, _ADDR33),
    ]


def outpoint(rec):
    """(tx_hash, index) of one packed record."""
    return bytes(rec[:32]).hex(), int(rec[32])


def absent_outpoints(recs):
    """Outpoints that are not in ``recs``: before every possible first leaf, after every possible last one, and
    next to existing ones (the same txid with an index nobody has)."""
    have = {outpoint(r) for r in recs}
    out = [('00' * 32, 0), ('ff' * 32, 255)]
    for r in recs[:3]:
        h, i = outpoint(r)
        out += [(h, (i + 1) % 256), (h, (i + 255) % 256)]
    return [o for o in out if o not in have]


def level_by_level(entries):
    """(root, count) of E bytes from the level-by-level rule, written apart from the package: sort, hash the leaves,
    pair neighbours, carry an unpaired last node up unchanged."""
    nodes = [hashlib.sha256(b'\x00' + e).digest() for e in sorted(entries, key=lambda e: e[:34])]
    if not nodes:
        return hashlib.sha256(b'').digest(), 0
    n = len(nodes)
    while len(nodes) > 1:
        up = [hashlib.sha256(b'\x01' + nodes[k] + nodes[k + 1]).digest() for k in range(0, len(nodes) - 1, 2)]
        if len(nodes) % 2:
            up.append(nodes[-1])
        nodes = up
    return nodes[0], n


def check_snapshot(snap, recs, pay, queries=None):
    """``snap`` is the tree of (recs, pay), byte for byte: root, count, levels, and the proofs of ``queries``
    (default: every entry's outpoint plus the absent ones around them), each of which also verifies."""
    root, count = merkle_of(recs, pay)
    assert (snap.root, snap.count) == (root, count) and count == len(recs)
    assert snap.levels == (0 if count == 0 else 1 + (count - 1).bit_length())
    if queries is None:
        queries = [outpoint(r) for r in recs] + absent_outpoints(recs)
    got = snap.prove(queries)
    want = prove_of(recs, pay, queries)
    assert len(got) == len(queries)
    for g, w, (h, i) in zip(got, want, queries):
        assert g == w, (h, i)
        found = utxo_proof.verify_outpoint_all(root, count, h, i, g)
        assert bool(found) == g.present
    return got
