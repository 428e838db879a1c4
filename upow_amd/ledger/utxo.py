"""UTXO index: outpoint (txid, index) -> which of the seven output tables holds it.

reference: the reference answers every "is this outpoint unspent, and in which table" question with
``SELECT ... WHERE (tx_hash, index) = ANY($1::tx_output[])`` against PostgreSQL
(upow/database.py:788-825). Here the ledger keeps that relation in an index with two backends:

* ``gpu``  — the HBM open-addressing table of ``csrc/utxo_table.hip`` (probe/insert/erase kernels,
  one lane per outpoint; a whole block's inputs are one launch);
* ``host`` — the same table in C++ on the host (``csrc/utxo_host.cpp``; CPU-only nodes and the test
  suite), or a Python dict (``host-py``, and when the extension is not built).

Both expose the same batch API; the SQLite tables stay authoritative for address queries and the
index is rebuilt from them after a rollback.
"""
from __future__ import annotations

import functools
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

TAG_BY_TABLE = {
    'unspent_outputs': 0,
    'inode_registration_output': 1,
    'validator_registration_output': 2,
    'validators_voting_power': 3,
    'delegates_voting_power': 4,
    'validators_ballot': 5,
    'inodes_ballot': 6,
}
TABLE_BY_TAG = {v: k for k, v in TAG_BY_TABLE.items()}
MISSING = 0xFF

# per-outpoint payload carried by the index (csrc/utxo_dev.h UtxoPayload): the spent output's
# amount in smallest units, flags (bit 0: unspent_outputs.is_stake = 1) and its raw address bytes
# (33 compressed / 64 uncompressed)
PAYLOAD_DTYPE = np.dtype([('amount', '<u8'), ('len', '<u4'), ('flags', '<u4'), ('addr', 'u1', (64,))])
FLAG_STAKE = 1
STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY = 0, 1, 2  # address-scan selectors
assert PAYLOAD_DTYPE.itemsize == 80


def make_payload(amounts: Sequence[Optional[int]], addrs: Sequence[Optional[bytes]],
                 stake: Optional[Sequence] = None) -> np.ndarray:
    """Payload records; an unknown amount/address gives len 0 (consumers then fall back to SQL).
    ``stake``: per-output is_stake values (truthy -> FLAG_STAKE)."""
    n = len(amounts)
    p = np.zeros(n, dtype=PAYLOAD_DTYPE)
    if n == 0:
        return p
    if stake is not None:
        p['flags'] = np.fromiter((FLAG_STAKE if s else 0 for s in stake), dtype=np.uint32, count=n)
    raw = np.zeros((n, 64), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    amt = np.zeros(n, dtype=np.uint64)
    for k, (a, b) in enumerate(zip(amounts, addrs)):
        if a is None or b is None or len(b) not in (33, 64) or a < 0 or a >= 1 << 64:
            continue
        raw[k, :len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        lens[k] = len(b)
        amt[k] = a
    p['amount'] = amt
    p['len'] = lens
    p['addr'] = raw
    return p

Outpoint = Tuple[str, int]

# Holders report (``UtxoIndex.owner_totals``): one record per owner. An owner is a public key: ``key`` is the
# canonical 33 bytes ``42|43 || x`` that the 33-byte and the 64-byte form of an address both fold to (the rule of
# csrc/txcodec.cpp input_address_strings). ``sums`` are the amount sums modulo 2^64 in OWNER_COLUMNS order: column
# = table tag for tags 1..6; tag 0 is column 7 when staked, else column 0.
OWNER_COLUMNS = ('spendable', 'inode_registration_output', 'validator_registration_output',
                 'validators_voting_power', 'delegates_voting_power', 'validators_ballot', 'inodes_ballot', 'stake')
OWNER_DTYPE = np.dtype([('key', 'u1', (33,)), ('pad', 'u1', (7,)), ('outputs', '<u4'), ('outputs_full', '<u4'),
                        ('sums', '<u8', (8,))])
assert OWNER_DTYPE.itemsize == 112
_KEY33 = np.dtype((np.void, 33))


def _by_mask(top, by) -> int:
    """Argument check of ``owner_totals``: the ``by`` columns as a bit mask."""
    if top is not None and (not isinstance(top, (int, np.integer)) or top < 0):
        raise ValueError('top is None or a count >= 0')
    mask = 0
    for c in by:
        if not isinstance(c, (int, np.integer)) or not 0 <= c < len(OWNER_COLUMNS):
            raise ValueError(f'no owner column {c!r}: columns are 0..{len(OWNER_COLUMNS) - 1}')
        mask |= 1 << int(c)
    if not mask:
        raise ValueError('by names at least one column')
    return mask


def owner_totals_of(recs: np.ndarray, pay: np.ndarray):
    """Group live entries (packed records + payloads, as ``records_payload`` gives them) by owner key:
    (OWNER_DTYPE records ascending by key, info). What the host backends run, and the reference the HBM
    aggregation is tested against."""
    tags = np.ascontiguousarray(recs[:, 36:40]).view('<u4').ravel() if len(recs) else np.zeros(0, np.uint32)
    ok = ((pay['len'] == 33) | (pay['len'] == 64)) & (tags <= 6)
    p, t = pay[ok], tags[ok]
    n = len(p)
    full = p['len'] == 64
    addr = p['addr'].reshape(n, 64)
    key = np.empty((n, 33), dtype=np.uint8)
    key[:, 0] = np.where(full, 42 + (addr[:, 32] & 1), np.where(addr[:, 0] == 43, 43, 42))
    key[:, 1:] = np.where(full[:, None], addr[:, :32], addr[:, 1:33])
    col = np.where((t == 0) & ((p['flags'] & FLAG_STAKE) != 0), 7, t).astype(np.intp)
    uniq, inv = np.unique(key.view(_KEY33).ravel(), return_inverse=True)
    inv = inv.ravel()
    owners = np.zeros(len(uniq), dtype=OWNER_DTYPE)
    owners['key'] = uniq.view(np.uint8).reshape(-1, 33)
    sums = np.zeros((len(uniq), 8), dtype=np.uint64)
    np.add.at(sums, (inv, col), p['amount'])  # uint64: modulo 2^64
    owners['sums'] = sums
    owners['outputs'] = np.bincount(inv, minlength=len(uniq))
    owners['outputs_full'] = np.bincount(inv[full], minlength=len(uniq))
    info = {'owners': len(uniq), 'outputs': n, 'skipped': int(len(pay) - n), 'totals': sums.sum(axis=0, dtype=np.uint64)}
    return _owners_in_order(owners, None, 0xff), info


def _owners_in_order(owners: np.ndarray, top: Optional[int], by_mask: int) -> np.ndarray:
    """Owner records ascending by key; with ``top``, the first ``top`` in (metric descending, key ascending)
    order, the metric being the sum of the ``by_mask`` columns modulo 2^64."""
    if len(owners) > 1:
        key = np.ascontiguousarray(owners['key'])
        # the first eight bytes as one big-endian word order random keys; equal words: all 33 bytes decide
        head = np.ascontiguousarray(key[:, :8]).view('>u8').ravel()
        order = np.argsort(head, kind='stable')
        if (head[order][1:] == head[order][:-1]).any():
            order = np.argsort(key.view(_KEY33).ravel(), kind='stable')
        owners = owners[order]
    if top is None:
        return owners
    cols = [c for c in range(8) if (by_mask >> c) & 1]
    metric = owners['sums'][:, cols].sum(axis=1, dtype=np.uint64)
    return owners[np.argsort(~metric, kind='stable')[:top]]  # ~m = 2^64 - 1 - m: descending, ties by key


# State digest (``UtxoIndex.state_digest``): LtHash16/1024 (Lewi et al., "Securing Update Propagation with
# Homomorphic Hashing") over every live entry WITH its payload. For an entry with key (txid, index, tag) and
# payload (amount, len, flags, addr), L = len if it is 33 or 64, else 0 (then amount and flags count as 0; an
# entry without payload has L = 0):
#   E = txid[32] | u8(index) | u8(tag) | u8(flags & 1) | u8(L) | u64le(amount) | addr[0:L]
#   lane[16 c + k] = the big-endian u16 at bytes 2k, 2k + 1 of SHA-256(E | u8(c)),   c = 0..63, k = 0..15
# The digest of a set is the lane-wise sum modulo 2^16 of its entries' 1024 lanes plus the entry count, so
# digest(after a block) = digest(before) + digest(created) - digest(spent). 2 KB, not 32 bytes: anyone can put
# chosen entries into the set, and a short additive hash falls to the generalised-birthday attack.
STATE_LANES = 1024
_STATE_DOMAIN = b'upow-utxo-state-v1'
ALL_TAGS_MASK = 0x7f
DIGEST_HOST_THREADS = 16


class StateDigest:
    """``state`` (1024 x uint16) and ``count``. ``+`` / ``-`` are lane-wise modulo 2^16 on the state and plain
    on the count; ``tobytes()`` is the state as 1024 little-endian u16, ``hex()`` the short id
    SHA-256(b'upow-utxo-state-v1' | u64le(count) | state)."""
    __slots__ = ('state', 'count')

    def __init__(self, state=None, count: int = 0):
        if state is None:
            self.state = np.zeros(STATE_LANES, dtype=np.uint16)
        elif isinstance(state, (bytes, bytearray, memoryview)):
            self.state = np.frombuffer(bytes(state), dtype='<u2').astype(np.uint16)
        else:
            self.state = np.array(state, dtype=np.uint16).ravel()
        if self.state.shape != (STATE_LANES,):
            raise ValueError(f'a state digest has {STATE_LANES} lanes')
        self.count = int(count)

    def __add__(self, other: 'StateDigest') -> 'StateDigest':
        return StateDigest(self.state + other.state, self.count + other.count)  # uint16 arrays wrap

    def __sub__(self, other: 'StateDigest') -> 'StateDigest':
        return StateDigest(self.state - other.state, self.count - other.count)

    def __eq__(self, other):
        if not isinstance(other, StateDigest):
            return NotImplemented
        return self.count == other.count and bool((self.state == other.state).all())

    def __hash__(self):
        return hash((self.count, self.tobytes()))

    def tobytes(self) -> bytes:
        return self.state.astype('<u2').tobytes()

    def hex(self) -> str:
        import hashlib
        return hashlib.sha256(_STATE_DOMAIN + (self.count % (1 << 64)).to_bytes(8, 'little')
                              + self.tobytes()).hexdigest()

    def __repr__(self):
        return f'StateDigest({self.hex()}, count={self.count})'


def _digest_arrays(recs, pay):
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 40)
    if pay is not None:
        pay = np.ascontiguousarray(pay)
        if pay.dtype != PAYLOAD_DTYPE:
            pay = pay.view(np.uint8).reshape(-1).view(PAYLOAD_DTYPE)
        if len(pay) != len(recs):
            raise ValueError('one payload per record')
    return recs, pay


def state_digest_of(recs: np.ndarray, pay: Optional[np.ndarray]) -> StateDigest:
    """The state digest of packed records + payloads (``pay=None``: every entry has L = 0) with hashlib and
    numpy: what the ``host-py`` backend runs, and the reference the native and the HBM passes are tested
    against."""
    import hashlib
    recs, pay = _digest_arrays(recs, pay)
    n = len(recs)
    acc = np.zeros(STATE_LANES, dtype=np.uint64)
    raw = recs.tobytes()
    praw = pay.tobytes() if pay is not None else None
    lanes = bytearray(2 * STATE_LANES)
    for i in range(n):
        r = raw[40 * i:40 * i + 40]
        head, amount, addr = bytes((r[32], r[36], 0, 0)), bytes(8), b''
        if praw is not None:
            p = praw[80 * i:80 * i + 80]
            length = int.from_bytes(p[8:12], 'little')
            if length in (33, 64):
                head, amount, addr = bytes((r[32], r[36], p[12] & 1, length)), p[0:8], p[16:16 + length]
        h = hashlib.sha256(r[:32] + head + amount + addr)
        for c in range(64):
            hc = h.copy()
            hc.update(bytes((c,)))
            lanes[32 * c:32 * c + 32] = hc.digest()
        acc += np.frombuffer(bytes(lanes), dtype='>u2')
    return StateDigest((acc & 0xffff).astype(np.uint16), n)


def records_digest(recs: np.ndarray, pay: Optional[np.ndarray], device: Optional[str] = None,
                   threads: Optional[int] = None) -> StateDigest:
    """The state digest of packed records + payloads (a block's created or spent entries; ``pay=None``: no
    payloads). ``device='gpu'``: the records kernel of csrc/utxo_digest.hip; ``'cpu'``: the native host routine
    (csrc/utxo_digest_host.cpp) on ``threads`` (default 16) threads of the host worker pool, or
    :func:`state_digest_of` when the extension is not built. ``None``: the GPU when there is one. With
    ``threads=1`` the host routine runs on the calling thread and leaves the pool alone."""
    recs, pay = _digest_arrays(recs, pay)
    if device is None:
        from ..ops.native import gpu_available
        device = 'gpu' if gpu_available() else 'cpu'
    if device not in ('gpu', 'cpu'):
        raise ValueError("device is 'gpu', 'cpu' or None")
    praw = None if pay is None else pay.view(np.uint8)
    if device == 'gpu':
        from ..ops.native import require_gpu
        return StateDigest(*require_gpu().utxo_records_digest(recs, praw))
    try:
        from ..ops.native import lib
        fn = lib().utxo_records_digest_host
    except (ImportError, AttributeError):
        return state_digest_of(recs, pay)
    return StateDigest(*fn(recs, praw, DIGEST_HOST_THREADS if threads is None else int(threads)))


def _tag_mask(tags) -> int:
    """Argument check of ``state_digest``: the tables to cover as a bit mask (``None``: tags 0..6)."""
    if tags is None:
        return ALL_TAGS_MASK
    mask = 0
    for t in tags:
        if not isinstance(t, (int, np.integer)) or not 0 <= t <= 31:
            raise ValueError(f'no table tag {t!r}: tags are 0..31')
        mask |= 1 << int(t)
    return mask


def _record_words(recs: np.ndarray) -> np.ndarray:
    """Packed records (n x 40 bytes) as n x 10 little-endian words (no copy when they are contiguous): the txid's
    eight, the index, the tag."""
    return np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 40).view('<u4')


def _masked(recs: np.ndarray, pay: np.ndarray, mask: int):
    """The entries of (recs, pay) whose tag's bit is set in ``mask`` (``pay`` may be None)."""
    tags = _record_words(recs)[:, 9]
    keep = np.array([(mask >> t) & 1 for t in range(32)] + [0], dtype=bool)[np.minimum(tags, 32)]
    if keep.all():  # the usual case (every table asked for): no 120-byte-per-entry copy
        return np.ascontiguousarray(recs), None if pay is None else np.ascontiguousarray(pay)
    return np.ascontiguousarray(recs[keep]), None if pay is None else np.ascontiguousarray(pay[keep])


# UTXO proofs (``UtxoIndex.merkle_snapshot``): an RFC 6962 Merkle tree over the entries E above, in ascending order
# of E's first 34 bytes (txid, index, tag), so that ONE entry can be checked against ``(root, count)`` by somebody who
# holds nothing else: ``leaf = SHA-256(0x00 | E)``, ``node = SHA-256(0x01 | left | right)``, the tree of n leaves
# split at the largest power of two below n, the empty set's root SHA-256 of the empty string. The definition is in
# csrc/native.h and docs/WIRE_FORMAT.md; the verifier is ledger/utxo_proof.py (pure Python).
def entries_of(recs: np.ndarray, pay: Optional[np.ndarray]) -> List[bytes]:
    """E of every packed record + payload (``pay=None``: every entry has L = 0), in the order given."""
    recs, pay = _digest_arrays(recs, pay)
    raw = recs.tobytes()
    praw = pay.tobytes() if pay is not None else None
    out = []
    for i in range(len(recs)):
        r = raw[40 * i:40 * i + 40]
        head, amount, addr = bytes((r[32], r[36], 0, 0)), bytes(8), b''
        if praw is not None:
            p = praw[80 * i:80 * i + 80]
            length = int.from_bytes(p[8:12], 'little')
            if length in (33, 64):
                head, amount, addr = bytes((r[32], r[36], p[12] & 1, length)), p[0:8], p[16:16 + length]
        out.append(r[:32] + head + amount + addr)
    return out


class _ReferenceTree:
    """The tree of sorted entries from the RFC's recursive definition (MTH and PATH of RFC 9162 2.1.1 / 2.1.3.1),
    subtree hashes kept by leaf range: what ``merkle_of`` / ``prove_of`` and the ``host-py`` backend run."""

    def __init__(self, entries: List[bytes]):
        from .utxo_proof import leaf_hash
        self.entries = sorted(entries, key=lambda e: e[:34])  # stable: equal keys keep their order
        self.keys = [e[:34] for e in self.entries]
        self.leaves = [leaf_hash(e) for e in self.entries]
        self.memo: Dict[Tuple[int, int], bytes] = {}

    def mth(self, lo: int, hi: int) -> bytes:
        from .utxo_proof import EMPTY_ROOT, node_hash
        if hi == lo:
            return EMPTY_ROOT
        if hi - lo == 1:
            return self.leaves[lo]
        got = self.memo.get((lo, hi))
        if got is None:
            k = 1 << ((hi - lo - 1).bit_length() - 1)  # the largest power of two below n
            got = self.memo[(lo, hi)] = node_hash(self.mth(lo, lo + k), self.mth(lo + k, hi))
        return got

    def path(self, m: int, lo: int, hi: int) -> List[bytes]:
        if hi - lo == 1:
            return []
        k = 1 << ((hi - lo - 1).bit_length() - 1)
        if m < lo + k:
            return self.path(m, lo, lo + k) + [self.mth(lo + k, hi)]
        return self.path(m, lo + k, hi) + [self.mth(lo, lo + k)]

    def levels(self) -> int:
        n = len(self.entries)
        return 0 if n == 0 else 1 + (n - 1).bit_length()

    def prove(self, outpoints):
        import bisect
        from .utxo_proof import LeafProof, OutpointProof, query_key
        n, out = len(self.entries), []
        for tx_hash, index in outpoints:
            want = query_key(tx_hash, index)
            at = bisect.bisect_left(self.keys, want + b'\0')
            end = at
            while end < n and self.keys[end][:33] == want:
                end += 1
            pos = list(range(at, end)) if end > at else [p for p in (at - 1, at) if 0 <= p < n]
            out.append(OutpointProof(tx_hash, index, end > at,
                                     [LeafProof(p, self.entries[p], self.path(p, 0, n)) for p in pos]))
        return out


def merkle_of(recs: np.ndarray, pay: Optional[np.ndarray]) -> Tuple[bytes, int]:
    """``(root, count)`` of packed records + payloads with hashlib, from the recursive RFC definition: the reference
    the native and the HBM builds are tested against."""
    t = _ReferenceTree(entries_of(recs, pay))
    return t.mth(0, len(t.entries)), len(t.entries)


def prove_of(recs: np.ndarray, pay: Optional[np.ndarray], outpoints: Sequence[Outpoint]):
    """The :class:`~upow_amd.ledger.utxo_proof.OutpointProof` of each ``(tx_hash, index)`` in the set of packed
    records + payloads: the reference, as :func:`merkle_of`."""
    return _ReferenceTree(entries_of(recs, pay)).prove(outpoints)


class MerkleSnapshot:
    """The Merkle tree of one state of an index (or of a record set): ``root``, ``count``, ``levels`` (stored levels,
    the leaves' included) and ``nbytes`` held, and :meth:`prove`. It owns its buffers (HBM for the GPU backend) and
    answers whatever happens to the index afterwards, until :meth:`close`; also a context manager."""

    def __init__(self, lib=None, sid: Optional[int] = None, tree: Optional[_ReferenceTree] = None):
        self._lib, self._sid, self._tree = lib, sid, tree
        if tree is not None:
            self.root, self.count, self.levels = tree.mth(0, len(tree.entries)), len(tree.entries), tree.levels()
            self.nbytes = sum(map(len, tree.entries)) + 32 * (2 * self.count)
            self.on_device = False
        else:
            info = lib.utxo_merkle_info(sid)
            self.root, self.count, self.levels = info['root'], int(info['count']), int(info['levels'])
            self.nbytes, self.on_device = int(info['bytes']), bool(info['on_device'])

    def prove(self, outpoints: Sequence[Outpoint]):
        """One :class:`~upow_amd.ledger.utxo_proof.OutpointProof` per ``(tx_hash, index)``, in the order asked."""
        from .utxo_proof import LeafProof, OutpointProof
        outpoints = [(str(h), int(i)) for h, i in outpoints]
        if self._tree is not None:
            return self._tree.prove(outpoints)
        if self._sid is None:
            raise ValueError('the snapshot is closed')
        if not outpoints:
            return []
        for _, i in outpoints:
            if not 0 <= i <= 255:
                raise ValueError('an output index is in 0..255')
        present, first, position, slots, path_first, path = self._lib.utxo_merkle_prove(self._sid, pack_records(outpoints))
        leaves = []
        for j, pos in enumerate(position):
            slot = slots[112 * j:112 * j + 112]
            hashes = path[32 * path_first[j]:32 * path_first[j + 1]]
            leaves.append(LeafProof(int(pos), slot[:int.from_bytes(slot[108:112], 'little')],
                                    [hashes[k:k + 32] for k in range(0, len(hashes), 32)]))
        return [OutpointProof(h, i, bool(present[k]), leaves[first[k]:first[k + 1]])
                for k, (h, i) in enumerate(outpoints)]

    def close(self):
        sid, self._sid, self._tree = self._sid, None, None
        if sid is not None and self._lib is not None:
            self._lib.utxo_merkle_free(sid)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return f'MerkleSnapshot({self.root.hex()}, count={self.count})'


def records_merkle(recs: np.ndarray, pay: Optional[np.ndarray], device: Optional[str] = None,
                   threads: Optional[int] = None, *, launch_lever: int = 0) -> MerkleSnapshot:
    """The :class:`MerkleSnapshot` of packed records + payloads (``pay=None``: no payloads). ``device='gpu'``: the
    kernels of csrc/utxo_merkle.hip; ``'cpu'``: the native host routine (csrc/utxo_merkle_host.cpp) on ``threads``
    (default 16) host threads, or the hashlib reference when the extension is not built. ``None``: the GPU when
    there is one."""
    recs, pay = _digest_arrays(recs, pay)
    if device is None:
        from ..ops.native import gpu_available
        device = 'gpu' if gpu_available() else 'cpu'
    if device not in ('gpu', 'cpu'):
        raise ValueError("device is 'gpu', 'cpu' or None")
    praw = None if pay is None else pay.view(np.uint8)
    if device == 'gpu':
        from ..ops.native import require_gpu
        L = require_gpu()
        return MerkleSnapshot(L, L.utxo_merkle_build_records(recs, praw, launch_lever))
    try:
        from ..ops.native import lib
        L = lib()
        fn = L.utxo_merkle_build_records_host
    except (ImportError, AttributeError):
        return MerkleSnapshot(tree=_ReferenceTree(entries_of(recs, pay)))
    return MerkleSnapshot(L, fn(recs, praw, DIGEST_HOST_THREADS if threads is None else int(threads)))


# UTXO diff (``UtxoIndex.diff_records``): WHERE the index and a record set differ, an entry being what the state
# digest hashes (E above) and the outpoint (txid, index) alone its identity. Of the index I against the other set O:
# ``missing`` are the outpoints of O that I lacks, ``extra`` those of I that O lacks, ``changed`` those in both whose
# E differ (tag, stake flag, L, amount or addr[0:L]; bytes past L, other flag bits and the amount or flag of an
# L = 0 entry do not count). For O without repeated outpoints the diff is empty exactly when the digests agree.
DIFF_LIMIT = 65536


class UtxoDiff:
    """``missing = (recs, pay)`` and ``extra = (recs, pay)``; ``changed = (recs_other, pay_other, recs_index,
    pay_index)``, row-aligned; each list in canonical (txid, index) order and at most ``limit`` long. The counts
    ``n_missing``, ``n_extra``, ``n_changed`` are exact; ``compared`` is the entries of O and ``entries`` the live
    entries of I that took part; ``truncated``: some list is shorter than its count."""
    __slots__ = ('missing', 'extra', 'changed', 'n_missing', 'n_extra', 'n_changed', 'compared', 'entries', 'info')

    def __init__(self, missing, extra, changed, n_missing, n_extra, n_changed, compared, entries, info=None):
        self.missing, self.extra, self.changed = _in_order(*missing), _in_order(*extra), _in_order(*changed)
        self.n_missing, self.n_extra, self.n_changed = int(n_missing), int(n_extra), int(n_changed)
        self.compared, self.entries = int(compared), int(entries)
        self.info = info or {}  # what the backend measured (GPU: the table lock's wait and hold in seconds)

    @property
    def truncated(self) -> bool:
        return (len(self.missing[0]) < self.n_missing or len(self.extra[0]) < self.n_extra
                or len(self.changed[0]) < self.n_changed)

    @property
    def equal(self) -> bool:
        return self.n_missing == 0 and self.n_extra == 0 and self.n_changed == 0

    def __repr__(self):
        return (f'UtxoDiff(missing={self.n_missing}, extra={self.n_extra}, changed={self.n_changed}, '
                f'compared={self.compared}, entries={self.entries}, truncated={self.truncated})')


def _in_order(recs, *rest):
    """Row-aligned arrays sorted by the first one's canonical (txid, index) order."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 40)
    order = sort_order(recs)
    return (np.ascontiguousarray(recs[order]),) + tuple(np.ascontiguousarray(x[order]) for x in rest)


def _diff_arrays(recs, pay):
    """Argument check of a diff's record set: (records n x 40, payloads n or None)."""
    recs, pay = _digest_arrays(recs, pay)
    if len(recs):
        words = _record_words(recs)
        if words[:, 8].max() > 255 or words[:, 9].max() > 31:
            raise ValueError('a record has an index above 255 or a tag above 31')
    return recs, pay


def _entries(recs: np.ndarray, pay: Optional[np.ndarray]):
    """(33-byte outpoint, canonical bytes E) of each entry."""
    raw = recs.tobytes()
    praw = pay.tobytes() if pay is not None else None
    out = []
    for i in range(len(recs)):
        r = raw[40 * i:40 * i + 40]
        head, amount, addr = bytes((r[36], 0, 0)), bytes(8), b''
        if praw is not None:
            p = praw[80 * i:80 * i + 80]
            length = int.from_bytes(p[8:12], 'little')
            if length in (33, 64):
                head, amount, addr = bytes((r[36], p[12] & 1, length)), p[0:8], p[16:16 + length]
        out.append((r[:33], r[:33] + head + amount + addr))
    return out


def _rows(recs, pay, rows):
    rows = np.asarray(rows, dtype=np.intp)
    return recs[rows], (pay[rows] if pay is not None else np.zeros(len(rows), dtype=PAYLOAD_DTYPE))


def diff_of(recs_a: np.ndarray, pay_a: Optional[np.ndarray], recs_b: np.ndarray, pay_b: Optional[np.ndarray], *,
            tag_mask: Optional[int] = None, limit: Optional[int] = None) -> UtxoDiff:
    """The diff of the set b (the index's side) against the set a (the other side; ``pay=None``: every entry has
    L = 0) from the definition, with dicts over the canonical bytes: what the ``host-py`` backend runs, and the
    reference that ``diff_vectorised`` and the HBM pass are tested against. ``missing`` is in a and not in b,
    ``extra`` in b and not in a. An outpoint that a repeats is reported missing once per occurrence when b lacks
    it and is a ``ValueError`` when b has it.
    With ``tag_mask`` a is first cut to the tags in the mask and an entry of b outside the mask is never extra,
    but still makes its outpoint in a ``changed``. ``limit`` caps each list (the first ones in a's order; for
    ``extra`` in b's)."""
    recs_a, pay_a = _diff_arrays(recs_a, pay_a)
    recs_b, pay_b = _digest_arrays(recs_b, pay_b)
    if tag_mask is not None:
        recs_a, pay_a = _masked(recs_a, pay_a, tag_mask)
    where = {}
    ents_b = _entries(recs_b, pay_b)
    for j, (key, _) in enumerate(ents_b):
        if key in where:
            raise ValueError('the index side holds an outpoint twice')
        where[key] = j
    seen, missing, changed = set(), [], []
    for i, (key, e) in enumerate(_entries(recs_a, pay_a)):
        j = where.get(key)
        if j is None:
            missing.append(i)
            continue
        if j in seen:
            raise ValueError(f'outpoint {key[:32].hex()}:{key[32]} appears more than once and is live in the index')
        seen.add(j)
        if ents_b[j][1] != e:
            changed.append((i, j))
    in_mask = [j for j, tag in enumerate(_record_words(recs_b)[:, 9].tolist())
               if tag_mask is None or (tag < 32 and (tag_mask >> tag) & 1)]
    extra = [j for j in in_mask if j not in seen]
    n = (len(missing), len(extra), len(changed))
    if limit is not None:
        missing, extra, changed = missing[:limit], extra[:limit], changed[:limit]
    return UtxoDiff(_rows(recs_a, pay_a, missing), _rows(recs_b, pay_b, extra),
                    _rows(recs_a, pay_a, [i for i, _ in changed]) + _rows(recs_b, pay_b, [j for _, j in changed]),
                    *n, len(recs_a), len(in_mask))


def _canonical(recs: np.ndarray, pay: Optional[np.ndarray]):
    """E's payload part per entry, vectorised: (tag | flag << 8 | L << 16, amount, addr with the bytes past L
    zeroed)."""
    n = len(recs)
    tag = recs[:, 36].astype(np.uint32)
    if pay is None:
        return tag, np.zeros(n, np.uint64), np.zeros((n, 64), np.uint8)
    length = np.where((pay['len'] == 33) | (pay['len'] == 64), pay['len'], 0).astype(np.uint32)
    flag = np.where(length > 0, pay['flags'] & 1, 0).astype(np.uint32)
    addr = pay['addr'].reshape(n, 64) * (np.arange(64, dtype=np.uint32)[None, :] < length[:, None])
    return tag | (flag << 8) | (length << 16), np.where(length > 0, pay['amount'], 0).astype(np.uint64), addr


def diff_vectorised(recs_a: np.ndarray, pay_a: Optional[np.ndarray], recs_b: np.ndarray, pay_b: Optional[np.ndarray], *,
                    tag_mask: Optional[int] = None, limit: Optional[int] = None) -> UtxoDiff:
    """:func:`diff_of` in numpy, for sets of millions: b is sorted by a 64-bit head of the outpoint (the txid's
    first eight bytes mixed with the index), a's heads are looked up in it and every candidate pair is compared in
    full. Two outpoints of b with one head, or a head that matches under another outpoint, send the whole call to
    :func:`diff_of`, so the answer never depends on the heads. What the native host backend runs."""
    recs_a, pay_a = _diff_arrays(recs_a, pay_a)
    recs_b, pay_b = _digest_arrays(recs_b, pay_b)
    if tag_mask is not None:
        recs_a, pay_a = _masked(recs_a, pay_a, tag_mask)

    def heads(recs):
        w = _record_words(recs)
        return ((w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1]) ^ \
            ((w[:, 8] & np.uint32(0xff)).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    head_b = heads(recs_b)
    order = np.argsort(head_b, kind='stable')
    sorted_b = head_b[order]
    if (sorted_b[1:] == sorted_b[:-1]).any():
        return diff_of(recs_a, pay_a, recs_b, pay_b, tag_mask=tag_mask, limit=limit)
    head_a = heads(recs_a)
    order_a = np.argsort(head_a, kind='stable')  # sorted needles: the search walks sorted_b once, not at random
    at = np.empty(len(head_a), dtype=np.intp)
    at[order_a] = np.minimum(np.searchsorted(sorted_b, head_a[order_a]), max(len(sorted_b) - 1, 0))
    hit = sorted_b[at] == head_a if len(sorted_b) else np.zeros(len(recs_a), bool)
    rows_a = np.flatnonzero(hit)
    rows_b = order[at[rows_a]]
    if (recs_a[rows_a, :33] != recs_b[rows_b, :33]).any():
        return diff_of(recs_a, pay_a, recs_b, pay_b, tag_mask=tag_mask, limit=limit)
    seen = np.zeros(len(recs_b), bool)
    seen[rows_b] = True
    if int(seen.sum()) != len(rows_b):
        raise ValueError(f'{len(rows_b) - int(seen.sum())} record(s) repeat an outpoint that is live in the index')
    head_x, amount_x, addr_x = _canonical(recs_a[rows_a], None if pay_a is None else pay_a[rows_a])
    head_y, amount_y, addr_y = _canonical(recs_b[rows_b], None if pay_b is None else pay_b[rows_b])
    differ = (head_x != head_y) | (amount_x != amount_y) | (addr_x != addr_y).any(axis=1)
    tags_b = _record_words(recs_b)[:, 9]
    counted = np.ones(len(recs_b), bool) if tag_mask is None else \
        np.array([(tag_mask >> t) & 1 for t in range(32)] + [0], dtype=bool)[np.minimum(tags_b, 32)]
    missing, extra = np.flatnonzero(~hit), np.flatnonzero(counted & ~seen)
    changed_a, changed_b = rows_a[differ], rows_b[differ]
    n = (len(missing), len(extra), len(changed_a))
    if limit is not None:
        missing, extra, changed_a, changed_b = missing[:limit], extra[:limit], changed_a[:limit], changed_b[:limit]
    return UtxoDiff(_rows(recs_a, pay_a, missing), _rows(recs_b, pay_b, extra),
                    _rows(recs_a, pay_a, changed_a) + _rows(recs_b, pay_b, changed_b),
                    *n, len(recs_a), int(counted.sum()))


def pack_records(keys: Sequence[Outpoint], tags=None) -> np.ndarray:
    """40-byte records {txid raw 32 B, u32 index, u32 tag} for the native table."""
    n = len(keys)
    rec = np.zeros((n, 40), dtype=np.uint8)
    if n == 0:
        return rec
    raw = b''.join(bytes.fromhex(h) for h, _ in keys)
    rec[:, :32] = np.frombuffer(raw, dtype=np.uint8).reshape(n, 32)
    idx = np.fromiter((int(i) for _, i in keys), dtype=np.uint32, count=n)
    rec[:, 32:36] = idx.view(np.uint8).reshape(n, 4)
    if tags is None:
        t = np.full(n, MISSING, dtype=np.uint32)
    elif isinstance(tags, int):
        t = np.full(n, tags, dtype=np.uint32)
    else:
        t = np.asarray(tags, dtype=np.uint32)
    rec[:, 36:40] = t.view(np.uint8).reshape(n, 4)
    return rec


class _HostBackend:
    def __init__(self):
        self.d: Dict[Outpoint, int] = {}
        self.p: Dict[Outpoint, bytes] = {}  # raw 80-byte payloads
        self.by_addr: Dict[bytes, Dict[Outpoint, None]] = {}  # owner address bytes -> outpoints (K14 on the host)

    def reset(self, keys, tags, payload=None):
        self.d, self.p, self.by_addr = {}, {}, {}
        self.insert(keys, tags, payload)

    def insert(self, keys, tags, payload=None) -> int:
        """Returns the number of outpoints already present (left untouched, like the HBM table)."""
        raw = payload.tobytes() if payload is not None else None
        dups = 0
        for n, ((h, i), t) in enumerate(zip(keys, tags)):
            k = (h, int(i))
            if k in self.d:
                dups += 1
                continue
            self.d[k] = int(t)
            p = self.p[k] = raw[80 * n:80 * n + 80] if raw is not None else bytes(80)
            a = self._addr(p)
            if a:
                self.by_addr.setdefault(a, {})[k] = None
        return dups

    def probe(self, keys) -> np.ndarray:
        return np.array([self.d.get((h, int(i)), MISSING) for h, i in keys], dtype=np.uint8)

    def lookup(self, keys):
        zero = bytes(80)
        tags = np.array([self.d.get((h, int(i)), MISSING) for h, i in keys], dtype=np.uint8)
        pay = np.frombuffer(b''.join(self.p.get((h, int(i)), zero) for h, i in keys), dtype=PAYLOAD_DTYPE)
        return tags, pay

    def erase(self, keys, tag=None) -> np.ndarray:
        out = np.zeros(len(keys), dtype=np.uint8)
        for n, (h, i) in enumerate(keys):
            k = (h, int(i))
            t = self.d.get(k)
            if t is not None and (tag is None or t == tag):
                del self.d[k]
                a = self._addr(self.p.pop(k, None))
                owned = self.by_addr.get(a)
                if owned is not None:
                    owned.pop(k, None)
                    if not owned:
                        del self.by_addr[a]
                out[n] = 1
        return out

    def records(self) -> np.ndarray:
        return pack_records(list(self.d.keys()), list(self.d.values()))

    def address_scan(self, addr: bytes, tag_mask: int, stake_sel: int = STAKE_ANY):
        def stake_ok(k, t):
            if stake_sel == STAKE_ANY:
                return True
            st = t == 0 and bool(int.from_bytes(self.p.get(k, bytes(80))[12:16], 'little') & FLAG_STAKE)
            return st == (stake_sel == STAKE_ONLY)
        hits = [k for k in self.by_addr.get(bytes(addr), ()) if (tag_mask >> self.d[k]) & 1 and stake_ok(k, self.d[k])]
        pay = np.frombuffer(b''.join(self.p[k] for k in hits), dtype=PAYLOAD_DTYPE)
        return pack_records(hits, [self.d[k] for k in hits]), pay

    def address_scan_batch(self, queries):
        """``address_scan`` for each (addr, tag_mask, stake_sel): the owner map answers each directly."""
        return [self.address_scan(a, m, s) for a, m, s in queries]

    @staticmethod
    def _addr(raw: Optional[bytes]) -> bytes:
        if not raw:
            return b''
        n = int.from_bytes(raw[8:12], 'little')
        return raw[16:16 + n]

    def records_payload(self):
        keys = list(self.d.keys())
        pay = np.frombuffer(b''.join(self.p.get(k, bytes(80)) for k in keys), dtype=PAYLOAD_DTYPE)
        return pack_records(keys, [self.d[k] for k in keys]), pay

    def owner_totals(self, top, by_mask, log2_groups=0, tag_bits=32):
        """Every owner's record and the whole-set info, grouped on the host (``owner_totals_of``)."""
        return owner_totals_of(*self.records_payload())

    def state_digest(self, tag_mask, grid_blocks=0):
        """The state digest of the entries with a tag in ``tag_mask``: the reference (``state_digest_of``)."""
        return state_digest_of(*_masked(*self.records_payload(), tag_mask))

    def merkle_snapshot(self, tag_mask, launch_lever=0):
        """The Merkle tree of the entries with a tag in ``tag_mask``: the reference (``_ReferenceTree``)."""
        return MerkleSnapshot(tree=_ReferenceTree(entries_of(*_masked(*self.records_payload(), tag_mask))))

    def diff(self, recs, pay, tag_mask, limit, chunk_records=0):
        """The index against the record set: the reference (``diff_of``) on a dump."""
        return diff_of(recs, pay, *self.records_payload(), tag_mask=tag_mask, limit=limit)

    def __len__(self):
        return len(self.d)


class _NativeHostBackend:
    """The host table in C++ (csrc/utxo_host.cpp ``HostUtxo``): the HBM table's record contract — keys
    (txid, index & 0xff), tag-filtered erase, zero payload when absent, an owner-address index for K14 — as
    one call per batch of packed records, so the CPU block path never walks its outpoints in Python."""

    def __init__(self):
        from ..ops.native import lib
        self.L = lib()
        self.t = self.L.HostUtxo()

    def reset(self, keys, tags, payload=None):
        self.t.clear()
        return self.insert(keys, tags, payload)

    def insert(self, keys, tags, payload=None) -> int:
        if not len(keys):
            return 0
        return self.insert_records(pack_records(keys, list(tags)), payload)

    def insert_records(self, recs: np.ndarray, payload=None) -> int:
        if not len(recs):
            return 0
        pay = None if payload is None else np.ascontiguousarray(payload).view(np.uint8)
        return int(self.t.insert(np.ascontiguousarray(recs), pay))

    def lookup_records(self, recs: np.ndarray):
        tags, pay = self.t.lookup(np.ascontiguousarray(recs))
        return tags, pay.view(PAYLOAD_DTYPE)

    def lookup(self, keys):
        if not len(keys):
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=PAYLOAD_DTYPE)
        return self.lookup_records(pack_records(keys))

    def probe_records(self, recs: np.ndarray) -> np.ndarray:
        return self.t.probe(np.ascontiguousarray(recs))

    def probe(self, keys) -> np.ndarray:
        if not len(keys):
            return np.zeros(0, dtype=np.uint8)
        return self.probe_records(pack_records(keys))

    def erase_records(self, recs: np.ndarray) -> np.ndarray:
        if not len(recs):
            return np.zeros(0, dtype=np.uint8)
        return self.t.erase(np.ascontiguousarray(recs))

    def erase(self, keys, tag=None) -> np.ndarray:
        if not len(keys):
            return np.zeros(0, dtype=np.uint8)
        return self.erase_records(pack_records(keys, MISSING if tag is None else tag))

    def records(self) -> np.ndarray:
        return self.t.dump(False)[0].reshape(-1, 40)

    def records_payload(self):
        raw, pay = self.t.dump(True)
        return raw.reshape(-1, 40), pay.view(PAYLOAD_DTYPE)

    def address_scan(self, addr: bytes, tag_mask: int, stake_sel: int = STAKE_ANY):
        raw, pay = self.t.address_scan(bytes(addr), tag_mask, stake_sel)
        return raw.reshape(-1, 40), pay.view(PAYLOAD_DTYPE)

    def address_scan_batch(self, queries):
        """``address_scan`` for each (addr, tag_mask, stake_sel): the owner map answers each directly."""
        return [self.address_scan(a, m, s) for a, m, s in queries]

    def owner_totals(self, top, by_mask, log2_groups=0, tag_bits=32):
        """Every owner's record and the whole-set info, grouped on the host (``owner_totals_of``)."""
        return owner_totals_of(*self.records_payload())

    def state_digest(self, tag_mask, grid_blocks=0):
        """The state digest of the entries with a tag in ``tag_mask``: a dump, then the native host routine
        (``utxo_records_digest_host``) on the host pool."""
        recs, pay = _masked(*self.records_payload(), tag_mask)
        return StateDigest(*self.L.utxo_records_digest_host(recs, pay.view(np.uint8), DIGEST_HOST_THREADS))

    def merkle_snapshot(self, tag_mask, launch_lever=0):
        """The Merkle tree of the entries with a tag in ``tag_mask``: a dump, then the native host routine
        (``utxo_merkle_build_records_host``) on the host pool."""
        recs, pay = _masked(*self.records_payload(), tag_mask)
        return MerkleSnapshot(self.L, self.L.utxo_merkle_build_records_host(recs, pay.view(np.uint8),
                                                                              DIGEST_HOST_THREADS))

    def diff(self, recs, pay, tag_mask, limit, chunk_records=0):
        """The index against the record set: a dump, then the join in numpy (``diff_vectorised``)."""
        return diff_vectorised(recs, pay, *self.records_payload(), tag_mask=tag_mask, limit=limit)

    def __len__(self):
        return len(self.t)


class _GpuBackend:
    """HBM table; past 50 % load it is rebuilt on the device (``utxo_rehash``), grown when needed."""

    def __init__(self, log2_cap: int = 20):
        from ..ops.native import require_gpu
        self.L = require_gpu()
        self.log2 = log2_cap
        self.h = self.L.utxo_create(log2_cap)
        self.count = 0
        self.tombs = 0
        self.pending = None  # (inserts, erases) of an async block apply not yet booked

    def __del__(self):
        try:
            self.L.utxo_destroy(self.h)
        except Exception:
            pass

    def apply_async(self, ins: Sequence[Tuple[np.ndarray, Optional[np.ndarray]]], dels: np.ndarray) -> int:
        """One committed block's inserts (groups of records + payloads) then erases, queued on the node
        stream without waiting (csrc/utxo_table.hip utxo_apply_async); every later pass on the table runs
        behind them. The counters are booked by :meth:`complete` (the caller's next access). Returns the
        previous apply's duplicates."""
        dups = self.complete()
        n_ins = sum(len(r) for r, _ in ins)
        self._ensure(n_ins)
        groups = [(np.ascontiguousarray(r), None if p is None else np.ascontiguousarray(p).view(np.uint8))
                  for r, p in ins]
        self.L.utxo_apply_async(self.h, groups, np.ascontiguousarray(dels))
        self.pending = (n_ins, len(dels))
        return dups

    def complete(self) -> int:
        """Book the pending async apply's counters (waits for it): returns its duplicates."""
        if self.pending is None:
            return 0
        n_ins, _ = self.pending
        self.pending = None
        _, failed, dups, erased = self.L.utxo_apply_wait(self.h)
        if failed:
            raise RuntimeError(f'UTXO table insert failed for {failed} entries')
        self.count += n_ins - dups - erased
        self.tombs += erased
        return dups

    def _ensure(self, extra: int):
        """Past 50 % load (live entries + tombstones + the coming inserts) the table is rebuilt on the device
        (``utxo_rehash``): at the same size when dropping the tombstones is enough, else grown. The set never
        leaves HBM (the dump + host re-insert this replaced moved it over PCIe twice, a ~50 ms stall per
        rebuild on a 5 M-outpoint set, every ~30 blocks of 2 MB)."""
        need = self.count + self.tombs + extra
        if need * 2 <= (1 << self.log2):
            return
        log2 = self.log2
        # headroom: after the rebuild the live set and the coming inserts fill at most a third of the table,
        # so tombstones have room to accumulate before the next one
        while (self.count + extra) * 3 > (1 << log2):
            log2 += 1
        moved, failed = self.L.utxo_rehash(self.h, log2)
        if failed or moved != self.count:
            raise RuntimeError(f'UTXO table rehash moved {moved} of {self.count} entries ({failed} found no slot)')
        self.log2, self.tombs = log2, 0

    def reset(self, keys, tags, payload=None):
        self.L.utxo_destroy(self.h)
        self.log2 = int(np.ceil(np.log2(max(2 * len(keys), 1 << 20))))
        self.h = self.L.utxo_create(self.log2)
        self.count = self.tombs = 0
        self.insert(keys, tags, payload)

    def insert(self, keys, tags, payload=None):
        if not len(keys):
            return 0
        return self.insert_records(pack_records(keys, list(tags)), payload)

    def insert_records(self, recs: np.ndarray, payload=None):
        if not len(recs):
            return
        self._ensure(len(recs))
        pay = None if payload is None else np.ascontiguousarray(payload).view(np.uint8)
        failed, dups = self.L.utxo_insert(self.h, np.ascontiguousarray(recs), pay)
        if failed:
            raise RuntimeError(f'UTXO table insert failed for {failed} entries')
        self.count += len(recs) - dups
        return dups

    def lookup_records(self, recs: np.ndarray):
        tags, pay = self.L.utxo_lookup(self.h, np.ascontiguousarray(recs))
        return np.frombuffer(tags, dtype=np.uint8), np.frombuffer(pay, dtype=PAYLOAD_DTYPE)

    def lookup(self, keys):
        if not len(keys):
            return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=PAYLOAD_DTYPE)
        return self.lookup_records(pack_records(keys))

    def probe(self, keys) -> np.ndarray:
        if not len(keys):
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer(self.L.utxo_probe(self.h, pack_records(keys)), dtype=np.uint8)

    def probe_records(self, recs: np.ndarray) -> np.ndarray:
        return np.frombuffer(self.L.utxo_probe(self.h, recs), dtype=np.uint8)

    def erase(self, keys, tag=None) -> np.ndarray:
        if not len(keys):
            return np.zeros(0, dtype=np.uint8)
        out = np.frombuffer(self.L.utxo_erase(self.h, pack_records(keys, MISSING if tag is None else tag)),
                            dtype=np.uint8)
        k = int(out.sum())
        self.count -= k
        self.tombs += k
        return out

    def records(self) -> np.ndarray:
        return np.frombuffer(self.L.utxo_dump(self.h), dtype=np.uint8).reshape(-1, 40)

    def address_scan(self, addr: bytes, tag_mask: int, stake_sel: int = STAKE_ANY):
        raw, pay, _total = self.L.utxo_address_scan(self.h, addr, tag_mask, stake_sel)
        return np.frombuffer(raw, dtype=np.uint8).reshape(-1, 40), np.frombuffer(pay, dtype=PAYLOAD_DTYPE)

    def address_scan_batch(self, queries):
        """``address_scan`` for each (addr, tag_mask, stake_sel), all answered by ONE pass over the HBM table
        (``utxo_address_scan_batch``: the queries are a device-resident table sorted by fingerprint)."""
        n = len(queries)
        if not n:
            return []
        addrs = np.zeros((n, 64), dtype=np.uint8)
        lens = np.zeros(n, dtype=np.uint32)
        for k, (a, _, _) in enumerate(queries):
            if len(a) > 64:
                raise ValueError('address is at most 64 bytes')
            addrs[k, :len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
            lens[k] = len(a)
        masks = np.array([m for _, m, _ in queries], dtype=np.uint32)
        sels = np.array([s for _, _, s in queries], dtype=np.uint32)
        qidx, raw, pay, _totals = self.L.utxo_address_scan_batch(self.h, addrs, lens, masks, sels)
        recs = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 40)
        pay = np.frombuffer(pay, dtype=PAYLOAD_DTYPE)
        order = np.argsort(qidx, kind='stable')
        cuts = np.searchsorted(qidx[order], np.arange(n + 1))
        return [(recs[order[cuts[k]:cuts[k + 1]]], pay[order[cuts[k]:cuts[k + 1]]]) for k in range(n)]

    def owner_totals(self, top, by_mask, log2_groups=0, tag_bits=32):
        """Holders report from ONE pass over the HBM table (``utxo_owner_totals``: a hash aggregation by owner
        key into a scratch group table, then a compaction; with ``top`` below the owner count a radix sort of
        the metrics and a threshold compaction, which hands back every boundary tie). The group table has the
        smallest power of two >= 2 x the booked live count slots, at least 16: distinct owners cannot exceed
        the live entries, so it never fills on a consistent index."""
        if not log2_groups:
            log2_groups = min(31, (max(16, 2 * self.count) - 1).bit_length())
        raw, owners, outputs, skipped, totals = self.L.utxo_owner_totals(
            self.h, -1 if top is None else int(top), by_mask, log2_groups, tag_bits)
        info = {'owners': int(owners), 'outputs': int(outputs), 'skipped': int(skipped),
                'totals': np.asarray(totals, dtype=np.uint64)}
        return np.frombuffer(raw, dtype=OWNER_DTYPE), info

    def state_digest(self, tag_mask, grid_blocks=0):
        """The state digest of the live entries with a tag in ``tag_mask`` from ONE pass over the HBM table
        (``utxo_state_digest``: live slots queued per wave, 1 + 64 SHA-256 compressions per entry, the lanes
        summed across each wave in registers); 8 stripes of lane sums (33 KB) come back. ``grid_blocks``: test lever."""
        return StateDigest(*self.L.utxo_state_digest(self.h, tag_mask, grid_blocks))

    def merkle_snapshot(self, tag_mask, launch_lever=0):
        """The Merkle tree of the live entries with a tag in ``tag_mask``, built in HBM (``utxo_merkle_build``: one
        collection of the table under one hold of its lock, K12's radix sort with the tag as one more column, one
        lane per leaf, one launch per level); 32 bytes come back. ``launch_lever``: test lever."""
        return MerkleSnapshot(self.L, self.L.utxo_merkle_build(self.h, tag_mask, launch_lever))

    def diff(self, recs, pay, tag_mask, limit, chunk_records=0):
        """The index against the record set (tags in ``tag_mask`` only) from ONE pass over the HBM table
        (``utxo_diff``: the records go up in chunks and probe the table, each hit is compared in place and marks
        its slot in a bitmap, then a sweep over the slots compacts the live ones nobody marked): one status byte
        per record and at most ``limit`` extras come back. The index side of the changed entries is one
        ``utxo_lookup`` of those records."""
        status, xr, xp, extra, repeated, live, wait, hold = self.L.utxo_diff(
            self.h, recs, None if pay is None else pay.view(np.uint8), tag_mask, limit, chunk_records)
        if repeated:
            raise ValueError(f'{repeated} record(s) repeat an outpoint that is live in the index')
        miss, chg = np.flatnonzero(status == 1), np.flatnonzero(status == 2)
        n_missing, n_changed = len(miss), len(chg)
        other = _rows(recs, pay, chg[:limit])
        mine = np.array(other[0])
        tags, mine_pay = self.lookup_records(mine) if len(mine) else (np.zeros(0, np.uint8), np.zeros(0, PAYLOAD_DTYPE))
        mine[:, 36] = tags
        return UtxoDiff(_rows(recs, pay, miss[:limit]),
                        (np.frombuffer(xr, dtype=np.uint8).reshape(-1, 40), np.frombuffer(xp, dtype=PAYLOAD_DTYPE)),
                        other + (mine, mine_pay), n_missing, extra, n_changed, len(recs), live,
                        {'lock_wait_seconds': wait, 'lock_hold_seconds': hold})

    def records_payload(self):
        raw, pay = self.L.utxo_dump_payload(self.h)
        return np.frombuffer(raw, dtype=np.uint8).reshape(-1, 40), np.frombuffer(pay, dtype=PAYLOAD_DTYPE)

    def __len__(self):
        return self.count


def _host_backend(name: str):
    """``host``: the C++ table when the extension is built, else the dict; ``host-py``: the dict."""
    if name != 'host-py':
        try:
            from ..ops.native import lib
            if hasattr(lib(), 'HostUtxo'):
                return _NativeHostBackend()
        except Exception:
            pass
    return _HostBackend()


def default_backend() -> str:
    env = os.environ.get('UPOW_UTXO_BACKEND')
    if env:
        return env
    from ..ops.native import gpu_available
    try:
        return 'gpu' if gpu_available() else 'host'
    except Exception:
        return 'host'


# UPOW_UTXO_ASYNC=0: the block path's index update as synchronous insert + erase calls (A/B)
ASYNC_APPLY = os.environ.get('UPOW_UTXO_ASYNC', '1') != '0'


def _locked(fn):
    """Run under the index lock, after any deferred writes (:meth:`UtxoIndex.defer_block`) reached the
    backend: every read and every direct write sees the index as the committed blocks left it."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with self.lock:
            if self._pend_ins or self._pend_del:
                self._apply_pending()
            if self._gpu and self.be.pending is not None:
                self._dups(self.be.complete())
            return fn(self, *args, **kwargs)
    return wrapper


class UtxoIndex:
    def __init__(self, backend: Optional[str] = None):
        import threading
        self.lock = threading.RLock()
        self.backend_name = backend or default_backend()
        self.be = _GpuBackend() if self.backend_name == 'gpu' else _host_backend(self.backend_name)
        self._gpu = isinstance(self.be, _GpuBackend)
        self._rec = self._gpu or isinstance(self.be, _NativeHostBackend)  # packed records in, no Python walk
        self.duplicates = 0  # inserts of an outpoint that was already live (skipped; a ledger bug if ever > 0)
        # deferred writes of committed blocks (a sync page's blocks, ledger/pagesync.py): applied as ONE insert
        # launch and ONE erase launch before anything else touches the index
        self._pend_ins: List[Tuple[np.ndarray, Optional[np.ndarray]]] = []
        self._pend_del: List[np.ndarray] = []
        self.deferred_flushes = 0

    def defer_block(self, ins: Sequence[Tuple[np.ndarray, Optional[np.ndarray]]], spent: np.ndarray):
        """Record one committed block's index writes (created-output records + payloads, spent records)
        without touching the backend. Applying every deferred insert, then every deferred erase, equals
        applying the blocks in order: an outpoint is created at most once, spent at most once, and only
        after its creation (the page plan checks both before a block takes this path)."""
        with self.lock:
            for recs, pay in ins:
                if len(recs):
                    self._pend_ins.append((recs, pay))
            if len(spent):
                self._pend_del.append(spent)

    def settle(self):
        """Apply the deferred writes now and book any async apply (no-op when there is neither)."""
        with self.lock:
            if self._pend_ins or self._pend_del:
                self._apply_pending()
            if self._gpu and self.be.pending is not None:
                self._dups(self.be.complete())

    def apply_block(self, ins: Sequence[Tuple[np.ndarray, Optional[np.ndarray]]], spent: np.ndarray):
        """The block path's index update after the commit point: the block's created outputs (records +
        payloads, one or more groups) in, then its spent records out. GPU backend: one H2D copy, one insert
        and one erase launch queued on the node stream, no wait (``_GpuBackend.apply_async``): the next
        block's lookup is queued behind them, and its counters are booked at the next access."""
        with self.lock:
            if self._pend_ins or self._pend_del:
                self._apply_pending()
            self._apply(list(ins), [spent] if len(spent) else [])

    def _apply(self, ins, dels):
        ins = [(r, p) for r, p in ins if len(r)]
        if ins and any(p is None for _, p in ins):  # payloads for every group or for none
            ins = [(r, None) for r, _ in ins]
        spent = np.ascontiguousarray(np.concatenate(dels)) if len(dels) > 1 else \
            (np.ascontiguousarray(dels[0]) if dels else np.zeros((0, 40), np.uint8))
        if self._gpu and ASYNC_APPLY:
            if ins or len(spent):
                self._dups(self.be.apply_async(ins, spent))
            return
        recs = np.ascontiguousarray(np.concatenate([r for r, _ in ins])) if ins else np.zeros((0, 40), np.uint8)
        pay = None if (not ins or ins[0][1] is None) else np.ascontiguousarray(np.concatenate([p for _, p in ins]))
        if len(recs):
            self._insert_records(recs, pay)
        if len(spent):
            self._erase_records(spent)

    def _apply_pending(self):
        ins, dels = self._pend_ins, self._pend_del
        self._pend_ins, self._pend_del = [], []
        self.deferred_flushes += 1
        self._apply(ins, dels)

    def _dups(self, n: int):
        if n:
            self.duplicates += int(n)
            import logging
            logging.getLogger('upow').error(f'UTXO index: {n} insert(s) of an already live outpoint skipped')

    @_locked
    def reset(self, keys: Sequence[Outpoint], tags: Sequence[int], payload: Optional[np.ndarray] = None):
        self.be.reset(list(keys), list(tags), payload)

    @_locked
    def insert(self, keys: Sequence[Outpoint], tag, payload: Optional[np.ndarray] = None):
        keys = list(keys)
        tags = [tag] * len(keys) if isinstance(tag, int) else list(tag)
        self._dups(self.be.insert(keys, tags, payload))

    @_locked
    def insert_records(self, recs: np.ndarray, payload: Optional[np.ndarray] = None):
        """Insert packed 40-byte key records (tags inside) — the block fast path's form."""
        self._insert_records(recs, payload)

    def _insert_records(self, recs: np.ndarray, payload: Optional[np.ndarray] = None):
        if self._rec:
            self._dups(self.be.insert_records(recs, payload))
            return
        idx = recs[:, 32:36].copy().view(np.uint32).ravel()
        tags = recs[:, 36:40].copy().view(np.uint32).ravel()
        keys = [(bytes(recs[n, :32]).hex(), int(idx[n])) for n in range(len(recs))]
        self._dups(self.be.insert(keys, [int(t) for t in tags], payload))

    @_locked
    def lookup(self, keys: Sequence[Outpoint]):
        """(tags uint8[n], payload PAYLOAD_DTYPE[n]) for each outpoint (tag 0xff / len 0 when absent)."""
        return self.be.lookup(list(keys))

    @_locked
    def lookup_records(self, recs: np.ndarray):
        if self._rec:
            return self.be.lookup_records(recs)
        idx = recs[:, 32:36].copy().view(np.uint32).ravel()
        return self.be.lookup([(bytes(recs[n, :32]).hex(), int(idx[n])) for n in range(len(recs))])

    @_locked
    def erase_records(self, recs: np.ndarray) -> np.ndarray:
        return self._erase_records(recs)

    def _erase_records(self, recs: np.ndarray) -> np.ndarray:
        if isinstance(self.be, _GpuBackend):
            if not len(recs):
                return np.zeros(0, dtype=np.uint8)
            out = np.frombuffer(self.be.L.utxo_erase(self.be.h, np.ascontiguousarray(recs)), dtype=np.uint8)
            k = int(out.sum())
            self.be.count -= k
            self.be.tombs += k
            return out
        if self._rec:
            return self.be.erase_records(recs)
        if not len(recs):
            return np.zeros(0, dtype=np.uint8)
        idx = recs[:, 32:36].copy().view(np.uint32).ravel()
        tags = recs[:, 36:40].copy().view(np.uint32).ravel()
        keys = [(bytes(recs[n, :32]).hex(), int(idx[n])) for n in range(len(recs))]
        out = np.zeros(len(recs), dtype=np.uint8)
        for tag in np.unique(tags).tolist():  # per-record tag filter, like the HBM erase kernel
            sel = np.nonzero(tags == tag)[0]
            out[sel] = self.be.erase([keys[k] for k in sel.tolist()], None if tag == MISSING else int(tag))
        return out

    @_locked
    def probe(self, keys: Sequence[Outpoint]) -> np.ndarray:
        return self.be.probe(list(keys))

    @_locked
    def erase(self, keys: Sequence[Outpoint], tag: Optional[int] = None) -> np.ndarray:
        return self.be.erase(list(keys), tag)

    @_locked
    def filter(self, outputs: Iterable[Outpoint], tag: int) -> List[Outpoint]:
        """Outpoints of ``outputs`` present in table ``tag`` (unique, in first-seen order)."""
        uniq = list(dict.fromkeys((h, int(i)) for h, i in outputs))
        if not uniq:
            return []
        t = self.probe(uniq)
        return [k for k, v in zip(uniq, t) if v == tag]

    @_locked
    def records(self) -> np.ndarray:
        """All live entries as 40-byte records, in canonical (txid, index) order."""
        return sort_records(np.ascontiguousarray(self.be.records()))

    @_locked
    def address_outputs(self, addr: bytes, tags: Iterable[int] = (0,), stake_sel: int = STAKE_ANY):
        """K14 (reference ``database.py:909-937,1138-1205``): the live outpoints whose payload address is
        ``addr`` (raw 33/64 bytes, prefix normalised as stored) in the given tables, as (records, payloads)
        in canonical (txid, index) order, plus their amount sum in smallest units. GPU backend: one pass
        over the HBM table instead of an index walk (``utxo_address_scan``: a batch of one query through the
        batch kernel of csrc/utxo_scan.hip)."""
        mask = 0
        for t in tags:
            mask |= 1 << int(t)
        recs, pay = self.be.address_scan(bytes(addr), mask, stake_sel)
        order = sort_order(np.ascontiguousarray(recs))
        recs, pay = np.ascontiguousarray(recs[order]), np.ascontiguousarray(pay[order])
        return recs, pay, int(pay['amount'].sum()) if len(pay) else 0

    @_locked
    def address_outputs_many(self, queries: Sequence[Tuple[bytes, Iterable[int], int]]):
        """:meth:`address_outputs` for each ``(addr, tags, stake_sel)`` of ``queries``: one
        ``(records, payloads, amount_sum)`` per query, in query order, each what the single call returns.
        GPU backend: every query is answered by the same pass over the HBM table
        (``utxo_address_scan_batch``), where single calls, each a batch of one, make one pass each."""
        qs = []
        for addr, tags, stake_sel in queries:
            mask = 0
            for t in tags:
                mask |= 1 << int(t)
            qs.append((bytes(addr), mask, int(stake_sel)))
        out = []
        for recs, pay in self.be.address_scan_batch(qs):
            order = sort_order(np.ascontiguousarray(recs))
            recs, pay = np.ascontiguousarray(recs[order]), np.ascontiguousarray(pay[order])
            out.append((recs, pay, int(pay['amount'].sum()) if len(pay) else 0))
        return out

    @_locked
    def owner_totals(self, top: Optional[int] = None, by: Sequence[int] = (0, 7), *, log2_groups: int = 0,
                     tag_bits: int = 32):
        """Holders report: ``(owners, info)`` over the whole index. An owner is a public key, so the 33-byte
        and the 64-byte form of an address are one owner (OWNER_DTYPE / OWNER_COLUMNS above). ``top=None``:
        every owner, ascending by key; ``top=N``: at most N owners in (metric descending, key ascending)
        order, the metric being the sum of the ``by`` columns modulo 2^64. ``info`` is always over the whole
        set: ``owners`` distinct owners, ``outputs`` entries grouped, ``skipped`` live entries without a
        33/64-byte payload or with a tag above 6, ``totals`` u64[8]. GPU backend: one pass over the HBM table
        (``_GpuBackend.owner_totals``); the keyword arguments size and weaken its scratch group table (test
        levers, ignored by the host backends)."""
        mask = _by_mask(top, by)
        owners, info = self.be.owner_totals(top, mask, log2_groups, tag_bits)
        return _owners_in_order(owners, top, mask), info

    @_locked
    def state_digest(self, tags: Optional[Iterable[int]] = None, *, grid_blocks: int = 0) -> StateDigest:
        """The state digest (:class:`StateDigest`, LtHash16/1024) of every live entry of the tables ``tags``
        (``None``: all seven) with its payload: one value that a wrong amount, address, stake flag, tag or
        index changes, and that adds up: after a block it is the digest before + ``records_digest`` of the
        created entries - ``records_digest`` of the spent ones. GPU backend: one pass over the HBM table
        behind any queued block apply (``grid_blocks`` sizes its launch: a test lever); host backends: a dump
        and 65 compressions per entry on the CPU."""
        return self.be.state_digest(_tag_mask(tags), grid_blocks)

    @_locked
    def merkle_snapshot(self, tags: Optional[Iterable[int]] = None, *, launch_lever: int = 0) -> MerkleSnapshot:
        """A :class:`MerkleSnapshot` of every live entry of the tables ``tags`` (default: all seven): the RFC 6962
        tree over the entries in (txid, index, tag) order, whose ``(root, count)`` commits to the set and whose
        :meth:`MerkleSnapshot.prove` shows for any outpoint that it is live with this amount and owner, or that it
        is not (verified by ledger/utxo_proof.py). The snapshot owns its memory, about 176 bytes per entry (HBM on the
        GPU backend, built there by csrc/utxo_merkle.hip), and keeps answering for this state after the index moves
        on. ``launch_lever`` is a test lever."""
        return self.be.merkle_snapshot(_tag_mask(tags), launch_lever)

    @_locked
    def diff_records(self, recs: np.ndarray, pay: Optional[np.ndarray] = None, tags: Optional[Iterable[int]] = None,
                     *, limit: int = DIFF_LIMIT, chunk_records: int = 0) -> UtxoDiff:
        """WHERE the index differs from the record set O = (``recs``, ``pay``; ``pay=None``: no payloads): a
        :class:`UtxoDiff` of the missing, extra and changed entries, an entry being what :meth:`state_digest`
        hashes, so for O without repeated outpoints the diff is empty exactly when ``state_digest(tags)`` equals
        ``records_digest`` of O. ``tags`` as in :meth:`state_digest`: O is first cut to the records whose tag is
        in them and the index to its live entries whose tag is; an outpoint of O that is live under a tag outside
        them is ``changed``, not missing plus extra. ``limit`` caps each list, the counts stay exact: a truncated
        ``missing`` or ``changed`` list holds the first ``limit`` such records in O's order, a truncated ``extra``
        list some ``limit`` of them. ``ValueError``: a record with an index above 255 or a tag above 31, payloads
        that are not one per record, or an outpoint that O holds more than once and that is live in the index
        (one that is not live is reported missing once per occurrence). GPU backend: one pass over the HBM table
        behind any queued block apply (``_GpuBackend.diff``; ``chunk_records`` sizes its uploads: a test lever,
        ignored by the host backends); host backends: a dump, then ``diff_vectorised`` (``host``) or the
        reference ``diff_of`` (``host-py``)."""
        if not isinstance(limit, (int, np.integer)) or limit < 0:
            raise ValueError('limit is a count >= 0')
        if not isinstance(chunk_records, (int, np.integer)) or not 0 <= chunk_records < 1 << 32:
            raise ValueError('chunk_records is a count >= 0 (0: the default)')
        mask = _tag_mask(tags)
        recs, pay = _masked(*_diff_arrays(recs, pay), mask)
        return self.be.diff(recs, pay, mask, min(int(limit), 0xffffffff), int(chunk_records))

    @_locked
    def records_payload(self, sort: bool = True):
        """(records, payloads) of every live entry, in canonical (txid, index) order (``sort=False``: in the
        backend's own order, for a caller that sorts later off the ledger's critical path)."""
        recs, pay = self.be.records_payload()
        if not sort:
            return recs, pay
        order = sort_order(np.ascontiguousarray(recs))
        return np.ascontiguousarray(recs[order]), np.ascontiguousarray(pay[order])

    @_locked
    def reset_records(self, recs: np.ndarray, payload: Optional[np.ndarray] = None):
        """Replace the whole index with packed records (snapshot restore: one H2D copy + insert launch)."""
        recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 40)
        if self._rec:
            self.be.reset([], [])
            if len(recs):
                self.be.insert_records(recs, payload)
        else:
            idx = recs[:, 32:36].copy().view(np.uint32).ravel()
            tags = recs[:, 36:40].copy().view(np.uint32).ravel()
            keys = [(bytes(recs[n, :32]).hex(), int(idx[n])) for n in range(len(recs))]
            self.be.reset(keys, [int(t) for t in tags], payload)

    @_locked
    def block_inputs(self, in_keys: np.ndarray, in_start: np.ndarray, out_amount: np.ndarray,
                     out_start: np.ndarray, want_tag: int = 0):
        """One pass over a block's inputs: K7 lookup (tag + payload), K10 duplicate detection and K11
        per-tx fees. GPU backend: one H2D/D2H round trip and three kernels (csrc/utxo_block.hip).

        Returns (tags u8[n_in], payload[n_in], dup_of u32[n_in] (1 + earlier duplicate, else 0),
        fee i64[n_tx], missing u32[n_tx], n_dup)."""
        in_start = np.ascontiguousarray(in_start, dtype=np.int32)
        out_start = np.ascontiguousarray(out_start, dtype=np.int32)
        out_amount = np.ascontiguousarray(out_amount, dtype=np.uint64)
        if isinstance(self.be, _GpuBackend):
            # the segment arrays are read in place; the outputs are arrays the pass filled from its pinned staging
            t, p, d, f, m, nd = self.be.L.utxo_block_inputs(self.be.h, np.ascontiguousarray(in_keys), in_start,
                                                            out_amount, out_start, want_tag)
            return t, p.view(PAYLOAD_DTYPE), d, f, m, int(nd)
        tags, pay = self.lookup_records(in_keys)
        n_in = len(in_keys)
        dup_of = np.zeros(n_in, dtype=np.uint32)
        if n_in > 1:  # K10: (txid, index byte) seen earlier in the block -> 1 + the first occurrence
            k = np.ascontiguousarray(in_keys[:, :33]).view(np.dtype((np.void, 33))).ravel()
            _, first, inv = np.unique(k, return_index=True, return_inverse=True)
            first = first[inv.ravel()]
            later = first != np.arange(n_in)
            dup_of[later] = first[later] + 1
        bad = ((tags != want_tag) | (pay['len'] == 0)).astype(np.int64)
        amt = pay['amount'].astype(np.int64)

        def seg_sum(x, starts):  # per-tx sums over contiguous segments (empty segments -> 0)
            cs = np.concatenate([[0], np.cumsum(x, dtype=np.int64)])
            return cs[starts[1:]] - cs[starts[:-1]]
        ins = seg_sum(amt, in_start)
        outs = seg_sum(out_amount.astype(np.int64), out_start)
        miss = seg_sum(bad, in_start).astype(np.uint32)
        return tags, pay, dup_of, ins - outs, miss, int((dup_of > 0).sum())

    @_locked
    def set_message(self, tag: int = 0) -> np.ndarray:
        """K12's message: (txid || index byte) of every outpoint of table ``tag`` sorted by (txid, index).
        GPU backend: compaction + stable LSD radix sort + message gather on the device."""
        if isinstance(self.be, _GpuBackend):
            return self.be.L.utxo_set_message(self.be.h, tag)
        recs = self.records()
        recs = recs[recs[:, 36:40].copy().view(np.uint32).ravel() == tag]
        # records() is in canonical (txid, index) order; index byte = the reference's bytes([i])
        return np.ascontiguousarray(np.concatenate([recs[:, :32], recs[:, 32:33]], axis=1)).ravel()

    def k12_snapshot(self, tag: int = 0):
        """K12 at this block, computed later: returns a callable giving the hex digest (the same value
        :meth:`set_hash` gives now). GPU backend: the snapshot is one compaction launch on the node stream;
        the callable (meant for a worker thread) sorts, gathers and hashes on the aux stream."""
        with self.lock:
            if self._pend_ins or self._pend_del:
                self._apply_pending()
            if isinstance(self.be, _GpuBackend):  # queued behind any async apply on the node stream
                L, sid = self.be.L, self.be.L.utxo_k12_snapshot(self.be.h, tag)
                return lambda: L.utxo_k12_digest(sid)[0].hex()
        msg = self.set_message(tag)
        import hashlib
        return lambda: hashlib.sha256(msg).hexdigest()

    def set_hash(self, tag: int = 0) -> str:
        """K12 from the index: SHA-256 over :meth:`set_message` — byte-identical to
        ``Database.get_unspent_outputs_hash`` (reference database.py:827-830). The sequential hash tail
        runs outside the index lock (hashlib releases the GIL), so block application is not held up by it."""
        import hashlib
        return hashlib.sha256(self.set_message(tag)).hexdigest()

    def __len__(self):
        self.settle()
        return len(self.be)


def sort_order(recs: np.ndarray) -> np.ndarray:
    """Permutation sorting packed records by (txid bytes, index): SQL ``ORDER BY tx_hash, index``."""
    if len(recs) < 2:
        return np.arange(len(recs))
    be = recs[:, :32].copy().view('>u8')  # 4 big-endian words compare like the hex strings
    idx = recs[:, 32:36].copy().view(np.uint32).ravel()
    return np.lexsort((idx, be[:, 3], be[:, 2], be[:, 1], be[:, 0]))


def sort_records(recs: np.ndarray) -> np.ndarray:
    return recs[sort_order(recs)] if len(recs) >= 2 else recs
