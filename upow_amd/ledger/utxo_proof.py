"""UTXO proofs, the verifier's side: check one outpoint against a 32-byte root and a count.

The tree (csrc/native.h "UTXO proofs", docs/WIRE_FORMAT.md): the index's entries
``E = txid[32] | u8(index) | u8(tag) | u8(flags & 1) | u8(L) | u64le(amount) | addr[0:L]`` (L in 0, 33, 64) in
ascending order of E's first 34 bytes, as the leaves of an RFC 6962 / RFC 9162 Merkle tree:
``leaf = SHA-256(0x00 | E)``, ``node = SHA-256(0x01 | left | right)``, split at the largest power of two below n.
The commitment is ``(root, count)``.

Pure Python on hashlib: no native extension and no numpy, so a wallet without a node can use it. What a proof
shows: the outpoint is in the committed set with exactly this amount, owner and table, or it is not in it. What it
does not show: that the root is the chain's (compare it between nodes), or that a list of outpoints is complete
(the tree is ordered by outpoint, not by owner).
"""
from __future__ import annotations

import hashlib
from typing import List, Optional, Sequence, Tuple

TABLE_BY_TAG = {0: 'unspent_outputs', 1: 'inode_registration_output', 2: 'validator_registration_output',
                3: 'validators_voting_power', 4: 'delegates_voting_power', 5: 'validators_ballot', 6: 'inodes_ballot'}
EMPTY_ROOT = hashlib.sha256(b'').digest()
_B58 = '123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz'


class ProofError(ValueError):
    """A proof that does not check against the commitment."""


def leaf_hash(entry: bytes) -> bytes:
    return hashlib.sha256(b'\x00' + entry).digest()


def node_hash(left: bytes, right: bytes) -> bytes:
    return hashlib.sha256(b'\x01' + left + right).digest()


def entry_key(entry: bytes) -> bytes:
    """What the leaves are ordered by: txid, index, tag."""
    return bytes(entry[:34])


def query_key(tx_hash: str, index: int) -> bytes:
    """The outpoint's 33 bytes: every leaf of the outpoint has them as the head of its key."""
    raw = bytes.fromhex(tx_hash)
    if len(raw) != 32 or not 0 <= int(index) <= 255:
        raise ValueError('an outpoint is a 32-byte transaction hash and an index in 0..255')
    return raw + bytes((int(index),))


def _b58(data: bytes) -> str:
    n, out = int.from_bytes(data, 'big'), ''
    while n:
        n, r = divmod(n, 58)
        out = _B58[r] + out
    return '1' * (len(data) - len(data.lstrip(b'\0'))) + out


def decode_entry(entry: bytes) -> dict:
    """The fields of E; ``ProofError`` for bytes that are no entry (an impossible length, a length byte that does
    not match, flag bits, or an amount or flag on an entry without owner)."""
    entry = bytes(entry)
    if len(entry) not in (44, 77, 108):
        raise ProofError(f'an entry has 44, 77 or 108 bytes, not {len(entry)}')
    length, flags, amount = entry[35], entry[34], int.from_bytes(entry[36:44], 'little')
    if length != len(entry) - 44 or flags > 1 or (length == 0 and (flags or amount)):
        raise ProofError('malformed entry')
    addr = entry[44:]
    if length == 64:
        address = addr.hex()
    elif length == 33:  # the canonical string: the specifier is 43, else 42
        address = _b58(bytes((43 if addr[0] == 43 else 42,)) + addr[1:])
    else:
        address = None
    return {'tx_hash': entry[:32].hex(), 'index': entry[32], 'tag': entry[33],
            'table': TABLE_BY_TAG.get(entry[33]), 'amount': amount, 'address': address,
            'address_bytes': addr.hex(), 'is_stake': bool(flags)}


def root_from_path(count: int, position: int, entry: bytes, path: Sequence[bytes]) -> bytes:
    """RFC 9162 2.1.3.2: the root that the audit path of leaf ``position`` in a tree of ``count`` leaves leads to;
    ``ProofError`` when the path does not have the tree's shape."""
    if not 0 <= position < count:
        raise ProofError(f'position {position} is not below the count {count}')
    fn, sn = position, count - 1
    r = leaf_hash(bytes(entry))
    for p in path:
        if len(p) != 32:
            raise ProofError('a path element has 32 bytes')
        if sn == 0:
            raise ProofError('the path is longer than the tree is high')
        if fn & 1 or fn == sn:
            r = node_hash(bytes(p), r)
            if not fn & 1:
                while fn and not fn & 1:
                    fn >>= 1
                    sn >>= 1
        else:
            r = node_hash(r, bytes(p))
        fn >>= 1
        sn >>= 1
    if sn != 0:
        raise ProofError('the path is shorter than the tree is high')
    return r


def verify_leaf(root: bytes, count: int, position: int, entry_bytes: bytes, path: Sequence[bytes]) -> bool:
    """Is ``entry_bytes`` leaf ``position`` of the tree ``(root, count)``?"""
    try:
        return root_from_path(int(count), int(position), entry_bytes, path) == bytes(root)
    except ProofError:
        return False


class LeafProof:
    """One leaf: its position, its entry bytes E and its audit path, bottom up."""
    __slots__ = ('position', 'entry', 'path')

    def __init__(self, position: int, entry: bytes, path: Sequence[bytes]):
        self.position, self.entry, self.path = int(position), bytes(entry), [bytes(p) for p in path]

    def to_json(self) -> dict:
        d = {'position': self.position, 'entry': self.entry.hex(), 'path': [p.hex() for p in self.path]}
        try:  # for readers only: the verifier decodes from `entry`
            d['decoded'] = decode_entry(self.entry)
        except ProofError:
            pass
        return d

    @classmethod
    def from_json(cls, d: dict) -> 'LeafProof':
        try:
            return cls(int(d['position']), bytes.fromhex(d['entry']), [bytes.fromhex(p) for p in d['path']])
        except (KeyError, TypeError, ValueError) as e:
            raise ProofError(f'unreadable leaf proof: {e}') from None

    def __eq__(self, other):
        return isinstance(other, LeafProof) and (self.position, self.entry, self.path) == \
            (other.position, other.entry, other.path)

    def __repr__(self):
        return f'LeafProof({self.position}, {self.entry.hex()}, {len(self.path)} hashes)'


class OutpointProof:
    """The answer for one queried outpoint: ``present`` with the leaves that have it (normally one), or absent with
    its neighbours in the order (the predecessor, then the successor; one of them at either end of the set, none in
    the empty set)."""
    __slots__ = ('tx_hash', 'index', 'present', 'leaves')

    def __init__(self, tx_hash: str, index: int, present: bool, leaves: Sequence[LeafProof]):
        self.tx_hash, self.index, self.present, self.leaves = str(tx_hash), int(index), bool(present), list(leaves)

    def to_json(self) -> dict:
        return {'tx_hash': self.tx_hash, 'index': self.index, 'present': self.present,
                'leaves': [x.to_json() for x in self.leaves]}

    @classmethod
    def from_json(cls, d: dict) -> 'OutpointProof':
        try:
            return cls(d['tx_hash'], int(d['index']), bool(d['present']), [LeafProof.from_json(x) for x in d['leaves']])
        except (KeyError, TypeError, ValueError) as e:
            if isinstance(e, ProofError):
                raise
            raise ProofError(f'unreadable proof: {e}') from None

    def __eq__(self, other):
        return isinstance(other, OutpointProof) and (self.tx_hash, self.index, self.present, self.leaves) == \
            (other.tx_hash, other.index, other.present, other.leaves)

    def __repr__(self):
        return f'OutpointProof({self.tx_hash}:{self.index}, present={self.present}, {self.leaves})'


def _as_proof(proof) -> OutpointProof:
    return proof if isinstance(proof, OutpointProof) else OutpointProof.from_json(proof)


def verify_outpoint_all(root: bytes, count: int, tx_hash: str, index: int, proof) -> List[dict]:
    """Check ``proof`` (an :class:`OutpointProof` or its JSON form) for the outpoint against ``(root, count)``:
    the decoded entries of the leaves that hold it, ``[]`` when it is proven absent, ``ProofError`` otherwise."""
    proof = _as_proof(proof)
    root, count = bytes(root), int(count)
    if len(root) != 32 or count < 0:
        raise ProofError('a commitment is a 32-byte root and a count')
    try:
        want = query_key(tx_hash, index)
    except ValueError as e:
        raise ProofError(str(e)) from None
    if (proof.tx_hash.lower(), proof.index) != (tx_hash.lower(), int(index)):
        raise ProofError('the proof answers another outpoint')
    leaves = proof.leaves
    for leaf in leaves:
        decode_entry(leaf.entry)
        if root_from_path(count, leaf.position, leaf.entry, leaf.path) != root:
            raise ProofError(f'the path of leaf {leaf.position} does not lead to the root')
    for a, b in zip(leaves, leaves[1:]):  # consecutive leaves in ascending order, whatever they prove
        if b.position != a.position + 1 or not entry_key(a.entry) < entry_key(b.entry):
            raise ProofError('the leaves are not neighbours in ascending order')
    if proof.present:
        if not leaves or any(entry_key(x.entry)[:33] != want for x in leaves):
            raise ProofError('a leaf of a "present" proof holds another outpoint')
        return [decode_entry(x.entry) for x in leaves]
    # absent: nothing fits between the neighbours, and the query sorts strictly between them
    if count == 0:
        if leaves or root != EMPTY_ROOT:
            raise ProofError('the empty set has no leaves and the root of the empty string')
        return []
    if not 1 <= len(leaves) <= 2:
        raise ProofError('an absence proof in a non-empty set names one or two neighbours')
    below = [x for x in leaves if entry_key(x.entry)[:33] < want]
    above = [x for x in leaves if entry_key(x.entry)[:33] > want]
    if len(below) + len(above) != len(leaves) or len(below) > 1 or len(above) > 1:
        raise ProofError('the neighbours do not bracket the outpoint')
    if not below and above[0].position != 0:
        raise ProofError('the predecessor is missing')
    if not above and below[0].position != count - 1:
        raise ProofError('the successor is missing')
    return []


def verify_outpoint(root: bytes, count: int, tx_hash: str, index: int, proof) -> Optional[dict]:
    """The decoded entry (``table``/``tag``, ``amount``, ``address``, ``is_stake``) of the outpoint when ``proof``
    shows it in the set ``(root, count)``, ``None`` when it shows that it is not; :class:`ProofError` on anything
    that does not check: a bad path, neighbours that are not adjacent or do not bracket the outpoint, a position at
    or beyond ``count``, a missing neighbour in a non-empty set, an entry of impossible length. An outpoint held
    under several tags (an unhealthy index) gives the first entry; :func:`verify_outpoint_all` gives all."""
    found = verify_outpoint_all(root, count, tx_hash, index, proof)
    return found[0] if found else None


def split_outpoint(text: str) -> Tuple[str, int]:
    """``TXHASH:INDEX`` as the tools take it."""
    tx_hash, _, index = text.partition(':')
    query_key(tx_hash, int(index))
    return tx_hash.lower(), int(index)
