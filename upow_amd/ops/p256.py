"""P-256 front end: single sign/verify (host C++) and batched verify/decompress/keygen/sign/vanity search (gfx950 kernels).

Batch record layout (160 B, little-endian like the wire format): ``qx | qy | r | s | e`` where ``e``
is the SHA-256 digest of the signed message (big-endian, as hashed). Status codes: 1 valid,
0 invalid, 2 public key not on the curve, 3 r or s outside [1, n] — fastecdsa raises for 2 and 3
(reference transaction_input.py:100-109), which :func:`verify` reproduces with ``EcdsaError``.
"""
from __future__ import annotations

import hashlib
import os
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..utils import coalesce
from ..utils.cpus import cpu_budget
from ..utils import p256 as oracle
from ..utils.p256 import EcdsaError, Point
from .native import gpu_available, lib

VALID, INVALID, BAD_KEY, BAD_RANGE = 1, 0, 2, 3
# below this many signatures (or keys) a batch runs on host threads. The quad kernel's latency floor is
# ~1.3 ms whatever the batch (one signature's double-scalar chain on four lanes); 16 host threads pass it
# near 100 signatures on an MI355X box (a 200-tx sync block: 2.5 ms host vs 1.4 ms GPU, docs/PERF.md)
GPU_MIN_BATCH = int(os.environ.get('UPOW_P256_GPU_MIN_BATCH', '64'))


def _msg(m: Union[str, bytes]) -> bytes:
    return m.encode() if isinstance(m, str) else bytes(m)


def public_key(d: int) -> Point:
    out = lib().p256_pubkey(int(d).to_bytes(32, 'big'))
    if out is None:
        raise ValueError('private key out of range')
    return Point(int.from_bytes(out[:32], 'little'), int.from_bytes(out[32:], 'little'), check=False)


def sign(msg: Union[str, bytes], d: int) -> Tuple[int, int]:
    res = lib().p256_sign(int(d).to_bytes(32, 'big'), hashlib.sha256(_msg(msg)).digest())
    if res is None:
        raise ValueError('signing failed')
    return int.from_bytes(res[0], 'little'), int.from_bytes(res[1], 'little')


def record(q: Point, sig: Tuple[int, int], digest: bytes) -> bytes:
    r, s = sig
    if not (0 <= r < 1 << 256 and 0 <= s < 1 << 256):
        raise EcdsaError('signature component out of range')
    return (q.x.to_bytes(32, 'little') + q.y.to_bytes(32, 'little') + r.to_bytes(32, 'little')
            + s.to_bytes(32, 'little') + digest)


def verify_records(records: Union[bytes, bytearray, np.ndarray], device: Optional[str] = None,
                   threads: int = 0) -> np.ndarray:
    """Batched verify of packed 160-byte records -> uint8 status array."""
    buf = records if isinstance(records, np.ndarray) else np.frombuffer(bytes(records), dtype=np.uint8)
    n = buf.size // 160
    if device is None:
        device = 'gpu' if (gpu_available() and n >= GPU_MIN_BATCH) else 'cpu'
    st = lib().p256_verify(buf, device == 'gpu', threads or max(1, min(cpu_budget(), 16)))
    return np.frombuffer(st, dtype=np.uint8)


def verify(sig: Tuple[int, int], msg: Union[str, bytes], q: Point) -> bool:
    """fastecdsa.ecdsa.verify(sig, msg, Q, P256) contract, on the host C++ core."""
    r, s = sig
    if r >= 1 << 256 or s >= 1 << 256 or r < 0 or s < 0:
        raise EcdsaError('Invalid Signature: r/s out of range')
    st = verify_records(record(q, sig, hashlib.sha256(_msg(msg)).digest()), device='cpu', threads=1)[0]
    if st == BAD_KEY:
        raise EcdsaError('Invalid public key, point is not on curve P256')
    if st == BAD_RANGE:
        raise EcdsaError('Invalid Signature: r or s is not a positive integer smaller than the curve order')
    return bool(st == VALID)


# ---------------------------------------------------------------------------------------------- batched signing
# below this many items a batch of keys or signatures runs on host threads; UPOW_P256_SIGN_GPU_MIN (read per
# call) overrides it. Measured by scripts/p256_sign_throughput.py on an MI355X (docs/PERF.md "P-256 signing"):
# the smallest measured n at which the GPU beats 16 host threads end to end by >= 20 % for both functions is
# the smallest n measured, 256 (signing 1.66x, keys 1.24x; 5.2x / 4.1x at 1,024)
SIGN_GPU_MIN = 256


def _keys_be(keys: Sequence[int]) -> bytes:
    for i, d in enumerate(keys):
        if not 1 <= int(d) < oracle.N:
            raise ValueError(f'private key {i} out of range')
    return b''.join(int(d).to_bytes(32, 'big') for d in keys)


def _sign_on_gpu(n: int, device: Optional[str]) -> bool:
    if device is None:
        return gpu_available() and n >= int(os.environ.get('UPOW_P256_SIGN_GPU_MIN', SIGN_GPU_MIN))
    if device not in ('gpu', 'cpu'):
        raise ValueError("device must be 'gpu', 'cpu' or None")
    return device == 'gpu'


def _rows64(out: bytes, n: int, what: str) -> np.ndarray:
    rows = np.frombuffer(out, dtype=np.uint8).reshape(n, 64)
    bad = np.flatnonzero(~rows.any(axis=1))
    if bad.size:  # keys were range-checked: a failed candidate loop (or a device that returned nothing)
        raise ValueError(f'{what} failed for item {int(bad[0])}')
    return rows


def public_keys(keys: Sequence[int], device: Optional[str] = None) -> np.ndarray:
    """Public keys of n private keys -> uint8 array (n, 64), x | y little-endian. Runs the batched signer's
    core (csrc/p256_sign.h; not constant-time: bulk work on a trusted machine) on the GPU or on host threads.
    ``ValueError`` names the first key outside [1, n-1]."""
    n = len(keys)
    if n == 0:
        return np.zeros((0, 64), dtype=np.uint8)
    out = lib().p256_pubkey_many(_keys_be(keys), _sign_on_gpu(n, device), max(1, min(cpu_budget(), 16)))
    return _rows64(out, n, 'key derivation')


def sign_digests(keys: Sequence[int], digests: Sequence[bytes], device: Optional[str] = None) -> np.ndarray:
    """RFC 6979 signatures of n SHA-256 digests, key i over digest i -> uint8 array (n, 64), r | s
    little-endian (no low-s normalisation, like :func:`sign`). Same core and caveat as :func:`public_keys`."""
    n = len(keys)
    if len(digests) != n:
        raise ValueError('need one digest per key')
    if n == 0:
        return np.zeros((0, 64), dtype=np.uint8)
    dig = b''.join(bytes(h) for h in digests)
    if len(dig) != 32 * n:
        raise ValueError('digests must be 32 bytes each')
    out = lib().p256_sign_many(_keys_be(keys), dig, _sign_on_gpu(n, device), max(1, min(cpu_budget(), 16)))
    return _rows64(out, n, 'signing')


def sign_records(keys: Sequence[int], digests: Sequence[bytes], device: Optional[str] = None) -> np.ndarray:
    """Ready-made verify records ``qx | qy | r | s | e`` -> uint8 array (n, 160) for :func:`verify_records`."""
    n = len(keys)
    recs = np.empty((n, 160), dtype=np.uint8)
    recs[:, 64:128] = sign_digests(keys, digests, device)
    recs[:, :64] = public_keys(keys, device)
    if n:
        recs[:, 128:] = np.frombuffer(b''.join(bytes(h) for h in digests), dtype=np.uint8).reshape(n, 32)
    return recs


# ---------------------------------------------------------------------------------------------- vanity search
def vanity_on_gpu(device: Optional[str] = None) -> bool:
    """Where a vanity search runs, whatever its size: the GPU when there is one, unless ``device`` says otherwise
    (``find`` sizes its calls by the same answer)."""
    if device is None:
        return gpu_available()
    if device not in ('gpu', 'cpu'):
        raise ValueError("device must be 'gpu', 'cpu' or None")
    return device == 'gpu'


def vanity_search(base: int, count: int, ranges: Sequence[Tuple[int, int]], max_hits: int = 4096,
                  device: Optional[str] = None) -> Tuple[int, np.ndarray]:
    """Which of the private keys ``base + i``, ``i`` in [0, count), have an address whose 33 bytes, read as a
    big-endian integer, lie in one of ``ranges`` (half-open ``(lo, hi)``, sorted and disjoint: wallet/vanity.py
    ``prefix_ranges``) -> ``(number of hits, their i ascending as uint64)``; any ``max_hits`` of them when there
    are more, the number still exact. K16 (csrc/p256_vanity.h; not constant-time, ``base`` is a secret: bulk work
    on a trusted machine) on the GPU or the same core on host threads (:func:`vanity_on_gpu`; ``device`` as in
    :func:`public_keys`).
    ``ValueError`` unless 1 <= base and base + count <= n, and for malformed ranges."""
    if not 0 <= int(count) < 1 << 63:
        raise ValueError('count must be in [0, 2**63)')
    try:
        base_be = int(base).to_bytes(32, 'big')
        packed = b''.join(int(lo).to_bytes(33, 'big') + int(hi).to_bytes(33, 'big') for lo, hi in ranges)
    except OverflowError:
        raise ValueError('base or a range bound does not fit its field') from None
    total, idx = lib().p256_vanity_search(base_be, int(count), packed, int(max_hits), vanity_on_gpu(device),
                                          max(1, min(cpu_budget(), 16)))
    return int(total), np.frombuffer(idx, dtype='<u8')


# ---------------------------------------------------------------------------------------------- admission
# reference: every /push_tx verifies its signatures one at a time on the node's event loop
# (transaction_input.py:100-109 via fastecdsa). Inside an admission context (utils/coalesce.py) the
# checks of concurrent requests are verified together on an executor thread: on the GPU when the batch is
# large enough to beat a round trip, else on host threads. The event loop never runs an ECDSA verify.
ADMISSION_GPU_MIN = int(os.environ.get('UPOW_ADMISSION_GPU_MIN', '32'))


def _verify_batch(recs: List[bytes]) -> bytes:
    n = len(recs)
    gpu = gpu_available() and n >= ADMISSION_GPU_MIN
    return lib().p256_verify(np.frombuffer(b''.join(recs), dtype=np.uint8), gpu, max(1, min(n, 8)))


async def verify_async(sig: Tuple[int, int], msg: Union[str, bytes], q: Point) -> bool:
    """:func:`verify` (same result, same exceptions); inside an admission context it goes through the
    event loop's signature coalescer instead of running on the loop."""
    if not coalesce.ADMISSION.get():
        return verify(sig, msg, q)
    r, s = sig
    if r >= 1 << 256 or s >= 1 << 256 or r < 0 or s < 0:
        raise EcdsaError('Invalid Signature: r/s out of range')
    st = await coalesce.coalescer('p256-admit', _verify_batch).submit(record(q, sig, hashlib.sha256(_msg(msg)).digest()))
    if st == BAD_KEY:
        raise EcdsaError('Invalid public key, point is not on curve P256')
    if st == BAD_RANGE:
        raise EcdsaError('Invalid Signature: r or s is not a positive integer smaller than the curve order')
    return st == VALID


def decompress(addresses33: Sequence[bytes], device: Optional[str] = None):
    """Batch decompression of 33-byte addresses -> (list of (x, y) or None)."""
    n = len(addresses33)
    if n == 0:
        return []
    buf = b''.join(bytes(a) for a in addresses33)
    if device is None:
        device = 'gpu' if (gpu_available() and n >= GPU_MIN_BATCH) else 'cpu'
    out, ok = lib().p256_decompress(buf, device == 'gpu')
    res = []
    for i in range(n):
        if ok[i]:
            res.append((int.from_bytes(out[64 * i:64 * i + 32], 'little'),
                        int.from_bytes(out[64 * i + 32:64 * i + 64], 'little')))
        else:
            res.append(None)
    return res


__all__ = ['public_key', 'sign', 'verify', 'verify_async', 'verify_records', 'decompress', 'record', 'EcdsaError', 'oracle',
           'public_keys', 'sign_digests', 'sign_records', 'SIGN_GPU_MIN', 'vanity_search', 'vanity_on_gpu']
