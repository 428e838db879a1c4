"""Shared by tests/test_vanity.py (host path) and tests/test_vanity_gpu.py: the oracle (the existing key derivation),
the recorded end-to-end search, and the range-edge cases of the K16 vanity search."""
import numpy as np

from upow_amd.ops.native import lib

LO, HI = 42 << 256, 44 << 256
INFO = lib().p256_vanity_info()
B = INFO['keys_per_lane']

# the end-to-end search: the enumeration below of the 2**16 keys from E2E_BASE on finds 'E5' first at index 638
# (an odd-y address at the very top of the address space, 'E5' ends at 'E56wJq...')
E2E_BASE = 0x5eed << 200
E2E_PREFIX = 'E5'
E2E_COUNT = 1 << 16
E2E_FIRST = 638


def be32(v):
    return int(v).to_bytes(32, 'big')


def pack(ranges):
    return b''.join(lo.to_bytes(33, 'big') + hi.to_bytes(33, 'big') for lo, hi in ranges)


def oracle_rows(base, count):
    """The 33 address bytes of the keys base .. base + count - 1 from the existing derivation (p256_pubkey_many on
    the host pool), laid out as utils/codec.point_to_bytes(..., COMPRESSED) does -> uint8 array (count, 33)."""
    xy = np.frombuffer(lib().p256_pubkey_many(b''.join(be32(base + i) for i in range(count)), False, 8),
                       dtype=np.uint8).reshape(count, 64)
    assert xy.any(axis=1).all()
    rows = np.empty((count, 33), dtype=np.uint8)
    rows[:, 0] = 42 + (xy[:, 32] & 1)  # y is little-endian: its first byte carries the parity
    rows[:, 1:] = xy[:, :32]
    return rows


def oracle_addresses(base, count):
    return [bytes(r) for r in oracle_rows(base, count)]


def search(base, count, ranges, max_hits=4096, gpu=False, **kw):
    total, idx = lib().p256_vanity_search(be32(base), count, pack(ranges), max_hits, gpu, 8, **kw)
    return total, [int(v) for v in np.frombuffer(idx, dtype='<u8')]


EDGE_BASE = 0xabcdef << 128
EDGE_COUNT = 3 * B + 5


def edge_cases(addresses):
    """(ranges, expected indexes) over the walked keys with the given 33-byte addresses."""
    vals = [int.from_bytes(a, 'big') for a in addresses]
    cases = []
    for k in (0, 1, B // 2, B, len(vals) - 1):
        nk = vals[k]
        for lo, hi in [(nk, nk + 1), (nk + 1, nk + 2), (nk - 1, nk)]:
            cases.append(([(lo, hi)], [i for i, v in enumerate(vals) if lo <= v < hi]))
    cases.append(([(LO, 43 << 256)], [i for i, v in enumerate(vals) if v < (43 << 256)]))
    cases.append(([(43 << 256, HI)], [i for i, v in enumerate(vals) if v >= (43 << 256)]))
    cases.append(([(LO, HI)], list(range(len(vals)))))
    # several ranges at once: around three keys, sorted
    picks = sorted(vals[i] for i in (2, B + 1, 2 * B + 3))
    multi = [(v, v + 1) for v in picks]
    cases.append((multi, sorted(i for i, v in enumerate(vals) if v in picks)))
    return cases
