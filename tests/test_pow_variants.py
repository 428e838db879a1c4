"""Every PoW kernel variant the build exposes against the host exact search, and the host-precomputed
job constants of the kernel (csrc/pow_search.hip make_pow_job / pow_h0_pre) against hashlib."""
import functools
import hashlib
import random

import pytest

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search
from upow_amd.utils import p256
from upow_amd.utils.codec import AddressFormat, point_to_string

# (v1 header, difficulty): the 108-byte header on the fractional-nibble path and on a whole nibble count,
# the 138-byte header on the fractional path
CONFIGS = [(False, '2.5'), (False, '3'), (True, '2.5')]
SPAN = 3 * (1 << 20) + 777
# (start, count, grid_blocks, chunk_iters). The explicit 3-block grid gives several dispatches, a short final
# dispatch, a sub-grid block launch and the < 256-nonce host remainder; 5 and 4 iterations per dispatch are an
# odd and an even count for kernels that hash more than one nonce per lane.
RANGES = [
    (0, SPAN, 3, 5),
    (0, SPAN, 3, 4),
    (0, SPAN, 0, 0),                    # the default grid and dispatch size
    ((1 << 32) - (1 << 20), 1 << 20, 0, 0),  # the top of the nonce space
    (0, 100, 0, 0),                     # host-only path
    (0, 256, 0, 0),                     # exactly one block
    (0, 257, 0, 0),
]


@functools.lru_cache(maxsize=None)
def _job(v1, difficulty):
    rng = random.Random(23)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    key = p256.get_public_key(rng.randrange(1, p256.N))
    addr = point_to_string(key, AddressFormat.FULL_HEX if v1 else AddressFormat.COMPRESSED)
    pre = header_prefix(prev, addr, hashlib.sha256(rng.randbytes(8)).hexdigest(), 1_700_000_023, difficulty)
    return PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))


@functools.lru_cache(maxsize=None)
def _host(v1, difficulty, start, count):
    """The host exact search over a range, computed once and shared by all variants."""
    r = search(_job(v1, difficulty), start, count, device='cpu', threads=8)
    assert r.searched == count
    return r.candidates, frozenset(r.nonces)


def _variants():
    return range(lib().pow_variant_count())


@pytest.mark.gpu
@pytest.mark.parametrize('v1,difficulty', CONFIGS)
@pytest.mark.parametrize('variant', _variants())
def test_variant_matches_host_search(gpu, variant, v1, difficulty):
    job = _job(v1, difficulty)
    for start, count, grid_blocks, chunk_iters in RANGES:
        hits, nonces = _host(v1, difficulty, start, count)
        g = search(job, start, count, device='gpu', grid_blocks=grid_blocks, chunk_iters=chunk_iters,
                   variant=variant)
        where = (variant, start, count, grid_blocks, chunk_iters)
        assert g.searched == count, where
        assert g.candidates == hits, where
        assert len(g.nonces) == len(set(g.nonces)) and set(g.nonces) == nonces, where
    assert len(_host(v1, difficulty, 0, SPAN)[1]) > 100  # the comparison is not of empty sets


@pytest.mark.gpu
@pytest.mark.parametrize('v1,difficulty', CONFIGS)
@pytest.mark.parametrize('variant', _variants())
def test_variant_capacity_overflow(gpu, variant, v1, difficulty):
    """cap = 4 on a range with more hits: the count is still exact, 4 words are stored, each a true hit."""
    job = _job(v1, difficulty)
    count = 1 << 20  # whole blocks only: no host remainder appends past the cap
    hits, _ = _host(v1, difficulty, 0, count)
    assert hits > 4
    searched, total, words = gpu.pow_search_gpu(*job.native_args(), 0, count, 3, 5, 4, variant)
    assert searched == count and total == hits
    assert len(words) == 4 and len(set(words)) == 4
    for w in words:
        assert 0 <= w < count and job.exact_check(job.word_to_nonce(w))


@pytest.mark.parametrize('v1', [False, True])
def test_precomputed_job_constants_reproduce_h0(native, v1):
    """make_pow_job's nonce-independent constants, run through the kernel's own round code on the host, give
    the H0 of hashlib.sha256 over the full header."""
    job = _job(v1, '2.5')
    rng = random.Random(5)
    words = [0, 1, 0xff, 0x100, 0x01020304, 0x80000000, 0xffffffff] + [rng.getrandbits(32) for _ in range(25)]
    for w in words:
        digest = hashlib.sha256(job.header_with_nonce(job.word_to_nonce(w))).digest()
        assert native.pow_job_h0(job.header, w) == int.from_bytes(digest[:4], 'big'), hex(w)
