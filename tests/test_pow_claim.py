"""PoW kernel variant 12 (csrc/pow_search.hip, pow_search_claim_kernel): variant 11's loop under a claiming wave
loop. A dispatch covers the range it covered before; which wave runs which values of U is decided at run time, by a
counter that every wave adds `claim` to until the range is used up. What can go wrong is therefore a chunk left out
or run twice, a ragged last chunk, a counter that was not zero, and the wave prologue at a chunk's first U.

The reference is hashlib over the same nonce words for ranges up to 2^18 words and variant 11 on the GPU above
that. The difficulties are 1.0 to 2.5, so every chunk of a range holds hits: a chunk left out shows in the sorted
nonces, a chunk run twice in `candidates`, which counts every hit the kernels reported (the sorted set hides a
double).
"""
import functools
import hashlib
import random
import struct

import pytest

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search

VARIANT = 12
M32 = 0xffffffff


@functools.lru_cache(maxsize=None)
def _job(seed, difficulty='2.0'):
    rng = random.Random(seed)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    pre = header_prefix(prev, 'DgQKikeDqS2Fzue23KuA36L4eJSFh649zA9jJ6zwbzUMp', hashlib.sha256(rng.randbytes(8)).hexdigest(),
                        1_790_000_000 + seed, difficulty)
    job = PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))
    assert len(job.header) == 108
    return job


def _h0(job, word):
    return struct.unpack('>I', hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).digest()[:4])[0]


def _sum_consts(job):
    """The constants in front of the nonce word: v, ce + v, ca + v, kw17 + v, c24 + v."""
    c = lib().pow_split_consts(*job.native_args())
    return [0, c['ce'], c['ca'], c['c17'], c['c24']]


def _mask_form(job, h0):
    return ((h0 ^ job.tword) & job.tmask) == 0 and ((h0 >> job.frac_shift) & 0xf) < job.frac_limit


@functools.lru_cache(maxsize=None)
def _reference(seed, difficulty, start, count):
    """(valid nonces sorted, number of words whose H0 passes the kernel's predicate) of [start, start + count),
    nonce words wrapping at 2^32, by hashlib. Computed once per range and shared."""
    assert count <= (1 << 18) + (1 << 14)
    job = _job(seed, difficulty)
    nonces, candidates = [], 0
    for k in range(count):
        word = (start + k) & M32
        digest = hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).digest()
        if _mask_form(job, struct.unpack('>I', digest[:4])[0]):
            candidates += 1
            if job.target.check_hex(digest.hex()):
                nonces.append(job.word_to_nonce(word))
    return tuple(sorted(nonces)), candidates


def _check(seed, difficulty, start, count, **kw):
    nonces, candidates = _reference(seed, difficulty, start, count)
    g = search(_job(seed, difficulty), start, count, device='gpu', variant=VARIANT, **kw)
    assert tuple(sorted(g.nonces)) == nonces, (difficulty, start, count, kw)
    assert g.searched == count, (difficulty, start, count, kw)
    assert g.candidates == candidates, (difficulty, start, count, kw)
    return nonces


# ---- CPU ----

def test_variant_12_is_exposed():
    assert lib().pow_variant_count() >= 13


@pytest.mark.parametrize('seed', [71, 72, 73])
def test_h0_at_edge_words(seed):
    """Variant 12 computes what variant 11 computes: test_pow_fill.py's edge words, the word just below and at the
    wrap of the low 26 bits of each of the five sums and the ends of the lane and word ranges."""
    job = _job(seed)
    m = (1 << 26) - 1
    words = [0, 1, m, 1 << 26, 1 << 31, M32]
    for c in _sum_consts(job):
        at = (0 - c) & m
        words += [(at - 1) & M32, at, ((5 << 26) + at - 1) & M32, ((5 << 26) + at) & M32]
    for word in words:
        assert lib().pow_job_h0_variant(job.header, word, VARIANT) == _h0(job, word), (seed, hex(word))


def test_host_wave_loop_accepts_variant_12():
    job = _job(71)
    vb, p, u_first, iters = 0x1234abcd, 8, 250, 6
    got = lib().pow_split_wave(job.header, vb, p, u_first, iters, VARIANT)
    assert got.shape == (iters, 64)
    for it in range(iters):
        for lane in (0, 1, 63):
            assert int(got[it, lane]) == _h0(job, (vb + u_first + it + (lane << p)) & M32)


# ---- GPU ----

@pytest.fixture(scope='module')
def resident(gpu):
    return lib().pow_kernel_info(VARIANT)['resident_blocks']


@pytest.mark.gpu
@pytest.mark.parametrize('grid', [1, 2, 'resident'])
@pytest.mark.parametrize('claim', [1, 3, 7, 32, 256, 1000])
def test_gpu_one_small_piece(gpu, resident, claim, grid):
    """One p = 8 piece, 256 values of U: more waves than chunks, one block that takes everything, a claim that does
    not divide the range, a claim as large as the range and one larger."""
    nonces = _check(71, '2.0', 5 << 14, 1 << 14, claim=claim, grid_blocks=resident if grid == 'resident' else grid)
    assert len(nonces) > 30


@pytest.mark.gpu
def test_gpu_dispatch_cut_with_ragged_last_chunk(gpu):
    """p = 10 on two blocks, five iterations per wave per dispatch: a dispatch covers 40 values of U, thirteen
    chunks of three and one of one; the last dispatch of the piece is cut at the piece's end (1024 = 25 * 40 + 24)."""
    nonces = _check(71, '2.0', 9 << 16, 1 << 16, claim=3, grid_blocks=2, chunk_iters=5)
    assert len(nonces) > 150


@pytest.mark.gpu
@pytest.mark.parametrize('start', [987_655, (1 << 32) - (1 << 12)])
def test_gpu_pieces_remainder_host_words_and_wrap(gpu, start):
    """2^16 + 2^14 + 2^8 + 5 words: pieces of p = 10 and p = 8, one block on the unsplit kernel, five words on the
    host; from an odd start, and from 2^12 words below 2^32."""
    count = (1 << 16) + (1 << 14) + (1 << 8) + 5
    nonces = _check(71, '2.5', start, count)
    assert len(nonces) > 60
    _check(71, '2.5', start, count, claim=5, grid_blocks=3)


@pytest.mark.gpu
def test_gpu_many_dispatches_and_reused_buffers(gpu):
    """A p = 8 piece on one block, one iteration per wave per dispatch: 64 dispatches, one more than there are
    counters, so the counters are zeroed again on the way. Then two more searches on the same thread, whose
    counters the searches before them left past their ranges."""
    for _ in range(2):
        _check(71, '2.0', 5 << 14, 1 << 14, claim=1, grid_blocks=1, chunk_iters=1)
    _check(71, '2.0', 5 << 14, 1 << 14, claim=2, grid_blocks=1, chunk_iters=5)
    _check(71, '2.0', 5 << 14, 1 << 14)


@pytest.mark.gpu
@pytest.mark.parametrize('at', [32, 40, 47])
def test_gpu_flip_inside_a_chunk(gpu, at):
    """p = 8, claim = 16 in one dispatch: the chunks start at the multiples of 16. vb is chosen so that the low eight
    bits of one of the five sums wrap (cached.next) at U = `at`: a chunk's first U, where the prologue computes the
    lane constants, its middle and its last, where the loop recomputes them."""
    job = _job(71, '2.0')
    for c in _sum_consts(job):
        start = ((0x2b << 14) | ((0 - c - at) & 0xff)) & M32
        assert (c + start + at) & 0xff == 0
        nonces = _check(71, '2.0', start, 1 << 14, claim=16, grid_blocks=2)
        assert len(nonces) > 30


@pytest.mark.gpu
def test_gpu_cap_smaller_than_hits(gpu):
    job = _job(71, '1.0')
    start, count = 1 << 24, 1 << 14
    nonces, candidates = _reference(71, '1.0', start, count)
    assert candidates > 500
    searched, total, words = gpu.pow_search_gpu(*job.native_args(), start, count, 2, 0, 4, VARIANT, claim=3)
    assert searched == count and total == candidates
    assert len(words) == 4 and len(set(words)) == 4
    for w in words:
        assert job.word_to_nonce(w) in nonces


@pytest.mark.gpu
def test_gpu_workload_predicate_against_variant_11(gpu):
    """Difficulty 6.3 over 2^22 words, the range-form kernel at the workload's own predicate; and difficulty 2.0
    over the same range, where every chunk has hits."""
    for difficulty in ('6.3', '2.0'):
        job = _job(74, difficulty)
        assert lib().pow_split_consts(*job.native_args())['range_ok']
        want = search(job, 3 << 22, 1 << 22, device='gpu', variant=11)
        got = search(job, 3 << 22, 1 << 22, device='gpu', variant=VARIANT)
        assert got.searched == want.searched == 1 << 22
        assert got.candidates == want.candidates and got.nonces == want.nonces
    assert len(want.nonces) > 10000


@pytest.mark.gpu
def test_gpu_mask_form_piece(gpu):
    """The kernel's other instantiation. Difficulty 0.5 has no range form (test_pow_split.py): one p = 8 piece,
    where a 32-bit condition finds nothing, so the candidate count is compared. And a mask that is no prefix, given
    to the native search directly, which has hits in every chunk."""
    job = _job(71, '0.5')
    assert not lib().pow_split_consts(*job.native_args())['range_ok']
    nonces, candidates = _reference(71, '0.5', 5 << 14, 1 << 14)
    g = search(job, 5 << 14, 1 << 14, device='gpu', variant=VARIANT, claim=3)
    assert g.searched == 1 << 14 and g.candidates == candidates and tuple(sorted(g.nonces)) == nonces
    tmask, tword = 0x0f000000, 0x03000000
    assert not lib().pow_split_consts(job.header, tmask, tword, 0, 16)['range_ok']
    start, count = 5 << 14, 1 << 14
    want = sorted(w for w in range(start, start + count) if ((_h0(job, w) ^ tword) & tmask) == 0)
    assert len(want) > 500
    searched, total, words = gpu.pow_search_gpu(job.header, tmask, tword, 0, 16, start, count, 2, 0, 1 << 16, VARIANT,
                                                claim=3)
    assert searched == count and total == len(want) and sorted(words) == want
