"""PoW kernel variant 11 (csrc/pow_search.hip, pow_a_fill / pow_search_fill_kernel): variant 10 with one scalar or
sequencer instruction in front of every slow instruction. What differs from variant 10 in arithmetic: K[i] comes
through PowSchedRegs::kx, rounds 12 and 13 are pinned with their constant operands, the nonce word and W17 are not
materialised (a11, e11, W24, round 17's sum and the first adds of W26 and W33 take a scalar sum plus lane << p), and
the range-form kernel folds range_base into round 63's constant.

The reference throughout is hashlib over the same nonce words.
"""
import functools
import hashlib
import random
import struct

import pytest

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search

VARIANT = 11
M32 = 0xffffffff
RANGE_DIFFICULTIES = ['1.0', '1.3', '2.0', '6.3', '7.9', '8.0', '9.5']  # test_pow_split.py's range-form list


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


def test_variant_11_is_exposed():
    assert lib().pow_variant_count() >= 12


@pytest.mark.parametrize('seed', [71, 72, 73])
def test_h0_at_edge_words(seed):
    """pow_job_h0_variant splits a word as lane << 26 | U: the word just below and at the wrap of the low 26 bits
    of each of the five sums, and the ends of the lane and word ranges."""
    job = _job(seed)
    m = (1 << 26) - 1
    words = [0, 1, m, 1 << 26, 1 << 31, M32]
    for c in _sum_consts(job):
        at = (0 - c) & m  # the low 26 bits of c + word wrap to zero here
        words += [(at - 1) & M32, at, ((5 << 26) + at - 1) & M32, ((5 << 26) + at) & M32]
    for word in words:
        assert lib().pow_job_h0_variant(job.header, word, VARIANT) == _h0(job, word), (seed, hex(word))
        assert lib().pow_job_h0_variant(job.header, word, 0) == _h0(job, word), (seed, hex(word))


@pytest.mark.parametrize('p', [0, 8, 26])
def test_host_wave_loop_straddles_flip(p):
    """40 iterations with cached.next (the first flip of one of the five sums) inside the window, all 64 lanes."""
    job = _job(71)
    rng = random.Random(300 + p)
    m = (1 << p) - 1
    n = 1 << p
    vb = rng.getrandbits(32)
    flips = sorted({(n - ((c + vb) & m)) & m for c in _sum_consts(job)} - {0})
    iters = 40
    if p == 0:
        u_first = 0  # no low bits: the loop walks on word by word and every iteration recomputes
    else:
        flip = flips[len(flips) // 2]
        u_first = min(max(0, flip - 20), n - iters)
        assert u_first <= flip < u_first + iters
    for variant in (VARIANT, 0):
        got = lib().pow_split_wave(job.header, vb, p, u_first, iters, variant)
        assert got.shape == (iters, 64)
        for it in range(iters):
            for lane in range(64):
                word = (vb + u_first + it + (lane << p)) & M32
                assert int(got[it, lane]) == _h0(job, word), (variant, hex(vb), p, u_first + it, lane)


def test_wave_loop_rejects_other_variants():
    with pytest.raises(Exception):
        lib().pow_split_wave(_job(71).header, 0, 8, 0, 1, 9)


def _mask_form(job, h0):
    return ((h0 ^ job.tword) & job.tmask) == 0 and ((h0 >> job.frac_shift) & 0xf) < job.frac_limit


@pytest.mark.parametrize('difficulty', RANGE_DIFFICULTIES)
def test_folded_range_constant(difficulty):
    """Round 63 adds K[63] + range_base, so the kernel compares its result with range_width alone: the same
    verdict as the mask form at both ends of the range."""
    L = lib()
    job = _job(61, difficulty)
    c = L.pow_split_consts(*job.native_args())
    assert c['range_ok']
    width = c['range_width']
    for h0 in (job.tword - 1, job.tword, job.tword + width - 1, job.tword + width):
        h0 &= M32
        assert L.pow_range_hit_folded(*job.native_args(), h0) == _mask_form(job, h0), (difficulty, hex(h0))
        assert L.pow_range_hit_folded(*job.native_args(), h0) == L.pow_range_hit(*job.native_args(), h0)
    assert L.pow_range_hit_folded(*job.native_args(), job.tword)


# ---- GPU ----

@functools.lru_cache(maxsize=None)
def _host_exact(seed, difficulty, start, count):
    """Valid nonces of [start, start + count) (nonce words, wrapping at 2^32) by hashlib, sorted."""
    job = _job(seed, difficulty)
    out = []
    for k in range(count):
        word = (start + k) & M32
        if job.target.check_hex(hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).hexdigest()):
            out.append(job.word_to_nonce(word))
    return tuple(sorted(out))


def _same_on_10_and_11(seed, difficulty, start, count, **kw):
    want = _host_exact(seed, difficulty, start, count)
    for variant in (10, 11):
        g = search(_job(seed, difficulty), start, count, device='gpu', variant=variant, **kw)
        assert g.searched == count
        assert tuple(sorted(g.nonces)) == want, (variant, difficulty, start, count, kw)
    return want


@pytest.mark.gpu
def test_gpu_piece_remainder_and_host_words(gpu):
    """2^14 + 2^8 + 5 words from an odd start at difficulty 2.5: one p = 8 piece, one block on variant 9's kernel,
    five words on the host."""
    want = _same_on_10_and_11(71, '2.5', 987_655, (1 << 14) + (1 << 8) + 5)
    assert len(want) > 10


@pytest.mark.gpu
def test_gpu_low_bits_wrap_inside_a_wave_run(gpu):
    """2^15 words (p = 9) placed so that the low nine bits of ca + v wrap in the middle of the piece; one block,
    eight iterations per dispatch: many dispatches, and a recompute inside a wave's run."""
    job = _job(71, '2.0')
    ca = _sum_consts(job)[2]
    start = ((0xabc << 9) | ((0 - ca - 300) & 0x1ff)) & M32  # ca + start + 300 has its low nine bits zero
    assert (ca + start + 300) & 0x1ff == 0
    want = _same_on_10_and_11(71, '2.0', start, 1 << 15, grid_blocks=1, chunk_iters=8)
    assert len(want) > 60


@pytest.mark.gpu
def test_gpu_piece_crosses_2_32(gpu):
    want = _same_on_10_and_11(71, '2.0', (1 << 32) - (1 << 14) - 3, 1 << 15, grid_blocks=2, chunk_iters=7)
    assert len(want) > 60
