"""PoW kernel variant 10 (csrc/pow_search.hip, pow_a_split / pow_search_split_kernel): the lane index in the top
bits of the nonce word, the wave-uniform low bits on the scalar unit, per-lane constants cached across iterations,
and the hit predicate as one range check.

The reference throughout is hashlib over the same nonce words. A piece of the search is
v = vb + U + (lane << p), U in [0, 2^p); the host wave loop (pow_split_wave) runs the kernel's loop body for 64
lanes with the kernel's cached lane constants, which are recomputed only when a carry out of bit p-1 flips.
"""
import functools
import hashlib
import random
import struct

import pytest

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search

VARIANT = 10
M32 = 0xffffffff


@functools.lru_cache(maxsize=None)
def _job(difficulty='2.0'):
    rng = random.Random(61)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    pre = header_prefix(prev, 'DgQKikeDqS2Fzue23KuA36L4eJSFh649zA9jJ6zwbzUMp', hashlib.sha256(rng.randbytes(8)).hexdigest(),
                        1_790_000_061, difficulty)
    return PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))


def _h0(job, word):
    return struct.unpack('>I', hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).digest()[:4])[0]


@functools.lru_cache(maxsize=None)
def _brute_force(difficulty, start, count):
    """Valid nonces of [start, start + count) (nonce words, wrapping at 2^32) by hashlib."""
    job = _job(difficulty)
    out = []
    for k in range(count):
        word = (start + k) & M32
        if job.target.check_hex(hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).hexdigest()):
            out.append(job.word_to_nonce(word))
    return frozenset(out)


def _consts(job):
    return lib().pow_split_consts(*job.native_args())


def _sum_consts(job):
    """The constants in front of the nonce word: W10 = v, a11 = ca + v, e11 = ce + v, W17 = c17 + v, W24 = c24 + v."""
    c = _consts(job)
    return [0, c['ca'], c['ce'], c['c17'], c['c24']]


def _bases(job, p, rng):
    """vb values: the ends of the word range, random ones, and for each sum one whose low p bits are all zero (its
    carry never flips inside the piece) and one whose low p bits are all ones (it flips at U = 1)."""
    m = (1 << p) - 1
    out = [0, M32, rng.getrandbits(32), rng.getrandbits(32)]
    for c in _sum_consts(job):
        high = rng.getrandbits(32) & ~m & M32
        out.append((high | ((0 - c) & m)) & M32)
        out.append((high | ((m - c) & m)) & M32)
    return out


def _check_window(job, vb, p, u_first, iters):
    got = lib().pow_split_wave(job.header, vb, p, u_first, iters)
    assert got.shape == (iters, 64)
    for it in range(iters):
        for lane in range(64):
            word = (vb + u_first + it + (lane << p)) & M32
            assert int(got[it, lane]) == _h0(job, word), (hex(vb), p, u_first + it, lane)


def test_split_sum_constants():
    """The exposed constants are the ones the additive forms use: checked through H0 of the split function on
    single words (pow_job_h0_variant) and by W17 / W24 of the schedule recomputed here."""
    job = _job()
    c = _consts(job)
    assert c['min_log2'] <= 8 and c['max_log2'] == 26
    tail = bytearray(job.header[64:] + b'\x80' + bytes(64 - 44 - 1 - 8) + struct.pack('>Q', 108 * 8))
    w = list(struct.unpack('>16I', bytes(tail)))
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    s0 = lambda x: rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)
    s1 = lambda x: rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10)
    for v in (0, 1, 0x12345678, M32):
        w[10] = v
        ws = list(w)
        for i in range(16, 25):
            ws.append((ws[i - 16] + s0(ws[i - 15]) + ws[i - 7] + s1(ws[i - 2])) & M32)
        assert ws[17] == (c['c17'] + v) & M32
        assert ws[24] == (c['c24'] + v) & M32
    rng = random.Random(3)
    for word in [0, 1, M32, 1 << 26, (1 << 26) - 1] + [rng.getrandbits(32) for _ in range(200)]:
        assert lib().pow_job_h0_variant(job.header, word, VARIANT) == _h0(job, word), hex(word)


@pytest.mark.parametrize('p', [0, 1, 8])
def test_host_wave_loop_complete_piece(p):
    """All 2^p values of U, 64 lanes, in one loop call: each of the four carries (and the nonce word's own) flips
    inside it unless its sum's low bits are zero."""
    job = _job()
    rng = random.Random(100 + p)
    for vb in _bases(job, p, rng):
        _check_window(job, vb, p, 0, 1 << p)


@pytest.mark.parametrize('p', [12, 26])
def test_host_wave_loop_windows(p):
    """Windows of U around each flip and at both ends of the piece; each call walks across its flip."""
    job = _job()
    rng = random.Random(200 + p)
    m = (1 << p) - 1
    n = 1 << p
    for vb in _bases(job, p, rng):
        windows = {(0, 6), (n - 6, 6)}
        for c in _sum_consts(job):
            flip = (n - ((c + vb) & m)) & m  # the first U at which this sum's low bits have wrapped
            if flip:
                first = max(0, flip - 3)
                windows.add((first, min(n, flip + 3) - first))
        for u_first, iters in sorted(windows):
            _check_window(job, vb, p, u_first, iters)
    # one longer walk that starts in the middle of a piece and passes several flips
    vb = rng.getrandbits(32)
    flips = sorted((n - ((c + vb) & m)) & m for c in _sum_consts(job))
    _check_window(job, vb, p, max(0, flips[0] - 2), 40)


def test_wave_loop_rejects_wide_lane_shift():
    with pytest.raises(Exception):
        lib().pow_split_wave(_job().header, 0, 27, 0, 1)


def _mask_form(job, h0):
    return ((h0 ^ job.tword) & job.tmask) == 0 and ((h0 >> job.frac_shift) & 0xf) < job.frac_limit


# difficulty -> the job's predicate has the range form. 0.5: the reference compares the whole hash (the prefix of
# length 0 quirk), so the mask is the full word with the fractional nibble inside it, no prefix above it.
RANGE_FORM = {'0.5': False, '1.0': True, '1.3': True, '2.0': True, '6.3': True, '7.9': True, '8.0': True, '9.5': True}


@pytest.mark.parametrize('difficulty', sorted(RANGE_FORM))
def test_range_predicate_matches_mask_form(difficulty):
    L = lib()
    job = _job(difficulty)
    c = _consts(job)
    assert c['range_ok'] == RANGE_FORM[difficulty]
    if not c['range_ok']:
        with pytest.raises(Exception):
            L.pow_range_hit(*job.native_args(), 0)
        return
    assert c['range_base'] == (c['mid0'] - job.tword) & M32 and 0 < c['range_width'] <= M32
    lo, hi = job.tword, job.tword + c['range_width']  # the range is [lo, hi)
    rng = random.Random(int(float(difficulty) * 10))
    edge = [lo - 2, lo - 1, lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, hi + 1, hi + 2, 0, M32]
    inside = [lo + rng.randrange(c['range_width']) for _ in range(500)]
    hits = 0
    for h0 in edge + inside + [rng.getrandbits(32) for _ in range(3000)]:
        h0 &= M32
        want = _mask_form(job, h0)
        assert L.pow_range_hit(*job.native_args(), h0) == want, (difficulty, hex(h0))
        hits += want
    assert hits >= 500
    assert _mask_form(job, lo) and _mask_form(job, (hi - 1) & M32)
    if hi <= M32:
        assert not _mask_form(job, hi)
    if lo > 0:
        assert not _mask_form(job, lo - 1)


@pytest.mark.parametrize('tmask,tword,fs,fl', [
    (0x0f000000, 0x03000000, 0, 16),   # a mask that is no prefix from the top
    (0, 0, 0, 16),                     # no condition on H0: the width is 2^32
    (0xff000000, 0x12000000, 16, 5),   # a gap between the prefix and the fractional nibble
    (0xf0000000, 0x10000001, 0, 16),   # target bits outside the mask
])
def test_range_predicate_fallback_is_flagged(tmask, tword, fs, fl):
    c = lib().pow_split_consts(_job().header, tmask, tword, fs, fl)
    assert not c['range_ok']


# ---- GPU ----

def _gpu_matches(difficulty, start, count, **kw):
    want = _brute_force(difficulty, start, count)
    g = search(_job(difficulty), start, count, device='gpu', variant=VARIANT, **kw)
    assert g.searched == count
    assert len(g.nonces) == len(set(g.nonces)) and set(g.nonces) == want, (difficulty, start, count, kw)
    return want


@pytest.mark.gpu
def test_gpu_ragged_count_from_odd_start(gpu):
    """Pieces of p = 12 and p = 8, two blocks on the unsplit kernel and 77 words on the host."""
    count = (1 << 18) + (1 << 14) + (1 << 9) + 77
    want = _gpu_matches('2.0', 987_655, count, grid_blocks=4, chunk_iters=3)
    assert 900 < len(want) < 1300  # one nonce in 256
    _gpu_matches('2.0', 987_655, count)  # the default grid and dispatch size


@pytest.mark.gpu
def test_gpu_small_piece_many_dispatches(gpu):
    """One piece of 2^14 (p = 8) on one block, five iterations per dispatch: every wave meets the carry flips."""
    for start in (0x00ffff37, 5 << 14):
        _gpu_matches('2.0', start, 1 << 14, grid_blocks=1, chunk_iters=5)


@pytest.mark.gpu
def test_gpu_piece_crosses_wrap(gpu):
    want = _gpu_matches('2.0', (1 << 32) - (1 << 15) - 5, 1 << 16, grid_blocks=2, chunk_iters=7)
    assert len(want) > 150


@pytest.mark.gpu
@pytest.mark.parametrize('difficulty', ['2.5', '1.0'])
def test_gpu_fractional_and_integer_difficulty(gpu, difficulty):
    want = _gpu_matches(difficulty, 3 << 20, 1 << 16)
    assert len(want) > 50


@pytest.mark.gpu
def test_gpu_mask_form_fallback(gpu):
    """Difficulty 0.5 has no range form: the split kernel keeps the mask predicate (no hit is expected in 2^16
    words of a 32-bit condition, so the count of candidates is compared as well)."""
    job = _job('0.5')
    assert not _consts(job)['range_ok']
    count = 1 << 16
    h = search(job, 0, count, device='cpu', threads=4)
    g = search(job, 0, count, device='gpu', variant=VARIANT)
    assert g.searched == count and g.candidates == h.candidates and g.nonces == h.nonces


@pytest.mark.gpu
def test_gpu_cap_smaller_than_hits(gpu):
    job = _job('2.0')
    start, count = 1 << 24, 1 << 16
    want = _brute_force('2.0', start, count)
    assert len(want) > 4
    searched, total, words = gpu.pow_search_gpu(*job.native_args(), start, count, 2, 3, 4, VARIANT)
    assert searched == count and total == len(want)
    assert len(words) == 4 and len(set(words)) == 4
    for w in words:
        assert job.word_to_nonce(w) in want
