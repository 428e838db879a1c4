"""Planted full-word targets for the PoW kernels (tests/pow_plant.py): every search has tmask = 0xffffffff and
tword = H0 of one chosen nonce word by hashlib, so a hit depends on all 32 bits of H0 at that word's lane, iteration
and piece position. The words sit where the split kernels (variants 10 and 11) can go wrong: every lane, the ends of
a wave's run, the iterations around a recompute of the per-lane constants (a flip: the low p bits of one of the five
sums wrap), the seams between pieces, the unsplit kernel and the host, and the production piece p = 26 with the
dedicated miner's 2^28-nonce dispatch.

The unmarked tests check every planted case's arguments against the host predicate; the gpu tests run them.
"""
import functools
import random
from collections import Counter, namedtuple

import pytest

from upow_amd.models.block import PowTarget
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search

import pow_plant as P
from pow_plant import FULL, M32, SUMS

SPLIT_VARIANTS = (10, 11)
PRODUCTION = None  # grid_blocks: the resident grid of the variant, chunk_iters: 2^28 nonces per dispatch
HOST_EXACT_MAX = 1 << 19  # the unmarked tests search ranges up to this size exactly on the host

# One planted search. where: what the word was chosen for (shown when a test fails); present: the word must be
# reported (False: it must not be).
Case = namedtuple('Case', 'where job word form start count grid_blocks chunk_iters present')


def _case(where, j, word, form, start, count, gb, ci, present=True):
    return Case(where, j, word & M32, form, start & M32, count, gb, ci, present)


def _args(case):
    if case.form in ('range', 'mask', 'excluded'):
        return P.plant(case.job, case.word, case.form)
    delta = {'below': -1, 'above': 1}[case.form]  # a range target one off the word's H0
    return (case.job.header, FULL, (P.h0(case.job, case.word) + delta) & M32, 0, 16)


# ---- the planted cases ----

U_CLASSES = ('zero', 'one', 'top', 'run_first', 'run_last', 'dispatch_first')


def _class_u(cut, cls, rng):
    """A U of the only piece of `cut`: 0, 1, 2^p - 1, the first or the last iteration of a wave's run, or the first
    iteration of a dispatch (a run boundary that also starts the next launch)."""
    p = cut.pieces[0][1]
    runs = list(cut.runs(0))
    if cls == 'zero':
        return 0
    if cls == 'one':
        return 1
    if cls == 'top':
        return (1 << p) - 1
    k = rng.randrange(1, len(runs) - 1)
    if cls == 'run_first':
        return runs[k | 1][0]  # an odd wave of a four-wave grid: never the first of its dispatch
    if cls == 'run_last':
        return runs[k][1]
    assert cls == 'dispatch_first' and cut.waves == 4
    return runs[k & ~3 or 4][0]


@functools.lru_cache(maxsize=None)
def cases_small_pieces():
    """Test 1: one piece on one block, five iterations per dispatch; p = 8 on every lane, p = 12 on six."""
    out = []
    j = P.job(71)
    for p, start, lanes in ((8, 0x00ffff37, range(64)), (12, 0x5bd1e995, (0, 1, 31, 32, 62, 63))):
        count = 1 << (p + 6)
        cut = P.positions(j, start, count, 1, 5)
        assert cut.pieces == [(0, p)]
        for n, lane in enumerate(lanes):
            cls = U_CLASSES[n % len(U_CLASSES)]
            U = _class_u(cut, cls, random.Random(1000 * p + lane))
            for form in ('range', 'mask'):
                out.append(_case(f'p={p} lane={lane} U={U} ({cls})', j, cut.word(0, U, lane), form, start, count, 1, 5))
    return tuple(out)


# p -> (grid_blocks, chunk_iters) of the small flip tests
FLIP_GRID = {8: (1, 5), 12: (2, 7), 16: (4, 64)}
# seed -> two sums whose constants agree mod 2^8, so both flip at the same U of a p = 8 piece: e and a share a
# recompute; seeds 61 and 338 tie sums of different recompute groups (found by scanning seeds on the host)
TIES = {32: ('e', 'a'), 61: ('e', 'w17'), 338: ('w17', 'w24')}
# seed 45: ce = c17 + 1 mod 2^8, so at p = 8 e flips at U_f and W17 at U_f + 1
ADJACENT = (45, 'e', 'w17')


def _flip_cases(j, p, name, u_off, extra_u, tag):
    gb, ci = FLIP_GRID[p]
    count = 1 << (p + 6)
    runs = P.Cut(0, count, gb, ci)  # the runs of a piece do not depend on its base
    first, last = P.inner_run(runs, 0, (1 << p) // 4 + 23 * SUMS.index(name))
    u_f = first + u_off
    start = P.start_with_flip(j, p, name, u_f, random.Random(p * 10 + SUMS.index(name)).getrandbits(32))
    cut = P.positions(j, start, count, gb, ci)
    out = []
    for lane, form in ((0, 'range'), (63, 'mask')) if SUMS.index(name) % 2 else ((0, 'mask'), (63, 'range')):
        for U in (u_f - 1, u_f, u_f + 1, *extra_u(u_f), last):
            out.append(_case(f'{tag} p={p} {name} flips at U={u_f}, run {first}..{last}: lane={lane} U={U}', j,
                             cut.word(0, U, lane), form, start, count, gb, ci))
    return out, cut, u_f


@functools.lru_cache(maxsize=None)
def cases_flips_small():
    """Test 2: for p in (8, 12, 16) and each sum, a piece whose base puts that sum's flip strictly inside a wave's
    run; the tie jobs and the job with adjacent flips at p = 8."""
    out = []
    for p in FLIP_GRID:
        for name in SUMS:
            out += _flip_cases(P.job(71), p, name, 2, lambda u: (), 'flip')[0]
    for seed, (a, _) in TIES.items():
        out += _flip_cases(P.job(seed), 8, a, 2, lambda u: (), f'tie seed={seed}')[0]
    seed, a, _ = ADJACENT
    out += _flip_cases(P.job(seed), 8, a, 1, lambda u: (u + 2,), f'adjacent seed={seed}')[0]
    return tuple(out)


PROD_JOB = (71, '6.3')
PROD_COUNT = 1 << 32
WRAP_START = 0x9e3779b9


def _prod_lanes(name):
    return (0, 63, random.Random(SUMS.index(name)).randrange(1, 63))


@functools.lru_cache(maxsize=None)
def cases_production(name):
    """Test 3, one sum: U_f - 1, U_f, U_f + 1 of the whole-sweep piece (p = 26) on lanes 0, 63 and a seeded random
    one. From start 0 the nonce word's own low 26 bits never wrap inside the piece (U_f = 2^26), so the flip of
    'v' is planted in the sweep that starts at WRAP_START, where it lies inside."""
    j = P.job(*PROD_JOB)
    start = WRAP_START if name == 'v' else 0
    u_f = P.flip_u(j, start, 26, name)
    assert 1 < u_f < (1 << 26) - 1
    out = []
    for lane in _prod_lanes(name):
        form = 'mask' if lane not in (0, 63) else 'range'
        for U in (u_f - 1, u_f, u_f + 1):
            word = start + U + (lane << 26)
            out.append(_case(f'p=26 start={start:#x} {name} flips at U={u_f}: lane={lane} U={U}', j, word, form,
                             start, PROD_COUNT, PRODUCTION, PRODUCTION))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_production_ends():
    """Test 3: both ends of the piece on the first and the last lane; the words on either side of 2^32 in the sweep
    that starts at WRAP_START (its flip of 'v' is cases_production('v'))."""
    j = P.job(*PROD_JOB)
    out = []
    for lane in (0, 63):
        for U, form in ((0, 'range'), ((1 << 26) - 1, 'mask')):
            out.append(_case(f'p=26 start=0: lane={lane} U={U}', j, U + (lane << 26), form, 0, PROD_COUNT,
                             PRODUCTION, PRODUCTION))
    for word, form in ((M32, 'range'), (0, 'mask')):
        out.append(_case(f'p=26 start={WRAP_START:#x}: word {word:#x} at the wrap', j, word, form, WRAP_START,
                         PROD_COUNT, PRODUCTION, PRODUCTION))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_production_default_dispatch():
    """Test 3: one planted search with chunk_iters = 0 (2^23 nonces per dispatch once the process has run node
    kernels, 2^28 otherwise): the flip of W24."""
    c = cases_production('w24')[1]
    return (c._replace(where=c.where + ' (default dispatch)', chunk_iters=0),)


SEAM_START, SEAM_COUNT, SEAM_GRID = 987_655, (1 << 18) + (1 << 14) + (1 << 9) + 77, (4, 3)


@functools.lru_cache(maxsize=None)
def cases_seams():
    """Test 4: the words on either side of every seam of a ragged range (a p = 12 piece, a p = 8 piece, two blocks
    of the unsplit kernel, 77 host words), and one word outside each end."""
    j = P.job(71)
    a, b = 1 << 18, (1 << 18) + (1 << 14)
    spots = [('last word of the first piece', a - 1, 'piece', 0), ('first word of the second piece', a, 'piece', 1),
             ('last word of the last piece', b - 1, 'piece', 1), ('first word of the unsplit kernel', b, 'remainder', None),
             ('last word of the unsplit kernel', b + 511, 'remainder', None), ('first host word', b + 512, 'host', None),
             ('last host word', SEAM_COUNT - 1, 'host', None), ('the word below the range', -1, 'outside', None),
             ('the word above the range', SEAM_COUNT, 'outside', None)]
    cut = P.positions(j, SEAM_START, SEAM_COUNT, *SEAM_GRID)
    assert cut.pieces == [(0, 12), (a, 8)]
    out = []
    for n, (where, off, kind, piece) in enumerate(spots):
        word = (SEAM_START + off) & M32
        pos = cut.locate(word)
        assert (pos.kind, pos.piece) == (kind, piece), (where, pos)
        out.append(_case(where, j, word, ('range', 'mask')[n % 2], SEAM_START, SEAM_COUNT, *SEAM_GRID,
                         present=kind != 'outside'))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_no_false_hit():
    """Test 5: three words of test 1 under targets that they just miss."""
    picked = [c for c in cases_small_pieces() if c.form == 'range'][3:40:17]
    assert len(picked) == 3
    return tuple(c._replace(form=form, present=False, where=f'{c.where} {form}')
                 for c in picked for form in ('excluded', 'below', 'above'))


@functools.lru_cache(maxsize=None)
def cases_older(v1):
    """Test 7: ten words of a 2^16 range, its first and last among them, on the default grid and dispatch."""
    j = P.job_v1() if v1 else P.job(73, '2.5')
    start, count = 0x3c6ef372, 1 << 16
    rng = random.Random(7 + v1)
    offs = [0, count - 1] + rng.sample(range(1, count - 1), 8)
    return tuple(_case(f'{"138" if v1 else "108"}-byte header, word {n} of the range', j, start + n,
                       ('range', 'mask')[k % 2], start, count, 0, 0) for k, n in enumerate(offs))


def _all_cases():
    out = list(cases_small_pieces()) + list(cases_flips_small())
    for name in SUMS:
        out += cases_production(name)
    out += cases_production_ends() + cases_production_default_dispatch() + cases_seams() + cases_no_false_hit()
    out += cases_older(True) + cases_older(False)
    return out


# ---- on the host: the generator and the arguments ----

def test_classes_are_covered():
    """Test 1's draws: every class of U at least twice per p, all 64 lanes at p = 8."""
    for p, lanes, least in ((8, 64, 2), (12, 6, 1)):  # p = 12: six lanes for six classes
        for form in ('range', 'mask'):
            cases = [c for c in cases_small_pieces() if c.where.startswith(f'p={p} ') and c.form == form]
            assert len(cases) == lanes and len({c.word for c in cases}) == lanes
            seen = Counter(c.where[c.where.index('('):] for c in cases)
            assert len(seen) == len(U_CLASSES) and min(seen.values()) >= least, (p, seen)


def test_model_places_each_word():
    """positions() puts every planted word of a split piece at the lane and U it was made from, and inside the
    run the case names."""
    j = P.job(71)
    cut = P.positions(j, 0x00ffff37, 1 << 14, 1, 5)
    runs = list(cut.runs(0))
    assert runs[:5] == [(0, 4), (5, 9), (10, 14), (15, 19), (20, 24)] and runs[-4:] == [(240, 243), (244, 247),
                                                                                         (248, 251), (252, 255)]
    assert sum(last - first + 1 for first, last in runs) == 256
    for lane in (0, 17, 63):
        for U in (0, 4, 5, 239, 240, 255):
            pos = cut.locate(cut.word(0, U, lane))
            assert (pos.kind, pos.p, pos.U, pos.lane) == ('piece', 8, U, lane)
            assert pos.run_first <= U <= pos.run_last and (pos.run_first, pos.run_last) in runs
    # a whole sweep on 2,048 blocks: sixteen dispatches of 8,192 runs of 512
    big = P.positions(j, WRAP_START, 1 << 32, 2048, (1 << 28) // (2048 * 256))
    assert big.pieces == [(0, 26)]
    pos = big.locate(0)
    assert pos.kind == 'piece' and (WRAP_START + pos.U + (pos.lane << 26)) & M32 == 0
    assert pos.run_last - pos.run_first == 511 and pos.run_first % 512 == 0


def test_flips_lie_inside_a_run():
    """Test 2's bases: the named sum's first flip is strictly inside a wave's run (iterations before and after
    it in the same run), the ties tie and the adjacent flips are adjacent."""
    for p in FLIP_GRID:
        for name in SUMS:
            cases, cut, u_f = _flip_cases(P.job(71), p, name, 2, lambda u: (), 'flip')
            assert P.flip_u(cases[0].job, cases[0].start, p, name) == u_f
            for c in cases:
                pos = cut.locate(c.word)
                assert pos.kind == 'piece' and pos.run_first < u_f < pos.run_last, c.where
                assert pos.run_first <= pos.U <= pos.run_last
    for seed, (a, b) in TIES.items():
        j = P.job(seed)
        c = P.sum_consts(j)
        assert (c[a] - c[b]) & 0xff == 0
        cases, cut, u_f = _flip_cases(j, 8, a, 2, lambda u: (), 'tie')
        assert P.flip_u(j, cases[0].start, 8, a) == P.flip_u(j, cases[0].start, 8, b) == u_f
    assert P.GROUP['e'] == P.GROUP['a'] and P.GROUP['e'] != P.GROUP['w17'] != P.GROUP['w24']
    seed, a, b = ADJACENT
    j = P.job(seed)
    cases, cut, u_f = _flip_cases(j, 8, a, 1, lambda u: (u + 2,), 'adjacent')
    assert P.flip_u(j, cases[0].start, 8, a) == u_f and P.flip_u(j, cases[0].start, 8, b) == u_f + 1
    assert P.GROUP[a] != P.GROUP[b]
    pos = cut.locate(cases[0].word)
    assert pos.run_first < u_f and u_f + 2 <= pos.run_last


def test_planted_arguments_on_the_host():
    """Every planted case against the host predicate and the host forms of the kernels' arithmetic."""
    L = lib()
    cases = _all_cases()
    assert len(cases) > 300
    for c in cases:
        args = _args(c)
        t = P.h0(c.job, c.word)
        v2 = len(c.job.header) == 108
        hit = c.form in ('range', 'mask')
        assert L.pow_check_word(*args, c.word) == hit, c.where
        assert not L.pow_check_word(*args, c.word ^ 1), c.where
        if hit:
            assert args[1] == FULL and args[2] == t
        if v2:
            assert P.range_ok(args) == (c.form in ('range', 'below', 'above')), c.where
            if P.range_ok(args):
                for h in (t - 1, t, t + 1):
                    h &= M32
                    assert L.pow_range_hit_folded(*args, h) == L.pow_range_hit(*args, h) == (h == args[2]), c.where
        for variant in (9, 10, 11):
            assert L.pow_job_h0_variant(c.job.header, c.word, variant) == t, (c.where, variant)


def test_small_ranges_on_the_host():
    """pow_search_host over every planted range of up to 2^19 words: exactly the planted word, or nothing where the
    word must be absent."""
    L = lib()
    ran = 0
    for c in _all_cases():
        if c.count > HOST_EXACT_MAX:
            continue
        searched, total, words = L.pow_search_host(*_args(c), c.start, c.count, 8)
        assert searched == c.count and total == len(words)
        assert [int(w) for w in words] == ([c.word] if c.present else []), c.where
        ran += 1
    assert ran > 150


# ---- GPU ----

def _grid(gpu, case, variant):
    if case.grid_blocks is not PRODUCTION:
        return case.grid_blocks, case.chunk_iters
    gb = gpu.pow_kernel_info(variant)['resident_blocks']
    return gb, ((1 << 28) // (gb * 256) if case.chunk_iters is PRODUCTION else case.chunk_iters)


def _run(gpu, case, variant):
    """One planted search: one pow_search_gpu call."""
    args = _args(case)
    gb, ci = _grid(gpu, case, variant)
    searched, total, words = gpu.pow_search_gpu(*args, case.start, case.count, gb, ci, 1 << 16, variant)
    words = [int(w) for w in words]
    where = (variant, case.where, hex(case.word), case.form)
    assert searched == case.count, where
    assert (case.word in words) == case.present, (where, [hex(w) for w in words[:8]])
    assert total == len(words), where
    for w in words:
        assert P.h0(case.job, w) == args[2], (where, hex(w))
    if case.form != 'range' and case.present:
        assert all(((P.h0(case.job, w) >> args[3]) & 0xf) < args[4] for w in words), where


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_small_pieces_every_lane(gpu, variant):
    for c in cases_small_pieces():
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_flips_small_p(gpu, variant):
    for c in cases_flips_small():
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('name', SUMS)
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_production_piece_flip(gpu, variant, name):
    """The whole sweep as one p = 26 piece with the dedicated miner's dispatch, passed explicitly; the flip lies
    inside a wave's run on this card's grid, so U_f is reached through the recompute and not through a prologue."""
    cases = cases_production(name)
    j, start = cases[0].job, cases[0].start
    cut = P.positions(j, start, PROD_COUNT, *_grid(gpu, cases[0], variant))
    u_f = P.flip_u(j, start, 26, name)
    pos = cut.locate(start + u_f)
    assert (pos.p, pos.U, pos.lane) == (26, u_f, 0) and pos.run_first < u_f <= pos.run_last, pos
    for c in cases:
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_production_piece_ends_and_wrap(gpu, variant):
    for c in cases_production_ends():
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_production_piece_default_dispatch(gpu, variant):
    for c in cases_production_default_dispatch():
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_seams(gpu, variant):
    for c in cases_seams():
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_no_false_hit(gpu, variant):
    for c in cases_no_false_hit():
        assert not c.present
        _run(gpu, c, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('v1,variant', [(True, 0), (False, 9)])
def test_gpu_older_paths(gpu, v1, variant):
    for c in cases_older(v1):
        _run(gpu, c, variant)


# ---- whole-digest targets through search() ----

DIGEST_SEED = 72


def _word_with_digit(j, first, index, wanted):
    """The first word from `first` on whose digest has one of the `wanted` hex digits at `index`."""
    for word in range(first, first + 4096):
        if P.digest(j, word)[index] in wanted:
            return word
    raise AssertionError('no such word')


def _digest_job(difficulty, word, near_miss=False):
    """A job whose target is the leading floor(difficulty) digits of `word`'s own digest: the fake previous hash ends
    in them. The header holds the difficulty, so the digest is that of the header which is searched. near_miss: the
    ninth digit changed, which H0 does not see."""
    base = P.job(DIGEST_SEED, difficulty)
    d = int(float(difficulty))
    want = P.digest(base, word)[:d]
    if near_miss:
        assert d >= 9
        want = want[:8] + '%x' % (int(want[8], 16) ^ 1) + want[9:]
    target = PowTarget.from_difficulty('0' * (64 - d) + want, difficulty)
    return PowJob.create(base.header[:-4], target)


def _digest_cases():
    """(difficulty, word): 10.5 needs the digit under the fractional nibble (the eleventh) below 8, and the words of
    the other two are picked the same way."""
    out = []
    for k, difficulty in enumerate(('8.0', '9.0', '10.5')):
        base = P.job(DIGEST_SEED, difficulty)
        word = _word_with_digit(base, 0x6a09e667 + (k << 20), 10, '01234567')
        out.append((difficulty, word))
    return out


def _around(word, k):
    return (word - 12_345 - 7_001 * k) & M32


def test_digest_targets_on_the_host():
    for k, (difficulty, word) in enumerate(_digest_cases()):
        j = _digest_job(difficulty, word)
        assert j.native_args()[1:] == (FULL, P.h0(j, word), 0, 16)
        r = search(j, _around(word, k), 1 << 16, device='cpu', threads=4)
        assert (r.searched, r.candidates, r.nonces) == (1 << 16, 1, [j.word_to_nonce(word)])
        if float(difficulty) >= 9:
            r = search(_digest_job(difficulty, word, True), _around(word, k), 1 << 16, device='cpu', threads=4)
            assert (r.candidates, r.nonces) == (1, [])
    for wanted, hit in (('01', True), ('2', False)):
        j, word = _frac_job(wanted)
        r = search(j, _around(word, 5), 1 << 16, device='cpu', threads=4)
        assert (r.candidates, r.nonces) == ((1, [j.word_to_nonce(word)]) if hit else (0, []))


def _frac_job(wanted):
    """Difficulty 7.9: seven digits and the eighth below 2. A word whose eighth digit is one of `wanted`."""
    base = P.job(DIGEST_SEED, '7.9')
    word = _word_with_digit(base, 0xbb67ae85, 7, wanted)
    j = _digest_job('7.9', word)
    assert j.native_args()[1:] == (0xfffffff0, P.h0(j, word) & 0xfffffff0, 0, 2)
    return j, word


@pytest.mark.gpu
@pytest.mark.parametrize('variant', (0,) + SPLIT_VARIANTS)
def test_gpu_digest_targets_through_search(gpu, variant):
    """Difficulty >= 8: the kernel hands over a candidate on H0 and search() confirms the other digits."""
    for k, (difficulty, word) in enumerate(_digest_cases()):
        j = _digest_job(difficulty, word)
        r = search(j, _around(word, k), 1 << 16, device='gpu', variant=variant)
        assert (r.searched, r.candidates, r.nonces) == (1 << 16, 1, [j.word_to_nonce(word)]), (variant, difficulty)
        if float(difficulty) >= 9:
            r = search(_digest_job(difficulty, word, True), _around(word, k), 1 << 16, device='gpu', variant=variant)
            assert (r.searched, r.candidates, r.nonces) == (1 << 16, 1, []), (variant, difficulty)
    for wanted, hit in (('01', True), ('2', False)):
        j, word = _frac_job(wanted)
        r = search(j, _around(word, 5), 1 << 16, device='gpu', variant=variant)
        assert (r.searched, r.candidates, r.nonces) == ((1 << 16, 1, [j.word_to_nonce(word)]) if hit
                                                        else (1 << 16, 0, [])), (variant, wanted)


# ---- the exact set of a mid-size piece ----

MID_START, MID_COUNT = 0x243f6a89, 1 << 26


@functools.lru_cache(maxsize=None)
def _mid_host():
    r = search(P.job(74, '5.0'), MID_START, MID_COUNT, device='cpu', threads=16)
    assert r.searched == MID_COUNT
    return r.candidates, tuple(r.nonces)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', SPLIT_VARIANTS)
def test_gpu_mid_size_piece_exact_set(gpu, variant):
    """2^26 words (p = 20) at difficulty 5.0 on the resident grid with 2^28 nonces per dispatch, against the host
    search: one word in 2^20 hits."""
    candidates, nonces = _mid_host()
    assert len(nonces) > 20  # expectation 64
    gb = gpu.pow_kernel_info(variant)['resident_blocks']
    g = search(P.job(74, '5.0'), MID_START, MID_COUNT, device='gpu', grid_blocks=gb,
               chunk_iters=(1 << 28) // (gb * 256), variant=variant)
    assert g.searched == MID_COUNT and g.candidates == candidates
    assert tuple(g.nonces) == nonces
