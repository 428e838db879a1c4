"""Planted PoW targets: a search whose only hit is a nonce word chosen in advance.

pow_search_gpu takes the target directly, so a test picks a nonce word w, takes H0(w) from hashlib and searches with
tmask = 0xffffffff, tword = H0(w): the kernel must report w, and all 32 bits of H0 at that lane, iteration and
piece position are checked. Another word with the same H0 is a legitimate hit too (over 2^32 words one is expected
more often than not), so the tests ask that w is among the reported words and that every reported word has that H0.

positions() is a Python model of how pow_search_gpu cuts a range (csrc/pow_search.hip). The tests use it to choose
words at particular places of a piece; what a search must return is always decided by hashlib.
"""
import functools
import hashlib
import random
from collections import namedtuple

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob
from upow_amd.utils import p256
from upow_amd.utils.codec import AddressFormat, point_to_string

M32 = 0xffffffff
FULL = 0xffffffff
SUMS = ('v', 'e', 'a', 'w17', 'w24')  # the five sums whose low p bits the split kernels keep on the scalar unit
# which sums share a recompute in pow_split_lane_update: e and a are one branch
GROUP = {'v': 0, 'e': 1, 'a': 1, 'w17': 2, 'w24': 3}
MIN_LOG2, MAX_LOG2 = 8, 26  # kPowSplitMinLog2, kPowSplitMaxLog2


@functools.lru_cache(maxsize=None)
def job(seed, difficulty='2.0'):
    """The 108-byte-header job of tests/test_pow_fill.py's _job(seed, difficulty)."""
    rng = random.Random(seed)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    pre = header_prefix(prev, 'DgQKikeDqS2Fzue23KuA36L4eJSFh649zA9jJ6zwbzUMp', hashlib.sha256(rng.randbytes(8)).hexdigest(),
                        1_790_000_000 + seed, difficulty)
    j = PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))
    assert len(j.header) == 108
    return j


@functools.lru_cache(maxsize=None)
def job_v1(difficulty='2.5'):
    """The 138-byte-header job of tests/test_pow_variants.py's _job(True, difficulty)."""
    rng = random.Random(23)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    key = p256.get_public_key(rng.randrange(1, p256.N))
    addr = point_to_string(key, AddressFormat.FULL_HEX)
    pre = header_prefix(prev, addr, hashlib.sha256(rng.randbytes(8)).hexdigest(), 1_700_000_023, difficulty)
    j = PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))
    assert len(j.header) == 138
    return j


def digest(j, word):
    """Hex SHA-256 of the header with nonce word `word`, by hashlib."""
    return hashlib.sha256(j.header_with_nonce(j.word_to_nonce(word & M32))).hexdigest()


def h0(j, word):
    return int(digest(j, word)[:8], 16)


def sum_consts(j):
    """The constants in front of vb + U in the five sums, by name: W10 = v, e11 = ce + v, a11 = ca + v,
    W17 = c17 + v, W24 = c24 + v."""
    c = lib().pow_split_consts(*j.native_args())
    return {'v': 0, 'e': c['ce'], 'a': c['ca'], 'w17': c['c17'], 'w24': c['c24']}


def flip_u(j, vb, p, c):
    """The first U >= 1 at which the low p bits of c + vb + U have wrapped; 2^p (outside the piece) if they are
    zero at U = 0. `c` is a constant or one of SUMS."""
    if isinstance(c, str):
        c = sum_consts(j)[c]
    n = 1 << p
    return n - ((c + vb) & (n - 1))


def plant(j, word, form):
    """Native target arguments (header, tmask, tword, frac_shift, frac_limit) under which `word` is a hit
    ('range', 'mask') or just not one ('excluded').
    range:    the full mask alone: the kernels' range form of width 1
    mask:     the full mask and a fractional nibble with limit nibble + 1, at a shift for which the job has no range
              form, so the kernels keep the mask predicate
    excluded: the same with limit = nibble, which the word's own nibble does not pass"""
    t = h0(j, word)
    if form == 'range':
        return (j.header, FULL, t, 0, 16)
    assert form in ('mask', 'excluded'), form
    if len(j.header) != 108:  # no split kernel and no range form for this header: any shift keeps the mask form
        s = 12
        return (j.header, FULL, t, s, ((t >> s) & 0xf) + (form == 'mask'))
    for s in range(0, 32, 4):
        nib = (t >> s) & 0xf
        if not lib().pow_split_consts(j.header, FULL, t, s, nib + 1)['range_ok']:
            return (j.header, FULL, t, s, nib + (form == 'mask'))
    raise AssertionError('no fractional shift keeps the mask form for H0 = %08x' % t)


def range_ok(args):
    return bool(lib().pow_split_consts(*args)['range_ok'])


# kind: 'piece' (a split kernel), 'remainder' (the unsplit kernel, whole blocks), 'host', 'outside'.
# For 'piece': its index, p, U, lane, and the first and last U of the run of the wave that takes U (one wave's
# consecutive iterations within one dispatch, behind one prologue).
Position = namedtuple('Position', 'kind piece p U lane run_first run_last')


class Cut:
    """pow_search_gpu's cutting of [start, start + count) for variants 10 and 11 on the 108-byte header: maximal
    power-of-two pieces of at least 2^14 words, largest first, p = min(log2 - 6, 26); then the unsplit kernel in
    whole blocks of 256; then the host."""

    def __init__(self, start, count, grid_blocks, chunk_iters):
        assert grid_blocks > 0 and chunk_iters > 0 and 0 < count <= 1 << 32
        self.start, self.count = start & M32, count
        self.waves, self.chunk_iters = grid_blocks * 4, chunk_iters
        self.pieces = []  # (offset from start, p)
        done = 0
        while count - done >= 1 << (MIN_LOG2 + 6):
            p = min((count - done).bit_length() - 1 - 6, MAX_LOG2)
            self.pieces.append((done, p))
            done += 1 << (p + 6)
        self.split_end = done
        self.kernel_end = done + (count - done) // 256 * 256

    def vb(self, piece):
        return (self.start + self.pieces[piece][0]) & M32

    def word(self, piece, U, lane):
        p = self.pieces[piece][1]
        assert 0 <= U < 1 << p and 0 <= lane < 64
        return (self.vb(piece) + U + (lane << p)) & M32

    def runs(self, piece):
        """(first U, last U) of every wave's run of the piece, in order."""
        n = 1 << self.pieces[piece][1]
        u = 0
        while u < n:
            left = n - u
            iters = min(self.chunk_iters, (left + self.waves - 1) // self.waves)
            need = (left + iters - 1) // iters
            gb = min(self.waves // 4, (need + 3) // 4)
            u_end = min(n, u + gb * 4 * iters)
            for first in range(u, u_end, iters):
                yield first, min(u_end, first + iters) - 1
            u = u_end

    def run_of(self, piece, U):
        n = 1 << self.pieces[piece][1]
        u = 0
        while u < n:  # dispatch by dispatch, as runs() does, without listing the waves
            left = n - u
            iters = min(self.chunk_iters, (left + self.waves - 1) // self.waves)
            need = (left + iters - 1) // iters
            gb = min(self.waves // 4, (need + 3) // 4)
            u_end = min(n, u + gb * 4 * iters)
            if U < u_end:
                first = u + (U - u) // iters * iters
                return first, min(u_end, first + iters) - 1
            u = u_end
        raise AssertionError((piece, U))

    def locate(self, word):
        off = (word - self.start) & M32
        if off >= self.count:
            return Position('outside', None, None, None, None, None, None)
        if off >= self.kernel_end:
            return Position('host', None, None, None, None, None, None)
        if off >= self.split_end:
            return Position('remainder', None, None, None, None, None, None)
        for k, (first, p) in enumerate(self.pieces):
            if first <= off < first + (1 << (p + 6)):
                rel = off - first
                U, lane = rel & ((1 << p) - 1), rel >> p
                return Position('piece', k, p, U, lane, *self.run_of(k, U))
        raise AssertionError(off)


def positions(j, start, count, grid_blocks, chunk_iters):
    assert len(j.header) == 108, 'only the 108-byte header is cut into pieces'
    return Cut(start, count, grid_blocks, chunk_iters)


def start_with_flip(j, p, name, u_f, high):
    """A piece base vb (high bits from `high`) for which sum `name`'s first flip is at U = u_f, 0 < u_f < 2^p."""
    m = (1 << p) - 1
    assert 0 < u_f <= m
    vb = ((high & ~m) | ((0 - u_f - sum_consts(j)[name]) & m)) & M32
    assert flip_u(j, vb, p, name) == u_f
    return vb


def inner_run(cut, piece, near):
    """The first run at or after U = near that has room for U_f - 1, U_f, U_f + 1 and a later last iteration."""
    for first, last in cut.runs(piece):
        if first >= near and last - first >= 4:
            return first, last
    raise AssertionError('no run of five iterations')
