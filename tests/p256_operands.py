"""Operand sets for the P-256 arithmetic tests (test_p256_arith.py on the host, test_p256_arith_gpu.py on the
device; the two older host tests of test_p256.py take their case lists from here too).

Whole signatures feed the field code pseudo-random limbs. These sets hold what they practically never do: zero
and all-ones limbs, long carry and borrow runs, values next to p, n and the powers of 2^32, unreduced inputs,
both ends of the Solinas overflow, scalars that leave the divsteps loop after one round next to ones that need
nearly all twenty, and points with Z != 1. Every generator is seeded: the sets are the same on every run.
"""
import functools
import random

from upow_amd.utils import p256 as o

P, N = o.P, o.N
R = (1 << 256) % N          # the scalar Montgomery radix mod n
R2 = R * R % N
WORDS = (0, 1, 0xffffffff, 0x80000000, 0xfffffffe)

FE_EDGE = tuple([0, 1, 2, P - 1, P - 2, (P - 1) // 2, (1 << 255) % P, (1 << 224) - 1, (1 << 96) + 5, P - (1 << 96)]
                + [1 << (32 * k) for k in range(1, 8)] + [(1 << (32 * k)) - 1 for k in range(1, 8)]
                + [P - (1 << (32 * k)) for k in range(1, 8)] + [o.B, o.GX, o.GY])


def _pattern(rng, limbs: int) -> int:
    return sum(rng.choice(WORDS) << (32 * k) for k in range(limbs))


def fe_patterned(count: int, seed: int = 101):
    """Field values whose every limb is one of WORDS, reduced mod p."""
    rng = random.Random(seed)
    return [_pattern(rng, 8) % P for _ in range(count)]


def fe_random(count: int, seed: int = 102):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def fe_unreduced():
    """256-bit inputs at or past p (fe_mul, fe_sqr and the pair-split product only; the decompression kernel
    meets them for x >= p) and patterned words left as they are, about a third of which are >= p."""
    rng = random.Random(103)
    vals = [P, P + 1, (1 << 256) - 1, (1 << 256) - (1 << 224)] + [_pattern(rng, 8) for _ in range(300)]
    assert sum(v >= P for v in vals) >= 50
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def field_pairs():
    """(a, b) canonical: all pairs of FE_EDGE, then 600 patterned and 1,500 random values with a seeded partner."""
    rng = random.Random(104)
    singles = fe_patterned(600) + fe_random(1500)
    pool = list(FE_EDGE) + singles
    return tuple([(a, b) for a in FE_EDGE for b in FE_EDGE] + [(a, rng.choice(pool)) for a in singles])


@functools.lru_cache(maxsize=None)
def field_pairs_unreduced():
    """(a, b) with a unreduced and b unreduced or an edge value, both orders."""
    rng = random.Random(105)
    pool = list(fe_unreduced()) + list(FE_EDGE)
    pairs = [(a, rng.choice(pool)) for a in fe_unreduced()]
    return tuple(pairs + [(b, a) for a, b in pairs[::3]])


@functools.lru_cache(maxsize=None)
def field_singles():
    """Canonical values for the one-operand field operations."""
    return tuple(list(FE_EDGE) + fe_patterned(600) + fe_random(1500))


@functools.lru_cache(maxsize=None)
def legacy_field_cases():
    """The cases test_p256.py::test_field_arithmetic_matches_python has always drawn, from the same stream:
    (2,011 operand pairs, 4,000 512-bit values for fe_reduce)."""
    rng = random.Random(13)
    edge = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 1 << 255, (1 << 224) - 1, (1 << 96) + 5, P - (1 << 96),
            (1 << 256) - 1 - (1 << 224) - P // 3]
    vals = [v % P for v in edge] + [rng.randrange(P) for _ in range(1500)]
    vals += [sum(rng.choice((0, 0xffffffff, 1)) << (32 * k) for k in range(8)) % P for _ in range(500)]
    pairs = [(vals[k], vals[rng.randrange(len(vals))]) for k in range(len(vals))]
    wide = [sum(rng.choice(WORDS) << (32 * k) for k in range(16)) if rng.random() < 0.7 else rng.getrandbits(512)
            for _ in range(4000)]
    return tuple(pairs), tuple(wide)


def reduce_cases():
    """The 4,000 512-bit values of the host test: 70 % word patterns from WORDS, the rest random."""
    return legacy_field_cases()[1]


def solinas_sums(c: int):
    """s1..s9 of the NIST fast reduction (FIPS 186-4 D.2.3) of a 512-bit c, as integers: the rows of fe_reduce."""
    w = [(c >> (32 * k)) & 0xffffffff for k in range(16)]
    rows = [(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]),
            (0, 0, 0, w[11], w[12], w[13], w[14], w[15]),
            (0, 0, 0, w[12], w[13], w[14], w[15], 0),
            (w[8], w[9], w[10], 0, 0, 0, w[14], w[15]),
            (w[9], w[10], w[11], w[13], w[14], w[15], w[13], w[8]),
            (w[11], w[12], w[13], 0, 0, 0, w[8], w[10]),
            (w[12], w[13], w[14], w[15], 0, 0, w[9], w[11]),
            (w[13], w[14], w[15], w[8], w[9], w[10], 0, w[12]),
            (w[14], w[15], 0, w[9], w[10], w[11], 0, w[13])]
    return [sum(x << (32 * k) for k, x in enumerate(row)) for row in rows]


def solinas_overflow(c: int) -> int:
    """T = floor((s1 + 2 s2 + 2 s3 + s4 + s5 - s6 - s7 - s8 - s9) / 2^256): the signed ninth limb fe_reduce folds."""
    s = solinas_sums(c)
    return (s[0] + 2 * s[1] + 2 * s[2] + s[3] + s[4] - s[5] - s[6] - s[7] - s[8]) >> 256


def solinas_extreme(sign: int) -> int:
    """The 512-bit c that maximises (sign = 1) or minimises (-1) the Solinas sum: it is linear in each word of c,
    so each word goes to 0 or 0xffffffff by the sign of its coefficient."""
    def total(c):
        s = solinas_sums(c)
        return s[0] + 2 * s[1] + 2 * s[2] + s[3] + s[4] - s[5] - s[6] - s[7] - s[8]
    c = 0
    for k in range(16):
        if sign * total(1 << (32 * k)) > 0:
            c |= 0xffffffff << (32 * k)
    return c


@functools.lru_cache(maxsize=None)
def legacy_scalar_cases():
    """The full case list of test_p256.py::test_scalar_inverse_divsteps_matches_pow: small values, 2^k, n - 2^k,
    runs of ones, 3,000 random; reduced mod n, zero dropped."""
    rng = random.Random(11)
    cases = [1, 2, 3, N - 1, N - 2, (N - 1) // 2, (1 << 255) % N, (1 << 256) - 1 - N, (1 << 128) - 1]
    cases += [1 << k for k in range(256)] + [N - (1 << k) for k in range(255)]
    cases += [((1 << k) - 1) % N for k in range(1, 257)] + [rng.randrange(1, N) for _ in range(3000)]
    return tuple(s % N for s in cases if s % N)


def sc_patterned(count: int, seed: int = 111):
    rng = random.Random(seed)
    return [v for v in (_pattern(rng, 8) % N for _ in range(count)) if v]


@functools.lru_cache(maxsize=None)
def scalar_cases():
    """Invertible scalars in [1, n): the legacy list, n - 1, n - 2, R, R^2 mod n, and patterned values mod n."""
    return tuple(list(legacy_scalar_cases()) + [N - 1, N - 2, R, R2] + sc_patterned(700))


def scalar_cases_shuffled():
    """scalar_cases in a fixed random order, for the device: every wave then mixes scalars that leave the divsteps
    loop after one or two rounds (1, 2^k) with ones that need nearly all twenty."""
    cases = list(scalar_cases())
    random.Random(112).shuffle(cases)
    return tuple(cases)


SC_EDGE = (0, 1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, R, R2, N - R, (1 << 255) % N, (1 << 128) - 1,
           (1 << 224) - 1, 1 << 32, (1 << 32) - 1, N - (1 << 32), 1 << 192, N - (1 << 192))


@functools.lru_cache(maxsize=None)
def scalar_pairs():
    """(a, b) in [0, n): all pairs of SC_EDGE, then patterned and random scalars with a seeded partner."""
    rng = random.Random(113)
    singles = sc_patterned(400, 114) + [rng.randrange(N) for _ in range(1000)]
    pool = list(SC_EDGE) + singles
    return tuple([(a, b) for a in SC_EDGE for b in SC_EDGE] + [(a, rng.choice(pool)) for a in singles])


@functools.lru_cache(maxsize=None)
def scalar_reduce_cases():
    """sc_reduce: values below n, and values in [n, 2^256)."""
    rng = random.Random(115)
    high = [N, N + 1, N + 2, (1 << 256) - 1, (1 << 256) - 2, N + (1 << 32), N + (1 << 128) - 1, (1 << 256) - (1 << 224)]
    high += [rng.randrange(N, 1 << 256) for _ in range(300)] + [v for v in (_pattern(rng, 8) for _ in range(300)) if v >= N]
    return tuple(list(SC_EDGE) + sc_patterned(300, 116) + high)


@functools.lru_cache(maxsize=None)
def booth_cases():
    """Scalars below 2^256 for the signed 5-bit windows: the structured u2 of test_p256_edges.py, 500 random, and
    both ends of the range."""
    from test_p256_edges import _STRUCTURED_U2
    rng = random.Random(117)
    return tuple(list(_STRUCTURED_U2) + [0, (1 << 256) - 1, (1 << 255) - 1] + [rng.getrandbits(256) for _ in range(500)])


# ------------------------------------------------------------------------------------------------ points
@functools.lru_cache(maxsize=None)
def affine_points():
    """12 affine points: G, 2G, (n - 1)G = -G, and kG for nine seeded k."""
    rng = random.Random(121)
    ks = [1, 2, N - 1] + [rng.randrange(1, N) for _ in range(9)]
    return tuple(o.scalar_mult(k, o.GX, o.GY) for k in ks)


@functools.lru_cache(maxsize=None)
def lambdas():
    """Z values for lifting: 1, p - 1, a patterned value and a random one."""
    rng = random.Random(122)
    pat = 0
    while pat == 0:
        pat = _pattern(rng, 8) % P
    return (1, P - 1, pat, rng.randrange(1, P))


def to_jac(pt, lam: int):
    x, y = pt
    return (x * lam * lam % P, y * pow(lam, 3, P) % P, lam)


def to_xz(pt, lam: int):
    x, y = pt
    zz, zzz = lam * lam % P, pow(lam, 3, P)
    return (x * zz % P, y * zzz % P, zz, zzz)


def neg(pt):
    return (pt[0], (P - pt[1]) % P)


def affine_add(p, q):
    """p + q on affine points (None = infinity) by the integer oracle."""
    jp = (p[0], p[1], 1) if p else (0, 1, 0)
    jq = (q[0], q[1], 1) if q else (0, 1, 0)
    return o._to_affine(o._jadd(jp, jq))


def jac_affine(X, Y, Z):
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * pow(zi, 3, P) % P)


def xz_affine(X, Y, ZZ, ZZZ):
    if ZZ % P == 0:
        return None
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


@functools.lru_cache(maxsize=None)
def point_pair_cases():
    """(label, P, lambda_P, Q, lambda_Q) with P, Q affine or None (infinity): generic sums of different points,
    P + P and P + (-P) under every pair of lifts, and the infinity cases. lambda None marks an infinity."""
    pts, lams = affine_points(), lambdas()
    cases = []
    for i, p in enumerate(pts):
        for j, q in enumerate(pts):
            if i != j:
                cases.append(('sum', p, lams[(i + j) % 4], q, lams[(3 * i + j + 1) % 4]))
    for p in pts:
        for la in lams:
            for lb in lams:
                cases.append(('double', p, la, p, lb))
                cases.append(('opposite', p, la, neg(p), lb))
    for i, p in enumerate(pts):
        for la in lams:
            cases.append(('inf+q', None, i % 2, p, la))
            cases.append(('p+inf', p, la, None, i % 2))
    cases += [('inf+inf', None, 0, None, 0), ('inf+inf', None, 1, None, 0), ('inf+inf', None, 1, None, 1)]
    return tuple(cases)


def infinity_jac(kind: int):
    """Two representations of infinity: the one jac_inf() returns and one with patterned X, Y."""
    return (1, 1, 0) if kind == 0 else (P - (1 << 96), (1 << 224) - 1, 0)


def infinity_xz(kind: int):
    return (1, 1, 0, 0) if kind == 0 else (P - (1 << 96), (1 << 224) - 1, 0, 0)
