"""P-256 field, scalar and point arithmetic at edge operands: every function the signature kernels are built from
(csrc/p256_field.h, the pair-split product and the lane-group step schedule of csrc/p256_steps.h, the signer's
madd_window) run one item at a time through the p256_probe hook and compared with Python integers.

This file runs the host compile (mode 'host'; the lane-group operations through QuadHost and OctHost).
test_p256_arith_gpu.py runs the same check_* functions through the two device builds.

What the probe can and cannot show: it checks what the arithmetic computes under each file's compiler flags. It
cannot prove that the copy of a function inlined into a production kernel is the same machine code, so the
whole-signature tests (test_p256.py, test_p256_edges.py, test_p256_fused_edges.py) stay as they are.

Expectations are always Python integers, never another native mode.
"""
import functools
import random

import pytest

import p256_operands as po
from p256_operands import N, P, R

R_INV = pow(R, -1, N)
LANES = {'quad': 4, 'oct': 8}


# ------------------------------------------------------------------------------------------------ plumbing
def le(v: int, nbytes: int = 32) -> bytes:
    return v.to_bytes(nbytes, 'little')


def pack(vals, nbytes: int = 32) -> bytes:
    """Items to flat little-endian bytes; an item is an int or a tuple of ints (a point's coordinates)."""
    return b''.join(le(v, nbytes) if isinstance(v, int) else b''.join(le(c) for c in v) for v in vals)


def hexs(v) -> str:
    if v is None:
        return 'inf'
    return hex(v) if isinstance(v, int) else '(' + ', '.join(hex(c) for c in v) + ')'


def run(native, op: str, mode: str, a, b=None, a_bytes: int = 32):
    """One probe call over all items; the result cut into one bytes object per item (on the device a lane-group
    operation's item holds every lane's copy)."""
    if b is not None:
        assert len(b) == len(a)
    out = native.p256_probe(op, pack(a, a_bytes), pack(b) if b is not None else b'', mode)
    assert len(a) > 0 and len(out) % len(a) == 0, (op, mode, len(out), len(a))
    k = len(out) // len(a)
    return [out[k * i:k * (i + 1)] for i in range(len(a))]


def ints(raw: bytes):
    return [int.from_bytes(raw[i:i + 32], 'little') for i in range(0, len(raw), 32)]


def check_values(native, op: str, mode: str, a, b, expect, a_bytes: int = 32):
    """op over (a[i], b[i]) must give the integer expect[i]."""
    got = run(native, op, mode, a, b, a_bytes)
    for i, (g, e) in enumerate(zip(got, expect)):
        assert len(g) == 32
        if int.from_bytes(g, 'little') != e:
            raise AssertionError('%s [%s] item %d: a=%s b=%s got %s expected %s' % (
                op, mode, i, hexs(a[i]), hexs(b[i]) if b is not None else '-', hex(int.from_bytes(g, 'little')), hex(e)))


# ------------------------------------------------------------------------------------------------ field
def check_field_binary(native, mode: str):
    """fe_mul and the pair-split product (mul_pair_host: split_rows on both halves, combine_rows) against a*b mod p
    on canonical and unreduced pairs; fe_add and fe_sub on canonical pairs."""
    pairs = list(po.field_pairs())
    wide = pairs + list(po.field_pairs_unreduced()) + list(CARRY_REGRESSIONS)
    a, b = [x for x, _ in wide], [y for _, y in wide]
    prod = [x * y % P for x, y in wide]
    check_values(native, 'fe_mul', mode, a, b, prod)
    check_values(native, 'mul_pair', mode, a, b, prod)
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    check_values(native, 'fe_add', mode, a, b, [(x + y) % P for x, y in pairs])
    check_values(native, 'fe_sub', mode, a, b, [(x - y) % P for x, y in pairs])


# Pairs whose pair-split product carries out of column 11 through columns 12..15 of combine_rows: the lower rows'
# column 11 is all ones and the upper rows' columns 8..11 (hi[4..7]) too, so the carry runs to the top.
CARRY_REGRESSIONS = (((1 << 256) - 1, (1 << 256) - 1), ((1 << 256) - 1, (1 << 128) - 1), ((1 << 128) - 1, (1 << 256) - 1),
                     (P - 1, P - 1), ((1 << 256) - (1 << 128), (1 << 256) - 1))


def check_field_unary(native, mode: str):
    """fe_sqr (canonical and unreduced), fe_neg with 0 -> 0, fe_inv with 0 -> 0, and the square-root candidate
    a^((p+1)/4) exactly, on residues and non-residues."""
    vals = list(po.field_singles())
    sq = vals + list(po.fe_unreduced())
    check_values(native, 'fe_sqr', mode, sq, None, [v * v % P for v in sq])
    assert vals[0] == 0  # fe_neg(0) must be 0, not p
    check_values(native, 'fe_neg', mode, vals, None, [(P - v) % P for v in vals])
    inv = list(po.FE_EDGE) + po.fe_patterned(300, 131) + po.fe_random(300, 132)
    check_values(native, 'fe_inv', mode, inv, None, [pow(v, P - 2, P) for v in inv])
    roots = [pow(v, (P + 1) // 4, P) for v in inv]
    residue = [r * r % P == v for r, v in zip(roots, inv)]
    assert residue.count(True) > 100 and residue.count(False) > 100
    check_values(native, 'fe_sqrt_candidate', mode, inv, None, roots)


def check_fe_reduce(native, mode: str):
    """The Solinas reduction of 512-bit values: the 4,000 of the host test (overflow T from -4 to 4) and the two
    inputs that put the Solinas sum at its extremes."""
    cs = list(po.reduce_cases()) + [po.solinas_extreme(1), po.solinas_extreme(-1), 0, (1 << 512) - 1]
    check_values(native, 'fe_reduce', mode, cs, None, [c % P for c in cs], a_bytes=64)


# ------------------------------------------------------------------------------------------------ scalars
def check_scalar_mul(native, mode: str):
    """Montgomery products mod n (a*b*R^-1), into and out of the Montgomery domain, and sc_reduce on [0, 2^256)."""
    pairs = list(po.scalar_pairs())
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    check_values(native, 'sc_mont_mul', mode, a, b, [x * y * R_INV % N for x, y in pairs])
    check_values(native, 'sc_to_mont', mode, a, None, [x * R % N for x in a])
    check_values(native, 'sc_from_mont', mode, a, None, [x * R_INV % N for x in a])
    red = list(po.scalar_reduce_cases())
    assert sum(v >= N for v in red) > 300
    check_values(native, 'sc_reduce', mode, red, None, [v % N for v in red])


def check_scalar_inverse(native, mode: str, cases=None):
    """s^-1 * R mod n by divsteps, one call over the whole list (on the device: one launch, shuffled, so a wave's
    lanes leave the loop at different rounds)."""
    cases = list(po.scalar_cases() if cases is None else cases)
    check_values(native, 'sc_inv_safegcd_mont', mode, cases, None, [pow(s, -1, N) * R % N for s in cases])


def check_booth(native, mode: str):
    """BoothW5: 52 digits in [-16, 16], digit w stored as int8 at byte w, with sum d_w 32^w = k."""
    ks = list(po.booth_cases())
    for k, raw in zip(ks, run(native, 'booth_w5', mode, ks)):
        assert len(raw) == 52
        digits = [d - 256 if d > 127 else d for d in raw]
        assert all(-16 <= d <= 16 for d in digits), 'booth_w5 [%s] k=%s digits %s' % (mode, hex(k), digits)
        assert sum(d << (5 * w) for w, d in enumerate(digits)) == k, 'booth_w5 [%s] k=%s digits %s' % (mode, hex(k), digits)


# ------------------------------------------------------------------------------------------------ points
def _lift(pt, lam, lift, infinity):
    return infinity(lam) if pt is None else lift(pt, lam)


def _same_point(op, mode, label, operands, got_affine, expect):
    if got_affine != expect:
        raise AssertionError('%s [%s] %s: operands %s got %s expected %s' % (
            op, mode, label, ' '.join(hexs(x) for x in operands), hexs(got_affine), hexs(expect)))


def check_points_one_lane(native, mode: str):
    """jac_dbl, jac_add, jac_madd, madd_window, jac_to_aff and jac_to_xz on lifted points (Z = 1, p - 1, patterned,
    random), compared as affine points; a result has Z = 0 exactly when the sum is infinity."""
    cases = po.point_pair_cases()
    pa = [_lift(p, lp, po.to_jac, po.infinity_jac) for _, p, lp, _, _ in cases]
    qa = [_lift(q, lq, po.to_jac, po.infinity_jac) for _, _, _, q, lq in cases]
    for (label, p, _, q, _), x, y, raw in zip(cases, pa, qa, run(native, 'jac_add', mode, pa, qa, 96)):
        _same_point('jac_add', mode, label, (x, y), po.jac_affine(*ints(raw)), po.affine_add(p, q))
    # doubling: every operand of the list above, infinity included
    for (label, p, _, _, _), x, raw in zip(cases, pa, run(native, 'jac_dbl', mode, pa, None, 96)):
        _same_point('jac_dbl', mode, label, (x,), po.jac_affine(*ints(raw)), po.affine_add(p, p))
    # mixed addition: the second operand affine, so never infinity
    mixed = [(c, x) for c, x in zip(cases, pa) if c[3] is not None]
    ja, qb = [x for _, x in mixed], [c[3] for c, _ in mixed]
    for ((label, p, _, q, _), x), raw in zip(mixed, run(native, 'jac_madd', mode, ja, qb, 96)):
        _same_point('jac_madd', mode, label, (x, q), po.jac_affine(*ints(raw)), po.affine_add(p, q))
    # madd_window: p = infinity gives q with `bad` clear; p = +-q sets `bad`; anything else adds and leaves it clear
    seen = set()
    for ((label, p, _, q, _), x), raw in zip(mixed, run(native, 'madd_window', mode, ja, qb, 96)):
        assert len(raw) == 100
        bad = int.from_bytes(raw[96:], 'little')
        want_bad = p is not None and p[0] == q[0]
        assert bad == int(want_bad), 'madd_window [%s] %s: operands %s %s bad=%d' % (mode, label, hexs(x), hexs(q), bad)
        seen.add((p is None, want_bad))
        if not want_bad:
            _same_point('madd_window', mode, label, (x, q), po.jac_affine(*ints(raw[:96])), po.affine_add(p, q))
    assert seen == {(True, False), (False, True), (False, False)}
    for (label, p, _, _, _), x, raw in zip(cases, pa, run(native, 'jac_to_aff', mode, pa, None, 96)):
        assert len(raw) == 68
        ok, xy = int.from_bytes(raw[:4], 'little'), tuple(ints(raw[4:]))
        _same_point('jac_to_aff', mode, label, (x,), xy if ok else None, p)
        assert ok in (0, 1) and (ok or xy == (0, 0))
    for (label, p, _, _, _), x, raw in zip(cases, pa, run(native, 'jac_to_xz', mode, pa, None, 96)):
        X, Y, ZZ, ZZZ = ints(raw)
        assert (ZZ, ZZZ) == (x[2] * x[2] % P, pow(x[2], 3, P)), 'jac_to_xz [%s] %s: operand %s' % (mode, label, hexs(x))
        _same_point('jac_to_xz', mode, label, (x,), po.xz_affine(X, Y, ZZ, ZZZ), p)


# ------------------------------------------------------------------------------------------------ lane groups
def group_copies(op: str, mode: str, policy: str, raw: bytes, operands):
    """The copies of one group's 128-byte result: one on the host, one per lane on the device. Per-lane agreement:
    every lane of the group must hold the same four values, so what a DPP broadcast or the pair split's row
    shifts delivered to lanes 1..3 and to the upper quad is compared, not only what lane 0 saw."""
    want = 128 * (1 if mode == 'host' else LANES[policy])
    assert len(raw) == want, (op, mode, len(raw), want)
    copies = [raw[k:k + 128] for k in range(0, len(raw), 128)]
    for lane, c in enumerate(copies):
        if c != copies[0]:
            raise AssertionError('%s_%s [%s]: lane %d holds %s, lane 0 holds %s; operands %s' % (
                policy, op, mode, lane, hexs(tuple(ints(c))), hexs(tuple(ints(copies[0]))),
                ' '.join(hexs(x) for x in operands)))
    return tuple(ints(copies[0]))


def product_groups(pairs):
    """Operand pairs in groups of four whose four products differ pairwise (a value broadcast from the wrong lane
    then cannot equal the expected one); pairs that collide wait for a later group, the last group is filled up."""
    rng = random.Random(141)
    groups, cur, waiting = [], [], []
    def fits(pr):
        return all(pr[0] * pr[1] % P != x * y % P for x, y in cur)
    for pr in pairs:
        for w in [w for w in waiting if fits(w)][:1]:
            waiting.remove(w)
            cur.append(w)
        if len(cur) < 4 and fits(pr):
            cur.append(pr)
        else:
            waiting.append(pr)
        if len(cur) == 4:
            groups.append(tuple(cur))
            cur = []
    while waiting or cur:
        for w in [w for w in waiting if fits(w)][:1]:
            waiting.remove(w)
            cur.append(w)
        while len(cur) < 4 and not any(fits(w) for w in waiting):
            pr = (rng.randrange(P), rng.randrange(P))
            if fits(pr):
                cur.append(pr)
        if len(cur) == 4:
            groups.append(tuple(cur))
            cur = []
    return groups


@functools.lru_cache(maxsize=None)
def mul4_groups():
    pairs = list(po.field_pairs())[::2] + list(po.field_pairs_unreduced()) + list(CARRY_REGRESSIONS)
    groups = product_groups(pairs)
    assert all(len({x * y % P for x, y in g}) == 4 for g in groups)
    return tuple(groups)


@functools.lru_cache(maxsize=None)
def sqr4_groups():
    vals = list(dict.fromkeys(list(po.field_singles()) + list(po.fe_unreduced())))
    groups = product_groups([(v, v) for v in vals])
    return tuple(tuple(x for x, _ in g) for g in groups)


def check_mul4_groups(native, mode: str, policy: str, groups=None):
    """mul4 over groups of four distinct operand pairs: every lane's four results equal the four products."""
    groups = list(mul4_groups() if groups is None else groups)
    a = [tuple(x for x, _ in g) for g in groups]
    b = [tuple(y for _, y in g) for g in groups]
    for g, raw in zip(groups, run(native, policy + '_mul4', mode, a, b, 128)):
        got = group_copies('mul4', mode, policy, raw, g)
        if got != tuple(x * y % P for x, y in g):
            raise AssertionError('%s_mul4 [%s]: operands %s got %s' % (policy, mode, ' '.join(hexs(x) for x in g), hexs(got)))


def check_sqr4_groups(native, mode: str, policy: str):
    groups = list(sqr4_groups())
    for g, raw in zip(groups, run(native, policy + '_sqr4', mode, groups, None, 128)):
        got = group_copies('sqr4', mode, policy, raw, g)
        if got != tuple(x * x % P for x in g):
            raise AssertionError('%s_sqr4 [%s]: operands %s got %s' % (policy, mode, hexs(g), hexs(got)))


def check_point_groups(native, mode: str, policy: str):
    """dbl4 and add4 on XYZZ points with ZZ != 1: add4 of P + P must double, P + (-P) must give ZZ = 0, infinity
    on either side returns the other operand, and doubling infinity stays infinity."""
    cases = po.point_pair_cases()
    pa = [_lift(p, lp, po.to_xz, po.infinity_xz) for _, p, lp, _, _ in cases]
    qa = [_lift(q, lq, po.to_xz, po.infinity_xz) for _, _, _, q, lq in cases]
    for (label, p, _, q, _), x, y, raw in zip(cases, pa, qa, run(native, policy + '_add4', mode, pa, qa, 128)):
        got = group_copies('add4', mode, policy, raw, (x, y))
        _same_point(policy + '_add4', mode, label, (x, y), po.xz_affine(*got), po.affine_add(p, q))
    for (label, p, _, _, _), x, raw in zip(cases, pa, run(native, policy + '_dbl4', mode, pa, None, 128)):
        got = group_copies('dbl4', mode, policy, raw, (x,))
        _same_point(policy + '_dbl4', mode, label, (x,), po.xz_affine(*got), po.affine_add(p, p))


# ------------------------------------------------------------------------------------------------ host tests
def test_operand_sets():
    """The sets hold what the issue lists, and the 512-bit set drives the Solinas overflow T to every value it
    can take: the extremes of the sum are -4 and 4 (solinas_extreme), and all of -4..4 occur."""
    assert len(po.FE_EDGE) == 34 and all(0 <= v < P for v in po.FE_EDGE)
    assert len(po.field_pairs()) == 34 * 34 + 2100
    assert len(po.reduce_cases()) == 4000
    ts = {po.solinas_overflow(c) for c in po.reduce_cases()}
    assert ts == set(range(-4, 5)), sorted(ts)
    assert po.solinas_overflow(po.solinas_extreme(1)) == 4 and po.solinas_overflow(po.solinas_extreme(-1)) == -4
    for c in po.reduce_cases()[:200]:  # the restated rows are the reduction: s1 + 2 s2 + ... == c (mod p)
        s = po.solinas_sums(c)
        assert (s[0] + 2 * s[1] + 2 * s[2] + s[3] + s[4] - s[5] - s[6] - s[7] - s[8] - c) % P == 0
    assert all(1 <= s < N for s in po.scalar_cases()) and len(po.scalar_cases()) > 4400
    assert {N - 1, N - 2, R, po.R2, 1, 1 << 255} <= set(po.scalar_cases())
    assert sorted(po.scalar_cases_shuffled()) == sorted(po.scalar_cases())
    assert po.scalar_cases_shuffled() != po.scalar_cases()
    pts = po.affine_points()
    assert len(pts) == len(set(pts)) == 12 and all(po.o.is_on_curve(*pt) for pt in pts)
    assert pts[2] == po.neg(pts[0])


def test_probe_argument_checks(native):
    one = le(1)
    with pytest.raises(ValueError, match='unknown op'):
        native.p256_probe('fe_cube', one, one, 'host')
    with pytest.raises(ValueError, match='unknown op'):
        native.p256_probe('mul4', one * 4, one * 4, 'host')  # a lane-group operation needs its policy
    with pytest.raises(ValueError, match='unknown op'):
        native.p256_probe('quad_fe_mul', one, one, 'host')
    for mode in ('gpu', '', 'HOST'):
        with pytest.raises(ValueError, match='unknown mode'):
            native.p256_probe('fe_mul', one, one, mode)
    # lengths are checked before anything is launched, so the device modes raise without a device too
    for mode in ('host', 'ilp', 'occ'):
        with pytest.raises(ValueError, match='whole number of items'):
            native.p256_probe('fe_mul', one + b'\0', one, mode)
        with pytest.raises(ValueError, match='does not match'):
            native.p256_probe('fe_mul', one * 2, one, mode)
        with pytest.raises(ValueError, match='does not match'):
            native.p256_probe('fe_sqr', one, one, mode)
        with pytest.raises(ValueError, match='whole number of items'):
            native.p256_probe('fe_reduce', one, b'', mode)
        assert native.p256_probe('fe_mul', b'', b'', mode) == b''  # empty: no launch
    with pytest.raises(ValueError, match='host and ilp'):
        native.p256_probe('oct_mul4', one * 4, one * 4, 'occ')
    with pytest.raises(ValueError, match='host only'):
        native.p256_probe('sc_inv_mont', one, b'', 'ilp')
    assert native.p256_probe('quad_mul4', b'', b'', 'ilp') == b''


def test_field_binary_host(native):
    check_field_binary(native, 'host')


def test_field_unary_host(native):
    check_field_unary(native, 'host')


def test_fe_reduce_host(native):
    check_fe_reduce(native, 'host')


def test_scalar_mul_host(native):
    check_scalar_mul(native, 'host')


def test_scalar_inverse_host(native):
    check_scalar_inverse(native, 'host')
    check_scalar_inverse(native, 'host', po.scalar_cases_shuffled()[:500])


def test_scalar_inverse_other_algorithms_host(native):
    """The binary-Euclid inverse of the A/B build and the host signer's Fermat chain (Montgomery form in and out)."""
    cases = list(po.scalar_cases())[::8]
    want = [pow(s, -1, N) * R % N for s in cases]
    check_values(native, 'sc_inv_bgcd_mont', 'host', cases, None, want)
    check_values(native, 'sc_inv_mont', 'host', [s * R % N for s in cases], None, want)


def test_booth_host(native):
    check_booth(native, 'host')


def test_points_one_lane_host(native):
    check_points_one_lane(native, 'host')


@pytest.mark.parametrize('policy', ['quad', 'oct'])
def test_product_groups_host(native, policy):
    check_mul4_groups(native, 'host', policy)
    check_sqr4_groups(native, 'host', policy)


@pytest.mark.parametrize('policy', ['quad', 'oct'])
def test_point_groups_host(native, policy):
    check_point_groups(native, 'host', policy)
