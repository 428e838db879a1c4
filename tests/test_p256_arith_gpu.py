"""P-256 field, scalar and point arithmetic at edge operands on the device: the checks of test_p256_arith.py
through the two device builds of the p256_probe hook: 'ilp' is a kernel of csrc/p256_probe.hip (the ILP-first
scheduler of the block-latency kernels), 'occ' one of csrc/p256_batch.hip (the default scheduler). The lane-group
operations (mul4, sqr4, dbl4, add4) run through QuadDev and OctDev, whose DPP broadcasts and pair split exist on
the device only; there every lane of a group returns all it holds, and every copy must equal the expectation.

As in the host file, expectations are Python integers. The probe checks what the arithmetic computes under each
file's device flags; it cannot prove that the copy inlined into a production kernel is the same machine code, so
the whole-signature device tests stay as they are.
"""
import random

import pytest

import p256_operands as po
from p256_operands import P
from test_p256_arith import (check_booth, check_fe_reduce, check_field_binary, check_field_unary, check_mul4_groups,
                             check_point_groups, check_points_one_lane, check_scalar_inverse, check_scalar_mul,
                             check_sqr4_groups, check_values, product_groups)

pytestmark = pytest.mark.gpu

MODES = ['ilp', 'occ']


@pytest.mark.parametrize('mode', MODES)
def test_field_binary_gpu(gpu, mode):
    check_field_binary(gpu, mode)


@pytest.mark.parametrize('mode', MODES)
def test_field_unary_gpu(gpu, mode):
    check_field_unary(gpu, mode)


@pytest.mark.parametrize('mode', MODES)
def test_fe_reduce_gpu(gpu, mode):
    check_fe_reduce(gpu, mode)


@pytest.mark.parametrize('mode', MODES)
def test_scalar_mul_gpu(gpu, mode):
    check_scalar_mul(gpu, mode)


@pytest.mark.parametrize('mode', MODES)
def test_scalar_inverse_gpu(gpu, mode):
    # one launch, shuffled: each wave mixes scalars that leave the divsteps loop after one or two rounds with
    # ones that need nearly all twenty
    check_scalar_inverse(gpu, mode, po.scalar_cases_shuffled())


@pytest.mark.parametrize('mode', MODES)
def test_booth_gpu(gpu, mode):
    check_booth(gpu, mode)


@pytest.mark.parametrize('mode', MODES)
def test_points_one_lane_gpu(gpu, mode):
    check_points_one_lane(gpu, mode)


@pytest.mark.parametrize('policy', ['quad', 'oct'])
def test_product_groups_gpu(gpu, policy):
    check_mul4_groups(gpu, 'ilp', policy)
    check_sqr4_groups(gpu, 'ilp', policy)


@pytest.mark.parametrize('policy', ['quad', 'oct'])
def test_point_groups_gpu(gpu, policy):
    check_point_groups(gpu, 'ilp', policy)


def _shape_pairs(n: int, per_wave: int, seed: int):
    """n random operand pairs with patterned ones first, last and in the middle of the final partial wave."""
    rng = random.Random(seed)
    pairs = [(rng.randrange(P), rng.randrange(P)) for _ in range(n)]
    pat = po.fe_patterned(6, seed)
    last_wave = per_wave * ((n - 1) // per_wave)
    for k, i in enumerate(sorted({0, n - 1, last_wave + (n - last_wave) // 2})):
        pairs[i] = (pat[2 * k] or 1, pat[2 * k + 1] or P - 1)
    return pairs


# a wave short of / at / past its 64 lanes, a 256-thread block likewise, several blocks with a tail
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_launch_shapes_one_lane(gpu, mode, n):
    pairs = _shape_pairs(n, 64, 2000 + n)
    check_values(gpu, 'fe_mul', mode, [a for a, _ in pairs], [b for _, b in pairs], [a * b % P for a, b in pairs])


# groups: one short of / at / past a wave (16 quads, 8 octets) and a four-wave block (64 quads, 32 octets)
@pytest.mark.parametrize('policy,groups', [('quad', g) for g in (1, 15, 16, 17, 63, 64, 65)]
                         + [('oct', g) for g in (1, 7, 8, 9, 31, 32, 33)])
def test_launch_shapes_groups(gpu, policy, groups):
    per_wave = 16 if policy == 'quad' else 8
    gs = product_groups(_shape_pairs(4 * groups, 4 * per_wave, 3000 + groups))[:groups]
    assert len(gs) == groups
    check_mul4_groups(gpu, 'ilp', policy, gs)
