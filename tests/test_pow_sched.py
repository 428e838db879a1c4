"""The PoW kernel variants with a pinned instruction order (csrc/pow_search.hip, pow_h0_sched) and the
dependency-distance audit that records the order (scripts/pow_dep_audit.py).

The reference throughout is hashlib over the same nonce words. The default kernel runs the same launch shapes,
so the cases stay covered whichever variants a build carries.
"""
import functools
import hashlib
import importlib.util
import os
import random
import struct

import pytest

from upow_amd.models.block import PowTarget, header_prefix
from upow_amd.ops.native import lib
from upow_amd.ops.pow import PowJob, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_SCHED_VARIANT = 6
SPLIT_LOG2 = 19  # 2,048 blocks x 256 threads, the default grid: where a lane / iteration split of the nonce word falls
COUNT = 1 << 18


def _variants():
    """The default kernel and every pinned-order variant of this build."""
    return [0] + list(range(FIRST_SCHED_VARIANT, lib().pow_variant_count()))


@functools.lru_cache(maxsize=None)
def _job(difficulty='2.0'):
    rng = random.Random(61)
    prev = hashlib.sha256(rng.randbytes(8)).hexdigest()
    pre = header_prefix(prev, 'DgQKikeDqS2Fzue23KuA36L4eJSFh649zA9jJ6zwbzUMp', hashlib.sha256(rng.randbytes(8)).hexdigest(),
                        1_790_000_061, difficulty)
    return PowJob.create(pre, PowTarget.from_difficulty(prev, difficulty))


def _digest(job, word):
    return hashlib.sha256(job.header[:-4] + struct.pack('>I', word)).digest()


@functools.lru_cache(maxsize=None)
def _brute_force(start, count):
    """Valid nonces of [start, start + count) (nonce words, wrapping at 2^32) by hashlib, shared by all variants."""
    job = _job()
    out = []
    for k in range(count):
        word = (start + k) & 0xffffffff
        if job.target.check_hex(_digest(job, word).hex()):
            out.append(job.word_to_nonce(word))
    return frozenset(out)


@pytest.mark.parametrize('variant', _variants())
def test_host_h0_matches_hashlib(variant):
    """The variant's device function compiled for the host gives hashlib's H0 (108-byte header: the pinned
    orders exist for it alone; the 138-byte kernel is untouched)."""
    L = lib()
    job = _job()
    rng = random.Random(variant)
    k = SPLIT_LOG2
    words = [0, 1, 0xffffffff, 0x80000000, (1 << k) - 1, 1 << k, (1 << k) + 1] + [rng.getrandbits(32) for _ in range(1000)]
    for word in words:
        want = struct.unpack('>I', _digest(job, word)[:4])[0]
        assert L.pow_job_h0_variant(job.header, word, variant) == want, (variant, hex(word))


# many iterations, many dispatches and a ragged tail: 4 blocks x 256 threads x 3 iterations per dispatch
@pytest.mark.gpu
@pytest.mark.parametrize('start', [0, (1 << 32) - (1 << 17), 12345])
@pytest.mark.parametrize('variant', _variants())
def test_variant_matches_hashlib(gpu, variant, start):
    want = _brute_force(start, COUNT)
    assert 800 < len(want) < 1250  # difficulty 2.0: one nonce in 256
    g = search(_job(), start, COUNT, device='gpu', grid_blocks=4, chunk_iters=3, variant=variant)
    assert g.searched == COUNT
    assert len(g.nonces) == len(set(g.nonces)) and set(g.nonces) == want, (variant, start)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', _variants())
def test_variant_power_of_two_grid(gpu, variant):
    """8 x 256 threads is a power of two and the start a multiple of it."""
    start = 1 << 20
    want = _brute_force(start, COUNT)
    g = search(_job(), start, COUNT, device='gpu', grid_blocks=8, chunk_iters=3, variant=variant)
    assert g.searched == COUNT
    assert len(g.nonces) == len(set(g.nonces)) and set(g.nonces) == want, variant


# ---- the audit script: distances and schedule leads of a loop written out by hand ----

def _audit():
    spec = importlib.util.spec_from_file_location('pow_dep_audit', os.path.join(ROOT, 'scripts', 'pow_dep_audit.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_ASM = """
_ZN4upow11pow_search_toyEv:
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, s4, v0
\ts_mov_b32 s0, 0x1234
\tv_alignbit_b32 v2, v1, v1, 6
\tv_alignbit_b32 v3, v1, v1, 11
\tv_lshrrev_b32_e32 v9, 3, v0
\tv_alignbit_b32 v4, v1, v1, 25
\tv_bitop3_b32 v5, v2, v3, v4 bitop3:0x96
\tv_add3_u32 v6, v5, s0, v9
\tv_add_u32_e32 v7, v6, v6
\ts_cbranch_execz .LBB0_1
.Lfunc_end0:
; NumVgprs: 10
; ScratchSize: 0
; Occupancy: 8
"""


def test_audit_distances():
    A = _audit()
    name, ins, scalar, res = A.loop_valu(_ASM, 'pow_search_toy')
    assert name == '_ZN4upow11pow_search_toyEv' and len(ins) == 8 and scalar == 1
    assert res == {'NumVgprs': 10, 'ScratchSize': 0, 'Occupancy': 8}
    d = [x for x, _ in A.distances(ins)]
    # v1 has no producer in the loop; the rotates sit 1, 2 and 4 behind it (a shift of v0 in between); the XOR3
    # follows its last rotate; the add3 the XOR3 (and the shift, 3 back); the last add the add3
    assert d == [None, 1, 2, None, 4, 1, 1, 1]
    text = A.report(_ASM, 'pow_search_toy')
    assert 'at distance 1: 4   at distance 2: 1' in text
    assert 'longest run of consecutively dependent instructions: 4' in text
    assert 'first round in the loop: 63' in text  # one Sigma1 group: it is numbered as the last round
