"""Batched P-256 key derivation and RFC 6979 signing on the device (csrc/p256_sign.hip) against the host
signer: the cases of test_p256_sign_many.py with gpu=True, launch shapes with lanes retiring early inside live
waves, the sign -> verify round trip and the front end's dispatch."""
import random

import numpy as np
import pytest

from upow_amd.ops import p256 as op

from test_p256_sign_many import (INVALID_KEYS, N, be, check_candidates, check_edge_digests, check_edge_keys,
                                 check_invalid_keys, check_known_answers, host_reference, random_pairs)

pytestmark = pytest.mark.gpu


def test_known_answers_gpu(gpu):
    check_known_answers(gpu, True)


def test_edge_keys_gpu(gpu):
    check_edge_keys(gpu, True)


def test_invalid_keys_gpu(gpu):
    check_invalid_keys(gpu, True)
    with pytest.raises(ValueError, match='private key 1 out of range'):
        op.sign_digests([5, N, 7], [bytes(32)] * 3, device='gpu')


def test_edge_digests_gpu(gpu):
    check_edge_digests(gpu, True)


def test_candidates_gpu(gpu):
    check_candidates(gpu, True)


# one lane, a wave short of / at / past its 64 lanes, a 256-thread block likewise, several blocks with a tail
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_launch_shapes(gpu, n):
    keys, digests = random_pairs(n, 1000 + n)
    rng = random.Random(n)
    # invalid keys at both ends and in the middle of a wave: their lanes retire while the neighbours run on
    for i in {0, n - 1, n // 2 if n < 64 else 64 * ((n - 1) // 128) + 29}:
        keys[i] = rng.choice(INVALID_KEYS)
    kb, db = b''.join(be(d) for d in keys), b''.join(digests)
    ref_sig, ref_pub = host_reference(gpu, kb, db)
    sig, pub = gpu.p256_sign_many(kb, db, True), gpu.p256_pubkey_many(kb, True)
    assert len(sig) == len(pub) == 64 * n
    assert sig == ref_sig
    assert pub == ref_pub


def test_round_trip_on_device(gpu):
    keys, digests = random_pairs(4096, 21)
    assert len(set(keys)) == 4096
    recs = op.sign_records(keys, digests, device='gpu')
    assert (op.verify_records(recs, device='gpu') == op.VALID).all()
    flipped = recs.copy()
    rng = random.Random(22)
    for row in flipped:
        bit = rng.randrange(256)
        row[128 + bit // 8] ^= 1 << (bit % 8)
    assert (op.verify_records(flipped, device='gpu') == op.INVALID).all()


def test_dispatch_threshold(gpu, monkeypatch):
    monkeypatch.setenv('UPOW_P256_SIGN_GPU_MIN', '8')
    calls = []
    real = gpu.p256_sign_many
    monkeypatch.setattr(op, 'lib', lambda: _Spy(gpu, lambda *a: (calls.append(a[2]), real(*a))[1]))
    for n in (16, 4):
        keys, digests = random_pairs(n, 30 + n)
        ref = host_reference(gpu, b''.join(be(d) for d in keys), b''.join(digests))[0]
        assert op.sign_digests(keys, digests).tobytes() == ref
    assert calls == [True, False]  # 16 items went to the device, 4 stayed on the host


class _Spy:
    """The native module with p256_sign_many wrapped, to see which device the front end chose."""

    def __init__(self, native, sign_many):
        self._native, self.p256_sign_many = native, sign_many

    def __getattr__(self, name):
        return getattr(self._native, name)
