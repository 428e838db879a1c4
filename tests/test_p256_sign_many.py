"""Batched P-256 key derivation and RFC 6979 signing: the kernels' shared core (csrc/p256_sign.h) on host
threads against the separate host signer (p256_sign / p256_pubkey), the Python oracle and the RFC's vectors."""
import functools
import hashlib
import hmac
import json
import random

import numpy as np
import pytest

from upow_amd.ops import p256 as op
from upow_amd.utils import p256 as o

from test_p256 import RFC6979_D

N = o.N
# RFC 6979 A.2.5, P-256 with SHA-256: message -> (k, r, s)
RFC_VECTORS = {
    b'sample': (0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
                0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
                0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8),
    b'test': (0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0,
              0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
              0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083),
}
# 1, 2, n-2, n-1; a single non-zero 16-bit window (lowest of its limb, highest, straddling none); no zero window
EDGE_KEYS = [1, 2, N - 2, N - 1, 1 << 16, 1 << 240, 0xffff << 112, (1 << 256) // 3]
INVALID_KEYS = [0, N, N + 1, (1 << 256) - 1]
# bits2octets reduces the last three (>= n)
EDGE_DIGESTS = [bytes(32), N.to_bytes(32, 'big'), (N - 1).to_bytes(32, 'big'), (N + 1).to_bytes(32, 'big'),
                b'\xff' * 32]


def be(d: int) -> bytes:
    return d.to_bytes(32, 'big')


def rs_le(r: int, s: int) -> bytes:
    return r.to_bytes(32, 'little') + s.to_bytes(32, 'little')


def random_pairs(count: int, seed: int):
    rng = random.Random(seed)
    return [rng.randrange(1, N) for _ in range(count)], [rng.randbytes(32) for _ in range(count)]


def drbg_candidates(d: int, digest: bytes, count: int) -> bytes:
    """RFC 6979 section 3.2 with every candidate rejected: steps b-g, then step h `count` times."""
    seed = be(d) + be(int.from_bytes(digest, 'big') % N)
    mac = lambda k, m: hmac.new(k, m, hashlib.sha256).digest()
    K, V = bytes(32), b'\x01' * 32
    for sep in (b'\x00', b'\x01'):
        K = mac(K, V + sep + seed)
        V = mac(K, V)
    out = []
    for _ in range(count):
        V = mac(K, V)
        out.append(V)
        K = mac(K, V + b'\x00')
        V = mac(K, V)
    return b''.join(out)


def candidate_cases():
    keys, digests = random_pairs(4, 77)
    return [(RFC6979_D, hashlib.sha256(b'sample').digest())] + list(zip(keys, digests))


@functools.lru_cache(maxsize=None)
def host_reference(native, keys_be: bytes, digests: bytes):
    """(p256_sign_batch, p256_pubkey_batch) of the separate host signer, computed once per input."""
    return native.p256_sign_batch(keys_be, digests, 8), native.p256_pubkey_batch(keys_be, 8)


def check_known_answers(native, gpu: bool):
    for msg, (k, r, s) in RFC_VECTORS.items():
        digest = hashlib.sha256(msg).digest()
        assert native.p256_sign_many(be(RFC6979_D), digest, gpu) == rs_le(r, s), msg
        assert native.p256_rfc6979_candidates(be(RFC6979_D), digest, 1, gpu) == be(k), msg
    q = native.p256_pubkey_many(be(RFC6979_D), gpu)
    assert int.from_bytes(q[:32], 'little') == 0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6
    assert int.from_bytes(q[32:], 'little') == 0x7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299


def check_edge_keys(native, gpu: bool):
    keys = b''.join(be(d) for d in EDGE_KEYS)
    digests = b''.join(hashlib.sha256(be(d)).digest() for d in EDGE_KEYS)
    sig, pub = host_reference(native, keys, digests)
    assert native.p256_sign_many(keys, digests, gpu) == sig
    assert native.p256_pubkey_many(keys, gpu) == pub
    assert all(any(pub[64 * i:64 * i + 64]) and any(sig[64 * i:64 * i + 64]) for i in range(len(EDGE_KEYS)))


def check_invalid_keys(native, gpu: bool):
    """Each invalid key between valid neighbours: its row is zero, theirs are what they are without it."""
    good, good_dig = random_pairs(len(INVALID_KEYS) + 1, 5)
    mixed = [good[0]]
    for bad, d in zip(INVALID_KEYS, good[1:]):
        mixed += [bad, d]
    keys = b''.join(be(d) for d in mixed)
    digests = b''.join(hashlib.sha256(bytes([i])).digest() if i % 2 else good_dig[i // 2] for i in range(len(mixed)))
    sig = np.frombuffer(native.p256_sign_many(keys, digests, gpu), dtype=np.uint8).reshape(-1, 64)
    pub = np.frombuffer(native.p256_pubkey_many(keys, gpu), dtype=np.uint8).reshape(-1, 64)
    ref_sig, ref_pub = host_reference(native, b''.join(be(d) for d in good), b''.join(good_dig))
    assert not sig[1::2].any() and not pub[1::2].any()
    assert sig[0::2].tobytes() == ref_sig and pub[0::2].tobytes() == ref_pub


def check_edge_digests(native, gpu: bool):
    keys = b''.join(be(d) for d in (RFC6979_D, 1, N - 1, (1 << 256) // 3, 0xffff << 112))
    digests = b''.join(EDGE_DIGESTS)
    assert native.p256_sign_many(keys, digests, gpu) == host_reference(native, keys, digests)[0]


def check_candidates(native, gpu: bool):
    for d, digest in candidate_cases():
        assert native.p256_rfc6979_candidates(be(d), digest, 3, gpu) == drbg_candidates(d, digest, 3)


def test_known_answers(native):
    check_known_answers(native, False)
    # the published nonce and signature of "test" against the pure-Python signer
    k, r, s = RFC_VECTORS[b'test']
    assert o.rfc6979_nonce(RFC6979_D, hashlib.sha256(b'test').digest()) == k
    assert o.sign(b'test', RFC6979_D) == (r, s)


def test_edge_keys(native):
    check_edge_keys(native, False)


def test_invalid_keys(native):
    check_invalid_keys(native, False)
    for bad in INVALID_KEYS:
        keys = [5, 6, bad, 7]
        for call in (lambda: op.public_keys(keys, device='cpu'),
                     lambda: op.sign_digests(keys, [bytes(32)] * 4, device='cpu'),
                     lambda: op.sign_records(keys, [bytes(32)] * 4, device='cpu')):
            with pytest.raises(ValueError, match='private key 2 out of range'):
                call()


def test_edge_digests(native):
    check_edge_digests(native, False)


def test_random_differential(native):
    keys, digests = random_pairs(2000, 11)
    kb, db = b''.join(be(d) for d in keys), b''.join(digests)
    ref_sig, ref_pub = host_reference(native, kb, db)
    sig, pub = native.p256_sign_many(kb, db, False), native.p256_pubkey_many(kb, False)
    assert sig == ref_sig
    assert pub == ref_pub
    for i in range(32):
        q = o.get_public_key(keys[i])
        assert pub[64 * i:64 * i + 64] == q.x.to_bytes(32, 'little') + q.y.to_bytes(32, 'little')
        k = o.rfc6979_nonce(keys[i], digests[i])
        r = o.scalar_mult(k, o.GX, o.GY)[0] % N
        s = pow(k, -1, N) * (int.from_bytes(digests[i], 'big') + r * keys[i]) % N
        assert sig[64 * i:64 * i + 64] == rs_le(r, s)


def test_front_end_matches_bindings(native):
    keys, digests = random_pairs(70, 12)
    kb, db = b''.join(be(d) for d in keys), b''.join(digests)
    ref_sig, ref_pub = host_reference(native, kb, db)
    assert op.sign_digests(keys, digests, device='cpu').tobytes() == ref_sig
    assert op.public_keys(keys, device='cpu').tobytes() == ref_pub
    with pytest.raises(ValueError):
        op.sign_digests(keys, digests[:-1], device='cpu')
    with pytest.raises(ValueError):
        op.sign_digests(keys[:1], [b'short'], device='cpu')


def test_closed_loop(native):
    keys, digests = random_pairs(300, 13)
    recs = op.sign_records(keys + EDGE_KEYS, digests + EDGE_DIGESTS + EDGE_DIGESTS[:3], device='cpu')
    assert recs.shape == (308, 160)
    assert (op.verify_records(recs, device='cpu') == op.VALID).all()


def test_candidates(native):
    check_candidates(native, False)
    assert native.p256_rfc6979_candidates(be(1), bytes(32), 0, False) == b''
    with pytest.raises(ValueError):
        native.p256_rfc6979_candidates(be(1), bytes(32), 65, False)


def test_empty_batch(native):
    assert native.p256_sign_many(b'', b'', False) == b''
    assert native.p256_pubkey_many(b'', False) == b''
    assert op.public_keys([], device='cpu').shape == (0, 64)
    assert op.sign_digests([], [], device='cpu').shape == (0, 64)
    assert op.sign_records([], [], device='cpu').shape == (0, 160)


def test_default_dispatch_stays_on_host_below_threshold(native, monkeypatch):
    monkeypatch.delenv('UPOW_P256_SIGN_GPU_MIN', raising=False)
    assert not op._sign_on_gpu(op.SIGN_GPU_MIN - 1, None)
    assert op._sign_on_gpu(1, 'gpu') and not op._sign_on_gpu(1 << 20, 'cpu')
    with pytest.raises(ValueError):
        op._sign_on_gpu(1, 'tpu')


def test_sign_batch_tool(native, tmp_path, capsys):
    from upow_amd import tools
    keys, digests = random_pairs(6, 14)
    keys[4] = N
    (tmp_path / 'k').write_bytes(b''.join(be(d) for d in keys))
    (tmp_path / 'd').write_bytes(b''.join(digests))
    argv = ['sign-batch', '--keys', str(tmp_path / 'k'), '--digests', str(tmp_path / 'd'), '--out', str(tmp_path / 'o'),
            '--device', 'cpu']
    assert tools.main(argv) == 1  # one key out of range
    printed = capsys.readouterr().out
    res = json.loads(printed)
    assert (res['signatures'], res['failed'], res['first_failed'], res['device']) == (5, 1, 4, 'cpu')
    out = (tmp_path / 'o').read_bytes()
    good = [i for i in range(6) if i != 4]
    ref = host_reference(native, b''.join(be(keys[i]) for i in good), b''.join(digests[i] for i in good))[0]
    assert out[:256] == ref[:256] and out[256:320] == bytes(64) and out[320:] == ref[256:]
    assert not any(be(d).hex() in printed for d in keys)  # the key file is never echoed
    (tmp_path / 'd').write_bytes(b'short')
    with pytest.raises(SystemExit):
        tools.main(argv)
