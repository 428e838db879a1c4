"""P-256 verify on crafted signatures and launch shapes that random inputs never reach.

Random signatures meet the special branches of the point formulas (P == Q, P == -Q, infinity in the middle
of a chain) with probability ~2^-256, and a digest >= n with probability 2^-32. Whoever knows the private
key d can aim at them: for any (u1, u2, d) the record with Q = dG, k = u1 + u2 d, r = x(kG) mod n,
s = r / u2 and e = u1 s makes the verifier compute exactly that u1*G + u2*Q. The batch built here puts the
accumulator of every GPU path onto +-(the next G part), onto infinity, through e >= n, and through the
extreme Booth digits of u2; the launch-shape tests then run it at the wave boundaries, with partial waves,
sliced launches and the large-batch split of the dispatcher (csrc/p256.hip verify_launch).

The expectation is always the pure-integer oracle (upow_amd.utils.p256), never another native path.
"""
import functools
import random

import numpy as np
import pytest

from upow_amd.ops import p256 as op
from upow_amd.utils import p256 as o

from test_p256 import _off_curve_x, _x_below_wrap

N = o.N
M64 = (1 << 64) - 1
_ENV = ('UPOW_P256_VARIANT', 'UPOW_P256_SPW', 'UPOW_P256_SLICE', 'UPOW_P256_TAIL', 'UPOW_P256_HOST32')


def _env(monkeypatch, **kw):
    """Exactly the given UPOW_P256_* settings (keys without the prefix), every other one unset."""
    for name in _ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv('UPOW_P256_' + k, str(v))


@functools.lru_cache(maxsize=None)
def _pub(d: int):
    return o.get_public_key(d)


def _quarters(u1: int):
    """u1 as the quad and oct kernels split it: P_q = bits [64 q, 64 q + 64) of u1, in place."""
    return [((u1 >> (64 * q)) & M64) << (64 * q) for q in range(4)]


class _Batch:
    def __init__(self):
        self.recs, self.exp, self.labels = [], [], []
        self.rng = random.Random(0x9256ED6E)

    def emit(self, label, q, r, s, e, want):
        """One record, its expectation checked against the oracle."""
        assert 1 <= r <= N and 1 <= s <= N and 0 <= e < 1 << 256, label
        assert o.verify_digest(r, s, e, q.x, q.y) == bool(want), label
        self.recs.append(op.record(q, (r, s), e.to_bytes(32, 'big')))
        self.exp.append(want)
        self.labels.append(label)

    def emit_with_bad_copy(self, label, q, r, s, e):
        """A valid record, followed by the same with s + 1 (s - 1 at the top), which must not verify."""
        self.emit(label, q, r, s, e, 1)
        self.emit(label + '/bad-s', q, r, s + 1 if s + 1 < N else s - 1, e, 0)

    def craft(self, label, u1, u2, d):
        """The record that makes the verifier compute u1*G + u2*(dG): valid unless that sum is infinity.
        Emitted again with digest e + n where that fits 256 bits. Returns k = u1 + u2 d mod n."""
        assert 0 <= u1 < N and 1 <= u2 < N and 1 <= d < N, label
        q = _pub(d)
        k = (u1 + u2 * d) % N
        r = _pub(k).x % N if k else self.rng.randrange(1, N)
        assert r, label
        s = r * pow(u2, -1, N) % N
        e = u1 * s % N
        w = pow(s, -1, N)
        assert e * w % N == u1 and r * w % N == u2, label  # what verify_prologue will derive
        for dig, lab in ((e, label), (e + N, label + '/e+n')):
            if dig >= 1 << 256:
                continue
            if k:
                self.emit_with_bad_copy(lab, q, r, s, dig)
            else:
                self.emit(lab + '/inf', q, r, s, dig, 0)
        return k


# u2 shapes for the signed 5-bit windows (BoothW5): leading windows all zero, digits +-16 (the last table
# entry), carries that run through the whole chain, and the values next to n
_STRUCTURED_U2 = ([1, 2, 15, 16, 17, 31, 32, 33]
                  + [(1 << 64) - 1, 1 << 64, (1 << 200) - 1, 1 << 255]
                  + [N - 1, N - 2, N - 16, N - 17]
                  + [int('10000' * 51, 2), int('01111' * 51, 2)]
                  + [((1 << 256) // 31) % N])


@functools.lru_cache(maxsize=None)
def _edge_batch():
    """(records as an (n, 160) uint8 array, expected statuses, labels); built once, read-only.

    Ordered case-major and key-minor: the first 12 records already hold a doubling collision for every
    key, and the first 257 every quarter and whole-sum collision (the prefixes the launch-shape tests run)."""
    b = _Batch()
    rng = b.rng
    keys = [1, 2, N - 1, (N + 1) // 2, rng.randrange(1, N), rng.randrange(1, N)]
    inv = {d: pow(d, -1, N) for d in keys}

    # --- quarter collisions (quad and oct kernels). These follow the current schedule of
    # verify_quad_core: u1*G is added to u2*Q in four quarters of 64 bits, in the order 0 to 3. Before
    # quarter q is added the accumulator is (pre_q + u2 d) G with pre_q = P_0 + .. + P_{q-1}; u2 is chosen
    # so that this is +P_q G (add4 must double) or -P_q G (add4 must pass through infinity, and the
    # signature still verifies unless q was the last non-zero quarter).
    edge_win = (3, 4, 7, 8, 11, 12)  # per key: a 16-bit window just below / above a quarter boundary
    shapes = [('full', (0, 1, 2, 3), [rng.randrange(1 << 255, N) for _ in keys]),
              ('top0', (0, 1, 2), [rng.randrange(1 << 191, 1 << 192) for _ in keys]),
              ('only2', (2,), [rng.randrange(1, 1 << 64) << 128 for _ in keys]),
              ('only0', (0,), [rng.randrange(1, 1 << 64) for _ in keys]),
              ('window', None, [rng.randrange(1, 1 << 16) << (16 * w) for w in edge_win])]
    for name, nonzero, u1s in shapes:
        for q in range(4):
            for sign in (1, -1):
                for ki, d in enumerate(keys):
                    u1 = u1s[ki]
                    P = _quarters(u1)
                    mine = nonzero or (edge_win[ki] // 4,)
                    assert sum(P) == u1 and tuple(j for j in range(4) if P[j]) == mine, name
                    if q not in mine:
                        continue
                    pre = sum(P[:q])
                    u2 = (sign * P[q] - pre) * inv[d] % N
                    label = 'quarter/%s/q%d%s/key%d' % (name, q, '+' if sign > 0 else '-', ki)
                    assert (pre + u2 * d - sign * P[q]) % N == 0 and P[q] % N, label
                    k = b.craft(label, u1, u2, d)
                    if sign > 0:
                        assert k == (2 * P[q] + sum(P[q + 1:])) % N and k, label
                    else:
                        assert k == sum(P[q + 1:]) % N and (k == 0) == (q == mine[-1]), label

    # --- whole-sum collisions (one-lane kernel): its last step is jac_add(u1*G, u2*Q)
    for ki, d in enumerate(keys):
        u1 = rng.randrange(1, N)
        u2 = u1 * inv[d] % N
        assert (u2 * d - u1) % N == 0
        assert b.craft('whole/+/key%d' % ki, u1, u2, d) == 2 * u1 % N
        u2 = (N - u1) * inv[d] % N
        assert (u2 * d + u1) % N == 0
        assert b.craft('whole/-/key%d' % ki, u1, u2, d) == 0

    # --- u1 = 0: every G part is infinity; reached through e = 0 and, by craft's second record, e = n
    for ki, d in enumerate(keys):
        for u2 in (rng.randrange(1, N), rng.randrange(1, N), 31):
            n0 = len(b.exp)
            b.craft('u1zero/key%d' % ki, 0, u2, d)
            digs = [int.from_bytes(r[128:], 'big') for r in b.recs[n0:]]
            assert digs == [0, 0, N, N]

    # --- u1 with a single non-zero 16-bit window: one G-table read, three quarters at infinity
    for j in range(16):
        for bits in (1, 0x00ff, 0x0100, 0xffff):
            for ki, d in enumerate(keys):
                u1 = bits << (16 * j)
                assert u1 < N and [w for w in range(16) if (u1 >> (16 * w)) & 0xffff] == [j]
                b.craft('window/%d/%04x/key%d' % (j, bits, ki), u1, rng.randrange(1, N), d)

    # --- structured u2, with a random u1 and with u1 = 0
    for u2 in _STRUCTURED_U2:
        assert 1 <= u2 < N
        for ki, d in enumerate(keys):
            b.craft('u2/%x/key%d' % (u2, ki), rng.randrange(1, N), u2, d)
            b.craft('u2/%x/u1zero/key%d' % (u2, ki), 0, u2, d)

    # --- chosen s with a digest in [n, 2^256): solve for the key, as test_p256._chosen_s_batch does. With
    # the e + n records above these are what runs the prologue's sc_reduce of e
    for s in [1, 2, 3, N - 1, N - 2, (N + 1) // 2, 1 << 255, 0xffffffff, rng.randrange(1, N), rng.randrange(1, N)]:
        k = rng.randrange(1, N)
        r = _pub(k).x % N
        e = rng.randrange(N, 1 << 256)
        d = (s * k - e) * pow(r, -1, N) % N
        assert e >= N and d and (e + r * d - s * k) % N == 0
        b.emit_with_bad_copy('chosen-s/e>=n', _pub(d), r, s, e)

    # --- r = n and s = n pass the range check (fastecdsa raises only for r > n) and never verify. r = n is
    # u2 = 0, the whole u2*Q chain at infinity; with e = 0 as well, so is every G part
    for ki, d in enumerate(keys):
        b.emit('range/r=n/key%d' % ki, _pub(d), N, rng.randrange(1, N), rng.randrange(1 << 256), 0)
        b.emit('range/r=n/e=0/key%d' % ki, _pub(d), N, rng.randrange(1, N), 0, 0)
        b.emit('range/s=n/key%d' % ki, _pub(d), rng.randrange(1, N), N, rng.randrange(1 << 256), 0)

    recs = np.frombuffer(b''.join(b.recs), dtype=np.uint8).reshape(-1, 160)
    exp = np.array(b.exp, dtype=np.uint8)
    recs.setflags(write=False)
    exp.setflags(write=False)
    return recs, exp, tuple(b.labels)


def _tiled(n, tail_at):
    """The edge batch repeated to n records, rolled so that the launch that starts at record `tail_at` (a
    slice, or the remainder of the large-batch split) starts at the batch's first infinity record: that
    launch then runs the quarter collisions, and its expectations are an aperiodic run of 0s and 1s that
    the launches before it do not have at the same place. Returns (records, expectations, batch index of
    each record); asserts that a launch at a lost or shifted offset could not give these expectations."""
    recs, exp, labels = _edge_batch()
    anchor = next(i for i, l in enumerate(labels) if l.endswith('/inf'))
    idx = (np.arange(n) + (anchor - tail_at)) % len(exp)
    rem = n - tail_at
    tail = idx[tail_at:].tolist()
    assert sum(labels[i].startswith('quarter/') for i in tail) >= min(rem, 30)
    assert sum(labels[i].endswith('/inf') for i in tail) >= 6
    e = exp[idx]
    for other in (0, tail_at - rem, tail_at - 1, tail_at - 2, tail_at - 16, tail_at - 64):
        assert 0 <= other < other + rem <= n and (e[other:other + rem] != e[tail_at:]).any(), other
    return recs[idx], e, idx


def _mismatches(got, exp, idx=None):
    labels = _edge_batch()[2]
    bad = np.flatnonzero(got != exp)[:8].tolist()
    return [(i, labels[i if idx is None else idx[i]], int(got[i]), int(exp[i])) for i in bad]


def _check(recs, exp, device, idx=None):
    got = op.verify_records(recs, device=device, threads=4)
    assert got.shape == exp.shape
    assert (got == exp).all(), _mismatches(got, exp, idx)


# ---------------------------------------------------------------------------------------------- CPU

def test_edge_batch_covers_its_cases():
    """The crafted batch holds what it is meant to hold (each record's own congruence and oracle verdict
    are asserted where it is built): every kind for all six keys, digests >= n, both verdicts."""
    recs, exp, labels = _edge_batch()
    assert len(exp) == len(labels) == recs.shape[0]
    count = lambda pre, suf='': sum(1 for l in labels if l.startswith(pre) and l.endswith(suf))
    # per key: 4 + 3 + 1 + 1 + 1 non-zero quarters, both signs; '-' at the last quarter is infinity
    assert count('quarter/') == 6 * (2 * 2 * 10 - 5) and count('quarter/', '/inf') == 6 * 5
    assert count('whole/+') == 12 and count('whole/-') == 6
    # the launch-shape tests run prefixes: the collisions come first
    assert all(l.startswith(('quarter/', 'whole/')) for l in labels[:228]) and 'key5' in labels[11]
    assert count('u1zero/') == 6 * 3 * 4
    assert count('window/') == 16 * 4 * 6 * 2
    assert count('u2/') == len(_STRUCTURED_U2) * 6 * (2 + 4)
    assert count('chosen-s/') == 20
    high = sum(1 for r in recs if int.from_bytes(r[128:].tobytes(), 'big') >= N)
    assert high >= 20 + 6 * 3 * 2 + len(_STRUCTURED_U2) * 6 * 2
    assert sorted(set(exp.tolist())) == [0, 1]
    assert count('range/') == 18
    # every valid record has its bad copy; 36 records are at infinity and 18 have r = n or s = n
    assert int((exp == 1).sum()) == (len(exp) - 36 - 18) // 2


@pytest.mark.parametrize('mode', [None, '1', 'quad', 'oct'])  # 64-bit host verifier; the GPU kernels' code on the host
def test_edge_batch_host(native, mode, monkeypatch):
    _env(monkeypatch, **({'HOST32': mode} if mode else {}))
    recs, exp, _ = _edge_batch()
    _check(recs, exp, 'cpu')


@pytest.mark.parametrize('n, tail_at', [(2 * 1024 + 37, 2 * 1024)] + [(k * cus * 1024 + rem, k * cus * 1024)
                                                                       for cus in (64, 128, 240, 256)
                                                                       for k, rem in ((1, 37), (2, 83))])
def test_tiled_tail_is_distinct(n, tail_at):
    """The batches of the sliced and the split launches, at the slice size and at several CU counts: the
    last launch holds quarter collisions and infinities, and its expectations differ from those at the
    offsets a wrong launch would read or write (asserted in _tiled), so the GPU tests can see one."""
    recs, exp, idx = _tiled(n, tail_at)
    assert recs.shape == (n, 160) and exp.shape == idx.shape == (n,)
    assert idx[tail_at] == idx[tail_at - 1] + 1 and set(exp[tail_at:tail_at + 6].tolist()) == {0}


def _decompress_edges():
    """33-byte addresses at the edges of the field and of the prefix byte, with the oracle's answer."""
    rng = random.Random(77)
    rows = [(42, 0), (43, 0)]
    rows += [(pre, x) for x in (o.P - 1, o.P, o.P + 1, (1 << 256) - 1) for pre in (42, 43)]
    x0 = _x_below_wrap()
    assert o.is_on_curve(x0, o.x_to_y(x0)) and o.P <= x0 + o.P < 1 << 256
    rows += [(42, x0 + o.P), (43, x0 + o.P)]
    rows += [(42 + (k & 1), _off_curve_x(rng)) for k in range(3)]
    for _ in range(4):
        q = _pub(rng.randrange(1, N))
        rows += [(42, q.x), (43, q.x)]
        # any other prefix byte is read as "even" (a[0] == 43 is the only test): pinned against x_to_y(x, False)
        rows += [(pre, q.x) for pre in (0, 41, 44, 255)]
    addrs, want = [], []
    for pre, x in rows:
        y = o.x_to_y(x, pre == 43)
        addrs.append(bytes([pre]) + x.to_bytes(32, 'little'))
        want.append((x, y) if o.is_on_curve(x, y) else None)
    assert all(w is None for (_, x), w in zip(rows, want) if x >= o.P)
    assert sum(w is None for w in want) >= 9 and sum(w is not None for w in want) >= 24
    return addrs, want


def test_decompress_edges_host(native):
    addrs, want = _decompress_edges()
    assert op.decompress(addrs, device='cpu') == want


# ---------------------------------------------------------------------------------------------- GPU

_WAVE_SIZES = (1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['0', '1', '2', '3', '5', '4', '8', 'a'])
def test_edge_batch_gpu(gpu, variant, monkeypatch):
    """Every kernel variant: one lane per signature ('0' '1' '2' '3' '5'), quad '4', oct '8', auto 'a'."""
    _env(monkeypatch, VARIANT=variant)
    recs, exp, _ = _edge_batch()
    _check(recs, exp, 'gpu')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['4', '8', '1', '3'])  # 16, 8, 64 and 4 x 64 signatures per wave / workgroup
def test_wave_boundary_sizes_gpu(gpu, variant, monkeypatch):
    _env(monkeypatch, VARIANT=variant)
    recs, exp, _ = _edge_batch()
    got = op.verify_records(recs[:0], device='gpu')
    assert got.dtype == np.uint8 and got.shape == (0,)
    for n in _WAVE_SIZES:
        got = op.verify_records(recs[:n], device='gpu')
        assert got.shape == (n,) and (got == exp[:n]).all(), (n, _mismatches(got, exp[:n]))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['1', '3'])
@pytest.mark.parametrize('spw', [1, 16, 63])
def test_partial_waves_gpu(gpu, variant, spw, monkeypatch):
    """UPOW_P256_SPW signatures per 64-lane wave: the idle lanes and the item index of the rest."""
    _env(monkeypatch, VARIANT=variant, SPW=spw)
    recs, exp, _ = _edge_batch()
    _check(recs[:300], exp[:300], 'gpu')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['1', '2'])  # per-lane and dword-major window tables
def test_sliced_launches_gpu(gpu, variant, monkeypatch):
    """Three launches (1024 + 1024 + 37) over one reused window-table scratch."""
    _env(monkeypatch, VARIANT=variant, SLICE=1024)
    recs, exp, idx = _tiled(2 * 1024 + 37, 2 * 1024)
    assert (exp[1024:2048] != exp[:1024]).any()
    _check(recs, exp, 'gpu', idx)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [None, 'a'])
@pytest.mark.parametrize('shape', ['round+37', '2round+83'])
def test_auto_split_gpu(gpu, variant, shape, monkeypatch):
    """The production path of a large batch: whole rounds of CUs x 1024 signatures on the one-lane kernel,
    the remainder on the quad kernel at its offset into the items and the statuses."""
    import torch
    _env(monkeypatch, **({'VARIANT': variant} if variant else {}))
    rnd = torch.cuda.get_device_properties(0).multi_processor_count * 1024
    n = rnd + 37 if shape == 'round+37' else 2 * rnd + 16 * 5 + 3
    if n > 600_000:
        pytest.skip('%d CUs put the split at %d signatures; this test stays below 600,000' % (rnd // 1024, n))
    recs, exp, idx = _tiled(n, n // rnd * rnd)
    _check(recs, exp, 'gpu', idx)


@pytest.mark.gpu
def test_decompress_edges_gpu(gpu):
    addrs, want = _decompress_edges()
    assert op.decompress(addrs, device='gpu') == want
