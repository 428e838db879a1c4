"""The fused block verify (csrc/txcodec.cpp block_verify_fused, csrc/p256.hip p256_verify_fused_gpu) on the
crafted signatures of test_p256_edges, on key edges in every role, and at the launch shapes of its key kernel.

In production the verify items are not packed by the host: p256_keyrec_kernel decompresses each job's signer
key into item t and copies r | s | digest behind it, the threads past n_jobs curve-check every other address
of the block, and the verify kernels read the items that kernel wrote. _fused_cols turns 160-byte records
back into the block's columns (many jobs per key row, shared digest rows, every index column shuffled), so the
edge batch, its prefixes and its tilings run through that kernel at one block and at several, with the role
change at t == n_jobs inside a wave, with no jobs, with no addresses past the jobs, and past the quad limit.

The expectation is always the pure-integer oracle (upow_amd.utils.p256) or the edge batch's verdicts, which
are asserted against it where the batch is built. The host's fused path is a second check where it is run.
"""
import functools
import random

import numpy as np
import pytest

from upow_amd.utils import p256 as o

from test_p256 import _off_curve_x
from test_p256_edges import _decompress_edges, _edge_batch, _env, _mismatches, _pub, _tiled, _x_below_wrap

N = o.N


def _le(v: int) -> bytes:
    return v.to_bytes(32, 'little')


def _addr33(x: int, y: int) -> bytes:
    return bytes([42 + (y & 1)]) + _le(x)


def _rows64(addrs) -> np.ndarray:
    """33-byte addresses as the codec's 64-byte zero-padded rows."""
    a = np.zeros((len(addrs), 64), np.uint8)
    for i, ad in enumerate(addrs):
        assert len(ad) == 33
        a[i, :33] = np.frombuffer(ad, np.uint8)
    return a


def _identity(col) -> bool:
    return len(col) > 0 and bool((col == np.arange(len(col))).all())


def _fused_cols(recs, extra_in=(), outs=(), seed=0xF05ED):
    """The nine columns of block_verify_fused for the (n, 160) records `recs`.

    One pay row per distinct signer key (prefix 42 / 43 by the parity of y, x little-endian), shuffled with
    the check-only addresses `extra_in` among them, so job_input maps many jobs to one row. The signatures sit
    in a random permutation behind sig_ids, the distinct digests in a random order behind job_tx (records
    with one digest share its row), each table with one row of noise that no job refers to. No index column
    is the identity (asserted; job_input cannot help it when one job has one input). Reassembling
    pay[job_input] | sigs[sig_ids] | digest[job_tx] with the oracle's decompression gives `recs` again."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 160)
    n = len(recs)
    if n:
        keys, key_of = np.unique(recs[:, :64], axis=0, return_inverse=True)
        digs, dig_of = np.unique(recs[:, 128:], axis=0, return_inverse=True)
        key_of, dig_of = key_of.reshape(-1), dig_of.reshape(-1)
    else:
        keys, digs = np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8)
        key_of = dig_of = np.zeros(0, np.int64)
    num = lambda b: int.from_bytes(b.tobytes(), 'little')
    rows = _rows64([_addr33(num(k[:32]), num(k[32:])) for k in keys] + [bytes(a) for a in extra_in])
    n_in, n_dig = len(rows), len(digs)
    rng = np.random.default_rng(seed)
    for _ in range(64):
        perm = rng.permutation(n_in)
        pay = np.zeros((n_in, 64), np.uint8)
        pay[perm] = rows
        job_input = perm[key_of].astype(np.int64)
        sperm = rng.permutation(n + 1)
        sigs = rng.integers(0, 256, (n + 1, 64), dtype=np.uint8)
        sigs[sperm[:n]] = recs[:, 64:128]
        sig_ids = sperm[:n].astype(np.int64)
        dperm = rng.permutation(n_dig + 1)
        digest = rng.integers(0, 256, (n_dig + 1, 32), dtype=np.uint8)
        digest[dperm[:n_dig]] = digs
        job_tx = dperm[dig_of].astype(np.int64)
        if not (_identity(sig_ids) or _identity(job_tx) or (_identity(job_input) and (n > 1 or n_in > 1))):
            break
    else:
        raise AssertionError('no shuffle without an identity column')
    # the builder's own check: what the key kernel must make of these columns is `recs`
    xy = np.zeros((n_in, 64), np.uint8)
    for row in set(job_input.tolist()):
        x = int.from_bytes(pay[row, 1:33].tobytes(), 'little')
        y = o.x_to_y(x, pay[row, 0] == 43)
        assert pay[row, 0] in (42, 43) and not pay[row, 33:].any() and o.is_on_curve(x, y)
        xy[row] = np.frombuffer(_le(x) + _le(y), np.uint8)
    assert (np.concatenate([xy[job_input], sigs[sig_ids], digest[job_tx]], axis=1) == recs).all()
    out = _rows64([bytes(a) for a in outs])
    return (pay, np.full(n_in, 33, np.uint8), out, np.full(len(out), 33, np.uint8), job_input, sigs, sig_ids,
            digest, job_tx)


def _plant(cols, c, addr):
    """The columns with checked address c (pay rows first, then the new outputs) replaced by `addr`."""
    pay, out = cols[0].copy(), cols[2].copy()
    if c < len(pay):
        pay[c, :33] = np.frombuffer(addr, np.uint8)
    else:
        out[c - len(pay), :33] = np.frombuffer(addr, np.uint8)
    return (pay, cols[1], out) + tuple(cols[3:])


@functools.lru_cache(maxsize=None)
def _good_addrs(k, first=0):
    """k addresses of curve points that sign nothing in the edge batch."""
    pts = [_pub(0xC0FFEE + first + i) for i in range(k)]
    return tuple(_addr33(q.x, q.y) for q in pts)


def _bad_addr(k):
    """An address that is not a curve point: no point has this x (even k), or x = x0 + p for a point's x0."""
    if k % 2:
        return bytes([42 + (k // 2) % 2]) + _le(_x_below_wrap() + o.P)
    return bytes([42 + (k // 2) % 2]) + _le(_off_curve_x(random.Random(1000 + k)))


def _run(L, cols, gpu):
    code, st, ok, items = L.block_verify_fused(*cols, threads=4, gpu=gpu)
    assert code == 1 and isinstance(ok, bool)
    return (np.frombuffer(st, np.uint8), ok,
            None if items is None else np.frombuffer(items, np.uint8).reshape(-1, 160))


def _check(L, cols, recs, exp, gpu, all_ok=True, bad_rows=(), idx=None, what=None):
    """One call against the oracle's verdicts: statuses `exp`, except 2 for the jobs whose key row is in
    `bad_rows`; the all_ok flag; and the verify items, which come back exactly when a signature is invalid
    and are `recs`, with x = y = 0 for a bad key."""
    job_input = cols[4]
    bad = np.isin(job_input, list(bad_rows)) if len(bad_rows) else np.zeros(len(exp), bool)
    exp = np.where(bad, 2, exp).astype(np.uint8)
    st, ok, items = _run(L, cols, gpu)
    assert st.shape == exp.shape, what
    assert (st == exp).all(), (what, _mismatches(st, exp, idx))
    assert ok is all_ok, what
    if (exp == 0).any():
        want = np.array(recs, dtype=np.uint8).reshape(-1, 160)
        want[bad, :64] = 0
        assert items is not None and items.shape == want.shape, what
        rows = np.flatnonzero((items != want).any(axis=1))[:8].tolist()
        labels = _edge_batch()[2]
        assert not rows, (what, 'items differ', [(i, labels[i if idx is None else idx[i]]) for i in rows])
    else:
        assert items is None, what
    return st, ok, items


@functools.lru_cache(maxsize=None)
def _edge_cols():
    """The whole edge batch as one block: 16 signer keys among 21 inputs, 7 new outputs. Read-only."""
    cols = _fused_cols(_edge_batch()[0], extra_in=_good_addrs(5), outs=_good_addrs(7, first=5))
    for c in cols:
        c.setflags(write=False)
    return cols


# ------------------------------------------------------------------------------------- key edges, three roles

def _forged(x, y, rng):
    """A signature that verifies under the curve point (x, y) whose private key nobody knows: choose u1, u2,
    take R = u1 G + u2 Q, r = x(R) mod n, s = r / u2 and the digest e = u1 s. Returns r | s | e (96 bytes)."""
    while True:
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        pt = o.shamir(u1, u2, x, y)
        r = pt[0] % N if pt else 0
        if r:
            break
    s = r * pow(u2, -1, N) % N
    e = u1 * s % N
    assert o.verify_digest(r, s, e, x, y) is True
    return _le(r) + _le(s) + e.to_bytes(32, 'big')


@functools.lru_cache(maxsize=None)
def _edge_calls():
    """One block per (edge address, role): ('signer' | 'spent' | 'output', address, columns, records,
    expected statuses, expected all_ok, the edge job or None). The other jobs are valid signatures."""
    recs, exp, _ = _edge_batch()
    first_valid = lambda key: next(i for i in range(len(exp)) if exp[i] == 1 and (recs[i, :64] == key).all())
    valid = recs[[first_valid(key) for key in _lead_keys()]]  # six valid records, one per key
    assert len(np.unique(valid[:, :64], axis=0)) == 6
    rng = random.Random(0xED6E5)
    addrs, want = _decompress_edges()
    x0 = _x_below_wrap()
    assert sum(a[1:] == _le(x0 + o.P) for a in addrs) == 2
    stand_in = _pub(0x57A9D)  # signs in place of an edge address that is no point, then is overwritten by it
    calls = []
    for k, (addr, w) in enumerate(zip(addrs, want)):
        x = int.from_bytes(addr[1:], 'little')
        y = o.x_to_y(x, addr[0] == 43)
        on = o.is_on_curve(x, y)
        assert on == (w is not None) and (not on or w == (x, y))
        # signer: the edge job goes in the middle of the others
        q = (x, y) if on else (stand_in.x, stand_in.y)
        edge_rec = np.frombuffer(_le(q[0]) + _le(q[1]) + _forged(q[0], q[1], rng), np.uint8)
        jobs = np.concatenate([valid[:3], edge_rec[None], valid[3:]])
        cols = _fused_cols(jobs, extra_in=_good_addrs(2), outs=_good_addrs(3, first=2), seed=k)
        cols = _plant(cols, int(cols[4][3]), addr)  # same point, the edge's own prefix byte; or no point
        e = np.ones(7, np.uint8)
        e[3] = 1 if on else 2
        calls.append(('signer', addr, cols, jobs, e, on, 3))
        # a spent output's owner that signs nothing, and a new output
        g = _good_addrs(4)
        cols = _fused_cols(valid, extra_in=(g[0], addr, g[1]), outs=g[2:], seed=100 + k)
        calls.append(('spent', addr, cols, valid, np.ones(6, np.uint8), on, None))
        cols = _fused_cols(valid, extra_in=g[:2], outs=(g[2], addr, g[3]), seed=200 + k)
        calls.append(('output', addr, cols, valid, np.ones(6, np.uint8), on, None))
    return tuple(calls)


def _check_edge_calls(L, gpu):
    seen = set()
    for role, addr, cols, recs, exp, on, job in _edge_calls():
        what = (role, addr[0], hex(int.from_bytes(addr[1:], 'little')))
        st, ok, items = _run(L, cols, gpu)
        assert st.tolist() == exp.tolist(), what
        assert ok is on and items is None, what
        seen.add((role, on, addr[0] in (42, 43)))
    # every role met points and non-points, and points behind a foreign prefix byte
    kinds = ((True, True), (True, False), (False, True))
    assert seen == {(r, on, pre) for r in ('signer', 'spent', 'output') for on, pre in kinds}


# ------------------------------------------------------------------------------------------- launch shapes

# (n_jobs, n_in, n_out, blocks of the key kernel): n_jobs + n_in + n_out threads in blocks of 256. Up to, at
# and past one block and two; the role changes at thread n_jobs, inside a wave unless 64 divides it; no jobs;
# no addresses but the signers' own
_SHAPES = ((0, 0, 1, 1), (0, 0, 257, 2), (1, 1, 0, 1), (1, 1, 1, 1), (63, 5, 60, 1), (64, 16, 0, 1),
           (65, 16, 175, 1), (255, 16, 0, 2), (256, 16, 1, 2), (257, 3, 252, 2), (511, 16, 1, 3), (513, 16, 511, 5))


def _lead_keys():
    """The six keys of the edge batch's collision records (any leading run of 12 or more has them all), in
    the order of their first record."""
    head = _edge_batch()[0][:228, :64]
    keys, first = np.unique(head, axis=0, return_index=True)
    assert len(keys) == 6 and first.max() < 12
    return keys[np.argsort(first)]


@functools.lru_cache(maxsize=None)
def _shape_block(n_jobs, n_in, n_out):
    """(columns, records, expectations, batch index of each job): the first n_jobs records of the edge batch,
    of those signed by its first n_in keys where n_in is below the six that any leading run holds."""
    recs, exp, labels = _edge_batch()
    n_keys = min(n_in, 6) if n_jobs else 0
    mine = (recs[:, None, :64] == _lead_keys()[None, :n_keys]).all(axis=2).any(axis=1)
    sel = np.flatnonzero(mine)[:n_jobs]
    assert len(sel) == n_jobs and (n_in < 6 or (sel == np.arange(n_jobs)).all())
    assert n_jobs < n_keys or len(np.unique(recs[sel, :64], axis=0)) == n_keys
    cols = _fused_cols(recs[sel], extra_in=_good_addrs(n_in - n_keys), outs=_good_addrs(n_out, first=16),
                       seed=n_jobs * 1000 + n_out)
    assert len(cols[0]) == n_in and len(cols[2]) == n_out and len(cols[4]) == n_jobs
    return cols, recs[sel], exp[sel], sel


def test_shapes_are_where_they_should_be():
    assert sum(1 for nj, _, _, _ in _SHAPES if nj % 64) >= 3  # the role boundary is inside a wave
    for nj, n_in, n_out, blocks in _SHAPES:
        assert (nj + n_in + n_out + 255) // 256 == blocks, (nj, n_in, n_out)
    totals = {nj + n_in + n_out for nj, n_in, n_out, _ in _SHAPES}
    assert {256, 257, 512} <= totals and any(t > 512 for t in totals) and any(255 < t < 512 for t in totals)
    assert {0, 1, 255, 256, 257} <= {nj for nj, _, _, _ in _SHAPES}
    assert all(l.startswith(('quarter/', 'whole/')) for l in _edge_batch()[2][:228])


def _check_shape(L, gpu, n_jobs, n_in, n_out):
    cols, recs, exp, sel = _shape_block(n_jobs, n_in, n_out)
    shape = (n_jobs, n_in, n_out)
    got = _check(L, cols, recs, exp, gpu, idx=sel, what=shape)
    if gpu:  # second check: the host's fused path says the same, items included
        host = _run(L, cols, False)
        assert (got[0] == host[0]).all() and got[1] == host[1] and (got[2] is None) == (host[2] is None), shape
        assert got[2] is None or (got[2] == host[2]).all(), shape
    # an address that is no curve point at the ends of the inputs and of the new outputs: all_ok is False,
    # and the statuses change only for the jobs (if any) that sign with that very input
    n_c = n_in + n_out
    planted = sorted({c for c in (0, n_in - 1, n_in, n_c - 1) if 0 <= c < n_c})
    if n_jobs:  # the key rows of the first and the last job
        planted = sorted(set(planted) | {int(cols[4][0]), int(cols[4][-1])})
    for k, c in enumerate(planted):
        rows = [c] if c < n_in else []
        _check(L, _plant(cols, c, _bad_addr(k)), recs, exp, gpu, all_ok=False, bad_rows=rows, idx=sel,
               what=shape + (c,))


# ---------------------------------------------------------------------------------------------- CPU

def test_fused_cols_hold_what_they_claim():
    recs = _edge_batch()[0]
    pay, pay_len, out, out_len, job_input, sigs, sig_ids, digest, job_tx = _edge_cols()
    n = len(recs)
    assert pay.shape == (21, 64) and out.shape == (7, 64) and (pay_len == 33).all() and (out_len == 33).all()
    assert sigs.shape == (n + 1, 64) and len(job_input) == len(sig_ids) == len(job_tx) == n
    per_key = np.bincount(job_input, minlength=21)
    assert (per_key > 0).sum() == 16 and per_key[per_key > 0].min() >= 2  # many jobs to one key row
    assert sorted(np.bincount(sig_ids, minlength=n + 1).tolist()) == [0] + [1] * n
    per_dig = np.bincount(job_tx, minlength=len(digest))
    assert (per_dig == 0).sum() == 1 and len(digest) < n
    shared = np.flatnonzero(per_dig >= 2)
    assert len(shared) >= 2  # the digests 0 and n of the u1 = 0 records at the least
    for e in (0, N):
        row = np.flatnonzero((digest == np.frombuffer(e.to_bytes(32, 'big'), np.uint8)).all(axis=1))
        assert len(row) == 1 and per_dig[row[0]] >= 2
    assert not _identity(job_input) and not _identity(sig_ids) and not _identity(job_tx)
    # gathering by another index column would be noticed: the columns differ in most places
    assert (sig_ids != job_tx).mean() > 0.9 and (job_input != job_tx).mean() > 0.9


def test_edge_batch_fused_host(native):
    """Every crafted record through the host's fused stages: verdicts, all_ok, and the items byte for byte."""
    recs, exp, _ = _edge_batch()
    _check(native, _edge_cols(), recs, exp, False)


def test_key_edges_fused_host(native):
    """Each address of _decompress_edges (x >= p, x0 + p among them, no point at x, points behind every
    prefix byte) as a signer's key, as a spent output's owner that signs nothing, and as a new output."""
    _check_edge_calls(native, False)


@pytest.mark.parametrize('n_jobs, n_in, n_out', [s[:3] for s in _SHAPES])
def test_role_boundary_shapes_fused_host(native, n_jobs, n_in, n_out):
    """The GPU test's blocks on the host's fused stages: the gathers behind job_input, sig_ids and job_tx,
    the order of the checked addresses, and x = y = 0 in the item of a signer whose key is no point."""
    _check_shape(native, False, n_jobs, n_in, n_out)


# ---------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize('variant', [None, '4', '8', '1'])  # auto (quad at this size), quad, oct, one lane
def test_edge_batch_fused_gpu(gpu, variant, monkeypatch):
    """1,790 jobs, 7 blocks of the key kernel, then each verify family on the items it wrote. The item
    comparison checks the device's decompression of every signer key against the oracle-made records."""
    _env(monkeypatch, **({'VARIANT': variant} if variant else {}))
    recs, exp, _ = _edge_batch()
    got = _check(gpu, _edge_cols(), recs, exp, True, what=variant)
    if variant is None:
        host = _run(gpu, _edge_cols(), False)
        assert (got[0] == host[0]).all() and got[1] == host[1] and (got[2] == host[2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('n_jobs, n_in, n_out', [s[:3] for s in _SHAPES])
def test_role_boundary_shapes_fused_gpu(gpu, n_jobs, n_in, n_out, monkeypatch):
    """The key kernel's grid and its role change at thread n_jobs: all addresses good, then one address
    that is no point at each end of the inputs and of the outputs and under the first and the last job."""
    _env(monkeypatch)
    _check_shape(gpu, True, n_jobs, n_in, n_out)


@pytest.mark.gpu
def test_pooled_buffers_reused_fused_gpu(gpu, monkeypatch):
    """1,790 jobs, then 17 and 300 from other parts of the batch, then 1,640, 13 and 210, whose items fall in
    the pool's size classes of the first three (csrc/dev_pool.h) and so in their buffers: a key kernel that
    wrote too few items, or a verify that read past them, would give an earlier call's verdicts or items."""
    _env(monkeypatch)
    recs, exp, _ = _edge_batch()
    assert len(exp) == 1790
    _check(gpu, _edge_cols(), recs, exp, True, what=1790)
    anchor = next(i for i, l in enumerate(_edge_batch()[2]) if l.endswith('/inf'))  # where _tiled starts a tail
    before = {19: exp}
    for n, start in ((17, anchor), (300, 1200), (1640, 701), (13, 901), (210, 401)):
        idx = (np.arange(n) + start) % 1790
        r, e = recs[idx], exp[idx]
        cls = (160 * n - 1).bit_length()  # the pool's size class of the items: 2^cls bytes
        assert set(e.tolist()) == {0, 1} and (e != exp[:n]).any()
        if cls in before:  # these items lie in the buffer of that earlier, larger call
            assert len(before[cls]) > n and (e != before[cls][:n]).any()
        before[cls] = e
        cols = _fused_cols(r, extra_in=_good_addrs(3), outs=_good_addrs(2, first=3), seed=n)
        _check(gpu, cols, r, e, True, idx=idx, what=n)


@pytest.mark.gpu
@pytest.mark.parametrize('extra', [0, 37])  # the quad kernel's last size; the first of the one-lane kernel
def test_past_quad_limit_fused_gpu(gpu, extra, monkeypatch):
    """32 x 1024 jobs run the quad kernel behind the key kernel, 37 more the one-lane kernel of
    csrc/p256_batch.hip. Sixteen key rows serve all of them; the oracle's tile is the only expectation."""
    _env(monkeypatch)
    n = 32 * 1024 + extra
    recs, exp, idx = _tiled(n, 32 * 1024) if extra else _tiled(n, n - 37)
    cols = _fused_cols(recs, extra_in=_good_addrs(3), outs=_good_addrs(2, first=3), seed=n)
    assert len(cols[0]) == 19 and len(cols[4]) == n
    _check(gpu, cols, recs, exp, True, idx=idx, what=n)


@pytest.mark.gpu
def test_key_edges_fused_gpu(gpu, monkeypatch):
    """test_key_edges_fused_host's calls on the key kernel: in the two check-only roles its comparison of x
    with p is the only guard against x0 + p, no verify prologue runs behind it."""
    _env(monkeypatch)
    _check_edge_calls(gpu, True)
