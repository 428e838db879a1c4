"""``utxo_merkle_build`` / ``utxo_merkle_build_records`` / ``utxo_merkle_prove`` (csrc/utxo_merkle.hip: the Merkle
tree of the HBM table or of uploaded records, and the audit paths out of it), byte for byte against the hashlib
reference ``merkle_of`` / ``prove_of`` and against the host twin: live counts around the wave, the block and the
odd levels, a sparse 2^20-slot table, 65,537 entries, tombstones, a rehash, tag subsets, the hand-made sort cases,
the launch lever at one item per block, proofs of every leaf and of absent outpoints, and a snapshot that outlives
an asynchronous block apply."""
import numpy as np
import pytest

from state_digest_cases import arrays
from upow_amd.ledger.utxo import MerkleSnapshot, UtxoIndex, _GpuBackend, merkle_of, prove_of, records_merkle
from utxo_merkle_cases import (absent_outpoints, check_snapshot, outpoint, pool as make_pool, random_arrays,
                               sort_entries)

pytestmark = pytest.mark.gpu
TAGS = [(0,), (1, 2, 3, 4, 5, 6), None]
LEVERS = (0, 1)  # the default launch shape, and one item per block


def _pair(log2_cap):
    g = UtxoIndex(backend='gpu')
    g.be = _GpuBackend(log2_cap=log2_cap)
    return g, UtxoIndex(backend='host')


@pytest.fixture(scope='module')
def pool():
    """5,000 random entries (records, payloads), shared and never written."""
    return make_pool(5000, 72)


def some_queries(recs, step):
    return [outpoint(r) for r in recs[::step]] + absent_outpoints(recs)


def check_table(g, levers=LEVERS, tags=TAGS, step=1):
    """Every (tags, lever) build of g's table equals the reference on g's own dump, proofs included."""
    recs, pay = g.records_payload()
    for t in tags:
        keep = np.ones(len(recs), bool) if t is None else np.isin(recs[:, 36], t)
        for lever in levers:
            with g.merkle_snapshot(t, launch_lever=lever) as snap:
                assert snap.on_device or snap.count == 0
                check_snapshot(snap, recs[keep], pay[keep], some_queries(recs[keep], step))


@pytest.mark.parametrize('log2_cap', [8, 12])
@pytest.mark.parametrize('n', [0, 1, 2, 3, 5, 7, 63, 64, 65, 255, 256, 257])
def test_table_counts(gpu, pool, log2_cap, n):
    g, _ = _pair(log2_cap)
    recs, pay = pool
    g.insert_records(recs[:n], pay[:n])
    assert len(g) == n
    check_table(g, tags=[None], step=1 if n <= 65 else 29)
    with g.merkle_snapshot() as snap:
        assert (snap.root, snap.count) == merkle_of(recs[:n], pay[:n])


def test_sparse_table_and_host_parity(gpu, pool):
    g, h = _pair(20)
    recs, pay = pool
    for idx in (g, h):
        idx.insert_records(recs, pay)
    assert g.be.log2 == 20
    queries = some_queries(recs, 97)
    for t in TAGS:
        with g.merkle_snapshot(t) as a, h.merkle_snapshot(t) as b:
            assert (a.root, a.count, a.levels) == (b.root, b.count, b.levels) and a.on_device and not b.on_device
            assert a.prove(queries) == b.prove(queries)
    check_table(g, levers=(0,), tags=[None], step=97)


def test_65537_entries(gpu):
    """17 levels below the root, odd counts on several of them, more than one radix-sort tile."""
    recs, pay = random_arrays(65537, 5)
    queries = some_queries(recs, 4099)
    want_root, want_count = merkle_of(recs, pay)
    with records_merkle(recs, pay, device='gpu') as a, records_merkle(recs, pay, device='cpu') as b:
        assert (a.root, a.count) == (b.root, b.count) == (want_root, want_count)
        assert a.levels == b.levels == 18
        got = a.prove(queries)
        assert got == b.prove(queries) == prove_of(recs, pay, queries)
        assert max(len(p.leaves[0].path) for p in got) == 17
    g, _ = _pair(18)
    g.insert_records(recs, pay)
    with g.merkle_snapshot() as snap:
        assert (snap.root, snap.count) == (want_root, want_count) and snap.prove(queries) == got


def test_tombstones_rehash_and_payloadless(gpu, pool):
    g, h = _pair(12)
    recs, pay = pool
    for idx in (g, h):
        idx.insert_records(recs[:300], pay[:300])
        assert idx.erase_records(np.ascontiguousarray(recs[100:200])).all()
        idx.insert_records(recs[300:340], None)  # entries without payload: L = 0
    assert g.be.tombs == 100
    left = np.r_[0:100, 200:300]
    want_recs = np.concatenate([recs[left], recs[300:340]])
    want_pay = np.concatenate([pay[left], np.zeros(40, dtype=pay.dtype)])
    want = merkle_of(want_recs, want_pay)
    with h.merkle_snapshot() as snap:
        assert (snap.root, snap.count) == want
    for rehash in (None, 12, 13):
        if rehash:
            assert g.be.L.utxo_rehash(g.be.h, rehash) == (240, 0)
            g.be.tombs, g.be.log2 = 0, rehash
        check_table(g, step=31)
        with g.merkle_snapshot() as snap:
            assert (snap.root, snap.count) == want


def test_sort_cases(gpu):
    recs, pay = arrays(sort_entries())
    g, _ = _pair(8)
    g.insert_records(recs, pay)
    assert len(g) == len(recs) - 1  # the outpoint under two tags: the table holds one of them
    check_table(g)
    for lever in LEVERS:
        with records_merkle(recs, pay, device='gpu', launch_lever=lever) as snap:
            got = check_snapshot(snap, recs, pay)
        both = got[[outpoint(r) for r in recs].index(('ff' * 32, 9))]
        assert both.present and [x.entry[33] for x in both.leaves] == [0, 6]
        with records_merkle(recs, None, device='gpu', launch_lever=lever) as snap:
            check_snapshot(snap, recs, None)
    with pytest.raises(Exception):
        records_merkle(recs, pay, device='gpu', launch_lever=257)


@pytest.mark.parametrize('n', [1, 2, 3, 5, 7, 65])
def test_prove_every_leaf(gpu, pool, n):
    recs, pay = np.ascontiguousarray(pool[0][:n]), np.ascontiguousarray(pool[1][:n])
    for lever in LEVERS:
        with records_merkle(recs, pay, device='gpu', launch_lever=lever) as snap:
            got = check_snapshot(snap, recs, pay)
            assert all(p.present and len(p.leaves) == 1 for p in got[:n])
            assert sorted(p.leaves[0].position for p in got[:n]) == list(range(n))
            assert not any(p.present for p in got[n:])


@pytest.mark.parametrize('q', [0, 1, 64, 65, 1000])
def test_prove_query_counts(gpu, pool, q):
    """q queries in one call: live ones, duplicates of them, and absent ones before, between and after."""
    recs, pay = pool[0][:500], pool[1][:500]
    live = [outpoint(r) for r in recs]
    absent = absent_outpoints(recs)
    queries = [(live[(7 * k) % 300] if k % 3 else absent[k % len(absent)]) for k in range(q)]  # repeats past 300
    with records_merkle(recs, pay, device='gpu') as snap:
        got = snap.prove(queries)
        assert got == prove_of(recs, pay, queries) and len(got) == q
        if q >= 64:
            assert len({(h, i) for h, i in queries}) < q and {p.present for p in got} == {True, False}
            ends = {tuple(x.position for x in p.leaves) for p in got if not p.present}
            assert (0,) in ends and (499,) in ends and any(len(e) == 2 for e in ends)


def test_snapshot_outlives_apply_block(gpu, pool):
    """A snapshot taken before a block still proves the old state afterwards; one built while the block's
    asynchronous apply is still queued sees the new state (the collection runs behind it on the stream)."""
    g, _ = _pair(12)
    recs, pay = pool
    g.insert_records(recs[:400], pay[:400])
    old = g.merkle_snapshot()
    ins = [(np.ascontiguousarray(recs[400:520]), np.ascontiguousarray(pay[400:520])),
           (np.ascontiguousarray(recs[520:600]), np.ascontiguousarray(pay[520:600]))]
    spent = np.ascontiguousarray(recs[37:137])
    g.apply_block(ins, spent)
    assert g.be.pending is not None  # queued, not yet booked
    queued = MerkleSnapshot(g.be.L, g.be.L.utxo_merkle_build(g.be.h, 0x7f, 0))
    assert g.be.pending is not None
    new = g.merkle_snapshot()
    assert g.be.pending is None and g.duplicates == 0 and len(g) == 500
    keep = np.r_[0:37, 137:600]
    spent_q, created_q, kept_q = outpoint(recs[50]), outpoint(recs[450]), outpoint(recs[0])
    check_snapshot(old, recs[:400], pay[:400], [spent_q, created_q, kept_q])
    for snap in (queued, new):
        got = check_snapshot(snap, recs[keep], pay[keep], [spent_q, created_q, kept_q])
        assert [p.present for p in got] == [False, True, True]
    assert [p.present for p in old.prove([spent_q, created_q, kept_q])] == [True, False, True]
    for snap in (old, queued, new):
        snap.close()


def test_free_returns_the_bytes(gpu, pool):
    recs, pay = np.ascontiguousarray(pool[0][:1000]), np.ascontiguousarray(pool[1][:1000])
    n0, b0 = gpu.utxo_merkle_held()
    a = records_merkle(recs, pay, device='gpu')
    b = records_merkle(recs[:10], pay[:10], device='cpu')
    info = gpu.utxo_merkle_info(a._sid)
    assert info['on_device'] and info['bytes'] == a.nbytes and info['count'] == 1000 and info['levels'] == 11
    # 112 bytes a slot and fewer than 2 n + 32 nodes of 32 bytes, plus the level table and alignment
    assert 1000 * (112 + 32) < a.nbytes < 1000 * 112 + (2 * 1000 + 32) * 32 + 3 * 256
    assert gpu.utxo_merkle_held() == (n0 + 2, b0 + a.nbytes + b.nbytes)
    a.close()
    assert gpu.utxo_merkle_held() == (n0 + 1, b0 + b.nbytes)
    a.close()  # closing twice is nothing
    with b:
        pass
    assert gpu.utxo_merkle_held() == (n0, b0)
    with pytest.raises(ValueError):
        a.prove([outpoint(recs[0])])
    del a, b
    c = records_merkle(recs[:100], pay[:100], device='gpu')
    assert gpu.utxo_merkle_held()[0] == n0 + 1
    del c  # freed by __del__
    assert gpu.utxo_merkle_held() == (n0, b0)
