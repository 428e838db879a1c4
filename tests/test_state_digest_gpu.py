"""``utxo_state_digest`` and ``utxo_records_digest`` (csrc/utxo_digest.hip: the state digest of the HBM table and
of uploaded records) on small tables, byte for byte against the hashlib reference ``state_digest_of``: live counts
around the 64-entry queue, the wave and the block, a sparse 2^20-slot table, tombstones, a rehash, tag subsets, a
one-block grid, and the additive rule across a real asynchronous block apply."""
import numpy as np
import pytest

from state_digest_cases import C_NOISE, ENTRY, KNOWN, arrays, check_known, random_entries
from upow_amd.ledger.utxo import StateDigest, UtxoIndex, _GpuBackend, records_digest, state_digest_of

pytestmark = pytest.mark.gpu
TAGS = [(0,), (1, 2, 3, 4, 5, 6), None]


def _pair(log2_cap):
    """The HBM table at 2^log2_cap slots and the host table (as tests/test_owner_totals_gpu.py builds them)."""
    g = UtxoIndex(backend='gpu')
    g.be = _GpuBackend(log2_cap=log2_cap)
    return g, UtxoIndex(backend='host')


@pytest.fixture(scope='module')
def pool():
    """5,000 random entries (records, payloads), shared and never written."""
    recs, pay = arrays(random_entries(5000, 72))
    recs.setflags(write=False)
    pay.setflags(write=False)
    return recs, pay


def check_table(g, grids=(0, 1), tags=TAGS):
    """Every (tags, grid) pass over g's table equals the reference on g's own dump; returns the full digest."""
    recs, pay = g.records_payload()
    for t in tags:
        keep = np.ones(len(recs), bool) if t is None else np.isin(recs[:, 36], t)
        want = state_digest_of(recs[keep], pay[keep])
        for grid in grids:
            got = g.state_digest(t, grid_blocks=grid)
            assert got.tobytes() == want.tobytes() and got.count == want.count == int(keep.sum())
            assert got.hex() == want.hex()
    return g.state_digest()


@pytest.mark.parametrize('log2_cap', [8, 12])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 257])
def test_table_counts(gpu, pool, log2_cap, n):
    """0, 1, 63, 64, 65, 257 live entries: an empty pass, a lone tail batch, one short of a full batch, exactly
    one, one over, and more than a block's lanes (the 2^8-slot table has grown by then: it holds at most 128)."""
    g, _ = _pair(log2_cap)
    recs, pay = pool
    g.insert_records(recs[:n], pay[:n])
    assert len(g) == n and (g.be.log2 == log2_cap or n > (1 << log2_cap) // 2)
    assert check_table(g) == state_digest_of(recs[:n], pay[:n])


def test_sparse_table_and_host_parity(gpu, pool):
    """5,000 entries in 2^20 slots: most waves of the default grid see no live slot, and one block walks 4,096
    slots per wave iteration."""
    g, h = _pair(20)
    recs, pay = pool
    for idx in (g, h):
        idx.insert_records(recs, pay)
    assert g.be.log2 == 20
    want = state_digest_of(recs, pay)
    assert check_table(g, tags=[None]) == want == h.state_digest()
    assert g.state_digest((0,)) == h.state_digest((0,)) and g.state_digest((1, 2, 3, 4, 5, 6)) == h.state_digest(range(1, 7))
    assert g.state_digest((0,), grid_blocks=7) + g.state_digest(range(1, 7), grid_blocks=3) == want


def test_tombstones_rehash_and_payloadless(gpu, pool):
    g, h = _pair(12)
    recs, pay = pool
    for idx in (g, h):
        idx.insert_records(recs[:300], pay[:300])
        assert idx.erase_records(np.ascontiguousarray(recs[100:200])).all()
        idx.insert_records(recs[300:340], None)  # entries without payload: L = 0
    assert g.be.tombs == 100
    left = np.r_[0:100, 200:300]
    want = state_digest_of(recs[left], pay[left]) + state_digest_of(recs[300:340], None)
    assert check_table(g) == want == h.state_digest()
    moved, failed = g.be.L.utxo_rehash(g.be.h, 12)
    assert (moved, failed) == (240, 0)
    g.be.tombs = 0
    assert check_table(g) == want
    assert g.be.L.utxo_rehash(g.be.h, 13) == (240, 0)
    g.be.log2 = 13
    assert check_table(g) == want


@pytest.mark.parametrize('names', list(KNOWN))
def test_known_answers(gpu, names):
    recs, pay = arrays([ENTRY[x] for x in names])
    check_known(names, StateDigest(*gpu.utxo_records_digest(recs, pay.view(np.uint8))))
    check_known(names, records_digest(recs, pay, device='gpu'))
    g, _ = _pair(8)
    g.insert_records(recs, pay)
    for grid in (0, 1):
        check_known(names, g.state_digest(grid_blocks=grid))


def test_canonical_payload(gpu):
    recs, pay = arrays([C_NOISE])
    check_known(('C',), records_digest(recs, pay, device='gpu'))
    check_known(('C',), records_digest(recs, None, device='gpu'))
    g, _ = _pair(8)
    g.insert_records(recs, pay)
    check_known(('C',), g.state_digest())


@pytest.mark.parametrize('n', [0, 1, 64, 65, 1000])
def test_records_kernel(gpu, pool, n):
    recs, pay = np.ascontiguousarray(pool[0][:n]), np.ascontiguousarray(pool[1][:n])
    for p in (pay, None):
        want = state_digest_of(recs, p)
        for grid in (0, 1, 5):
            got = StateDigest(*gpu.utxo_records_digest(recs, None if p is None else p.view(np.uint8), grid))
            assert got.tobytes() == want.tobytes() and got.count == n
        assert records_digest(recs, p, device='gpu') == want == records_digest(recs, p, device='cpu')
    with pytest.raises(Exception):
        gpu.utxo_records_digest(recs, pay.view(np.uint8), 65537)


def test_additive_rule_across_apply_block(gpu, pool):
    """digest(after) = digest(before) + digest(created) - digest(spent), the block applied through the
    asynchronous path (one H2D, insert + erase queued on the node stream): the pass runs behind it."""
    g, h = _pair(12)
    recs, pay = pool
    g.insert_records(recs[:400], pay[:400])
    d0 = g.state_digest()
    ins = [(np.ascontiguousarray(recs[400:520]), np.ascontiguousarray(pay[400:520])),
           (np.ascontiguousarray(recs[520:600]), np.ascontiguousarray(pay[520:600]))]
    spent = np.ascontiguousarray(recs[37:137])
    g.apply_block(ins, spent)
    assert g.be.pending is not None  # not yet booked: state_digest settles it
    got = g.state_digest()
    created = records_digest(ins[0][0], ins[0][1]) + records_digest(ins[1][0], ins[1][1])
    assert got == d0 + created - records_digest(spent, np.ascontiguousarray(pay[37:137]))
    assert g.duplicates == 0 and got.count == 500 == len(g)
    keep = np.r_[0:37, 137:600]
    assert got == state_digest_of(recs[keep], pay[keep])
    h.insert_records(recs[keep], pay[keep])
    assert h.state_digest() == got
