"""``utxo_diff`` (csrc/utxo_diff.hip: the HBM table against uploaded records, a match kernel and a sweep for the
extras) on small tables, list for list and byte for byte against the reference ``diff_of`` on the table's own dump:
record and extra counts around the wave, the block and the tail, chunk boundaries that cut through waves, dense and
sparse tables, engineered probe chains, every single-field change, payload-less entries, tombstones and rehashes,
the argument error that the device detects, and a diff behind a real asynchronous block apply."""
import numpy as np
import pytest

from test_utxo_adversarial import _assert_mirrors, near_equal, same_home
from utxo_diff_cases import (CHANGES, NOISE, arrays, assert_same, brute_diff, check_lists, check_rows, keys_of, plant,
                             random_entries)
from upow_amd.ledger.utxo import PAYLOAD_DTYPE, UtxoIndex, _GpuBackend, diff_of, records_digest

pytestmark = pytest.mark.gpu
COUNTS = [0, 1, 63, 64, 65, 257]


def _table(log2_cap, recs=None, pay=None):
    """The HBM table at 2^log2_cap slots (as tests/test_state_digest_gpu.py builds it), holding (recs, pay)."""
    g = UtxoIndex(backend='gpu')
    g.be = _GpuBackend(log2_cap=log2_cap)
    if recs is not None and len(recs):
        g.insert_records(np.ascontiguousarray(recs), None if pay is None else np.ascontiguousarray(pay))
    return g


@pytest.fixture(scope='module')
def pool():
    """5,000 random entries (records, payloads) and O planted on the first 257 of them, shared and never written."""
    recs, pay = arrays(random_entries(5000, 72))
    p = plant(recs[:257], pay[:257], 11)
    for a in (recs, pay, p.recs, p.pay):
        a.setflags(write=False)
    return recs, pay, p


def check(g, o_recs, o_pay, tags=None, **levers):
    """g's diff against O equals the reference on g's own dump; returns it."""
    mask = None if tags is None else sum(1 << t for t in tags)
    d = g.diff_records(o_recs, o_pay, tags, **levers)
    assert_same(d, diff_of(o_recs, o_pay, *g.records_payload(), tag_mask=mask))
    return d


@pytest.mark.parametrize('n', COUNTS)
def test_record_counts_and_chunks(gpu, pool, n):
    """O of 0, 1, 63, 64, 65 and 257 records (same, missing and changed ones mixed) on a 257-entry table, uploaded
    whole and in chunks of 64 and 100 records: a lone lane, one short of a wave, a wave, one over, more than a
    block, and chunk ends inside a wave."""
    recs, pay, p = pool
    g = _table(12, recs[:257], pay[:257])
    assert len(g) == 257 and g.be.log2 == 12
    o_recs, o_pay = np.ascontiguousarray(p.recs[:n]), np.ascontiguousarray(p.pay[:n])
    first = None
    for chunk in (0, 64, 100):
        for o in (o_pay, None):
            d = check(g, o_recs, o, chunk_records=chunk)
            check_lists(d, *brute_diff(o_recs, o, recs[:257], pay[:257]))
        first = first or d
        assert (d.compared, d.entries) == (n, 257) and d.n_extra == 257 - (n - d.n_missing)
    if n == 257:
        assert first.n_missing and first.n_changed


def test_empty_sides(gpu, pool):
    recs, pay, _ = pool
    g = _table(8)
    d = check(g, recs[:70], pay[:70])
    assert (d.n_missing, d.n_extra, d.n_changed, d.entries) == (70, 0, 0, 0)
    assert check(g, np.zeros((0, 40), np.uint8), None).equal
    g = _table(8, recs[:70], pay[:70])
    d = check(g, np.zeros((0, 40), np.uint8), np.zeros(0, PAYLOAD_DTYPE))
    assert (d.n_missing, d.n_extra, d.n_changed, d.compared, d.entries) == (0, 70, 0, 0, 70)
    check_rows(d, recs[:0], pay[:0], recs[:70], pay[:70])


@pytest.mark.parametrize('log2_cap', [8, 12])
@pytest.mark.parametrize('extras', COUNTS)
def test_extra_counts(gpu, pool, log2_cap, extras):
    """0, 1, 63, 64, 65 and 257 extras: the sweep's compaction with no extra, a lone one, around a wave's ballot
    and across blocks. The 2^8-slot table is dense (120 entries; it has grown to 2^10 slots for the 300 of the
    last case), so neighbouring live slots share a word of the seen bitmap."""
    recs, pay, _ = pool
    n = 300 if extras > 100 else 120
    g = _table(log2_cap, recs[:n], pay[:n])
    assert g.be.log2 == (log2_cap if n == 120 or log2_cap == 12 else 10)
    d = check(g, recs[extras:n], pay[extras:n])
    check_lists(d, [], sorted(keys_of(recs[:extras])), [])
    check_rows(d, recs[extras:n], pay[extras:n], recs[:n], pay[:n])


def test_sparse_table_and_host_parity(gpu, pool):
    """5,000 entries in 2^20 slots: most blocks of the sweep see no live slot. The same planted case on the host
    table gives the same diff."""
    recs, pay, _ = pool
    p = plant(recs, pay, 23, k=40)
    g, h = _table(20, recs, pay), UtxoIndex(backend='host')
    h.insert_records(np.array(recs), np.array(pay))
    assert g.be.log2 == 20 and len(g) == 5000
    d = check(g, p.recs, p.pay)
    check_lists(d, p.missing, p.extra, p.changed)
    assert_same(d, h.diff_records(p.recs, p.pay))
    assert (d.n_missing, d.n_extra, d.n_changed) == (41, 40, 360)


def test_limit(gpu, pool):
    """limit 10 with 65 extras, 20 missing and 12 changed: exact counts, ten true ones of each kind listed."""
    recs, pay, _ = pool
    g = _table(12, recs[:200], pay[:200])
    o_recs, o_pay = np.array(recs[65:220]), np.array(pay[65:220])
    o_pay['amount'][10:22] += np.uint64(1 << 33)  # entries 75..86: these all have a payload below
    o_pay['len'][10:22] = 33
    full = check(g, o_recs, o_pay)
    assert (full.n_missing, full.n_extra, full.n_changed) == (20, 65, 12) and not full.truncated
    d = g.diff_records(o_recs, o_pay, limit=10)
    ref = diff_of(o_recs, o_pay, *g.records_payload(), limit=10)
    assert d.truncated and (d.n_missing, d.n_extra, d.n_changed) == (20, 65, 12)
    for got, want in zip(d.missing + d.changed, ref.missing + ref.changed):  # the first ten in O's order
        assert len(got) == 10 and got.tobytes() == want.tobytes()
    assert len(d.extra[0]) == len(d.extra[1]) == 10 and len(set(keys_of(d.extra[0]))) == 10
    assert set(keys_of(d.extra[0])) <= set(keys_of(recs[:65])) and keys_of(d.extra[0]) == sorted(keys_of(d.extra[0]))
    check_rows(d, o_recs, o_pay, recs[:200], pay[:200])
    none = g.diff_records(o_recs, o_pay, limit=0)
    assert none.truncated and (none.n_missing, none.n_extra, none.n_changed) == (20, 65, 12)
    assert len(none.extra[0]) == len(none.missing[0]) == len(none.changed[2]) == 0


@pytest.mark.parametrize('slot', [100, 250])
def test_probe_chains(gpu, slot):
    """40 outpoints with one home slot (from slot 250 the chain wraps past the last slot of the 2^8 table), five
    erased in the middle: O asks for all 40 and finds 35 across the tombstones. Then keys that differ from a
    present one in one bit of one word, and the same txid under index 0 (present) and 255 (absent)."""
    keys = same_home(40, 8, slot, 3, seed=slot)
    _assert_mirrors(gpu, keys, 8)
    pay = arrays(random_entries(40, slot))[1]
    g = _table(8, keys, pay)
    assert g.be.log2 == 8
    assert g.erase_records(np.ascontiguousarray(keys[17:22])).all()
    d = check(g, keys, pay)
    check_lists(d, sorted(keys_of(keys[17:22])), [], [])
    near = near_equal(keys[0])  # same home slot, one bit of words 1..7 flipped
    g.insert_records(np.ascontiguousarray(near[:1]), np.ascontiguousarray(pay[:1]))
    o_recs = np.concatenate([keys[:1], near[:2]])
    d = check(g, o_recs, np.concatenate([pay[:1], pay[:1], pay[:1]]))
    check_lists(d, keys_of(near[1:2]), sorted(keys_of(keys[1:17]) + keys_of(keys[22:])), [])
    zero = np.array(keys[30:31])
    zero[0, 32] = 0
    top = np.array(zero)
    top[0, 32] = 255
    g.insert_records(zero, np.ascontiguousarray(pay[30:31]))
    d = check(g, np.concatenate([zero, top]), np.concatenate([pay[30:31], pay[30:31]]))
    assert keys_of(d.missing[0]) == keys_of(top) and d.n_changed == 0 and d.n_extra == 36


def test_every_single_field_change_and_noise(gpu, pool):
    recs, pay, _ = pool
    p = plant(recs[:300], pay[:300], 31)
    assert all(len(p.edits[name]) == 3 for name in CHANGES + NOISE)
    g = _table(12, recs[:300], pay[:300])
    d = check(g, p.recs, p.pay, chunk_records=128)
    check_lists(d, p.missing, p.extra, p.changed)
    check_rows(d, p.recs, p.pay, recs[:300], pay[:300])
    for name in CHANGES:  # each kind of edit alone, on top of the noise
        one = plant(recs[:300], pay[:300], 31, kinds=NOISE + (name,))
        assert len(one.changed) == 3
        check_lists(check(g, one.recs, one.pay), [], [], one.changed)
    quiet = plant(recs[:300], pay[:300], 31, kinds=NOISE)
    assert quiet.pay.tobytes() != plant(recs[:300], pay[:300], 31, kinds=()).pay.tobytes()
    assert check(g, quiet.recs, quiet.pay).equal
    assert g.state_digest() == records_digest(quiet.recs, quiet.pay, device='cpu')


def test_payloadless_entries(gpu, pool):
    recs, pay, _ = pool
    g = _table(10, recs[:100], None)
    assert check(g, recs[:100], None).equal
    assert check(g, recs[:100], np.zeros(100, PAYLOAD_DTYPE)).equal
    d = check(g, recs[:100], pay[:100])
    with_payload = sorted(k for k, n in zip(keys_of(recs[:100]), pay['len'][:100]) if int(n) in (33, 64))
    assert 80 < len(with_payload) < 100
    check_lists(d, [], [], with_payload)
    assert not d.changed[3]['len'].any() and d.changed[1]['len'].all()


def test_repeated_live_outpoint(gpu, pool):
    """A live outpoint twice in O (in one wave, and in two chunks): ValueError; an absent one twice: missing twice.
    The table still answers afterwards."""
    recs, pay, _ = pool
    g = _table(10, recs[:200], pay[:200])
    rows = np.r_[0:200, 7]
    for chunk in (0, 64):
        with pytest.raises(ValueError):
            g.diff_records(recs[rows], pay[rows], chunk_records=chunk)
    with pytest.raises(ValueError):
        g.diff_records(recs[np.r_[5, 5, 5]], None)
    rows = np.r_[0:200, 300, 300]
    d = check(g, recs[rows], pay[rows])
    assert (d.n_missing, d.n_extra, d.n_changed) == (2, 0, 0) and keys_of(d.missing[0]) == keys_of(recs[300:301]) * 2
    assert check(g, recs[:200], pay[:200]).equal and len(g) == 200


def test_tombstones_and_rehash(gpu, pool):
    recs, pay, p = pool
    g = _table(12, recs[:300], pay[:300])
    assert g.erase_records(np.ascontiguousarray(recs[257:300])).all() and g.be.tombs == 43
    want = check(g, p.recs, p.pay)
    check_lists(want, p.missing, p.extra, p.changed)
    assert g.be.L.utxo_rehash(g.be.h, 12) == (257, 0)
    g.be.tombs = 0
    assert_same(check(g, p.recs, p.pay), want)
    assert g.be.L.utxo_rehash(g.be.h, 13) == (257, 0)
    g.be.log2 = 13
    assert_same(check(g, p.recs, p.pay, chunk_records=100), want)


def test_behind_an_asynchronous_apply_block(gpu, pool):
    """The diff against the dump from before a block, queued behind the block's asynchronous apply, is exactly
    the block: its created entries are extra, its spent ones missing."""
    recs, pay, _ = pool
    g = _table(12, recs[:400], pay[:400])
    before = g.records_payload()
    ins = [(np.ascontiguousarray(recs[400:520]), np.ascontiguousarray(pay[400:520])),
           (np.ascontiguousarray(recs[520:600]), np.ascontiguousarray(pay[520:600]))]
    spent = np.ascontiguousarray(recs[37:137])
    g.apply_block(ins, spent)
    assert g.be.pending is not None  # not yet booked: diff_records settles it
    d = g.diff_records(*before)
    assert g.be.pending is None and g.duplicates == 0 and len(g) == 500
    check_lists(d, sorted(keys_of(spent)), sorted(keys_of(recs[400:600])), [])
    check_rows(d, *before, recs[np.r_[0:37, 137:600]], pay[np.r_[0:37, 137:600]])
    assert (d.compared, d.entries) == (400, 500)
    assert_same(d, diff_of(*before, *g.records_payload()))


def test_read_only(gpu, pool):
    recs, pay, p = pool
    g = _table(12, recs[:257], pay[:257])
    before, digest = g.records_payload(), g.state_digest()
    assert not g.diff_records(p.recs, p.pay).equal and not g.diff_records(p.recs, None, (0,), limit=1).equal
    after = g.records_payload()
    assert len(g) == 257 and g.state_digest() == digest
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


@pytest.mark.parametrize('tags', [(0,), (1, 2, 3, 4, 5, 6)])
def test_tag_subsets(gpu, pool, tags):
    recs, pay, p = pool
    g = _table(12, recs[:257], pay[:257])
    d = check(g, p.recs, p.pay, tags)
    check_lists(d, *brute_diff(p.recs, p.pay, recs[:257], pay[:257], tags))
    assert d.entries == int(np.isin(recs[:257, 36], tags).sum()) and d.compared == int(np.isin(p.recs[:, 36], tags).sum())
    # live under a tag outside the subset, asked for under one inside it: changed, neither missing nor extra
    inside, outside = tags[0], 6 if tags == (0,) else 0
    one = np.array(recs[:1])
    one[0, 36] = outside
    g = _table(8, one, pay[:1])
    one[0, 36] = inside
    d = check(g, one, pay[:1], tags)
    assert (d.n_missing, d.n_extra, d.n_changed, d.compared, d.entries) == (0, 0, 1, 1, 0)
    assert int(d.changed[0][0, 36]) == inside and int(d.changed[2][0, 36]) == outside
