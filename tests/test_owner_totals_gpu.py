"""``utxo_owner_totals`` (the holders report's hash aggregation over the HBM table) on small tables: 2^8 slots
are one block of the pass, 2^12 sixteen. Every case is compared byte for byte, and in every info field, with the
dict-loop oracle of ``tests/test_owner_totals.py`` and with a host index filled identically."""
import random
import re

import pytest

from test_owner_totals import (ALL, BYS, Case, check, edge_key_case, expected, high_tag_case, mixed_case, pub,
                               skipped_only_case, tie_case, wrap_case)
from upow_amd.ledger.utxo import OWNER_DTYPE, UtxoIndex, _GpuBackend, _owners_in_order, make_payload, pack_records

pytestmark = pytest.mark.gpu
SHAPES = [(8, 120), (12, 1900)]
M64 = (1 << 64) - 1


def _pair(log2_cap):
    """The HBM table at 2^log2_cap slots and the host table (as tests/test_address_batch_gpu.py builds them)."""
    g = UtxoIndex(backend='gpu')
    g.be = _GpuBackend(log2_cap=log2_cap)
    return g, UtxoIndex(backend='host')


def both(g, h, case, top=None, by=(0, 7), extra_skipped=0, **levers):
    """The HBM table's answer equals the oracle's and the host table's."""
    owners, info = check(g, case, top, by, extra_skipped, **levers)
    want, winfo = h.owner_totals(top, by)
    assert owners.tobytes() == want.tobytes()
    assert {k: v for k, v in info.items() if k != 'totals'} == {k: v for k, v in winfo.items() if k != 'totals'}
    assert info['totals'].tolist() == winfo['totals'].tolist()
    return owners, info


def owner_home(key33, log2_groups):
    """The group-table slot the pass starts at for an owner key: ``owner_hash`` of csrc/utxo_owners.hip."""
    w = [int.from_bytes(key33[1 + 4 * i:5 + 4 * i], 'little') for i in range(8)]
    h = (0x9E3779B97F4A7C15 * (key33[0] + 1)) & M64
    for i in range(4):
        h = ((h ^ ((w[2 * i] << 32) | w[2 * i + 1])) * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 29
    h = (h * 0x94D049BB133111EB) & M64
    return (h ^ (h >> 32)) & ((1 << log2_groups) - 1)


def spread_case(n, seed, keys):
    """n entries over ``keys`` (every key in both forms), all eight columns, amounts below 2^44."""
    c = Case(seed)
    for k in range(n):
        short, full = keys[k % len(keys)]
        col = (k // len(keys)) % 8
        c.add(full if (k // 3) % 2 else short, 0 if col == 7 else col, col == 7, c.rng.randrange(1, 1 << 44))
    return c


@pytest.mark.parametrize('log2_cap,n', SHAPES)
def test_mixed_set(gpu, log2_cap, n):
    g, h = _pair(log2_cap)
    case = mixed_case(n, 61).load(g, h)
    assert g.be.log2 == log2_cap and g.be.tombs == n // 10  # the erases left tombstones
    owners, info = both(g, h, case)
    n_owners = info['owners']
    assert 35 <= n_owners <= 40 and info['skipped'] == 25
    # owners and owners + 5: no sort; owners - 1: owners = N + 1, the sort path; the rest: sort + threshold compaction
    for top in (0, 1, 7, n_owners - 1, n_owners, n_owners + 5):
        for by in BYS:
            assert len(both(g, h, case, top, by)[0]) == min(top, n_owners)


@pytest.mark.parametrize('log2_cap,owners,tie,top', [(12, 300, (90, 140), 100), (8, 100, (30, 50), 37)])
def test_ties_across_the_boundary(gpu, log2_cap, owners, tie, top):
    """The device hands back every owner at the boundary metric, so the order among the ties is the key order.
    A 2^8-slot table cannot hold 300 owners: there the same block is scaled to 100 owners."""
    g, h = _pair(log2_cap)
    case = tie_case(62, owners, tie).load(g, h)
    assert g.be.log2 == log2_cap
    both(g, h, case)
    got, _ = both(g, h, case, top)
    assert len(got) == top
    raw, *_ = g.be.L.utxo_owner_totals(g.be.h, top, 0x81, 0, 32)
    assert len(raw) // OWNER_DTYPE.itemsize == tie[1]  # all the ties came back, not just enough to fill top
    for n in (tie[0], tie[0] + 1, tie[1] - 1, tie[1], tie[1] + 1):
        both(g, h, case, n)
    both(g, h, case, top, (7,))


@pytest.mark.parametrize('log2_cap,n', SHAPES)
def test_edge_keys_wrap_empty_skipped(gpu, log2_cap, n):
    g, h = _pair(log2_cap)
    for top in (None, 0, 3):  # the empty table
        owners, info = both(g, h, Case(0), top)
        assert len(owners) == 0 and info['owners'] == info['outputs'] == info['skipped'] == 0
    case = skipped_only_case(63, n // 10).load(g, h)
    for top in (None, 0, 3):
        owners, info = both(g, h, case, top)
        assert len(owners) == 0 and info['skipped'] == n // 10 and not info['totals'].any()

    g, h = _pair(log2_cap)
    case, n_owners = edge_key_case(64)
    case.load(g, h)
    assert both(g, h, case)[1]['owners'] == n_owners
    both(g, h, case, 2, (0,))
    for tag_bits in (8, 0):
        both(g, h, case, tag_bits=tag_bits, log2_groups=4)

    g, h = _pair(log2_cap)
    case = wrap_case(65).load(g, h)
    owners, info = both(g, h, case)
    assert int(owners[0]['sums'][0]) == 5 and int(info['totals'][0]) == 5
    both(g, h, case, 1)

    g, h = _pair(log2_cap)
    case, n_high = high_tag_case(66)
    case.load(g, h)
    both(g, h, case, extra_skipped=n_high)


@pytest.mark.parametrize('log2_cap,n', SHAPES)
def test_tag_bits_and_group_table_size(gpu, log2_cap, n):
    """A narrower fingerprint tag (at 0 bits every occupied slot on a chain is a tag match and the full compare
    decides alone) and the smallest group table that holds the owners give byte-identical results."""
    g, h = _pair(log2_cap)
    case = mixed_case(n, 67).load(g, h)
    base = g.owner_totals()[0].tobytes()
    for tag_bits in (32, 8, 0):
        for log2_groups in (0, 6):  # at most 40 owners: 2^6 slots
            assert both(g, h, case, tag_bits=tag_bits, log2_groups=log2_groups)[0].tobytes() == base
            both(g, h, case, 7, tag_bits=tag_bits, log2_groups=log2_groups)
    for bad in ({'log2_groups': 3}, {'log2_groups': 32}, {'tag_bits': 33}):
        with pytest.raises(ValueError):
            g.owner_totals(**bad)


@pytest.mark.parametrize('log2_cap,n', SHAPES)
def test_group_table_wrap_and_fill(gpu, log2_cap, n):
    rng = random.Random(68)
    late, keys = [], []
    while len(late) < 12:  # twelve owners whose chains start in the last three of 16 slots: they run past slot 15
        k = pub(rng)
        if owner_home(k[0], 4) >= 13:
            late.append(k)
    g, h = _pair(log2_cap)
    case = spread_case(n, 69, late).load(g, h)
    assert both(g, h, case, log2_groups=4)[1]['owners'] == 12
    both(g, h, case, 5, log2_groups=4, tag_bits=0)

    keys = late + [pub(rng) for _ in range(4)]  # exactly 16 owners: the table is full and every owner is found
    g, h = _pair(log2_cap)
    case = spread_case(n, 70, keys).load(g, h)
    assert both(g, h, case, log2_groups=4)[1]['owners'] == 16
    both(g, h, case, 15, ALL, log2_groups=4, tag_bits=0)

    keys.append(pub(rng))  # 17 owners: one owner's entries find no slot
    g, h = _pair(log2_cap)
    case = spread_case(n, 71, keys).load(g, h)
    with pytest.raises(RuntimeError) as e:
        g.owner_totals(log2_groups=4)
    failed = int(re.search(r'(\d+) entries found no slot', str(e.value)).group(1))
    assert failed in set(expected(case)[0]['outputs'].tolist())  # the entries of one owner
    assert both(g, h, case)[1]['owners'] == 17  # the table was only read: the default call is right


def test_seventeen_owners_one_entry_each(gpu):
    g, h = _pair(8)
    case = Case(72)
    for _ in range(17):
        case.add(pub(case.rng)[0], 0, False, 7)
    case.load(g, h)
    with pytest.raises(RuntimeError, match=r'\b1 entries found no slot'):
        g.owner_totals(log2_groups=4)
    both(g, h, case)


def test_hot_owner(gpu):
    """Every entry of a 2^12 table belongs to one key: all lanes meet in one group slot."""
    g, h = _pair(12)
    case = spread_case(1900, 73, [pub(random.Random(74))]).load(g, h)
    owners, info = both(g, h, case)
    assert len(owners) == 1 and int(owners[0]['outputs']) == 1900 and 0 < int(owners[0]['outputs_full']) < 1900
    assert (owners[0]['sums'] > 0).all() and info['totals'].tolist() == owners[0]['sums'].tolist()
    both(g, h, case, 1, ALL, tag_bits=0)


def test_after_rehash(gpu):
    g, h = _pair(8)
    case = mixed_case(120, 75)
    case.load(g, h)
    assert g.be.log2 == 8
    more = Case(76)
    keys = [pub(more.rng) for _ in range(30)]
    for k in range(80):
        more.add(keys[k % 30][k % 2], (0, 4)[k % 2], k % 4 == 0, more.rng.randrange(1, 1 << 44))
    more.load(g, h)
    assert g.be.log2 > 8 and g.be.tombs == 0  # 200 live entries: the table was rebuilt on the device
    case.entries += more.entries
    assert both(g, h, case)[1]['owners'] > 40
    both(g, h, case, 10)


def test_sees_a_pending_async_apply(gpu):
    """The pass is queued on the node stream behind a block's insert and erase launches: it sees that block
    although its counters have not been collected."""
    g, h = _pair(8)
    case = mixed_case(100, 77, n_none=5).load(g, h)
    block = Case(78)
    for k in range(20):
        block.add(pub(block.rng)[k % 2], 0, k % 5 == 0, 1000 + k)
    spent = [e[0] for e in case.live if e[1] is not None][:10]
    recs = pack_records([e[0] for e in block.entries], 0)
    pay = make_payload([e[4] for e in block.entries], [e[1] for e in block.entries], [e[3] for e in block.entries])
    g.be.apply_async([(recs, pay)], pack_records(spent))
    assert g.be.pending is not None
    raw, info = g.be.owner_totals(None, 0x81)  # the backend call: UtxoIndex would collect the counters first
    assert g.be.pending is not None
    case.entries += block.entries
    case.erase(spent)
    want, winfo = expected(case)
    assert _owners_in_order(raw, None, 0x81).tobytes() == want.tobytes()
    assert (info['owners'], info['outputs'], info['skipped']) == (winfo['owners'], winfo['outputs'], 5)
    assert info['totals'].tolist() == winfo['totals']
    h.insert([e[0] for e in block.entries], 0, pay)
    h.erase(spent)
    both(g, h, case)
    assert g.be.pending is None
