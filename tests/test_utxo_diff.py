"""The UTXO diff on the host (``upow_amd.ledger.utxo``: ``diff_of``, ``UtxoDiff``, ``UtxoIndex.diff_records`` on the
``host`` / ``host-py`` indices): the reference against an independent oracle on planted differences, tag subsets,
truncation, the argument errors, the tie to the state digest, patching an index from its diff, and ``tools
utxo-diff`` in its three modes on a small mined ledger."""
import asyncio
import json

import numpy as np
import pytest

from state_digest_cases import C, C_NOISE, chain, small_ledger  # noqa: F401
from utxo_diff_cases import (CHANGES, NOISE, arrays, assert_same, brute_diff, check_lists, check_rows, keys_of, plant,
                             random_entries)
from upow_amd.ledger.utxo import PAYLOAD_DTYPE, UtxoDiff, UtxoIndex, diff_of, diff_vectorised, records_digest

BACKENDS = ['host', 'host-py']


@pytest.fixture(scope='module')
def pool():
    """300 random entries (records, payloads) and a planted O, shared and never written."""
    recs, pay = arrays(random_entries(300, 91))
    p = plant(recs, pay, 5)
    for a in (recs, pay, p.recs, p.pay):
        a.setflags(write=False)
    return recs, pay, p


def _index(backend, recs, pay):
    idx = UtxoIndex(backend=backend)
    idx.insert_records(np.array(recs), None if pay is None else np.array(pay))
    return idx


@pytest.mark.parametrize('n', [0, 1, 300])
def test_reference_against_oracle(n):
    recs, pay = arrays(random_entries(n, 17 + n))
    p = plant(recs, pay, n)
    if n == 300:  # every edit found entries to work on
        assert all(len(p.edits[name]) == 3 for name in CHANGES + NOISE + ('dropped', 'fresh'))
        assert len(p.edits['sibling']) == 1 and len(p.changed) == 27 and len(p.missing) == 4 and len(p.extra) == 3
    assert (p.missing, p.extra, p.changed) == brute_diff(p.recs, p.pay, recs, pay)
    d = diff_of(p.recs, p.pay, recs, pay)
    assert isinstance(d, UtxoDiff) and (d.compared, d.entries) == (len(p.recs), n)
    check_lists(d, p.missing, p.extra, p.changed)
    check_rows(d, p.recs, p.pay, recs, pay)
    # O without payloads: every entry of I that has one is changed
    d = diff_of(p.recs, None, recs, pay)
    check_lists(d, *brute_diff(p.recs, None, recs, pay))
    check_rows(d, p.recs, None, recs, pay)


def test_vectorised_join_equals_reference(pool):
    """``diff_vectorised`` (what the native host table runs) against ``diff_of``: planted sets with every lever,
    and outpoints that share the 64-bit head it sorts by, which must fall back to the reference's answer."""
    recs, pay, p = pool
    for o_pay in (p.pay, None):
        for mask in (None, 0x01, 0x7e):
            for limit in (None, 2):
                assert_same(diff_vectorised(p.recs, o_pay, recs, pay, tag_mask=mask, limit=limit),
                            diff_of(p.recs, o_pay, recs, pay, tag_mask=mask, limit=limit))
    assert diff_vectorised(recs[:0], None, recs[:0], None).equal
    assert diff_vectorised(recs[:5], pay[:5], recs[:0], pay[:0]).n_missing == 5
    assert diff_vectorised(recs[:0], pay[:0], recs[:5], pay[:5]).n_extra == 5
    # the head is the txid's first eight bytes and the index: a twin differs in the bytes behind them
    twins = np.array(recs[:4])
    twins[:, 8:32] ^= 0x55
    both_r, both_p = np.concatenate([recs[:50], twins]), np.concatenate([pay[:50], pay[50:54]])
    for o_recs, o_pay, i_recs, i_pay in ((both_r, both_p, recs[:50], pay[:50]),   # O's twin finds the other's head
                                         (recs[:50], pay[:50], both_r, both_p),   # two of the index share a head
                                         (both_r, both_p, both_r[::-1], both_p[::-1])):
        d = diff_vectorised(o_recs, o_pay, i_recs, i_pay)
        assert_same(d, diff_of(o_recs, o_pay, i_recs, i_pay))
        check_lists(d, *brute_diff(o_recs, o_pay, i_recs, i_pay))
    with pytest.raises(ValueError):
        diff_vectorised(np.concatenate([recs[:5], recs[4:5]]), None, recs[:20], pay[:20])
    with pytest.raises(ValueError):
        diff_vectorised(both_r[[50, 50]], None, both_r, both_p)


@pytest.mark.parametrize('backend', BACKENDS)
def test_index_equals_reference(pool, backend):
    recs, pay, p = pool
    idx = _index(backend, recs, pay)
    assert idx.backend_name == backend
    before = idx.records_payload()
    for o_pay in (p.pay, None):
        d = idx.diff_records(p.recs, o_pay, chunk_records=7)
        assert_same(d, diff_of(p.recs, o_pay, *before))
        check_lists(d, *brute_diff(p.recs, o_pay, recs, pay))
        check_rows(d, p.recs, o_pay, recs, pay)
    after = idx.records_payload()
    assert len(idx) == 300 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


@pytest.mark.parametrize('backend', BACKENDS)
def test_equal_sets(pool, backend):
    recs, pay, _ = pool
    idx = _index(backend, recs, pay)
    order = np.random.default_rng(3).permutation(len(recs))
    d = idx.diff_records(recs[order], pay[order])
    assert d.equal and not d.truncated and (d.compared, d.entries) == (300, 300)
    check_lists(d, [], [], [])
    assert d.missing[0].shape == (0, 40) and d.missing[1].dtype == PAYLOAD_DTYPE and len(d.changed) == 4
    empty = UtxoIndex(backend=backend).diff_records(np.zeros((0, 40), np.uint8))
    assert empty.equal and (empty.compared, empty.entries) == (0, 0)


def test_noise_does_not_count():
    recs, pay = arrays([C])
    noisy = arrays([C_NOISE])
    for backend in BACKENDS:
        idx = _index(backend, recs, pay)
        assert idx.diff_records(*noisy).equal and idx.diff_records(noisy[0], None).equal
        assert _index(backend, *noisy).diff_records(recs, pay).equal


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('tags', [(0,), (1, 2, 3, 4, 5, 6)])
def test_tag_subsets(pool, backend, tags):
    recs, pay, p = pool
    idx = _index(backend, recs, pay)
    d = idx.diff_records(p.recs, p.pay, tags)
    check_lists(d, *brute_diff(p.recs, p.pay, recs, pay, tags))
    check_rows(d, p.recs, p.pay, recs, pay)
    assert d.compared == int(np.isin(p.recs[:, 36], tags).sum()) and d.entries == int(np.isin(recs[:, 36], tags).sum())
    assert_same(d, diff_of(p.recs, p.pay, *idx.records_payload(), tag_mask=sum(1 << t for t in tags)))
    # an outpoint that O holds under a tag of the subset and the index under one outside it: changed, and the
    # index's entry, outside the subset, is not extra
    moved = [k for k in p.edits['tag'] if k in set(keys_of(d.changed[0]))]
    for k in moved:
        row = keys_of(d.changed[0]).index(k)
        assert int(d.changed[0][row, 36]) in tags and int(d.changed[2][row, 36]) != int(d.changed[0][row, 36])
    one = np.array(recs[:1])
    inside, outside = tags[0], 6 if tags == (0,) else 0
    one[0, 36] = outside
    idx2 = _index(backend, one, pay[:1])
    one[0, 36] = inside
    d = idx2.diff_records(one, pay[:1], tags)
    assert (d.n_missing, d.n_extra, d.n_changed, d.compared, d.entries) == (0, 0, 1, 1, 0)
    assert int(d.changed[2][0, 36]) == outside and int(d.changed[0][0, 36]) == inside


@pytest.mark.parametrize('backend', BACKENDS)
def test_limit_truncates_lists_not_counts(pool, backend):
    recs, pay, p = pool
    idx = _index(backend, recs, pay)
    full = idx.diff_records(p.recs, p.pay)
    d = idx.diff_records(p.recs, p.pay, limit=2)
    assert d.truncated and not d.equal
    assert (d.n_missing, d.n_extra, d.n_changed) == (full.n_missing, full.n_extra, full.n_changed) == (4, 3, 27)
    assert len(d.missing[0]) == len(d.extra[0]) == len(d.changed[0]) == len(d.changed[2]) == 2
    assert set(keys_of(d.extra[0])) <= set(p.extra)
    # the first two of each kind in O's order, then sorted
    o_keys = keys_of(p.recs)
    assert keys_of(d.missing[0]) == sorted([k for k in o_keys if k in set(p.missing)][:2])
    assert keys_of(d.changed[0]) == sorted([k for k in o_keys if k in set(p.changed)][:2])
    check_rows(d, p.recs, p.pay, recs, pay)
    none = idx.diff_records(p.recs, p.pay, limit=0)
    assert none.truncated and len(none.missing[0]) == len(none.extra[0]) == len(none.changed[0]) == 0
    assert none.n_changed == 27
    assert not idx.diff_records(p.recs, p.pay, limit=27).truncated


@pytest.mark.parametrize('backend', BACKENDS)
def test_value_errors(pool, backend):
    recs, pay, _ = pool
    idx = _index(backend, recs[:20], pay[:20])
    bad = np.array(recs[:3])
    bad[1, 33] = 1  # index 256 + x
    with pytest.raises(ValueError):
        idx.diff_records(bad, pay[:3])
    bad = np.array(recs[:3])
    bad[2, 36] = 32
    with pytest.raises(ValueError):
        idx.diff_records(bad, pay[:3])
    with pytest.raises(ValueError):
        idx.diff_records(recs[:3], pay[:2])
    with pytest.raises(ValueError):
        idx.diff_records(recs[:3], pay[:3], tags=(40,))
    with pytest.raises(ValueError):
        idx.diff_records(recs[:3], pay[:3], limit=-1)
    twice = np.concatenate([recs[:5], recs[4:5]])
    with pytest.raises(ValueError):
        idx.diff_records(twice, np.concatenate([pay[:5], pay[4:5]]))
    with pytest.raises(ValueError):
        diff_of(twice, None, recs[:20], pay[:20])
    # a repeated outpoint that is absent: missing once per occurrence
    absent = np.concatenate([recs[:5], recs[30:31], recs[30:31]])
    d = idx.diff_records(absent, np.concatenate([pay[:5], pay[30:31], pay[30:31]]))
    assert (d.n_missing, d.n_extra, d.n_changed) == (2, 15, 0)
    assert keys_of(d.missing[0]) == keys_of(recs[30:31]) * 2
    assert len(idx) == 20 and idx.diff_records(recs[:20], pay[:20]).equal


@pytest.mark.parametrize('seed', range(12))
def test_tie_to_the_digest(seed):
    """The diff is empty exactly when the digests agree: planted differences (seeds 0..5), the noise edits alone
    (6..8) and the same set in another order (9..11)."""
    recs, pay = arrays(random_entries(40, 200 + seed))
    if seed < 9:
        p = plant(recs, pay, seed, k=1, kinds=None if seed < 6 else NOISE)
        o_recs, o_pay = p.recs, p.pay
        assert all(p.edits[name] for name in NOISE) and bool(p.changed) == (seed < 6)
    else:
        o_recs, o_pay = np.ascontiguousarray(recs[::-1]), np.ascontiguousarray(pay[::-1])
    idx = _index(BACKENDS[seed % 2], recs, pay)
    d = idx.diff_records(o_recs, o_pay)
    assert d.equal == (seed >= 6)
    assert d.equal == (idx.state_digest() == records_digest(o_recs, o_pay, device='cpu'))


@pytest.mark.parametrize('backend', BACKENDS)
def test_patching_the_index_from_its_diff(pool, backend):
    recs, pay, p = pool
    idx = _index(backend, recs, pay)
    d = idx.diff_records(p.recs, p.pay)
    assert not d.equal and idx.state_digest() != records_digest(p.recs, p.pay, device='cpu')
    assert idx.erase_records(np.ascontiguousarray(d.extra[0])).all()
    assert idx.erase_records(np.ascontiguousarray(d.changed[2])).all()
    idx.insert_records(*d.missing)
    idx.insert_records(*d.changed[:2])
    assert idx.duplicates == 0 and len(idx) == len(p.recs)
    assert idx.state_digest() == records_digest(p.recs, p.pay, device='cpu')
    assert idx.diff_records(p.recs, p.pay).equal


def test_tools_utxo_diff(chain, monkeypatch, capsys, tmp_path):  # noqa: F811
    from upow_amd import tools
    from upow_amd.ledger import snapshot
    asyncio.run(small_ledger(chain))

    async def opened(path=None):
        return chain
    monkeypatch.setattr(tools, 'open_ledger', opened)
    fresh = str(tmp_path / 'fresh.bin')
    snapshot.save(chain, fresh)
    capsys.readouterr()

    def run(*args):
        code = tools.main(['utxo-diff', *args])
        lines = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
        return code, lines[:-1], lines[-1]

    live = chain.utxo.state_digest()
    for mode in (['--snapshot', fresh], ['--sql'], ['--snapshot', fresh, '--against', fresh]):
        code, lines, summary = run(*mode)
        assert code == 0 and lines == [] and summary['equal'] is True and summary['truncated'] is False
        assert set(summary) == {'equal', 'missing', 'extra', 'changed', 'compared', 'entries', 'truncated', 'backend',
                                'seconds'}
        assert (summary['missing'], summary['extra'], summary['changed']) == (0, 0, 0)
        assert summary['compared'] == summary['entries'] == live.count

    # the rebuild through the extracted helper restores an equal index
    sql_recs, sql_pay = chain._utxo_arrays_from_sql()
    assert len(sql_recs) == live.count and records_digest(sql_recs, sql_pay, device='cpu') == live
    chain._rebuild_utxo_index()
    assert chain.utxo.state_digest() == live and chain.utxo.diff_records(sql_recs, sql_pay).equal

    # one entry erased from the index, one foreign entry inserted, one amount rewritten
    recs, pay = chain.utxo.records_payload()
    full = [j for j in range(len(recs)) if int(pay['len'][j]) in (33, 64)]
    gone, rewritten = full[0], full[-1]
    assert gone != rewritten
    foreign = arrays(random_entries(1, 7))
    assert chain.utxo.erase_records(np.ascontiguousarray(recs[[gone, rewritten]])).all()
    other_amount = np.array(pay[rewritten:rewritten + 1])
    other_amount['amount'] += np.uint64(1)
    chain.utxo.insert_records(np.ascontiguousarray(recs[rewritten:rewritten + 1]), other_amount)
    chain.utxo.insert_records(*foreign)
    edited = str(tmp_path / 'edited.bin')
    snapshot.save(chain, edited)
    want = {('missing', bytes(recs[gone, :32]).hex(), int(recs[gone, 32])),
            ('extra', bytes(foreign[0][0, :32]).hex(), int(foreign[0][0, 32])),
            ('changed', bytes(recs[rewritten, :32]).hex(), int(recs[rewritten, 32]))}
    out_file = tmp_path / 'diff.jsonl'
    for mode in (['--snapshot', fresh], ['--sql'], ['--snapshot', edited, '--against', fresh],
                 ['--sql', '--out', str(out_file)]):
        code, lines, summary = run(*mode)
        if '--out' in mode:
            assert lines == []
            lines = [json.loads(x) for x in out_file.read_text().splitlines()]
        assert code == 1 and summary['equal'] is False
        assert (summary['missing'], summary['extra'], summary['changed']) == (1, 1, 1)
        assert {(x['kind'], x['tx_hash'], x['index']) for x in lines} == want and len(lines) == 3
        by_kind = {x['kind']: x for x in lines}
        assert set(by_kind['missing']) == {'kind', 'tx_hash', 'index', 'table', 'amount', 'address', 'is_stake'}
        assert set(by_kind['missing']) == set(by_kind['extra'])
        assert set(by_kind['changed']) == {'kind', 'tx_hash', 'index', 'other', 'index_entry'}
        one, two = by_kind['changed']['other'], by_kind['changed']['index_entry']
        assert isinstance(one['amount'], str) and one['amount'] != two['amount']
        assert {k: v for k, v in one.items() if k != 'amount'} == {k: v for k, v in two.items() if k != 'amount'}
        assert by_kind['missing']['address'] == bytes(pay['addr'][gone][:int(pay['len'][gone])]).hex()
    code, lines, summary = run('--sql', '--limit', '0')
    assert code == 1 and lines == [] and summary['truncated'] is True and summary['changed'] == 1
    with pytest.raises(SystemExit):
        tools.main(['utxo-diff'])
    with pytest.raises(SystemExit):
        tools.main(['utxo-diff', '--sql', '--snapshot', fresh])

    # the rebuild brings the index back to the SQL tables' set
    chain._rebuild_utxo_index()
    assert chain.utxo.state_digest() == live
    assert run('--sql')[0] == 0 and run('--snapshot', fresh)[0] == 0
