"""Batched address queries (K14 for many addresses in one pass): ``UtxoIndex.address_outputs_many`` against
the single ``address_outputs`` on every backend, the ledger's ``_many`` forms against the per-address calls,
``POST /get_addresses_info`` against ``/get_address_info`` and ``tools address-utxos A B`` against two runs."""
import asyncio
import hashlib
import json
import random
from decimal import Decimal

import numpy as np
import pytest

from upow_amd.ledger.utxo import STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY, UtxoIndex, make_payload

BACKENDS = ['host', 'host-py', pytest.param('gpu', marks=pytest.mark.gpu)]
KEY_A = 0x1111111111111111111111111111111111111111111111111111111111111111
KEY_B = 0x2222222222222222222222222222222222222222222222222222222222222222
KEY_C = 0x3333333333333333333333333333333333333333333333333333333333333333


def _keys(n, seed):
    rng = random.Random(seed)
    return [(rng.randbytes(32).hex(), rng.randrange(0, 256)) for _ in range(n)]


def _index(backend, request):
    if backend == 'gpu':
        request.getfixturevalue('gpu')
    return UtxoIndex(backend=backend)


def _address_case(idx, seed):
    """3000 outputs over 40 owners (33-byte and 64-byte addresses) in tables 0, 3 and 5, a third of the
    table-0 ones staked, 300 erased. Owner 40 owns nothing."""
    rng = random.Random(seed)
    owners = [bytes([42 + (k & 1)]) + rng.randbytes(32) if k % 4 else rng.randbytes(64) for k in range(41)]
    keys = _keys(3000, seed)
    own = [rng.randrange(40) for _ in keys]
    amounts = [rng.randrange(1, 1 << 44) for _ in keys]
    tags = [rng.choice((0, 0, 0, 3, 5)) for _ in keys]
    stake = [t == 0 and rng.random() < 0.33 for t in tags]
    for t in (0, 3, 5):
        sel = [k for k in range(3000) if tags[k] == t]
        idx.insert([keys[k] for k in sel], t, make_payload([amounts[k] for k in sel], [owners[own[k]] for k in sel],
                                                           [stake[k] for k in sel]))
    idx.erase(keys[:300])
    return owners


def _same(got, want):
    """One query's (records, payloads, sum) equals another's, byte for byte."""
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes()
    assert got[2] == want[2]


@pytest.mark.parametrize('backend', BACKENDS)
def test_batch_equals_single_scans(backend, request):
    """Every owner x three tag sets x three stake selectors in one batch: each answer is the single scan's."""
    idx = _index(backend, request)
    owners = _address_case(idx, 21)
    queries = [(o, tagset, sel) for o in owners for tagset in ((0,), (0, 3, 5), (5,))
               for sel in (STAKE_ANY, STAKE_EXCLUDE, STAKE_ONLY)]
    got = idx.address_outputs_many(queries)
    assert len(got) == len(queries) == 41 * 9
    hits = 0
    for q, g in zip(queries, got):
        _same(g, idx.address_outputs(*q))
        hits += len(g[0])
    assert hits > 2700  # the (0, 3, 5) / any-stake queries alone return every live output


@pytest.mark.parametrize('backend', BACKENDS)
def test_edge_batches(backend, request):
    idx = _index(backend, request)
    owners = _address_case(idx, 22)
    assert idx.address_outputs_many([]) == []
    one = idx.address_outputs_many([(owners[1], (0,), STAKE_ANY)])
    assert len(one) == 1 and len(one[0][0]) > 0
    _same(one[0], idx.address_outputs(owners[1], (0,), STAKE_ANY))
    # an owner without outputs: empty arrays of the usual shapes
    none = idx.address_outputs_many([(owners[40], (0, 3, 5), STAKE_ANY)])[0]
    assert none[0].shape == (0, 40) and len(none[1]) == 0 and none[2] == 0
    _same(none, idx.address_outputs(owners[40], (0, 3, 5), STAKE_ANY))
    # the same query twice, and the same address under two filters
    q = (owners[2], (0, 3, 5), STAKE_ANY)
    a, b, c, d = idx.address_outputs_many([q, q, (owners[2], (0,), STAKE_EXCLUDE), (owners[2], (5,), STAKE_ANY)])
    _same(a, b)
    _same(a, idx.address_outputs(*q))
    _same(c, idx.address_outputs(owners[2], (0,), STAKE_EXCLUDE))
    _same(d, idx.address_outputs(owners[2], (5,), STAKE_ANY))
    assert len(a[0]) > len(c[0]) > 0 and len(a[0]) > len(d[0]) > 0
    # a 33-byte query and the 64-byte address that starts with the same bytes: each its own matches only
    long = owners[0]
    assert len(long) == 64
    short = long[:33]
    ks = _keys(7, 23)
    idx.insert(ks, 0, make_payload([3] * 7, [short] * 7))
    s, l = idx.address_outputs_many([(short, (0, 3, 5), STAKE_ANY), (long, (0, 3, 5), STAKE_ANY)])
    assert len(s[0]) == 7 and s[2] == 21 and all(int(p['len']) == 33 for p in s[1])
    assert len(l[0]) > 7 and all(int(p['len']) == 64 for p in l[1])
    _same(s, idx.address_outputs(short, (0, 3, 5)))
    _same(l, idx.address_outputs(long, (0, 3, 5)))


# ------------------------------------------------------------------------------------------------ ledger
@pytest.fixture
def chain(monkeypatch):
    from upow_amd.ledger import manager
    from upow_amd.ledger.database import Database
    monkeypatch.setattr(manager, 'START_DIFFICULTY', Decimal('1.5'))
    manager.Manager.difficulty = None
    manager.cache.clear()
    db = asyncio.run(Database.create(utxo_backend='host'))
    yield db
    db.close()


async def _small_ledger(chain):
    """A mines, pays B in both address forms, B stakes; a transfer A -> B is left pending."""
    from upow_amd import devnet
    from upow_amd.utils.codec import AddressFormat, point_to_string, string_to_point
    from upow_amd.wallet import builders
    a, b, c = (builders.address_of(k) for k in (KEY_A, KEY_B, KEY_C))
    a_full = point_to_string(string_to_point(a), AddressFormat.FULL_HEX)
    b_full = point_to_string(string_to_point(b), AddressFormat.FULL_HEX)
    base = 1_700_000_000
    for k in range(4):
        await devnet.mine_block(a, ts=base + 1 + k)
    tx = await builders.create_transaction(KEY_A, b, '2.5')
    assert await chain.add_pending_transaction(tx)
    tx2 = await builders.create_transaction(KEY_A, b_full, '1.25', send_back_address=a_full)
    assert await chain.add_pending_transaction(tx2)
    await devnet.mine_block(a, [tx, tx2], ts=base + 10)
    stx = await builders.create_stake_transaction(KEY_B, '1')
    assert await chain.add_pending_transaction(stx)
    await devnet.mine_block(a, [stx], ts=base + 11)
    pending = await builders.create_transaction(KEY_A, b, '0.75')
    assert await chain.add_pending_transaction(pending)
    return [a, b, c, b_full, a_full]


def _inputs(outs):
    return [(i.tx_hash, i.index, i.amount, i.public_key) for i in outs]


def test_ledger_many_equal_per_address_calls(chain):
    async def go():
        addrs = await _small_ledger(chain)
        differs = False
        for from_index in (True, False):  # False: the UPOW_ADDRESS_SQL=1 setting
            chain.address_queries_from_index = from_index
            for pend in (False, True):
                many = await chain.get_spendable_outputs_many(addrs, pend)
                bals = await chain.get_address_balances(addrs, pend)
                assert list(many) == addrs and list(bals) == addrs
                for x in addrs:
                    assert _inputs(many[x]) == _inputs(await chain.get_spendable_outputs(x, pend))
                    assert bals[x] == await chain.get_address_balance(x, pend)
            differs |= _inputs((await chain.get_spendable_outputs_many(addrs, True))[addrs[0]]) != \
                _inputs((await chain.get_spendable_outputs_many(addrs, False))[addrs[0]])
        assert differs  # the pending spend does take outputs of A away
        chain.address_queries_from_index = True
        assert await chain.get_spendable_outputs_many([]) == {} and await chain.get_address_balances([], True) == {}
        rows = chain._index_address_rows_many(addrs, STAKE_ANY, False)
        assert rows == [chain._index_address_rows(x, STAKE_ANY, False) for x in addrs]
        assert rows[2] == [] and rows[0] and rows[1]
    asyncio.run(go())


def test_tools_address_utxos_two_addresses(chain, monkeypatch, capsys):
    from upow_amd import tools

    async def go():
        addrs = await _small_ledger(chain)
        both = await tools.address_utxos_many(addrs[:2], db=chain)
        assert both == [await tools.address_utxos(x, db=chain) for x in addrs[:2]]
        assert both[0]['outputs'] and both[1]['outputs']
        return addrs
    addrs = asyncio.run(go())

    async def opened(path=None):
        return chain
    monkeypatch.setattr(tools, 'open_ledger', opened)
    capsys.readouterr()
    tools.main(['address-utxos', addrs[0], addrs[1]])
    two = capsys.readouterr().out
    tools.main(['address-utxos', addrs[0]])
    first = capsys.readouterr().out
    tools.main(['address-utxos', addrs[1]])
    second = capsys.readouterr().out
    assert two == first + second and len(two.splitlines()) == 2
    assert json.loads(first)['address'] == addrs[0] and json.loads(first)['outputs']


# ------------------------------------------------------------------------------------------------ REST
@pytest.fixture
def node(tmp_path, monkeypatch):
    monkeypatch.setenv('UPOW_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('UPOW_CORE_URL', '')
    monkeypatch.setenv('UPOW_DATABASE_PATH', str(tmp_path / 'ledger.sqlite3'))
    monkeypatch.setenv('UPOW_UTXO_BACKEND', 'host')
    from upow_amd.ledger import manager
    monkeypatch.setattr(manager, 'START_DIFFICULTY', Decimal('1.5'))
    manager.Manager.difficulty = None
    from upow_amd.node import main, peers
    peers.reset()
    main.limiter.reset()
    main.transactions_cache.clear()
    from starlette.testclient import TestClient
    with TestClient(main.app, base_url='http://testserver') as c:
        yield c, main
    main.db.close()


def _mine(client, address, ts):
    from upow_amd.models.block import PowTarget, header_prefix
    from upow_amd.ops.pow import PowJob, search
    info = client.get('/get_mining_info').json()['result']
    last = info['last_block']
    prev = last.get('hash', (18_884_643).to_bytes(32, 'little').hex())
    hashes = info['pending_transactions_hashes']
    merkle = hashlib.sha256(b''.join(bytes.fromhex(h) for h in hashes)).hexdigest()
    job = PowJob.create(header_prefix(prev, address, merkle, ts, info['difficulty']),
                        PowTarget.from_difficulty(prev, info['difficulty']))
    r = search(job, 0, 1 << 20, device='cpu', threads=2)
    content = job.header_with_nonce(r.nonces[0]).hex()
    return client.post('/push_block', json={'block_content': content, 'txs': hashes,
                                            'block_no': last.get('id', 0) + 1}).json()


def test_get_addresses_info(node):
    client, main = node
    from starlette.testclient import TestClient
    from upow_amd.wallet.builders import address_of, create_transaction
    a, b, c = address_of(KEY_A), address_of(KEY_B), address_of(KEY_C)
    base = 1_700_000_000
    for k in range(1, 4):
        assert _mine(client, a, base + k) == {'ok': True}
    tx = asyncio.run(create_transaction(KEY_A, b, '1.25'))
    assert client.post('/push_tx', json={'tx_hex': tx.hex()}).json()['ok']
    assert _mine(client, a, base + 10) == {'ok': True}
    order = [b, c, a, b]
    r = client.post('/get_addresses_info', json={'addresses': order})
    assert r.status_code == 200
    body = r.json()
    assert body['ok'] is True and [e['address'] for e in body['result']] == order
    for e in body['result']:
        one = client.get('/get_address_info', params={'address': e['address']}).json()['result']
        assert set(e) == {'address', 'balance', 'spendable_outputs'}
        assert e['balance'] == one['balance'] and e['spendable_outputs'] == one['spendable_outputs']
    assert body['result'][0]['balance'] == '1.25' and body['result'][3] == body['result'][0]
    assert Decimal(body['result'][1]['balance']) == 0 and body['result'][1]['spendable_outputs'] == []
    assert len(body['result'][2]['spendable_outputs']) >= 3
    # check_pending_txs leaves out what a pending transaction spends
    tx2 = asyncio.run(create_transaction(KEY_A, b, '0.5'))
    assert client.post('/push_tx', json={'tx_hex': tx2.hex()}).json()['ok']
    with_pending = client.post('/get_addresses_info', json={'addresses': [a], 'check_pending_txs': True}).json()
    without = client.post('/get_addresses_info', json={'addresses': [a]}).json()
    spent = {(i.tx_hash, i.index) for i in tx2.inputs}
    outs = lambda res: {(o['tx_hash'], o['index']) for o in res['result'][0]['spendable_outputs']}  # noqa: E731
    assert outs(without) - outs(with_pending) == spent
    # an empty list and 1001 addresses are refused before any scan
    assert 400 <= client.post('/get_addresses_info', json={'addresses': []}).status_code < 500
    assert 400 <= client.post('/get_addresses_info', json={'addresses': [a] * 1001}).status_code < 500
    assert 400 <= client.post('/get_addresses_info', json={}).status_code < 500
    assert client.post('/get_addresses_info', json={'addresses': [a] * 1000}).status_code == 200
    # a malformed address fails the whole request the way /get_address_info fails for it
    raw = TestClient(main.app, base_url='http://testserver', raise_server_exceptions=False)  # 500s as responses
    single = raw.get('/get_address_info', params={'address': 'not-an-address'})
    many = raw.post('/get_addresses_info', json={'addresses': [a, 'not-an-address']})
    assert single.json()['ok'] is False
    assert many.status_code == single.status_code and many.json() == single.json()
