"""``GET /get_utxo_root`` and ``POST /get_utxo_proofs`` on a small ledger (host backend): the commitment and proofs
against the hashlib reference, the 422 cases, a block that spends one output and creates others, one build for two
concurrent requests after a tip move, and ``nodeless balance --verify`` against that node with an honest and a lying
peer."""
import asyncio
import hashlib
from decimal import Decimal

import pytest

from state_digest_cases import KEY_A, KEY_B
from upow_amd.ledger.utxo import merkle_of
from upow_amd.ledger.utxo_proof import ProofError, verify_outpoint


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


def _root(client):
    r = client.get('/get_utxo_root')
    assert r.status_code == 200 and r.json()['ok'] is True
    return r.json()['result']


def _proofs(client, outpoints):
    r = client.post('/get_utxo_proofs', json={'outpoints': outpoints})
    assert r.status_code == 200 and r.json()['ok'] is True
    return r.json()['result']


def test_routes_block_and_wallet(node, monkeypatch, capsys, tmp_path):
    client, main = node
    from upow_amd.wallet import nodeless
    from upow_amd.wallet.builders import address_of, create_transaction
    a, b = address_of(KEY_A), address_of(KEY_B)
    base = 1_700_000_000
    empty = _root(client)
    assert (empty['root'], empty['count'], empty['height']) == (hashlib.sha256(b'').hexdigest(), 0, 0)
    for k in range(1, 4):
        assert _mine(client, a, base + k) == {'ok': True}
    before = _root(client)
    tip = client.get('/get_mining_info').json()['result']['last_block']
    want = merkle_of(*main.db.utxo.records_payload())
    assert set(before) == {'root', 'count', 'block_hash', 'height'}
    assert (bytes.fromhex(before['root']), before['count']) == want and before['count'] == 3
    assert (before['block_hash'], before['height']) == (tip['hash'], tip['id']) and tip['id'] == 3
    builds = main.utxo_proofs.builds
    assert _root(client) == before and main.utxo_proofs.builds == builds  # the tip did not move: no new build

    # proofs in request order, each checked from its bytes alone
    outs = client.get('/get_address_info', params={'address': a}).json()['result']['spendable_outputs']
    live = [[o['tx_hash'], o['index']] for o in outs]
    gone = ['ab' * 32, 1]
    res = _proofs(client, live + [gone] + live[:1])
    assert {k: res[k] for k in before} == before and len(res['proofs']) == len(live) + 2
    root, count = bytes.fromhex(res['root']), res['count']
    for (h, i), p, o in zip(live, res['proofs'], outs):
        entry = verify_outpoint(root, count, h, i, p)
        assert (p['tx_hash'], p['index'], p['present']) == (h, i, True)
        assert entry['table'] == 'unspent_outputs' and entry['address'] == a and not entry['is_stake']
        assert Decimal(entry['amount']) / 10 ** 8 == Decimal(o['amount'])
    assert res['proofs'][-2]['present'] is False and verify_outpoint(root, count, *gone, res['proofs'][-2]) is None
    assert res['proofs'][-1] == res['proofs'][0]

    # the 422 cases
    for body in ({'outpoints': []}, {'outpoints': [live[0]] * 1001}, {}, {'outpoints': [['zz' * 32, 0]]},
                 {'outpoints': [[live[0][0], 256]]}, {'outpoints': [[live[0][0]]]}):
        assert client.post('/get_utxo_proofs', json=body).status_code == 422
    assert client.post('/get_utxo_proofs', json={'outpoints': [live[0]] * 1000}).status_code == 200

    # the wallet: every listed output proven, an agreeing peer and a peer at another block accepted, a peer with
    # another root for the same block refused
    peers_say = {'http://honest/': before, 'http://behind/': {**before, 'block_hash': 'cd' * 32, 'root': 'ef' * 32},
                 'http://liar/': {**before, 'root': '12' * 32}}

    class Shim:
        class _R:
            def __init__(self, body):
                self.body = body

            def json(self):
                return self.body

        @staticmethod
        def get(url, params=None, timeout=None):
            for peer, says in peers_say.items():
                if url.startswith(peer):
                    assert url == peer + 'get_utxo_root'
                    return Shim._R({'ok': True, 'result': says})
            assert url.startswith('http://testserver/')
            return client.get(url[len('http://testserver'):], params=params)

        @staticmethod
        def post(url, json=None, timeout=None):
            assert url.startswith('http://testserver/')
            return client.post(url[len('http://testserver'):], json=json)

    monkeypatch.setattr(nodeless, 'httpx', Shim)
    monkeypatch.setenv('UPOW_WALLET_NODE_URL', 'http://testserver/')
    monkeypatch.setenv('UPOW_NODELESS_KEY_FILE', str(tmp_path / 'wallet.json'))
    from upow_amd.utils.jsonstore import JsonStore
    JsonStore(str(tmp_path / 'wallet.json')).set('private_keys', [KEY_A])
    balance = client.get('/get_address_info', params={'address': a}).json()['result']['balance']
    proven, against = nodeless.verified_balance(a, ['http://honest/', 'http://behind/'])
    assert proven == Decimal(balance) > 0 and against['peers_agreeing'] == 1 and against['outputs'] == len(live)
    capsys.readouterr()
    assert not nodeless.main(['balance', '--verify', '--peer', 'http://honest/'])
    text = capsys.readouterr().out
    assert f'Proven balance: {proven}' in text and before['root'] in text and 'REFUSED' not in text
    with pytest.raises(nodeless.VerifyError):
        nodeless.verified_balance(a, ['http://honest/', 'http://liar/'])
    assert nodeless.main(['balance', '--verify', '--peer', 'http://liar/']) == 1
    assert 'REFUSED' in capsys.readouterr().out
    # a node that inflates an amount is caught
    honest_info = nodeless.get_address_info

    def inflated(address):
        bal, inputs = honest_info(address)
        inputs[0].amount += 1
        return bal + 1, inputs
    monkeypatch.setattr(nodeless, 'get_address_info', inflated)
    with pytest.raises(nodeless.VerifyError):
        nodeless.verified_balance(a)
    monkeypatch.setattr(nodeless, 'get_address_info', honest_info)

    # a block spends one of a's outputs and creates two: the root changes and the proofs follow
    tx = asyncio.run(create_transaction(KEY_A, b, '1.25'))
    spent = [[i.tx_hash, i.index] for i in tx.inputs]
    created = [[tx.hash(), 0], [tx.hash(), 1]]
    old = _proofs(client, spent + created)['proofs']
    assert [p['present'] for p in old] == [True] * len(spent) + [False, False]
    assert client.post('/push_tx', json={'tx_hex': tx.hex()}).json()['ok']
    assert _mine(client, a, base + 10) == {'ok': True}
    builds = main.utxo_proofs.builds
    from upow_amd.ops.native import lib
    held = lib().utxo_merkle_held()
    stale = main.utxo_proofs.state
    assert held[0] >= 1 and stale['snapshot'] is not None and stale['users'] == 0

    async def two():
        return await asyncio.gather(main.utxo_proofs.current(), main.utxo_proofs.current())
    first, second = client.portal.call(two)  # two concurrent requests after the tip moved: one build
    assert first is second and main.utxo_proofs.builds == builds + 1
    # the snapshot of the old tip was closed (nobody was proving from it): one native snapshot replaced one
    assert stale['retired'] and stale['snapshot'] is None and lib().utxo_merkle_held()[0] == held[0]
    assert first['snapshot']._sid is not None and first['users'] == 0
    after = _root(client)
    assert main.utxo_proofs.builds == builds + 1
    assert after['root'] != before['root'] and after['height'] == 4 and after['block_hash'] != before['block_hash']
    assert (bytes.fromhex(after['root']), after['count']) == merkle_of(*main.db.utxo.records_payload())
    res = _proofs(client, spent + created)
    assert {k: res[k] for k in after} == after
    assert [p['present'] for p in res['proofs']] == [False] * len(spent) + [True, True]
    root, count = bytes.fromhex(after['root']), after['count']
    for (h, i), p in zip(spent + created, res['proofs']):
        entry = verify_outpoint(root, count, h, i, p)
        assert (entry is None) == ([h, i] in spent)
    assert verify_outpoint(root, count, *created[0], res['proofs'][len(spent)])['address'] == b
    with pytest.raises(ProofError):  # the proof from before the block does not hold against the new root
        verify_outpoint(root, count, *spent[0], old[0])
