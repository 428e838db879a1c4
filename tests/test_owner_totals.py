"""Holders report (``UtxoIndex.owner_totals``: per-owner totals of the whole UTXO set) on the host backends,
``Database.get_owner_totals`` against the per-address ledger calls, and ``tools holders``.

The oracle is the dict loop of ``expected``: it runs over the entries a case inserted, minus what it erased, and
applies the fold rule (an owner is a public key: the 33-byte and the 64-byte form of an address are one owner).
It never calls the code under test. ``tests/test_owner_totals_gpu.py`` runs the same cases on the HBM table."""
import asyncio
import json
import random
from decimal import Decimal

import numpy as np
import pytest

from upow_amd.ledger.utxo import OWNER_COLUMNS, OWNER_DTYPE, UtxoIndex, make_payload

BACKENDS = ['host', 'host-py']
KEY_A = 0x1111111111111111111111111111111111111111111111111111111111111111
KEY_B = 0x2222222222222222222222222222222222222222222222222222222222222222
KEY_C = 0x3333333333333333333333333333333333333333333333333333333333333333
ALL = tuple(range(8))
BYS = [(0, 7), (7,), (3,), ALL]


def test_layout():
    assert OWNER_DTYPE.itemsize == 112 and OWNER_DTYPE.names == ('key', 'pad', 'outputs', 'outputs_full', 'sums')
    assert [OWNER_DTYPE.fields[f][1] for f in OWNER_DTYPE.names] == [0, 33, 40, 44, 48]
    assert OWNER_COLUMNS == ('spendable', 'inode_registration_output', 'validator_registration_output',
                             'validators_voting_power', 'delegates_voting_power', 'validators_ballot',
                             'inodes_ballot', 'stake')


# ------------------------------------------------------------------------------------------------ cases
def pub(rng, parity=None):
    """One public key as (33-byte form, 64-byte form): x, and a little-endian y of which only bit 0 counts."""
    x = rng.randbytes(32)
    parity = rng.randrange(2) if parity is None else parity
    y = rng.randbytes(32)
    y = bytes([(y[0] & 0xfe) | parity]) + y[1:]
    return bytes([42 + parity]) + x, x + y


class Case:
    """Entries (outpoint, owner bytes or None for ``payload=None``, tag, stake, amount) and the erased outpoints."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.entries = []
        self.erased = set()

    def add(self, owner, tag=0, stake=False, amount=1):
        key = (self.rng.randbytes(32).hex(), self.rng.randrange(0, 256))
        self.entries.append((key, owner, tag, bool(stake), amount))
        return key

    def erase(self, keys):
        self.erased.update(keys)

    @property
    def live(self):
        return [e for e in self.entries if e[0] not in self.erased]

    @property
    def n_none(self):
        return sum(1 for e in self.live if e[1] is None)

    def load(self, *indexes):
        """The same inserts and erases on every index: one insert per (tag, with or without payload)."""
        for tag in sorted({e[2] for e in self.entries}):
            for none in (False, True):
                sel = [e for e in self.entries if e[2] == tag and (e[1] is None) == none]
                if not sel:
                    continue
                pay = None if none else make_payload([e[4] for e in sel], [e[1] for e in sel], [e[3] for e in sel])
                for idx in indexes:
                    idx.insert([e[0] for e in sel], tag, pay)
        for idx in indexes:
            if self.erased:
                assert int(idx.erase(sorted(self.erased)).sum()) == len(self.erased)
        return self


def fold(owner):
    if len(owner) == 33:
        return bytes([43 if owner[0] == 43 else 42]) + owner[1:]
    assert len(owner) == 64
    return bytes([43 if owner[32] & 1 else 42]) + owner[:32]


def expected(case, top=None, by=(0, 7)):
    """(OWNER_DTYPE records, info) the issue's semantics give for the case's live entries."""
    groups, skipped, grouped = {}, 0, 0
    totals = [0] * 8
    for _, owner, tag, stake, amount in case.live:
        if owner is None or len(owner) not in (33, 64) or tag > 6:
            skipped += 1
            continue
        g = groups.setdefault(fold(owner), [0, 0, [0] * 8])
        col = 7 if tag == 0 and stake else tag
        g[0] += 1
        g[1] += len(owner) == 64
        g[2][col] = (g[2][col] + amount) % (1 << 64)
        totals[col] = (totals[col] + amount) % (1 << 64)
        grouped += 1
    keys = sorted(groups)
    if top is not None:
        keys = sorted(keys, key=lambda k: (-(sum(groups[k][2][c] for c in set(by)) % (1 << 64)), k))[:top]
    out = np.zeros(len(keys), dtype=OWNER_DTYPE)
    for n, k in enumerate(keys):
        out[n]['key'] = np.frombuffer(k, dtype=np.uint8)
        out[n]['outputs'], out[n]['outputs_full'] = groups[k][0], groups[k][1]
        out[n]['sums'] = np.array(groups[k][2], dtype=np.uint64)
    return out, {'owners': len(groups), 'outputs': grouped, 'skipped': skipped, 'totals': totals}


def check(idx, case, top=None, by=(0, 7), extra_skipped=0, **levers):
    """``idx.owner_totals`` equals the oracle byte for byte, in every info field; nothing but the case's
    ``payload=None`` entries (and ``extra_skipped`` it names) is left out."""
    owners, info = idx.owner_totals(top, by, **levers)
    want, winfo = expected(case, top, by)
    assert owners.dtype == OWNER_DTYPE and len(owners) == len(want)
    assert owners.tobytes() == want.tobytes()
    assert set(info) == {'owners', 'outputs', 'skipped', 'totals'}
    assert (info['owners'], info['outputs'], info['skipped']) == (winfo['owners'], winfo['outputs'], winfo['skipped'])
    assert np.asarray(info['totals']).dtype == np.uint64 and [int(v) for v in info['totals']] == winfo['totals']
    assert info['skipped'] == case.n_none + extra_skipped
    assert info['outputs'] + info['skipped'] == len(case.live) == len(idx)
    return owners, info


def mixed_case(n, seed, n_keys=40, n_none=25):
    """n outputs over n_keys keys, each key in both forms, all seven tags, a third of tag 0 staked, n // 10
    erased, n_none of the n inserted without a payload, and key 0 (even parity) also under prefix 2."""
    c = Case(seed)
    rng = c.rng
    keys = [pub(rng, parity=0 if k == 0 else None) for k in range(n_keys)]
    made = []
    for k in range(n - n_none):
        short, full = keys[k % n_keys]  # every key gets entries
        form = (k // n_keys) % 3
        owner = short if form == 0 else full if form == 1 else (bytes([2]) + short[1:] if k % n_keys == 0 else short)
        tag = rng.choice((0, 0, 0, 1, 2, 3, 4, 5, 6))
        made.append(c.add(owner, tag, tag == 0 and rng.random() < 0.33, rng.randrange(1, 1 << 44)))
    for _ in range(n_none):
        c.add(None, rng.choice((0, 3)))
    c.erase(rng.sample(made, n // 10))
    return c


def tie_case(seed, owners=300, tie=(90, 140)):
    """One owner per rank by spendable + stake; the owners at ranks tie[0] .. tie[1] - 1 share one metric,
    split differently over the two columns."""
    c = Case(seed)
    for rank in range(owners):
        short, full = pub(c.rng)
        if rank < tie[0]:
            c.add(short, 0, rank % 2, 10_000_000 - rank)
        elif rank < tie[1]:
            c.add(full if rank % 3 == 0 else short, 0, False, 2000 + rank)
            c.add(short, 0, True, 3000 - rank)
        else:
            c.add(short, 0, rank % 2, 4000 - rank)
    return c


def edge_key_case(seed):
    """Keys that differ only in x byte 0, only in x byte 31, or only in parity: four owners. Two 64-byte
    addresses with equal x and equal y parity but different y bytes: one owner."""
    c = Case(seed)
    short, full = pub(c.rng, parity=0)
    x, y = full[:32], full[32:]
    flip0 = bytes([x[0] ^ 1]) + x[1:]
    flip31 = x[:31] + bytes([x[31] ^ 0x80])
    owners = [short, bytes([42]) + flip0, flip31 + y, bytes([43]) + x,
              full, x + bytes([y[0]]) + bytes(b ^ 0x5a for b in y[1:])]
    for k in range(24):
        c.add(owners[k % 6], (0, 3)[k % 2], k % 4 == 0, c.rng.randrange(1, 1 << 44))
    return c, 4


def wrap_case(seed):
    c = Case(seed)
    short, full = pub(c.rng)
    c.add(short, 0, False, 1 << 63)
    c.add(full, 0, False, (1 << 63) + 5)
    return c


def skipped_only_case(seed, n=9):
    c = Case(seed)
    for _ in range(n):
        c.add(None, c.rng.choice((0, 5)))
    return c


def high_tag_case(seed):
    """Entries of a tag above 6 carry payloads and are still not grouped."""
    c = Case(seed)
    keys = [pub(c.rng) for _ in range(5)]
    for k in range(32):
        c.add(keys[k % 5][k % 2], (0, 6, 7, 9)[k % 4], False, 100 + k)
    return c, sum(1 for e in c.entries if e[2] > 6)


# ------------------------------------------------------------------------------------------------ index
@pytest.mark.parametrize('backend', BACKENDS)
def test_mixed_set(backend):
    idx = UtxoIndex(backend=backend)
    case = mixed_case(3000, 51).load(idx)
    owners, info = check(idx, case)
    assert info['owners'] == 40 and info['skipped'] == 25 and len(owners) == 40
    assert int(owners['outputs_full'].sum()) > 0 and (info['totals'] > 0).all()
    assert not any(bytes(k)[0] == 2 for k in owners['key'])  # prefix 2 folded into its prefix-42 owner
    for top in (0, 1, 7, 40, 45):
        for by in BYS:
            got, _ = check(idx, case, top, by)
            assert len(got) == min(top, 40)


@pytest.mark.parametrize('backend', BACKENDS)
def test_ties_across_the_boundary(backend):
    idx = UtxoIndex(backend=backend)
    case = tie_case(52).load(idx)
    full, _ = check(idx, case)
    got, info = check(idx, case, 100)
    assert info['owners'] == 300 and len(got) == 100
    metric = (got['sums'][:, 0] + got['sums'][:, 7]).tolist()
    assert metric[89] > metric[90] == metric[99] == 5000 and metric == sorted(metric, reverse=True)
    tied = [bytes(k) for k in got['key'][90:]]
    every = sorted(bytes(o['key']) for o in full if int(o['sums'][0] + o['sums'][7]) == 5000)
    assert len(every) == 50 and tied == every[:10]  # the ten smallest keys of the fifty


@pytest.mark.parametrize('backend', BACKENDS)
def test_edge_keys(backend):
    idx = UtxoIndex(backend=backend)
    case, n_owners = edge_key_case(53)
    case.load(idx)
    owners, info = check(idx, case)
    assert info['owners'] == n_owners == len(owners)
    check(idx, case, 2, (0,))


@pytest.mark.parametrize('backend', BACKENDS)
def test_sums_are_modulo_2_64(backend):
    idx = UtxoIndex(backend=backend)
    case = wrap_case(54).load(idx)
    owners, info = check(idx, case)
    assert len(owners) == 1 and int(owners[0]['sums'][0]) == 5 and int(info['totals'][0]) == 5
    assert (int(owners[0]['outputs']), int(owners[0]['outputs_full'])) == (2, 1)
    check(idx, case, 1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_empty_and_skipped_only(backend):
    idx = UtxoIndex(backend=backend)
    for top in (None, 0, 3):
        owners, info = check(idx, Case(0), top)
        assert len(owners) == 0 and info['owners'] == info['outputs'] == info['skipped'] == 0
    case = skipped_only_case(55).load(idx)
    for top in (None, 0, 3):
        owners, info = check(idx, case, top)
        assert len(owners) == 0 and info['owners'] == 0 and info['skipped'] == 9
        assert not np.asarray(info['totals']).any()


@pytest.mark.parametrize('backend', BACKENDS)
def test_tag_above_six_is_skipped(backend):
    idx = UtxoIndex(backend=backend)
    case, n_high = high_tag_case(56)
    case.load(idx)
    assert n_high == 16
    _, info = check(idx, case, extra_skipped=n_high)
    assert info['outputs'] == 16
    check(idx, case, 3, ALL, extra_skipped=n_high)


@pytest.mark.parametrize('backend', BACKENDS)
def test_argument_errors(backend):
    idx = UtxoIndex(backend=backend)
    wrap_case(57).load(idx)
    for top, by in [(None, ()), (None, (8,)), (None, (-1,)), (None, (0, 9)), (-1, (0, 7)), (-5, (0,)),
                    (None, ('stake',))]:
        with pytest.raises(ValueError):
            idx.owner_totals(top, by)
    assert len(idx.owner_totals(None, [7, 0])[0]) == 1  # any sequence of columns


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
    """A mines, pays B in both address forms, B stakes: the scenario of tests/test_address_batch.py, with the
    64-byte payment mined after the stake."""
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
    await devnet.mine_block(a, [tx], ts=base + 10)
    stx = await builders.create_stake_transaction(KEY_B, '1')
    assert await chain.add_pending_transaction(stx)
    await devnet.mine_block(a, [stx], ts=base + 11)
    # the payment to B's 64-byte form comes after the stake, so the stake cannot spend it: it stays live
    tx2 = await builders.create_transaction(KEY_A, b_full, '1.25', send_back_address=a_full)
    assert await chain.add_pending_transaction(tx2)
    await devnet.mine_block(a, [tx2], ts=base + 12)
    return [a, b, c, b_full, a_full]


def test_ledger_owner_totals(chain):
    from upow_amd.utils.codec import point_to_string, string_to_bytes, string_to_point

    async def go():
        addrs = await _small_ledger(chain)
        rows, summary = await chain.get_owner_totals()
        by_address = {r['address']: r for r in rows}
        assert len(by_address) == len(rows) == summary['holders'] and summary['skipped'] == 0
        keys = [string_to_bytes(r['address']) for r in rows]  # base58 of the 33 key bytes
        assert all(len(k) == 33 for k in keys) and keys == sorted(keys)
        for x in addrs:
            row = by_address.get(point_to_string(string_to_point(x)))
            balance, stake = await chain.get_address_balance(x), await chain.get_address_stake(x)
            if row is None:
                assert balance == 0 and stake == 0 and x == addrs[2]
                continue
            assert row['spendable'] == balance and row['stake'] == stake
            assert set(row) == {'address', 'outputs', 'outputs_full_form', 'spendable', 'stake', 'tables'}
            assert set(row['tables']) == set(OWNER_COLUMNS[1:7])
        b = by_address[addrs[1]]
        assert b['outputs_full_form'] >= 1 and b['outputs'] > b['outputs_full_form'] and b['stake'] == Decimal(1)
        assert by_address[addrs[0]]['outputs_full_form'] >= 1  # A's change came back to its 64-byte form
        assert sum(r['outputs'] for r in rows) == summary['outputs'] == len(chain.utxo)
        for col in OWNER_COLUMNS:
            want = sum((r[col] if col in r else r['tables'][col] for r in rows), Decimal(0))
            assert summary['totals'][col] == want
        assert summary['totals']['spendable'] > 0 and summary['totals']['stake'] == Decimal(1)
        # top 1 by stake is B; by the default columns it is the miner
        top, s1 = await chain.get_owner_totals(1, ('stake',))
        assert [r['address'] for r in top] == [addrs[1]] and s1 == summary
        top, _ = await chain.get_owner_totals(1)
        assert [r['address'] for r in top] == [addrs[0]]
        with pytest.raises(ValueError):
            await chain.get_owner_totals(None, ('balance',))
        return addrs
    asyncio.run(go())


def test_tools_holders(chain, monkeypatch, capsys, tmp_path):
    from upow_amd import tools
    addrs = asyncio.run(_small_ledger(chain))
    rows, summary = asyncio.run(chain.get_owner_totals())

    async def opened(path=None):
        return chain
    monkeypatch.setattr(tools, 'open_ledger', opened)
    capsys.readouterr()
    assert tools.main(['holders']) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    assert len(lines) == len(rows) + 1 and [x['address'] for x in lines[:-1]] == [r['address'] for r in rows]
    for x, r in zip(lines, rows):
        assert Decimal(x['spendable']) == r['spendable'] and Decimal(x['stake']) == r['stake']
        assert x['outputs'] == r['outputs'] and x['outputs_full_form'] == r['outputs_full_form']
        assert {t: Decimal(v) for t, v in x['tables'].items()} == r['tables']
    last = lines[-1]
    assert set(last) == {'holders', 'outputs', 'skipped', 'totals', 'backend'}
    assert (last['holders'], last['outputs'], last['skipped']) == (len(rows), summary['outputs'], 0)
    assert last['backend'] == 'host' and list(last['totals']) == list(OWNER_COLUMNS)
    assert {c: Decimal(v) for c, v in last['totals'].items()} == summary['totals']

    assert tools.main(['holders', '--top', '1', '--by', 'stake']) == 0
    top = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    assert len(top) == 2 and top[0]['address'] == addrs[1] and top[1] == last

    out = tmp_path / 'holders.jsonl'
    assert tools.main(['holders', '--out', str(out)]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 1 and json.loads(printed[0]) == last
    assert [json.loads(x) for x in out.read_text().splitlines()] == lines[:-1]

    # an entry indexed without its payload is reported, not guessed at: exit status 1
    chain.utxo.insert([('ab' * 32, 0)], 0, None)
    assert tools.main(['holders', '--top', '0']) == 1
    only = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    assert len(only) == 1 and only[0]['skipped'] == 1 and only[0]['holders'] == last['holders']
