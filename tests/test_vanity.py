"""K16 vanity search on the host path: the prefix arithmetic against brute-force base58, the batched-affine walk
against the existing key derivation, the range test at its edges, and a search end to end through both CLIs."""
import asyncio
import json
import random

import numpy as np
import pytest

from upow_amd.ops import p256 as op
from upow_amd.ops.native import lib
from upow_amd.utils.codec import b58encode, point_to_string
from upow_amd.utils.p256 import N
from upow_amd.wallet import vanity
from vanity_cases import (B, E2E_BASE, E2E_COUNT, E2E_FIRST, E2E_PREFIX, EDGE_BASE, EDGE_COUNT, HI, INFO, LO, be32,
                          edge_cases, oracle_addresses, pack, search)


@pytest.fixture(scope='module')
def e2e_oracle():
    rows = oracle_addresses(E2E_BASE, E2E_COUNT)
    return [b58encode(r) for r in rows]


# ------------------------------------------------------------------------------------------------ prefix_ranges
def in_ranges(ranges, v):
    return any(lo <= v < hi for lo, hi in ranges)


def spellings(prefix):
    out = ['']
    for c in prefix:
        out = [s + v for s in out for v in sorted({c.lower(), c.upper()}) if v in vanity._B58_INDEX]
    return out


SAMPLES = None


def samples():
    global SAMPLES
    if SAMPLES is None:
        rng = random.Random(58)
        vals = [LO, (43 << 256) - 1, 43 << 256, HI - 1] + [rng.randrange(LO, HI) for _ in range(3000)]
        SAMPLES = [(v, b58encode(v.to_bytes(33, 'big'))) for v in vals]
    return SAMPLES


def sample_prefixes():
    """Prefixes of length 1 to 6 taken from sampled addresses (so they are feasible), the boundary addresses among them."""
    rng = random.Random(7)
    picks = [s for _, s in samples()[:4]] + [s for _, s in rng.sample(samples(), 8)]
    return sorted({s[:k] for s in picks for k in range(1, 7)})


def test_prefix_ranges_match_base58_text():
    for prefix in sample_prefixes():
        ranges = vanity.prefix_ranges(prefix)
        assert ranges == sorted(ranges) and all(LO <= lo < hi <= HI for lo, hi in ranges)
        assert all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))  # disjoint and merged: never adjacent
        for v, text in samples():
            assert in_ranges(ranges, v) == text.startswith(prefix), (prefix, text)
        # the bounds themselves: the first and the last value of every range start with the prefix, their neighbours
        # outside the range do not (unless they leave the address space)
        for lo, hi in ranges:
            assert b58encode(lo.to_bytes(33, 'big')).startswith(prefix)
            assert b58encode((hi - 1).to_bytes(33, 'big')).startswith(prefix)
            assert lo == LO or not b58encode((lo - 1).to_bytes(33, 'big')).startswith(prefix)
            assert hi == HI or not b58encode(hi.to_bytes(33, 'big')).startswith(prefix)


def test_prefix_ranges_ignore_case():
    for prefix in sample_prefixes():
        try:
            ranges = vanity.prefix_ranges(prefix, ignore_case=True)
        except ValueError:
            assert len(spellings(prefix)) > INFO['max_ranges']
            continue
        assert len(ranges) <= INFO['max_ranges']
        assert all(a[1] < b[0] for a, b in zip(ranges, ranges[1:]))
        for v, text in samples():
            assert in_ranges(ranges, v) == text.lower().startswith(prefix.lower()), (prefix, text)
        # exactly the union of the feasible spellings' own ranges
        want = set()
        for s in spellings(prefix):
            try:
                want.update(vanity.prefix_ranges(s))
            except ValueError:
                pass
        merged = []
        for lo, hi in sorted(want):
            if merged and merged[-1][1] == lo:
                merged[-1] = (merged[-1][0], hi)
            else:
                merged.append((lo, hi))
        assert ranges == merged
    assert vanity.prefix_ranges('dv', ignore_case=True) == vanity.prefix_ranges('DV') + vanity.prefix_ranges('Dv')
    assert vanity.prefix_ranges('e5', ignore_case=True) == vanity.prefix_ranges('E5')  # 'e...' has no address


def test_prefix_ranges_address_space():
    assert vanity.prefix_ranges('') == [(LO, HI)]
    assert vanity.prefix_ranges('D') == [(LO, 58 ** 44 * 13)]
    assert vanity.prefix_ranges('E') == [(58 ** 44 * 13, HI)]
    first = b58encode(LO.to_bytes(33, 'big'))
    assert vanity.prefix_ranges(first) == [(LO, LO + 1)]  # a whole address: 45 characters
    assert vanity.expected_keys([(LO, HI)]) == 1.0
    assert vanity.expected_keys([(LO, 43 << 256)]) == 2.0
    assert vanity.expected_keys(vanity.prefix_ranges('Dv')) == pytest.approx(2 * 2 ** 256 / 58 ** 43)


@pytest.mark.parametrize('prefix', ['D0', 'DO', 'DI', 'Dl', 'D v', 'Dé'])
def test_prefix_ranges_invalid_character(prefix):
    with pytest.raises(ValueError, match='base58'):
        vanity.prefix_ranges(prefix)
    if prefix in ('D0', 'D v', 'Dé'):  # neither case of the character is in the alphabet
        with pytest.raises(ValueError, match='base58'):
            vanity.prefix_ranges(prefix, ignore_case=True)


def test_prefix_ranges_ignore_case_takes_the_other_case():
    # 'o' and 'L' are in the alphabet, 'O' and 'l' are not: without case both spell the one that is
    assert vanity.prefix_ranges('DO', ignore_case=True) == vanity.prefix_ranges('Do')
    assert vanity.prefix_ranges('Dzl', ignore_case=True) == vanity.prefix_ranges('DZL') + vanity.prefix_ranges('DzL')


def test_prefix_ranges_infeasible():
    for prefix in ['DA', 'DT', 'A', 'z', 'E6', 'Ez', 'DU1', 'E57']:
        with pytest.raises(ValueError, match='no address starts with') as e:
            vanity.prefix_ranges(prefix)
        assert "'U'..'z'" in str(e.value) and "'1'..'5'" in str(e.value)
    with pytest.raises(ValueError, match='45 characters'):
        vanity.prefix_ranges('D' + 'v' * 45)
    with pytest.raises(ValueError, match='spellings|ranges'):
        vanity.prefix_ranges('Dabcdefgh', ignore_case=True)  # 2**8 spellings, all inside the address space


# ------------------------------------------------------------------------------------------------ the walk
WALK_COUNTS = [1, 2, B - 1, B, B + 1, 2 * B + 1]


def walk_bases(count):
    rng = random.Random(count)
    return [1, 2, N - count] + [rng.randrange(1, N - count) for _ in range(3)]


@pytest.mark.parametrize('count', WALK_COUNTS)
def test_walk_matches_pubkey_many(count):
    for base in walk_bases(count):
        got = lib().p256_vanity_walk(be32(base), count, False, 8)
        assert got == b''.join(oracle_addresses(base, count)), (hex(base), count)


def test_walk_exceptional_centres():
    """Runs whose centre or centre advance would meet dx = 0 if it were not handled: a run from scalar (B + 1) / 2
    advances from the centre B G by B G (a doubling); even tails at the top of the range end at n - 1; a run of
    more than one host work item."""
    run = 16 * B
    for base, count in [((B + 1) // 2, 2 * B), ((B + 1) // 2, 3 * B + 2), (2, B + 2), (2, B + 3), (1, B + 2),
                        (N - 4, 4), (N - B - 2, B + 2), (N - 2 * B - 6, 2 * B + 6), (3, run + 2), (N - run - 5, run + 5)]:
        got = lib().p256_vanity_walk(be32(base), count, False, 8)
        assert got == b''.join(oracle_addresses(base, count)), (hex(base), count)


def test_host_pool_walk_and_search():
    """Enough batches for the host pool to run them on several threads (64 work items or more): the walk's rows and
    the search's atomic hit sink, at every thread count the same as on one thread."""
    count = 80 * B + 7
    base = N - count
    want = oracle_addresses(base, count)
    evens = [i for i, a in enumerate(want) if a[0] == 42]
    for threads in (1, 3, 8):
        assert lib().p256_vanity_walk(be32(base), count, False, threads) == b''.join(want)
        total, idx = lib().p256_vanity_search(be32(base), count, pack([(LO, 43 << 256)]), count, False, threads)
        assert (total, [int(v) for v in np.frombuffer(idx, dtype='<u8')]) == (len(evens), evens)
        total, idx = lib().p256_vanity_search(be32(base), count, pack([(LO, 43 << 256)]), 9, False, threads)
        assert total == len(evens) and len(idx) == 72 and set(np.frombuffer(idx, dtype='<u8').tolist()) <= set(evens)


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    full = [(LO, HI)]
    L = lib()
    for base, count in [(0, 1), (N, 1), (N - 1, 2), (N - 5, 6), (5, -1)]:
        with pytest.raises(ValueError):
            L.p256_vanity_search(be32(base), count, pack(full), 8, False, 8)
        with pytest.raises(ValueError):
            L.p256_vanity_walk(be32(base), count, False, 8)
    assert L.p256_vanity_search(be32(N - 1), 1, pack(full), 8, False, 8)[0] == 1  # base + count = n is the limit
    assert L.p256_vanity_search(be32(5), 0, pack(full), 8, False, 8) == (0, b'')
    assert L.p256_vanity_walk(be32(5), 0, False, 8) == b''
    with pytest.raises(ValueError):
        L.p256_vanity_search(b'\x01' * 31, 1, pack(full), 8, False, 8)  # base length
    with pytest.raises(ValueError):
        L.p256_vanity_search(be32(1), 1, pack(full)[:-1], 8, False, 8)  # range length
    with pytest.raises(ValueError):
        L.p256_vanity_search(be32(1), 1, b'', 8, False, 8)  # R = 0
    many = [(LO + 2 * i, LO + 2 * i + 1) for i in range(INFO['max_ranges'] + 1)]
    with pytest.raises(ValueError):
        L.p256_vanity_search(be32(1), 1, pack(many), 8, False, 8)  # R > max_ranges
    assert L.p256_vanity_search(be32(1), 1, pack(many[:-1]), 8, False, 8)[0] == 0
    for bad in [[(LO + 5, LO + 9), (LO, LO + 2)],      # unsorted
                [(LO, LO + 5), (LO + 4, LO + 9)],      # overlapping
                [(LO + 5, LO + 5)],                    # empty
                [(LO + 5, LO + 4)]]:                   # reversed
        with pytest.raises(ValueError):
            L.p256_vanity_search(be32(1), 1, pack(bad), 8, False, 8)
    assert L.p256_vanity_search(be32(1), 1, pack([(LO, LO + 5), (LO + 5, LO + 9)]), 8, False, 8)[0] == 0  # adjacent is fine
    with pytest.raises(ValueError):
        op.vanity_search(0, 1, full)
    with pytest.raises(ValueError):
        op.vanity_search(1, N, full)
    with pytest.raises(ValueError):
        op.vanity_search(1, 1, [(LO, 1 << 264)])


# ------------------------------------------------------------------------------------------------ range edges
def test_search_range_edges():
    addresses = oracle_addresses(EDGE_BASE, EDGE_COUNT)
    for ranges, want in edge_cases(addresses):
        assert search(EDGE_BASE, EDGE_COUNT, ranges) == (len(want), want), ranges
    k = B // 2
    assert edge_cases(addresses)[6][1] == [k]  # the one-value range around key k hits exactly k


def test_search_hit_buffer_overflow():
    total, idx = search(EDGE_BASE, EDGE_COUNT, [(LO, HI)], max_hits=7)
    assert total == EDGE_COUNT and len(idx) == 7 and len(set(idx)) == 7
    assert idx == sorted(idx) and all(0 <= i < EDGE_COUNT for i in idx)
    assert search(EDGE_BASE, EDGE_COUNT, [(LO, HI)], max_hits=0) == (EDGE_COUNT, [])


# ------------------------------------------------------------------------------------------------ end to end
def test_find_returns_first_oracle_hit(e2e_oracle):
    hits = [i for i, a in enumerate(e2e_oracle) if a.startswith(E2E_PREFIX)]
    assert hits and hits[0] == E2E_FIRST
    seen = []
    d, address = vanity.find(E2E_PREFIX, base=E2E_BASE, device='cpu', max_keys=E2E_COUNT, chunk=1 << 12,
                             progress=lambda done, expect: seen.append(done))
    assert d == E2E_BASE + hits[0] and address == e2e_oracle[hits[0]] and address.startswith(E2E_PREFIX)
    assert point_to_string(op.public_key(d)) == address
    assert seen == []  # found in the first chunk
    # every hit of the walk, against the enumeration
    total, idx = op.vanity_search(E2E_BASE, E2E_COUNT, vanity.prefix_ranges(E2E_PREFIX), device='cpu')
    assert (total, [int(i) for i in idx]) == (len(hits), hits)
    # more hits than the buffer returns: still the first
    common = 'E' if e2e_oracle[0][0] == 'D' else 'D'
    first = next(i for i, a in enumerate(e2e_oracle) if a.startswith(common))
    assert first > 0
    assert sum(a.startswith(common) for a in e2e_oracle) > 4096
    assert vanity.find(common, base=E2E_BASE, device='cpu', max_keys=E2E_COUNT, chunk=E2E_COUNT)[0] == E2E_BASE + first
    # without case
    low = [i for i, a in enumerate(e2e_oracle) if a.lower().startswith('dz')]
    assert vanity.find('dZ', ignore_case=True, base=E2E_BASE, device='cpu', max_keys=E2E_COUNT)[0] == E2E_BASE + low[0]


def test_find_gives_up_and_reports_progress(e2e_oracle):
    prefix = e2e_oracle[0][:6]
    later = [i for i, a in enumerate(e2e_oracle) if a.startswith(prefix)]
    assert later == [0]
    seen = []
    assert vanity.find(prefix, base=E2E_BASE + 1, device='cpu', max_keys=3000, chunk=1024,
                       progress=lambda done, expect: seen.append((done, expect))) is None
    assert [d for d, _ in seen] == [1024, 2048, 3000] and seen[0][1] == vanity.expected_keys(vanity.prefix_ranges(prefix))


def test_find_rechecks_the_walk(monkeypatch):
    monkeypatch.setattr(op, 'vanity_search', lambda base, count, ranges, **kw: (1, np.array([3], dtype='<u8')))
    with pytest.raises(RuntimeError, match='does not start with'):
        vanity.find('DVau1t', base=E2E_BASE, device='cpu', max_keys=100)


@pytest.fixture
def ledger(tmp_path, monkeypatch):
    monkeypatch.setenv('UPOW_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('UPOW_KEY_FILE', str(tmp_path / 'keys.json'))
    monkeypatch.setattr('upow_amd.ops.native._gpu', False)  # the host path, whatever the machine has
    from upow_amd.ledger.database import Database
    db = asyncio.run(Database.create(utxo_backend='host'))
    yield db
    db.close()


def test_createwallet_prefix_cli(ledger, tmp_path, capsys):
    from upow_amd.wallet import cli
    asyncio.run(cli.main(['createwallet', '--prefix', 'Dv']))
    asyncio.run(cli.main(['createwallet', '--prefix', 'dx', '--ignore-case', '--max-keys', '100000']))
    out = capsys.readouterr().out
    assert out.count('expected keys to try') == 2 and out.count('Address: ') == 2
    keys = json.loads((tmp_path / 'keys.json').read_text())['keys']
    assert len(keys) == 2
    for kp, prefix in zip(keys, ['Dv', 'dx']):
        address = point_to_string(op.public_key(int(kp['private_key'])))
        assert address == kp['public_key'] and address.lower().startswith(prefix.lower())
    assert keys[0]['public_key'].startswith('Dv')
    asyncio.run(cli.main(['createwallet', '--prefix', 'E5555', '--max-keys', '1000']))  # gives up, stores nothing
    assert 'No address' in capsys.readouterr().out
    assert len(json.loads((tmp_path / 'keys.json').read_text())['keys']) == 2
    with pytest.raises(SystemExit):
        asyncio.run(cli.main(['createwallet', '--prefix', 'DA']))


def test_tools_vanity_cli(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv('UPOW_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('UPOW_KEY_FILE', str(tmp_path / 'keys.json'))
    from upow_amd import tools
    out = tmp_path / 'vanity.json'
    assert tools.main(['vanity', 'Dw', '--count', '3', '--out', str(out), '--device', 'cpu']) == 0
    keys = json.loads(out.read_text())['keys']
    assert len(keys) == 3 and len({kp['private_key'] for kp in keys}) == 3
    for kp in keys:
        address = point_to_string(op.public_key(int(kp['private_key'])))
        assert address == kp['public_key'] and address.startswith('Dw')
    assert not (tmp_path / 'keys.json').exists()  # the key store is not touched
    assert 'expected keys to try' in capsys.readouterr().err
    assert tools.main(['vanity', 'E5555', '--max-keys', '1000', '--device', 'cpu']) == 1
    assert json.loads(capsys.readouterr().out) == {'keys': []}
    with pytest.raises(SystemExit):
        tools.main(['vanity', 'D0'])


def test_oracle_layout_is_point_to_bytes():
    """vanity_cases.oracle_rows lays the derived keys out as the codec does."""
    from upow_amd.utils.codec import AddressFormat, point_to_bytes
    base = 0x1234567 << 100
    rows = oracle_addresses(base, 9)
    assert rows == [point_to_bytes(op.public_key(base + i), AddressFormat.COMPRESSED) for i in range(9)]
