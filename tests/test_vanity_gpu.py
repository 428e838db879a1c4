"""K16 vanity search on the GPU: the device walk against the host derivation at every launch shape, the device
search against the host search, and two searches in a row."""
import asyncio
import json
import random

import numpy as np
import pytest

from upow_amd.ops import p256 as op
from upow_amd.ops.native import gpu_available, lib
from upow_amd.utils.codec import point_to_string
from upow_amd.utils.p256 import N
from upow_amd.wallet import vanity
from vanity_cases import (B, E2E_BASE, E2E_COUNT, E2E_FIRST, E2E_PREFIX, EDGE_BASE, EDGE_COUNT, HI, INFO, LO, be32,
                          edge_cases, oracle_addresses, oracle_rows, search)

pytestmark = pytest.mark.gpu
L = INFO['lanes_per_block']


@pytest.fixture(scope='module', autouse=True)
def device():
    if not gpu_available():
        pytest.fail('gpu-marked test ran without a visible HIP device')


def walk(base, count, **kw):
    return np.frombuffer(lib().p256_vanity_walk(be32(base), count, True, 8, **kw), dtype=np.uint8).reshape(count, 33)


# one batch; a partial wave; a partial block; two blocks and one lane of a third
SHAPES = [1, B - 1, B, B + 1, 64 * B - 1, 64 * B + 1, L * B + 1, 2 * L * B + 1]


@pytest.mark.parametrize('count', SHAPES)
def test_walk_matches_host(count):
    for base in (1, N - count, random.Random(count).randrange(1, N - count)):
        want = oracle_rows(base, count)
        got = walk(base, count)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (hex(base), count, bad[:8])


def test_walk_across_launches_and_steps():
    """keys_per_launch is far above the shapes of this file, so the launch levers shrink a launch: three launches of
    one batch per lane; launches of 64 lanes with three batches each (the centre advance); and 64 lanes with six
    batches each in one launch, from the scalar whose first advance is a doubling."""
    assert INFO['keys_per_launch'] > 2 * L * B + 1
    count = 2 * L * B + 1
    for base, kw in [(1, dict(launch_keys=L * B)), (N - count, dict(launch_keys=L * B)),
                     (7 << 230, dict(launch_keys=64 * 3 * B, launch_lanes=64)),
                     (N - count, dict(launch_keys=64 * 3 * B, launch_lanes=64))]:
        assert (walk(base, count, **kw) == oracle_rows(base, count)).all(), (hex(base), kw)
    count = 64 * 6 * B - 2
    for base in ((B + 1) // 2, N - count):
        assert (walk(base, count, launch_lanes=64) == oracle_rows(base, count)).all(), hex(base)


@pytest.mark.parametrize('lanes', [300, 1536])
def test_walk_when_a_later_launch_has_more_lanes(lanes):
    """launch_keys one above a whole number of batches per lane: the first launch takes two batches per lane on
    half the lanes (1 and 4 blocks), the second, one key shorter, one batch per lane on all of them (2 and 6
    blocks). The workspace has to hold the larger launch."""
    launch_keys = lanes * B + 1
    count = 2 * launch_keys - 1
    for base in (1, N - count):
        got = walk(base, count, launch_keys=launch_keys, launch_lanes=lanes)
        assert (got == oracle_rows(base, count)).all(), (hex(base), lanes)
    evens = [(LO, 43 << 256)]
    assert search(E2E_BASE, count, evens, max_hits=count, gpu=True, launch_keys=launch_keys, launch_lanes=lanes) \
        == search(E2E_BASE, count, evens, max_hits=count)


def test_search_matches_host_search():
    addresses = oracle_addresses(EDGE_BASE, EDGE_COUNT)
    for ranges, want in edge_cases(addresses):
        got = search(EDGE_BASE, EDGE_COUNT, ranges, gpu=True)
        assert got == (len(want), want) == search(EDGE_BASE, EDGE_COUNT, ranges), ranges
    # hit-buffer overflow: the count stays exact, the indexes are distinct hits
    total, idx = search(EDGE_BASE, EDGE_COUNT, [(LO, HI)], max_hits=7, gpu=True)
    assert total == EDGE_COUNT and len(set(idx)) == 7 and idx == sorted(idx) and idx[-1] < EDGE_COUNT
    evens = [(LO, 43 << 256)]
    want = search(EDGE_BASE, EDGE_COUNT, evens)
    total, idx = search(EDGE_BASE, EDGE_COUNT, evens, max_hits=5, gpu=True)
    assert total == want[0] and len(idx) == 5 and set(idx) <= set(want[1])
    # the same across launches
    assert search(EDGE_BASE, EDGE_COUNT, evens, gpu=True, launch_keys=B) == want
    assert search(5, 0, evens, gpu=True) == (0, [])
    with pytest.raises(ValueError):
        search(0, 5, evens, gpu=True)


def test_search_end_to_end_prefix():
    ranges = vanity.prefix_ranges(E2E_PREFIX)
    host = op.vanity_search(E2E_BASE, E2E_COUNT, ranges, device='cpu')
    dev = op.vanity_search(E2E_BASE, E2E_COUNT, ranges, device='gpu')
    assert dev[0] == host[0] and (dev[1] == host[1]).all() and int(dev[1][0]) == E2E_FIRST
    d, address = vanity.find(E2E_PREFIX, base=E2E_BASE, device='gpu', max_keys=E2E_COUNT)
    assert d == E2E_BASE + E2E_FIRST and address.startswith(E2E_PREFIX)
    assert point_to_string(op.public_key(d)) == address
    assert vanity.find('E55555', base=E2E_BASE, device='gpu', max_keys=E2E_COUNT, chunk=1 << 15) is None


def test_two_searches_in_a_row():
    """A stale hit counter, hit buffer or workspace would change the second answer."""
    ranges = [(LO, 43 << 256)]
    first = search(EDGE_BASE, EDGE_COUNT, ranges, gpu=True)
    other = search(E2E_BASE, 2 * L * B + 1, [(LO, HI)], max_hits=3, gpu=True)
    assert other[0] == 2 * L * B + 1 and len(other[1]) == 3
    assert search(EDGE_BASE, EDGE_COUNT, ranges, gpu=True) == first == search(EDGE_BASE, EDGE_COUNT, ranges)


def test_cli_on_the_gpu(tmp_path, monkeypatch, capsys):
    """Both commands find, re-verify and store keys through the GPU search."""
    monkeypatch.setenv('UPOW_DATA_DIR', str(tmp_path))
    monkeypatch.setenv('UPOW_KEY_FILE', str(tmp_path / 'keys.json'))
    from upow_amd import tools
    from upow_amd.ledger.database import Database
    from upow_amd.wallet import cli
    assert op.vanity_on_gpu()
    out = tmp_path / 'vanity.json'
    assert tools.main(['vanity', 'DvA', '--count', '2', '--out', str(out), '--device', 'gpu']) == 0
    db = asyncio.run(Database.create(utxo_backend='host'))
    try:
        asyncio.run(cli.main(['createwallet', '--prefix', 'dVa', '--ignore-case']))
    finally:
        db.close()
    found = json.loads(out.read_text())['keys'] + json.loads((tmp_path / 'keys.json').read_text())['keys']
    assert len(found) == 3
    for kp in found:
        address = point_to_string(op.public_key(int(kp['private_key'])))
        assert address == kp['public_key'] and address.lower().startswith('dva')
    assert all(kp['public_key'].startswith('DvA') for kp in found[:2])


def test_window_zero_of_the_table_is_b_times_g():
    """The walk reads j G from window 0 of the 16-bit fixed-base table: entries 1 .. B and the last one, 65535 G."""
    raw = lib().p256_g16_entries(1, B)
    for b in list(range(1, B + 1)) + [65535]:
        e = raw[64 * (b - 1):64 * b] if b <= B else lib().p256_g16_entries(b, 1)
        q = op.public_key(b)
        assert e == q.x.to_bytes(32, 'little') + q.y.to_bytes(32, 'little'), b
