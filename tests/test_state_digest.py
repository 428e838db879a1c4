"""State digest (``UtxoIndex.state_digest``, ``records_digest``: LtHash16/1024 over every live entry with its
payload) on the host: the known answers as literals through the Python reference, the native host routine and the
``host`` / ``host-py`` indices; the algebra (order, union, insert - erase); ``tools utxo-digest`` and the snapshot
header key. ``tests/test_state_digest_gpu.py`` runs the HBM passes against the same reference."""
import asyncio
import hashlib
import json

import numpy as np
import pytest

from state_digest_cases import (C_NOISE, ENTRY, KNOWN, arrays, chain, check_known, random_entries,  # noqa: F401
                                small_ledger)
from upow_amd.ledger.utxo import StateDigest, UtxoIndex, records_digest, state_digest_of

BACKENDS = ['host', 'host-py']


@pytest.fixture(scope='module')
def big():
    """1,500 random entries and their reference digest, computed once."""
    recs, pay = arrays(random_entries(1500, 71))
    tags = recs[:, 36]
    assert set(tags.tolist()) == set(range(7)) and {0, 33, 64} == set(pay['len'].tolist())
    assert {0, 255} <= set(recs[:, 32].tolist()) and pay['flags'].any()
    return recs, pay, state_digest_of(recs, pay)


def host_native(native, recs, pay, threads=1):
    return StateDigest(*native.utxo_records_digest_host(recs, None if pay is None else pay.view(np.uint8), threads))


@pytest.mark.parametrize('names', list(KNOWN))
def test_known_answers(native, names):
    recs, pay = arrays([ENTRY[x] for x in names])
    check_known(names, state_digest_of(recs, pay))
    check_known(names, host_native(native, recs, pay))
    check_known(names, records_digest(recs, pay, device='cpu'))
    for backend in BACKENDS:
        idx = UtxoIndex(backend=backend)
        idx.insert_records(recs, pay)
        check_known(names, idx.state_digest())


def test_canonical_payload(native):
    """Nothing of a payload whose length is neither 33 nor 64 is hashed: C with a flag, an amount and three
    address bytes is C; so is C inserted without payload."""
    recs, pay = arrays([C_NOISE])
    assert pay['len'][0] == 3 and pay['amount'][0] == 999
    for d in (state_digest_of(recs, pay), host_native(native, recs, pay), state_digest_of(recs, None),
              host_native(native, recs, None), records_digest(recs, None, device='cpu')):
        check_known(('C',), d)
    for backend in BACKENDS:
        idx = UtxoIndex(backend=backend)
        idx.insert_records(recs, None)
        check_known(('C',), idx.state_digest())


def test_random_entries_threads_order(native, big):
    """1,500 entries are 94 work items of the host routine, above the 64 below which the pool keeps a region on
    the caller: with 3 and 16 threads the per-item accumulators and the locked merge run concurrently."""
    recs, pay, want = big
    got = [host_native(native, recs, pay, t) for t in (1, 3, 16)]
    assert all(g.tobytes() == want.tobytes() and g.count == 1500 for g in got)
    order = np.random.default_rng(5).permutation(len(recs))
    assert host_native(native, np.ascontiguousarray(recs[order]), np.ascontiguousarray(pay[order]), 3) == want
    assert state_digest_of(recs[order][:200], pay[order][:200]) == host_native(
        native, np.ascontiguousarray(recs[order][:200]), np.ascontiguousarray(pay[order][:200]), 3)
    assert host_native(native, recs, None, 3) == state_digest_of(recs, None) != want


def test_empty_and_union(native, big):
    recs, pay, want = big
    zero = host_native(native, recs[:0], pay[:0], 4)
    assert zero == StateDigest() == state_digest_of(recs[:0], pay[:0]) and not zero.state.any() and zero.count == 0
    x, y = host_native(native, recs[:700], pay[:700], 3), host_native(native, recs[700:], pay[700:], 3)
    assert x + y == want and want - y == x and (x + y).hex() == want.hex()
    assert x != want and x.hex() != want.hex()
    assert (zero - x) + x == zero  # lanes wrap modulo 2^16, the count goes through -700


@pytest.mark.parametrize('backend', BACKENDS)
def test_index_insert_erase_tags(native, big, backend):
    recs, pay, _ = big
    idx = UtxoIndex(backend=backend)
    idx.insert_records(recs[:300], pay[:300])
    d300 = host_native(native, recs[:300], pay[:300])
    assert idx.state_digest() == d300
    assert idx.erase_records(np.ascontiguousarray(recs[100:200])).all()
    assert idx.state_digest() == d300 - host_native(native, recs[100:200], pay[100:200])
    left = np.r_[0:100, 200:300]
    for tags in ((0,), (1, 2, 3, 4, 5, 6), None):
        keep = left if tags is None else left[np.isin(recs[left, 36], tags)]
        assert idx.state_digest(tags) == state_digest_of(recs[keep], pay[keep])
    with pytest.raises(ValueError):
        idx.state_digest((32,))


def test_every_field_counts():
    base = ENTRY['B']
    want = state_digest_of(*arrays([base])).hex()
    txid, index, tag, flags, amount, addr = base
    changed = [(txid, index, tag, flags, amount ^ (1 << 40), addr),
               (txid, index, tag, flags, amount, addr[:63] + bytes([addr[63] ^ 1])),
               (txid, index, tag, flags ^ 1, amount, addr),
               (txid, index, 3, flags, amount, addr),
               (txid, index - 1, tag, flags, amount, addr),
               (bytes([txid[0] ^ 0x80]) + txid[1:], index, tag, flags, amount, addr)]
    ids = [state_digest_of(*arrays([e])).hex() for e in changed]
    assert len(set(ids + [want])) == len(changed) + 1


def test_tools_utxo_digest_and_snapshot_header(chain, monkeypatch, capsys, tmp_path):  # noqa: F811
    from upow_amd import tools
    from upow_amd.ledger import snapshot
    asyncio.run(small_ledger(chain))
    live = chain.utxo.state_digest()
    assert live.count == len(chain.utxo) > 0 and live == state_digest_of(*chain.utxo.records_payload())

    async def opened(path=None):
        return chain
    monkeypatch.setattr(tools, 'open_ledger', opened)
    capsys.readouterr()
    assert tools.main(['utxo-digest']) == 0
    line = json.loads(capsys.readouterr().out)
    assert set(line) == {'digest', 'entries', 'backend', 'seconds'}
    assert (line['digest'], line['entries'], line['backend']) == (live.hex(), live.count, 'host')
    assert tools.main(['utxo-digest', '--full']) == 0
    assert bytes.fromhex(json.loads(capsys.readouterr().out)['state']) == live.tobytes()

    # the status of a rank: on a host backend the key is there under deep only; the other keys stay
    from upow_amd.parallel import cluster
    quick, deep = asyncio.run(cluster.status_all(chain)), asyncio.run(cluster.status_all(chain, deep=True))
    assert 'state_digest' not in quick[0] and deep[0]['state_digest'] == live.hex()
    assert {k: v for k, v in deep[0].items() if k != 'state_digest'} == quick[0]
    assert quick[0]['utxo_hash'] == chain.utxo.set_hash(0) and quick[0]['utxo_entries'] == live.count

    path = tmp_path / 'snap.bin'
    monkeypatch.setattr(snapshot, 'DIGEST_SLICE', 3)  # the save sums the digests of several slices
    assert live.count > 6 and {33, 64} <= set(chain.utxo.records_payload()[1]['len'].tolist())
    header = snapshot.save(chain, str(path))
    assert header['state_digest'] == live.hex()
    assert json.loads(path.read_bytes().split(b'\n', 1)[0])['state_digest'] == live.hex()
    assert tools.main(['utxo-digest', '--snapshot', str(path)]) == 0
    line = json.loads(capsys.readouterr().out)
    assert line['match'] is True and line['snapshot_digest'] == line['digest'] == live.hex()

    # one amount bit patched in the file, the payload checksum recomputed: K12 and the checksum pass, the digest
    # does not
    head, body = path.read_bytes().split(b'\n', 1)
    hdr, n = json.loads(head), header['count']
    body = bytearray(body)
    k = next(i for i in range(n) if int.from_bytes(body[40 * n + 80 * i + 8:40 * n + 80 * i + 12], 'little') == 33)
    body[40 * n + 80 * k] ^= 1
    hdr['payload_sha256'] = hashlib.sha256(bytes(body)).hexdigest()
    bad = tmp_path / 'patched.bin'
    bad.write_bytes(json.dumps(hdr, separators=(',', ':')).encode() + b'\n' + bytes(body))
    assert snapshot.read(str(bad))[0]['utxo_hash'] == header['utxo_hash']
    assert tools.main(['utxo-digest', '--snapshot', str(bad)]) == 1
    line = json.loads(capsys.readouterr().out)
    assert line['match'] is False and line['digest'] == live.hex() != line['snapshot_digest']

    # a file from before the key existed still loads
    del hdr['state_digest']
    hdr['payload_sha256'] = header['payload_sha256']
    old = tmp_path / 'old.bin'
    old.write_bytes(json.dumps(hdr, separators=(',', ':')).encode() + b'\n' + path.read_bytes().split(b'\n', 1)[1])
    assert snapshot.try_restore(chain, str(old)) and chain.utxo.state_digest() == live
