"""UTXO proofs on the host: the native host twin (``utxo_merkle_build_records_host``) and the ``host`` /
``host-py`` indices against the hashlib reference ``merkle_of`` / ``prove_of`` (the RFC's recursive definition),
that reference against a level-by-level tree written here, every leaf's proof, absence proofs, what
``verify_outpoint`` refuses, and the ``utxo-root`` / ``utxo-proof`` tools."""
import asyncio
import copy
import json

import numpy as np
import pytest

from state_digest_cases import arrays, chain, small_ledger  # noqa: F401
from upow_amd.ledger import utxo_proof
from upow_amd.ledger.utxo import MerkleSnapshot, UtxoIndex, entries_of, merkle_of, prove_of, records_merkle
from upow_amd.ledger.utxo_proof import OutpointProof, ProofError, verify_leaf, verify_outpoint
from utxo_merkle_cases import SIZES, absent_outpoints, check_snapshot, level_by_level, outpoint, pool, sort_entries


@pytest.fixture(scope='module')
def entries():
    return pool()


def test_reference_against_level_by_level(entries):
    recs, pay = entries
    for n in SIZES:
        assert merkle_of(recs[:n], pay[:n]) == level_by_level(entries_of(recs[:n], pay[:n]))
    assert merkle_of(recs[:0], None) == (bytes.fromhex('e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855'), 0)
    srecs, spay = arrays(sort_entries())
    assert merkle_of(srecs, spay) == level_by_level(entries_of(srecs, spay))
    assert merkle_of(srecs, None) == level_by_level(entries_of(srecs, None)) != merkle_of(srecs, spay)
    assert merkle_of(srecs[::-1], spay[::-1]) == merkle_of(srecs, spay)  # a set: the order given does not count


@pytest.mark.parametrize('threads', [1, 8])
@pytest.mark.parametrize('n', SIZES)
def test_host_twin(native, entries, n, threads):
    """``utxo_merkle_build_records_host`` itself (no fall-back to the reference), and ``records_merkle`` on top."""
    recs, pay = np.ascontiguousarray(entries[0][:n]), np.ascontiguousarray(entries[1][:n])
    queries = None if n <= 65 else [outpoint(r) for r in recs[::37]] + absent_outpoints(recs)
    with MerkleSnapshot(native, native.utxo_merkle_build_records_host(recs, pay.view(np.uint8), threads)) as snap:
        info = native.utxo_merkle_info(snap._sid)
        assert (info['root'], info['count'], info['on_device']) == (snap.root, n, False)
        assert not snap.on_device and (snap.nbytes > 0) == (n > 0)
        check_snapshot(snap, recs, pay, queries)
        assert (snap.root, snap.count) == level_by_level(entries_of(recs, pay))
        assert snap.prove([]) == []
    with MerkleSnapshot(native, native.utxo_merkle_build_records_host(recs, None, threads)) as snap:
        assert (snap.root, snap.count) == merkle_of(recs, None)
    with records_merkle(recs, pay, device='cpu', threads=threads) as snap:
        assert snap._sid is not None and (snap.root, snap.count) == merkle_of(recs, pay)


@pytest.mark.parametrize('backend', ['host', 'host-py'])
@pytest.mark.parametrize('n', SIZES)
def test_index_backends(entries, backend, n):
    """The ``host`` and ``host-py`` indices at every size, against ``merkle_of`` / ``prove_of`` and, since ``host-py``
    runs the reference's own tree, against the level-by-level computation of this suite too."""
    recs, pay = entries
    idx = UtxoIndex(backend=backend)
    idx.insert_records(recs[:n], pay[:n])
    assert type(idx.be).__name__ == {'host': '_NativeHostBackend', 'host-py': '_HostBackend'}[backend]
    queries = None if n <= 65 else [outpoint(r) for r in recs[:n:37]] + absent_outpoints(recs[:n])
    with idx.merkle_snapshot() as snap:
        assert (snap._sid is None) == (backend == 'host-py')
        got = check_snapshot(snap, recs[:n], pay[:n], queries)
        assert (snap.root, snap.count) == level_by_level(entries_of(recs[:n], pay[:n]))
        for p in got:  # each path leads to the level-by-level root too
            for leaf in p.leaves:
                assert verify_leaf(snap.root, n, leaf.position, leaf.entry, leaf.path)
    keep = np.isin(recs[:n, 36], (1, 2, 3, 4, 5, 6))
    with idx.merkle_snapshot((1, 2, 3, 4, 5, 6)) as snap:
        assert (snap.root, snap.count) == merkle_of(recs[:n][keep], pay[:n][keep])
        assert (snap.root, snap.count) == level_by_level(entries_of(recs[:n][keep], pay[:n][keep]))


def test_sort_cases():
    recs, pay = arrays(sort_entries())
    with records_merkle(recs, pay, device='cpu') as snap:
        got = check_snapshot(snap, recs, pay)
    keys = [e[:34] for e in entries_of(recs, pay)]
    assert len(set(keys)) == len(keys)
    both = got[[outpoint(r) for r in recs].index(('ff' * 32, 9))]
    assert both.present and [x.entry[33] for x in both.leaves] == [0, 6]  # one outpoint under two tags: both leaves
    assert both.leaves[1].position == both.leaves[0].position + 1
    assert [len(e) for e in entries_of(recs, pay)].count(44) == 2


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_leaf_verifies(entries, n):
    recs, pay = entries[0][:n], entries[1][:n]
    root, count = merkle_of(recs, pay)
    proofs = prove_of(recs, pay, [outpoint(r) for r in recs])
    lengths = set()
    for p, r in zip(proofs, recs):
        assert p.present and len(p.leaves) == 1
        leaf = p.leaves[0]
        assert verify_leaf(root, count, leaf.position, leaf.entry, leaf.path)
        assert not verify_leaf(root, count, leaf.position, leaf.entry, leaf.path + [bytes(32)])
        assert not verify_leaf(root, count, leaf.position, leaf.entry, leaf.path[:-1]) or n == 1
        found = verify_outpoint(root, count, *outpoint(r), p)
        assert (found['tx_hash'], found['index'], found['tag']) == (*outpoint(r), int(r[36]))
        lengths.add(len(leaf.path))
    assert max(lengths) == (n - 1).bit_length()
    if n in (3, 5, 9):  # the promoted last leaf has the shortest path
        last = max(proofs, key=lambda p: p.leaves[0].position).leaves[0]
        assert last.position == n - 1 and len(last.path) == min(lengths) < max(lengths)


def test_absence_proofs(entries):
    recs, pay = entries[0][:9], entries[1][:9]
    root, count = merkle_of(recs, pay)
    order = sorted(outpoint(r) for r in recs)
    first, last = order[0], order[-1]
    mid = order[4]
    between = (mid[0], mid[1] + 1 if mid[1] < 255 else 254)
    assert between not in order
    before, after = ('00' * 32, 0), ('ff' * 32, 255)
    proofs = prove_of(recs, pay, [before, after, between])
    for q, p, npos in zip([before, after, between], proofs, [[0], [8], None]):
        assert not p.present and verify_outpoint(root, count, *q, p) is None
        if npos is not None:
            assert [x.position for x in p.leaves] == npos
        else:
            assert len(p.leaves) == 2 and p.leaves[1].position == p.leaves[0].position + 1
    assert bytes.fromhex(first[0]) > bytes(32) and bytes.fromhex(last[0]) < b'\xff' * 32
    # the empty set
    root0, count0 = merkle_of(recs[:0], None)
    p0 = prove_of(recs[:0], None, [before])[0]
    assert not p0.present and p0.leaves == [] and verify_outpoint(root0, 0, *before, p0) is None
    with pytest.raises(ProofError):
        verify_outpoint(root, count, *before, p0)  # no neighbour named in a non-empty set
    with pytest.raises(ProofError):
        verify_outpoint(root, 0, *before, p0)  # the empty set has another root


def test_verify_outpoint_refuses(entries):
    recs, pay = entries[0][:9], entries[1][:9]
    root, count = merkle_of(recs, pay)
    order = sorted(range(9), key=lambda k: outpoint(recs[k]))
    k = next(i for i in order[1:8] if int(pay['len'][i]) in (33, 64))
    q = outpoint(recs[k])
    present = prove_of(recs, pay, [q])[0]
    mid = outpoint(recs[order[4]])
    gap = (mid[0], mid[1] + 1 if mid[1] < 255 else 254)
    absent = prove_of(recs, pay, [gap])[0]
    assert verify_outpoint(root, count, *q, present)['amount'] == int(pay['amount'][k])
    assert verify_outpoint(root, count, *q, present.to_json())['amount'] == int(pay['amount'][k])
    assert verify_outpoint(root, count, *gap, absent) is None and len(absent.leaves) == 2

    def refused(query, proof, c=count):
        with pytest.raises(ProofError):
            verify_outpoint(root, c, *query, proof)

    bad = copy.deepcopy(present)  # a flipped path byte
    bad.leaves[0].path[0] = bytes([bad.leaves[0].path[0][0] ^ 1]) + bad.leaves[0].path[0][1:]
    refused(q, bad)
    bad = copy.deepcopy(present)  # a changed amount in E
    e = bytearray(bad.leaves[0].entry)
    e[36] ^= 1
    bad.leaves[0].entry = bytes(e)
    refused(q, bad)
    # a wrong count, shown on the last leaf: its path has the shape of a 9-leaf tree only (a path further left can
    # fit a neighbouring count too: the count is part of the commitment, compared with the root)
    q_last = outpoint(recs[order[8]])
    p_last = prove_of(recs, pay, [q_last])[0]
    assert verify_outpoint(root, count, *q_last, p_last) is not None
    refused(q_last, p_last, count + 1)
    refused(q_last, p_last, count - 1)  # and a position at the count
    refused(q, present, present.leaves[0].position)
    bad = copy.deepcopy(absent)  # neighbours swapped
    bad.leaves.reverse()
    refused(gap, bad)
    far = prove_of(recs, pay, [outpoint(recs[order[0]]), outpoint(recs[order[8]])])  # neighbours not adjacent
    refused(gap, OutpointProof(*gap, False, [far[0].leaves[0], far[1].leaves[0]]))
    other = outpoint(recs[order[0]])  # a "present" proof reused for another outpoint
    refused(other, present)
    refused(other, OutpointProof(*other, True, present.leaves))
    # an absence proof whose neighbours do not bracket the query: the gap's proof for an outpoint elsewhere
    elsewhere = ('00' * 32, 0)
    refused(elsewhere, OutpointProof(*elsewhere, False, absent.leaves))
    refused(q, OutpointProof(*q, False, absent.leaves if q != mid else present.leaves))
    refused(gap, OutpointProof(*gap, False, absent.leaves[:1]))  # a missing neighbour
    refused(gap, OutpointProof(*gap, False, []))
    bad = copy.deepcopy(present)  # an E of impossible length
    bad.leaves[0].entry = bad.leaves[0].entry[:-1]
    refused(q, bad)
    refused(q, OutpointProof(*q, True, []))
    # the readable fields are not what is verified
    doc = present.to_json()
    doc['leaves'][0]['decoded']['amount'] = 1
    assert verify_outpoint(root, count, *q, doc)['amount'] == int(pay['amount'][k])


def test_tools_root_and_proof_round_trip(chain, monkeypatch, capsys, tmp_path):  # noqa: F811
    from upow_amd import tools
    from upow_amd.ledger import snapshot
    asyncio.run(small_ledger(chain))
    recs, pay = chain.utxo.records_payload()
    root, count = merkle_of(recs, pay)
    assert count == len(chain.utxo) > 6

    async def opened(path=None):
        return chain
    monkeypatch.setattr(tools, 'open_ledger', opened)
    capsys.readouterr()
    assert tools.main(['utxo-root']) == 0
    line = json.loads(capsys.readouterr().out)
    assert (line['root'], line['count'], line['backend']) == (root.hex(), count, 'host')
    path = tmp_path / 'snap.bin'
    snapshot.save(chain, str(path))
    assert tools.main(['utxo-root', '--snapshot', str(path)]) == 0
    line = json.loads(capsys.readouterr().out)
    assert (line['root'], line['count']) == (root.hex(), count)

    live = [outpoint(r) for r in recs[:3]]
    gone = ('12' * 32, 7)
    out = tmp_path / 'proofs.json'
    args = [f'{h}:{i}' for h, i in live + [gone]]
    assert tools.main(['utxo-proof', *args, '--out', str(out)]) == 0
    capsys.readouterr()
    doc = json.loads(out.read_text())
    assert (doc['root'], doc['count'], len(doc['proofs'])) == (root.hex(), count, 4)
    assert tools.main(['utxo-proof', '--check', str(out), '--root', root.hex(), '--count', str(count)]) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines()]
    assert [x['result'] for x in lines[:-1]] == ['present'] * 3 + ['absent'] and lines[-1]['ok'] is True
    assert lines[0]['entries'][0]['table'] in utxo_proof.TABLE_BY_TAG.values()
    assert tools.main(['utxo-proof', '--check', str(out)]) == 0
    capsys.readouterr()
    assert tools.main(['utxo-proof', '--check', str(out), '--root', '00' * 32, '--count', str(count)]) == 1
    assert json.loads(capsys.readouterr().out.splitlines()[-1])['failed'] == 4
    assert tools.main(['utxo-proof', *args[:1], '--snapshot', str(path)]) == 0
    assert json.loads(capsys.readouterr().out)['proofs'][0] == doc['proofs'][0]
    with pytest.raises(SystemExit):
        tools.main(['utxo-proof'])
    with pytest.raises(SystemExit):
        tools.main(['utxo-proof', '--check', str(out), '--root', root.hex()])
