"""Operator tools.

``python -m upow_amd.tools rebuild-utxo``: rebuild the UTXO set by replaying every transaction in
block order (reference: create_unspent_outputs.py:9-45, database.py:846-862).
``python -m upow_amd.tools utxo-hash``: print the UTXO-set hash served at ``GET /``.
``python -m upow_amd.tools snapshot [--out FILE]``: checkpoint the UTXO index at the tip (ledger/snapshot.py).
``python -m upow_amd.tools verify-utxo``: audit the UTXO index against the SQL tables (K12 hash + sets).
``python -m upow_amd.tools address-utxos ADDRESS [ADDRESS ...]``: each address's live outputs in all seven output
tables, one JSON line per address, straight from the UTXO index (on a GPU node ONE ``utxo_address_scan_batch``
pass over the HBM table for all of them, K14).
``python -m upow_amd.tools holders [--top N] [--by COL[,COL...]] [--db PATH] [--out FILE]``: who holds what. One
JSON line per public key (both address forms folded): its spendable balance, stake and governance outputs, from
one pass over the UTXO index (on a GPU node a hash aggregation over the HBM table, ``utxo_owner_totals``); every
holder ascending by key, or with ``--top N`` the N greatest by the sum of the ``--by`` columns (default
``spendable,stake``). The holder lines go to ``--out FILE`` when given; the last line printed is the summary
``{"holders", "outputs", "skipped", "totals", "backend"}`` over the whole set. Exit status 1 when entries were
skipped (indexed without their payload, so nobody can be credited with them).
``python -m upow_amd.tools utxo-digest [--db PATH] [--snapshot FILE] [--full]``: the state digest of the UTXO index
(``UtxoIndex.state_digest``: LtHash16/1024 over every live entry of all seven tables WITH its amount, address and
stake flag; on a GPU node one pass over the HBM table, ``utxo_state_digest``). One JSON line ``{"digest", "entries",
"backend", "seconds"}``, ``digest`` being the short id; ``--full`` adds ``"state"``, the 2048 bytes as hex. Two
replicas, or a replica and a snapshot, hold the same set exactly when their lines agree. With ``--snapshot FILE`` the
line also carries ``"snapshot_digest"`` (of the file's records and payloads, ``records_digest``) and ``"match"``;
exit status 1 on a mismatch.
``python -m upow_amd.tools utxo-diff --snapshot F [--db PATH] [--limit N] [--out FILE]``: WHERE the UTXO index and a
snapshot file differ (``UtxoIndex.diff_records``; on a GPU node one pass over the HBM table, ``utxo_diff``).
``utxo-diff --sql [--db PATH] [--limit N] [--out FILE]``: the index against the ledger's own SQL tables, one bulk
query per table and one diff: the audit that scales. ``utxo-diff --snapshot A --against B``: two snapshot files (A
loaded into a scratch index). One JSON line per differing entry, to ``--out FILE`` when given: ``{"kind": "missing" |
"extra" | "changed", "tx_hash", "index", "table", "amount", "address", "is_stake"}``; ``missing`` is in the other set
and not in the index, ``extra`` the reverse, and a changed entry shows both sides as ``"other": {...}, "index_entry":
{...}``. Amounts are decimal strings, addresses the raw 33 or 64 bytes as hex; an entry without payload has nulls. At
most ``--limit`` (default 65536) lines per kind. The last line printed is the summary ``{"equal", "missing", "extra",
"changed", "compared", "entries", "truncated", "backend", "seconds"}`` with the exact counts. Exit status 1 unless
the sets are equal.
``python -m upow_amd.tools utxo-root [--db PATH] [--snapshot F]``: the Merkle commitment of the UTXO index over all
seven tables (``UtxoIndex.merkle_snapshot``; on a GPU node built in HBM, csrc/utxo_merkle.hip), or with
``--snapshot F`` of that file's records: one JSON line ``{"root", "count", "levels", "backend", "seconds"}``.
``python -m upow_amd.tools utxo-proof TXHASH:INDEX [...] [--db PATH] [--snapshot F] [--out F]``: for each outpoint
the proof that it is in that set with its amount and owner, or that it is not, as one JSON document ``{"root",
"count", "backend", "proofs"}`` (to ``--out F`` when given). ``utxo-proof --check FILE [--root HEX --count N]``
verifies such a document offline with ledger/utxo_proof.py alone, against the commitment given (without one, against
the document's own, which shows that it is consistent and no more): one line per outpoint, then the summary; exit
status 1 when a proof fails.
``python -m upow_amd.tools materialise --db <rankN ledger>``: bring a lean cluster follower's SQL tables to its
tip from its op log (ledger/lean.py); every other command does this first when the ledger has an op log.
``python -m upow_amd.tools sign-batch --keys F --digests F --out F [--device gpu|cpu]``: bulk RFC 6979 signing
(K15 batched, ops/p256.py sign_digests; not constant-time, for a machine the operator trusts). F are raw files:
32-byte big-endian private keys, 32-byte SHA-256 digests, and 64-byte ``r | s`` little-endian out. One JSON
line with counts and seconds; a key outside [1, n-1] gets 64 zero bytes and exit status 1.
``python -m upow_amd.tools vanity PREFIX [--ignore-case] [--count K] [--max-keys N] [--out F] [--device gpu|cpu]``:
K private keys whose addresses start with PREFIX (K16, wallet/vanity.py; not constant-time, for a machine the
operator trusts), as JSON in the format of ``key_pair_list.json`` to F or standard output. The key store is not
touched. Exit status 1 when a search gave up after ``--max-keys`` keys.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import sys
from decimal import Decimal

from .constants import SMALLEST
from .ledger.database import Database


async def open_ledger(path: str = None) -> Database:
    """The ledger at ``path``, its SQL tables brought to the tip first when it is a lean follower's (op log)."""
    from .ledger import lean
    db = await Database.create(path=path)
    if lean.pending(db):
        n = await lean.materialise(db)
        print(f'materialised {n} block(s) from the op log', file=sys.stderr)
    return db


async def address_utxos(address: str, path: str = None, db: Database = None) -> dict:
    """Live outputs owned by ``address`` in all seven output tables, from the UTXO index (K14; one
    ``utxo_address_scan_batch`` pass for both address forms on a GPU node). Both string forms of the key
    are matched (compressed 33 B and full 64 B, like the reference's ``address = ANY(addresses)``).
    ``spendable`` is the reference's ``get_address_balance`` (database.py:1138-1160: unspent_outputs rows
    with is_stake NULL/0); ``stake`` and each governance table are summed separately."""
    return (await address_utxos_many([address], path, db))[0]


async def address_utxos_many(addresses, path: str = None, db: Database = None) -> list:
    """:func:`address_utxos` of each address, in the order given: every form of every address is one query
    of a single ``address_outputs_many`` call (one pass over the HBM table on a GPU node)."""
    from .ledger.utxo import STAKE_ANY, TABLE_BY_TAG
    from .utils.codec import address_search_hex
    db = db or await open_ledger(path)
    forms = []
    for address in addresses:
        try:
            forms.append([bytes.fromhex(h) for h in address_search_hex(address)])
        except Exception:
            raise SystemExit(f'not an address: {address}')
    res = iter(db.utxo.address_outputs_many([(raw, TABLE_BY_TAG, STAKE_ANY) for fs in forms for raw in fs]))
    out = []
    for address, fs in zip(addresses, forms):
        outputs = []
        sums = {'spendable': 0, 'stake': 0, **{t: 0 for t in TABLE_BY_TAG.values() if t != 'unspent_outputs'}}
        for raw in fs:
            recs, pay, _ = next(res)
            idx = recs[:, 32:36].copy().view('<u4').ravel()
            tag = recs[:, 36:40].copy().view('<u4').ravel()
            for k in range(len(recs)):
                table = TABLE_BY_TAG[int(tag[k])]
                stake = table == 'unspent_outputs' and bool(int(pay['flags'][k]) & 1)
                amount = int(pay['amount'][k])
                key = ('stake' if stake else 'spendable') if table == 'unspent_outputs' else table
                sums[key] += amount
                outputs.append({'tx_hash': bytes(recs[k, :32]).hex(), 'index': int(idx[k]), 'table': table,
                                'is_stake': stake, 'amount': str(Decimal(amount) / SMALLEST), 'form': len(raw)})
        outputs.sort(key=lambda o: (o['tx_hash'], o['index']))
        out.append({'address': address, 'backend': db.utxo.backend_name,
                    'spendable': str(Decimal(sums.pop('spendable')) / SMALLEST),
                    'stake': str(Decimal(sums.pop('stake')) / SMALLEST),
                    'tables': {t: str(Decimal(v) / SMALLEST) for t, v in sums.items()},
                    'total': str(Decimal(sum(int(Decimal(o['amount']) * SMALLEST) for o in outputs)) / SMALLEST),
                    'outputs': outputs})
    return out


async def holders(top: int = None, by=('spendable', 'stake'), path: str = None, db: Database = None):
    """The ``holders`` command's lines: (one dict per holder in order, the summary dict), amounts as strings
    (``Database.get_owner_totals``)."""
    db = db or await open_ledger(path)
    rows, summary = await db.get_owner_totals(top, tuple(by))
    lines = [{**r, 'spendable': str(r['spendable']), 'stake': str(r['stake']),
              'tables': {t: str(v) for t, v in r['tables'].items()}} for r in rows]
    return lines, {**summary, 'totals': {c: str(v) for c, v in summary['totals'].items()},
                   'backend': db.utxo.backend_name}


async def utxo_digest(path: str = None, snapshot_path: str = None, full: bool = False, db: Database = None) -> dict:
    """The ``utxo-digest`` command's line: the state digest of the index over all seven tables, and with
    ``snapshot_path`` that of the snapshot file's records and payloads next to it."""
    import time

    from .ledger.utxo import ALL_TAGS_MASK, _masked, records_digest
    db = db or await open_ledger(path)
    t = time.perf_counter()
    d = db.utxo.state_digest()
    res = {'digest': d.hex(), 'entries': d.count, 'backend': db.utxo.backend_name,
           'seconds': round(time.perf_counter() - t, 6)}
    if full:
        res['state'] = d.tobytes().hex()
    if snapshot_path:
        from .ledger import snapshot
        _, recs, pay = snapshot.read(snapshot_path)
        sd = records_digest(*_masked(recs, pay, ALL_TAGS_MASK))
        res['snapshot_digest'] = sd.hex()
        res['match'] = sd == d
    return res


async def _merkle_snapshot(path: str = None, snapshot_path: str = None, db: Database = None):
    """(Merkle snapshot, backend name) of the index over all seven tables, or of a snapshot file's records and
    payloads (built on the GPU when there is one)."""
    from .ledger.utxo import ALL_TAGS_MASK, _masked, records_merkle
    if snapshot_path:
        from .ledger import snapshot
        _, recs, pay = snapshot.read(snapshot_path)
        snap = records_merkle(*_masked(recs, pay, ALL_TAGS_MASK))
        return snap, 'gpu' if snap.on_device else 'host'
    db = db or await open_ledger(path)
    return db.utxo.merkle_snapshot(), db.utxo.backend_name


async def utxo_root(path: str = None, snapshot_path: str = None, db: Database = None) -> dict:
    """The ``utxo-root`` command's line: the Merkle commitment ``(root, count)`` of the index, or of a snapshot
    file."""
    import time
    t = time.perf_counter()
    snap, backend = await _merkle_snapshot(path, snapshot_path, db)
    with snap:
        return {'root': snap.root.hex(), 'count': snap.count, 'levels': snap.levels, 'backend': backend,
                'seconds': round(time.perf_counter() - t, 6)}


async def utxo_proofs(outpoints, path: str = None, snapshot_path: str = None, db: Database = None) -> dict:
    """The ``utxo-proof`` command's document: the commitment and one proof per outpoint, in the order asked."""
    snap, backend = await _merkle_snapshot(path, snapshot_path, db)
    with snap:
        return {'root': snap.root.hex(), 'count': snap.count, 'backend': backend,
                'proofs': [p.to_json() for p in snap.prove(outpoints)]}


def check_proofs(doc: dict, root_hex: str = None, count: int = None):
    """``utxo-proof --check``: verify a ``utxo-proof`` document offline with ledger/utxo_proof.py alone, against
    the commitment given (else the document's own, which shows consistency only). One line per outpoint and the
    summary ``{"ok", "root", "count", "present", "absent", "failed"}``."""
    from .ledger import utxo_proof
    root = bytes.fromhex(root_hex if root_hex is not None else doc['root'])
    count = int(doc['count'] if count is None else count)
    lines, tally = [], {'present': 0, 'absent': 0, 'failed': 0}
    for p in doc['proofs']:
        line = {'tx_hash': p.get('tx_hash'), 'index': p.get('index')}
        try:
            found = utxo_proof.verify_outpoint_all(root, count, p['tx_hash'], p['index'], p)
            line.update(result='present' if found else 'absent', entries=found)
            for e in found:
                e['amount'] = str(Decimal(e['amount']) / SMALLEST)
        except (utxo_proof.ProofError, KeyError, TypeError, ValueError) as e:
            line.update(result='failed', error=str(e))
        tally[line['result']] += 1
        lines.append(line)
    return lines, {'ok': tally['failed'] == 0, 'root': root.hex(), 'count': count, **tally}


def _diff_entry(rec, pay) -> dict:
    """One side of a diff line: the fields of an entry that the diff compares (no payload: nulls)."""
    from .ledger.utxo import TABLE_BY_TAG
    tag, length = int(rec[36]), int(pay['len'])
    known = length in (33, 64)
    return {'table': TABLE_BY_TAG.get(tag, str(tag)),
            'amount': str(Decimal(int(pay['amount'])) / SMALLEST) if known else None,
            'address': bytes(pay['addr'][:length]).hex() if known else None,
            'is_stake': bool(int(pay['flags']) & 1) if known else False}


async def utxo_diff(path: str = None, snapshot_path: str = None, sql: bool = False, against: str = None,
                    limit: int = None, db: Database = None):
    """The ``utxo-diff`` command's lines: (one dict per differing entry: missing, then extra, then changed, each
    in (tx_hash, index) order; the summary dict). The index (with ``against``: a scratch index loaded from the
    snapshot ``snapshot_path``) against the other set: the snapshot ``against``, else the ledger's SQL tables
    (``sql``), else the snapshot ``snapshot_path``."""
    import time

    from .ledger import snapshot
    from .ledger.utxo import DIFF_LIMIT, UtxoIndex
    if against:
        index = UtxoIndex()
        index.reset_records(*snapshot.read(snapshot_path)[1:])
        _, recs, pay = snapshot.read(against)
    else:
        db = db or await open_ledger(path)
        index = db.utxo
        recs, pay = db._utxo_arrays_from_sql() if sql else snapshot.read(snapshot_path)[1:]
    t = time.perf_counter()
    d = index.diff_records(recs, pay, limit=DIFF_LIMIT if limit is None else limit)
    seconds = time.perf_counter() - t
    lines = []
    for kind, (r, p) in (('missing', d.missing), ('extra', d.extra)):
        for k in range(len(r)):
            lines.append({'kind': kind, 'tx_hash': bytes(r[k, :32]).hex(), 'index': int(r[k, 32]),
                          **_diff_entry(r[k], p[k])})
    ro, po, ri, pi = d.changed
    for k in range(len(ro)):
        lines.append({'kind': 'changed', 'tx_hash': bytes(ro[k, :32]).hex(), 'index': int(ro[k, 32]),
                      'other': _diff_entry(ro[k], po[k]), 'index_entry': _diff_entry(ri[k], pi[k])})
    return lines, {'equal': d.equal, 'missing': d.n_missing, 'extra': d.n_extra, 'changed': d.n_changed,
                   'compared': d.compared, 'entries': d.entries, 'truncated': d.truncated,
                   'backend': index.backend_name, 'seconds': round(seconds, 6)}


async def rebuild_utxo(path: str = None):
    db = await open_ledger(path)
    outputs = await db.get_unspent_outputs_from_all_transactions()
    with db.transaction():
        db._x('DELETE FROM unspent_outputs')
    await db.add_unspent_outputs(sorted(outputs))
    await db.set_unspent_outputs_addresses()
    db._rebuild_utxo_index()
    print(f'{len(outputs)} unspent outputs; hash {await db.get_unspent_outputs_hash()}')
    return len(outputs)


def sign_batch(keys_path: str, digests_path: str, out_path: str, device: str = None) -> dict:
    """Sign digest i of ``digests_path`` with key i of ``keys_path`` into ``out_path``; the result line of the
    ``sign-batch`` command. Nothing read from the key file is printed or returned."""
    import time

    import numpy as np

    from .ops import p256
    from .utils.cpus import cpu_budget
    with open(keys_path, 'rb') as f:
        keys = f.read()
    with open(digests_path, 'rb') as f:
        digests = f.read()
    if len(keys) % 32 or len(digests) != len(keys):
        raise SystemExit('sign-batch: need n x 32 bytes of keys and as many of digests')
    n = len(keys) // 32
    gpu = p256._sign_on_gpu(n, device)
    t = time.perf_counter()
    out = p256.lib().p256_sign_many(keys, digests, gpu, max(1, min(cpu_budget(), 16))) if n else b''
    seconds = time.perf_counter() - t
    with open(out_path, 'wb') as f:
        f.write(out)
    failed = np.flatnonzero(~np.frombuffer(out, dtype=np.uint8).reshape(n, 64).any(axis=1))
    return {'signatures': n - int(failed.size), 'failed': int(failed.size),
            'first_failed': int(failed[0]) if failed.size else None, 'device': 'gpu' if gpu else 'cpu',
            'seconds': round(seconds, 6)}


def vanity_keys(prefix: str, ignore_case: bool = False, count: int = 1, max_keys: int = None, device: str = None) -> list:
    """``count`` key pairs whose addresses start with ``prefix``, each from a fresh random base; fewer when a
    search gave up after ``max_keys`` keys."""
    from .wallet import vanity
    keys = []
    for _ in range(count):
        found = vanity.find(prefix, ignore_case, device=device, max_keys=max_keys,
                            progress=vanity.progress_printer())
        if found is None:
            break
        keys.append({'private_key': found[0], 'public_key': found[1]})
    return keys


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('command', choices=['rebuild-utxo', 'utxo-hash', 'snapshot', 'verify-utxo', 'address-utxos',
                                        'holders', 'materialise', 'sign-batch', 'vanity', 'utxo-digest',
                                        'utxo-diff', 'utxo-root', 'utxo-proof'])
    ap.add_argument('address', nargs='*')
    ap.add_argument('--db', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--keys', default=None)
    ap.add_argument('--digests', default=None)
    ap.add_argument('--device', choices=['gpu', 'cpu'], default=None)
    ap.add_argument('--top', type=int, default=None)
    ap.add_argument('--by', default='spendable,stake')
    ap.add_argument('--ignore-case', action='store_true')
    ap.add_argument('--count', type=int, default=None)  # vanity: keys to find (1); utxo-proof --check: leaves
    ap.add_argument('--check', default=None)
    ap.add_argument('--root', default=None)
    ap.add_argument('--max-keys', type=int, default=None)
    ap.add_argument('--snapshot', default=None)
    ap.add_argument('--full', action='store_true')
    ap.add_argument('--sql', action='store_true')
    ap.add_argument('--against', default=None)
    ap.add_argument('--limit', type=int, default=None)
    a = ap.parse_args(argv)
    if a.command == 'sign-batch':
        if not (a.keys and a.digests and a.out):
            ap.error('sign-batch needs --keys, --digests and --out')
        res = sign_batch(a.keys, a.digests, a.out, a.device)
        print(json.dumps(res))
        return 1 if res['failed'] else 0
    elif a.command == 'vanity':
        a.count = 1 if a.count is None else a.count
        if len(a.address) != 1 or a.count < 1:
            ap.error('vanity needs one PREFIX and --count >= 1')
        from .wallet import vanity
        try:
            print(vanity.progress_line(a.address[0], a.ignore_case), file=sys.stderr)
        except ValueError as e:
            ap.error(str(e))
        keys = vanity_keys(a.address[0], a.ignore_case, a.count, a.max_keys, a.device)
        text = json.dumps({'keys': keys})
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text)
        else:
            print(text)
        return 0 if len(keys) == a.count else 1
    elif a.command == 'address-utxos':
        if not a.address:
            ap.error('address-utxos needs an ADDRESS')
        for res in asyncio.run(address_utxos_many(a.address, a.db)):  # one JSON line per address
            print(json.dumps(res))
    elif a.command == 'holders':
        if a.top is not None and a.top < 0:
            ap.error('--top is a count >= 0')
        try:
            lines, summary = asyncio.run(holders(a.top, [c for c in a.by.split(',') if c], a.db))
        except ValueError as e:
            ap.error(str(e))
        out = open(a.out, 'w') if a.out else sys.stdout
        try:
            for line in lines:  # one JSON line per holder
                print(json.dumps(line), file=out)
        finally:
            if a.out:
                out.close()
        print(json.dumps(summary))
        return 1 if summary['skipped'] else 0
    elif a.command == 'utxo-digest':
        try:
            res = asyncio.run(utxo_digest(a.db, a.snapshot, a.full))
        except (ValueError, OSError) as e:
            raise SystemExit(f'utxo-digest: {e}')
        print(json.dumps(res))
        return 0 if res.get('match', True) else 1
    elif a.command == 'utxo-root':
        try:
            print(json.dumps(asyncio.run(utxo_root(a.db, a.snapshot))))
        except (ValueError, OSError) as e:
            raise SystemExit(f'utxo-root: {e}')
        return 0
    elif a.command == 'utxo-proof':
        if a.check:
            if a.address or (a.root is None) != (a.count is None):
                ap.error('utxo-proof --check FILE takes no outpoints, and --root HEX and --count N go together')
            try:
                with open(a.check) as f:
                    lines, summary = check_proofs(json.load(f), a.root, a.count)
            except (ValueError, OSError, KeyError, TypeError) as e:
                raise SystemExit(f'utxo-proof: {e}')
            for line in lines:  # one JSON line per outpoint
                print(json.dumps(line))
            print(json.dumps(summary))
            return 0 if summary['ok'] else 1
        from .ledger.utxo_proof import split_outpoint
        try:
            outpoints = [split_outpoint(x) for x in a.address]
        except ValueError:
            outpoints = []
        if not outpoints:
            ap.error('utxo-proof needs TXHASH:INDEX outpoints (or --check FILE)')
        try:
            doc = asyncio.run(utxo_proofs(outpoints, a.db, a.snapshot))
        except (ValueError, OSError) as e:
            raise SystemExit(f'utxo-proof: {e}')
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(doc, f)
            print(json.dumps({'root': doc['root'], 'count': doc['count'], 'proofs': len(doc['proofs']), 'out': a.out}))
        else:
            print(json.dumps(doc))
        return 0
    elif a.command == 'utxo-diff':
        if bool(a.snapshot) == a.sql or (a.against and not a.snapshot):
            ap.error('utxo-diff needs --snapshot FILE (with --against FILE for two files) or --sql')
        if a.limit is not None and a.limit < 0:
            ap.error('--limit is a count >= 0')
        try:
            lines, summary = asyncio.run(utxo_diff(a.db, a.snapshot, a.sql, a.against, a.limit))
        except (ValueError, OSError) as e:
            raise SystemExit(f'utxo-diff: {e}')
        out = open(a.out, 'w') if a.out else sys.stdout
        try:
            for line in lines:  # one JSON line per differing entry
                print(json.dumps(line), file=out)
        finally:
            if a.out:
                out.close()
        print(json.dumps(summary))
        return 0 if summary['equal'] else 1
    elif a.command == 'rebuild-utxo':
        asyncio.run(rebuild_utxo(a.db))
    elif a.command in ('snapshot', 'verify-utxo'):
        from .ledger import snapshot

        async def s():
            db = await open_ledger(a.db)
            res = snapshot.save(db, a.out) if a.command == 'snapshot' else snapshot.verify(db)
            print(json.dumps(res))
            return 0 if res.get('ok', True) else 1
        return asyncio.run(s())
    elif a.command == 'materialise':
        async def m():
            db = await open_ledger(a.db)
            db.flush()
            print(json.dumps({'height': db._tip_id(), 'unspent_outputs_hash': await db.get_unspent_outputs_hash()}))
            db.close()
        asyncio.run(m())
    else:
        async def h():
            db = await open_ledger(a.db)
            print(await db.get_unspent_outputs_hash())
        asyncio.run(h())


if __name__ == '__main__':
    sys.exit(main())
