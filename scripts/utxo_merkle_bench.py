"""UTXO proofs (``UtxoIndex.merkle_snapshot``: the RFC 6962 tree over every live entry, and ``prove``) on one MI355X
at the aged-ledger scale: the HBM table of ``--n`` (5 M) outpoints of scripts/owner_totals_bench.py, generated from
``--seed``.

Timed, each as a host clock around a call that ends in its D2H copy, ``--warmup`` (3) warm-ups then ``--reps``
(>= 10) rounds that run the calls in turn, so drift hits all of them alike; median, min and max in ms:

  a  ``merkle_snapshot()`` + ``close()``    collect, cut to the tags, sort, leaf kernel, one launch per level; 32 B back
  b  ``prove`` of 1 and of 1000 outpoints   on a snapshot that is kept (half of the 1000 are absent)
  c  dump + host twin                       ``records_payload`` and ``utxo_merkle_build_records_host`` on 16 threads
                                            (``--host-reps``, default 3: it takes seconds)
  d  ``set_hash(0)`` and ``state_digest()`` K12 and the LtHash digest in the same session, for scale

(a) and (c) are checked to give the same root before anything is timed, and a proof of each kind is verified with
ledger/utxo_proof.py. The split of (a) into collect, sort, leaf kernel and level kernels comes from the kernels' own
times: run ``--only-build`` under ``rocprofv3 --kernel-trace --stats`` and hand its kernel_stats CSV to
``--stats-csv FILE --merge RESULT``. ``compressions``: the leaf kernel issues 2 per entry (1 + one per entry with a
33/64-byte address are used), the level kernels 2 per inner node (n - 1 of them). ``--host-sort N`` needs no GPU: it
times the host twin alone on N entries in random and in leaf order (what its serial sort costs). The JSON goes to
``--out``."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from owner_totals_bench import generate  # noqa: E402
from upow_amd.ledger import utxo_proof  # noqa: E402
from upow_amd.ledger.utxo import DIGEST_HOST_THREADS, MerkleSnapshot, UtxoIndex  # noqa: E402

STAGES = {'collect': ('utxo_collect_kernel', 'merkle_count_kernel', 'merkle_filter_kernel'),
          'sort': ('sort_column_kernel', 'iota_kernel', 'RadixSort', 'radix_sort', 'onesweep', 'histogram', 'scan'),
          'leaf': ('merkle_leaf_kernel',), 'levels': ('merkle_level_kernel',)}


def kernel_split(path, res):
    """Per build: each stage's kernel time from rocprofv3's kernel_stats CSV (total over the calls / builds run), and
    the hashing kernels' compressions per second."""
    total = {k: 0.0 for k in STAGES}
    calls = {k: 0 for k in STAGES}
    other = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row.get('Name', '')
            stage = next((s for s, keys in STAGES.items() if any(k.lower() in name.lower() for k in keys)), None)
            if stage is None:
                other[name[:80]] = round(float(row['TotalDurationNs']) * 1e-6, 3)
                continue
            total[stage] += float(row['TotalDurationNs'])
            calls[stage] += int(row['Calls'])
    builds = calls['leaf']
    if not builds:
        raise SystemExit(f'merkle_leaf_kernel is not in {path}')
    out = {'builds_profiled': builds, 'level_launches_per_build': calls['levels'] // builds,
           'ms_per_build': {k: round(v * 1e-6 / builds, 4) for k, v in total.items()}, 'other_kernels_total_ms': other}
    leaf_s, level_s = total['leaf'] * 1e-9 / builds, total['levels'] * 1e-9 / builds
    out['leaf_compressions_issued_per_s'] = round(res['leaf_compressions_issued'] / leaf_s, 1)
    out['leaf_compressions_used_per_s'] = round(res['leaf_compressions_used'] / leaf_s, 1)
    out['level_compressions_per_s'] = round(res['level_compressions'] / level_s, 1)
    return out


def host_sort_probe(a):
    """What the host twin's serial sort costs: ``utxo_merkle_build_records_host`` on ``--host-sort`` entries as
    generated (random order) and on the same entries handed over in leaf order, where the stable merge sort has
    nothing to move; the hashing is the same in both. ``--host-reps`` runs each after one warm-up, in turn."""
    from upow_amd.ops.native import lib
    L = lib()
    n = a.host_sort
    recs, pay = generate(n, a.seed, True)
    order = np.lexsort([recs[:, 36], recs[:, 32]] + [recs[:, k] for k in range(31, -1, -1)])
    inputs = {'random_order': (recs, pay),
              'leaf_order': (np.ascontiguousarray(recs[order]), np.ascontiguousarray(pay[order]))}
    roots, times = {}, {k: [] for k in inputs}
    for rep in range(1 + a.host_reps):
        for name, (r, p) in inputs.items():
            t = time.perf_counter()
            with MerkleSnapshot(L, L.utxo_merkle_build_records_host(r, p.view(np.uint8), a.host_threads)) as s:
                dt = time.perf_counter() - t
                roots[name] = s.root.hex()
            if rep:
                times[name].append(dt * 1e3)
    assert roots['random_order'] == roots['leaf_order']
    res = {'entries': n, 'seed': a.seed, 'host_threads': a.host_threads, 'cpus': os.cpu_count(), 'root': roots['leaf_order'],
           'ms': {k: {'median': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1),
                      'n': len(v)} for k, v in times.items()}}
    res['sort_share'] = round(1 - res['ms']['leaf_order']['median'] / res['ms']['random_order']['median'], 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=5_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--only-build', action='store_true', help='time (a) alone: the run to put under rocprofv3')
    ap.add_argument('--stats-csv', default=None)
    ap.add_argument('--merge', default=None, help='with --stats-csv: add the kernel split to this earlier result '
                    'file and stop (nothing runs)')
    ap.add_argument('--host-sort', type=int, default=0, metavar='N', help='host only, no GPU: the host twin on N '
                    'entries in random order and on the same entries already in leaf order, and stop')
    ap.add_argument('--host-threads', type=int, default=DIGEST_HOST_THREADS)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 10 and not a.only_build:
        ap.error('at least 10 repetitions')
    if a.merge:
        if not a.stats_csv:
            ap.error('--merge needs --stats-csv')
        with open(a.merge) as f:
            res = json.load(f)
        res['kernels'] = kernel_split(a.stats_csv, res)
        with open(a.merge, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return

    if a.host_sort:
        host_sort_probe(a)
        return
    recs, pay = generate(a.n, a.seed, True)
    idx = UtxoIndex(backend='gpu')
    for at in range(0, a.n, 1_000_000):
        idx.insert_records(recs[at:at + 1_000_000], pay[at:at + 1_000_000])
    assert len(idx) == a.n, 'duplicate outpoints in the generated set'
    L = idx.be.L
    with_addr = int(np.isin(pay['len'], (33, 64)).sum())

    def build():
        with idx.merkle_snapshot() as s:
            return s.root, s.count, s.levels, s.nbytes

    def host_twin():
        r, p = idx.records_payload(sort=False)
        with MerkleSnapshot(L, L.utxo_merkle_build_records_host(r, p.view(np.uint8), DIGEST_HOST_THREADS)) as s:
            return s.root, s.count
    root, count, levels, nbytes = build()
    res = {'outpoints': a.n, 'capacity': L.utxo_capacity(idx.be.h), 'seed': a.seed, 'warmup': a.warmup, 'reps': a.reps,
           'root': root.hex(), 'levels': levels, 'level_launches': levels - 1, 'snapshot_bytes': nbytes,
           'snapshot_bytes_per_entry': round(nbytes / a.n, 2), 'host_threads': DIGEST_HOST_THREADS,
           'leaf_compressions_issued': 2 * a.n, 'leaf_compressions_used': a.n + with_addr,
           'level_compressions': 2 * (a.n - 1)}
    calls = {'a_build': build}
    host_ms = []
    if not a.only_build:
        assert host_twin() == (root, count) and count == a.n
        keep = idx.merkle_snapshot()
        rng = np.random.default_rng(a.seed + 1)
        live = [(bytes(recs[k, :32]).hex(), int(recs[k, 32])) for k in rng.choice(a.n, 500, replace=False)]
        absent = [(rng.bytes(32).hex(), 0) for _ in range(500)]
        thousand = [x for pair in zip(live, absent) for x in pair]
        for (h, i), p in zip(thousand[:4], keep.prove(thousand[:4])):
            assert (utxo_proof.verify_outpoint(root, count, h, i, p) is not None) == p.present
        res['proof_hashes_of_one'] = len(keep.prove(live[:1])[0].leaves[0].path)
        calls['b_prove_1'] = lambda: keep.prove(live[:1])
        calls['b_prove_1000'] = lambda: keep.prove(thousand)
        calls['d_set_hash_k12'] = lambda: idx.set_hash(0)
        calls['d_state_digest'] = lambda: idx.state_digest()
        for _ in range(a.host_reps):
            t = time.perf_counter()
            host_twin()
            host_ms.append((time.perf_counter() - t) * 1e3)
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, call in calls.items():  # alternating: one round runs every call once
            t = time.perf_counter()
            call()
            dt = time.perf_counter() - t
            if rep >= a.warmup:
                times[name].append(dt * 1e3)
    if host_ms:
        times['c_dump_and_host_twin'] = host_ms
    res['ms'] = {k: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3),
                     'n': len(v)} for k, v in times.items()}
    if a.stats_csv:
        res['kernels'] = kernel_split(a.stats_csv, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
