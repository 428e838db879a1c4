"""State digest (``UtxoIndex.state_digest``: LtHash16/1024 over every live entry with its payload) on one MI355X
at the aged-ledger scale: the HBM table of ``--n`` (5 M) outpoints of scripts/owner_totals_bench.py, generated from
``--seed``.

Timed, each as a host clock around a call that ends in its D2H copy, ``--warmup`` (3) warm-ups then ``--reps``
(>= 10) rounds that run the calls in turn, so drift hits all of them alike; median, min and max in ms:

  a  ``state_digest()``                              one pass over the HBM table; 8 stripes (32,896 B) come back
                                                     and are summed into the 2 KB state + the count
  b  ``set_hash(0)``                                 K12, the keys-only hash it complements
  c  ``records_payload(sort=False)`` + host digest   the dump (120 B per outpoint) and ``utxo_records_digest_host``
                                                     on 16 threads
  d  ``records_digest`` of a block-sized delta       about 17 k created + 8 k spent entries, on the GPU and on the host

(a) and (c) are checked to give the same bytes before anything is timed. ``compressions`` = 65 per entry with a
33/64-byte address, 64 per entry without: (a)'s rate over the PoW kernel's 35.5 G compressions/s (README) is the
yardstick. ``--only-a`` times (a) alone: the run to put under ``rocprofv3 --kernel-trace --stats``, whose
kernel_stats CSV ``--stats-csv FILE`` (``--merge FILE``: into an earlier result, without running anything) turns
into the kernel's own mean time and rate. The JSON goes to ``--out``."""
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
from upow_amd.ledger.utxo import DIGEST_HOST_THREADS, StateDigest, UtxoIndex, records_digest  # noqa: E402

POW_RATE = 35.5e9  # compressions/s of the PoW kernel, about one per nonce (README)
KERNEL = 'utxo_digest_kernel'
D2H_BYTES = 8 * (1024 + 4) * 4  # what a pass copies back: 8 stripes of 1024 u32 lane sums + the count (utxo_digest.hip)


def kernel_figures(path, compressions):
    """The digest kernel's mean time from rocprofv3's kernel_stats CSV, and compressions over it."""
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            if KERNEL in row.get('Name', ''):
                sec = float(row['AverageNs']) * 1e-9
                return {'mean_ms': round(sec * 1e3, 4), 'calls': int(row['Calls']),
                        'compressions_per_s': round(compressions / sec, 1),
                        'share_of_pow_rate': round(compressions / sec / POW_RATE, 4)}
    raise SystemExit(f'{KERNEL} is not in {path}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=5_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--created', type=int, default=17_000)
    ap.add_argument('--spent', type=int, default=8_000)
    ap.add_argument('--only-a', action='store_true', help='time (a) alone: the run to put under rocprofv3')
    ap.add_argument('--stats-csv', default=None)
    ap.add_argument('--merge', default=None, help='with --stats-csv: add the kernel figures to this earlier '
                    'result file and stop (nothing runs)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.reps < 10 and not a.only_a:
        ap.error('at least 10 repetitions')
    if a.merge:
        if not a.stats_csv:
            ap.error('--merge needs --stats-csv')
        with open(a.merge) as f:
            res = json.load(f)
        res['digest_kernel'] = kernel_figures(a.stats_csv, res['compressions'])
        with open(a.merge, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return

    recs, pay = generate(a.n + a.created, a.seed, True)
    idx = UtxoIndex(backend='gpu')
    for at in range(0, a.n, 1_000_000):
        idx.insert_records(recs[at:min(a.n, at + 1_000_000)], pay[at:min(a.n, at + 1_000_000)])
    assert len(idx) == a.n, 'duplicate outpoints in the generated set'
    L = idx.be.L
    cap = L.utxo_capacity(idx.be.h)
    compressions = int(64 * a.n + np.isin(pay['len'][:a.n], (33, 64)).sum())

    def host_digest():
        r, p = idx.records_payload(sort=False)
        return StateDigest(*L.utxo_records_digest_host(r, p.view(np.uint8), DIGEST_HOST_THREADS))
    calls = {'a_state_digest': lambda: idx.state_digest()}
    if not a.only_a:
        created = (np.ascontiguousarray(recs[a.n:]), np.ascontiguousarray(pay[a.n:]))
        pick = np.random.default_rng(a.seed + 1).choice(a.n, a.spent, replace=False)
        spent = (np.ascontiguousarray(recs[pick]), np.ascontiguousarray(pay[pick]))
        calls['b_set_hash_k12'] = lambda: idx.set_hash(0)
        calls['c_dump_and_host_digest'] = host_digest
        calls['d_delta_gpu'] = lambda: records_digest(*created, device='gpu') - records_digest(*spent, device='gpu')
        calls['d_delta_host'] = lambda: records_digest(*created, device='cpu') - records_digest(*spent, device='cpu')
        got, want = calls['a_state_digest'](), calls['c_dump_and_host_digest']()
        assert got.tobytes() == want.tobytes() and got.count == want.count == a.n
        assert calls['d_delta_gpu']() == calls['d_delta_host']()
    digest = calls['a_state_digest']()
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, call in calls.items():  # alternating: one round runs every call once
            t = time.perf_counter()
            call()
            dt = time.perf_counter() - t
            if rep >= a.warmup:
                times[name].append(dt * 1e3)
    res = {'outpoints': a.n, 'capacity': cap, 'seed': a.seed, 'warmup': a.warmup, 'reps': a.reps,
           'digest': digest.hex(), 'compressions': compressions, 'delta_created': a.created, 'delta_spent': a.spent,
           'host_threads': DIGEST_HOST_THREADS, 'digest_bytes': 2048 + 8, 'd2h_bytes': D2H_BYTES,
           'dump_bytes_returned': 120 * a.n,
           'ms': {k: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
                  for k, v in times.items()}}
    sec = res['ms']['a_state_digest']['median'] * 1e-3
    res['a_compressions_per_s'] = round(compressions / sec, 1)
    res['a_share_of_pow_rate'] = round(compressions / sec / POW_RATE, 4)
    if not a.only_a:
        m = {k: v['median'] for k, v in res['ms'].items()}
        res['a_over_b'] = round(m['a_state_digest'] / m['b_set_hash_k12'], 4)
        res['a_over_c'] = round(m['a_state_digest'] / m['c_dump_and_host_digest'], 4)
    if a.stats_csv:
        res['digest_kernel'] = kernel_figures(a.stats_csv, compressions)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
