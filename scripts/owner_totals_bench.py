"""Holders report (``UtxoIndex.owner_totals``) on one MI355X at the aged-ledger scale: an HBM table of ``--n``
(5 M) outpoints owned by about 2.5 M public keys with a skewed distribution, one of which (the hot owner) holds
10 % of the entries; a second table holds the same set with the hot owner's entries dealt out to the others.
Everything is generated from ``--seed``.

Timed, each as a host clock around a call that ends in its D2H copy, ``--warmup`` (3) warm-ups then ``--reps``
(>= 10) rounds that run the calls in turn, so drift hits all of them alike; median, min and max in ms:

  a  ``owner_totals()``                          every owner, from the HBM aggregation
  b  ``owner_totals(top=100)``                   aggregation + radix sort + threshold compaction
  c  ``records_payload(sort=False)`` + grouping  what there was before: dump 120 B per outpoint, group in numpy
  d  ``owner_totals()`` and ``owner_totals(top=100)`` on the table without the hot owner. That table has more
     owners, so more records come back in full mode; the top-100 pair (b - d_top100) returns 100 records either
     way and isolates what 10 % of the lanes meeting in one group slot cost

(a) and (c) are checked to give the same bytes before anything is timed. ``must_read_bytes`` = 48 B x capacity
+ 80 B x live entries: the key-slot lines and the payload lines the pass is defined over. ``--stats-csv FILE``
(the kernel_stats CSV of a separate ``rocprofv3 --kernel-trace --stats`` run of this script with ``--only-a``,
or ``--only-a --no-hot-owner`` for the other table, kept apart with ``--stats-key``)
adds the aggregation kernel's mean time, must_read_bytes over it, and that rate as a share of the HBM peaks
(``--merge FILE``: into an earlier result file, without running anything).
The JSON goes to ``--out``."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from upow_amd.ledger.utxo import PAYLOAD_DTYPE, UtxoIndex, owner_totals_of  # noqa: E402

HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12  # bytes/s: spec, and the measured float4 copy
GROUP_KERNEL = 'utxo_owner_group_kernel'


def generate(n, seed, hot):
    """(records, payloads) of n outpoints. Owner of an entry: pool[floor(P u^2)] for uniform u (a few owners
    hold many outputs, most hold one; P = 1.15 n gives about n / 2 distinct owners), or with ``hot`` the hot
    owner for every tenth entry. A fifth of the entries are stored in the 64-byte form; 85 % are spendable,
    10 % stake, 5 % in the six governance tables."""
    rng = np.random.default_rng(seed)
    pool = int(1.15 * n)
    x = rng.integers(0, 256, (pool + 1, 32), dtype=np.uint8)
    y = rng.integers(0, 256, (pool + 1, 32), dtype=np.uint8)
    who = np.minimum((pool * rng.random(n) ** 2).astype(np.int64), pool - 1)
    tenth = rng.random(n) < 0.1
    if hot:
        who[tenth] = pool  # the extra key
    full = rng.random(n) < 0.2
    kind = rng.random(n)
    recs = np.zeros((n, 40), np.uint8)
    recs[:, :32] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    recs[:, 32] = rng.integers(0, 256, n, dtype=np.uint8)
    recs[:, 36] = np.where(kind < 0.95, 0, rng.integers(1, 7, n)).astype(np.uint8)
    pay = np.zeros(n, PAYLOAD_DTYPE)
    pay['amount'] = rng.integers(1, 1 << 40, n)
    pay['len'] = np.where(full, 64, 33)
    pay['flags'] = ((kind >= 0.85) & (kind < 0.95)).astype(np.uint32)
    addr = np.zeros((n, 64), np.uint8)
    short = ~full
    addr[short, 0] = 42 + (y[who[short], 0] & 1)
    addr[short, 1:33] = x[who[short]]
    addr[full, :32] = x[who[full]]
    addr[full, 32:] = y[who[full]]
    pay['addr'] = addr
    return recs, pay


def table(n, seed, hot):
    idx = UtxoIndex(backend='gpu')
    recs, pay = generate(n, seed, hot)
    for at in range(0, n, 1_000_000):
        idx.insert_records(recs[at:at + 1_000_000], pay[at:at + 1_000_000])
    assert len(idx) == n, 'duplicate outpoints in the generated set'
    return idx


def kernel_figures(path, must_read):
    """The aggregation kernel's mean time from rocprofv3's kernel_stats CSV, and must_read bytes over it."""
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            if GROUP_KERNEL in row.get('Name', ''):
                sec = float(row['AverageNs']) * 1e-9
                return {'mean_ms': round(sec * 1e3, 4), 'calls': int(row['Calls']),
                        'must_read_GB_per_s': round(must_read / sec / 1e9, 1),
                        'share_of_hbm_spec_peak': round(must_read / sec / HBM_PEAK_SPEC, 4),
                        'share_of_hbm_measured_peak': round(must_read / sec / HBM_PEAK_MEASURED, 4)}
    raise SystemExit(f'{GROUP_KERNEL} is not in {path}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=5_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only-a', action='store_true', help='time (a) alone: the run to put under rocprofv3')
    ap.add_argument('--no-hot-owner', action='store_true', help='with --only-a: the table without the hot owner')
    ap.add_argument('--stats-csv', default=None)
    ap.add_argument('--stats-key', default='group_kernel', help='where the kernel figures go in the result')
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
        res[a.stats_key] = kernel_figures(a.stats_csv, res['must_read_bytes'])
        with open(a.merge, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return

    hot = table(a.n, a.seed, not (a.only_a and a.no_hot_owner))
    cap = hot.be.L.utxo_capacity(hot.be.h)
    calls = {'a_owner_totals': lambda: hot.owner_totals()}
    if not a.only_a:
        flat = table(a.n, a.seed, False)
        calls['b_owner_totals_top100'] = lambda: hot.owner_totals(top=100)
        calls['c_dump_and_numpy_grouping'] = lambda: owner_totals_of(*hot.records_payload(sort=False))
        calls['d_owner_totals_no_hot_owner'] = lambda: flat.owner_totals()
        calls['d_top100_no_hot_owner'] = lambda: flat.owner_totals(top=100)
        got, info = calls['a_owner_totals']()
        want, winfo = calls['c_dump_and_numpy_grouping']()
        assert got.tobytes() == want.tobytes() and info['totals'].tolist() == winfo['totals'].tolist()
        assert (info['owners'], info['outputs'], info['skipped']) == (winfo['owners'], a.n, 0)
        top = calls['b_owner_totals_top100']()[0]
        metric = want['sums'][:, 0] + want['sums'][:, 7]
        assert top.tobytes() == want[np.argsort(~metric, kind='stable')[:100]].tobytes()
    owners, info = calls['a_owner_totals']()
    times = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, call in calls.items():  # alternating: one round runs every call once
            t = time.perf_counter()
            call()
            dt = time.perf_counter() - t
            if rep >= a.warmup:
                times[name].append(dt * 1e3)
    must_read = 48 * cap + 80 * a.n
    res = {'outpoints': a.n, 'capacity': cap, 'owners': info['owners'], 'hot_owner_outputs': int(owners['outputs'].max()),
           'seed': a.seed, 'warmup': a.warmup, 'reps': a.reps, 'must_read_bytes': must_read,
           'record_bytes_returned': int(owners.nbytes), 'dump_bytes_returned': 120 * a.n,
           'ms': {k: {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
                  for k, v in times.items()}}
    if not a.only_a:
        m = {k: v['median'] for k, v in res['ms'].items()}
        res['a_over_c'] = round(m['a_owner_totals'] / m['c_dump_and_numpy_grouping'], 4)
        res['b_over_c'] = round(m['b_owner_totals_top100'] / m['c_dump_and_numpy_grouping'], 4)
        res['owners_no_hot_owner'] = flat.owner_totals(top=0)[1]['owners']
        res['hot_owner_cost_ms'] = round(m['b_owner_totals_top100'] - m['d_top100_no_hot_owner'], 3)
    if a.stats_csv:
        res[a.stats_key] = kernel_figures(a.stats_csv, must_read)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
