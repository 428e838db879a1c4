"""UTXO diff (``UtxoIndex.diff_records``: which entries differ between the index and a record set) on one MI355X at
the aged-ledger scale: the HBM table of ``--n`` (5 M) outpoints of scripts/owner_totals_bench.py, generated from
``--seed``, against O = the same set with 0, 1,000 and 100,000 planted differences (``--planted``): a third of them
entries dropped from O (extra), a third fresh entries added to O (missing), the rest one amount bit flipped (changed).

Timed, each as a host clock around a call that ends in its D2H copy, ``--warmup`` (2) warm-ups then ``--reps`` (>= 5)
rounds that run the calls in turn; median, min and max in ms:

  a  ``diff_records(O)`` per planted count     the whole GPU path: O uploaded in 2^20-record chunks (126 MB each),
                                               the match kernel per chunk, the sweep, one status byte per record
                                               and the extras back, the lists built on the host. Next to it the
                                               native call alone (``utxo_diff``) and the hold of the table lock
                                               that it reports (the block path waits behind it)
  b  ``state_digest()``                        the floor for one pass over the slots
  c  ``records_payload(sort=False)``           the dump (120 B per outpoint over PCIe, the other way): what the host
                                               way needs first
  d  ``diff_of`` / ``diff_vectorised`` on      what an operator can do without the GPU pass (the dict-based reference
     that dump                                 and the numpy join of the native host table): once each, for the
                                               largest planted count, on ``--host-n`` entries (default: all)

Every diff's counts are checked against the plant before anything is timed. ``--only-a`` times (a) alone: the run to
put under ``rocprofv3 --kernel-trace --memory-copy-trace --stats``, whose stats CSVs ``--stats-csv FILE [FILE ...]``
(``--merge FILE``: into an earlier result, without running anything) turn into per-call means of the two kernels and
the copies. ``bytes`` are what each kernel touches at least, for the HBM rate. The JSON goes to ``--out``."""
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
from upow_amd.ledger.utxo import DIFF_LIMIT, UtxoIndex, diff_of, diff_vectorised  # noqa: E402

HBM_RATE = 6.29e12  # B/s: the measured float4 copy rate of the MI355X (8.0 TB/s specified)
SLOT, REC, PAY = 48, 40, 80


def plant(recs, pay, fresh, n_diff, seed):
    """O with n_diff planted differences and their counts (missing, extra, changed)."""
    rng = np.random.default_rng(seed)
    n = len(recs)
    n_extra, n_missing = n_diff // 3, n_diff // 3
    n_changed = n_diff - n_extra - n_missing
    pick = rng.choice(n, n_extra + n_changed, replace=False)
    keep = np.ones(n, bool)
    keep[pick[:n_extra]] = False
    o_pay = pay[:n].copy()
    o_pay['amount'][pick[n_extra:]] ^= np.uint64(1 << 20)
    o_recs = np.concatenate([recs[:n][keep], fresh[0][:n_missing]])
    o_pay = np.concatenate([o_pay[keep], fresh[1][:n_missing]])
    order = rng.permutation(len(o_recs))
    return np.ascontiguousarray(o_recs[order]), np.ascontiguousarray(o_pay[order]), (n_missing, n_extra, n_changed)


def stats_figures(paths, calls_per_kernel):
    """Calls, total and mean of the two kernels and of the copies (the runtime moves pageable memory with
    ``__amd_rocclr_copyBuffer`` blits, which are kernels to the profiler) from rocprofv3's stats CSVs."""
    out = {}
    for path in paths:
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                name = row.get('Name', '')
                for key in ('utxo_diff_match_kernel', 'utxo_diff_extra_kernel', '__amd_rocclr_copyBuffer',
                            'HOST_TO_DEVICE', 'DEVICE_TO_HOST'):
                    if key in name:
                        out[key] = {'calls': int(row['Calls']),
                                    'total_ms': round(float(row['TotalDurationNs']) * 1e-6, 4),
                                    'mean_ms': round(float(row['AverageNs']) * 1e-6, 4)}
    if not out:
        raise SystemExit('none of the diff kernels or copies is in ' + ', '.join(paths))
    out['diff_calls'] = calls_per_kernel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=5_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--planted', default='0,1000,100000')
    ap.add_argument('--host-n', type=int, default=None, help='entries of the host way (d); 0: skip it')
    ap.add_argument('--only-a', action='store_true', help='time (a) alone: the run to put under rocprofv3')
    ap.add_argument('--stats-csv', nargs='+', default=None)
    ap.add_argument('--merge', default=None, help='with --stats-csv: add the kernel and copy figures to this earlier '
                    'result file and stop (nothing runs)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    planted = [int(x) for x in a.planted.split(',')]
    if a.reps < 5 and not a.only_a:
        ap.error('at least 5 repetitions')
    if a.merge:
        if not a.stats_csv:
            ap.error('--merge needs --stats-csv')
        with open(a.merge) as f:
            res = json.load(f)
        res['rocprof'] = stats_figures(a.stats_csv, None)
        with open(a.merge, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return

    most = max(planted)
    recs, pay = generate(a.n + most, a.seed, True)
    fresh = (recs[a.n:], pay[a.n:])
    idx = UtxoIndex(backend='gpu')
    for at in range(0, a.n, 1_000_000):
        idx.insert_records(recs[at:min(a.n, at + 1_000_000)], pay[at:min(a.n, at + 1_000_000)])
    assert len(idx) == a.n, 'duplicate outpoints in the generated set'
    L = idx.be.L
    cap = L.utxo_capacity(idx.be.h)
    cases = {d: plant(recs[:a.n], pay[:a.n], fresh, d, a.seed + 7 + k) for k, d in enumerate(planted)}
    calls, info = {}, {}
    for d, (o_recs, o_pay, want) in cases.items():
        got = idx.diff_records(o_recs, o_pay, limit=max(DIFF_LIMIT, most))
        if (got.n_missing, got.n_extra, got.n_changed) != want or got.truncated or got.entries != a.n or \
                got.equal != (d == 0) or got.compared != len(o_recs):
            raise SystemExit(f'{d} planted differences {want}: {got!r}')
        info[d] = {'records': len(o_recs), 'missing': want[0], 'extra': want[1], 'changed': want[2],
                   'h2d_bytes': len(o_recs) * (REC + PAY),
                   'd2h_bytes': len(o_recs) + min(want[1], DIFF_LIMIT) * (REC + PAY) + 64 * 128 + 4,
                   # the match kernel reads each record and payload, the slot lines of its probe walk (at least one)
                   # and on a hit the entry's payload, and writes a status byte; the sweep reads every slot line and
                   # the bitmap, and for an extra its payload, and writes it out
                   'match_kernel_bytes_at_least': len(o_recs) * (REC + PAY + 1) + (len(o_recs) - want[0]) * (SLOT + PAY)
                   + want[0] * SLOT,
                   'extra_kernel_bytes_at_least': cap * SLOT + cap // 8 + want[1] * (SLOT + 2 * PAY + REC)}
        calls[f'a_diff_records_{d}'] = (lambda r=o_recs, p=o_pay: idx.diff_records(r, p, limit=DIFF_LIMIT))
        calls[f'a_native_call_{d}'] = (lambda r=o_recs, p=o_pay: L.utxo_diff(idx.be.h, r, p.view(np.uint8), 0x7f,
                                                                             DIFF_LIMIT, 0))
    if not a.only_a:
        calls['b_state_digest'] = lambda: idx.state_digest()
        calls['c_dump'] = lambda: idx.records_payload(sort=False)
    times = {k: [] for k in calls}
    holds = {d: [] for d in cases}
    for rep in range(a.warmup + a.reps):
        for name, call in calls.items():  # alternating: one round runs every call once
            t = time.perf_counter()
            out = call()
            dt = time.perf_counter() - t
            if rep >= a.warmup:
                times[name].append(dt * 1e3)
                if name.startswith('a_native_call_'):
                    holds[int(name.rsplit('_', 1)[1])].append(out[7] * 1e3)

    def spread(v):
        return {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    res = {'outpoints': a.n, 'capacity': cap, 'seed': a.seed, 'warmup': a.warmup, 'reps': a.reps, 'limit': DIFF_LIMIT,
           'chunk_records': 1 << 20, 'hbm_rate_bytes_per_s': HBM_RATE, 'cases': {str(d): v for d, v in info.items()},
           'ms': {k: spread(v) for k, v in times.items()},
           'lock_hold_ms': {str(d): spread(v) for d, v in holds.items()}}
    for d, v in info.items():
        v['match_kernel_ms_at_hbm_rate'] = round(v['match_kernel_bytes_at_least'] / HBM_RATE * 1e3, 4)
        v['extra_kernel_ms_at_hbm_rate'] = round(v['extra_kernel_bytes_at_least'] / HBM_RATE * 1e3, 4)
    host_n = a.n if a.host_n is None else min(a.host_n, a.n)
    if not a.only_a and host_n:
        o_recs, o_pay, _ = cases[most]
        t = time.perf_counter()
        dump = idx.records_payload(sort=False)
        t_dump = time.perf_counter() - t
        if host_n < a.n:  # a slice of both sides: the join's cost per entry, not the 5 M answer
            dump, o_recs, o_pay = (dump[0][:host_n], dump[1][:host_n]), o_recs[:host_n], o_pay[:host_n]
        t = time.perf_counter()
        ref = diff_of(o_recs, o_pay, *dump, limit=DIFF_LIMIT)
        t_join = time.perf_counter() - t
        t = time.perf_counter()
        vec = diff_vectorised(o_recs, o_pay, *dump, limit=DIFF_LIMIT)
        t_vec = time.perf_counter() - t
        assert (ref.n_missing, ref.n_extra, ref.n_changed) == (vec.n_missing, vec.n_extra, vec.n_changed)
        if host_n == a.n:
            want = cases[most][2]
            assert (ref.n_missing, ref.n_extra, ref.n_changed) == want
        res['d_host_way'] = {'planted': most, 'entries': host_n, 'dump_ms': round(t_dump * 1e3, 1),
                             'diff_of_ms': round(t_join * 1e3, 1), 'diff_vectorised_ms': round(t_vec * 1e3, 1),
                             'runs': 1}
    if a.stats_csv:
        res['rocprof'] = stats_figures(a.stats_csv, (a.warmup + a.reps) * 2 * len(cases) + len(cases))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
