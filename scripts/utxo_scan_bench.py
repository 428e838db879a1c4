"""K14 utxo_address_scan throughput on one MI355X: fill the HBM UTXO table to ~45 % load with random
outpoints owned by 1 000 addresses, then time address queries (one full-table scan each).

The figure of merit is slots/s. ``logical_key_GB_per_s`` = capacity x 48 B key slots per scan time: the
bytes a scan is DEFINED over, not the bytes it moves — the kernel reads only each slot's meta words (the
80 B payload line only for live slots whose tag matches), so the HBM traffic is lower; take that from
rocprofv3 ``--pmc FETCH_SIZE`` on this script, not from this figure.

``--batch [Q,Q,...]`` (default 1,2,16,256,1024): in the same process, on the same table, time the single
scan and the batched pass (``utxo_address_scan_batch``, one table pass for Q queries) at each Q, queries
drawn from the 1 000 owners; every figure is the median wall time of ``--reps`` calls of the binding after a
warm-up, so it includes the call's memsets, launches and blocking copies. Two series: ``hits`` asks table 0
(every query returns its owner's ~n/1000 outputs: the result transfer and, past 4096 matches, the second
pass are part of the time), ``pass`` asks with the tag mask of an empty table (the pass itself: the search
per slot and the payload line of every slot whose fingerprint is asked for, no result to move).
``--out FILE`` writes the table as text."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from upow_amd.ledger.utxo import PAYLOAD_DTYPE, STAKE_ANY, UtxoIndex  # noqa: E402

N_OWNERS = 1000


def fill(n):
    rng = np.random.default_rng(1)
    idx = UtxoIndex(backend='gpu')
    owners = np.zeros((N_OWNERS, 64), np.uint8)
    owners[:, 0] = 42
    owners[:, 1:33] = rng.integers(0, 256, (N_OWNERS, 32), dtype=np.uint8)
    done = 0
    while done < n:
        m = min(1_000_000, n - done)
        recs = np.zeros((m, 40), np.uint8)
        recs[:, :32] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        pay = np.zeros(m, PAYLOAD_DTYPE)
        pay['amount'] = rng.integers(1, 1 << 40, m)
        pay['len'] = 33
        pay['addr'] = owners[rng.integers(0, N_OWNERS, m)]
        idx.insert_records(recs, pay)
        done += m
    return idx, owners


def main(n=int(os.environ.get('N', 7_500_000)), queries=50):
    idx, owners = fill(n)
    L, h = idx.be.L, idx.be.h
    cap = L.utxo_capacity(h)
    L.utxo_address_scan(h, bytes(owners[0, :33]), 1, STAKE_ANY)  # warm
    t = time.perf_counter()
    hits = 0
    for q in range(queries):
        raw, _, _ = L.utxo_address_scan(h, bytes(owners[q % 1000, :33]), 1, STAKE_ANY)
        hits += len(raw) // 40
    dt = (time.perf_counter() - t) / queries
    print(json.dumps({'live': len(idx), 'capacity': cap, 'ms_per_query': round(dt * 1e3, 3),
                      'slots_per_s': round(cap / dt / 1e9, 2), 'unit': 'G slots/s',
                      'logical_key_GB_per_s': round(cap * 48 / dt / 1e9, 1), 'avg_hits': hits / queries}))


def _median_ms(call, reps):
    call()  # warm-up
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    return statistics.median(times) * 1e3


def batch_queries(owners, q, rng):
    """q distinct queries over the owners, in random order; past 1 000 the first owners are asked again under
    a second tag mask (a distinct query record, so the sorted table holds q entries)."""
    pick = rng.permutation(N_OWNERS)
    who = np.concatenate([pick] * (q // N_OWNERS + 1))[:q]
    second = np.arange(q) >= N_OWNERS
    return np.ascontiguousarray(owners[who]), np.full(q, 33, np.uint32), second


def main_batch(qs, reps, out, n=int(os.environ.get('N', 7_500_000))):
    idx, owners = fill(n)
    L, h = idx.be.L, idx.be.h
    cap = L.utxo_capacity(h)
    rng = np.random.default_rng(2)
    # tag masks: 'hits' = table 0 (second ask of an owner: tables 0 and 3), 'pass' = table 1, which is empty
    series = {'hits': (0b1, 0b1001), 'pass': (0b10, 0b10010)}
    res = {'live': len(idx), 'capacity': cap, 'reps': reps, 'single': {}, 'batch': []}
    for name, (mask, _) in series.items():
        found = []
        res['single'][name] = {
            'ms': _median_ms(lambda: found.append(len(L.utxo_address_scan(h, bytes(owners[len(found) % N_OWNERS, :33]),
                                                                          mask, STAKE_ANY)[0]) // 40), reps),
            'matches': found[-1]}
    for q in qs:
        addrs, lens, second = batch_queries(owners, q, rng)
        sels = np.zeros(q, np.uint32)
        row = {'q': q}
        for name, (mask, mask2) in series.items():
            masks = np.where(second, mask2, mask).astype(np.uint32)
            found = []
            ms = _median_ms(lambda: found.append(len(L.utxo_address_scan_batch(h, addrs, lens, masks, sels)[0])), reps)
            single = res['single'][name]['ms']
            row[name] = {'ms_per_pass': ms, 'us_per_query': ms * 1e3 / q, 'matches': found[-1],
                         'vs_one_single': ms / single, 'vs_q_singles': ms / (q * single)}
        res['batch'].append(row)
    print(json.dumps(res))
    if out:
        lines = [f'K14 batched address scan (scripts/utxo_scan_bench.py --batch): {res["live"]} live outputs in '
                 f'{cap} slots, {N_OWNERS} owners;',
                 f'median wall time of {reps} binding calls after a warm-up, one process, one table.',
                 'hits: queries ask table 0 (results returned; > 4096 matches take a second pass). pass: queries ask',
                 'an empty table (the table pass alone: per-slot search + payload line of asked fingerprints).', '']
        for name in series:
            s = res['single'][name]
            lines += [f'[{name}] single scan: {s["ms"]:.3f} ms per query ({s["matches"]} matches)',
                      f'{"Q":>6} {"ms/pass":>10} {"us/query":>10} {"matches":>9} {"x 1 single":>11} {"x Q singles":>12}']
            for row in res['batch']:
                r = row[name]
                lines.append(f'{row["q"]:>6} {r["ms_per_pass"]:>10.3f} {r["us_per_query"]:>10.2f} {r["matches"]:>9} '
                             f'{r["vs_one_single"]:>11.2f} {r["vs_q_singles"]:>12.4f}')
            lines.append('')
        with open(out, 'w') as f:
            f.write('\n'.join(lines))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', nargs='?', const='1,2,16,256,1024', default=None,
                    help='compare the batched pass at these query counts with the single scan')
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.batch is None:
        main()
    else:
        main_batch([int(q) for q in a.batch.split(',')], max(a.reps, 20), a.out)
