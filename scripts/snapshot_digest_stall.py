"""What a background snapshot's state digest costs the block path on the host: the host worker pool runs one
parallel region at a time (csrc/thread_pool.h), the block path's decode and the host signers use it, and a save
digests ``--n`` (5 M) entries (ledger/snapshot.py ``_state_digest``: slices of ``DIGEST_SLICE`` entries on
``DIGEST_THREADS`` threads of its own, each outside the pool).

The probe is a pool region of the block path: ``sha256_hex_prefixes`` (the fast path's hashing of a block's
transaction hex, a ``HostPool`` region) over ``--msgs`` (8,300) hex strings of 600 characters on 16 threads, a
2 MB block's worth. It is timed ``--probes`` times alone, then again and again, 0 - 4 ms apart, while a thread
digests the set (i) as a save does, (ii) in slices of the same size on the pool, 16 threads each, and (iii) in
one call on the pool: the two ways a save does not go. Median, 99th percentile and worst probe latency in ms,
and each digest's wall time, as one JSON line; no GPU is used. ``--out`` takes the JSON."""
import argparse
import json
import os
import random
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from owner_totals_bench import generate  # noqa: E402
from upow_amd.ledger import snapshot  # noqa: E402
from upow_amd.ledger.utxo import StateDigest, records_digest  # noqa: E402
from upow_amd.ops.native import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=5_000_000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--msgs', type=int, default=8300)
    ap.add_argument('--probes', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    L = lib()
    recs, pay = generate(a.n, a.seed, True)
    raw = np.random.default_rng(a.seed).integers(0, 256, (a.msgs, 300), dtype=np.uint8)
    hexes = [bytes(r).hex() for r in raw]
    idx, nchars = np.arange(a.msgs, dtype=np.int64), np.full(a.msgs, 600, dtype=np.int64)

    def probe():
        t = time.perf_counter()
        L.sha256_hex_prefixes(hexes, idx, nchars, 16)
        return (time.perf_counter() - t) * 1e3

    def stats(v):
        return {'probes': len(v), 'median': round(statistics.median(v), 3), 'p99': round(float(np.percentile(v, 99)), 3),
                'max': round(max(v), 3)}

    rng = random.Random(a.seed)

    def during(work):
        """Probe latencies while ``work`` runs on a thread, and its wall time and result."""
        box = {}

        def run():
            t = time.perf_counter()
            box['digest'] = work()
            box['s'] = time.perf_counter() - t
        th = threading.Thread(target=run)
        th.start()
        v = []
        while th.is_alive():
            v.append(probe())
            time.sleep(rng.uniform(0.0, 0.004))  # not in step with the slices
        th.join()
        return v, box

    for _ in range(20):
        probe()
    res = {'entries': a.n, 'slice': snapshot.DIGEST_SLICE, 'save_threads': snapshot.DIGEST_THREADS, 'probe': f'sha256_hex_prefixes, {a.msgs} x 600 characters, 16 threads',
           'cpus': os.cpu_count(), 'alone_ms': stats([probe() for _ in range(a.probes)])}
    def pool_slices():
        d = StateDigest()
        for at in range(0, a.n, snapshot.DIGEST_SLICE):
            d = d + records_digest(recs[at:at + snapshot.DIGEST_SLICE], pay[at:at + snapshot.DIGEST_SLICE], device='cpu')
        return d
    v, own = during(lambda: snapshot._state_digest(recs, pay))
    res['during_save_digest_ms'], res['save_digest_s'] = stats(v), round(own['s'], 3)
    v, sliced = during(pool_slices)
    res['during_pool_slices_ms'], res['pool_slices_s'] = stats(v), round(sliced['s'], 3)
    v, whole = during(lambda: records_digest(recs, pay, device='cpu'))
    res['during_pool_one_call_ms'], res['pool_one_call_s'] = stats(v), round(whole['s'], 3)
    assert own['digest'] == sliced['digest'] == whole['digest']
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
