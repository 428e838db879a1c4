"""Vanity search throughput (K16, csrc/p256_vanity.hip) against the existing way to derive candidate keys.

Search: ``p256_vanity_search`` on the GPU over a range set that matches nothing (one value at the bottom of the
address space), ``--launches`` full launches per call (sized after a probe call so that one call runs about
``--seconds``), one untimed call first (it builds the window table, sizes the pooled workspace and the staging),
median of ``--reps`` calls. A call is end to end at the binding: H2D of the base and the ranges, the launches on
the node stream, D2H of the hit buffer.

Baseline: ``p256_pubkey_many(gpu=True)`` in the same run on distinct consecutive scalars (the search's first
keys), end to end at the binding too, at 65,536 keys (its best measured size, docs/PERF.md "P-256 signing") and
at ``--equal-n`` keys; the search is timed at ``--equal-n`` keys as well. The results are checked equal first.
``ratio`` is the smaller of search / best baseline and search / baseline at the equal number of keys; the script
exits with status 1 when it is below ``--min-ratio`` (10).

Writes <--name>.json (default vanity_bench.json) into --out (default profiles/p256_vanity) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from upow_amd.ops.native import gpu_available, lib  # noqa: E402
from upow_amd.utils.p256 import N  # noqa: E402
from upow_amd.wallet import vanity  # noqa: E402

BASE = 0x5eed << 200
NOTHING = (42 << 256).to_bytes(33, 'big') + ((42 << 256) + 1).to_bytes(33, 'big')


def median_s(call, reps: int):
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), ts


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='profiles/p256_vanity')
    ap.add_argument('--name', default='vanity_bench', help='the result goes to <out>/<name>.json')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=2.0)
    ap.add_argument('--launches', type=int, default=0, help='full launches per timed call (0: sized for --seconds)')
    ap.add_argument('--equal-n', type=int, default=1 << 22)
    ap.add_argument('--min-ratio', type=float, default=10.0)
    a = ap.parse_args(argv)
    native = lib()
    if not gpu_available():
        sys.exit('vanity_bench: no HIP device (this measurement does not fall back to the host)')
    info = native.p256_vanity_info()
    per_launch = info['keys_per_launch']
    base_be = BASE.to_bytes(32, 'big')

    def search(count):
        total, _ = native.p256_vanity_search(base_be, count, NOTHING, 16, True)
        assert total == 0

    # the walk and the baseline agree on the first keys before anything is timed
    n_chk = 4 * info['keys_per_lane'] * info['lanes_per_block'] + 3
    keys = b''.join((BASE + i).to_bytes(32, 'big') for i in range(max(a.equal_n, 65536)))
    xy = np.frombuffer(native.p256_pubkey_many(keys[:32 * n_chk], True), dtype=np.uint8).reshape(n_chk, 64)
    walked = np.frombuffer(native.p256_vanity_walk(base_be, n_chk, True), dtype=np.uint8).reshape(n_chk, 33)
    assert (walked[:, 1:] == xy[:, :32]).all() and (walked[:, 0] == 42 + (xy[:, 32] & 1)).all(), 'walk != pubkey_many'

    search(per_launch)  # untimed
    t = time.perf_counter()
    search(per_launch)
    probe = time.perf_counter() - t
    launches = a.launches or max(1, round(a.seconds / probe))
    count = launches * per_launch
    assert BASE + count < N
    s, ts = median_s(lambda: search(count), a.reps)
    out = {'keys_per_launch': per_launch, 'launches_per_call': launches, 'keys_per_call': count, 'reps': a.reps,
           'search_call_s': [round(x, 6) for x in ts], 'search_keys_per_s': round(count / s, 1),
           'launch_ms': round(s / launches * 1e3, 3)}
    s_eq, _ = median_s(lambda: search(a.equal_n), a.reps)
    out['equal_n'] = a.equal_n
    out['search_equal_n_keys_per_s'] = round(a.equal_n / s_eq, 1)
    for name, n in (('baseline_65536', 65536), ('baseline_equal_n', a.equal_n)):
        kb = keys[:32 * n]
        s_b, _ = median_s(lambda: native.p256_pubkey_many(kb, True), a.reps)
        out[f'{name}_keys_per_s'] = round(n / s_b, 1)
    best = max(out['baseline_65536_keys_per_s'], out['baseline_equal_n_keys_per_s'])
    out['ratio_steady_vs_best_baseline'] = round(out['search_keys_per_s'] / best, 2)
    out['ratio_equal_n'] = round(out['search_equal_n_keys_per_s'] / out['baseline_equal_n_keys_per_s'], 2)
    out['ratio'] = min(out['ratio_steady_vs_best_baseline'], out['ratio_equal_n'])
    print(json.dumps(out), file=sys.stderr, flush=True)
    out['expected_seconds'] = {}
    for prefix in ('DVauLt1234'[:k] for k in range(4, 11)):
        e = vanity.expected_keys(vanity.prefix_ranges(prefix))
        out['expected_seconds'][prefix] = {'expected_keys': e, 'seconds': round(e / out['search_keys_per_s'], 3),
                                           'baseline_seconds': round(e / best, 1)}
    out['pass'] = out['ratio'] >= a.min_ratio
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name + '.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)
    return 0 if out['pass'] else 1


if __name__ == '__main__':
    sys.exit(main())
