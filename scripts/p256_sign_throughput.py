"""Batched P-256 signing and key derivation: the GPU kernels against the host signer on 16 threads.

For n in 256 .. 531,200 distinct random keys: wall time of ``p256_sign_many`` / ``p256_pubkey_many`` with
gpu=True (packing into pinned staging, H2D, kernel, D2H, the scrub of the key buffers), after one untimed call
of the same size (it grows the pooled buffers), median of 5; and of ``p256_sign_batch`` / ``p256_pubkey_batch``
at 16 threads in the same process (median of 3 at 531,200). The results are checked equal before anything is timed. ``gpu_min`` is the
smallest measured n at which the GPU wins by >= 20 % for both functions: the default of SIGN_GPU_MIN
(upow_amd/ops/p256.py). Last, the saturating batch through the one-lane verify kernel (UPOW_P256_VARIANT=1) in
the same session: a signature does less curve work than a verify, so signing should not be slower per item.

Writes p256_sign_throughput.json and .txt into --out (default profiles/p256_sign) and prints the JSON."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from upow_amd.ops.native import gpu_available, lib  # noqa: E402
from upow_amd.ops import p256 as op  # noqa: E402

SIZES = (256, 1024, 8300, 65536, 531200)
HOST_THREADS = 16
WIN = 1.2  # the GPU must be this much faster: a margin over the +-7 % spread of host-bound stages


def median_s(call, reps: int) -> float:
    call()  # untimed: sizes pinned staging and pooled device buffers, warms the table and the host pool
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='profiles/p256_sign')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
    a = ap.parse_args(argv)
    if a.reps < 5:
        ap.error('--reps must be at least 5')
    native = lib()
    if not gpu_available():
        sys.exit('p256_sign_throughput: no HIP device (this measurement does not fall back to the host)')
    import torch
    torch.cuda.set_device(0)
    rng = random.Random(6979)
    top = max(a.sizes)
    keys = b''.join(rng.randrange(1, op.oracle.N).to_bytes(32, 'big') for _ in range(top))
    digests = rng.randbytes(32 * top)
    rows = []
    for n in sorted(a.sizes):
        kb, db = keys[:32 * n], digests[:32 * n]
        sig = native.p256_sign_many(kb, db, True)
        pub = native.p256_pubkey_many(kb, True)
        assert sig == native.p256_sign_batch(kb, db, HOST_THREADS), f'sign mismatch at n={n}'
        assert pub == native.p256_pubkey_batch(kb, HOST_THREADS), f'pubkey mismatch at n={n}'
        host_reps = a.reps if n <= 65536 else 3  # the host takes tens of seconds per call at the top size
        row = {'n': n,
               'sign_gpu_s': median_s(lambda: native.p256_sign_many(kb, db, True), a.reps),
               'sign_host16_s': median_s(lambda: native.p256_sign_batch(kb, db, HOST_THREADS), host_reps),
               'pubkey_gpu_s': median_s(lambda: native.p256_pubkey_many(kb, True), a.reps),
               'pubkey_host16_s': median_s(lambda: native.p256_pubkey_batch(kb, HOST_THREADS), host_reps)}
        for f in ('sign', 'pubkey'):
            row[f'{f}_gpu_per_s'] = round(n / row[f'{f}_gpu_s'], 1)
            row[f'{f}_host16_per_s'] = round(n / row[f'{f}_host16_s'], 1)
            row[f'{f}_speedup'] = round(row[f'{f}_host16_s'] / row[f'{f}_gpu_s'], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    gpu_min = None  # the smallest measured n from which the GPU wins at every larger measured n too
    for r in reversed(rows):
        if r['sign_speedup'] < WIN or r['pubkey_speedup'] < WIN:
            break
        gpu_min = r['n']
    out = {'host_threads': HOST_THREADS, 'reps': a.reps, 'rows': rows, 'gpu_min': gpu_min}
    # signing against the one-lane verify kernel at the saturating size, records from distinct signers
    n = top
    recs = np.empty((n, 160), dtype=np.uint8)
    recs[:, :64] = np.frombuffer(native.p256_pubkey_many(keys, True), dtype=np.uint8).reshape(n, 64)
    recs[:, 64:128] = np.frombuffer(native.p256_sign_many(keys, digests, True), dtype=np.uint8).reshape(n, 64)
    recs[:, 128:] = np.frombuffer(digests, dtype=np.uint8).reshape(n, 32)
    os.environ['UPOW_P256_VARIANT'] = '1'
    assert (op.verify_records(recs, device='gpu') == op.VALID).all()
    verify_s = median_s(lambda: op.verify_records(recs, device='gpu'), a.reps)
    os.environ.pop('UPOW_P256_VARIANT')
    sign_s = rows[-1]['sign_gpu_s']
    out['saturating'] = {'n': n, 'sign_gpu_us_per_item': round(sign_s / n * 1e6, 4),
                         'verify_one_lane_gpu_us_per_item': round(verify_s / n * 1e6, 4),
                         'sign_not_slower_than_verify': sign_s <= verify_s}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'p256_sign_throughput.json'), 'w') as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, 'p256_sign_throughput.txt'), 'w') as f:
        f.write(f'{"n":>8} {"sign GPU/s":>12} {"sign host16/s":>14} {"x":>6} {"pubkey GPU/s":>13} '
                f'{"pubkey host16/s":>16} {"x":>6}\n')
        for r in rows:
            f.write(f'{r["n"]:>8} {r["sign_gpu_per_s"]:>12.0f} {r["sign_host16_per_s"]:>14.0f} {r["sign_speedup"]:>6.2f} '
                    f'{r["pubkey_gpu_per_s"]:>13.0f} {r["pubkey_host16_per_s"]:>16.0f} {r["pubkey_speedup"]:>6.2f}\n')
        f.write(f'gpu_min (GPU >= {WIN}x host on both): {out["gpu_min"]}\n')
        f.write(f'saturating batch: {json.dumps(out["saturating"])}\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
