"""lexls_lse_solve_rhs_device on 4096 IK problems (n = 40, 5 x 12) with the factor kept, plain and damped (type 1), at K = 1, 8, 40, 64, 65 new
right-hand sides — against what the call replaces, timed in the same process: K x factorize_solve with the factor kept on problem data already in
device memory, and K single-right-hand-side calls.  Median of --reps timings per figure, device time between two events on the handle's stream.
One JSON line per (kind, K).  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_lse_solve_rhs.py`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lexls_amd  # noqa: E402
from lexls_amd import problems as P  # noqa: E402


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 40, 64, 65])
    a = ap.parse_args()
    n, dims, B = 40, [12] * 5, a.batch
    cap = sum(dims)
    lod = torch.from_numpy(P.lse_batch(20330300, B, n, dims)).cuda()
    for kind, reg in (("plain", 0), ("damped type 1", 1)):
        s = lexls_amd.BatchedLexLSE(B, n, dims, device=0)
        s.set_stream(torch.cuda.current_stream().cuda_stream)
        s.setProblemDevice(lod.data_ptr())
        if reg:
            s.setRegularization(reg, [0.1] * len(dims))
        s.factorize_solve(keep_factor=True)
        producer = s.last_kernel()
        t_fac = median_ms(lambda: s.factorize_solve(keep_factor=True), a.reps)
        for K in a.ks:
            rhs = torch.randn((K, B, cap), dtype=torch.float64, device="cuda")
            x = torch.empty((K, B, n), dtype=torch.float64, device="cuda")
            t_call = median_ms(lambda: s.solve_rhs_device(rhs, x), a.reps)
            variant = s.last_consumer_kernel()

            def singles():
                for c in range(K):
                    s.solve_rhs_device(rhs[c], x[c])
            t_single = median_ms(singles, max(3, a.reps // 3))
            floor_bytes = 8 * K * B * (cap + n)
            print(json.dumps(dict(kind=kind, K=K, variant=variant, producer=producer, solve_rhs_ms=round(t_call, 4), k_single_calls_ms=round(t_single, 4),
                                  factorize_solve_ms=round(t_fac, 4), k_refactorizations_ms=round(K * t_fac, 4), floor_bytes=floor_bytes,
                                  speedup_vs_refactorization=round(K * t_fac / t_call, 2))), flush=True)
        s.close()


if __name__ == "__main__":
    main()
