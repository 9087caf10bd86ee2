"""lexls_lse_residual_rhs_device (v, cost and x in one call) on 4096 IK problems (n = 40, 5 x 12) with the factor kept, at K = 1, 8, 40, 64, 65 new
right-hand sides — against what the call replaces, timed in the same process: K x (factorize_solve with the factor kept on problem data already in
device memory + lexls_lse_residual), and against lexls_lse_solve_rhs_device alone on the same factor (what the residuals cost on top of x).
Median of --reps timings per figure, with the range [min, max], device time between two events on the handle's stream.  One JSON line per K.
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/bench_lse_residual_rhs.py`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lexls_amd  # noqa: E402
from lexls_amd import capi, problems as P  # noqa: E402


def timed_ms(fn, reps, warmup=3):
    """(median, min, max) of reps timings"""
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
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 40, 64, 65])
    a = ap.parse_args()
    n, dims, B = 40, [12] * 5, a.batch
    cap, nobj = sum(dims), len(dims)
    lod = torch.from_numpy(P.lse_batch(20330300, B, n, dims)).cuda()
    s = lexls_amd.BatchedLexLSE(B, n, dims, device=0)
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    s.setProblemDevice(lod.data_ptr())
    s.factorize_solve(keep_factor=True)
    producer = s.last_kernel()

    def refactorize():
        s.factorize_solve(keep_factor=True)
        capi.check(capi.lib().lexls_lse_residual(s._h))

    t_fac = timed_ms(refactorize, a.reps)
    for K in a.ks:
        rhs = torch.randn((K, B, cap), dtype=torch.float64, device="cuda")
        x = torch.empty((K, B, n), dtype=torch.float64, device="cuda")
        v = torch.empty((K, B, cap), dtype=torch.float64, device="cuda")
        cost = torch.empty((K, B, nobj), dtype=torch.float64, device="cuda")
        t_res = timed_ms(lambda: s.residual_rhs_device(rhs, v, cost, x), a.reps)
        variant = s.last_consumer_kernel()
        t_cost = timed_ms(lambda: s.residual_rhs_device(rhs, None, cost, None), a.reps)
        t_x = timed_ms(lambda: s.solve_rhs_device(rhs, x), a.reps)
        floor_bytes = 8 * K * B * (2 * cap + n + nobj)
        print(json.dumps(dict(K=K, variant=variant, producer=producer, residual_rhs_ms=round(t_res[0], 4), residual_rhs_range=[round(t_res[1], 4), round(t_res[2], 4)],
                              cost_only_ms=round(t_cost[0], 4), solve_rhs_ms=round(t_x[0], 4), solve_rhs_range=[round(t_x[1], 4), round(t_x[2], 4)],
                              over_solve_rhs=round(t_res[0] / t_x[0], 2), refactorize_residual_ms=round(t_fac[0], 4),
                              k_refactorizations_ms=round(K * t_fac[0], 4), floor_bytes=floor_bytes, speedup_vs_refactorization=round(K * t_fac[0] / t_res[0], 2))), flush=True)
    s.close()


if __name__ == "__main__":
    main()
