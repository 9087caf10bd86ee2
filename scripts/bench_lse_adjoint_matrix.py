"""Time the gradient of the LexLSE solve with respect to the matrix (lexls_lse_solve_adjoint_matrix_device, "solve_adjoint_matrix<64>": the chain
solve_adjoint -> level search -> sensitivity of level k* -> apply_solve_map -> assembly) on the kept factor of a batch of IK problems (n = 40,
5 x 12) and, in the same process on the same factor, lexls_lse_solve_adjoint_device (solve_adjoint<64>) and lexls_lse_residual (residual<64>),
the yardsticks.  Device events around `--calls` back-to-back calls in the handle's stream, `--runs` alternated runs of each after a warm-up;
prints one JSON line with the middle values and the spreads.  The floor of the call: it writes batch x 41 x 60 x 8 bytes and reads the factor
of the same size at least twice.

    python scripts/bench_lse_adjoint_matrix.py [--batch 4096] [--calls 200] [--runs 3]

Per-kernel times of the chain: the same script, in a run of its own, under the profiler's kernel trace —
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_lse_adjoint_matrix.py --calls 50 --runs 1
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lexls_amd  # noqa: E402
from lexls_amd import capi, problems as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--policy", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lse_adjoint_matrix: no GPU (there is nothing to time without one)")
    n, dims = 40, [12] * 5
    s = lexls_amd.BatchedLexLSE(a.batch, n, dims)
    s.set_kernel_policy(a.policy)
    s.setProblem(P.lse_batch_fast(20290301, a.batch, n, dims))
    s.factorize_solve(keep_factor=True)
    producer = s.last_kernel()
    g = torch.from_numpy(P.normal(20290302, a.batch * n).reshape(a.batch, n)).cuda()
    grad_lod = torch.zeros((a.batch, n + 1, s.cap), dtype=torch.float64, device="cuda")
    flags = torch.zeros((a.batch,), dtype=torch.uint8, device="cuda")
    grad_rhs = torch.zeros((a.batch, s.cap), dtype=torch.float64, device="cuda")
    grad_fixed = torch.zeros((a.batch, n), dtype=torch.float64, device="cuda")
    lib = capi.lib()

    def matrix():
        capi.check(lib.lexls_lse_solve_adjoint_matrix_device(s._h, C.c_void_p(g.data_ptr()), C.c_void_p(grad_lod.data_ptr()), C.c_void_p(flags.data_ptr())))

    def adjoint():
        capi.check(lib.lexls_lse_solve_adjoint_device(s._h, C.c_void_p(g.data_ptr()), C.c_void_p(grad_rhs.data_ptr()), C.c_void_p(grad_fixed.data_ptr())))

    def residual():
        capi.check(lib.lexls_lse_residual(s._h))

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.calls  # microseconds per call

    fns = (matrix, adjoint, residual)
    names = {}
    for fn in fns:  # warm-up: code objects loaded, work buffers made, clocks up
        for _ in range(20):
            fn()
        names[fn.__name__] = s.last_consumer_kernel()
    torch.cuda.synchronize()
    stable = int(flags.sum().item())
    t = {fn.__name__: [] for fn in fns}
    for _ in range(a.runs):
        for fn in fns:
            t[fn.__name__].append(timed(fn))
    mid = {k: float(np.median(v)) for k, v in t.items()}
    out_bytes = 8 * a.batch * (n + 1) * s.cap
    floor_us = 3 * out_bytes / 8e12 * 1e6  # the gradient written once, the factor read twice, at 8 TB/s
    print(json.dumps(dict(bench="lse_adjoint_matrix", batch=a.batch, n=n, dims=dims, producer=producer, kernels=names, calls=a.calls, runs=a.runs,
                          rank_stable=stable, matrix_us=mid["matrix"], adjoint_us=mid["adjoint"], residual_us=mid["residual"], us_runs=t,
                          spread={k: (max(v) - min(v)) / mid[k] for k, v in t.items()}, floor_us=floor_us, matrix_over_floor=mid["matrix"] / floor_us,
                          matrix_over_adjoint=mid["matrix"] / mid["adjoint"], written_GBps=out_bytes / mid["matrix"] * 1e-3)))
    s.close()


if __name__ == "__main__":
    main()
