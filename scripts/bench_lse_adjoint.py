"""Time the adjoint of the LexLSE solve (lexls_lse_solve_adjoint_device, solve_adjoint<64>) on the kept factor of a batch of IK problems
(n = 40, 5 x 12) and, in the same process on the same factor, lexls_lse_residual (residual<64>): the existing sibling that walks the same
bytes and the yardstick.  Device events around `--calls` back-to-back launches in the handle's stream, `--runs` alternated runs of each after a
warm-up; prints one JSON line with the middle values, the spreads and the ratio.

    python scripts/bench_lse_adjoint.py [--batch 4096] [--calls 1000] [--runs 3]
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
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--policy", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lse_adjoint: no GPU (there is nothing to time without one)")
    n, dims = 40, [12] * 5
    s = lexls_amd.BatchedLexLSE(a.batch, n, dims)
    s.set_kernel_policy(a.policy)
    s.setProblem(P.lse_batch_fast(20290301, a.batch, n, dims))
    s.factorize_solve(keep_factor=True)
    producer = s.last_kernel()
    g = torch.from_numpy(P.normal(20290302, a.batch * n).reshape(a.batch, n)).cuda()
    grad_rhs = torch.zeros((a.batch, s.cap), dtype=torch.float64, device="cuda")
    grad_fixed = torch.zeros((a.batch, n), dtype=torch.float64, device="cuda")
    lib = capi.lib()

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

    names = {}
    for fn in (adjoint, residual):  # warm-up: code objects loaded, clocks up
        for _ in range(20):
            fn()
        names[fn.__name__] = s.last_consumer_kernel()
    torch.cuda.synchronize()
    t = {"adjoint": [], "residual": []}
    for _ in range(a.runs):
        t["adjoint"].append(timed(adjoint))
        t["residual"].append(timed(residual))
    mid = {k: float(np.median(v)) for k, v in t.items()}
    # what the algorithm has to move per problem: the factor's [R | T] rows, reflectors and multipliers once (the stored factor without its
    # right-hand-side column is an upper bound), g in, the two gradients out
    bytes_adjoint = 8 * (s.cap * n + n + s.cap + n)
    print(json.dumps(dict(bench="lse_adjoint", batch=a.batch, n=n, dims=dims, producer=producer, kernels=names, calls=a.calls, runs=a.runs,
                          adjoint_us=mid["adjoint"], adjoint_us_runs=t["adjoint"], residual_us=mid["residual"], residual_us_runs=t["residual"],
                          spread_adjoint=(max(t["adjoint"]) - min(t["adjoint"])) / mid["adjoint"],
                          spread_residual=(max(t["residual"]) - min(t["residual"])) / mid["residual"],
                          ratio=mid["adjoint"] / mid["residual"], adjoint_GBps=bytes_adjoint * a.batch / mid["adjoint"] * 1e-3)))
    s.close()


if __name__ == "__main__":
    main()
