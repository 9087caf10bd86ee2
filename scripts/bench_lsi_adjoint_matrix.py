"""Time the gradients of a LexLSI batch with respect to its constraint data (lexls_lsi_batch_solve_adjoint_matrix_device) on the flagship LexLSI
workload, next to the gradients with respect to the bounds (lexls_lsi_batch_solve_adjoint_device): n = 40, simple bounds (12) + 4 x 12, `--batch`
instances in device memory, warm-started from the solution of the unperturbed neighbour as bench.py's lsi workload is.  Host wall clock around the
host-synchronous calls, `--runs` rounds after a warm-up, the two gradients alternated (which comes first changes from round to round); one JSON
line with the middle values and the ranges [min, max] of
    matrix_first_ms   solve_adjoint_matrix_device right behind a run: forming and factorizing the final problems, their x, the chain, the scatter
    matrix_again_ms   a second g on the same run: the chain and the scatter alone
    bounds_first_ms / bounds_again_ms   the same two for solve_adjoint_device
    lambda_ms         run_device(..., with_lambda=True) minus run_device without it
    run_ms            the warm run itself
and ratio_again = matrix_again_ms / bounds_again_ms, floor_us = the bytes grad_data writes at 8 TB/s, differentiable = the share of instances that
come back with flag 1 (solved = those that ended PROBLEM_SOLVED).

    python scripts/bench_lsi_adjoint_matrix.py [--batch 1024] [--runs 7]
    python scripts/bench_lsi_adjoint_matrix.py --loop 20      # 20 second-g calls and nothing else timed: the run to put under a kernel profiler
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lexls_amd import lexlsi, problems as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--loop", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsi_adjoint_matrix: no GPU (there is nothing to time without one)")
    n, dims, B = 40, (12, 12, 12, 12, 12), a.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims) for i in range(B)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims, perturb=0.9) for i in range(B)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, B)
    up = lambda x, t: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()  # noqa: E731
    var = up(base.var_index.view(np.int32), np.int32)
    cold = b.run_device(up(base.data, np.float64), var_index=var)
    guess = torch.where(cold["active"] == 3, torch.zeros_like(cold["active"]), cold["active"]).contiguous()  # (equalities are activated by the driver itself)
    x0, data = cold["x"].clone(), up(pert.data, np.float64)
    g = up(P.normal(20300901, B * n).reshape(B, n), np.float64)
    g2 = up(P.normal(20300902, B * n).reshape(B, n), np.float64)
    grad_lb, grad_ub = (torch.zeros((B, b.total), dtype=torch.float64, device="cuda") for _ in range(2))
    grad_data = torch.zeros((B, b.per_data), dtype=torch.float64, device="cuda")
    flags = torch.zeros((B,), dtype=torch.uint8, device="cuda")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    run = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0)  # noqa: E731
    run_lam = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0, with_lambda=True)  # noqa: E731
    adj = lambda gg=g: b.solve_adjoint_device(gg, grad_lb, grad_ub)  # noqa: E731
    mat = lambda gg=g: b.solve_adjoint_matrix_device(gg, grad_data, flags)  # noqa: E731
    for _ in range(3):  # warm-up: code objects loaded, buffers made, clocks up
        run_lam(), run(), adj(), mat(), run(), mat(), adj()
    if a.loop:
        run()
        for _ in range(a.loop):
            mat(g2)
        print(json.dumps(dict(bench="lsi_adjoint_matrix", loop=a.loop)))
        b.close()
        return
    solved = int((run()["info"][:, 0] == 0).sum())
    mat()
    differentiable = int(flags.sum())
    t = {k: [] for k in ("run", "run_lam", "matrix_first", "matrix_again", "bounds_first", "bounds_again")}
    for r in range(a.runs):
        for what in (("matrix", "lam", "bounds") if r % 2 == 0 else ("bounds", "lam", "matrix")):
            if what == "lam":
                t["run_lam"].append(clock(run_lam))
                continue
            fn = mat if what == "matrix" else adj
            t["run"].append(clock(run))
            t[what + "_first"].append(clock(fn))
            t[what + "_again"].append(clock(lambda: fn(g2)))
    mid = {k: float(np.median(v)) for k, v in t.items()}
    rng = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    print(json.dumps(dict(bench="lsi_adjoint_matrix", batch=B, n=n, dims=list(dims), kernel=b.last_kernel(), solved=solved, differentiable=differentiable,
                          differentiable_share=differentiable / B, runs=a.runs,
                          matrix_first_ms=mid["matrix_first"], matrix_again_ms=mid["matrix_again"], bounds_first_ms=mid["bounds_first"],
                          bounds_again_ms=mid["bounds_again"], ratio_again=mid["matrix_again"] / mid["bounds_again"],
                          ratio_first=mid["matrix_first"] / mid["bounds_first"], lambda_ms=mid["run_lam"] - mid["run"], run_ms=mid["run"],
                          grad_data_bytes=8 * B * b.per_data, floor_us=8 * B * b.per_data / 8e12 * 1e6, ranges=rng)))
    b.close()


if __name__ == "__main__":
    main()
