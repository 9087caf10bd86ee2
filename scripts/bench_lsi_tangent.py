"""Time the forward-mode tangents of a LexLSI batch with respect to its constraint data (lexls_lsi_batch_solve_tangent_device) on the flagship
LexLSI workload: n = 40, simple bounds (12) + 4 x 12, `--batch` instances in device memory, warm-started from the solution of the unperturbed
neighbour as bench.py's lsi workload is, for K = 1, 8, 40, 64, 65 directions per instance.  Next to it, on the same run: K single-direction calls,
and lexls_lsi_batch_solve_adjoint_matrix_device — nVar calls of which on unit cotangents gave the same quantity before.  Host wall clock around
the host-synchronous calls, `--runs` alternated rounds after a warm-up; one JSON line with the middle values and the ranges [min, max] of
    tangent_first_ms   the call right behind a run: forming and factorizing the final problems, their x, the gather, the chain
    tangent_again_ms   a second call on the same run: the gather and the chain alone
    singles_ms         K calls of one direction each, on the same run
    matrix_again_ms    one matrix adjoint on the same run (nvar_matrix_ms = nVar times it)
and floor_us = the bytes of K x ddata read once at 8 TB/s.

    python scripts/bench_lsi_tangent.py [--batch 1024] [--runs 5] [--ks 1,8,40,64,65]
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ks", type=str, default="1,8,40,64,65")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsi_tangent: no GPU (there is nothing to time without one)")
    ks = [int(k) for k in a.ks.split(",")]
    n, dims, B = 40, (12, 12, 12, 12, 12), a.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims) for i in range(B)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims, perturb=0.9) for i in range(B)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, B)
    up = lambda x, t: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()  # noqa: E731
    var = up(base.var_index.view(np.int32), np.int32)
    cold = b.run_device(up(base.data, np.float64), var_index=var)
    guess = torch.where(cold["active"] == 3, torch.zeros_like(cold["active"]), cold["active"]).contiguous()  # (equalities are activated by the driver itself)
    x0, data = cold["x"].clone(), up(pert.data, np.float64)
    gen = torch.Generator(device="cuda").manual_seed(20330402)
    ddata = torch.randn((max(ks), B, b.per_data), dtype=torch.float64, device="cuda", generator=gen)
    dx = torch.zeros((max(ks), B, n), dtype=torch.float64, device="cuda")
    flags = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    g = up(P.normal(20300901, B * n).reshape(B, n), np.float64)
    grad_data = torch.zeros((B, b.per_data), dtype=torch.float64, device="cuda")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    run = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0)  # noqa: E731
    mat = lambda: b.solve_adjoint_matrix_device(g, grad_data, flags)  # noqa: E731

    def tangent(K):
        b.solve_tangent_device(ddata[:K], dx[:K], flags)

    def singles(K):
        for c in range(K):
            b.solve_tangent_device(ddata[c], dx[c], flags)

    for _ in range(2):  # warm-up: code objects loaded, buffers made, clocks up
        run(), tangent(max(ks)), tangent(1), mat()
    solved = int((run()["info"][:, 0] == 0).sum())
    tangent(1)
    differentiable = int(flags.sum())
    rows = []
    for K in ks:
        t = {k: [] for k in ("run", "tangent_first", "tangent_again", "singles", "matrix_again")}
        for _ in range(a.runs):
            t["run"].append(clock(run))
            t["tangent_first"].append(clock(lambda: tangent(K)))
            t["tangent_again"].append(clock(lambda: tangent(K)))
            t["matrix_again"].append(clock(mat))
            t["singles"].append(clock(lambda: singles(K)))
        mid = {k: float(np.median(v)) for k, v in t.items()}
        rows.append(dict(K=K, tangent_first_ms=mid["tangent_first"], tangent_again_ms=mid["tangent_again"], singles_ms=mid["singles"],
                         matrix_again_ms=mid["matrix_again"], nvar_matrix_ms=n * mid["matrix_again"], run_ms=mid["run"],
                         floor_us=8 * K * B * b.per_data / 8e12 * 1e6, ranges={k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}))
    print(json.dumps(dict(bench="lsi_tangent", batch=B, n=n, dims=list(dims), kernel=b.last_kernel(), solved=solved, differentiable=differentiable,
                          runs=a.runs, results=rows)))
    b.close()


if __name__ == "__main__":
    main()
