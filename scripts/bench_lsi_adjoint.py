"""Time the gradients of a LexLSI batch with respect to its bounds (lexls_lsi_batch_solve_adjoint_device) on the flagship LexLSI workload: n = 40,
simple bounds (12) + 4 x 12, `--batch` instances in device memory, warm-started from the solution of the unperturbed neighbour as bench.py's lsi
workload is.  Host wall clock around the host-synchronous calls, `--runs` alternated rounds after a warm-up; one JSON line with the middle values and
the spreads (max - min over the middle value) of
    (a) first_ms   solve_adjoint_device right behind a run: forming and factorizing the final equality problems, the adjoint, the scatter
    (b) again_ms   a second call on the same run: the adjoint and the scatter alone (the kept factor is reused)
    (c) lambda_ms  run_device(..., with_lambda=True) minus run_device without it, same process: the yardstick for (a) — both pay the same
                   formation and factorization
and run_ms, the warm run itself.

    python scripts/bench_lsi_adjoint.py [--batch 1024] [--runs 7]
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsi_adjoint: no GPU (there is nothing to time without one)")
    n, dims, B = 40, (12, 12, 12, 12, 12), a.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims) for i in range(B)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims, perturb=0.9) for i in range(B)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, B)
    up = lambda x, t: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()
    var = up(base.var_index.view(np.int32), np.int32)
    cold = b.run_device(up(base.data, np.float64), var_index=var)
    guess = torch.where(cold["active"] == 3, torch.zeros_like(cold["active"]), cold["active"]).contiguous()  # (equalities are activated by the driver itself)
    x0, data = cold["x"].clone(), up(pert.data, np.float64)
    g = up(P.normal(20300901, B * n).reshape(B, n), np.float64)
    grad_lb, grad_ub = (torch.zeros((B, b.total), dtype=torch.float64, device="cuda") for _ in range(2))

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    run = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0)
    run_lam = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0, with_lambda=True)
    adj = lambda: b.solve_adjoint_device(g, grad_lb, grad_ub)
    for _ in range(3):  # warm-up: code objects loaded, buffers made, clocks up
        run_lam(), run(), adj(), adj()
    solved = int((run()["info"][:, 0] == 0).sum())
    t = dict(run=[], run_lam=[], first=[], again=[])
    for r in range(a.runs):
        order = ("plain", "lam") if r % 2 == 0 else ("lam", "plain")
        for what in order:
            if what == "lam":
                t["run_lam"].append(clock(run_lam))
            else:
                t["run"].append(clock(run))
                t["first"].append(clock(adj))
                t["again"].append(clock(adj))
    mid = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / mid[k] for k, v in t.items()}
    print(json.dumps(dict(bench="lsi_adjoint", batch=B, n=n, dims=list(dims), kernel=b.last_kernel(), solved=solved, runs=a.runs,
                          first_ms=mid["first"], again_ms=mid["again"], lambda_ms=mid["run_lam"] - mid["run"], run_ms=mid["run"], run_lambda_ms=mid["run_lam"],
                          spread={k: round(v, 3) for k, v in spread.items()}, first_ms_runs=t["first"], again_ms_runs=t["again"],
                          run_ms_runs=t["run"], run_lambda_ms_runs=t["run_lam"])))
    b.close()


if __name__ == "__main__":
    main()
