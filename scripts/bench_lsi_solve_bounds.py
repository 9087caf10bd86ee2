"""Time the re-solve of a LexLSI batch's final working sets on new bounds (lexls_lsi_batch_solve_bounds_device) on the flagship LexLSI workload:
n = 40, simple bounds (12) + 4 x 12, `--batch` instances in device memory, warm-started from the solution of the unperturbed neighbour as
bench.py's lsi workload is, for K = 1, 8, 64, 65 bound sets per instance (the run's bounds moved by `--size` * N(0, 1)).  Next to it, in the same
session, the only way to the same answers without the call: K warm run_device steps, each on the data with one set's bounds written in, started
from the run's x and working set.  Host wall clock around the host-synchronous calls, `--runs` alternated rounds after a warm-up; one JSON line
with the middle values and the ranges [min, max] of
    bounds_first_ms   the call right behind a run: forming and factorizing the final problems, then gather, solve_rhs and check
    bounds_again_ms   a second call on the same run: gather, solve_rhs and check alone
    steps_ms          K warm run_device steps (step_ms = one of them)
and, for lsi_bounds_check_kernel, floor_us: the constraint data read once per instance and tile of 64 sets, lb / ub and x once, x written once,
at 8 TB/s.  pays_from_K = the smallest K of the list at which bounds_first_ms is below steps_ms.  held = how many (instance, set) pairs of the
largest K the warm steps ended on the run's working set with, and max_dx_gap = the largest |x_step - x_call| among those, relative to
max(1, |x|): the answers are the same ones.
Per-kernel times (lsi_bounds_gather_kernel, the solve_rhs kernel, lsi_bounds_check_kernel) come from a kernel trace of this script in a run of
its own: rocprofv3 --kernel-trace --stats -- python scripts/bench_lsi_solve_bounds.py --runs 1

    python scripts/bench_lsi_solve_bounds.py [--batch 1024] [--runs 5] [--ks 1,8,64,65] [--size 1e-3]
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
    ap.add_argument("--ks", type=str, default="1,8,64,65")
    ap.add_argument("--size", type=float, default=1e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsi_solve_bounds: no GPU (there is nothing to time without one)")
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
    total, Kmax = b.total, max(ks)
    # where the bounds live in one instance's data: per objective a column-major dim x w block, lb and ub its last two columns
    lb_at, ub_at, off = [], [], 0
    for d, t in zip(base.dims, base.types):
        w = 2 if t == 1 else n + 2
        lb_at += list(range(off + (w - 2) * int(d), off + (w - 1) * int(d)))
        ub_at += list(range(off + (w - 1) * int(d), off + w * int(d)))
        off += w * int(d)
    lb_at, ub_at = torch.tensor(lb_at, device="cuda"), torch.tensor(ub_at, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(20340601)
    lb0, ub0 = data[:, lb_at], data[:, ub_at]
    size = torch.where(lb0 == ub0, torch.full_like(lb0, a.size), torch.minimum(torch.full_like(lb0, a.size), 0.1 * (ub0 - lb0)))[None]  # (lb stays below ub)
    dl = size * torch.randn((Kmax, B, total), dtype=torch.float64, device="cuda", generator=gen)
    du = size * torch.randn((Kmax, B, total), dtype=torch.float64, device="cuda", generator=gen)
    du = torch.where((lb0 == ub0)[None], dl, du)  # an equality moves as one
    lb, ub = (lb0[None] + dl).contiguous(), (ub0[None] + du).contiguous()
    x = torch.zeros((Kmax, B, n), dtype=torch.float64, device="cuda")
    viol = torch.zeros((Kmax, B), dtype=torch.float64, device="cuda")
    valid = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    nd = min(Kmax, 8)  # the warm steps cycle through the data of the first nd sets
    datas = []
    for c in range(nd):
        d = data.clone()
        d[:, lb_at], d[:, ub_at] = lb[c], ub[c]
        datas.append(d)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    run = lambda: b.run_device(data, var_index=var, active_guess=guess, x0=x0)  # noqa: E731

    def bounds(K):
        b.solve_bounds_device(lb[:K], ub[:K], x[:K], viol[:K], valid)

    r = run()
    ws = torch.where(r["active"] == 3, torch.zeros_like(r["active"]), r["active"]).contiguous()
    x_run = r["x"].clone()

    def steps(K):
        for c in range(K):
            b.run_device(datas[c % nd], var_index=var, active_guess=ws, x0=x_run)

    for _ in range(2):  # warm-up: code objects loaded, buffers made, clocks up
        run(), bounds(Kmax), bounds(1), steps(2)
    solved = int((run()["info"][:, 0] == 0).sum())
    bounds(nd)
    held, gap = 0, 0.0
    for c in range(nd):  # the same answers: where a warm step ends on the run's working set its x is the call's
        s = b.run_device(datas[c], var_index=var, active_guess=ws, x0=x_run)
        same = ((s["active"] == r["active"]).all(dim=1) & (s["info"][:, 0] == 0) & (r["info"][:, 0] == 0))
        held += int(same.sum())
        if bool(same.any()):
            gap = max(gap, float(((s["x"] - x[c]).abs().amax(dim=1) / x[c].abs().amax(dim=1).clamp(min=1.0))[same].max()))
    run()
    variant = b.last_consumer_kernel() if hasattr(b, "last_consumer_kernel") else ""
    rows, pays = [], None
    for K in ks:
        t = {k: [] for k in ("run", "bounds_first", "bounds_again", "steps")}
        for _ in range(a.runs):
            t["run"].append(clock(run))
            t["bounds_first"].append(clock(lambda: bounds(K)))
            t["bounds_again"].append(clock(lambda: bounds(K)))
            t["steps"].append(clock(lambda: steps(K)))
        mid = {k: float(np.median(v)) for k, v in t.items()}
        tiles = (K + 63) // 64
        floor = 8 * (B * tiles * b.per_data + 2 * K * B * total + 2 * K * B * n) / 8e12 * 1e6
        if pays is None and mid["bounds_first"] < mid["steps"]:
            pays = K
        rows.append(dict(K=K, bounds_first_ms=mid["bounds_first"], bounds_again_ms=mid["bounds_again"], steps_ms=mid["steps"], step_ms=mid["steps"] / K,
                         run_ms=mid["run"], check_floor_us=floor, ranges={k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}))
    print(json.dumps(dict(bench="lsi_solve_bounds", batch=B, n=n, dims=list(dims), kernel=b.last_kernel(), variant=variant, solved=solved, size=a.size,
                          held=[held, nd * B], max_dx_gap=gap, pays_from_K=pays, runs=a.runs, results=rows)))
    b.close()


if __name__ == "__main__":
    main()
