"""Time lexls_lsi_batch_solve_bounds_cost_device against lexls_lsi_batch_solve_bounds_device on the same run: the flagship LexLSI workload of
scripts/bench_lsi_solve_bounds.py (n = 40, simple bounds (12) + 4 x 12, `--batch` instances in device memory), K = 1, 8, 64, 65 bound sets per
instance (the run's bounds moved by `--size` * N(0, 1)).  Both calls are timed on a run whose final factor is already formed (the second call on
a run: gather, solve_rhs and the check kernel alone), host wall clock around the host-synchronous calls, `--runs` alternated rounds after a
warm-up; one JSON line with the middle values and the ranges [min, max].

    python scripts/bench_lsi_solve_bounds_cost.py [--batch 1024] [--runs 7] [--ks 1,8,64,65] [--size 1e-3]
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
    ap.add_argument("--ks", type=str, default="1,8,64,65")
    ap.add_argument("--size", type=float, default=1e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lsi_solve_bounds_cost: no GPU (there is nothing to time without one)")
    ks = [int(k) for k in a.ks.split(",")]
    n, dims, B = 40, (12, 12, 12, 12, 12), a.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims) for i in range(B)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, B)
    up = lambda x, t: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()  # noqa: E731
    var, data = up(base.var_index.view(np.int32), np.int32), up(base.data, np.float64)
    r = b.run_device(data, var_index=var)
    solved = int((r["info"][:, 0] == 0).sum())
    total, Kmax, nobj = b.total, max(ks), len(dims)
    lb_at, ub_at, off = [], [], 0  # where the bounds live in one instance's data: per objective a column-major dim x w block, lb and ub its last two columns
    for d, t in zip(base.dims, base.types):
        w = 2 if t == 1 else n + 2
        lb_at += list(range(off + (w - 2) * int(d), off + (w - 1) * int(d)))
        ub_at += list(range(off + (w - 1) * int(d), off + w * int(d)))
        off += w * int(d)
    lb0, ub0 = data[:, torch.tensor(lb_at, device="cuda")], data[:, torch.tensor(ub_at, device="cuda")]
    gen = torch.Generator(device="cuda").manual_seed(20350601)
    size = torch.where(lb0 == ub0, torch.full_like(lb0, a.size), torch.minimum(torch.full_like(lb0, a.size), 0.1 * (ub0 - lb0)))[None]  # (lb stays below ub)
    dl = size * torch.randn((Kmax, B, total), dtype=torch.float64, device="cuda", generator=gen)
    du = size * torch.randn((Kmax, B, total), dtype=torch.float64, device="cuda", generator=gen)
    du = torch.where((lb0 == ub0)[None], dl, du)  # an equality moves as one
    lb, ub = (lb0[None] + dl).contiguous(), (ub0[None] + du).contiguous()
    x = torch.zeros((Kmax, B, n), dtype=torch.float64, device="cuda")
    viol = torch.zeros((Kmax, B), dtype=torch.float64, device="cuda")
    cost = torch.zeros((Kmax, B, nobj), dtype=torch.float64, device="cuda")
    valid = torch.zeros((B,), dtype=torch.uint8, device="cuda")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    plain = lambda K: b.solve_bounds_device(lb[:K], ub[:K], x[:K], viol[:K], valid)  # noqa: E731
    with_cost = lambda K: b.solve_bounds_device(lb[:K], ub[:K], x[:K], viol[:K], valid, cost=cost[:K])  # noqa: E731
    for _ in range(2):  # warm-up: the final factor formed, code objects loaded, buffers made, clocks up
        plain(Kmax), with_cost(Kmax), plain(1), with_cost(1)
    variant = b.last_consumer_kernel()
    rows = []
    for K in ks:
        t = {"bounds": [], "bounds_cost": []}
        for _ in range(a.runs):
            t["bounds"].append(clock(lambda: plain(K)))
            t["bounds_cost"].append(clock(lambda: with_cost(K)))
        mid = {k: float(np.median(v)) for k, v in t.items()}
        rows.append(dict(K=K, bounds_ms=mid["bounds"], bounds_cost_ms=mid["bounds_cost"], ratio=mid["bounds_cost"] / mid["bounds"],
                         ranges={k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}))
    print(json.dumps(dict(bench="lsi_solve_bounds_cost", batch=B, n=n, dims=list(dims), kernel=b.last_kernel(), variant=variant, solved=solved, size=a.size, runs=a.runs,
                          results=rows)))
    b.close()


if __name__ == "__main__":
    main()
