#!/usr/bin/env python3
"""What per-instance regularization factors (LsiBatch.set_instance_regularization) cost on the configs[4] batch of scripts/time_lsi_reg.py (lock-step
LexLSI, n = 40, 5 levels x 12 rows, level 0 simple bounds, warm-started from the 0.9-perturbed neighbour, REGULARIZATION_TIKHONOV, factors
[0, 1e-3, 1e-3, 1e-3, 1e-3]) — three ways on the same data, alternating run by run within one visit, each on its own batch object:
  shared         LsiBatch.run(regularization_factors=shared): the run as it has always been;
  host_rows      set_instance_regularization((batch, nObj) numpy array) once, LsiBatch.run without factors;
  device_rows    set_instance_regularization(torch tensor) once; before every run a torch op rewrites the tensor in place (the adaptive damping
                 of a closed loop), LsiBatch.run without factors — phase 1 is device work on this route.
Every row equals the shared vector, so the three runs do the same active-set work and must return the same bits (checked every run): the
difference in time is the cost of the per-instance plumbing — a per-problem staging copy, or one small kernel plus the torch op.
Prints one JSON line with the median ms per batch of each way and its spread.
  python scripts/bench_lsi_instance_reg.py [batch] [runs]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
runs = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 25
n, dims, warmup = 40, [12] * 5, 3
shared = np.array([0, 1e-3, 1e-3, 1e-3, 1e-3])


def main():
    import torch
    from lexls_amd import capi, lexlsi, problems as P
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims) for b in range(batch)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims, perturb=0.9) for b in range(batch)])
    rows = np.tile(shared, (batch, 1))
    d_rows = torch.from_numpy(rows).to(torch.device("cuda", 0))
    d_ones = torch.ones_like(d_rows)
    srv = {k: lexlsi.LsiBatch(n, base.dims, base.types, batch) for k in ("shared", "host_rows", "device_rows")}
    srv["host_rows"].set_instance_regularization(rows)
    srv["device_rows"].set_instance_regularization(d_rows)

    def run(way, pk, **start):
        if way == "shared":
            return srv[way].run(pk, regularization_factors=shared, regularization_type=1, **start)
        if way == "device_rows":
            d_rows.mul_(d_ones)  # the loop's own update of its damping, in place (here: the same values again)
        return srv[way].run(pk, regularization_type=1, **start)

    for _ in range(3):  # library load, first launches, GPU clocks; the last result is the warm start's neighbour
        cold = {way: run(way, base) for way in srv}
    guess = np.where(cold["shared"]["active"] == 3, 0, cold["shared"]["active"]).astype(np.uint8)
    start = dict(active_guess=guess, x0=cold["shared"]["x"])
    t, same = {way: [] for way in srv}, True
    for k in range(warmup + runs):
        r = {}
        for way in srv:
            t0 = time.perf_counter()
            r[way] = run(way, pert, **start)  # (returns after the results are on the host: every stream has been waited for)
            if k >= warmup:
                t[way].append(time.perf_counter() - t0)
        for way in ("host_rows", "device_rows"):
            same = same and all(np.array_equal(np.ascontiguousarray(r[way][key].array if key == "info" else r[way][key]).view(np.uint8),
                                               np.ascontiguousarray(r["shared"][key].array if key == "info" else r["shared"][key]).view(np.uint8))
                                for key in ("x", "info", "active", "v"))

    def summary(s):
        s = np.sort(np.array(s))
        return dict(ms_per_batch=1e3 * float(np.median(s)), spread_ms=dict(min=1e3 * float(s[0]), q1=1e3 * float(np.percentile(s, 25)), q3=1e3 * float(np.percentile(s, 75)), max=1e3 * float(s[-1])))

    f = r["shared"]["info"].array[:, 4].astype(np.float64)
    res = dict(batch=batch, runs=runs, warmup=warmup, regularization_type=1, regularization_factors=shared.tolist(), library=capi.LIB_PATH,
               last_kernel={way: srv[way].last_kernel() for way in srv}, mean_factorizations=float(f.mean()), max_factorizations=int(f.max()),
               **{way: summary(t[way]) for way in srv}, same_bits_every_run=bool(same))
    for b in srv.values():
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
