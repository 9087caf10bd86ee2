#!/usr/bin/env python3
"""The configs[4] batch of scripts/bench_lsi.py (lock-step LexLSI, n = 40, 5 levels x 12 rows, level 0 simple bounds, warm-started from the
0.9-perturbed neighbour) REGULARIZED: regularization_type 1, factors [0, 1e-3, 1e-3, 1e-3, 1e-3].  One batch object, warm-up runs, then the
median of the timed runs with their spread.  Prints one JSON line: ms per batch, factorizations per second, the kernel that served the
resident iterations (LsiBatch.last_kernel; "n/a" on a library that predates it).
  python scripts/time_lsi_reg.py [batch] [runs] [regularization_type]        (runs unchanged in a checkout of an earlier commit, for an A/B)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lexls_amd import capi, lexlsi, problems as P  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
runs = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 25
reg = dict(regularization_type=int(sys.argv[3]) if len(sys.argv) > 3 else 1, regularization_factors=[0, 1e-3, 1e-3, 1e-3, 1e-3])
n, dims = 40, [12] * 5
base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims) for b in range(batch)])
pert = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims, perturb=0.9) for b in range(batch)])
has_name = hasattr(lexlsi.LsiBatch, "last_kernel")
srv = lexlsi.LsiBatch(n, base.dims, base.types, batch)
for _ in range(3):  # warm-up: library load, first launches, GPU clocks; the last result is the warm start's neighbour
    cold = srv.run(base, **reg)
guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
for _ in range(3):
    r = srv.run(pert, active_guess=guess, x0=cold["x"], **reg)
t = []
for _ in range(runs):
    t0 = time.perf_counter()
    r = srv.run(pert, active_guess=guess, x0=cold["x"], **reg)  # (returns after the results are on the host: every stream has been waited for)
    t.append(time.perf_counter() - t0)
kernel = srv.last_kernel() if has_name else "n/a"
stats = srv.stats()
srv.close()
t = np.sort(np.array(t))
f = np.array([i["factorizations"] for i in r["info"]], np.float64)
med = float(np.median(t))
print(json.dumps(dict(batch=batch, runs=runs, **{k: v for k, v in reg.items()}, library=capi.LIB_PATH, last_kernel=kernel,
                      ms_per_batch=1e3 * med, spread_ms=dict(min=1e3 * float(t[0]), q1=1e3 * float(np.percentile(t, 25)), q3=1e3 * float(np.percentile(t, 75)), max=1e3 * float(t[-1])),
                      factorizations_per_s=float(f.sum()) / med, mean_factorizations=float(f.mean()), max_factorizations=int(f.max()),
                      solved=int(sum(i["status"] == 0 for i in r["info"])), stages=stats,
                      x_checksum=float(np.abs(r["x"]).sum()))))
