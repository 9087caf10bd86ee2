"""Time a degenerate configs[4]-shaped batch (1024 instances of n = 40, 5 x 12, objective 0 simple bounds) with cycling handling on
(ParametersLexLSI::cycling_handling_enabled): the later objectives repeat rows of the first general one with a conflicting interval and
tol_wrong_sign_lambda is 0, so the instances REMOVE and re-ADD the same constraint and the handler relaxes bounds (random instances of this
shape never do).

    python scripts/bench_lsi_cycling.py [--batch 1024] [--reps 3] [--warmup 1] [--max-counter 3] [--relax-step 1e-6]

Prints one JSON line: milliseconds per run, the kernel that served the resident iterations, the outcomes and the relaxations done.  Uses the
public Python binding only, so the same file times any commit of the library (a commit whose cycling runs take the host path reports kernel
"host"; one without LsiBatch.cycling_counters reports no relaxation count)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import lexlsi, problems as P  # noqa: E402


def degenerate(seed, n, dims):
    """every general objective behind the first one repeats the first half of the first one's rows, its interval moved past their upper bound"""
    objs = P.lsi_problem(seed, n, dims)
    general = [k for k, o in enumerate(objs) if "A" in o]
    g0 = objs[general[0]]
    for k in general[1:]:
        o = objs[k]
        r = max(1, min(len(o["lb"]), len(g0["lb"])) // 2)
        o["A"][:r] = g0["A"][:r]
        o["lb"][:r] = g0["ub"][:r] + 0.5
        o["ub"][:r] = o["lb"][:r] if k == len(objs) - 1 else o["lb"][:r] + (g0["ub"][:r] - g0["lb"][:r])
    return objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-counter", type=int, default=3)
    ap.add_argument("--relax-step", type=float, default=1e-6)
    args = ap.parse_args()
    n, dims = 40, [12] * 5
    pk = lexlsi.pack_batch(n, [degenerate(20260500 + i, n, dims) for i in range(args.batch)])
    par = dict(tol_wrong_sign_lambda=0.0, cycling_handling_enabled=1, cycling_max_counter=args.max_counter, cycling_relax_step=args.relax_step)
    srv = lexlsi.LsiBatch(n, pk.dims, pk.types, args.batch)
    for _ in range(args.warmup):
        r = srv.run(pk, **par)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        r = srv.run(pk, **par)
    dt = (time.perf_counter() - t0) / args.reps
    counters = srv.cycling_counters() if hasattr(srv, "cycling_counters") else None
    status = np.array([i["status"] for i in r["info"]])
    f = np.array([i["factorizations"] for i in r["info"]], np.float64)
    out = dict(batch=args.batch, ms_per_batch=1e3 * dt, kernel=srv.last_kernel(), mean_factorizations=float(f.mean()), max_factorizations=float(f.max()),
               solved=int((status == 0).sum()), stopped_by_the_handler=int((status == 1).sum()), factorization_limit=int((status == 2).sum()),
               relaxations=None if counters is None else int(counters.sum()), instances_that_relax=None if counters is None else int((counters > 0).sum()),
               stages=srv.stats())
    srv.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
