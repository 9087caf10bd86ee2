"""Time the configs[4] batch (the inputs of `bench.py --workload lsi`: 1024 warm-started instances of n = 40, 5 x 12, objective 0 simple
bounds) under ParametersLexLSI::deactivate_first_wrong_sign, next to the same batch under the default removal rule.

    python scripts/bench_lsi_first_wrong_sign.py [--batch 1024] [--reps 5] [--warmup 2]

Prints one JSON line: milliseconds per run and the kernel that served the resident iterations for both rules, with the iteration and
factorization counts of each (the two rules take different trajectories).  Uses the public Python binding only, so the same file times
any commit of the library (a commit without resident flag runs reports kernel "host" and seconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import lexlsi, problems as P  # noqa: E402


def timed(srv, pert, guess, x0, warmup, reps, **params):
    for _ in range(warmup):
        r = srv.run(pert, active_guess=guess, x0=x0, **params)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = srv.run(pert, active_guess=guess, x0=x0, **params)
    dt = (time.perf_counter() - t0) / reps
    it = np.array([i["iterations"] for i in r["info"]], np.float64)
    f = np.array([i["factorizations"] for i in r["info"]], np.float64)
    return r, dict(ms_per_batch=1e3 * dt, kernel=srv.last_kernel(), mean_iterations=float(it.mean()), max_iterations=float(it.max()),
                   mean_factorizations=float(f.mean()), deactivations=int(sum(i["deactivations"] for i in r["info"])),
                   solved=int(sum(i["status"] == 0 for i in r["info"])), stages=srv.stats())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flag-reps", type=int, default=0, help="repetitions of the flag run (default: --reps)")
    args = ap.parse_args()
    n, dims, total = 40, [12] * 5, args.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + i, n, dims) for i in range(total)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + i, n, dims, perturb=0.9) for i in range(total)])
    srv = lexlsi.LsiBatch(n, base.dims, base.types, total)
    cold = srv.run(base)
    guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
    rp, plain = timed(srv, pert, guess, cold["x"], args.warmup, args.reps)
    rf, flag = timed(srv, pert, guess, cold["x"], min(args.warmup, 1), args.flag_reps or args.reps, deactivate_first_wrong_sign=1)
    srv.close()
    differ = int(sum(a != b for a, b in zip(rp["info"], rf["info"])))
    print(json.dumps(dict(batch=total, default_rule=plain, first_wrong_sign=flag, instances_whose_counters_differ=differ)), flush=True)


if __name__ == "__main__":
    main()
