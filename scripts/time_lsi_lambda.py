"""Cost of the multipliers of a lock-step LexLSI batch (lexls_lsi_batch_get_lambda) on BASELINE configs[4]: 1024 instances, n = 40, 5 x 12
with simple bounds, warm-started as `bench.py --workload lsi`.  Prints
  - lexls_lsi_batch_run alone against run + get_lambda (medians over the repeats),
  - get_lambda by stage (LEXLS_LSI_TIMING=1 lines of the library: forming the problems on the host, upload + gather + factorization,
    multipliers, scatter + copy back),
  - lexls_lse_multipliers (all objectives in one launch) against nObj launches of the per-objective kernels on the same factors.
Usage: python scripts/time_lsi_lambda.py [--batch 1024] [--repeats 20]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(f, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t)


def lsi_part(args):
    from lexls_amd import capi, lexlsi, problems as P
    n, dims, total = 40, (12, 12, 12, 12, 12), args.batch
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + i, n, dims) for i in range(total)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + i, n, dims, perturb=0.9) for i in range(total)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, total)
    cold = b.run(base)
    guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
    lam = np.zeros((total, len(dims), base.total))

    def get_lambda():
        capi.check(capi.lib().lexls_lsi_batch_get_lambda(b._h, lam.ctypes.data_as(C.POINTER(C.c_double))))

    def run():
        return b.run(pert, active_guess=guess, x0=cold["x"])

    for _ in range(3):
        run()
        get_lambda()
    run_only = median_ms(run, args.repeats)
    run_lam = median_ms(lambda: (run(), get_lambda()), args.repeats)
    get_only = median_ms(get_lambda, args.repeats)
    nf = sum(r["factorizations"] for r in run()["info"])
    b.close()
    return dict(batch=total, factorizations=nf, run_ms=run_only, run_plus_get_lambda_ms=run_lam, get_lambda_ms=get_only,
                get_lambda_share_of_run=get_only / run_only)


def lse_part(args):
    """lexls_lse_multipliers against nObj per-objective launches on the same factors: equality problems of the batch's shape
    (4 levels of 12 rows, 12 fixed variables)"""
    from lexls_amd import capi, lexlse, problems as P
    B, n, cap_dims = args.batch, 40, np.array([12, 12, 12, 12], np.uint32)
    lse = lexlse.BatchedLexLSE(B, n, cap_dims)
    lse.setProblem(P.lse_batch_fast(777, B, n, [int(d) for d in cap_dims]))
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.uint32)
    lse.fixVariables(np.full(B, 12, np.uint32), idx, rng.standard_normal((B, n)), np.full((B, n), 2, np.uint8))
    lse.factorize()
    lib, h, nobj, reps = capi.lib(), lse._h, len(cap_dims), 50

    def loop(f):
        f()
        lse.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        lse.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    def per_objective():
        for k in range(nobj):
            capi.check(lib.lexls_lse_sensitivity(h, None, C.c_int32(k), C.c_double(1e-8), C.c_double(1e-12)))

    one_launch = loop(lambda: capi.check(lib.lexls_lse_multipliers(h)))
    sweep_each = loop(per_objective)  # the removal-search sweep kernel, one objective per launch
    os.environ["LEXLS_SENS_NO_SWEEP"] = "1"  # (read at every call)
    kernel_each = loop(per_objective)  # sensitivity_kernel, one objective per launch
    fallback = loop(lambda: capi.check(lib.lexls_lse_multipliers(h)))  # the multipliers call's own fallback: those launches + column copies
    del os.environ["LEXLS_SENS_NO_SWEEP"]
    lse.close()
    return dict(batch=B, nObj=nobj, multipliers_one_launch_ms=one_launch, sensitivity_kernel_x_nObj_ms=kernel_each,
                sweep_kernel_x_nObj_ms=sweep_each, multipliers_fallback_ms=fallback, speedup_vs_sensitivity_kernel=kernel_each / one_launch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--part", choices=["all", "lsi", "lse"], default="all")
    args = ap.parse_args()
    out = {}
    if args.part in ("all", "lsi"):
        out["lsi"] = lsi_part(args)
    if args.part in ("all", "lse"):
        out["lse"] = lse_part(args)
    print(json.dumps(out), flush=True)
    if args.part == "all":
        # get_lambda by stage: the library's LEXLS_LSI_TIMING lines, in a child process of its own (a run prints its own lines too)
        env = dict(os.environ, LEXLS_LSI_TIMING="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "lsi", "--batch", str(args.batch), "--repeats", "3"], env=env, check=True)


if __name__ == "__main__":
    main()
