"""Time the many-cotangent adjoint of the regularized LexLSE solve (solve_adjoint_reg_multi) on 4096 IK problems (n = 40, 5 x 12) under TIKHONOV
damping (type 1), the factor kept, for K = 1, 2, 4, 8, 16, 40, 64, 65 cotangents per problem — in both placements (the shape's own, lds, and hbm
forced through LEXLS_ADJOINT_REG_MULTI_FORM, which the launcher reads at every call) — against the yardstick: K calls of
lexls_lse_solve_adjoint_device (solve_adjoint_reg, the single-cotangent kernel) on the same factor in the same process.  Beside them the
undamped multi call (solve_adjoint_multi) at K = 40 on the unregularized factor of the same problems.  Device forms only (no host copies); the
candidates are measured in alternated rounds (a round = REPS enqueued repetitions of each between two synchronisations); medians and spreads
(min .. max) over the rounds are printed, then the crossover K and one JSON line.

    python scripts/bench_lse_adjoint_reg_multi.py [--batch 4096] [--rounds 9] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch  # (before the HIP library loads: one process, one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import capi, problems as P  # noqa: E402
from lexls_amd.lexlse import BatchedLexLSE  # noqa: E402

KS = (1, 2, 4, 8, 16, 40, 64, 65)
SWITCH = "LEXLS_ADJOINT_REG_MULTI_FORM"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n, dims, B = 40, [12] * 5, a.batch
    lod = P.lse_batch(20290107, B, n, dims)
    plain, damped = BatchedLexLSE(B, n, dims), BatchedLexLSE(B, n, dims)
    for s in (plain, damped):
        s.setProblem(lod)
    damped.setRegularization(1, [0.1] * len(dims))
    damped.set_adjoint_regularized(True)
    damped.set_adjoint_regularized_multi(True)
    plain.factorize_solve(keep_factor=True)
    damped.factorize_solve(keep_factor=True)
    cap, kmax = damped.cap, max(KS)
    G = torch.from_numpy(P.normal(20290109, B * kmax * n).reshape(B, kmax, n)).cuda()
    Gk = {K: G[:, :K].contiguous() for K in KS}
    rhs = {K: torch.empty((B, K, cap), dtype=torch.float64, device="cuda") for K in KS}
    fixed = {K: torch.empty((B, K, n), dtype=torch.float64, device="cuda") for K in KS}
    g1, rhs1, fixed1 = Gk[1][:, 0].contiguous(), torch.empty((B, cap), dtype=torch.float64, device="cuda"), torch.empty((B, n), dtype=torch.float64, device="cuda")

    def multi(K, form):
        def run():
            if form:
                os.environ[SWITCH] = form
            else:
                os.environ.pop(SWITCH, None)
            # (through the C entry for K = 1 too: the Python method would send one cotangent to the single-cotangent kernel when that switch is on)
            capi.check(capi.lib().lexls_lse_solve_adjoint_multi_device(damped._h, C.c_void_p(Gk[K].data_ptr()), K, C.c_void_p(rhs[K].data_ptr()), C.c_void_p(fixed[K].data_ptr())))
        return run

    def singles(K):
        def run():
            for _ in range(K):
                damped.solve_adjoint_device(g1, rhs1, fixed1)
        return run

    def timed(fn, sync):
        sync.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        sync.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    runs, names = {}, {}
    for K in KS:
        runs[f"multi lds K={K}"] = (multi(K, None), damped)
        runs[f"multi hbm K={K}"] = (multi(K, "hbm"), damped)
        runs[f"single x K={K}"] = (singles(K), damped)
    runs["undamped multi K=40"] = (lambda: plain.solve_adjoint_multi_device(Gk[40], rhs[40], fixed[40]), plain)
    for k, (fn, s) in runs.items():  # warm-up (and the work buffers' allocation), and what each candidate launches
        timed(fn, s)
        names[k] = s.last_consumer_kernel()
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (fn, s) in runs.items():
            us[k].append(timed(fn, s))
    os.environ.pop(SWITCH, None)
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        print(f"{k:<22} {names[k]:<34} median {med[k]:10.1f} us  ({min(v):.1f} .. {max(v):.1f}) per {B} problems")
    # the smallest K of the list from which on the multi call (the shape's own placement) is faster than K single calls
    faster = [K for K in KS if med[f"multi lds K={K}"] < med[f"single x K={K}"]]
    crossover = next((K for K in KS if all(k2 in faster for k2 in KS if k2 >= K)), None)
    print(f"multi (lds) faster than K single calls from K = {crossover} on (of {list(KS)}); hbm / lds at K = 40: {med['multi hbm K=40'] / med['multi lds K=40']:.2f}")
    res = dict(batch=B, rounds=a.rounds, reps=a.reps, producer=damped.last_kernel(), variants=names,
               us={k: dict(median=med[k], min=min(v), max=max(v)) for k, v in us.items()}, crossover_K=crossover,
               speedup_at_40=med["single x K=40"] / med["multi lds K=40"], hbm_over_lds_at_40=med["multi hbm K=40"] / med["multi lds K=40"],
               damped_over_undamped_multi_at_40=med["multi lds K=40"] / med["undamped multi K=40"])
    print(json.dumps(res))
    plain.close()
    damped.close()


if __name__ == "__main__":
    main()
