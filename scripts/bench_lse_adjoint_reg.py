"""Time the adjoint of the regularized LexLSE solve (solve_adjoint_reg) on 4096 IK problems (n = 40, 5 x 12) under TIKHONOV damping (type 1), the
factor kept, against two yardsticks on the same device in the same process: solve_adjoint<64> on the unregularized factor of the same problems,
and the regularized factorization itself.  The three are measured in alternated rounds (a round = REPS enqueued calls of each between two
synchronisations, device form: no host copies); medians and spreads (min .. max) over the rounds are printed, and one JSON line.

    python scripts/bench_lse_adjoint_reg.py [--batch 4096] [--rounds 15] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the HIP library loads: one process, one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import problems as P  # noqa: E402
from lexls_amd.lexlse import BatchedLexLSE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n, dims, B = 40, [12] * 5, a.batch
    lod = P.lse_batch(20290107, B, n, dims)
    g = torch.from_numpy(P.normal(20290108, B * n).reshape(B, n)).cuda()
    plain, damped = BatchedLexLSE(B, n, dims), BatchedLexLSE(B, n, dims)
    for s in (plain, damped):
        s.setProblem(lod)
    damped.setRegularization(1, [0.1] * len(dims))
    damped.set_adjoint_regularized(True)
    plain.factorize_solve(keep_factor=True)
    damped.factorize_solve(keep_factor=True)
    out = {s: (torch.empty((B, s.cap), dtype=torch.float64, device="cuda"), torch.empty((B, n), dtype=torch.float64, device="cuda")) for s in (plain, damped)}

    def timed(fn, sync):
        sync.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        sync.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    runs = {
        "solve_adjoint<64> (unregularized factor)": (lambda: plain.solve_adjoint_device(g, *out[plain]), plain),
        "solve_adjoint_reg (type 1 factor)": (lambda: damped.solve_adjoint_device(g, *out[damped]), damped),
        "regularized factorization (type 1)": (lambda: damped.factorize_solve(keep_factor=True), damped),
        "unregularized factorization": (lambda: plain.factorize_solve(keep_factor=True), plain),
    }
    for fn, s in runs.values():  # warm-up
        timed(fn, s)
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (fn, s) in runs.items():
            us[k].append(timed(fn, s))
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        print(f"{k:<44} median {med[k]:9.1f} us  ({min(v):.1f} .. {max(v):.1f}) per {B} problems")
    keys = list(runs)
    runs[keys[1]][0]()  # (the last call on the damped handle: its variant is what last_consumer_kernel names)
    damped.synchronize()
    res = dict(batch=B, rounds=a.rounds, reps=a.reps, variant=damped.last_consumer_kernel(), producer=damped.last_kernel(),
               us={k: dict(median=med[k], min=min(v), max=max(v)) for k, v in us.items()},
               adjoint_reg_over_adjoint=med[keys[1]] / med[keys[0]], adjoint_reg_over_reg_factorization=med[keys[1]] / med[keys[2]],
               reg_over_plain_factorization=med[keys[2]] / med[keys[3]])
    print(json.dumps(res))
    plain.close()
    damped.close()


if __name__ == "__main__":
    main()
