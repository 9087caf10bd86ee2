"""Calibration of the accuracy guard's default threshold (lexls_lse_set_accuracy_guard): CPU only, with the oracle.

For every problem of the test sets (n = 40, levels [12] x 5) this computes
  * the one-ulp sensitivity (as in scripts/soak_qtol.py): the maximum, over three random one-ulp relative perturbations of the data, of
    max|dx| / max(1, |x|_inf) — a property of the problem, measured with the oracle, independent of any kernel;
  * the guard's estimate from the oracle's factor: the maximum over pivots of (norm of the pivot column in its level's RAW rows, before the
    elimination by the levels above) / |R_jj| — what lqr_qtol's guarded instantiations compute in-kernel from their own factorization.
and prints, per set, how many problems are sensitive (> 1e-11, > 1e-10), the smallest estimate among the sensitive ones, the largest
among the rest, and how many of each side a threshold leaves on the wrong side.
usage: python scripts/calibrate_guard.py [threshold]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from lexls_amd import problems as P
from oracle import oracle_ctypes as oracle

N, DIMS = 40, [12] * 5
DEFAULT_THRESHOLD = 64.0  # = kGuardDefaultThreshold in lexls_amd/csrc/lexls_capi.hip


def guard_sets():
    """(name, lod) of the calibration / test sets (the same seeds as tests/test_gpu_accuracy_guard.py)"""
    return [("configs[2]", P.lse_batch(20260100, 1024, N, DIMS)),
            ("badly scaled", P.badly_scaled_batch(20261101, 1024, N, DIMS)),
            ("near-dependent 1e-4", P.near_dependent_batch(20261102, 512, N, DIMS, 1e-4)),
            ("near-dependent 1e-5", P.near_dependent_batch(20261103, 512, N, DIMS, 1e-5)),
            ("near-dependent 3e-6", P.near_dependent_batch(20261104, 512, N, DIMS, 3e-6))]


def sensitivity(lod, dims, n, ref, seed=0):
    """one-ulp sensitivity of every problem of the batch (oracle only)"""
    xs = np.maximum(1.0, np.abs(ref["x"]).max(axis=1))
    sens = np.zeros(lod.shape[0])
    for rep in range(3):
        pert = lod * (1.0 + 1.1e-16 * np.sign(np.random.default_rng(1000 * seed + rep).standard_normal(lod.shape)))
        rp = oracle.lse_run(pert, dims, n, nthreads=8)
        sens = np.maximum(sens, np.abs(rp["x"] - ref["x"]).max(axis=1) / xs)
    return sens


def estimate(lod, dims, n, ref):
    """the guard's estimate from the oracle's factor (columns of the factor in final position order, diagonal = R_jj)"""
    B = lod.shape[0]
    est = np.zeros(B)
    for b in range(B):
        phys = np.arange(n)
        for c in range(int(ref["totalrank"][b])):
            q = int(ref["perm"][b, c])
            phys[c], phys[q] = phys[q], phys[c]
        row = 0
        for k, d in enumerate(dims):
            fc, r = int(ref["fcol"][b, k]), int(ref["rank"][b, k])
            for j in range(r):
                c = fc + j
                raw = np.linalg.norm(lod[b, phys[c], row:row + d])
                est[b] = max(est[b], raw / abs(ref["factor"][b, c, row + j]))
            row += d
    return est


def main():
    thr = float(sys.argv[1]) if len(sys.argv) > 1 else DEFAULT_THRESHOLD
    print(f"threshold {thr:.3g}")
    for i, (name, lod) in enumerate(guard_sets()):
        ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
        sens = sensitivity(lod, DIMS, N, ref, seed=i)
        est = estimate(lod, DIMS, N, ref)
        s11, s10 = sens > 1e-11, sens > 1e-10
        lo = est[s11].min() if s11.any() else float("nan")
        hi = est[~s11].max() if (~s11).any() else float("nan")
        print(f"{name:22s} {lod.shape[0]:5d} problems  sensitivity > 1e-11: {int(s11.sum()):4d}  > 1e-10: {int(s10.sum()):4d}  "
              f"max sensitivity {sens.max():.2e}  estimate: min over sensitive {lo:.3g}, max over the rest {hi:.3g}, max {est.max():.3g}  "
              f"missed (sensitive, below threshold) {int((s11 & (est < thr)).sum())}  flagged {int((est >= thr).sum())} "
              f"of which benign {int((~s11 & (est >= thr)).sum())}")


if __name__ == "__main__":
    main()
