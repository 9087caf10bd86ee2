"""x-only solves of 4096 problems (n = 40) with ragged levels: the ragged tolerance-contract kernel (kernel policy 10) against
  (a) the bit-exact four-per-wavefront kernel on the same batch (policy 4: what serves these batches otherwise), and
  (b) the shipped uniform tolerance-contract kernel (policy 6) on the same problems zero-padded on the host to 12 (or 8) rows per level
      (padding outside the timed region): the price of masking, per-lane offsets and 8-byte aligned segments.
The three solvers alternate; every run is `--inner` back-to-back solves ended by a synchronise; medians and min .. max over `--runs` runs.
usage: python scripts/time_ragged.py [6x5 | mixed | random | d0,d1,...] [--runs 8] [--inner 200] [--batch 4096]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import lexls_amd as hip  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

N = 40
NAMED = {"6x5": [6] * 5, "mixed": [5, 12, 7, 12, 9]}


def make_batch(name, batch):
    """(lod, dims (batch, nObj), capacities): `random` is the per-problem batch of tests/test_gpu_qtol_ragged.py's full-size case"""
    if name == "random":
        dims = np.minimum((P.uniform(18000, batch * 5) * 13).astype(np.uint32), 12).reshape(batch, 5)
        lod = np.zeros((batch, N + 1, 60))
        for b in range(batch):
            m = int(dims[b].sum())
            lod[b, :, :m] = P.lse_problem(20260100 + b, N, dims[b])
        return lod, dims, [12] * 5
    d = NAMED[name] if name in NAMED else [int(v) for v in name.split(",")]
    return P.lse_batch_fast(77, batch, N, d), np.tile(np.array(d, np.uint32), (batch, 1)), d


def zero_padded(lod, dims, md):
    out = np.zeros((lod.shape[0], N + 1, md * dims.shape[1]))
    for b in range(lod.shape[0]):
        f = 0
        for k, d in enumerate(dims[b]):
            out[b, :, k * md:k * md + d] = lod[b, :, f:f + d]
            f += int(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch_name", nargs="?", default="mixed")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    lod, dims, caps = make_batch(args.batch_name, args.batch)
    md = 8 if int(dims.max()) <= 8 else 12
    solvers = []
    for label, policy, data, d, c in (("ragged (policy 10)", 10, lod, dims, caps), ("bit-exact (policy 4)", 4, lod, dims, caps),
                                      ("uniform, host-padded (policy 6)", 6, zero_padded(lod, dims, md), None, [md] * dims.shape[1])):
        s = hip.BatchedLexLSE(args.batch, N, c)
        s.set_kernel_policy(policy)
        if d is not None:
            s.setObjDim(d)
        s.setProblem(data)
        for _ in range(10):
            s.factorize_solve(False)
        s.synchronize()
        solvers.append((label, s, []))
    x_rag, x_exact, x_pad = (s.get_x() for _, s, _ in solvers)
    for _ in range(args.runs):
        for _, s, times in solvers:
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                s.factorize_solve(False)
            s.synchronize()
            times.append((time.perf_counter() - t0) / args.inner * 1e6)
    out = {"batch_name": args.batch_name, "batch": args.batch, "n": N, "runs": args.runs, "inner": args.inner,
           "max_abs_x_difference_ragged_vs_bit_exact": float(np.abs(x_rag - x_exact).max()),
           "ragged_x_equals_padded_x": bool(np.array_equal(x_rag, x_pad))}
    for label, s, times in solvers:
        t = np.sort(np.array(times))
        print(f"{args.batch_name:8s} {label:34s} {s.last_kernel():34s} median {np.median(t):7.1f} us  min {t[0]:7.1f}  max {t[-1]:7.1f}  per {args.batch}")
        out[label] = {"kernel": s.last_kernel(), "median_us": float(np.median(t)), "min_us": float(t[0]), "max_us": float(t[-1])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
