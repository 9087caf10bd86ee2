"""Time the forward-mode tangents of the LexLSE solve (lexls_lse_solve_tangent_device, "solve_tangent<64,...>": the chain level search ->
sensitivity of level k* -> tangent_rhs -> solve_adjoint(_multi) -> apply_solve_map_multi) on the kept factor of a batch of IK problems (n = 40,
5 x 12) for K = 1, 8, 40, 64, 65 directions per problem, and, in the same process on the same factor, K single-direction calls and
lexls_lse_solve_adjoint_matrix_device — nVar calls of which on unit cotangents are what the library offered for the same quantity before.
Device events around `--calls` back-to-back calls (fewer for large K) in the handle's stream, `--runs` alternated runs of each after a warm-up;
prints one JSON line with the middle values and the spreads.  The floor of a call: K x batch x 41 x 60 x 8 bytes of directions read once.

    python scripts/bench_lse_tangent.py [--batch 4096] [--calls 100] [--runs 3] [--ks 1,8,40,64,65]

Per-kernel times of the chain: the same script, in a run of its own, under the profiler's kernel trace —
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_lse_tangent.py --calls 20 --runs 1 --ks 40
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lexls_amd  # noqa: E402
from lexls_amd import capi, problems as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ks", type=str, default="1,8,40,64,65")
    ap.add_argument("--policy", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lse_tangent: no GPU (there is nothing to time without one)")
    ks = [int(k) for k in a.ks.split(",")]
    n, dims = 40, [12] * 5
    s = lexls_amd.BatchedLexLSE(a.batch, n, dims)
    s.set_kernel_policy(a.policy)
    s.setProblem(P.lse_batch_fast(20290301, a.batch, n, dims))
    s.factorize_solve(keep_factor=True)
    producer = s.last_kernel()
    gen = torch.Generator(device="cuda").manual_seed(20330401)
    dlod = torch.randn((max(ks), a.batch, n + 1, s.cap), dtype=torch.float64, device="cuda", generator=gen)
    dx = torch.zeros((max(ks), a.batch, n), dtype=torch.float64, device="cuda")
    flags = torch.zeros((a.batch,), dtype=torch.uint8, device="cuda")
    g = torch.randn((a.batch, n), dtype=torch.float64, device="cuda", generator=gen)
    grad_lod = torch.zeros((a.batch, n + 1, s.cap), dtype=torch.float64, device="cuda")
    lib = capi.lib()
    slab, row = dlod[0].numel() * 8, dx[0].numel() * 8

    def tangent(K):
        capi.check(lib.lexls_lse_solve_tangent_device(s._h, C.c_void_p(dlod.data_ptr()), None, K, C.c_void_p(dx.data_ptr()), C.c_void_p(flags.data_ptr())))

    def singles(K):
        for c in range(K):
            capi.check(lib.lexls_lse_solve_tangent_device(s._h, C.c_void_p(dlod.data_ptr() + c * slab), None, 1, C.c_void_p(dx.data_ptr() + c * row),
                                                          C.c_void_p(flags.data_ptr())))

    def matrix(_K):
        capi.check(lib.lexls_lse_solve_adjoint_matrix_device(s._h, C.c_void_p(g.data_ptr()), C.c_void_p(grad_lod.data_ptr()), C.c_void_p(flags.data_ptr())))

    def timed(fn, K, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn(K)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / calls  # microseconds per call

    torch.cuda.synchronize()
    rows, kernel = [], None
    for K in ks:
        calls = max(3, a.calls // K)
        for fn in (tangent, singles, matrix):  # warm-up: code objects loaded, work buffers made, clocks up
            for _ in range(3):
                fn(K)
        tangent(K)
        kernel = s.last_consumer_kernel()
        torch.cuda.synchronize()
        t = dict(tangent=[], singles=[], matrix=[])
        for _ in range(a.runs):
            t["tangent"].append(timed(tangent, K, calls))
            t["singles"].append(timed(singles, K, max(1, calls // 4)))
            t["matrix"].append(timed(matrix, K, a.calls))
        mid = {k: float(np.median(v)) for k, v in t.items()}
        floor_us = K * slab / 8e12 * 1e6  # the directions read once, at 8 TB/s
        rows.append(dict(K=K, calls=calls, tangent_us=mid["tangent"], singles_us=mid["singles"], matrix_adjoint_us=mid["matrix"],
                         nvar_matrix_adjoints_us=n * mid["matrix"], spread={k: (max(v) - min(v)) / mid[k] for k, v in t.items()}, us_runs=t,
                         floor_us=floor_us, tangent_over_floor=mid["tangent"] / floor_us, read_GBps=K * slab / mid["tangent"] * 1e-3))
    print(json.dumps(dict(bench="lse_tangent", batch=a.batch, n=n, dims=dims, producer=producer, kernel=kernel, runs=a.runs,
                          rank_stable=int(flags.sum().item()), results=rows)))
    s.close()


if __name__ == "__main__":
    main()
