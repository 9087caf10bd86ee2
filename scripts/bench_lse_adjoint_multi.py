"""Time the multi-cotangent adjoint of the LexLSE solve (lexls_lse_solve_adjoint_multi_device, solve_adjoint_multi<64,...>: lane = cotangent)
on the kept factor of a batch of IK problems (n = 40, 5 x 12), in one process on one factor:
    (i)   K successive lexls_lse_solve_adjoint_device calls (solve_adjoint<64>), the yardstick, K = 40
    (ii)  lexls_lse_solve_adjoint_multi_device at K = 1, 8, 40, 64
    (iii) the staged form against the hbm form at K = 40 (LEXLS_ADJOINT_MULTI_FORM, read by the launcher at every call)
    (iv)  LsiBatch: 1024 warm-started IK instances, solve_adjoint_multi_device at K = 40 against 40 solve_adjoint_device calls on the same run
Device events around `--calls` back-to-back launches in the handle's stream for (i)-(iii), host wall clock around the host-synchronous calls
of (iv); `--runs` alternated runs of each after a warm-up; one JSON line with the middle values and the spreads ((max - min) / middle).

    python scripts/bench_lse_adjoint_multi.py [--batch 4096] [--calls 200] [--runs 5] [--lsi-batch 1024]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lexls_amd  # noqa: E402
from lexls_amd import capi, lexlsi, problems as P  # noqa: E402

SWITCH = "LEXLS_ADJOINT_MULTI_FORM"


def stats(v):
    mid = float(np.median(v))
    return dict(mid=mid, spread=(max(v) - min(v)) / mid, runs=[round(x, 3) for x in v])


def lse_part(a):
    n, dims, B = 40, [12] * 5, a.batch
    s = lexls_amd.BatchedLexLSE(B, n, dims)
    s.setProblem(P.lse_batch_fast(20290301, B, n, dims))
    s.factorize_solve(keep_factor=True)
    producer, lib, ptr = s.last_kernel(), capi.lib(), lambda t: C.c_void_p(t.data_ptr())
    KS = (1, 8, 40, 64)
    G = {K: torch.from_numpy(P.normal(20290400 + K, B * K * n).reshape(B, K, n)).cuda() for K in KS}
    R = {K: torch.zeros((B, K, s.cap), dtype=torch.float64, device="cuda") for K in KS}
    F = {K: torch.zeros((B, K, n), dtype=torch.float64, device="cuda") for K in KS}
    g1 = [G[40][:, c].contiguous() for c in range(40)]
    r1, f1 = torch.zeros((B, s.cap), dtype=torch.float64, device="cuda"), torch.zeros((B, n), dtype=torch.float64, device="cuda")

    def singles():  # (i)
        for c in range(40):
            capi.check(lib.lexls_lse_solve_adjoint_device(s._h, ptr(g1[c]), ptr(r1), ptr(f1)))

    def multi(K, form=None):
        def fn():
            capi.check(lib.lexls_lse_solve_adjoint_multi_device(s._h, ptr(G[K]), K, ptr(R[K]), ptr(F[K])))

        def forced():
            os.environ[SWITCH] = form
            try:
                fn()
            finally:
                del os.environ[SWITCH]
        return forced if form else fn

    def timed(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / calls  # microseconds per call

    what = {"singles_x40": (singles, max(1, a.calls // 40))}
    what.update({f"multi_K{K}": (multi(K), a.calls) for K in KS})
    what.update({"multi_K40_staged": (multi(40, "staged"), a.calls), "multi_K40_hbm": (multi(40, "hbm"), a.calls)})
    names = {}
    for k, (fn, _) in what.items():  # warm-up: code objects loaded, clocks up
        for _ in range(5):
            fn()
        names[k] = s.last_consumer_kernel()
    torch.cuda.synchronize()
    t = {k: [] for k in what}
    for r in range(a.runs):
        for k in (list(what) if r % 2 == 0 else list(what)[::-1]):  # alternated
            t[k].append(timed(*what[k]))
    s.close()
    return dict(batch=B, n=n, dims=dims, producer=producer, kernels=names, us={k: stats(v) for k, v in t.items()})


def lsi_part(a):
    n, dims, B, K = 40, (12, 12, 12, 12, 12), a.lsi_batch, 40
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims) for i in range(B)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260000 + i, n, dims, perturb=0.9) for i in range(B)])
    b = lexlsi.LsiBatch(n, base.dims, base.types, B)
    up = lambda x, t: torch.from_numpy(np.ascontiguousarray(x, t)).cuda()  # noqa: E731
    var = up(base.var_index.view(np.int32), np.int32)
    cold = b.run_device(up(base.data, np.float64), var_index=var)
    guess = torch.where(cold["active"] == 3, torch.zeros_like(cold["active"]), cold["active"]).contiguous()
    r = b.run_device(up(pert.data, np.float64), var_index=var, active_guess=guess, x0=cold["x"].clone())
    solved = int((r["info"][:, 0] == 0).sum())
    G = up(P.normal(20300911, B * K * n).reshape(B, K, n), np.float64)
    g1 = [G[:, c].contiguous() for c in range(K)]
    out1 = [torch.zeros((B, b.total), dtype=torch.float64, device="cuda") for _ in range(2)]
    outK = [torch.zeros((B, K, b.total), dtype=torch.float64, device="cuda") for _ in range(2)]

    def singles():
        for c in range(K):
            b.solve_adjoint_device(g1[c], *out1)

    def multi():
        b.solve_adjoint_multi_device(G, *outK)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(3):  # warm-up: the final factor is kept from here on, buffers made
        singles(), multi()
    t = dict(singles_x40=[], multi_K40=[])
    for i in range(a.runs):
        for k in (("singles_x40", "multi_K40") if i % 2 == 0 else ("multi_K40", "singles_x40")):
            t[k].append(clock(singles if k == "singles_x40" else multi))
    b.close()
    return dict(batch=B, solved=solved, ms={k: stats(v) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--lsi-batch", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lse_adjoint_multi: no GPU (there is nothing to time without one)")
    print(json.dumps(dict(bench="lse_adjoint_multi", calls=a.calls, runs=a.runs, lse=lse_part(a), lsi=lsi_part(a) if a.lsi_batch else None)))


if __name__ == "__main__":
    main()
