"""Timing of the accuracy guard (lexls_lse_set_accuracy_guard): x-only solves of 4096 IK problems (n = 40, levels [12] x 5) under mode 0 (the
unguarded lqr_qtol), mode 1 (estimate + status), mode 2 (+ the bit-exact re-solve of the flagged problems) and policy 4 (the bit-exact
four-per-wavefront kernel for everything), on the configs[2] distribution and on a near-dependent batch (delta = 1e-5: the guard flags them
all).  Wall time per solve over 200 back-to-back solves (four handles in rotation), best of five.
usage: python scripts/time_guard.py [batch]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lexls_amd as hip
from lexls_amd import problems as P

N, DIMS = 40, [12] * 5


def time_us(lods, mode, policy):
    ss = []
    for lod in lods:
        s = hip.BatchedLexLSE(lod.shape[0], N, DIMS)
        s.set_kernel_policy(policy)
        if mode:
            s.set_accuracy_guard(mode)
        s.setProblem(lod)
        s.factorize_solve(keep_factor=False)
        ss.append(s)
    flagged = ss[0].get_accuracy()[2]
    best = 1e9
    for _ in range(5):
        for s in ss:
            s.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            for s in ss:
                s.factorize_solve(keep_factor=False)
        for s in ss:
            s.synchronize()
        best = min(best, (time.perf_counter() - t0) / (50 * len(ss)))
    kernel = ss[0].last_kernel()
    for s in ss:
        s.close()
    return best * 1e6, kernel, flagged


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    sets = {"configs[2]": [P.lse_batch_fast(20260100 + 7 * i, batch, N, DIMS) for i in range(4)],
            "near-dependent 1e-5": [P.near_dependent_batch(20261200 + 7 * i, batch, N, DIMS, 1e-5) for i in range(4)]}
    out = {}
    for name, lods in sets.items():
        row = {}
        for label, mode, policy in (("mode 0", 0, 0), ("mode 1", 1, 0), ("mode 2", 2, 0), ("policy 4", 0, 4)):
            us, kernel, flagged = time_us(lods, mode, policy)
            row[label] = dict(us=round(us, 2), kernel=kernel, flagged=flagged)
            print(f"{name:20s} {label:9s} {us:8.2f} us per {batch}  kernel {kernel}  flagged {flagged}", flush=True)
        row["mode 2 / mode 0"] = round(row["mode 2"]["us"] / row["mode 0"]["us"], 3)
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
