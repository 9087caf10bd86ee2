#!/usr/bin/env python3
"""The configs[4] batch (1024 lock-step LexLSI instances, n = 40, 5 x 12, level 0 simple bounds, warm-started from the 0.9-perturbed neighbour:
the batch scripts/bench_lsi.py calls warm_30) three ways on ONE batch object, alternating within one visit:
  (a) LsiBatch.run as it is (phase 1 on the host over LexLSI objects),
  (b) LsiBatch.run under LEXLS_LSI_DEVICE_PHASE1=1 (phase 1 as device work, inputs uploaded),
  (c) LsiBatch.run_device with the inputs already resident (results stay on the device; the call is host-synchronous).
Warm-up runs, then `runs` rounds of a, b, c; median and quartiles per variant.  One more run of (a) and (b) under LEXLS_LSI_TIMING gives the
driver's own split (its stderr lines are captured).  Prints one JSON line.
  python scripts/bench_lsi_device_entry.py [batch] [runs]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

batch = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "--timing-split" else 1024
runs = max(5, int(sys.argv[2])) if len(sys.argv) > 2 and sys.argv[1] != "--timing-split" else 25
n, dims = 40, [12] * 5


def setup():
    from lexls_amd import lexlsi, problems as P
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims) for b in range(batch)])
    pert = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims, perturb=0.9) for b in range(batch)])
    srv = lexlsi.LsiBatch(n, base.dims, base.types, batch)
    for _ in range(3):  # warm-up: library load, first launches, GPU clocks; the last result is the warm start's neighbour
        cold = srv.run(base)
    guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
    return srv, pert, guess, cold["x"]


def timing_split():
    """child process: one timed-split run of (a) and of (b); the driver writes the split to stderr"""
    batch_, = (int(sys.argv[2]),)
    globals()["batch"] = batch_
    srv, pert, guess, x0 = setup()
    for _ in range(2):
        srv.run(pert, active_guess=guess, x0=x0)
    os.environ["LEXLS_LSI_TIMING"] = "1"
    for phase1 in ("0", "1"):
        os.environ["LEXLS_LSI_DEVICE_PHASE1"] = phase1
        srv.run(pert, active_guess=guess, x0=x0)  # (the switch's first use: buffers are made)
        sys.stderr.write(f"--- LEXLS_LSI_DEVICE_PHASE1={phase1}\n")
        sys.stderr.flush()
        srv.run(pert, active_guess=guess, x0=x0)
    srv.close()


def main():
    import torch
    from lexls_amd import capi
    srv, pert, guess, x0 = setup()
    dev = torch.device("cuda", 0)
    d = dict(data=torch.from_numpy(pert.data).to(dev), var=torch.from_numpy(pert.var_index.view(np.int32)).to(dev), guess=torch.from_numpy(guess).to(dev), x0=torch.from_numpy(x0).to(dev))

    def a():
        os.environ.pop("LEXLS_LSI_DEVICE_PHASE1", None)
        return srv.run(pert, active_guess=guess, x0=x0)

    def b():
        os.environ["LEXLS_LSI_DEVICE_PHASE1"] = "1"
        try:
            return srv.run(pert, active_guess=guess, x0=x0)
        finally:
            os.environ.pop("LEXLS_LSI_DEVICE_PHASE1", None)

    def c():
        return srv.run_device(d["data"], d["var"], d["guess"], d["x0"])

    variants = dict(run=a, run_device_phase1=b, run_device=c)
    out, t = {}, {k: [] for k in variants}
    for _ in range(3):
        for f in variants.values():
            f()
    for _ in range(runs):
        for k, f in variants.items():
            t0 = time.perf_counter()
            r = f()
            t[k].append(time.perf_counter() - t0)
            out[k] = (r, srv.last_kernel(), srv.stats())
    ref = out["run"][0]
    res = dict(batch=batch, runs=runs, library=capi.LIB_PATH)
    for k, (r, kernel, stats) in out.items():
        info = r["info"].array if hasattr(r["info"], "array") else r["info"].cpu().numpy()
        x = r["x"] if isinstance(r["x"], np.ndarray) else r["x"].cpu().numpy()
        s = np.sort(np.array(t[k]))
        res[k] = dict(ms_per_batch=1e3 * float(np.median(s)), spread_ms=dict(min=1e3 * float(s[0]), q1=1e3 * float(np.percentile(s, 25)), q3=1e3 * float(np.percentile(s, 75)), max=1e3 * float(s[-1])),
                      last_kernel=kernel, stages=stats, factorizations=int(info[:, 4].sum()), max_factorizations=int(info[:, 4].max()), solved=int((info[:, 0] == 0).sum()),
                      same_bits_as_run=bool(np.array_equal(x.view(np.uint64), ref["x"].view(np.uint64))))
    srv.close()
    split = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-split", str(batch)], capture_output=True, text=True)
    lines, key = {"run": [], "run_device_phase1": []}, None
    for line in split.stderr.splitlines():
        if line.startswith("--- LEXLS_LSI_DEVICE_PHASE1="):
            key = "run" if line.endswith("=0") else "run_device_phase1"
        elif key and line.startswith("lexls_lsi_batch_solve:"):
            lines[key].append(line)
            if "total" in line:
                key = None
    res["timing_split"] = lines
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--timing-split":
        timing_split()
    else:
        main()
