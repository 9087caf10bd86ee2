#!/usr/bin/env python3
"""The closed loop lexls_lsi_batch_run_device_ex exists for, on the configs[4] batch (1024 lock-step LexLSI instances, n = 40, 5 x 12, level 0
simple bounds): solve, perturb the right-hand sides, solve again warm-started from active / x / v of the previous answer — two ways, alternating
step by step within one visit, each on its own batch object:
  (a) host arrays: LsiBatch.run(pert_k, active_guess=active, x0=x, v0=v) with the previous run's numpy results,
  (b) device: the bounds are moved by a torch kernel on the device copy of the data, LsiBatch.run_device(..., active_guess=active, x0=x, v0=v)
      with the previous run's device tensors fed straight back (nothing of the loop passes through host memory).
Both loops see the same data (the perturbation is drawn once, on the host, and applied to the numpy copy for (a) and, uploaded before the
timing starts, on the device for (b)); every step the two answers are compared bit for bit.  Warm-up steps, then `steps` timed steps; median
and quartiles of the ms per step of each loop.  Prints one JSON line.
  python scripts/bench_lsi_device_warm_loop.py [batch] [steps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 25
n, dims, warmup, sigma = 40, [12] * 5, 3, 0.05


def bound_columns(pk):
    """per instance the positions of the lb / ub entries of the general objectives in the flat data (PackedBatch.data) and, per position, the row it
    belongs to: moving lb and ub of a row by the same amount is P.lsi_problem's `perturb`"""
    pos, row, off, r = [], [], 0, 0
    for d, t in zip(pk.dims.tolist(), pk.types.tolist()):
        w = 2 if t == 1 else n + 2
        if t != 1:
            for c in (n, n + 1):
                pos.extend(range(off + c * d, off + (c + 1) * d))
                row.extend(range(r, r + d))
            r += d
        off += d * w
    return np.array(pos), np.array(row), r


def main():
    import torch
    from lexls_amd import capi, lexlsi, problems as P
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims) for b in range(batch)])
    pos, row, rows = bound_columns(base)
    rng = np.random.default_rng(20260500)
    shifts = sigma * rng.standard_normal((warmup + steps, batch, rows))  # per step, instance and general row: how far its interval moves
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(pos).to(dev)
    d_shifts = torch.from_numpy(np.ascontiguousarray(shifts[:, :, row])).to(dev)
    d_var = torch.from_numpy(base.var_index.view(np.int32)).to(dev)
    host_srv, dev_srv = (lexlsi.LsiBatch(n, base.dims, base.types, batch) for _ in range(2))
    h_data = base.data.copy()
    d_data = torch.from_numpy(h_data).to(dev)
    for _ in range(3):  # library load, first launches, GPU clocks
        h = host_srv.run(base)
        d = dev_srv.run_device(d_data, d_var)
    t_host, t_dev, same, fact = [], [], True, 0
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        h_data[:, pos] += shifts[k][:, row]
        h = host_srv.run(lexlsi.PackedBatch(n, base.dims, base.types, h_data, base.var_index), active_guess=h["active"], x0=h["x"], v0=h["v"])
        t1 = time.perf_counter()
        d_data[:, d_pos] += d_shifts[k]
        d = dev_srv.run_device(d_data, d_var, active_guess=d["active"], x0=d["x"], v0=d["v"])
        t2 = time.perf_counter()
        if k >= warmup:
            t_host.append(t1 - t0)
            t_dev.append(t2 - t1)
            fact += int(h["info"].array[:, 4].sum())
        same = same and all(np.array_equal(d[key].cpu().numpy().view(np.uint8), np.ascontiguousarray(h[key].array if key == "info" else h[key]).view(np.uint8)) for key in ("x", "info", "active", "v"))

    def summary(t):
        s = np.sort(np.array(t))
        return dict(ms_per_step=1e3 * float(np.median(s)), spread_ms=dict(min=1e3 * float(s[0]), q1=1e3 * float(np.percentile(s, 25)), q3=1e3 * float(np.percentile(s, 75)), max=1e3 * float(s[-1])))

    res = dict(batch=batch, steps=steps, warmup=warmup, sigma=sigma, library=capi.LIB_PATH, last_kernel=dev_srv.last_kernel(), factorizations_per_step=fact / steps,
               host_arrays=summary(t_host), device=summary(t_dev), same_bits_every_step=bool(same))
    host_srv.close()
    dev_srv.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
