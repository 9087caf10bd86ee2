#!/usr/bin/env python3
"""What the hot-start options of LexLSI (h_params slots 12 .. 16) buy in the closed loop on the device: the configs[4] batch (1024 lock-step LexLSI
instances, n = 40, 5 x 12, level 0 simple bounds) in the perturbed-data warm loop of scripts/bench_lsi_device_warm_loop.py — solve, move the bounds
on the device, solve again from active / x of the previous answer (no v0: with v0 given phase 1 forms A x only and the options do nothing).
Four settings   defaults | modify_type_active_enabled + modify_type_inactive_enabled | use_phase1_v0 | all five on (set_min_init_ctr_violation off)
through three routes   LsiBatch.run_device | LsiBatch.enqueue_device + finish | a captured enqueue_device replayed (data moved inside the graph),
every (setting, route) on its own batch object, the twelve loops alternating step by step within one visit on the same perturbations.  Per loop:
median and quartiles of the ms per step and the factorizations per step and instance (info column 4).  Prints one JSON line.
  python scripts/bench_lsi_hot_start.py [batch] [steps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
steps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 25
n, dims, warmup, sigma = 40, [12] * 5, 3, 0.05
TYPES = dict(modify_type_active_enabled=1, modify_type_inactive_enabled=1)
SETTINGS = {"defaults": {}, "modify_type": TYPES, "use_phase1_v0": dict(use_phase1_v0=1),
            "all": dict(TYPES, modify_x_guess_enabled=1, set_min_init_ctr_violation=0, use_phase1_v0=1)}
ROUTES = ["run_device", "enqueue_device", "captured_replay"]


def main():
    import torch
    from bench_lsi_device_warm_loop import bound_columns
    from lexls_amd import capi, lexlsi, problems as P
    base = lexlsi.pack_batch(n, [P.lsi_problem(20260500 + b, n, dims) for b in range(batch)])
    pos, row, rows = bound_columns(base)
    rng = np.random.default_rng(20260500)
    shifts = sigma * rng.standard_normal((warmup + steps, batch, rows))
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(pos).to(dev)
    d_shifts = torch.from_numpy(np.ascontiguousarray(shifts[:, :, row])).to(dev)
    d_var = torch.from_numpy(base.var_index.view(np.int32)).to(dev)
    stream = torch.cuda.Stream(dev)
    loops = {}
    for sname, opts in SETTINGS.items():
        for route in ROUTES:
            srv = lexlsi.LsiBatch(n, base.dims, base.types, batch)
            data = torch.from_numpy(base.data.copy()).to(dev)
            shift = torch.zeros_like(d_shifts[0])
            state = {k: a.clone() for k, a in srv.run_device(data, d_var).items()}  # the cold answer every loop starts from (and library load, first launches)
            lp = dict(srv=srv, data=data, shift=shift, state=state, opts=opts, t=[], fact=0)
            if route != "run_device":
                with torch.cuda.stream(stream):
                    srv.enqueue_device(data, d_var, active_guess=state["active"], x0=state["x"], out=state, **opts)  # the uncaptured run that may allocate
                srv.finish()
                with torch.cuda.stream(stream):
                    srv.enqueue_device(data, d_var, out=state)
                srv.finish()
            if route == "captured_replay":
                lp["graph"] = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(lp["graph"], stream=stream):
                    data[:, d_pos] += shift
                    srv.enqueue_device(data, d_var, active_guess=state["active"], x0=state["x"], out=state, **opts)
            loops[(sname, route)] = lp
    torch.cuda.synchronize()
    for k in range(warmup + steps):
        for (sname, route), lp in loops.items():
            srv, data, state, opts = lp["srv"], lp["data"], lp["state"], lp["opts"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "run_device":
                data[:, d_pos] += d_shifts[k]
                r = srv.run_device(data, d_var, active_guess=state["active"], x0=state["x"], **opts)
                for key in state:
                    state[key] = r[key]
                torch.cuda.synchronize()
            elif route == "enqueue_device":
                with torch.cuda.stream(stream):
                    data[:, d_pos] += d_shifts[k]
                    srv.enqueue_device(data, d_var, active_guess=state["active"], x0=state["x"], out=state, **opts)
                stream.synchronize()
            else:
                with torch.cuda.stream(stream):
                    lp["shift"].copy_(d_shifts[k])
                    lp["graph"].replay()
                stream.synchronize()
            t1 = time.perf_counter()
            if k >= warmup:
                lp["t"].append(t1 - t0)
                lp["fact"] += int(state["info"][:, 4].sum().item())

    def summary(lp):
        s = np.sort(np.array(lp["t"]))
        return dict(ms_per_step=1e3 * float(np.median(s)), spread_ms=dict(min=1e3 * float(s[0]), q1=1e3 * float(np.percentile(s, 25)), q3=1e3 * float(np.percentile(s, 75)), max=1e3 * float(s[-1])),
                    factorizations_per_step_and_instance=lp["fact"] / (steps * batch))

    res = dict(batch=batch, steps=steps, warmup=warmup, sigma=sigma, library=capi.LIB_PATH,
               loops={f"{sname}/{route}": summary(lp) for (sname, route), lp in loops.items()})
    for (sname, route), lp in loops.items():
        lp.pop("graph", None)
        if route != "run_device":
            lp["srv"].finish(stream)  # the host's view of the last enqueued run, so that the batch can be closed
        lp["srv"].close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
