"""What per-instance objective row counts (LsiBatch.set_instance_obj_dims) cost and save: the warm step of scripts/bench_lsi_instance_mask.py — perturb
the data on the device, solve again from active / x / v of the previous answer — configs[4], 1024 instances, ms per step of three entries
    run_device      LsiBatch.run_device per step (host-synchronous)
    enqueue_device  LsiBatch.enqueue_device per step in one stream, one finish() at the end
    graph           one captured step (perturbation + enqueue_device) replayed
under three settings
    none      no counts set (the "none" line of bench_lsi_instance_mask.py: what the parent commit runs)
    capacity  every count equal to its capacity: the same problems, the counts read and used
    half      every second instance with its last two objectives at half their rows
Every timed region is bracketed by a device synchronisation; the first repetition of each is discarded (allocations, capture).  The counts are set
before the cold step, so every loop starts from the answer of the problems it goes on solving.

    python scripts/bench_lsi_instance_dims.py [--batch 1024] [--steps 50] [--reps 5] [--settings none capacity half]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import lexlsi, problems as P  # noqa: E402

SETTINGS = ("none", "capacity", "half")


def counts_of(setting, batch, dims):
    c = np.tile(np.array(dims, np.int32), (batch, 1))
    if setting == "half":
        c[1::2, -2:] //= 2
    return c


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nvar", type=int, default=40)
    ap.add_argument("--dims", type=int, nargs="+", default=[12] * 5)
    ap.add_argument("--settings", nargs="+", default=list(SETTINGS), choices=SETTINGS)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pk = lexlsi.pack_batch(a.nvar, [P.lsi_problem(1000 + i, a.nvar, a.dims, simple_bounds=True) for i in range(a.batch)])
    data0 = torch.from_numpy(np.ascontiguousarray(pk.data)).to(dev)
    var = torch.from_numpy(np.ascontiguousarray(pk.var_index.view(np.int32))).to(dev)
    noise = 1e-3 * torch.randn(data0.shape, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1))
    o = 0
    for d, t in zip(pk.dims, pk.types):  # only the matrices move: every [lb | ub] keeps its order
        rows = int(d) * (0 if t == 1 else a.nvar)
        noise[:, o + rows: o + rows + 2 * int(d)] = 0.0
        o += rows + 2 * int(d)
    stream = torch.cuda.Stream(dev)
    results = {}

    def timed(loop, solves):
        times = []
        for _ in range(a.reps + 1):
            data = data0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(data)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / solves)
        return dict(ms_per_step_median=1e3 * float(np.median(times[1:])), ms_per_step_min=1e3 * float(np.min(times[1:])))

    for setting in a.settings:
        b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)  # a batch object per setting: the captured step keeps the pointers it was given
        if setting != "none":
            b.set_instance_obj_dims(torch.from_numpy(counts_of(setting, a.batch, a.dims)).to(dev))
        cold = b.run_device(data0, var)

        def sync_loop(data):
            r = cold
            for _ in range(a.steps):
                data += noise
                r = b.run_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"])

        def enqueue_loop(data):
            with torch.cuda.stream(stream):
                r = {k: t.clone() for k, t in cold.items()}
                for _ in range(a.steps):
                    data += noise
                    r = b.enqueue_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"], out=r)
            b.finish()

        res = dict(run_device=timed(sync_loop, a.steps), enqueue_device=timed(enqueue_loop, a.steps))

        gdata, state = data0.clone(), {k: t.clone() for k, t in cold.items()}
        with torch.cuda.stream(stream):
            b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state)  # the uncaptured call with the captured one's options
        b.finish()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            gdata += noise
            b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state)

        def graph_loop(data):
            with torch.cuda.stream(stream):  # (while the graph is in use the only call on the batch is finish: the cold answer is copied in)
                gdata.copy_(data)
                for k, t in cold.items():
                    state[k].copy_(t)
                for _ in range(a.steps):
                    graph.replay()
            b.finish(stream)

        res["graph"] = timed(graph_loop, a.steps)
        res["kernel"] = b.last_kernel()
        results[setting] = res
        b.close()
    print(json.dumps(dict(batch=a.batch, nvar=a.nvar, dims=a.dims, steps=a.steps, reps=a.reps, **results)))


if __name__ == "__main__":
    main()
