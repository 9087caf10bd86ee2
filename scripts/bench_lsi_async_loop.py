"""The closed loop of scripts/bench_lsi_device_warm_loop.py — solve, perturb the data on the device, solve again from active / x / v of the previous
answer — three ways, per-step wall time of each:
    run_device      LsiBatch.run_device per step (host-synchronous: the baseline, unchanged code)
    enqueue_device  LsiBatch.enqueue_device per step in one stream, one finish() at the end
    graph           one captured step (perturbation + enqueue_device) replayed steps - 1 times from the cold answer
Every timed region is bracketed by a device synchronisation; the first repetition of each way is discarded (allocations, capture).

    python scripts/bench_lsi_async_loop.py [--batch 1024] [--steps 50] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import lexlsi, problems as P  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nvar", type=int, default=40)
    ap.add_argument("--dims", type=int, nargs="+", default=[12] * 5)
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
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    stream = torch.cuda.Stream(dev)
    results = {}

    def timed(name, loop, solves):
        times = []
        for _ in range(a.reps + 1):
            data = data0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(data)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / solves)
        results[name] = dict(ms_per_step_median=1e3 * float(np.median(times[1:])), ms_per_step_min=1e3 * float(np.min(times[1:])))

    def sync_loop(data):
        r = b.run_device(data, var)
        for _ in range(a.steps - 1):
            data += noise
            r = b.run_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"])

    def enqueue_loop(data):
        with torch.cuda.stream(stream):
            r = b.enqueue_device(data, var)
            for _ in range(a.steps - 1):
                data += noise
                r = b.enqueue_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"], out=r)
        b.finish()

    timed("run_device", sync_loop, a.steps)
    timed("enqueue_device", enqueue_loop, a.steps)

    # one captured step on buffers of its own: perturb, solve from the previous answer in place
    gdata = data0.clone()
    with torch.cuda.stream(stream):
        state = b.enqueue_device(gdata, var)
        b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state)  # the uncaptured call with the captured one's options
    b.finish()
    with torch.cuda.stream(stream):
        state = b.enqueue_device(gdata, var, out=state)  # the cold answer every repetition starts from
    b.finish()
    cold = {k: t.clone() for k, t in state.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        gdata += noise
        b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state)

    def graph_loop(data):
        with torch.cuda.stream(stream):  # (while the graph is in use the only call on the batch is finish: the cold answer is copied in)
            gdata.copy_(data)
            for k, t in cold.items():
                state[k].copy_(t)
            for _ in range(a.steps - 1):
                graph.replay()
        b.finish(stream)

    timed("graph", graph_loop, a.steps - 1)
    print(json.dumps(dict(batch=a.batch, nvar=a.nvar, dims=a.dims, steps=a.steps, reps=a.reps, kernel=b.last_kernel(), **results)))
    b.close()


if __name__ == "__main__":
    main()
