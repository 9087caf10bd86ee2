"""What per-instance factorization budgets (LsiBatch.set_instance_max_factorizations) cost: the warm step of scripts/bench_lsi_instance_mask.py —
perturb the data on the device, solve again from active / x / v of the previous answer — configs[4], 1024 instances, ms per step of three entries
    run_device      LsiBatch.run_device per step (host-synchronous)
    enqueue_device  LsiBatch.enqueue_device per step in one stream, one finish() at the end
    graph           one captured step (perturbation + enqueue_device) replayed
under four settings
    none     no limits set (the "none" line of bench_lsi_instance_mask.py: what the parent commit runs)
    zeros    every entry 0: the array is read, every instance takes the run's parameter
    budget2  every entry 2, the run's parameter 200: every instance continues from its own previous active / x / v (the anytime loop)
    shared2  no limits set, max_number_of_factorizations = 2 for the run: the same loop without the array
budget2 and shared2 must end in the same bits (x, info, active, v of the last step of each entry are compared: "same_bits") and take about the
same time.  Every timed region is bracketed by a device synchronisation; the first repetition of each is discarded (allocations, capture).

    python scripts/bench_lsi_instance_budget.py [--batch 1024] [--steps 50] [--reps 5] [--settings none zeros budget2 shared2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lexls_amd import lexlsi, problems as P  # noqa: E402

SETTINGS = ("none", "zeros", "budget2", "shared2")


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
    results, last = {}, {}

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
        limits = {"zeros": 0, "budget2": 2}.get(setting)
        par = dict(max_number_of_factorizations=2) if setting == "shared2" else {}
        cold = b.run_device(data0, var)  # every loop starts from the answer of the unlimited cold step
        if limits is not None:
            b.set_instance_max_factorizations(torch.full((a.batch,), limits, dtype=torch.int32, device=dev))
        final = {}

        def sync_loop(data):
            r = cold
            for _ in range(a.steps):
                data += noise
                r = b.run_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"], **par)
            final["run_device"] = r

        def enqueue_loop(data):
            with torch.cuda.stream(stream):
                r = {k: t.clone() for k, t in cold.items()}
                for _ in range(a.steps):
                    data += noise
                    r = b.enqueue_device(data, var, active_guess=r["active"], x0=r["x"], v0=r["v"], out=r, **par)
            b.finish()
            final["enqueue_device"] = r

        res = dict(run_device=timed(sync_loop, a.steps), enqueue_device=timed(enqueue_loop, a.steps))

        gdata, state = data0.clone(), {k: t.clone() for k, t in cold.items()}
        with torch.cuda.stream(stream):
            b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state, **par)  # the uncaptured call with the captured one's options
        b.finish()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            gdata += noise
            b.enqueue_device(gdata, var, active_guess=state["active"], x0=state["x"], v0=state["v"], out=state, **par)

        def graph_loop(data):
            with torch.cuda.stream(stream):  # (while the graph is in use the only call on the batch is finish: the cold answer is copied in)
                gdata.copy_(data)
                for k, t in cold.items():
                    state[k].copy_(t)
                for _ in range(a.steps):
                    graph.replay()
            b.finish(stream)
            final["graph"] = state

        res["graph"] = timed(graph_loop, a.steps)
        res["kernel"] = b.last_kernel()
        torch.cuda.synchronize()
        last[setting] = {e: {k: t.cpu().numpy().copy() for k, t in r.items()} for e, r in final.items()}
        res["on_budget"] = int((last[setting]["graph"]["info"][:, 0] == 2).sum())  # instances whose last step ended MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED
        results[setting] = res
        b.close()
    if "budget2" in last and "shared2" in last:
        results["same_bits"] = all(np.array_equal(np.ascontiguousarray(last["budget2"][e][k]).view(np.uint8), np.ascontiguousarray(last["shared2"][e][k]).view(np.uint8))
                                   for e in last["budget2"] for k in ("x", "info", "active", "v"))
    print(json.dumps(dict(batch=a.batch, nvar=a.nvar, dims=a.dims, steps=a.steps, reps=a.reps, **results)))


if __name__ == "__main__":
    main()
