"""Which kernel serves which shape: walks a fixed grid of small batches through the public API and records, per entry, the names the library
reports (lexls_lse_last_kernel, lexls_lse_last_consumer_kernel before and after a later solve, lexls_lse_prefix_reuse_ready;
lexls_lsi_batch_last_kernel for LexLSI batches) together with the device's CU count.

    python scripts/record_dispatch_table.py            # writes tests/dispatch_table.json

The table is a REFERENCE: it was recorded once, on the commit before the dispatch plan (lexls_dispatch.h) existed, and the code under test
never regenerates it.  tests/test_gpu_dispatch_table.py runs grid() through the same run_entries() and requires equality;
tests/test_dispatch_plan.py feeds query_line() of every entry to the planner on the host."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "dispatch_table.json")

# name: (caps, dims) — dims "caps": every problem at capacity; "ragged": per-problem dimensions (capacity or one row less, a zero level in
# problem 1); a list: the same dimensions for every problem, below capacity
LEVELS = {
    "u12": ([12, 12, 12], "caps"),
    "u8": ([8, 8, 8], "caps"),
    "r12": ([12, 12, 12], "ragged"),
    "r8": ([8, 8, 8], "ragged"),
    "l16": ([16, 14, 12], "caps"),
    "oddcap": ([13, 12, 12], [12, 12, 12]),  # uniform 12 in an odd capacity
    "deep12": ([12] * 6, "caps"),            # 72 rows: more than the register-resident kernel's image holds
    "deep16": ([16] * 5, "caps"),
    "mid": ([30] * 4, "caps"),               # generic kernel, 256 threads
    "row17": ([17, 12], "caps"),             # a level beyond 16 rows
    "big": ([103, 102], "caps"),             # 205 x 101 doubles: the smallest staging beyond a CU's LDS at n = 100
    "huge": ([100] * 4, "caps"),
}


def caps_of(e):
    """capacities of entry e: LEVELS' (every entry of grid()), or the entry's own "caps" (entries made outside the grid: tests/device_input_cases.py)"""
    return list(e["caps"]) if "caps" in e else LEVELS[e["levels"]][0]


def dims_of(e):
    """(batch, nObj) uint32 dimensions of entry e (batch resolved); an entry with its own "caps" is at capacity or carries "dims" (batch, nObj)"""
    if "caps" in e:
        return np.asarray(e["dims"], np.uint32) if "dims" in e else np.tile(np.asarray(e["caps"], np.uint32), (e["batch"], 1))
    caps, spec = LEVELS[e["levels"]]
    B = e["batch"]
    d = np.tile(np.asarray(caps, np.uint32), (B, 1))
    if spec == "ragged":
        for b in range(B):
            for k in range(len(caps)):
                if (b + k) % 2:
                    d[b, k] -= 1
        if B > 1:
            d[1, 1] = 0
    elif spec != "caps":
        d = np.tile(np.asarray(spec, np.uint32), (B, 1))
    return d


def E(levels, n, **kw):
    e = dict(kind="lse", levels=levels, n=n, batch=4, policy=0, keep=0, mode="fs", fixed=0, guard=0, reg=0, qtol0=0, align8=0)
    e.update(kw)
    return e


def grid():
    g = []
    # every policy on uniform levels of 12 rows at each column boundary (16/17, 32/33, 41/42, 48/49, 64/65), factor kept and x only
    for n in (15, 16, 31, 32, 40, 41, 47, 48, 63, 64):
        for policy in range(11):
            for keep in (0, 1):
                g.append(E("u12", n, policy=policy, keep=keep))
    for lv, ns, policies in (("u8", (15, 31, 32, 40, 47, 48), (0, 4, 6, 10)), ("r12", (15, 31, 32, 40, 47, 48), (0, 4, 6, 10)), ("r8", (20, 40), (0, 4, 6, 10)),
                             ("l16", (30, 40, 47, 55, 63), (0, 2, 3, 4)), ("oddcap", (40,), (0, 6, 7, 10)), ("deep12", (12, 20, 39, 40, 47), (0, 2, 4, 6)),
                             ("deep16", (50, 63, 64), (0, 2, 4)), ("mid", (100,), (0, 1, 5)), ("row17", (20,), (0, 4)), ("big", (100,), (0, 1, 5)),
                             ("huge", (200,), (1,))):
        for n in ns:
            for policy in policies:
                for keep in (0, 1):
                    g.append(E(lv, n, policy=policy, keep=keep, batch=2 if lv in ("mid", "big", "huge") else 4))
    # factorize alone (the caller asks for no x): what a later solve finds
    for lv, n, policy in (("u12", 40, 0), ("u12", 40, 4), ("mid", 100, 0), ("big", 100, 0), ("big", 100, 5), ("huge", 200, 1)):
        g.append(E(lv, n, policy=policy, keep=1, mode="f", batch=2))
    # fixed variables
    for lv, n in (("u12", 15), ("u12", 31), ("u12", 40), ("u12", 47), ("r12", 40), ("l16", 55), ("deep12", 40), ("deep16", 50), ("big", 100)):
        for policy in (0, 3, 4, 6):
            for keep in (0, 1):
                g.append(E(lv, n, policy=policy, keep=keep, fixed=1, batch=2 if lv == "big" else 4))
    # accuracy guard
    for lv, n in (("u12", 20), ("u12", 40), ("u12", 47), ("u8", 40), ("r12", 40), ("l16", 55), ("big", 100)):
        for policy in (0, 4, 6, 7, 10):
            for guard in (1, 2):
                g.append(E(lv, n, policy=policy, guard=guard, batch=2 if lv == "big" else 4))
    g.append(E("u12", 40, keep=1, guard=1))
    # LEXLS_QTOL=0
    for lv, n in (("u12", 20), ("u12", 40), ("u8", 40)):
        for policy in (0, 6):
            g.append(E(lv, n, policy=policy, qtol0=1))
    g.append(E("u12", 40, qtol0=1, guard=2))
    # regularization: Tikhonov (1), Tikhonov by CGLS (2), the experimental type 7
    for lv, n in (("u12", 20), ("u12", 40), ("u12", 41), ("l16", 55), ("deep12", 40), ("mid", 100)):
        for reg in (1, 2, 7):
            for policy in (0, 4):
                for keep in (0, 1):
                    g.append(E(lv, n, policy=policy, keep=keep, reg=reg, batch=2 if lv == "mid" else 4))
    # an input aligned to 8 bytes only
    for lv, n, policy in (("u12", 40, 0), ("u12", 40, 7), ("u12", 40, 10), ("r12", 40, 10), ("u12", 20, 6)):
        g.append(E(lv, n, policy=policy, align8=1))
    # both sides of the register-resident wave capacity, where the choice depends on it ("cap": CUs x 8)
    for lv, n, fixed in (("u12", 40, 0), ("u12", 39, 0), ("u12", 20, 0), ("u12", 20, 1), ("u12", 40, 1), ("l16", 55, 0)):
        for batch in ("cap-1", "cap", "cap+1"):
            g.append(E(lv, n, keep=1, fixed=fixed, batch=batch))
    g.append(E("u12", 40, keep=1, policy=2, batch="cap+1"))
    g.append(E("l16", 55, keep=0, batch="cap+1"))
    # LexLSI batches: plain, regularized, 42..48 columns; the persistent launch switched off, kernel policies from the environment (child processes)
    for shape in ("ik", "small", "wide", "slot48"):
        for reg in (0, 1, 7):
            g.append(dict(kind="lsi", shape=shape, reg=reg, env={}))
            g.append(dict(kind="lsi", shape=shape, reg=reg, env={"LEXLS_LSI_NO_FUSED": "1"}))
        for policy in ("1", "3", "4"):
            g.append(dict(kind="lsi", shape=shape, reg=0, env={"LEXLS_KERNEL_POLICY": policy}))
    for i, e in enumerate(g):
        e["id"] = i
    return g


LSI_SHAPES = {
    "ik": dict(n=40, dims=[12] * 5, factors=[0, 0.02, 0.05, 0.03, 0.04], count=8, seed=20261000),
    "small": dict(n=20, dims=[6, 5, 5, 6], factors=[0, 0.3, 0.2, 0.4], count=6, seed=700),
    "wide": dict(n=50, dims=[10, 16, 16, 14], factors=[0, 0.1, 0.2, 0.3], count=6, seed=20261500),
    "slot48": dict(n=47, dims=[8, 12, 12, 12], factors=[0, 0.1, 0.2, 0.3], count=6, seed=20261700),
}


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def resolve(e, cus):
    """the entry with its batch as a number"""
    e = dict(e)
    if isinstance(e.get("batch"), str):
        e["batch"] = cus * 8 + {"cap-1": -1, "cap": 0, "cap+1": 1}[e["batch"]]
    return e


def run_lse(e):
    import torch
    import lexls_amd
    from lexls_amd import problems as P
    from lexls_amd.capi import LexlsError
    caps, _ = LEVELS[e["levels"]]
    B, n = e["batch"], e["n"]
    qtol_before = os.environ.get("LEXLS_QTOL")  # (put back below: the library reads it at every solve)
    if e["qtol0"]:
        os.environ["LEXLS_QTOL"] = "0"
    else:
        os.environ.pop("LEXLS_QTOL", None)
    s = lexls_amd.BatchedLexLSE(B, n, caps)
    try:
        s.set_prefix_reuse(True)
        s.set_kernel_policy(e["policy"])
        s.setObjDim(dims_of(e))
        lod = P.lse_batch_fast(977 + e["id"], B, n, caps)
        keepalive = None
        if e["align8"]:
            keepalive = torch.zeros(lod.size + 1, dtype=torch.float64, device="cuda")
            keepalive[1:] = torch.from_numpy(lod.reshape(-1)).cuda()
            torch.cuda.synchronize()
            assert keepalive.data_ptr() % 16 == 0
            s.setProblemDevice(keepalive.data_ptr() + 8)
        else:
            s.setProblem(lod)
        if e["fixed"]:
            idx = np.zeros((B, n), np.uint32)
            idx[:, 0] = n - 1
            s.fixVariables(np.ones(B, np.uint32), idx, np.full((B, n), 0.25))
        if e["reg"]:
            s.setRegularization(e["reg"], [0.1] * len(caps))
        if e["guard"]:
            s.set_accuracy_guard(e["guard"])
        if e["mode"] == "f":
            s.factorize()
        else:
            s.factorize_solve(keep_factor=bool(e["keep"]))
        s.synchronize()
        out = dict(kernel=s.last_kernel(), consumer=s.last_consumer_kernel(), reuse_ready=int(s.prefix_reuse_ready()))
        try:
            s.solve()
            s.synchronize()
            out["solve"] = s.last_consumer_kernel()
        except LexlsError:
            out["solve"] = "error"
        return out
    finally:
        os.environ.pop("LEXLS_QTOL", None)
        if qtol_before is not None:
            os.environ["LEXLS_QTOL"] = qtol_before
        s.close()


def run_lsi(e):
    from lexls_amd import lexlsi, problems as P
    sh = LSI_SHAPES[e["shape"]]
    probs = [P.lsi_problem(sh["seed"] + i, sh["n"], sh["dims"]) for i in range(sh["count"])]
    pk = lexlsi.pack_batch(sh["n"], probs)
    b = lexlsi.LsiBatch(sh["n"], pk.dims, pk.types, len(probs))
    try:
        if e["reg"]:
            b.run(pk, regularization_factors=sh["factors"], regularization_type=e["reg"])
        else:
            b.run(pk)
        return dict(kernel=b.last_kernel())
    finally:
        b.close()


def run_entries(entries):
    """expectations of the entries, in order; LexLSI entries with environment switches run in one child process per switch set"""
    out = {}
    children = {}
    for e in entries:
        if e["kind"] == "lsi" and e["env"]:
            children.setdefault(json.dumps(e["env"], sort_keys=True), []).append(e)
        else:
            out[e["id"]] = run_lse(e) if e["kind"] == "lse" else run_lsi(e)
    for env_s, es in children.items():
        env = dict(os.environ)
        env.update(json.loads(env_s))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(es)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        got = json.loads(r.stdout.strip().splitlines()[-1])
        for e, g in zip(es, got):
            out[e["id"]] = g
    return [out[e["id"]] for e in entries]


def query_line(e, cus):
    """the plain numbers tests/dispatch_plan_check.cpp reads for one entry (resolved batch): kind id batch n nObj cap uniform_dim max_rows
    max_level_dim fixed reg align keep do_solve policy guard qtol0 wave_capacity sweep_serves"""
    if e["kind"] == "lsi":  # a resident round: capacities stand for the dimensions, simple bounds are fixed variables, the factor is kept
        sh = LSI_SHAPES[e["shape"]]
        cap = sum(sh["dims"])
        vals = ["lsi", e["id"], sh["count"], sh["n"], len(sh["dims"]), cap, 0, cap, max(sh["dims"]), 1, e["reg"], 16, 1, 1, int(e["env"].get("LEXLS_KERNEL_POLICY", 0)), 0, 0,
                cus * 8, 1]
        return " ".join(str(v) for v in vals)
    caps = caps_of(e)
    d = dims_of(e)
    uniform =int(d.max()) if d.min() == d.max() else 0
    keep, do_solve = (e["keep"], 1) if e["mode"] == "fs" else (1, 0)
    vals = ["lse", e["id"], e["batch"], e["n"], len(caps), int(sum(caps)), uniform, max(int(d.sum(axis=1).max()), 1), int(d.max()), e["fixed"], e["reg"], 8 if e["align8"] else 16,
            keep, do_solve, e["policy"], e["guard"], e["qtol0"], cus * 8, 0]
    return " ".join(str(v) for v in vals)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print(json.dumps([run_lsi(e) for e in json.loads(sys.argv[2])]))
        return
    cus = cu_count()
    entries = [resolve(e, cus) for e in grid()]
    got = run_entries(entries)
    table = dict(cu_count=cus, entries=[dict(entry=e, expect=x) for e, x in zip(grid(), got)])
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    with open(out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    names = sorted({x["kernel"] for x in got})
    print(f"{len(got)} entries, {len(names)} distinct kernels, CUs = {cus}")
    for nm in names:
        print("  ", nm)


if __name__ == "__main__":
    main()
