"""The hot-start options of LexLSI (h_params slots 12 .. 16) on the GPU, bit for bit against the host driver over the CPU equality solver
(tests/hot_start_ref.cpp, built with g++ here), on the routes that serve them: lexls_lsi_solve_ex, lexls_lsi_batch_run (host phase 1),
lexls_lsi_batch_run_device and lexls_lsi_batch_enqueue_device (device phase 1: lsi_phase1_setup_hot_kernel); every PROBLEM_SOLVED instance must
also pass the tests/lexopt.py certificate.  use_phase1_v0 runs on all of them (device: lsi_phase1_v0_kernel).  Further: the stages under LEXLS_LSI_NO_FUSED=1 and lexls_lsi_batch_run under
LEXLS_LSI_DEVICE_PHASE1=1 (one child process), a captured replay after data and x0 were rewritten in place, a mask with NaN in a masked x0, per-instance
budgets, cycling handling, a given v0, per-instance row counts (NaN in the absent rows), TIKHONOV damping, the multipliers (with_lambda) and the
working-set log, each against the helper."""
import functools
import os
import shutil
import subprocess
import tempfile
import atexit

import numpy as np
import pytest

import lexopt
from lexls_amd import capi
from lexls_amd import lexlsi as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCHES = ["inactive->LB", "inactive->UB", "LB kept", "LB->inactive", "LB->UB", "UB kept", "UB->inactive", "UB->LB", "EQ untouched",
            "x: inactive->midpoint", "x: LB->lb", "x: UB/EQ->ub", "v: inside->0", "v: outside->midpoint residual"]
SHAPES = {  # name -> (n, dims, simple bounds first, batch)
    "simple6": (6, [4, 3, 5, 4], True, 12),
    "general8": (8, [3, 5, 4], False, 12),
    "n50": (50, [16, 16, 16], False, 4),
}
ALL_ON = dict(modify_x_guess_enabled=1, modify_type_active_enabled=1, modify_type_inactive_enabled=1, set_min_init_ctr_violation=0)
TYPES_ON = dict(modify_type_active_enabled=1, modify_type_inactive_enabled=1)


@functools.lru_cache(maxsize=None)
def helper():
    cxx = shutil.which("g++")
    assert cxx is not None, "the expected values need g++"
    d = tempfile.mkdtemp(prefix="hot_start_ref_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "hot_start_ref")
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read() else []
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", *fma, "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "lexls_amd", "csrc"), os.path.join(ROOT, "tests", "hot_start_ref.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the batch in the flat layout (data, var, guess, x0) and as objective lists"""
    n, dims, simple, batch = SHAPES[name]
    rng = np.random.default_rng({"simple6": 6001, "general8": 8002, "n50": 5003}[name])
    total, types = sum(dims), [1 if (simple and k == 0) else 0 for k in range(len(dims))]
    data, var, probs = [], [], []
    for _ in range(batch):
        chunks, objs = [], []
        for k, m in enumerate(dims):
            if types[k]:
                vi = rng.permutation(n)[:m].astype(np.uint32)
                lb, ub = -0.5 - 0.25 * rng.random(m), 0.5 + 0.25 * rng.random(m)
                objs.append(dict(var=vi, lb=lb, ub=ub))
                chunks.append(np.concatenate([lb, ub]))
                var.append(vi)
            else:
                A, mid = rng.standard_normal((m, n)), rng.standard_normal(m) * 0.5
                lb, ub = mid - 0.375, mid + 0.375
                if m > 2:
                    ub[1] = lb[1]  # an equality
                objs.append(dict(A=A, lb=lb, ub=ub))
                chunks.append(np.asfortranarray(np.hstack([A, lb[:, None], ub[:, None]])).ravel(order="F"))
        data.append(np.concatenate(chunks))
        probs.append(objs)
    guess = rng.integers(0, 3, size=(batch, total)).astype(np.uint8)
    x0 = 0.75 * rng.standard_normal((batch, n))
    return dict(n=n, dims=np.array(dims, np.uint32), types=np.array(types, np.int32), batch=batch, total=total, data=np.ascontiguousarray(np.stack(data)),
                var=np.ascontiguousarray(np.stack(var)) if var else None, guess=guess, x0=x0, probs=probs)


@functools.lru_cache(maxsize=None)
def expected(name, opts, counts=None, reg=None, lam=False, with_x0=True):
    """counts: per instance the rows of every objective (tuple of tuples) or None; reg: one regularization factor per objective or None; lam: the
    multipliers as well; with_x0 = False: no x guess"""
    c, par = case(name), L.pack_params_hot(**dict(opts))
    lines = [f"{c['n']} {len(c['dims'])} {c['batch']} 1 {int(with_x0)} {int(counts is not None)} {int(reg is not None)} {int(lam)}", " ".join(str(int(d)) for d in c["dims"]),
             " ".join(str(int(t)) for t in c["types"]), " ".join(float(p).hex() for p in par)]
    if reg is not None:
        lines.append(" ".join(float(f).hex() for f in reg))
    for b in range(c["batch"]):
        if counts is not None:
            lines.append(" ".join(str(int(k)) for k in counts[b]))
        lines.append(" ".join(float(d).hex() for d in c["data"][b]))
        if c["var"] is not None:
            lines.append(" ".join(str(int(i)) for i in c["var"][b]))
        lines.append(" ".join(str(int(g)) for g in c["guess"][b]))
        if with_x0:
            lines.append(" ".join(float(d).hex() for d in c["x0"][b]))
    r = subprocess.run([helper()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(x=[], info=[], active=[], v=[], log=[], lam=[])
    for ln in r.stdout.splitlines():
        key, *vals = ln.split()
        if key in ("x", "v"):
            out[key].append([float.fromhex(t) for t in vals])
        elif key in ("info", "active"):
            out[key].append([int(t) for t in vals])
        elif key == "log":  # per entry: obj_index, ctr_index, ctr_type, cycling_detected, rank, alpha_or_lambda
            out["log"].append([tuple(int(t) for t in vals[1 + 6 * i:6 + 6 * i]) + (float.fromhex(vals[6 + 6 * i]),) for i in range(int(vals[0]))])
        elif key == "lambda":
            out["lam"].append([float.fromhex(t) for t in vals])
        elif key == "branches":
            out["branches"] = [int(t) for t in vals]
        elif key == "removed_hot":
            out["removed_hot"] = int(vals[0])
    for k in ("x", "v"):
        out[k] = np.array(out[k])
    out["info"], out["active"] = np.array(out["info"], np.int32), np.array(out["active"], np.uint8)
    out["lam"] = np.array(out["lam"]).reshape(c["batch"], len(c["dims"]), c["total"]) if lam else None
    return out


def same_bits(got, ref, what):
    for k in ("x", "v"):
        assert np.array_equal(np.asarray(got[k], np.float64).view(np.uint64), ref[k].view(np.uint64)), f"{what}: {k} differs from the host driver"
    assert np.array_equal(np.asarray(got["active"]), ref["active"]), f"{what}: active set"
    assert np.array_equal(np.asarray(got["info"]), ref["info"]), f"{what}: info6 {np.asarray(got['info']).tolist()} vs {ref['info'].tolist()}"


# deactivate_first_wrong_sign with a simple-bounds objective: the instances of simple6 that the rule leaves PROBLEM_SOLVED at a point that is not optimal,
# with modify_type_* on (with and without use_phase1_v0).  The defect is the rule's, known from tests/test_lexopt_certificate.py
# (FIRST_WRONG_SIGN_NOT_OPTIMAL); pinned by index so that one more such instance fails
FIRST_WRONG_SIGN_NOT_OPTIMAL = (2, 3, 4, 6, 7, 8, 9)


def certify(c, ref, known_not_optimal=()):
    for b in range(c["batch"]):
        if ref["info"][b, 0] == 0:  # PROBLEM_SOLVED
            t = lexopt.certificate(c["n"], c["probs"][b], ref["x"][b])
            if b in known_not_optimal:
                assert t.max() > lexopt.ACCEPT, (b, t, "listed as not optimal, but it is")
            else:
                assert t.max() <= lexopt.ACCEPT, (b, t)


def device_tensors(c):
    import torch
    dev = torch.device("cuda", 0)
    t = dict(data=torch.from_numpy(c["data"]).to(dev), guess=torch.from_numpy(c["guess"]).to(dev), x0=torch.from_numpy(c["x0"]).to(dev),
             var=None if c["var"] is None else torch.from_numpy(c["var"].astype(np.int32)).to(dev))
    return t


def host(r):
    return dict(x=r["x"].cpu().numpy(), v=r["v"].cpu().numpy(), active=r["active"].cpu().numpy(), info=r["info"].cpu().numpy())


OPTION_SETS = {"types": TYPES_ON, "all": ALL_ON, "types_first_wrong_sign": dict(TYPES_ON, deactivate_first_wrong_sign=1), "midpoint_only": dict(set_min_init_ctr_violation=0),
               "v0_only": dict(use_phase1_v0=1), "v0_all": dict(ALL_ON, use_phase1_v0=1), "v0_first_wrong_sign": dict(TYPES_ON, use_phase1_v0=1, deactivate_first_wrong_sign=1),
               "all_cycling": dict(ALL_ON, cycling_handling_enabled=1)}


def ref_of(name, o):
    return expected(name, tuple(sorted(o.items())))


def test_the_cases_take_every_branch_of_phase_1():
    """CPU only (the helper): over the batches every branch of formInitialWorkingSet, of the x rewrite and of initialize_v0 is taken, a
    constraint phase 1 activated leaves again later, and what the helper calls solved is lexicographically optimal (tests/lexopt.py)"""
    for name in SHAPES:
        for key, o in OPTION_SETS.items():
            # deactivate_first_wrong_sign is certified on the general-only shapes.  With a simple-bounds objective that rule alone, every option here at its
            # default, ends instances as PROBLEM_SOLVED at points that are not optimal (8 of the 12 of simple6): the known defect of the restated
            # driver that tests/test_gpu_lsi_optimality.py documents (FIRST_WRONG_SIGN_NOT_OPTIMAL), not something the hot-start options bring
            known = FIRST_WRONG_SIGN_NOT_OPTIMAL if ("first_wrong_sign" in key and name == "simple6") else ()
            certify(case(name), expected(name, tuple(sorted(o.items()))), known)
    tot, removed = np.zeros(len(BRANCHES), np.int64), 0
    for name in SHAPES:
        for o in (ALL_ON, OPTION_SETS["midpoint_only"]):  # (with modify_type_inactive_enabled no inactive row is left outside its bounds)
            ref = expected(name, tuple(sorted(o.items())))
            tot += np.array(ref["branches"])
            removed += ref["removed_hot"]
    print(dict(zip(BRANCHES, tot.tolist())), "removed after a hot activation:", removed)
    assert all(tot > 0), dict(zip(BRANCHES, tot.tolist()))
    assert removed > 0


@pytest.mark.gpu
@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_route_has_the_host_drivers_bits(name, opts):
    import torch
    c, o = case(name), OPTION_SETS[opts]
    ref = ref_of(name, o)
    # one problem at a time
    for b in range(min(c["batch"], 4)):
        r = L.lsi_solve(c["n"], c["probs"][b], active_guess=np.split(c["guess"][b], np.cumsum(c["dims"])[:-1]), x0=c["x0"][b], **o)
        one = dict(x=r["x"][None], v=np.concatenate(r["v"])[None], active=np.concatenate(r["active"])[None], info=np.array([[r["info"][k] for k in L.INFO_KEYS]], np.int32))
        same_bits(one, {k: ref[k][b:b + 1] for k in ("x", "v", "active", "info")}, f"lsi_solve, instance {b}")
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        pk = L.PackedBatch(c["n"], c["dims"], c["types"], c["data"], c["var"])
        r = s.run(pk, active_guess=c["guess"], x0=c["x0"], **o)
        same_bits(dict(x=r["x"], v=r["v"], active=r["active"], info=r["info"].array), ref, "batch_run")
        t = device_tensors(c)
        keep = {k: (None if v is None else v.clone()) for k, v in t.items()}
        d = s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
        torch.cuda.synchronize()
        same_bits(host(d), ref, "run_device")
        hot_kernel = s.last_kernel()
        s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"])
        assert hot_kernel == s.last_kernel(), (hot_kernel, s.last_kernel())
        d = s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], with_cycling_counters=True, **o)  # lexls_lsi_batch_run_device_ex
        same_bits(host(d), ref, "run_device_ex")
        e = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
        s.finish()
        same_bits(host(e), ref, "enqueue_device")
        for k, v in t.items():  # the caller's arrays keep their bits
            assert v is None or torch.equal(v, keep[k]), f"the caller's {k} was written"
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["all", "v0_all"])
def test_captured_replay_after_data_and_x0_were_rewritten_in_place(opts):
    """the instances move one place on (data, variable indices, guess, x0 rewritten where they lie): the replay gives the moved expected values"""
    import torch
    c, o = case("simple6"), OPTION_SETS[opts]
    ref = ref_of("simple6", o)
    moved = {k: np.roll(ref[k], 1, axis=0) for k in ("x", "v", "active", "info")}
    t = device_tensors(c)
    t2 = {k: torch.roll(v, 1, 0) for k, v in t.items()}
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        with torch.cuda.stream(stream):
            out = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
        s.finish()
        same_bits(host(out), ref, "enqueue_device before the capture")
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], out=out, **o)
        with torch.cuda.stream(stream):
            for k in t:
                t[k].copy_(t2[k])
            for a in out.values():
                a.fill_(3)
            graph.replay()
        s.finish(stream)
        same_bits(host(out), moved, "captured replay")
    finally:
        s.close()


def child_stages_and_device_phase1():
    """LEXLS_LSI_NO_FUSED=1 and LEXLS_LSI_DEVICE_PHASE1=1 are set: lexls_lsi_batch_run has the device's phase 1 (host arrays), run_device the stages"""
    import torch
    assert os.environ.get("LEXLS_LSI_NO_FUSED") == "1" and os.environ.get("LEXLS_LSI_DEVICE_PHASE1") == "1"
    for name in ("simple6", "general8"):
        c = case(name)
        s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
        t = device_tensors(c)
        for key in ("all", "types_first_wrong_sign", "midpoint_only", "v0_only", "v0_all"):
            o, ref = OPTION_SETS[key], ref_of(name, OPTION_SETS[key])
            r = s.run(L.PackedBatch(c["n"], c["dims"], c["types"], c["data"], c["var"]), active_guess=c["guess"], x0=c["x0"], **o)
            same_bits(dict(x=r["x"], v=r["v"], active=r["active"], info=r["info"].array), ref, f"{name} {key}: batch_run, phase 1 on the device")
            d = s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
            torch.cuda.synchronize()
            same_bits(host(d), ref, f"{name} {key}: run_device, stages")
        if name == "general8":  # without x0 the state is formed behind the first solve: lsi_phase1_finish_hot_kernel against lexls_lsi_solve_ex
            o = OPTION_SETS["midpoint_only"]
            d = host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], **o))
            for b in range(3):
                r = L.lsi_solve(c["n"], c["probs"][b], active_guess=np.split(c["guess"][b], np.cumsum(c["dims"])[:-1]), **o)
                assert np.array_equal(d["x"][b].view(np.uint64), r["x"].view(np.uint64)) and np.array_equal(d["v"][b].view(np.uint64), np.concatenate(r["v"]).view(np.uint64)), b
        s.close()
    print("child ok")


@pytest.mark.gpu
def test_stages_and_device_phase1_of_batch_run_in_a_child_process():
    import sys
    env = dict(os.environ, LEXLS_LSI_NO_FUSED="1", LEXLS_LSI_DEVICE_PHASE1="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_lsi_hot_start as T; T.child_stages_and_device_phase1()"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_use_phase1_v0_reports_one_factorization_fewer_where_the_helper_says_so():
    """use_phase1_v0 alone against the default run: on the instances where the host driver saves phase 1's factorization the device does too"""
    import torch
    c = case("general8")
    o = OPTION_SETS["v0_only"]
    ref, ref_plain = ref_of("general8", o), ref_of("general8", {})
    marked = ref["info"][:, 4] + 1 == ref_plain["info"][:, 4]
    print("factorizations with / without use_phase1_v0:", ref["info"][:, 4].tolist(), ref_plain["info"][:, 4].tolist())
    assert marked.any(), "no instance of the batch saves the factorization"
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        with_v0 = host(s.run_device(t["data"], active_guess=t["guess"], x0=t["x0"], **o))
        plain = host(s.run_device(t["data"], active_guess=t["guess"], x0=t["x0"]))
        same_bits(plain, ref_plain, "run_device, defaults")
        assert np.array_equal(with_v0["info"][marked, 4] + 1, plain["info"][marked, 4]), (with_v0["info"][:, 4], plain["info"][:, 4])
        assert np.array_equal(with_v0["info"][:, 4], ref["info"][:, 4])
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [1, 2])
def test_use_phase1_v0_with_per_instance_budgets(budget):
    """instance b under its own budget = one LexLSI object with that max_number_of_factorizations; every other instance has the run's"""
    import torch
    c = case("simple6")
    o = OPTION_SETS["v0_all"]
    full, short = ref_of("simple6", o), ref_of("simple6", dict(o, max_number_of_factorizations=budget))
    limits = np.zeros(c["batch"], np.int32)
    limits[::2] = budget
    want = {k: np.where((limits > 0).reshape(-1, *([1] * (full[k].ndim - 1))), short[k], full[k]) for k in ("x", "v", "active", "info")}
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        s.set_instance_max_factorizations(torch.from_numpy(limits).to("cuda"))
        same_bits(host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)), want, f"run_device, budget {budget}")
        e = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
        s.finish()
        same_bits(host(e), want, f"enqueue_device, budget {budget}")
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["all", "v0_all"])
def test_options_with_a_mask_and_nan_in_a_masked_x0(opts):
    import torch
    c, o = case("simple6"), OPTION_SETS[opts]
    ref = ref_of("simple6", o)
    mask = np.ones(c["batch"], np.uint8)
    mask[[1, 4, 11]] = 0
    t = device_tensors(c)
    t["x0"][torch.from_numpy(mask == 0).to("cuda")] = float("nan")
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        s.set_instance_mask(torch.from_numpy(mask).to("cuda"))
        out = {k: torch.full_like(a, 3) for k, a in s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"]).items()}
        e = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], out=out, **o)
        s.finish()
        got = host(e)
        on = mask != 0
        same_bits({k: got[k][on] for k in got}, {k: ref[k][on] for k in got}, "the instances the mask keeps")
        for k in got:
            assert (got[k][~on] == 3).all(), f"{k} of a masked instance was written"
    finally:
        s.close()


@pytest.mark.gpu
def test_a_given_v0_switches_the_options_off_and_keeps_its_bits():
    """with x0 and v0 phase 1 forms A x only (objective.h:226-236): the options change nothing, d_v0 is only read"""
    import torch
    c = case("simple6")
    t = device_tensors(c)
    v0 = torch.from_numpy(0.125 * np.random.default_rng(77).standard_normal((c["batch"], c["total"]))).to("cuda")
    keep = v0.clone()
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        plain = host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], v0=v0))
        hot = host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], v0=v0, **ALL_ON))
        same_bits(hot, plain, "run_device_ex with v0: options on against options off")
        for b in range(3):
            r = L.lsi_solve(c["n"], c["probs"][b], active_guess=np.split(c["guess"][b], np.cumsum(c["dims"])[:-1]), x0=c["x0"][b],
                            v0=np.split(keep[b].cpu().numpy(), np.cumsum(c["dims"])[:-1]), **ALL_ON)
            assert np.array_equal(hot["x"][b].view(np.uint64), r["x"].view(np.uint64)), b
        assert torch.equal(v0, keep), "the caller's v0 was written"
    finally:
        s.close()


@pytest.mark.gpu
def test_use_phase1_v0_without_x0_and_other_parameter_counts_are_refused():
    import ctypes as C
    import torch
    c = case("general8")
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        lib, dp = capi.lib(), C.POINTER(C.c_double)
        par = L.pack_params_hot(use_phase1_v0=1)
        x = torch.full((c["batch"], c["n"]), -7.0, dtype=torch.float64, device="cuda")
        info = torch.full((c["batch"], 6), -7, dtype=torch.int32, device="cuda")
        act = torch.full((c["batch"], c["total"]), 7, dtype=torch.uint8, device="cuda")
        v = torch.full((c["batch"], c["total"]), -7.0, dtype=torch.float64, device="cuda")
        outs = [C.c_void_p(a.data_ptr()) for a in (x, info, act, v)]
        data, guess = C.c_void_p(t["data"].data_ptr()), C.c_void_p(t["guess"].data_ptr())
        calls = {
            "run_device": lambda p, n: lib.lexls_lsi_batch_run_device(s._h, data, None, guess, None, None, p.ctypes.data_as(dp), C.c_uint32(n), *outs),
            "run_device_ex": lambda p, n: lib.lexls_lsi_batch_run_device_ex(s._h, data, None, guess, None, None, None, p.ctypes.data_as(dp), C.c_uint32(n), *outs, None, None),
            "enqueue_device": lambda p, n: lib.lexls_lsi_batch_enqueue_device(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), data, None, guess, None, None, None,
                                                                             p.ctypes.data_as(dp), C.c_uint32(n), *outs, None, None, None),
        }
        for who, call in calls.items():
            rc = call(par, 17)
            assert rc == 1, (who, rc)  # LEXLS_ERR_INVALID
            assert "when use_phase1_v0 = true, x_guess has to be specified" in lib.lexls_last_error().decode(), who
            rc = call(np.zeros(13), 13)
            assert rc == 1 and "9, 12 or 17" in lib.lexls_last_error().decode(), who
            torch.cuda.synchronize()
            assert bool((x == -7.0).all()) and bool((info == -7).all()) and bool((act == 7).all()) and bool((v == -7.0).all()), f"{who}: a refused call wrote an output"
        with pytest.raises(Exception, match="x_guess has to be specified"):
            s.run(L.PackedBatch(c["n"], c["dims"], c["types"], c["data"], c["var"]), active_guess=c["guess"], use_phase1_v0=1)
    finally:
        s.close()


def counts_of(c):
    """rows every objective of every instance has: between 1 and its capacity, full capacity for instance 0"""
    rng = np.random.default_rng(4242)
    k = np.stack([rng.integers(1, int(d) + 1, size=c["batch"]) for d in c["dims"]], axis=1).astype(np.int32)
    k[0] = c["dims"]
    return k


def absent_rows(c, counts):
    gone = np.zeros((c["batch"], c["total"]), bool)
    first = [int(f) for f in np.concatenate([[0], np.cumsum(c["dims"])[:-1]])]
    for b in range(c["batch"]):
        for k, d in enumerate(c["dims"]):
            gone[b, first[k] + int(counts[b, k]):first[k] + int(d)] = True
    return gone


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["all", "v0_all", "types_first_wrong_sign", "midpoint_only_no_x0"])
@pytest.mark.parametrize("name", ["simple6", "general8"])
def test_options_with_per_instance_row_counts(name, opts):
    """every instance is one LexLSI of its own dims; the absent rows of the capacity layout hold NaN (data, bounds) and are not looked at"""
    import torch
    c = case(name)
    with_x0 = not opts.endswith("_no_x0")
    o = OPTION_SETS[opts.replace("_no_x0", "")]
    counts = counts_of(c)
    ref = expected(name, tuple(sorted(o.items())), counts=tuple(map(tuple, counts.tolist())), with_x0=with_x0)
    gone = absent_rows(c, counts)
    assert not ref["active"][gone].any() and not ref["v"][gone].any()
    data, off, first = c["data"].copy(), 0, 0
    for k, d in enumerate(int(d) for d in c["dims"]):  # NaN into every entry of an absent row
        cols = 2 if c["types"][k] == 1 else c["n"] + 2
        blk = data[:, off:off + d * cols].reshape(c["batch"], cols, d)
        blk[np.repeat(gone[:, None, first:first + d], cols, axis=1)] = np.nan
        off, first = off + d * cols, first + d
    t = device_tensors(dict(c, data=data))
    x0 = t["x0"] if with_x0 else None
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        s.set_instance_obj_dims(torch.from_numpy(counts).to("cuda"))
        same_bits(host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=x0, **o)), ref, "run_device with row counts")
        e = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=x0, **o)
        s.finish()
        same_bits(host(e), ref, "enqueue_device with row counts")
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["all", "v0_all"])
@pytest.mark.parametrize("name", ["simple6", "general8"])
def test_options_with_tikhonov_damping(name, opts):
    import torch
    c = case(name)
    o = dict(OPTION_SETS[opts], regularization_type=1)  # REGULARIZATION_TIKHONOV
    reg = tuple(0.0 if t == 1 else 0.05 * (k + 1) for k, t in enumerate(c["types"]))
    ref = expected(name, tuple(sorted(o.items())), reg=reg)
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        r = s.run(L.PackedBatch(c["n"], c["dims"], c["types"], c["data"], c["var"]), active_guess=c["guess"], x0=c["x0"], regularization_factors=np.array(reg), **o)
        same_bits(dict(x=r["x"], v=r["v"], active=r["active"], info=r["info"].array), ref, "batch_run, TIKHONOV")
        same_bits(host(s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], regularization_factors=np.array(reg), **o)), ref, "run_device, TIKHONOV")
        e = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], regularization_factors=np.array(reg), **o)
        s.finish()
        same_bits(host(e), ref, "enqueue_device, TIKHONOV")
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["all", "v0_all", "v0_only"])
@pytest.mark.parametrize("name", ["simple6", "general8"])
def test_options_with_lambda(name, opts):
    """LexLSI::getLambda of the final working set, written on the device (d_lambda) and fetched afterwards (lexls_lsi_batch_get_lambda)"""
    import torch
    c, o = case(name), OPTION_SETS[opts]
    ref = expected(name, tuple(sorted(o.items())), lam=True)
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        for what in ("run_device", "enqueue_device"):
            if what == "run_device":
                r = s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], with_lambda=True, **o)
            else:
                r = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], with_lambda=True, **o)
                s.finish()
            same_bits(host(r), ref, what)
            lam = r["lambda"].cpu().numpy()
            assert np.array_equal(lam.view(np.uint64), ref["lam"].view(np.uint64)), f"{what}: the multipliers differ from the host driver's by {np.abs(lam - ref['lam']).max()}"
            assert np.array_equal(s.lambda_array().view(np.uint64), ref["lam"].view(np.uint64)), f"{what}: get_lambda afterwards"
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["v0_only", "v0_all", "v0_first_wrong_sign", "all"])
@pytest.mark.parametrize("name", ["simple6", "general8"])
def test_working_set_log_of_the_device_runs(name, opts):
    """every entry against LexLSI::getWorkingSetLog of the host driver: constraint, type, cycling flag, rank (0 for iteration 0 of use_phase1_v0: nothing
    has been factorized), step length or multiplier"""
    import torch
    c, o = case(name), OPTION_SETS[opts]
    ref = ref_of(name, o)
    t = device_tensors(c)
    s = L.LsiBatch(c["n"], c["dims"], c["types"], c["batch"])
    try:
        s.set_working_set_log(256)  # (an instance that runs into max_number_of_factorizations logs 200 changes)
        assert max(len(g) for g in ref["log"]) <= 256 and any(len(g) for g in ref["log"])
        for what in ("run_device", "enqueue_device"):
            if what == "run_device":
                r = s.run_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
            else:
                r = s.enqueue_device(t["data"], var_index=t["var"], active_guess=t["guess"], x0=t["x0"], **o)
                s.finish()
            same_bits(host(r), ref, what)
            logs, counts = s.working_set_log()
            for b in range(c["batch"]):
                got = [(e["obj_index"], e["ctr_index"], e["ctr_type"], e["cycling_detected"], e["rank"], e["alpha_or_lambda"]) for e in logs[b]]
                assert int(counts[b]) == len(ref["log"][b]) and got == ref["log"][b], (what, b, got, ref["log"][b])
        if opts == "v0_only":  # (with modify_type_inactive_enabled iteration 0 is never blocked: every violated row is active already)
            firsts = [g[0] for g in ref["log"] if g]
            assert any(e[4] == 0 for e in firsts), "no instance logs a change in iteration 0 (rank 0)"
    finally:
        s.close()
