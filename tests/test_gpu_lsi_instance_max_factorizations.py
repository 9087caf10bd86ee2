"""lexls_lsi_batch_set_instance_max_factorizations (LsiBatch.set_instance_max_factorizations): an int32 per instance in device memory, read by the
kernels at the start of every device run; instance b with entry L >= 1 runs as one LexLSI object with max_number_of_factorizations =
min(L, the run's parameter), an entry <= 0 leaves it the run's parameter.  The tolerance is zero, as for every LexLSI path.

The yardstick is the oracle-backed driver, one call per instance with that instance's own limit: oracle.lsi_run for x, info, active and v,
oracle.lsi_run_debug for the working-set log (hence the cycling counter) and the multipliers.  Every comparison is on the bits.

Inputs: "ik", 32 instances of P.lsi_problem(seed, 40, (12,) * 5) (the 41 x 12 instantiation), cold; "warm", their neighbours (perturb = 0.1)
started from active / x / v of the base problems' solutions, which need 1 .. 19 factorizations — limits of 1, 2, 3 and 5 then end some instances
on their limit and let others finish below it; "wide", 16 instances of n = 50, (8, 16, 16, 12) (51 columns: the 64 x 16 instantiation); the
degenerate 40-instance batch of tests/test_gpu_lsi_cycling_resident.py for cycling handling.  The limits mix 0, -1, 1, 2, 3, 5 and 1000 (instance b
gets MIX[b % 7]); the cycling case adds 12, 14 and 60, limits that cut a run off between its first relaxation and the handler's cap.

Every test first asserts from the oracle's results alone (require) that a quarter of the instances end on their own limit where the unlimited
run needs more factorizations, that a limited instance ends PROBLEM_SOLVED below its limit and that an entry <= 0 is present.  The anytime chain
is the exception the task fixes: all its limits are 2, so no entry <= 0 exists there; the other two conditions are asserted over its steps.

LEXLS_LSI_NO_FUSED=1 is read when a run starts (monkeypatch); the capture runs child_capture in a process of its own, under a time limit, as
tests/test_gpu_lsi_enqueue_device.py does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

from lexls_amd import capi, lexlsi, problems as P
from oracle import oracle_ctypes as ORACLE  # (the `oracle` fixture's module: child_capture has no fixtures)
from test_gpu_lsi_cycling_resident import CAP50, degenerate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LEXLS_ERR_UNSUPPORTED = 3
SOLVED, EXCEEDED = 0, 2  # TerminationStatus: PROBLEM_SOLVED, MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED
SENTINEL = 7
CAPACITY = 256  # working-set log entries per instance: above the run's parameter, so above every log here
RUN_MAX = 200   # the run's parameter (the default of ParametersLexLSI)
MIX = (0, -1, 1, 2, 3, 5, 1000)
ENTRIES = ("sync", "enqueue")
INFO_KEYS = ("status", "iterations", "activations", "deactivations", "factorizations", "total_rank")
IK = dict(n=40, dims=[12] * 5, seeds=range(20265000, 20265032))
WIDE = dict(n=50, dims=[8, 16, 16, 12], seeds=range(20266000, 20266016))
BOUNDS = dict(n=14, dims=[4, 5, 5, 4], seeds=range(1300, 1340))
REG_FACTORS = (0, 0.02, 0.05, 0.03, 0.04)  # ik shape: one per objective
_cache = {}


def device():
    return torch.device("cuda", 0)


def mix(batch, values=MIX):
    return np.array([values[b % len(values)] for b in range(batch)], np.int32)


def effective(limit, run_max=RUN_MAX):
    return min(int(limit), run_max) if limit >= 1 else run_max


# ---- inputs: (n, problems, guess, x0, v0), computed once, shared, never modified ----
def inputs(name):
    if name not in _cache:
        if name == "ik":
            _cache[name] = (IK["n"], [P.lsi_problem(s, IK["n"], IK["dims"]) for s in IK["seeds"]], None, None, None)
        elif name == "wide":
            _cache[name] = (WIDE["n"], [P.lsi_problem(s, WIDE["n"], WIDE["dims"]) for s in WIDE["seeds"]], None, None, None)
        elif name == "degenerate":
            _cache[name] = (BOUNDS["n"], [degenerate(s, BOUNDS["n"], BOUNDS["dims"]) for s in BOUNDS["seeds"]], None, None, None)
        else:  # "warm" (perturb 0.1) and "chain" (perturb 0.03): neighbours of the ik problems, started from the base problems' solutions
            n, base = inputs("ik")[:2]
            sol = [ORACLE.lsi_run(n, p) for p in base]
            probs = [P.lsi_problem(s, n, IK["dims"], perturb=0.1 if name == "warm" else 0.03, perturb_seed=1) for s in IK["seeds"]]
            _cache[name] = (n, probs, np.stack([np.concatenate(o["active"]) for o in sol]), np.stack([o["x"] for o in sol]), np.stack([np.concatenate(o["v"]) for o in sol]))
    return _cache[name]


def oracle_refs(name, limits, debug=False, run_max=RUN_MAX, start=None, **kw):
    """the oracle-backed driver per instance under min(limit, run_max) (limit <= 0: run_max); limits None: the unlimited run.  start: (guess, x0,
    v0) in place of the inputs' own (not cached).  debug: with ["log"] and ["lambda"] of lsi_run_debug.  Computed once per key, shared, never modified"""
    key = ("refs", name, None if limits is None else tuple(int(l) for l in limits), debug, run_max, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if start is not None or key not in _cache:
        n, probs, guess, x0, v0 = inputs(name)
        if start is not None:
            guess, x0, v0 = start
        cuts = np.cumsum([len(o["lb"]) for o in probs[0]])[:-1]
        refs = []
        for i, p in enumerate(probs):
            args = dict(active_guess=None if guess is None else np.split(guess[i], cuts), x0=None if x0 is None else x0[i], v0=None if v0 is None else np.split(v0[i], cuts),
                        max_number_of_factorizations=run_max if limits is None else effective(limits[i], run_max), **kw)
            o = ORACLE.lsi_run(n, p, **args)
            if debug:
                d = ORACLE.lsi_run_debug(n, p, **args)
                assert d["info"] == o["info"]
                o["log"], o["lambda"] = d["debug"]["working_set_log"], d["debug"]["lambda"]
            refs.append(o)
        if start is not None:
            return refs  # (a step of a chain: not kept)
        _cache[key] = refs
    return _cache[key]


def require(refs, unlimited, limits, run_max=RUN_MAX):
    """the precondition of every test, from the oracle alone"""
    cut = sum(l >= 1 and o["info"]["status"] == EXCEEDED and o["info"]["factorizations"] == effective(l, run_max) and u["info"]["factorizations"] > o["info"]["factorizations"]
              for l, o, u in zip(limits, refs, unlimited))
    assert 4 * cut >= len(refs), f"only {cut} of {len(refs)} instances end on their own limit while the unlimited run needs more"
    assert any(l >= 1 and o["info"]["status"] == SOLVED and o["info"]["factorizations"] < l for l, o in zip(limits, refs)), "no limited instance ends PROBLEM_SOLVED below its limit"
    assert any(l <= 0 for l in limits), "no entry <= 0"


# ---- the device side ----
def upload(name, start=None):
    n, probs, guess, x0, v0 = inputs(name)
    if start is not None:
        guess, x0, v0 = start
    pk = lexlsi.pack_batch(n, probs)
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(device())
    t = dict(data=up(pk.data.reshape(pk.batch, -1), np.float64), var_index=up(pk.var_index.reshape(pk.batch, -1).view(np.int32), np.int32),
             active_guess=up(guess, np.uint8), x0=up(x0, np.float64), v0=up(v0, np.float64))
    return pk, t


def new_batch(pk, limits=None, log=False):
    """-> the batch object and the limits tensor it holds (None: no limits set)"""
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    if log:
        b.set_working_set_log(CAPACITY)
    lt = None
    if limits is not None:
        lt = torch.from_numpy(np.asarray(limits, np.int32)).to(device())
        b.set_instance_max_factorizations(lt)
    return b, lt


def sentinel_outputs(pk):
    shapes = dict(x=((pk.batch, pk.nvar), torch.float64), info=((pk.batch, 6), torch.int32), active=((pk.batch, pk.total), torch.uint8), v=((pk.batch, pk.total), torch.float64),
                  cycling_counters=((pk.batch,), torch.int32), **{"lambda": ((pk.batch, len(pk.dims), pk.total), torch.float64)})
    out = {k: torch.full(s, SENTINEL, dtype=d, device=device()) for k, (s, d) in shapes.items()}
    torch.cuda.synchronize()
    return out


def solve(entry, b, t, out, lam=True, regularization_factors=None, **kw):
    """one run through `entry` into the tensors of `out` (lambda only with lam) -> host copies"""
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    torch.cuda.synchronize()
    if entry == "sync":
        par = lexlsi.pack_params_ex(**kw) if regularization_factors is not None or any(k in lexlsi.REG_PARAM_KEYS for k in kw) else lexlsi.pack_params(**kw)
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        capi.check(capi.lib().lexls_lsi_batch_run_device_ex(
            b._h, ptr(t["data"]), ptr(t["var_index"]), ptr(t["active_guess"]), ptr(t["x0"]), ptr(t["v0"]), None if rfa is None else rfa.ctypes.data_as(C.POINTER(C.c_double)),
            par.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(par)), ptr(out["x"]), ptr(out["info"]), ptr(out["active"]), ptr(out["v"]), ptr(out["lambda"]) if lam else None,
            ptr(out["cycling_counters"])))
    else:
        status = torch.zeros(1, dtype=torch.int32, device=device())
        b.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], regularization_factors=regularization_factors, v0=t["v0"], with_lambda=lam,
                         with_cycling_counters=True, status=status, out=out, **kw)
        b.finish()
        assert int(status.item()) == -1
    return host(out)


def host(out):
    torch.cuda.synchronize()
    return {k: a.detach().cpu().numpy().copy() for k, a in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def assert_equals_oracle(got, refs, what, lam=True, only=None):
    """every row of x, info, active, v, the cycling counter (with a log in the reference) and the multipliers (lam) is the oracle's"""
    for b, o in enumerate(refs):
        if only is not None and not only[b]:
            continue
        assert dict(zip(INFO_KEYS, got["info"][b].tolist())) == o["info"], (what, b, got["info"][b].tolist(), o["info"])
        np.testing.assert_array_equal(got["x"][b].view(np.uint64), o["x"].view(np.uint64), err_msg=f"{what}: x of instance {b}")
        np.testing.assert_array_equal(got["active"][b], np.concatenate(o["active"]), err_msg=f"{what}: active of instance {b}")
        np.testing.assert_array_equal(got["v"][b].view(np.uint64), np.concatenate(o["v"]).view(np.uint64), err_msg=f"{what}: v of instance {b}")
        if "log" in o:
            assert int(got["cycling_counters"][b]) == sum(1 for e in o["log"] if e["cycling_detected"]), (what, b)
        if lam:
            np.testing.assert_array_equal(np.ascontiguousarray(got["lambda"][b].T).view(np.uint64), np.vstack(o["lambda"]).view(np.uint64), err_msg=f"{what}: multipliers of instance {b}")


def assert_same_bits(got, ref, what, keys=("x", "info", "active", "v", "cycling_counters", "lambda")):
    for k in keys:
        np.testing.assert_array_equal(bits(got[k]), bits(ref[k]), err_msg=f"{what}: {k}")


def limited_run(entry, name, limits, what, lam=True, log=False, kernel="lsi_fused<", **kw):
    """the preconditions, then one run under `limits` on a fresh batch object against the per-instance oracle -> (outputs, the batch's log arrays)"""
    refs, unlimited = oracle_refs(name, limits, debug=True, **kw), oracle_refs(name, None, **kw)
    require(refs, unlimited, limits)
    pk, t = upload(name)
    b, _ = new_batch(pk, limits, log=log)
    try:
        got = solve(entry, b, t, sentinel_outputs(pk), lam=lam, **kw)
        assert b.last_kernel().startswith(kernel), b.last_kernel()
        assert_equals_oracle(got, refs, what, lam=lam)
        np.testing.assert_array_equal(b.cycling_counters(), got["cycling_counters"].view(np.uint32))  # the library's own record of the run
        if lam:
            np.testing.assert_array_equal(bits(b.lambda_array()), bits(got["lambda"]))
        return got, b.working_set_log_arrays() if log else None
    finally:
        b.close()


# ---- 1: the persistent launch ----
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["ik", "warm", "wide"])
def test_persistent_launch(hip, name, entry):
    limits = mix(len(inputs(name)[1]))
    limited_run(entry, name, limits, f"{name}, {entry}", kernel="lsi_fused<lqr_wave<64,16" if name == "wide" else "lsi_fused<lqr_wave<41,12")


# ---- 2: the lock-step stages ----
@pytest.mark.parametrize("name", ["warm", "wide"])
def test_stage_path(hip, monkeypatch, name):
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    pk, t = upload(name)
    limits = mix(pk.batch)
    refs = oracle_refs(name, limits, debug=True)
    require(refs, oracle_refs(name, None), limits)
    b, _ = new_batch(pk, limits)
    try:
        got = solve("sync", b, t, sentinel_outputs(pk))
        assert not b.last_kernel().startswith("lsi_fused<") and b.last_kernel() not in ("host", ""), b.last_kernel()
        assert_equals_oracle(got, refs, f"{name}, stages")
    finally:
        b.close()


def test_two_groups(hip, monkeypatch):
    """group g reads its limits from word lo[g] of the array"""
    monkeypatch.setenv("LEXLS_LSI_GROUPS", "2")  # (read when a batch object is made)
    pk, t = upload("warm")
    limits = mix(pk.batch)
    assert not np.array_equal(limits[:pk.batch // 2], limits[pk.batch // 2:])
    refs = oracle_refs("warm", limits, debug=True)
    require(refs, oracle_refs("warm", None), limits)
    b, _ = new_batch(pk, limits)
    try:
        got = solve("sync", b, t, sentinel_outputs(pk))
        assert b.stats()["groups"] == 2
        assert_equals_oracle(got, refs, "two groups")
    finally:
        b.close()


# ---- 3: enqueue_device + finish equals run_device on a second batch object ----
def test_enqueue_equals_run_device(hip):
    pk, t = upload("warm")
    limits = mix(pk.batch)
    refs = oracle_refs("warm", limits, debug=True)
    require(refs, oracle_refs("warm", None), limits)
    ba, _ = new_batch(pk, limits)
    bs, _ = new_batch(pk, limits)
    try:
        enq = ba.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], with_lambda=True, with_cycling_counters=True)
        ba.finish()
        ref = bs.run_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], with_lambda=True, with_cycling_counters=True)
        assert_same_bits(host(enq), host(ref), "enqueue_device against run_device")
        assert_equals_oracle(host(enq), refs, "enqueue_device")
        assert ba.last_kernel() == bs.last_kernel() and ba.stats() == bs.stats()
    finally:
        ba.close()
        bs.close()


# ---- 4: a captured step picks up rewritten limits on replay ----
def child_capture():
    """an uncaptured enqueue + finish, a captured one, two replays with the limits tensor rewritten by a torch op in between: each replay equals
    the oracle under the limits present at that replay.  A replay that reports a fault ends the test: nothing else is started"""
    pk, t = upload("warm")  # (torch opens the device first)
    first = mix(pk.batch)
    second, third = np.roll(first, 3), np.where(np.arange(pk.batch) % 2 == 0, 2, -1).astype(np.int32)
    unlimited = oracle_refs("warm", None)
    for limits in (first, second, third):
        require(oracle_refs("warm", limits, debug=True), unlimited, limits)
    assert any(a["info"] != b["info"] for a, b in zip(oracle_refs("warm", first, debug=True), oracle_refs("warm", second, debug=True)))
    b, lt = new_batch(pk, first)
    stream = torch.cuda.Stream(device())
    out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
    kw = dict(v0=t["v0"], with_cycling_counters=True, with_lambda=True, status=status, out=out)
    with torch.cuda.stream(stream):
        b.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], **kw)  # the uncaptured run that may allocate
    b.finish()
    assert_equals_oracle(host(out), oracle_refs("warm", first, debug=True), "uncaptured")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        b.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], **kw)
    for turn, limits in enumerate((second, third)):
        new = torch.from_numpy(limits).to(device())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for a in out.values():
                a.fill_(SENTINEL)
            lt.copy_(new)  # a torch op on the tensor the library holds
            graph.replay()
        b.finish(stream)  # (raises on a fault: the test ends here)
        assert int(status.item()) == -1, turn
        assert_equals_oracle(host(out), oracle_refs("warm", limits, debug=True), f"replay {turn}")
        np.testing.assert_array_equal(bits(b.lambda_array()), bits(host(out)["lambda"]))
    b.close()


def test_captured_step(hip):
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_instance_max_factorizations as m; m.child_capture()"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]


# ---- 5: the limits of a run are those present when it starts ----
def test_snapshot(hip):
    pk, t = upload("warm")
    limits = mix(pk.batch)
    refs, ones = oracle_refs("warm", limits, debug=True), oracle_refs("warm", np.ones(pk.batch, np.int32), debug=True)
    require(refs, oracle_refs("warm", None), limits)
    assert any(a["info"] != b["info"] for a, b in zip(refs, ones))
    b, lt = new_batch(pk, limits)
    try:
        stream = torch.cuda.Stream(device())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            first = b.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], with_lambda=True, with_cycling_counters=True)
            lt.fill_(1)  # directly behind the enqueue, in the same stream
        b.finish()
        assert_equals_oracle(host(first), refs, "the run in front of the rewrite")
        with torch.cuda.stream(stream):
            second = b.enqueue_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], with_lambda=True, with_cycling_counters=True)
        b.finish()
        assert_equals_oracle(host(second), ones, "the run behind the rewrite")
    finally:
        b.close()


# ---- 6: with an instance mask ----
@pytest.mark.parametrize("entry", ENTRIES)
def test_with_a_mask(hip, entry):
    pk, t = upload("warm")
    limits = mix(pk.batch)
    refs = oracle_refs("warm", limits, debug=True)
    mask = (np.arange(pk.batch) % 3 != 1).astype(np.uint8)
    solved = np.flatnonzero(mask)
    require([refs[i] for i in solved], [oracle_refs("warm", None)[i] for i in solved], limits[solved])  # (the solved instances alone satisfy it)
    assert {int(l) for l in limits[solved]} == set(MIX), "a value of the mix is only on skipped instances"
    garbage = limits.copy()
    garbage[mask == 0] = np.resize(np.array([-2 ** 31, 2 ** 31 - 1, 1], np.int32), int((mask == 0).sum()))  # a skipped instance's entry is not read
    b, _ = new_batch(pk, garbage)
    try:
        b.set_instance_mask(torch.from_numpy(mask).to(device()))
        got = solve(entry, b, t, sentinel_outputs(pk))
        for k, a in got.items():
            assert (a[mask == 0] == SENTINEL).all(), f"{entry}: {k} of a skipped instance was written"
        assert_equals_oracle(got, refs, f"{entry}: with a mask", only=mask != 0)
    finally:
        b.close()


# ---- 7: other options ----
@pytest.mark.parametrize("entry", ENTRIES)
def test_deactivate_first_wrong_sign(hip, entry):
    limited_run(entry, "ik", mix(len(IK["seeds"])), f"{entry}: deactivate_first_wrong_sign", deactivate_first_wrong_sign=1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_regularized_run(hip, entry):
    limited_run(entry, "ik", mix(len(IK["seeds"])), f"{entry}: TIKHONOV, shared factors", lam=False, kernel="lsi_fused<lqr_wave<41,12", regularization_type=1,
                regularization_factors=REG_FACTORS)


CYCLING_MIX = (0, -1, 1, 2, 3, 5, 12, 14, 60)
SOLVING = (6, 11, 24, 36, 39)  # instances of the degenerate batch that relax bounds and then end PROBLEM_SOLVED (asserted): they get 1000


@pytest.mark.parametrize("entry", ENTRIES)
def test_cycling_handling(hip, entry):
    limits = mix(len(BOUNDS["seeds"]), CYCLING_MIX)
    limits[list(SOLVING)] = 1000
    assert set(MIX) <= set(limits.tolist())
    refs = oracle_refs("degenerate", limits, debug=True, **CAP50)
    relaxed = [sum(1 for e in o["log"] if e["cycling_detected"]) for o in refs]
    assert all(refs[i]["info"]["status"] == SOLVED and relaxed[i] > 0 for i in SOLVING)
    # cycling handling is tested before the limit: some instance relaxes a bound and then ends on its own limit, before the handler's cap
    assert sum(l >= 1 and o["info"]["status"] == EXCEEDED and 0 < r < CAP50["cycling_max_counter"] for l, o, r in zip(limits, refs, relaxed)) >= 3
    assert any(o["info"]["status"] == 1 for o in refs), "no instance ends PROBLEM_SOLVED_CYCLING_HANDLING"
    got, _ = limited_run(entry, "degenerate", limits, f"{entry}: cycling handling", lam=False, **CAP50)
    np.testing.assert_array_equal(got["cycling_counters"].view(np.uint32), np.array(relaxed, np.uint32))


@pytest.mark.parametrize("entry", ENTRIES)
def test_working_set_log(hip, entry):
    limits = mix(len(IK["seeds"]))
    _, (log, alpha, counts) = limited_run(entry, "warm", limits, f"{entry}: working-set log", log=True)
    refs = oracle_refs("warm", limits, debug=True)
    assert sum(len(o["log"]) for o in refs) > 0 and max(len(o["log"]) for o in refs) <= CAPACITY
    np.testing.assert_array_equal(counts, np.array([len(o["log"]) for o in refs], np.uint32))
    for b, o in enumerate(refs):
        want = np.array([[e[k] for k in capi.WORKING_SET_LOG_FIELDS] for e in o["log"]], np.int32).reshape(len(o["log"]), len(capi.WORKING_SET_LOG_FIELDS))
        np.testing.assert_array_equal(log[b, :len(want)], want, err_msg=f"instance {b}")
        np.testing.assert_array_equal(alpha[b, :len(want)].view(np.uint64), np.array([e["alpha_or_lambda"] for e in o["log"]]).view(np.uint64), err_msg=f"instance {b}")
        assert not log[b, len(want):].any() and not alpha[b, len(want):].any(), b


# ---- 8: the anytime chain ----
STEPS = 6


def test_anytime_chain(hip):
    """every limit is 2, the run's parameter 200; active / x / v go back in as active_guess / x0 / v0, STEPS times, on the device and in the oracle"""
    pk, t = upload("chain")
    twos = np.full(pk.batch, 2, np.int32)
    start, chain = inputs("chain")[2:], []
    for _ in range(STEPS):
        refs = oracle_refs("chain", twos, start=start)
        chain.append(refs)
        start = (np.stack([np.concatenate(o["active"]) for o in refs]), np.stack([o["x"] for o in refs]), np.stack([np.concatenate(o["v"]) for o in refs]))
    unlimited = oracle_refs("chain", None)
    assert 4 * sum(o["info"]["status"] == EXCEEDED and u["info"]["factorizations"] > 2 for o, u in zip(chain[0], unlimited)) >= pk.batch
    assert any(o["info"]["status"] == EXCEEDED for o in chain[2]), "nobody is still on its budget at the third step"
    assert any(o["info"]["status"] == SOLVED and o["info"]["factorizations"] < 2 for refs in chain for o in refs)
    assert all(o["info"]["status"] == SOLVED for o in chain[-1]), "the chain has not converged"
    limited, _ = new_batch(pk, twos)
    shared, _ = new_batch(pk)
    try:
        a = b = t
        for step, refs in enumerate(chain):
            ra = limited.run_device(a["data"], a["var_index"], a["active_guess"], a["x0"], v0=a["v0"], with_cycling_counters=True, max_number_of_factorizations=RUN_MAX)
            rb = shared.run_device(b["data"], b["var_index"], b["active_guess"], b["x0"], v0=b["v0"], with_cycling_counters=True, max_number_of_factorizations=2)
            assert_equals_oracle(host(ra), refs, f"step {step}", lam=False)
            assert_same_bits(host(ra), host(rb), f"step {step}: per-instance limits 2 against the shared parameter 2", keys=("x", "info", "active", "v", "cycling_counters"))
            a = dict(t, active_guess=ra["active"], x0=ra["x"], v0=ra["v"])
            b = dict(t, active_guess=rb["active"], x0=rb["x"], v0=rb["v"])
    finally:
        limited.close()
        shared.close()


# ---- 9: None clears; run() is refused while limits are set ----
def test_none_clears_and_run_is_refused(hip):
    pk, t = upload("warm")
    limits = mix(pk.batch)
    require(oracle_refs("warm", limits, debug=True), oracle_refs("warm", None), limits)
    b, _ = new_batch(pk, limits)
    fresh, _ = new_batch(pk)
    try:
        with pytest.raises(capi.LexlsError) as e:
            b.run(pk)
        assert str(e.value).startswith(f"liblexls_hip error {LEXLS_ERR_UNSUPPORTED}:") and "lexls_lsi_batch_set_instance_max_factorizations" in str(e.value), str(e.value)
        x, info = np.full((pk.batch, pk.nvar), 7.0), np.full((pk.batch, 6), 7, np.int32)
        active, v, rounds = np.full((pk.batch, pk.total), 7, np.uint8), np.full((pk.batch, pk.total), 7.0), np.full(2, 7, np.int32)
        par = lexlsi.pack_params()
        p = lambda a, c: a.ctypes.data_as(C.POINTER(c))
        rc = capi.lib().lexls_lsi_batch_run(b._h, p(pk.data, C.c_double), p(pk.var_index, C.c_uint32), None, None, None, None, p(par, C.c_double), C.c_uint32(len(par)),
                                            p(x, C.c_double), p(info, C.c_int32), p(active, C.c_uint8), p(v, C.c_double), p(rounds, C.c_int32))
        assert rc == LEXLS_ERR_UNSUPPORTED
        assert all((a == 7).all() for a in (x, info, active, v, rounds)), "a refused run wrote an output"
        limited = solve("sync", b, t, sentinel_outputs(pk))
        b.set_instance_max_factorizations(None)
        got, want = solve("sync", b, t, sentinel_outputs(pk)), solve("sync", fresh, t, sentinel_outputs(pk))
        assert_same_bits(got, want, "after None")
        assert not np.array_equal(limited["info"], got["info"]), "the limits changed nothing: clearing them shows nothing"
        assert b.last_kernel() == fresh.last_kernel() and b.stats() == fresh.stats()
        assert_equals_oracle(got, oracle_refs("warm", None), "after None", lam=False)
        r, w = b.run(pk), fresh.run(pk)  # the host-driven entry serves the batch again
        np.testing.assert_array_equal(r["info"].array, w["info"].array)
        for k in ("x", "active", "v"):
            np.testing.assert_array_equal(bits(r[k]), bits(w[k]), err_msg=k)
    finally:
        b.close()
        fresh.close()
