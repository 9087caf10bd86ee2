"""lexls_lsi_batch_set_instance_obj_dims (LsiBatch.set_instance_obj_dims): batch x nObj row counts in device memory; the batch's dims are capacities
and instance i is the LexLSI problem made of the first counts[i, k] rows of every objective k.  The tolerance is zero.

Expected values never come from the batch code under test: x, info, active and v of instance i are oracle.lsi_run on the problem TRUNCATED to its
counts, embedded into the capacity layout with zeros in the absent rows; the multipliers and the working-set log are those of
lexls_lsi_solve_debug (the single-problem driver) on the same truncated problem.  Every comparison is assert_array_equal, on the bits of x, v and
the multipliers and on the values of the log's alpha_or_lambda.

Shapes: small, n = 10, (4, 3, 4), 8 instances; ik, n = 40, 5 x 12 with simple bounds, 6 instances (lsi_fused<lqr_wave<41,12,..>>); wide, n = 50, levels of
14 rows, 4 instances (the 64 x 16 instantiation); bounds, n = 14, (4, 5, 5, 4) with a simple-bounds objective 0 whose count differs per instance, 8
instances.  The preconditions of every batch (an ADD and a REMOVE in the oracle's runs, an x that differs from the full-capacity x, a truncated
equality objective, an instance at full capacity) are asserted from the oracle alone.  The capture runs child_capture in a process of its own, under
a time limit, as tests/test_gpu_lsi_enqueue_device.py does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

from lexls_amd import capi, lexlsi, problems as P
from oracle import oracle_ctypes as ORACLE  # (the `oracle` fixture's module: child_capture has no fixtures)
from test_gpu_lsi_cycling_resident import CAP3, degenerate
from test_gpu_lsi_instance_mask import device, host, rows, sentinel_outputs, solve

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LEXLS_ERR_INVALID, LEXLS_ERR_UNSUPPORTED = 1, 3
SENTINEL = 7
CAPACITY = 128  # working-set log entries per instance
INFO_KEYS = ("status", "iterations", "activations", "deactivations", "factorizations", "total_rank")
ENTRIES = ("sync", "enqueue")
SHAPES = dict(small=dict(n=10, dims=[4, 3, 4], simple_bounds=False, seeds=range(4100, 4108)),
              ik=dict(n=40, dims=[12] * 5, simple_bounds=True, seeds=range(20265000, 20265006)),
              wide=dict(n=50, dims=[14, 14, 14, 14], simple_bounds=False, seeds=range(20266000, 20266004)),
              bounds=dict(n=14, dims=[4, 5, 5, 4], simple_bounds=True, seeds=range(1300, 1308)))
KERNEL = dict(small="lsi_fused<", ik="lsi_fused<lqr_wave<41,12", wide="lsi_fused<lqr_wave<64,16", bounds="lsi_fused<")
_cache = {}


# ---- inputs and counts: computed once, shared, never modified ----
def problems(shape, maker=P.lsi_problem):
    key = ("problems", shape, maker.__name__)
    if key not in _cache:
        s = SHAPES[shape]
        _cache[key] = [maker(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"]) for seed in s["seeds"]]
    return _cache[key]


def full(shape):
    s = SHAPES[shape]
    return np.tile(np.array(s["dims"], np.uint32), (len(s["seeds"]), 1))


def counts_of(shape, variant=0):
    """every fourth instance at full capacity; the others lose 0 .. 2 rows per objective, the last (equality) objective at least one on odd instances"""
    c = full(shape)
    batch, nobj = c.shape
    for i in range(batch):
        if i % 4 == 0:
            continue
        for k in range(nobj):
            c[i, k] -= (i * (k + 2) + k + variant) % 3
        if i % 2 == 1 and c[i, -1] == SHAPES[shape]["dims"][-1]:
            c[i, -1] -= 1
    return c


def truncated(objs, cnt):
    return [{key: np.ascontiguousarray(a[:int(c)]) for key, a in o.items()} for o, c in zip(objs, cnt)]


def firsts(dims):
    return np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(int)


def embed(parts, dims, cnt, dtype):
    """per-objective arrays of the truncated problem -> one capacity-layout row, zeros in the absent rows"""
    out = np.zeros(int(np.sum(dims)), dtype)
    for f, c, p in zip(firsts(dims), cnt, parts):
        out[f:f + int(c)] = p
    return out


def split_start(dims, cnt, row):
    """a capacity-layout row (guess, v0) -> the truncated problem's per-objective arrays"""
    return [row[f:f + int(c)] for f, c in zip(firsts(dims), cnt)]


def oracle_refs(shape, counts, start=None, debug=False, maker=P.lsi_problem, **kw):
    """per instance the oracle-backed driver on the truncated problem, in capacity layout: x, info (6), active, v.  start: (guess, x0, v0) in capacity
    layout (v0 may be None).  debug: + "lambda" (nObj x total, capacity layout) and "log" of lexls_lsi_solve_debug on the truncated problem"""
    key = ("refs", shape, counts.tobytes(), None if start is None else tuple(None if a is None else a.tobytes() for a in start), debug, maker.__name__,
           tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        s = SHAPES[shape]
        dims, refs = s["dims"], []
        for i, objs in enumerate(problems(shape, maker)):
            cnt, args = counts[i], dict(kw)
            if start is not None:
                args.update(active_guess=split_start(dims, cnt, start[0][i]), x0=start[1][i])
                if start[2] is not None:
                    args.update(v0=split_start(dims, cnt, start[2][i]))
            o = ORACLE.lsi_run(s["n"], truncated(objs, cnt), **args)
            ref = dict(x=o["x"], info=np.array([o["info"][k] for k in INFO_KEYS], np.int32), active=embed(o["active"], dims, cnt, np.uint8), v=embed(o["v"], dims, cnt, np.float64))
            if debug:
                d = lexlsi.lsi_solve_debug(s["n"], truncated(objs, cnt), **args)
                assert d["info"] == o["info"], (shape, i)
                lam = np.vstack(d["debug"]["lambda"]).T  # nObj x (rows of the truncated problem)
                ft = firsts(cnt)
                ref["lambda"] = np.stack([embed([col[f:f + int(c)] for f, c in zip(ft, cnt)], dims, cnt, np.float64) for col in lam])
                ref["log"] = d["debug"]["working_set_log"]
            refs.append(ref)
        _cache[key] = refs
    return _cache[key]


def require(shape, counts, refs, cap=None, **kw):
    """the preconditions, from the oracle alone: a vacuous batch proves nothing.  cap: the oracle's results at full capacity (None: oracle_refs with kw)"""
    dims = np.array(SHAPES[shape]["dims"])
    info = np.stack([r["info"] for r in refs])
    assert info[:, 2].sum() > 0 and info[:, 3].sum() > 0, f"{shape}: the oracle makes no ADD or no REMOVE"
    if cap is None:
        cap = oracle_refs(shape, full(shape), **kw)
    assert any(not np.array_equal(r["x"], c["x"]) for r, c in zip(refs, cap)), f"{shape}: truncation changes no x"
    assert (counts[:, -1] < dims[-1]).any(), f"{shape}: no equality row is lost"
    assert (counts == dims).all(axis=1).any(), f"{shape}: no instance at full capacity"
    assert (counts <= dims).all()


# ---- the device side ----
def packed(shape, maker=P.lsi_problem):
    key = ("packed", shape, maker.__name__)
    if key not in _cache:
        _cache[key] = lexlsi.pack_batch(SHAPES[shape]["n"], problems(shape, maker))
    return _cache[key]


def upload(pk, start=None, data=None, var_index=None):
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(device())
    var = pk.var_index if var_index is None else var_index
    guess, x0, v0 = start if start is not None else (None, None, None)
    return dict(data=up((pk.data if data is None else data).reshape(pk.batch, -1), np.float64), var_index=None if var is None else up(var.reshape(pk.batch, -1).view(np.int32), np.int32),
                active_guess=up(guess, np.uint8), x0=up(x0, np.float64), v0=up(v0, np.float64))


def new_batch(pk, counts=None, log=False):
    """-> the batch object and the counts tensor it holds (None: the setting is off)"""
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    if log:
        b.set_working_set_log(CAPACITY)
    ct = None
    if counts is not None:
        ct = torch.from_numpy(np.ascontiguousarray(counts, np.uint32).view(np.int32)).to(device())
        b.set_instance_obj_dims(ct)
    return b, ct


def assert_equals_oracle(got, refs, what, lam=True, only=None):
    for b, o in enumerate(refs):
        if only is not None and not only[b]:
            continue
        np.testing.assert_array_equal(got["info"][b], o["info"], err_msg=f"{what}: info of instance {b}")
        np.testing.assert_array_equal(got["x"][b].view(np.uint64), o["x"].view(np.uint64), err_msg=f"{what}: x of instance {b}")
        np.testing.assert_array_equal(got["active"][b], o["active"], err_msg=f"{what}: active of instance {b}")
        np.testing.assert_array_equal(got["v"][b].view(np.uint64), o["v"].view(np.uint64), err_msg=f"{what}: v of instance {b}")
        if "log" in o:
            assert int(got["cycling_counters"][b]) == sum(1 for e in o["log"] if e["cycling_detected"]), (what, b)
        if lam:
            np.testing.assert_array_equal(got["lambda"][b].view(np.uint64), o["lambda"].view(np.uint64), err_msg=f"{what}: multipliers of instance {b}")


def absent(dims, counts):
    """batch x total: the row is absent"""
    out = np.zeros((len(counts), int(np.sum(dims))), bool)
    for i, cnt in enumerate(counts):
        for f, d, c in zip(firsts(dims), dims, cnt):
            out[i, f + int(c):f + d] = True
    return out


def assert_absent_rows_zero(got, dims, counts, lam, what):
    gone = absent(dims, counts)
    assert not rows(got["active"])[gone].any() and not got["v"].view(np.uint64)[gone].any(), f"{what}: an absent row of active / v is not 0"
    if lam:
        assert not got["lambda"].view(np.uint64)[np.repeat(gone[:, None, :], len(dims), axis=1)].any(), f"{what}: an absent row of lambda is not 0"


def assert_log(b, refs, dims, counts, what):
    log, alpha, cnt = b.working_set_log_arrays()
    assert sum(len(o["log"]) for o in refs) > 0 and max(len(o["log"]) for o in refs) <= CAPACITY
    np.testing.assert_array_equal(cnt, np.array([len(o["log"]) for o in refs], np.uint32), err_msg=what)
    for i, o in enumerate(refs):
        want = np.array([[e[k] for k in capi.WORKING_SET_LOG_FIELDS] for e in o["log"]], np.int32).reshape(len(o["log"]), len(capi.WORKING_SET_LOG_FIELDS))
        np.testing.assert_array_equal(log[i, :len(want)], want, err_msg=f"{what}: instance {i}")
        # (values, as tests/test_gpu_lsi_working_set_log.py compares them: a step of length zero is -0.0 in the batch's log and in the oracle's, +0.0 in
        # the single-problem driver's, with or without per-instance counts)
        np.testing.assert_array_equal(alpha[i, :len(want)], np.array([e["alpha_or_lambda"] for e in o["log"]]), err_msg=f"{what}: instance {i}")
        assert not log[i, len(want):].any() and not alpha[i, len(want):].any(), (what, i)
        assert all(e[1] < counts[i][e[0]] for e in want), f"{what}: the log of instance {i} names an absent row"


def ragged_run(entry, shape, counts, what, lam=True, log=False, start=None, kernel=None, maker=P.lsi_problem, prepare=None, regularization_factors=None, **kw):
    """the preconditions, then one run with `counts` on a fresh batch object against the per-instance oracle -> host copies of the outputs"""
    okw = dict(kw) if regularization_factors is None else dict(kw, regularization_factors=regularization_factors)
    refs = oracle_refs(shape, counts, start=start, debug=lam or log, maker=maker, **okw)
    require(shape, counts, refs, start=start, maker=maker, **okw)
    pk = packed(shape, maker)
    b, _ = new_batch(pk, counts, log=log)
    try:
        if prepare:
            prepare(b)
        out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
        assert solve(entry, b, upload(pk, start), out, lam=lam, status=status, regularization_factors=regularization_factors, **kw) == 0, (what, capi.lib().lexls_last_error())
        if entry == "enqueue":
            assert int(status.item()) == -1, what
        got = host(out)
        assert b.last_kernel().startswith(KERNEL[shape] if kernel is None else kernel), (what, b.last_kernel())
        assert_equals_oracle(got, refs, what, lam=lam)
        assert_absent_rows_zero(got, SHAPES[shape]["dims"], counts, lam, what)
        if lam:
            np.testing.assert_array_equal(rows(b.lambda_array()), rows(got["lambda"]), err_msg=f"{what}: get_lambda")
        if log:
            assert_log(b, refs, SHAPES[shape]["dims"], counts, what)
        return got
    finally:
        b.close()


# ---- 1: the persistent launch, every shape, both entries ----
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["small", "ik", "wide", "bounds"])
def test_persistent_launch(hip, shape, entry):
    counts = counts_of(shape)
    if shape == "bounds":
        assert len(set(counts[:, 0].tolist())) > 1, "the simple-bounds objective has one count"
    ragged_run(entry, shape, counts, f"{shape}, {entry}", log=True)


# ---- 2: the lock-step stages and two groups ----
@pytest.mark.parametrize("shape", ["small", "bounds"])
def test_stage_path(hip, monkeypatch, shape):
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    pk = packed(shape)
    counts = counts_of(shape)
    refs = oracle_refs(shape, counts, debug=True)
    require(shape, counts, refs)
    b, _ = new_batch(pk, counts, log=True)
    try:
        out = sentinel_outputs(pk)
        assert solve("sync", b, upload(pk), out) == 0, capi.lib().lexls_last_error()
        assert not b.last_kernel().startswith("lsi_fused<") and b.last_kernel() not in ("host", ""), b.last_kernel()
        assert_equals_oracle(host(out), refs, f"{shape}, stages")
        assert_absent_rows_zero(host(out), SHAPES[shape]["dims"], counts, True, f"{shape}, stages")
        assert_log(b, refs, SHAPES[shape]["dims"], counts, f"{shape}, stages")
    finally:
        b.close()


def test_two_groups(hip, monkeypatch):
    """the group whose first instance is lo reads the counts from row lo"""
    monkeypatch.setenv("LEXLS_LSI_GROUPS", "2")  # (read when a batch object is made)
    pk = packed("bounds")
    counts = counts_of("bounds")
    assert not np.array_equal(counts[:pk.batch // 2], counts[pk.batch // 2:])
    refs = oracle_refs("bounds", counts, debug=True)
    require("bounds", counts, refs)
    b, _ = new_batch(pk, counts)
    try:
        out = sentinel_outputs(pk)
        assert solve("sync", b, upload(pk), out) == 0, capi.lib().lexls_last_error()
        assert b.stats()["groups"] == 2
        assert_equals_oracle(host(out), refs, "two groups")
    finally:
        b.close()


# ---- 3: a captured step picks up rewritten counts on replay ----
def child_capture():
    """an uncaptured enqueue + finish, a captured one, two replays with the counts rewritten in place by a torch op in between: each replay equals the
    oracle under the counts present at that replay.  A replay that reports a fault ends the test: nothing else is started"""
    pk = packed("bounds")
    t = upload(pk)  # (torch opens the device first)
    first, second, third = counts_of("bounds"), counts_of("bounds", 1), counts_of("bounds", 2)
    for c in (first, second, third):
        require("bounds", c, oracle_refs("bounds", c, debug=True))
    assert any(not np.array_equal(a["x"], b["x"]) for a, b in zip(oracle_refs("bounds", second, debug=True), oracle_refs("bounds", third, debug=True)))
    b, ct = new_batch(pk, first)
    stream = torch.cuda.Stream(device())
    out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
    kw = dict(with_cycling_counters=True, with_lambda=True, status=status, out=out)
    with torch.cuda.stream(stream):
        b.enqueue_device(t["data"], t["var_index"], **kw)  # the uncaptured run that may allocate
    b.finish()
    assert_equals_oracle(host(out), oracle_refs("bounds", first, debug=True), "uncaptured")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        b.enqueue_device(t["data"], t["var_index"], **kw)
    for turn, counts in enumerate((second, third)):
        new = torch.from_numpy(counts.view(np.int32)).to(device())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for a in out.values():
                a.fill_(SENTINEL)
            ct.copy_(new)  # a torch op on the tensor the library holds
            graph.replay()
        b.finish(stream)  # (raises on a fault: the test ends here)
        assert int(status.item()) == -1, turn
        assert_equals_oracle(host(out), oracle_refs("bounds", counts, debug=True), f"replay {turn}")
        assert_absent_rows_zero(host(out), SHAPES["bounds"]["dims"], counts, True, f"replay {turn}")
        np.testing.assert_array_equal(rows(b.lambda_array()), rows(host(out)["lambda"]))
    b.close()


def test_captured_step(hip):
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_instance_obj_dims as m; m.child_capture()"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]


# ---- 4: options ----
def warm_start(shape, counts, with_v0):
    """active / x / v of the oracle's solutions of the truncated problems, in capacity layout"""
    sol = oracle_refs(shape, counts)
    return (np.stack([o["active"] for o in sol]), np.stack([o["x"] for o in sol]), np.stack([o["v"] for o in sol]) if with_v0 else None)


def neighbours(seed, n, dims, simple_bounds=True):
    return P.lsi_problem(seed, n, dims, simple_bounds=simple_bounds, perturb=1.0, perturb_seed=1)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("with_v0", [False, True])
def test_warm_start(hip, entry, with_v0):
    """the neighbours of the bounds problems, started from active / x (/ v) of the base problems' solutions under the same counts"""
    counts = counts_of("bounds")
    ragged_run(entry, "bounds", counts, f"{entry}: warm start, v0 {with_v0}", start=warm_start("bounds", counts, with_v0), maker=neighbours)


@pytest.mark.parametrize("entry", ENTRIES)
def test_deactivate_first_wrong_sign(hip, entry):
    ragged_run(entry, "bounds", counts_of("bounds"), f"{entry}: deactivate_first_wrong_sign", log=True, deactivate_first_wrong_sign=1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_cycling_handling(hip, entry):
    """the degenerate batch of tests/test_gpu_lsi_cycling_resident.py's kind with objective 2 truncated in every second instance"""
    counts = full("bounds")
    counts[1::2, 2] -= 2
    counts[1::4, 3] -= 1
    got = ragged_run(entry, "bounds", counts, f"{entry}: cycling handling", lam=False, log=True, maker=degenerate, **CAP3)
    assert got["cycling_counters"].view(np.uint32).sum() > 0, "no instance relaxes a bound: the case shows nothing of cycling handling"


FACTORS = [0.0, 0.02, 0.05, 0.03]  # bounds shape: one per objective


@pytest.mark.parametrize("entry", ENTRIES)
def test_regularized_with_device_factors(hip, entry):
    """TIKHONOV with per-instance factors in device memory: every row holds FACTORS, so the oracle's run with shared factors is the reference"""
    pk = packed("bounds")
    factors = torch.from_numpy(np.ascontiguousarray(np.tile(FACTORS, (pk.batch, 1)))).to(device())
    counts = counts_of("bounds")
    refs = oracle_refs("bounds", counts, regularization_type=1, regularization_factors=FACTORS)
    require("bounds", counts, refs, regularization_type=1, regularization_factors=FACTORS)
    b, _ = new_batch(pk, counts)
    try:
        b.set_instance_regularization(factors)
        out = sentinel_outputs(pk)
        assert solve(entry, b, upload(pk), out, lam=False, regularization_type=1) == 0, capi.lib().lexls_last_error()
        assert "regularized" in b.last_kernel(), b.last_kernel()
        assert_equals_oracle(host(out), refs, f"{entry}: TIKHONOV", lam=False)
        assert_absent_rows_zero(host(out), SHAPES["bounds"]["dims"], counts, False, f"{entry}: TIKHONOV")
    finally:
        b.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_with_a_mask(hip, entry):
    """a skipped instance's counts are not read: its row holds 0xffffffff, the run is good and its outputs keep the sentinel"""
    pk = packed("bounds")
    counts = counts_of("bounds")
    refs = oracle_refs("bounds", counts, debug=True)
    require("bounds", counts, refs)
    mask = np.ones(pk.batch, np.uint8)
    mask[[2, 5]] = 0
    garbage = counts.copy()
    garbage[mask == 0] = 0xffffffff
    b, _ = new_batch(pk, garbage)
    try:
        b.set_instance_mask(torch.from_numpy(mask).to(device()))
        out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
        assert solve(entry, b, upload(pk), out, status=status) == 0, capi.lib().lexls_last_error()
        got = host(out)
        for k, a in got.items():
            assert (a[mask == 0] == SENTINEL).all(), f"{entry}: {k} of a skipped instance was written"
        assert_equals_oracle(got, refs, f"{entry}: with a mask", only=mask != 0)
    finally:
        b.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_with_a_budget(hip, entry):
    """a budget of 2 for the odd instances, none (0) for the even ones: with 2 for everyone the oracle never gets as far as a REMOVE"""
    pk = packed("bounds")
    counts = counts_of("bounds")
    limits = np.where(np.arange(pk.batch) % 2 == 1, 2, 0).astype(np.int32)
    mixed = lambda c: [two if L == 2 else free for L, two, free in zip(limits, oracle_refs("bounds", c, debug=True, max_number_of_factorizations=2), oracle_refs("bounds", c, debug=True))]
    refs = mixed(counts)
    require("bounds", counts, refs, cap=mixed(full("bounds")))
    assert any(r["info"][0] == 2 for r in refs), "no instance ends on the budget"
    b, _ = new_batch(pk, counts)
    try:
        b.set_instance_max_factorizations(torch.from_numpy(limits).to(device()))
        out = sentinel_outputs(pk)
        assert solve(entry, b, upload(pk), out) == 0, capi.lib().lexls_last_error()
        assert_equals_oracle(host(out), refs, f"{entry}: budget 2")
    finally:
        b.close()


# ---- 5: absent rows are not interpreted; clearing the setting; counts at capacity ----
def poisoned(pk, counts):
    """NaN in the data and bounds of every absent row, nVar + 5 in the absent variable indices -> (data, var_index)"""
    data = pk.data.reshape(pk.batch, -1).copy()
    var = None if pk.var_index is None else pk.var_index.reshape(pk.batch, -1).copy()
    for i in range(pk.batch):
        off = 0
        for k, (d, simple) in enumerate(zip(pk.dims, pk.types)):
            cols = 2 if simple else pk.nvar + 2
            blk = data[i, off:off + d * cols].reshape(cols, d)  # column-major, leading dimension d
            blk[:, int(counts[i, k]):] = np.nan
            off += d * cols
        if var is not None:
            var[i, int(counts[i, 0]):] = pk.nvar + 5
    return data, var


@pytest.mark.parametrize("entry", ENTRIES)
def test_absent_rows_are_not_interpreted(hip, entry):
    pk = packed("bounds", neighbours)
    counts = counts_of("bounds")
    start = warm_start("bounds", counts, True)
    refs = oracle_refs("bounds", counts, start=start, debug=True, maker=neighbours)
    require("bounds", counts, refs, start=start, maker=neighbours)
    gone = absent(SHAPES["bounds"]["dims"], counts)
    assert gone.any()
    data, var = poisoned(pk, counts)
    assert np.isnan(data).any() and (var >= pk.nvar).any()
    guess, x0, v0 = (a.copy() for a in start)
    guess[gone], v0[gone] = 9, np.nan  # (a flag of 9 in a present row is fault code 4)
    b, _ = new_batch(pk, counts, log=True)
    try:
        clean, dirty = sentinel_outputs(pk), sentinel_outputs(pk)
        assert solve(entry, b, upload(pk, start), clean) == 0, capi.lib().lexls_last_error()
        assert solve(entry, b, upload(pk, (guess, x0, v0), data=data, var_index=var), dirty) == 0, capi.lib().lexls_last_error()
        got = host(dirty)
        for k, a in host(clean).items():
            np.testing.assert_array_equal(rows(got[k]), rows(a), err_msg=f"{entry}: {k} changes with what the absent rows hold")
        assert_equals_oracle(got, refs, f"{entry}: poisoned absent rows")
        assert_absent_rows_zero(got, SHAPES["bounds"]["dims"], counts, True, f"{entry}: poisoned absent rows")
        assert_log(b, refs, SHAPES["bounds"]["dims"], counts, f"{entry}: poisoned absent rows")
    finally:
        b.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_none_clears_and_capacity_counts_change_nothing(hip, entry):
    pk = packed("bounds")
    t = upload(pk)
    fresh, _ = new_batch(pk)
    b, ct = new_batch(pk, counts_of("bounds"))
    try:
        want, ragged, at_capacity, cleared = (sentinel_outputs(pk) for _ in range(4))
        assert solve(entry, fresh, t, want) == 0 and solve(entry, b, t, ragged) == 0
        assert not np.array_equal(host(want)["x"], host(ragged)["x"]), "the counts changed nothing: clearing them shows nothing"
        ct.copy_(torch.from_numpy(full("bounds").view(np.int32)).to(device()))
        assert solve(entry, b, t, at_capacity) == 0
        b.set_instance_obj_dims(None)
        assert solve(entry, b, t, cleared) == 0
        for k, a in host(want).items():
            np.testing.assert_array_equal(rows(host(at_capacity)[k]), rows(a), err_msg=f"{entry}: {k} with every count at capacity")
            np.testing.assert_array_equal(rows(host(cleared)[k]), rows(a), err_msg=f"{entry}: {k} after the setting was cleared")
        assert b.last_kernel() == fresh.last_kernel() and b.stats() == fresh.stats()
        np.testing.assert_array_equal(rows(b.lambda_array()), rows(fresh.lambda_array()))
    finally:
        b.close()
        fresh.close()


# ---- 6: errors ----
@pytest.mark.parametrize("entry", ENTRIES)
def test_count_above_capacity(hip, entry):
    pk = packed("bounds")
    counts = counts_of("bounds")
    counts[3, 1] = SHAPES["bounds"]["dims"][1] + 1
    b, ct = new_batch(pk, counts)
    try:
        out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
        assert solve(entry, b, upload(pk), out, status=status) == LEXLS_ERR_INVALID
        assert "instance 3:" in capi.lib().lexls_last_error().decode() and "capacity" in capi.lib().lexls_last_error().decode(), capi.lib().lexls_last_error()
        if entry == "enqueue":
            assert int(status.item()) == 3 * 8 + 5
        assert all((a == SENTINEL).all() for a in host(out).values()), "an output was written"
        # a good run on the same object afterwards
        good = counts_of("bounds")
        ct.copy_(torch.from_numpy(good.view(np.int32)).to(device()))
        assert solve(entry, b, upload(pk), out) == 0, capi.lib().lexls_last_error()
        assert_equals_oracle(host(out), oracle_refs("bounds", good, debug=True), f"{entry}: a good run after the faulty one")
    finally:
        b.close()


def test_run_is_refused(hip):
    pk = packed("bounds")
    b, _ = new_batch(pk, counts_of("bounds"))
    try:
        with pytest.raises(capi.LexlsError) as e:
            b.run(pk)
        assert str(e.value).startswith(f"liblexls_hip error {LEXLS_ERR_UNSUPPORTED}:") and "obj_dims" in str(e.value), str(e.value)
        x, info = np.full((pk.batch, pk.nvar), 7.0), np.full((pk.batch, 6), 7, np.int32)
        active, v, rounds = np.full((pk.batch, pk.total), 7, np.uint8), np.full((pk.batch, pk.total), 7.0), np.full(2, 7, np.int32)
        par = lexlsi.pack_params()
        p = lambda a, c: a.ctypes.data_as(C.POINTER(c))
        rc = capi.lib().lexls_lsi_batch_run(b._h, p(pk.data, C.c_double), p(pk.var_index, C.c_uint32), None, None, None, None, p(par, C.c_double), C.c_uint32(len(par)),
                                            p(x, C.c_double), p(info, C.c_int32), p(active, C.c_uint8), p(v, C.c_double), p(rounds, C.c_int32))
        assert rc == LEXLS_ERR_UNSUPPORTED and "obj_dims" in capi.lib().lexls_last_error().decode()
        assert all((a == 7).all() for a in (x, info, active, v, rounds)), "a refused run wrote an output"
    finally:
        b.close()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["small", "bounds"])
def test_count_zero_is_an_empty_objective(hip, shape, entry):
    """the oracle-backed driver solves a problem with an objective of no rows, so a count of 0 is served with its results: every objective is empty
    in one instance or another, the simple-bounds objective among them.  The single-problem driver (lexls_lsi_solve_debug) solves such a problem too:
    the multipliers, the working-set log and the cycling counter are compared with its own"""
    pk = packed(shape)
    counts = counts_of(shape)
    for j, i in enumerate(i for i in range(pk.batch) if i % 4):  # (every fourth instance stays at full capacity)
        counts[i, j % len(pk.dims)] = 0
    assert all((counts[:, k] == 0).any() for k in range(len(pk.dims)))
    refs = oracle_refs(shape, counts, debug=True)
    require(shape, counts, refs)
    b, _ = new_batch(pk, counts, log=True)
    try:
        out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
        assert solve(entry, b, upload(pk), out, status=status) == 0, capi.lib().lexls_last_error()
        if entry == "enqueue":
            assert int(status.item()) == -1
        got = host(out)
        assert_equals_oracle(got, refs, f"{shape}, {entry}: empty objectives")
        assert_absent_rows_zero(got, SHAPES[shape]["dims"], counts, True, f"{shape}, {entry}: empty objectives")
        np.testing.assert_array_equal(rows(b.lambda_array()), rows(got["lambda"]), err_msg=f"{shape}, {entry}: get_lambda")
        assert_log(b, refs, SHAPES[shape]["dims"], counts, f"{shape}, {entry}: empty objectives")
    finally:
        b.close()
