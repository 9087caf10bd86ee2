"""LexLSI batches whose phase 1 is device work: LsiBatch.run_device (lexls_lsi_batch_run_device: inputs and outputs in device memory) and
LsiBatch.run under LEXLS_LSI_DEVICE_PHASE1=1.  The yardstick is LsiBatch.run on the same numpy inputs in its default mode (phase 1 on the host over
LexLSI objects), which the earlier tests hold to the oracle-backed driver: x, v (compared as uint64), info and the final working set must be the
same bits, the kernel name, the multipliers and the cycling counters the same.  The tolerance is zero, as for every LexLSI path.

Shapes: n = 40, 5 x 12 with simple bounds (lsi_fused<lqr_wave<41,12,...>>); n = 10, (4, 6, 3), general objectives only; n = 50 with levels of 16
(the 64 x 16 instantiation).  Batches: 5 (a partial workgroup), 70 (18 workgroups, the last one partial), 9 in two groups.  Every batch holds rows
with lb == ub (the last objective, and one planted in a middle one), one of them with a zero normal, and a simple bound with lb == ub."""
import ctypes as C

import numpy as np
import pytest

from lexls_amd import capi, lexlsi, problems as P

pytestmark = pytest.mark.gpu

SHAPES = {
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True),
    "general": dict(n=10, dims=[4, 6, 3], simple_bounds=False),
    "wide": dict(n=50, dims=[8, 16, 16, 12], simple_bounds=True),
}
LEXLS_ERR_INVALID, LEXLS_ERR_UNSUPPORTED = 1, 3
CYCLING = dict(tol_wrong_sign_lambda=0.0, cycling_handling_enabled=1, cycling_max_counter=3, cycling_relax_step=1e-6)
_cache = {}


def special_rows(objs, b):
    """instance-dependent special rows: a middle row with lb == ub, one with lb == ub and a zero normal, a simple bound with lb == ub"""
    general = [k for k, o in enumerate(objs) if "A" in o]
    mid = objs[general[0]]
    if b % 3 == 1:
        mid["ub"][1] = mid["lb"][1]
    if b % 3 == 2:
        mid["A"][2, :] = 0.0
        mid["lb"][2] = mid["ub"][2] = 0.25
    if "var" in objs[0] and b % 2 == 1:
        objs[0]["lb"][3] = objs[0]["ub"][3] = 0.5
    return objs


def make(shape, batch, seed0=500, perturb=0.0):
    key = (shape, batch, seed0, perturb)
    if key not in _cache:
        s = SHAPES[shape]
        _cache[key] = [special_rows(P.lsi_problem(seed0 + b, s["n"], s["dims"], simple_bounds=s["simple_bounds"], perturb=perturb), b) for b in range(batch)]
    return _cache[key]


def degenerate(seed, n, dims, simple_bounds=True):
    """P.lsi_problem made to cycle: every general objective behind the first one repeats the first max(1, m // 2) rows of the first one
    (m = the smaller row count of the two) with the interval moved past its upper bound; the last objective holds equalities"""
    objs = P.lsi_problem(seed, n, dims, simple_bounds=simple_bounds)
    general = [k for k, o in enumerate(objs) if "A" in o]
    g0 = objs[general[0]]
    for k in general[1:]:
        o = objs[k]
        r = max(1, min(len(o["lb"]), len(g0["lb"])) // 2)
        o["A"][:r] = g0["A"][:r]
        o["lb"][:r] = g0["ub"][:r] + 0.5
        o["ub"][:r] = o["lb"][:r] if k == len(objs) - 1 else o["lb"][:r] + (g0["ub"][:r] - g0["lb"][:r])
    return objs


def to_device(pk, guess=None, x0=None):
    import torch
    dev = torch.device("cuda", 0)
    t = dict(data=torch.from_numpy(pk.data).to(dev))
    t["var_index"] = None if pk.var_index is None else torch.from_numpy(pk.var_index.view(np.int32)).to(dev)
    t["active_guess"] = None if guess is None else torch.from_numpy(np.ascontiguousarray(guess, np.uint8)).to(dev)
    t["x0"] = None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0, np.float64)).to(dev)
    return t


def to_host(r):
    return {k: r[k].cpu().numpy() for k in ("x", "info", "active", "v")}


def assert_same_bits(got, ref, what):
    """got: arrays of a device-phase-1 run; ref: the result of LsiBatch.run in its default mode"""
    info = got["info"].array if hasattr(got["info"], "array") else got["info"]
    np.testing.assert_array_equal(info, ref["info"].array, err_msg=what + ": info")
    np.testing.assert_array_equal(got["active"], ref["active"], err_msg=what + ": active")
    for k in ("x", "v"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[k]).view(np.uint64), ref[k].view(np.uint64), err_msg=what + ": " + k)


def three_ways(monkeypatch, probs, n, guess=None, x0=None, batch_object=None, **params):
    """the same inputs through run (host phase 1), run_device and run under LEXLS_LSI_DEVICE_PHASE1=1, on one batch object; -> the host
    result, the kernel name and the batch object's (lambdas or error code, cycling counters) after each of the three"""
    pk = lexlsi.pack_batch(n, probs)
    b = batch_object or lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs))
    lam = np.zeros((pk.batch, len(pk.dims), pk.total))

    def after():
        rc = capi.lib().lexls_lsi_batch_get_lambda(b._h, lam.ctypes.data_as(C.POINTER(C.c_double)))
        return b.last_kernel(), rc, lam.copy() if rc == 0 else None, b.cycling_counters(), b.stats()

    try:
        monkeypatch.delenv("LEXLS_LSI_DEVICE_PHASE1", raising=False)
        ref = b.run(pk, active_guess=guess, x0=x0, **params)
        ref_after = after()
        t = to_device(pk, guess, x0)
        before = {k: None if a is None else a.clone() for k, a in t.items()}
        dev = to_host(b.run_device(t["data"], t["var_index"], t["active_guess"], t["x0"], **params))
        dev_after = after()
        for k, a in t.items():  # the caller's arrays are never written
            assert a is None or bool((a == before[k]).all()), k
        monkeypatch.setenv("LEXLS_LSI_DEVICE_PHASE1", "1")  # (read per run)
        env = b.run(pk, active_guess=guess, x0=x0, **params)
        env_after = after()
    finally:
        monkeypatch.delenv("LEXLS_LSI_DEVICE_PHASE1", raising=False)
        if batch_object is None:
            b.close()
    assert_same_bits(dev, ref, "run_device")
    assert_same_bits(env, ref, "LEXLS_LSI_DEVICE_PHASE1=1")
    for name, a in (("run_device", dev_after), ("LEXLS_LSI_DEVICE_PHASE1=1", env_after)):
        assert a[0] == ref_after[0], (name, a[0], ref_after[0])  # the same kernel served the resident iterations
        assert a[1] == ref_after[1], (name, "get_lambda", a[1], ref_after[1])
        if ref_after[1] == 0:
            np.testing.assert_array_equal(a[2].view(np.uint64), ref_after[2].view(np.uint64), err_msg=name + ": lambda")
        np.testing.assert_array_equal(a[3], ref_after[3], err_msg=name + ": cycling counters")
        assert a[4] == ref_after[4], (name, "stats", a[4], ref_after[4])  # phase 1's stage counts like any other
    return ref, ref_after


def warm_start(shape, batch):
    """guess + x0 = the solution of a neighbour (perturbed right-hand sides): the guess names rows setData activates already and carries EQ flags"""
    key = ("warm", shape, batch)
    if key not in _cache:
        s = SHAPES[shape]
        r = lexlsi.lsi_batch_solve(s["n"], make(shape, batch, perturb=0.05))
        _cache[key] = (r["active"].copy(), r["x"].copy())
    return _cache[key]


@pytest.mark.parametrize("start", ["cold", "x0", "guess", "guess_x0"])
@pytest.mark.parametrize("shape", ["ik", "general", "wide"])
def test_starts(hip, monkeypatch, shape, start):
    s, probs = SHAPES[shape], make(shape, 5)
    guess, x0 = warm_start(shape, 5)
    assert (guess == 3).any() and ((guess == 1) | (guess == 2)).any()
    ref, after = three_ways(monkeypatch, probs, s["n"], guess=guess if "guess" in start else None, x0=x0 if "x0" in start else None)
    assert after[0].startswith("lsi_fused<"), after[0]
    assert all(i["status"] == 0 for i in ref["info"])


@pytest.mark.parametrize("start", ["cold", "guess_x0"])
def test_many_workgroups(hip, monkeypatch, start):
    probs = make("ik", 70)
    guess, x0 = warm_start("ik", 70) if start != "cold" else (None, None)
    three_ways(monkeypatch, probs, 40, guess=guess, x0=x0)


@pytest.mark.parametrize("shape", ["ik", "general"])
def test_two_groups(hip, monkeypatch, shape):
    monkeypatch.setenv("LEXLS_LSI_GROUPS", "2")  # (read when the batch object is made)
    probs = make(shape, 9)
    guess, x0 = warm_start(shape, 9)
    ref, after = three_ways(monkeypatch, probs, SHAPES[shape]["n"], guess=guess, x0=x0)
    assert after[4]["groups"] == 2
    three_ways(monkeypatch, probs, SHAPES[shape]["n"])


@pytest.mark.parametrize("shape", ["ik", "general"])
def test_stage_route(hip, monkeypatch, shape):
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    ref, after = three_ways(monkeypatch, make(shape, 5), SHAPES[shape]["n"])
    assert not after[0].startswith("lsi_fused<") and after[0] not in ("host", ""), after[0]
    guess, x0 = warm_start(shape, 5)
    three_ways(monkeypatch, make(shape, 5), SHAPES[shape]["n"], guess=guess, x0=x0)


@pytest.mark.parametrize("start", ["cold", "guess_x0"])
@pytest.mark.parametrize("shape", ["ik", "general"])
def test_deactivate_first_wrong_sign(hip, monkeypatch, shape, start):
    """cold: the first removals are decided by the stamps phase 1 handed out (the equality activations of setData, in its order)"""
    probs = make(shape, 5)
    guess, x0 = warm_start(shape, 5) if start != "cold" else (None, None)
    ref, after = three_ways(monkeypatch, probs, SHAPES[shape]["n"], guess=guess, x0=x0, deactivate_first_wrong_sign=1)
    if start == "cold":
        assert sum(i["deactivations"] for i in ref["info"]) > 0, "nothing is ever removed: the stamps are not exercised"


@pytest.mark.parametrize("shape", ["ik", "general"])
def test_cycling(hip, monkeypatch, shape):
    s = SHAPES[shape]
    seeds = range(100, 105) if shape == "ik" else [10, 11, 12, 13, 14, 117, 118, 121]
    probs = [degenerate(seed, s["n"], s["dims"], s["simple_bounds"]) for seed in seeds]
    ref, after = three_ways(monkeypatch, probs, s["n"], **CYCLING)
    assert after[3].sum() > 0, "no bound is relaxed: the batch does not exercise the cycling handler"
    assert after[1] == LEXLS_ERR_UNSUPPORTED  # get_lambda after a cycling run, on every entry (three_ways compares the codes)


def test_regularized(hip, monkeypatch):
    probs = make("ik", 5)
    guess, x0 = warm_start("ik", 5)
    factors = [0.0, 1e-3, 1e-2, 1e-1, 0.5]
    ref, after = three_ways(monkeypatch, probs, 40, regularization_factors=factors, regularization_type=1)
    assert "regularized" in after[0], after[0]
    three_ways(monkeypatch, probs, 40, guess=guess, x0=x0, regularization_factors=factors, regularization_type=1)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("start", ["cold", "guess_x0"])
def test_factorization_limit(hip, monkeypatch, limit, start):
    """1: every instance stops inside phase 1 (iteration 0); 2: in the first resident iteration"""
    probs = make("ik", 5)
    guess, x0 = warm_start("ik", 5) if start != "cold" else (None, None)
    ref, after = three_ways(monkeypatch, probs, 40, guess=guess, x0=x0, max_number_of_factorizations=limit)
    assert all(i["factorizations"] <= limit for i in ref["info"])
    assert any(i["status"] == 2 for i in ref["info"])
    if limit == 1:
        assert after[0] == "host", after[0]  # nobody's iterations were resident


def test_second_run_on_the_same_object(hip, monkeypatch):
    """a cycling run, then plain runs of other data on one batch object: nothing of the first reaches the second"""
    s = SHAPES["ik"]
    first = [degenerate(seed, s["n"], s["dims"], True) for seed in range(100, 105)]
    pk = lexlsi.pack_batch(s["n"], first)
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, 5)
    try:
        three_ways(monkeypatch, first, s["n"], batch_object=b, **CYCLING)
        ref, after = three_ways(monkeypatch, make("ik", 5, seed0=900), s["n"], batch_object=b)
        assert after[1] == 0 and after[3].sum() == 0
        fresh, _ = three_ways(monkeypatch, make("ik", 5, seed0=900), s["n"])
        assert_same_bits(ref, fresh, "after a cycling run")
    finally:
        b.close()


def _call_device(b, pk, t, out, par=None):
    par = lexlsi.pack_params() if par is None else par
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    return capi.lib().lexls_lsi_batch_run_device(b._h, ptr(t["data"]), ptr(t["var_index"]), ptr(t["active_guess"]), ptr(t["x0"]), None,
                                                 par.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(par)), ptr(out["x"]), ptr(out["info"]), ptr(out["active"]), ptr(out["v"]))


def _outputs(pk):
    import torch
    dev = torch.device("cuda", 0)
    return dict(x=torch.full((pk.batch, pk.nvar), 7.0, dtype=torch.float64, device=dev), info=torch.full((pk.batch, 6), 7, dtype=torch.int32, device=dev),
                active=torch.full((pk.batch, pk.total), 7, dtype=torch.uint8, device=dev), v=torch.full((pk.batch, pk.total), 7.0, dtype=torch.float64, device=dev))


def _untouched(out):
    return all(bool((a == 7).all()) for a in out.values())


@pytest.mark.parametrize("fault", ["lb_above_ub", "duplicate_var", "var_range", "guess_type"])
def test_input_faults(hip, monkeypatch, fault):
    """one faulty instance: LEXLS_ERR_INVALID with its index, on both entries; the batch object serves a correct run right after"""
    import torch
    probs = [[dict(o) for o in p] for p in make("ik", 5)]
    probs = [[{k: np.array(a) for k, a in o.items()} for o in p] for p in probs]
    guess = None
    if fault == "lb_above_ub":
        probs[3][2]["lb"][4] = probs[3][2]["ub"][4] + 1.0
    elif fault == "duplicate_var":
        probs[3][0]["var"][5] = probs[3][0]["var"][1]
    elif fault == "var_range":
        probs[3][0]["var"][5] = 40
    else:
        guess = np.zeros((5, 60), np.uint8)
        guess[3, 20] = 4
    pk = lexlsi.pack_batch(40, probs)
    b = lexlsi.LsiBatch(40, pk.dims, pk.types, 5)
    try:
        t, out = to_device(pk, guess), _outputs(pk)
        torch.cuda.synchronize()
        assert _call_device(b, pk, t, out) == LEXLS_ERR_INVALID
        assert "instance 3" in capi.lib().lexls_last_error().decode(), capi.lib().lexls_last_error().decode()
        monkeypatch.setenv("LEXLS_LSI_DEVICE_PHASE1", "1")
        with pytest.raises(capi.LexlsError, match="instance 3"):
            b.run(pk, active_guess=guess)
        monkeypatch.delenv("LEXLS_LSI_DEVICE_PHASE1")
        three_ways(monkeypatch, make("ik", 5), 40, batch_object=b)
    finally:
        b.close()


def test_unsupported_runs_leave_the_outputs_alone(hip, monkeypatch):
    import torch
    pk = lexlsi.pack_batch(40, make("ik", 5))
    t, out = to_device(pk), _outputs(pk)
    torch.cuda.synchronize()
    b = lexlsi.LsiBatch(40, pk.dims, pk.types, 5)
    try:
        assert _call_device(b, pk, t, out, lexlsi.pack_params_ex(regularization_type=7)) == LEXLS_ERR_UNSUPPORTED
        assert _call_device(b, pk, t, out, lexlsi.pack_params_ex(regularization_type=1, cycling_handling_enabled=1)) == LEXLS_ERR_UNSUPPORTED
    finally:
        b.close()
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    b = lexlsi.LsiBatch(40, pk.dims, pk.types, 5)
    try:
        assert _call_device(b, pk, t, out) == LEXLS_ERR_UNSUPPORTED
        with pytest.raises(capi.LexlsError):
            b.run_device(t["data"], t["var_index"])
    finally:
        b.close()
    torch.cuda.synchronize()
    assert _untouched(out)


def test_python_argument_checks(hip):
    import torch
    pk = lexlsi.pack_batch(40, make("ik", 5))
    t = to_device(pk)
    b = lexlsi.LsiBatch(40, pk.dims, pk.types, 5)
    try:
        with pytest.raises(TypeError):
            b.run_device(pk.data, t["var_index"])  # a numpy array
        with pytest.raises(TypeError):
            b.run_device(t["data"].float(), t["var_index"])
        with pytest.raises(ValueError):
            b.run_device(t["data"].cpu(), t["var_index"])
        with pytest.raises(ValueError):
            b.run_device(t["data"][:, ::2], t["var_index"])
        with pytest.raises(ValueError):
            b.run_device(t["data"])  # simple bounds without variable indices
        r = b.run_device(t["data"], t["var_index"])
        assert r["x"].is_cuda and r["x"].dtype == torch.float64 and tuple(r["info"].shape) == (5, 6)
    finally:
        b.close()
