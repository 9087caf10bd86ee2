"""lexls_lsi_batch_run_device_ex (LsiBatch.run_device with v0 / with_lambda / with_cycling_counters): the full warm start of the reference —
working set, x0 and v0 — and the multipliers and relaxation counters of a run, all in device memory, so that a loop "solve, perturb on the
device, solve again from the previous answer" never touches the host.  The tolerance is zero, as for every LexLSI path: x, info, the final
working set, v, the multipliers and the counters are compared with assert_array_equal against LsiBatch.run on host arrays (default path and
LEXLS_LSI_NO_FUSED=1), against the oracle-backed driver, and against lexls_lsi_solve_debug for the multipliers.

Inputs are warm-start chains: P.lsi_problem(seed) is solved with run, the neighbour P.lsi_problem(seed, perturb=PERTURB[...], perturb_seed=1) is
solved from active / x / v of that answer.  With v0 given, phase 1 takes v as it stands instead of deriving it from A x0 and the new bounds
(objective.h:226-236), which changes the rounding of later v updates and sometimes the trajectory.  Every test on v0 first asserts, from the
oracle-backed driver's results alone, that in at least a quarter of its instances the run with v0 differs (info or final v) from the run with
the same guess and x0 but without v0 — otherwise a dead v0 branch would pass.  PERTURB and the seeds were picked on the CPU with the oracle so
that this holds with a margin: PERTURB = 1.0, perturb_seed = 1 gave 16 / 40 (bounds), 18 / 40 (general), 9 / 12 (ik), 9 / 12 (wide); the
degenerate (cycling) chain needs PERTURB = 10.0 for 17 / 40 (1.0: 8 / 40), and 39 of its 40 instances still relax a bound.

Shapes: n = 14, (4, 5, 5, 4) with simple bounds and n = 10, 3 x 6 general only (lsi_fused<lqr_wave<41,12,...>>, 40 instances = 10 workgroups);
n = 40, 5 x 12 with simple bounds (the 41 x 12 instantiation at its full width, 12 instances); n = 50, (8, 16, 16, 12) (the 64 x 16
instantiation, 12 instances)."""
import ctypes as C

import numpy as np
import pytest

from lexls_amd import capi, lexlsi, problems as P

pytestmark = pytest.mark.gpu

SHAPES = {
    "bounds": dict(n=14, dims=[4, 5, 5, 4], simple_bounds=True, seeds=range(1300, 1340)),
    "general": dict(n=10, dims=[6, 6, 6], simple_bounds=False, seeds=range(10, 50)),
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True, seeds=range(100, 112)),
    "wide": dict(n=50, dims=[8, 16, 16, 12], simple_bounds=True, seeds=range(500, 512)),
}
PERTURB = {"lsi_problem": 1.0, "degenerate": 10.0}  # per problem maker (the cycling runs mostly end after three relaxations whatever v0 was: more is needed)
CAP3 = dict(tol_wrong_sign_lambda=0.0, cycling_handling_enabled=1, cycling_max_counter=3, cycling_relax_step=1e-6)
REG = dict(regularization_type=1)
REG_FACTORS = (0, 0.02, 0.05, 0.03, 0.04)  # ik shape: one per objective
LEXLS_ERR_UNSUPPORTED = 3
_cache = {}


def degenerate(seed, n, dims, simple_bounds=True, perturb=0.0, perturb_seed=0):
    """P.lsi_problem made to cycle (the construction of tests/test_gpu_lsi_cycling_resident.py): every general objective behind the first one
    repeats the first max(1, m // 2) rows of the first one (m = the smaller row count of the two) with the interval moved past its upper
    bound; the last objective holds equalities"""
    objs = P.lsi_problem(seed, n, dims, simple_bounds=simple_bounds, perturb=perturb, perturb_seed=perturb_seed)
    general = [k for k, o in enumerate(objs) if "A" in o]
    g0 = objs[general[0]]
    for k in general[1:]:
        o = objs[k]
        r = max(1, min(len(o["lb"]), len(g0["lb"])) // 2)
        o["A"][:r] = g0["A"][:r]
        o["lb"][:r] = g0["ub"][:r] + 0.5
        o["ub"][:r] = o["lb"][:r] if k == len(objs) - 1 else o["lb"][:r] + (g0["ub"][:r] - g0["lb"][:r])
    return objs


def problems_of(shape, step, maker=P.lsi_problem):
    """the batch of a chain's step: 0 the base problems, k > 0 the neighbours with perturb_seed = k"""
    key = ("problems", shape, step, maker.__name__)
    if key not in _cache:
        s = SHAPES[shape]
        _cache[key] = [maker(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"], perturb=PERTURB[maker.__name__] if step else 0.0, perturb_seed=step) for seed in s["seeds"]]
    return _cache[key]


def split(shape, a):
    return np.split(a, np.cumsum(SHAPES[shape]["dims"])[:-1])


def chain(shape, maker=P.lsi_problem, **params):
    """-> (packed neighbours, their objective lists, guess, x0, v0): step 1 of a warm-start chain, the base problems solved with run.  Computed
    once per shape and parameter set, shared, never modified"""
    key = ("chain", shape, maker.__name__, tuple(sorted(params.items())))
    if key not in _cache:
        n = SHAPES[shape]["n"]
        first = lexlsi.lsi_batch_solve(n, problems_of(shape, 0, maker), **params)
        probs = problems_of(shape, 1, maker)
        _cache[key] = (lexlsi.pack_batch(n, probs), probs, first["active"].copy(), first["x"].copy(), first["v"].copy())
    return _cache[key]


def oracle_refs(oracle, shape, probs, guess, x0, v0, **params):
    """per instance the oracle-backed driver's result, with the relaxations of its working-set log when the run handles cycling"""
    refs = []
    for i, p in enumerate(probs):
        args = dict(active_guess=None if guess is None else split(shape, guess[i]), x0=None if x0 is None else x0[i], v0=None if v0 is None else split(shape, v0[i]))
        o = oracle.lsi_run(SHAPES[shape]["n"], p, **args, **params)
        if params.get("cycling_handling_enabled"):
            o["relaxed"] = [e for e in oracle.lsi_run_debug(SHAPES[shape]["n"], p, **args, **params)["debug"]["working_set_log"] if e["cycling_detected"]]
        refs.append(o)
    return refs


def oracle_pair(oracle, shape, maker=P.lsi_problem, regularization_factors=None, **params):
    """the oracle's results of the chain's step 1 with v0 and, same guess and x0, without; the precondition of every test on v0 is checked here"""
    key = ("oracle", shape, maker.__name__, regularization_factors, tuple(sorted(params.items())))
    if key not in _cache:
        extra = {} if regularization_factors is None else dict(regularization_factors=regularization_factors)
        pk, probs, guess, x0, v0 = chain(shape, maker, **extra, **params)
        _cache[key] = (oracle_refs(oracle, shape, probs, guess, x0, v0, **extra, **params), oracle_refs(oracle, shape, probs, guess, x0, None, **extra, **params))
    with_v0, without = _cache[key]
    differ = sum(a["info"] != b["info"] or not np.array_equal(np.concatenate(a["v"]).view(np.uint64), np.concatenate(b["v"]).view(np.uint64)) for a, b in zip(with_v0, without))
    assert 4 * differ >= len(with_v0), f"{shape}: v0 changes only {differ} of {len(with_v0)} instances: the v0 branch is not exercised"
    return with_v0, without


def assert_equals_oracle(r, refs, what):
    info = r["info"].array if hasattr(r["info"], "array") else r["info"]
    for b, o in enumerate(refs):
        assert dict(zip(lexlsi.INFO_KEYS, info[b].tolist())) == o["info"], (what, b)
        np.testing.assert_array_equal(r["x"][b], o["x"], err_msg=f"{what}: x of instance {b}")
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]), err_msg=f"{what}: active of instance {b}")
        np.testing.assert_array_equal(r["v"][b].view(np.uint64), np.concatenate(o["v"]).view(np.uint64), err_msg=f"{what}: v of instance {b}")


def assert_same_bits(got, ref, what):
    """got: host copies of a run_device result; ref: the result of LsiBatch.run"""
    np.testing.assert_array_equal(got["info"], ref["info"].array, err_msg=what + ": info")
    np.testing.assert_array_equal(got["active"], ref["active"], err_msg=what + ": active")
    for k in ("x", "v"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[k]).view(np.uint64), ref[k].view(np.uint64), err_msg=what + ": " + k)


def to_device(pk, guess=None, x0=None, v0=None):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)
    return dict(data=up(pk.data, np.float64), var_index=None if pk.var_index is None else up(pk.var_index.view(np.int32), np.int32),
                active_guess=up(guess, np.uint8), x0=up(x0, np.float64), v0=up(v0, np.float64))


def to_host(r):
    return {k: a.cpu().numpy() for k, a in r.items()}


def run_device(b, t, **kw):
    return to_host(b.run_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], **kw))


def new_batch(pk):
    return lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)


def v0_four_ways(monkeypatch, oracle, shape, maker=P.lsi_problem, regularization_factors=None, **params):
    """step 1 of the chain with v0 through run (default path), run_device, and both under LEXLS_LSI_NO_FUSED=1, on one batch object: all the
    same bits and the oracle's.  -> the default run's result and kernel name"""
    refs, _ = oracle_pair(oracle, shape, maker, regularization_factors, **params)  # (precondition first: the oracle alone)
    extra = {} if regularization_factors is None else dict(regularization_factors=regularization_factors)
    pk, probs, guess, x0, v0 = chain(shape, maker, **extra, **params)
    b = new_batch(pk)
    try:
        monkeypatch.delenv("LEXLS_LSI_NO_FUSED", raising=False)
        ref = b.run(pk, active_guess=guess, x0=x0, v0=v0, **extra, **params)
        name = b.last_kernel()
        t = to_device(pk, guess, x0, v0)
        before = {k: None if a is None else a.clone() for k, a in t.items()}
        dev = run_device(b, t, **extra, **params)
        assert b.last_kernel() == name, (b.last_kernel(), name)
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
        staged = b.run(pk, active_guess=guess, x0=x0, v0=v0, **extra, **params)
        stage_kernel = b.last_kernel()
        dev_staged = run_device(b, t, **extra, **params)
        assert b.last_kernel() == stage_kernel
        assert not stage_kernel.startswith("lsi_fused<") and stage_kernel not in ("host", ""), stage_kernel
        for k, a in t.items():  # input safety: the caller's tensors, data and v0 among them, are the same bits as before
            assert a is None or bool((a.view(torch_bits(a)) == before[k].view(torch_bits(a))).all()), k
    finally:
        monkeypatch.delenv("LEXLS_LSI_NO_FUSED", raising=False)
        b.close()
    assert_equals_oracle(ref, refs, "run with v0")
    assert_same_bits(dev, ref, "run_device with v0")
    assert_same_bits(dev_staged, staged, "run_device with v0, LEXLS_LSI_NO_FUSED=1")
    assert_same_bits(dev_staged, ref, "LEXLS_LSI_NO_FUSED=1 against the default path")
    return ref, name


def torch_bits(a):
    import torch
    return torch.int64 if a.dtype == torch.float64 else a.dtype


@pytest.mark.parametrize("shape", ["bounds", "general", "ik", "wide"])
def test_v0(hip, oracle, monkeypatch, shape):
    ref, name = v0_four_ways(monkeypatch, oracle, shape)
    assert name.startswith("lsi_fused<"), name  # every shape here has a persistent launch


def test_v0_without_x0_is_disregarded(hip, oracle):
    pk, probs, guess, x0, v0 = chain("bounds")
    refs = oracle_refs(oracle, "bounds", probs, guess, None, None)
    b = new_batch(pk)
    try:
        plain = b.run(pk, active_guess=guess)
        got = run_device(b, to_device(pk, guess, None, v0))
        without = run_device(b, to_device(pk, guess))
    finally:
        b.close()
    assert_equals_oracle(plain, refs, "run without x0")
    assert_same_bits(got, plain, "run_device with v0 but no x0")
    assert_same_bits(without, plain, "run_device without v0")


def test_v0_with_deactivate_first_wrong_sign(hip, oracle, monkeypatch):
    ref, name = v0_four_ways(monkeypatch, oracle, "general", deactivate_first_wrong_sign=1)
    assert sum(i["deactivations"] for i in ref["info"]) > 0, "nothing is ever removed: the rule is not exercised"


def test_v0_with_cycling_handling(hip, oracle, monkeypatch):
    refs, _ = oracle_pair(oracle, "bounds", degenerate, **CAP3)
    assert sum(len(o["relaxed"]) > 0 for o in refs) >= 30
    ref, name = v0_four_ways(monkeypatch, oracle, "bounds", degenerate, **CAP3)
    assert name.startswith("lsi_fused<"), name


def test_v0_with_a_regularized_run(hip, oracle, monkeypatch):
    ref, name = v0_four_ways(monkeypatch, oracle, "ik", regularization_factors=REG_FACTORS, **REG)
    assert name.startswith("lsi_fused<") and "regularized" in name, name


def debug_lambdas(shape, probs, guess, x0, v0):
    """lexls_lsi_solve_debug's `lambda` of every instance as one (batch, nObj, total) array"""
    n = SHAPES[shape]["n"]
    return np.stack([np.vstack(lexlsi.lsi_solve_debug(n, p, active_guess=split(shape, guess[i]), x0=x0[i], v0=None if v0 is None else split(shape, v0[i]))["debug"]["lambda"]).T
                     for i, p in enumerate(probs)])


@pytest.mark.parametrize("with_v0", [True, False], ids=["v0", "no_v0"])
@pytest.mark.parametrize("shape", ["bounds", "general"])
def test_lambda(hip, shape, with_v0):
    pk, probs, guess, x0, v0 = chain(shape)
    v0 = v0 if with_v0 else None
    b = new_batch(pk)
    try:
        r = run_device(b, to_device(pk, guess, x0, v0), with_lambda=True)
        after = b.lambda_array()  # a later get_lambda still answers, with the same bits
        host = b.run(pk, active_guess=guess, x0=x0, v0=v0)
        host_lambda = b.lambda_array()
    finally:
        b.close()
    assert r["lambda"].shape == (pk.batch, len(pk.dims), pk.total) and np.any(r["lambda"])
    np.testing.assert_array_equal(r["lambda"].view(np.uint64), after.view(np.uint64))
    np.testing.assert_array_equal(r["lambda"].view(np.uint64), host_lambda.view(np.uint64))
    np.testing.assert_array_equal(r["lambda"], debug_lambdas(shape, probs, guess, x0, v0))
    assert_same_bits(r, host, "run_device with lambda")


def call_ex(b, t, out, par, factors=None):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rfa = None if factors is None else np.ascontiguousarray(factors, np.float64)
    return capi.lib().lexls_lsi_batch_run_device_ex(
        b._h, ptr(t["data"]), ptr(t["var_index"]), ptr(t["active_guess"]), ptr(t["x0"]), ptr(t["v0"]), None if rfa is None else rfa.ctypes.data_as(C.POINTER(C.c_double)),
        par.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(par)), ptr(out["x"]), ptr(out["info"]), ptr(out["active"]), ptr(out["v"]), ptr(out.get("lambda")),
        ptr(out.get("counts")))


def sentinel_outputs(pk, with_lambda=True, with_counts=True):
    import torch
    dev = torch.device("cuda", 0)
    out = dict(x=torch.full((pk.batch, pk.nvar), 7.0, dtype=torch.float64, device=dev), info=torch.full((pk.batch, 6), 7, dtype=torch.int32, device=dev),
               active=torch.full((pk.batch, pk.total), 7, dtype=torch.uint8, device=dev), v=torch.full((pk.batch, pk.total), 7.0, dtype=torch.float64, device=dev))
    if with_lambda:
        out["lambda"] = torch.full((pk.batch, len(pk.dims), pk.total), 7.0, dtype=torch.float64, device=dev)
    if with_counts:
        out["counts"] = torch.full((pk.batch,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return out


def test_lambda_is_refused_for_cycling_and_regularized_runs(hip):
    """LEXLS_ERR_UNSUPPORTED before any device work: every output still holds its sentinel; the same runs without d_lambda are served"""
    import torch
    pk, probs, guess, x0, v0 = chain("ik")
    t = to_device(pk, guess, x0, v0)
    b = new_batch(pk)
    try:
        for par, factors in ((lexlsi.pack_params(**CAP3), None), (lexlsi.pack_params_ex(**REG), REG_FACTORS)):
            out = sentinel_outputs(pk)
            assert call_ex(b, t, out, par, factors) == LEXLS_ERR_UNSUPPORTED
            assert "d_lambda" in capi.lib().lexls_last_error().decode()
            torch.cuda.synchronize()
            assert all(bool((a == 7).all()) for a in out.values())
            out = sentinel_outputs(pk, with_lambda=False)
            assert call_ex(b, t, out, par, factors) == 0
            torch.cuda.synchronize()
            assert not any(bool((a == 7).all()) for a in out.values())
        with pytest.raises(capi.LexlsError):
            b.run_device(t["data"], t["var_index"], with_lambda=True, **CAP3)
    finally:
        b.close()


def test_cycling_counters(hip, oracle):
    s = SHAPES["bounds"]
    probs = problems_of("bounds", 0, degenerate)
    refs = oracle_refs(oracle, "bounds", probs, None, None, None, **CAP3)
    counts = np.array([len(o["relaxed"]) for o in refs], np.uint32)
    assert (counts > 0).sum() >= 30, "fewer than 30 of the 40 instances relax a bound"
    pk = lexlsi.pack_batch(s["n"], probs)
    b = new_batch(pk)
    try:
        r = run_device(b, to_device(pk), with_cycling_counters=True, **CAP3)
        assert r["cycling_counters"].dtype == np.int32 and r["cycling_counters"].shape == (pk.batch,)
        np.testing.assert_array_equal(r["cycling_counters"].view(np.uint32), b.cycling_counters())
        np.testing.assert_array_equal(r["cycling_counters"].view(np.uint32), counts)
        assert_equals_oracle(r, refs, "cycling run")
        import torch
        t = to_device(pk)
        out = sentinel_outputs(pk)  # a plain run on the same object: the counters are written, as zeros
        assert call_ex(b, t, out, lexlsi.pack_params()) == 0
        torch.cuda.synchronize()
        assert bool((out["counts"] == 0).all())
        np.testing.assert_array_equal(b.cycling_counters(), np.zeros(pk.batch, np.uint32))
        np.testing.assert_array_equal(out["lambda"].cpu().numpy().view(np.uint64), b.lambda_array().view(np.uint64))
    finally:
        b.close()


@pytest.mark.parametrize("shape", ["bounds", "general"])
def test_all_null_is_the_old_entry_point(hip, shape):
    import torch
    pk, probs, guess, x0, v0 = chain(shape)
    t = to_device(pk, guess, x0)
    b = new_batch(pk)
    try:
        old = to_host(b.run_device(t["data"], t["var_index"], t["active_guess"], t["x0"]))
        old_after = (b.last_kernel(), b.stats(), b.lambda_array(), b.cycling_counters())
        out = sentinel_outputs(pk, with_lambda=False, with_counts=False)
        assert call_ex(b, t, out, lexlsi.pack_params()) == 0
        torch.cuda.synchronize()
        new_after = (b.last_kernel(), b.stats(), b.lambda_array(), b.cycling_counters())
    finally:
        b.close()
    for k in ("x", "info", "active", "v"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), old[k], err_msg=k)
    assert new_after[:2] == old_after[:2]
    np.testing.assert_array_equal(new_after[2].view(np.uint64), old_after[2].view(np.uint64))
    np.testing.assert_array_equal(new_after[3], old_after[3])


def test_closed_loop(hip):
    """three steps on the device, each fed active / x / v of the one before as device tensors, against the same loop through run with host arrays"""
    n = SHAPES["bounds"]["n"]
    base = lexlsi.pack_batch(n, problems_of("bounds", 0))
    b, h = new_batch(base), new_batch(base)
    try:
        host = h.run(base)
        t = to_device(base)
        dev = b.run_device(t["data"], t["var_index"])
        assert_same_bits(to_host(dev), host, "cold step")
        for step in (1, 2, 3):
            pk = lexlsi.pack_batch(n, problems_of("bounds", step))
            host = h.run(pk, active_guess=host["active"], x0=host["x"], v0=host["v"])
            host_lambda = h.lambda_array()
            t = to_device(pk)  # (the perturbed data; everything else of the warm start is the previous step's device output)
            dev = b.run_device(t["data"], t["var_index"], active_guess=dev["active"], x0=dev["x"], v0=dev["v"], with_lambda=True, with_cycling_counters=True)
            assert_same_bits(to_host(dev), host, f"step {step}")
            np.testing.assert_array_equal(dev["lambda"].cpu().numpy().view(np.uint64), host_lambda.view(np.uint64), err_msg=f"step {step}: lambda")
            assert not bool(dev["cycling_counters"].any())
    finally:
        b.close()
        h.close()
