"""The working-set log of batched LexLSI runs (lexls_lsi_batch_set_working_set_log / _get_working_set_log / _working_set_log_device,
LsiBatch.set_working_set_log / working_set_log / working_set_log_device): LexLSI::getWorkingSetLog() of every instance, written on the device
where the resident iterations change the working set and merged with what host objects logged.

The reference is the oracle-backed single-problem driver, oracle.lsi_run_debug(...)["debug"]["working_set_log"], per instance.  Every integer
field and alpha_or_lambda compare with assert_array_equal: the tolerance is zero, as on every LexLSI path.  Every test first asserts from the
oracle's logs alone that its batch holds what the test is about (ADD and REMOVE entries, an instance with three entries or more; for the cycling
tests a cycling_detected entry and an instance that ends on the relaxation limit), so that a change of the problem generator cannot empty it.

Shapes: n = 14 with simple bounds (4, 5, 5, 4), n = 10 general (6, 6, 6), n = 40 with 5 x 12 and 12 instances (the 41 x 12 EXACT instantiation)
and the 51-column shape of test_gpu_lsi_regularized_resident.py (n = 50 variables plus the right-hand side: the 64 x 16 instantiation)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime — run_device hands torch tensors to the library)

from lexls_amd import capi, lexlsi, problems as P
from test_gpu_lsi_cycling_resident import CAP3, CAP50, SHAPES as CYCLING_SHAPES, degenerate
from test_gpu_lsi_regularized_resident import SHAPES as REG_SHAPES

pytestmark = pytest.mark.gpu

FIELDS = capi.WORKING_SET_LOG_FIELDS
LEXLS_ERR_INVALID = 1
SOLVED_CYCLING = 1  # TerminationStatus PROBLEM_SOLVED_CYCLING_HANDLING
CAPACITY = 128      # entries per instance: above the longest log of every batch here (asserted where the logs are compared)
SHAPES = {
    "bounds": dict(n=14, dims=[4, 5, 5, 4], simple_bounds=True, seeds=range(1300, 1312)),
    "general": dict(n=10, dims=[6, 6, 6], simple_bounds=False, seeds=range(10, 22)),
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True, seeds=range(100, 112)),
}
_cache = {}


def make(shape):
    s = SHAPES[shape]
    return s, [P.lsi_problem(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"]) for seed in s["seeds"]]


def make_cycling(count=16):
    s = CYCLING_SHAPES["bounds"]
    return s, [degenerate(seed, s["n"], s["dims"], s["simple_bounds"]) for seed in list(s["seeds"])[:count]]


def make_wide(count=8):
    s = REG_SHAPES["wide"]
    return s, [P.lsi_problem(s["seed"] + i, s["n"], s["dims"]) for i in range(count)]


def split(flat, probs):
    return np.split(flat, np.cumsum([len(o["lb"]) for o in probs])[:-1])


def oracle_logs(oracle, key, n, probs, guesses=None, x0=None, v0=None, **run_args):
    """per instance the oracle-backed driver's result with ["log"] = its working-set log; computed once per key, shared, never modified"""
    if key not in _cache:
        refs = []
        for i, p in enumerate(probs):
            o = oracle.lsi_run_debug(n, p, active_guess=None if guesses is None else split(guesses[i], p), x0=None if x0 is None else x0[i],
                                     v0=None if v0 is None else split(v0[i], p), **run_args)
            o["log"] = o["debug"]["working_set_log"]
            refs.append(o)
        _cache[key] = refs
    return _cache[key]


def require_adds_and_removes(refs):
    """what every plain test relies on, from the oracle alone: ADD and REMOVE entries, and an instance with at least three entries"""
    entries = [e for o in refs for e in o["log"]]
    assert any(e["ctr_type"] != 0 for e in entries), "no ADD entry in the batch"
    assert any(e["ctr_type"] == 0 for e in entries), "no REMOVE entry in the batch"
    assert max(len(o["log"]) for o in refs) >= 3, "no instance with three entries"
    assert max(len(o["log"]) for o in refs) <= CAPACITY


def require_cycling(refs):
    assert any(e["cycling_detected"] for o in refs for e in o["log"]), "no cycling_detected entry in the batch"
    assert any(o["info"]["status"] == SOLVED_CYCLING for o in refs), "no instance ends on the relaxation limit"
    assert max(len(o["log"]) for o in refs) <= CAPACITY


def assert_logs_equal_oracle(arrays, refs, capacity=CAPACITY):
    """arrays = (log, alpha, counts) of the batch; the first min(count, capacity) entries are the oracle's, the rows behind are zero"""
    log, alpha, counts = arrays
    assert log.shape == (len(refs), capacity, len(FIELDS)) and alpha.shape == (len(refs), capacity)
    np.testing.assert_array_equal(counts, np.array([len(o["log"]) for o in refs], np.uint32))
    for b, o in enumerate(refs):
        kept = o["log"][:capacity]
        want = np.array([[e[k] for k in FIELDS] for e in kept], np.int32).reshape(len(kept), len(FIELDS))
        np.testing.assert_array_equal(log[b, :len(kept)], want, err_msg=f"instance {b}")
        np.testing.assert_array_equal(alpha[b, :len(kept)], np.array([e["alpha_or_lambda"] for e in kept]), err_msg=f"instance {b}")
        assert not log[b, len(kept):].any() and not alpha[b, len(kept):].any(), b


def assert_result_equals_oracle(r, refs):
    for b, o in enumerate(refs):
        assert r["info"][b] == o["info"], b
        np.testing.assert_array_equal(r["x"][b], o["x"])
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]))
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]))


def logged_run(probs, n, capacity=CAPACITY, **run_args):
    """-> result, (log, alpha, counts), kernel name of one run with the log on, on a fresh batch object"""
    pk = lexlsi.pack_batch(n, probs)
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs))
    try:
        b.set_working_set_log(capacity)
        r = b.run(pk, **run_args)
        return r, b.working_set_log_arrays(), b.last_kernel()
    finally:
        b.close()


def assert_same_arrays(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


# ---- 1: the persistent launch, cold start ----
@pytest.mark.parametrize("shape", ["bounds", "general", "ik"])
def test_persistent_launch(hip, oracle, shape):
    s, probs = make(shape)
    refs = oracle_logs(oracle, shape, s["n"], probs)
    require_adds_and_removes(refs)
    r, arrays, name = logged_run(probs, s["n"])
    assert name.startswith("lsi_fused<"), name
    if shape == "ik":
        assert name == "lsi_fused<lqr_wave<41,12,exact>>", name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


def test_python_decoder(hip, oracle):
    """LsiBatch.working_set_log(): the dicts of the oracle's debug structure, key for key"""
    s, probs = make("bounds")
    refs = oracle_logs(oracle, "bounds", s["n"], probs)
    require_adds_and_removes(refs)
    pk = lexlsi.pack_batch(s["n"], probs)
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    try:
        b.set_working_set_log(CAPACITY)
        b.run(pk)
        logs, counts = b.working_set_log()
    finally:
        b.close()
    assert logs == [o["log"] for o in refs]
    np.testing.assert_array_equal(counts, [len(o["log"]) for o in refs])


# ---- 2: the lock-step stages ----
@pytest.mark.parametrize("shape", ["bounds", "ik"])
def test_stage_route(hip, oracle, monkeypatch, shape):
    s, probs = make(shape)
    refs = oracle_logs(oracle, shape, s["n"], probs)
    require_adds_and_removes(refs)
    _, fused, name = logged_run(probs, s["n"])
    assert name.startswith("lsi_fused<"), name
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    r, staged, stage_kernel = logged_run(probs, s["n"])
    assert not stage_kernel.startswith("lsi_fused<") and stage_kernel not in ("host", ""), stage_kernel
    assert_same_arrays(staged, fused)
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(staged, refs)


# ---- 3: warm starts: iteration 0 is logged by the host object, the rest on the device ----
def warm_start(oracle, shape, perturb=0.05):
    """the batch of `shape` with perturbed right-hand sides, and the cold solution of the unperturbed one to start from"""
    s, probs = make(shape)
    cold = oracle_logs(oracle, shape, s["n"], probs)
    pert = [P.lsi_problem(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"], perturb=perturb) for seed in s["seeds"]]
    guess = np.stack([np.concatenate(o["active"]) for o in cold])
    x0 = np.stack([o["x"] for o in cold])
    v0 = np.stack([np.concatenate(o["v"]) for o in cold])
    return s, pert, guess, x0, v0


@pytest.mark.parametrize("with_v0", [False, True], ids=["x0", "x0_v0"])
def test_warm_start(hip, oracle, with_v0):
    s, pert, guess, x0, v0 = warm_start(oracle, "ik")
    refs = oracle_logs(oracle, ("ik warm", with_v0), s["n"], pert, guesses=guess, x0=x0, v0=v0 if with_v0 else None)
    require_adds_and_removes(refs)
    assert sum(len(o["log"]) >= 2 for o in refs) >= 6, "few instances log on the host (entry 0) and on the device (the entries behind)"
    r, arrays, name = logged_run(pert, s["n"], active_guess=guess, x0=x0, v0=v0 if with_v0 else None)
    assert name.startswith("lsi_fused<"), name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


def test_instances_that_stop_on_the_host(hip, oracle):
    """half of the batch starts at its solution with the final working set as the guess: those instances stop in iteration 0 on the host with an
    empty log, the others become resident — the merged log holds both"""
    s, pert, guess, x0, _ = warm_start(oracle, "bounds", perturb=1.0)
    _, plain = make("bounds")
    probs = [plain[i] if i % 2 == 0 else pert[i] for i in range(len(plain))]
    refs = oracle_logs(oracle, "bounds mixed", s["n"], probs, guesses=guess, x0=x0)
    require_adds_and_removes(refs)
    assert sum(len(o["log"]) == 0 and o["info"]["iterations"] == 1 for o in refs) >= 3, "no instance stops in iteration 0"
    r, arrays, name = logged_run(probs, s["n"], active_guess=guess, x0=x0)
    assert name.startswith("lsi_fused<"), name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


# ---- 4: phase 1 on the device ----
@pytest.mark.parametrize("shape", ["bounds", "ik"])
def test_run_device(hip, oracle, shape):
    s, probs = make(shape)
    refs = oracle_logs(oracle, shape, s["n"], probs)
    require_adds_and_removes(refs)
    _, from_run, _ = logged_run(probs, s["n"])
    pk = lexlsi.pack_batch(s["n"], probs)
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    try:
        b.set_working_set_log(CAPACITY)
        dev = torch.device("cuda", 0)
        r = b.run_device(torch.from_numpy(pk.data).to(dev), var_index=torch.from_numpy(pk.var_index.astype(np.int32)).to(dev))
        assert b.last_kernel().startswith("lsi_fused<"), b.last_kernel()
        arrays = b.working_set_log_arrays()
        d = b.working_set_log_device()
        assert all(t.is_cuda for t in d.values())
        on_device = (d["log"].cpu().numpy(), d["alpha_or_lambda"].cpu().numpy(), d["counts"].cpu().numpy().view(np.uint32))
    finally:
        b.close()
    np.testing.assert_array_equal(r["x"].cpu().numpy(), np.stack([o["x"] for o in refs]))
    assert_same_arrays(arrays, from_run)
    assert_same_arrays(on_device, arrays)
    assert_logs_equal_oracle(arrays, refs)


def test_phase1_on_the_device_from_host_arrays(hip, oracle, monkeypatch):
    s, probs = make("general")
    refs = oracle_logs(oracle, "general", s["n"], probs)
    require_adds_and_removes(refs)
    monkeypatch.setenv("LEXLS_LSI_DEVICE_PHASE1", "1")  # (read per run)
    r, arrays, name = logged_run(probs, s["n"])
    assert name.startswith("lsi_fused<"), name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


# ---- 5: deactivate_first_wrong_sign ----
@pytest.mark.parametrize("route", ["fused", "stages", "one_by_one"])
def test_deactivate_first_wrong_sign(hip, oracle, monkeypatch, route):
    s, probs = make("general")
    refs = oracle_logs(oracle, "general first", s["n"], probs, deactivate_first_wrong_sign=1)
    require_adds_and_removes(refs)
    removes = [e for o in refs for e in o["log"] if e["ctr_type"] == 0]
    assert len(removes) >= 3 and all(e["alpha_or_lambda"] == 0.0 for e in removes)
    if route == "stages":
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    if route == "one_by_one":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    r, arrays, name = logged_run(probs, s["n"], deactivate_first_wrong_sign=1)
    assert name.startswith("lsi_fused<") if route == "fused" else name == "host" if route == "one_by_one" else name not in ("host", ""), name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)
    log, alpha, _ = arrays
    assert not alpha[log[:, :, FIELDS.index("ctr_type")] == 0].any()


# ---- 6: cycling handling, resident ----
@pytest.mark.parametrize("par", [CAP3, CAP50], ids=["cap3", "cap50"])
def test_cycling(hip, oracle, par):
    s, probs = make_cycling()
    refs = oracle_logs(oracle, ("cycling", par["cycling_max_counter"]), s["n"], probs, **par)
    require_cycling(refs)
    r, arrays, name = logged_run(probs, s["n"], **par)
    assert name.startswith("lsi_fused<"), name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


def test_cycling_stage_route(hip, oracle, monkeypatch):
    s, probs = make_cycling()
    refs = oracle_logs(oracle, ("cycling", CAP3["cycling_max_counter"]), s["n"], probs, **CAP3)
    require_cycling(refs)
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    r, arrays, name = logged_run(probs, s["n"], **CAP3)
    assert not name.startswith("lsi_fused<") and name not in ("host", ""), name
    assert_logs_equal_oracle(arrays, refs)


# ---- 7: regularized runs on the persistent REG launch: 41 x 12 cold, 64 x 16 warm-started (its cold start only ADDs: more rows than columns) ----
def test_regularized(hip, oracle):
    s = REG_SHAPES["ik"]
    probs = [P.lsi_problem(s["seed"] + i, s["n"], s["dims"]) for i in range(8)]
    par = dict(regularization_factors=s["factors"], regularization_type=1)
    refs = oracle_logs(oracle, "ik reg1", s["n"], probs, **par)
    require_adds_and_removes(refs)
    r, arrays, name = logged_run(probs, s["n"], **par)
    assert name == "lsi_fused<lqr_wave<41,12,exact,regularized>>", name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


def test_regularized_64x16(hip, oracle):
    s, probs = make_wide()
    par = dict(regularization_factors=s["factors"], regularization_type=1)
    cold = oracle_logs(oracle, "wide reg1", s["n"], probs, **par)
    pert = [P.lsi_problem(s["seed"] + i, s["n"], s["dims"], perturb=1.0) for i in range(len(probs))]
    guess = np.stack([np.concatenate(o["active"]) for o in cold])
    x0 = np.stack([o["x"] for o in cold])
    refs = oracle_logs(oracle, "wide reg1 warm", s["n"], pert, guesses=guess, x0=x0, **par)
    require_adds_and_removes(refs)
    r, arrays, name = logged_run(pert, s["n"], active_guess=guess, x0=x0, **par)
    assert name == "lsi_fused<lqr_wave<64,16,regularized>>", name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


# ---- 8: the host path ----
@pytest.mark.parametrize("why", ["resident_off", "type7", "cycling_regularized"])
def test_host_path(hip, oracle, monkeypatch, why):
    s, probs = make("bounds")
    factors = [0, 0.3, 0.2, 0.4]
    par = {"resident_off": dict(), "type7": dict(regularization_factors=factors, regularization_type=7, max_number_of_factorizations=30),  # (it ends on the limit)
           "cycling_regularized": dict(regularization_factors=factors, regularization_type=1, cycling_handling_enabled=1)}[why]
    refs = oracle_logs(oracle, ("bounds host", why), s["n"], probs, **par)
    require_adds_and_removes(refs)
    if why == "resident_off":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    r, arrays, name = logged_run(probs, s["n"], **par)
    assert name == "host", name
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)


# ---- 9: capacity ----
@pytest.mark.parametrize("route", ["fused", "host"])
def test_capacity(hip, oracle, monkeypatch, route):
    s, probs = make("ik")
    refs = oracle_logs(oracle, "ik", s["n"], probs)
    require_adds_and_removes(refs)
    assert min(len(o["log"]) for o in refs) > 2, "every log must be longer than the capacity of this test"
    if route == "host":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")
    pk = lexlsi.pack_batch(s["n"], probs)
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    batch, cap, pad = len(probs), 2, 7
    log = np.full((batch * cap + pad) * len(FIELDS), -77, np.int32)  # sentinels behind what the call may write
    alpha = np.full(batch * cap + pad, -77.0)
    counts = np.full(batch + pad, 0xABCDABCD, np.uint32)
    try:
        b.set_working_set_log(cap)
        r = b.run(pk)
        assert (b.last_kernel() == "host") == (route == "host"), b.last_kernel()
        capi.check(capi.lib().lexls_lsi_batch_get_working_set_log(b._h, log.ctypes.data_as(C.POINTER(C.c_int32)), alpha.ctypes.data_as(C.POINTER(C.c_double)),
                                                                  counts.ctypes.data_as(C.POINTER(C.c_uint32))))
        only_counts = np.zeros(batch, np.uint32)  # any pointer may be NULL
        capi.check(capi.lib().lexls_lsi_batch_get_working_set_log(b._h, None, None, only_counts.ctypes.data_as(C.POINTER(C.c_uint32))))
    finally:
        b.close()
    assert_result_equals_oracle(r, refs)
    assert (log[batch * cap * len(FIELDS):] == -77).all() and (alpha[batch * cap:] == -77.0).all() and (counts[batch:] == 0xABCDABCD).all()
    np.testing.assert_array_equal(only_counts, counts[:batch])
    assert_logs_equal_oracle((log[:batch * cap * len(FIELDS)].reshape(batch, cap, len(FIELDS)), alpha[:batch * cap].reshape(batch, cap), counts[:batch]), refs, capacity=cap)


# ---- 10: off means off ----
def test_off_means_off(hip, oracle):
    s, probs = make("ik")
    refs = oracle_logs(oracle, "ik", s["n"], probs)
    require_adds_and_removes(refs)
    pk = lexlsi.pack_batch(s["n"], probs)
    fresh = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    null = [None, None, None]
    try:
        never_logged = fresh.run(pk)
        assert capi.lib().lexls_lsi_batch_get_working_set_log(b._h, *null) == LEXLS_ERR_INVALID  # the log is off
        b.set_working_set_log(CAPACITY)
        assert capi.lib().lexls_lsi_batch_get_working_set_log(b._h, *null) == LEXLS_ERR_INVALID  # no run yet
        logged = b.run(pk)
        assert_logs_equal_oracle(b.working_set_log_arrays(), refs)
        b.set_working_set_log(0)
        unlogged = b.run(pk)
        assert b.last_kernel() == fresh.last_kernel()
        assert capi.lib().lexls_lsi_batch_get_working_set_log(b._h, *null) == LEXLS_ERR_INVALID  # the last run ran with the log off
        with pytest.raises(capi.LexlsError):
            b.working_set_log_device()
        b.set_working_set_log(4)  # on again: nothing to report before the next run
        assert capi.lib().lexls_lsi_batch_get_working_set_log(b._h, *null) == LEXLS_ERR_INVALID
    finally:
        b.close()
        fresh.close()
    for r in (logged, unlogged):
        np.testing.assert_array_equal(r["info"].array, never_logged["info"].array)
        for k in ("x", "active", "v"):
            np.testing.assert_array_equal(r[k], never_logged[k])


# ---- 11: two groups ----
@pytest.mark.parametrize("route", ["fused", "host"])
def test_two_groups(hip, oracle, monkeypatch, route):
    s, probs = make("bounds")
    assert len(probs) >= 8
    refs = oracle_logs(oracle, "bounds", s["n"], probs)
    require_adds_and_removes(refs)
    assert len({tuple(tuple(sorted(e.items())) for e in o["log"]) for o in refs}) >= 8, "the instances' logs must differ to tell their rows apart"
    monkeypatch.setenv("LEXLS_LSI_GROUPS", "2")  # (read when the batch object is made)
    if route == "host":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")
    pk = lexlsi.pack_batch(s["n"], probs)
    b = lexlsi.LsiBatch(s["n"], pk.dims, pk.types, len(probs))
    try:
        b.set_working_set_log(CAPACITY)
        r = b.run(pk)
        assert b.stats()["groups"] == 2
        arrays = b.working_set_log_arrays()
    finally:
        b.close()
    assert_result_equals_oracle(r, refs)
    assert_logs_equal_oracle(arrays, refs)
