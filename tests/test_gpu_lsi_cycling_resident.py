"""LexLSI batches with ParametersLexLSI::cycling_handling_enabled (cycling.h:32-65) and no regularization keep their active-set iterations on
the device: the handler of every instance (last working-set change, relaxations done) travels with it, an ADD of the triple that was just REMOVEd
relaxes that bound in the resident constraint data, and after cycling_max_counter relaxations the instance ends PROBLEM_SOLVED_CYCLING_HANDLING.
Persistent launch, lock-step stages (LEXLS_LSI_NO_FUSED=1), with and without deactivate_first_wrong_sign, and the unchanged host path
(LEXLS_LSI_RESIDENT=0), against the oracle-backed driver: info, x, the final working set and v with assert_array_equal, the counters
(LsiBatch.cycling_counters) against the cycling_detected entries of the oracle's working-set log.  The tolerance is zero, as for every LexLSI path.

Random problems never relax a bound, so the inputs are made degenerate (degenerate()): the later objectives repeat rows of the first general one
with a conflicting interval, and tol_wrong_sign_lambda = 0.  Every test first asserts, from the oracle's results alone, that its batch relaxes
what the test relies on — a change of the problem generator cannot silently turn it into a test without relaxations."""
import ctypes as C

import numpy as np
import pytest

from lexls_amd import capi, lexlsi, problems as P

pytestmark = pytest.mark.gpu

SHAPES = {
    "bounds": dict(n=14, dims=[4, 5, 5, 4], simple_bounds=True, seeds=range(1300, 1340)),  # objective 0 = simple bounds
    # (seeds 10-49 hold two instances that relax and then end PROBLEM_SOLVED; 117, 118 and 121 are three more of that kind)
    "general": dict(n=10, dims=[6, 6, 6], simple_bounds=False, seeds=[*range(10, 50), 117, 118, 121]),
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True, seeds=range(100, 112)),  # the 41 x 12 instantiation
}
CYCLING = dict(tol_wrong_sign_lambda=0.0, cycling_handling_enabled=1)
CAP3 = dict(cycling_max_counter=3, cycling_relax_step=1e-6, **CYCLING)
CAP50 = dict(cycling_max_counter=50, cycling_relax_step=1e-8, **CYCLING)
SOLVED, SOLVED_CYCLING = 0, 1  # TerminationStatus: PROBLEM_SOLVED, PROBLEM_SOLVED_CYCLING_HANDLING
LEXLS_ERR_UNSUPPORTED = 3
_cache = {}


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


def make(shape):
    s = SHAPES[shape]
    return s, [degenerate(seed, s["n"], s["dims"], s["simple_bounds"]) for seed in s["seeds"]]


def oracle_refs(oracle, shape, **params):
    """per instance the oracle-backed driver's result and the relaxations of its working-set log; computed once per parameter set, shared, never modified"""
    key = (shape, tuple(sorted(params.items())))
    if key not in _cache:
        s, probs = make(shape)
        refs = []
        for p in probs:
            o = oracle.lsi_run(s["n"], p, **params)
            o["relaxed"] = [e for e in oracle.lsi_run_debug(s["n"], p, **params)["debug"]["working_set_log"] if e["cycling_detected"]]
            refs.append(o)
        _cache[key] = refs
    return _cache[key]


def counts_of(refs):
    return np.array([len(o["relaxed"]) for o in refs], np.uint32)


def assert_equals_oracle(r, counters, refs):
    for b, o in enumerate(refs):
        assert r["info"][b] == o["info"], b  # status, iterations, activations, deactivations, factorizations, rank
        np.testing.assert_array_equal(r["x"][b], o["x"])
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]))
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]))
    np.testing.assert_array_equal(counters, counts_of(refs))


def assert_same_run(a, b):
    np.testing.assert_array_equal(a["info"].array, b["info"].array)
    for k in ("x", "active", "v"):
        np.testing.assert_array_equal(a[k], b[k])


def new_batch(probs, n):
    pk = lexlsi.pack_batch(n, probs)
    return lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs)), pk


def run_once(probs, n, **params):
    """-> result, cycling counters, kernel name of one run on a fresh batch object"""
    b, pk = new_batch(probs, n)
    try:
        r = b.run(pk, **params)
        return r, b.cycling_counters(), b.last_kernel()
    finally:
        b.close()


def run_fused_against_the_oracle(oracle, shape, **params):
    refs = oracle_refs(oracle, shape, **params)
    s, probs = make(shape)
    r, counters, name = run_once(probs, s["n"], **params)
    assert name.startswith("lsi_fused<"), name
    assert_equals_oracle(r, counters, refs)
    return r, counters


def require_bounds_batch_relaxes(refs):
    """what the persistent-launch, stage and host tests rely on: most instances relax, a simple bound among them, both activation types"""
    assert sum(len(o["relaxed"]) > 0 for o in refs) >= 30
    assert any(e["obj_index"] == 0 for o in refs for e in o["relaxed"]), "no instance relaxes a simple bound"
    assert {e["ctr_type"] for o in refs for e in o["relaxed"]} >= {1, 2}, "CTR_ACTIVE_LB and CTR_ACTIVE_UB must both be relaxed"


def test_persistent_launch(hip, oracle):
    require_bounds_batch_relaxes(oracle_refs(oracle, "bounds", **CAP3))
    run_fused_against_the_oracle(oracle, "bounds", **CAP3)


def test_outcomes(hip, oracle):
    """with 50 relaxations allowed some instances relax and then finish PROBLEM_SOLVED, others exhaust the handler"""
    refs = oracle_refs(oracle, "bounds", **CAP50)
    assert sum(o["info"]["status"] == SOLVED and len(o["relaxed"]) > 0 for o in refs) >= 3
    assert sum(o["info"]["status"] == SOLVED_CYCLING for o in refs) >= 10
    run_fused_against_the_oracle(oracle, "bounds", **CAP50)


def test_stage_route(hip, oracle, monkeypatch):
    refs = oracle_refs(oracle, "bounds", **CAP3)
    require_bounds_batch_relaxes(refs)
    s, probs = make("bounds")
    fused, fused_counters, name = run_once(probs, s["n"], **CAP3)
    assert name.startswith("lsi_fused<"), name
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    staged, counters, stage_kernel = run_once(probs, s["n"], **CAP3)
    assert not stage_kernel.startswith("lsi_fused<") and stage_kernel not in ("host", ""), stage_kernel
    assert_same_run(staged, fused)
    np.testing.assert_array_equal(counters, fused_counters)
    assert_equals_oracle(staged, counters, refs)


def test_host_route_unchanged(hip, oracle, monkeypatch):
    refs = oracle_refs(oracle, "bounds", **CAP3)
    require_bounds_batch_relaxes(refs)
    s, probs = make("bounds")
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    r, counters, name = run_once(probs, s["n"], **CAP3)
    assert name == "host", name
    assert_equals_oracle(r, counters, refs)


def test_no_simple_bounds(hip, oracle):
    refs = oracle_refs(oracle, "general", **CAP3)
    assert sum(len(o["relaxed"]) > 0 for o in refs) >= 15
    assert sum(o["info"]["status"] == SOLVED and len(o["relaxed"]) > 0 for o in refs) >= 3
    run_fused_against_the_oracle(oracle, "general", **CAP3)


@pytest.mark.parametrize("route", ["fused", "stages"])
def test_with_deactivate_first_wrong_sign(hip, oracle, monkeypatch, route):
    par = dict(deactivate_first_wrong_sign=1, **CAP3)
    refs = oracle_refs(oracle, "general", **par)
    assert sum(len(o["relaxed"]) > 0 for o in refs) >= 20
    if route == "fused":
        run_fused_against_the_oracle(oracle, "general", **par)
        return
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    s, probs = make("general")
    r, counters, name = run_once(probs, s["n"], **par)
    assert not name.startswith("lsi_fused<") and name not in ("host", ""), name
    assert_equals_oracle(r, counters, refs)


@pytest.mark.parametrize("par", [CAP3, dict(max_number_of_factorizations=120, **CAP50)], ids=["cap3", "cap50_limit120"])
def test_ik_shape(hip, oracle, par):
    refs = oracle_refs(oracle, "ik", **par)
    assert all(len(o["relaxed"]) > 0 for o in refs)
    if "max_number_of_factorizations" in par:  # relaxations and the factorization limit occur together; nobody exhausts the handler
        assert all(o["info"]["status"] != SOLVED_CYCLING for o in refs)
        assert any(o["info"]["status"] == 2 for o in refs), "no instance reaches MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED"
    else:
        assert all(o["info"]["status"] == SOLVED_CYCLING for o in refs)
    run_fused_against_the_oracle(oracle, "ik", **par)


def closes_a_circle_the_host_opened(log):
    """the first working-set change (iteration 0, on the host) is a REMOVE and the second one (the first resident iteration) its ADD, relaxed"""
    return (len(log) >= 2 and log[0]["ctr_type"] == 0 and log[1]["cycling_detected"] != 0 and
            (log[1]["obj_index"], log[1]["ctr_index"]) == (log[0]["obj_index"], log[0]["ctr_index"]))


def test_hand_over_of_the_handler_state(hip, oracle):
    """warm start from the cold run's final working set and x: iteration 0 runs on the host and REMOVEs a constraint, the first iteration on the
    device ADDs it again — a circle only a handler that came over with its last event can see"""
    s, probs = make("bounds")
    cold = oracle_refs(oracle, "bounds", **CAP3)
    guess = np.stack([np.concatenate(o["active"]) for o in cold])
    x0 = np.stack([o["x"] for o in cold])
    refs, opened_on_the_host = [], 0
    for p, o in zip(probs, cold):
        w = oracle.lsi_run_debug(s["n"], p, active_guess=o["active"], x0=o["x"], **CAP3)
        log = w["debug"]["working_set_log"]
        opened_on_the_host += closes_a_circle_the_host_opened(log)
        w["relaxed"] = [e for e in log if e["cycling_detected"]]
        refs.append(w)
    assert opened_on_the_host >= 1, "no instance closes on the device a circle that iteration 0 opened on the host"
    b, pk = new_batch(probs, s["n"])
    try:
        r = b.run(pk, active_guess=guess, x0=x0, **CAP3)
        assert b.last_kernel().startswith("lsi_fused<"), b.last_kernel()
        assert_equals_oracle(r, b.cycling_counters(), refs)
    finally:
        b.close()


def test_no_leak_between_runs(hip, oracle):
    """a cycling run, then a plain run of the same packed data on one batch object: the plain run starts from the caller's bounds, reports no
    relaxations and has its multipliers again"""
    cyc = oracle_refs(oracle, "bounds", **CAP3)
    require_bounds_batch_relaxes(cyc)
    s, probs = make("bounds")
    plain = [oracle.lsi_run(s["n"], p) for p in probs]
    b, pk = new_batch(probs, s["n"])
    out = np.zeros((pk.batch, len(s["dims"]), pk.total))
    try:
        r = b.run(pk, **CAP3)
        assert b.last_kernel().startswith("lsi_fused<"), b.last_kernel()
        assert_equals_oracle(r, b.cycling_counters(), cyc)
        assert capi.lib().lexls_lsi_batch_get_lambda(b._h, out.ctypes.data_as(C.POINTER(C.c_double))) == LEXLS_ERR_UNSUPPORTED
        r = b.run(pk)
        for i, o in enumerate(plain):
            assert r["info"][i] == o["info"], i
            np.testing.assert_array_equal(r["x"][i], o["x"])
            np.testing.assert_array_equal(r["active"][i], np.concatenate(o["active"]))
            np.testing.assert_array_equal(r["v"][i], np.concatenate(o["v"]))
        np.testing.assert_array_equal(b.cycling_counters(), np.zeros(pk.batch, np.uint32))
        assert b.lambda_array().shape == (pk.batch, len(s["dims"]), pk.total)
    finally:
        b.close()
