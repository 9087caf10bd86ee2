"""LexLSI batches with ParametersLexLSI::deactivate_first_wrong_sign (lexlsi.h:1063-1105) keep their active-set iterations on the device:
the removal search collects the SET of wrong-sign multipliers (lexls_lse_sensitivity_collect) and the iteration removes its member that
entered the working set first (an activation stamp per constraint stands for the reference's WS list).  Three paths — the persistent launch,
the lock-step stages (LEXLS_LSI_NO_FUSED=1) and the one-by-one host driver (LEXLS_LSI_RESIDENT=0) — against the oracle-backed driver
(oracle.lsi_run(..., deactivate_first_wrong_sign=1)) and against each other.  The tolerance is zero: info, x, the final working set and v
compare with assert_array_equal, as for every LexLSI path.

Every batch is warm-started with all constraints active at the upper bound, so removals are needed.  The rule must matter on the inputs: the
oracle's own runs with and without the flag have to differ (info or final working set) on at least a quarter of the instances of a batch,
and every instance has to deactivate under the flag — asserted from the oracle's results (require_the_rules_differ), so a change of the
problem generator cannot silently empty these tests."""
import numpy as np
import pytest

from lexls_amd import lexlsi, problems as P

pytestmark = pytest.mark.gpu

SHAPES = {
    # the batch of tests/test_gpu_lsi.py::test_batch_with_deactivate_first_wrong_sign, twelve instances
    "small": dict(n=20, dims=[6, 5, 5, 6], count=12, seed=800),
    # the IK shape (BASELINE configs[2..4])
    "ik": dict(n=40, dims=[12] * 5, count=32, seed=20261000),
}
FLAG = dict(deactivate_first_wrong_sign=1)
_cache = {}


def make(shape, bounds):
    s = SHAPES[shape]
    probs = [P.lsi_problem(s["seed"] + i, s["n"], s["dims"], simple_bounds=bounds) for i in range(s["count"])]
    guess = np.full((s["count"], sum(s["dims"])), 2, np.uint8)  # everything active at the upper bound
    return s, probs, guess


def oracle_refs(oracle, shape, bounds, **params):
    """the oracle-backed driver on every instance of a batch; computed once per parameter set and shared (never modified)"""
    key = (shape, bounds, tuple(sorted(params.items())))
    if key not in _cache:
        s, probs, guess = make(shape, bounds)
        cuts = np.cumsum(s["dims"])[:-1]
        _cache[key] = [oracle.lsi_run(s["n"], p, active_guess=np.split(guess[i], cuts), **params) for i, p in enumerate(probs)]
    return _cache[key]


def require_the_rules_differ(oracle, shape, bounds, **params):
    with_flag, without = oracle_refs(oracle, shape, bounds, **params, **FLAG), oracle_refs(oracle, shape, bounds, **params)
    differ = sum(a["info"] != b["info"] or not np.array_equal(np.concatenate(a["active"]), np.concatenate(b["active"])) for a, b in zip(with_flag, without))
    assert 4 * differ >= len(with_flag), f"{shape}: the two removal rules differ on {differ} of {len(with_flag)} instances only"
    assert all(o["info"]["deactivations"] > 0 for o in with_flag), f"{shape}: an instance removes nothing under the flag"
    return with_flag


def assert_equals_oracle(r, refs):
    for b, o in enumerate(refs):
        assert r["info"][b] == o["info"], b  # status, iterations, activations, deactivations, factorizations, rank
        np.testing.assert_array_equal(r["x"][b], o["x"])
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]))
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]))


def assert_same_run(a, b):
    np.testing.assert_array_equal(a["info"].array, b["info"].array)
    for k in ("x", "active", "v"):
        np.testing.assert_array_equal(a[k], b[k])


def new_batch(probs, n):
    pk = lexlsi.pack_batch(n, probs)
    return lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs)), pk


def three_paths(monkeypatch, probs, n, guess, **params):
    b, pk = new_batch(probs, n)
    fused = b.run(pk, active_guess=guess, **params)
    name, stats = b.last_kernel(), b.stats()
    assert name.startswith("lsi_fused<"), name
    longest = max(i["factorizations"] for i in fused["info"])
    assert stats["groups"] >= 1 and stats["device_step"] >= longest - 2, (stats, longest)  # real stages: the resident iterations are counted
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    staged = b.run(pk, active_guess=guess, **params)
    stage_kernel = b.last_kernel()
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")
    b.close()
    assert not stage_kernel.startswith("lsi_fused<") and stage_kernel != "host" and stage_kernel != "", stage_kernel
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    h, _ = new_batch(probs, n)
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    host = h.run(pk, active_guess=guess, **params)
    assert h.last_kernel() == "host"
    h.close()
    assert_same_run(staged, fused)
    assert_same_run(host, fused)
    return fused


@pytest.mark.parametrize("bounds", [True, False], ids=["simple_bounds", "general_only"])
@pytest.mark.parametrize("shape", ["small", "ik"])
def test_three_paths_against_the_oracle(hip, oracle, monkeypatch, shape, bounds):
    refs = require_the_rules_differ(oracle, shape, bounds)
    s, probs, guess = make(shape, bounds)
    r = three_paths(monkeypatch, probs, s["n"], guess, **FLAG)
    assert_equals_oracle(r, refs)


@pytest.mark.parametrize("shape", ["small", "ik"])
def test_factorization_limit(hip, oracle, monkeypatch, shape):
    """max_number_of_factorizations cuts some instances short (status 2 with the counters of that moment) and lets others finish"""
    limit = {"small": 12, "ik": 150}[shape]
    par = dict(max_number_of_factorizations=limit, **FLAG)
    refs = oracle_refs(oracle, shape, True, **par)
    stopped = sum(o["info"]["status"] != 0 for o in refs)
    assert 0 < stopped < len(refs), f"the limit must cut some instances short and let others finish ({stopped} of {len(refs)})"
    s, probs, guess = make(shape, True)
    r = three_paths(monkeypatch, probs, s["n"], guess, **par)
    assert_equals_oracle(r, refs)


def test_regularized_run_with_the_flag(hip, oracle):
    s, probs, guess = make("small", True)
    factors = [0, 0.3, 0.2, 0.4]
    par = dict(regularization_type=1, **FLAG)
    cuts = np.cumsum(s["dims"])[:-1]
    refs = [oracle.lsi_run(s["n"], p, active_guess=np.split(guess[i], cuts), regularization_factors=factors, **par) for i, p in enumerate(probs)]
    assert all(o["info"]["deactivations"] > 0 for o in refs)
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, active_guess=guess, regularization_factors=factors, **par)
    name = b.last_kernel()
    b.close()
    assert name.startswith("lsi_fused<") and "regularized" in name, name
    assert_equals_oracle(r, refs)


def test_no_leakage_on_a_reused_batch_object(hip, oracle):
    """plain run, flag run, plain run on one object: neither the rule nor the stamps of a run reach the next one"""
    with_flag = require_the_rules_differ(oracle, "ik", True)
    plain = oracle_refs(oracle, "ik", True)
    s, probs, guess = make("ik", True)
    b, pk = new_batch(probs, s["n"])
    got, names = [], []
    for par in (dict(), FLAG, dict(), FLAG):
        got.append(b.run(pk, active_guess=guess, **par))
        names.append(b.last_kernel())
    b.close()
    assert all(k.startswith("lsi_fused<") for k in names), names
    for r, refs in zip(got, (plain, with_flag, plain, with_flag)):
        assert_equals_oracle(r, refs)


@pytest.mark.parametrize("shape,bounds", [("small", True), ("ik", True), ("small", False)])
def test_lambdas_after_a_resident_flag_run(hip, oracle, shape, bounds):
    """LsiBatch.lambdas() (lexls_lsi_batch_get_lambda) after a resident run with the flag: the oracle-backed driver's getLambda, bit for bit"""
    s, probs, guess = make(shape, bounds)
    cuts = np.cumsum(s["dims"])[:-1]
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, active_guess=guess, **FLAG)
    assert b.last_kernel().startswith("lsi_fused<"), b.last_kernel()
    lam = b.lambdas()
    b.close()
    assert_equals_oracle(r, oracle_refs(oracle, shape, bounds, **FLAG))
    for i, p in enumerate(probs):
        o = oracle.lsi_run_debug(s["n"], p, active_guess=np.split(guess[i], cuts), **FLAG)
        assert len(lam[i]) == len(o["debug"]["lambda"])
        for k, (a, c) in enumerate(zip(lam[i], o["debug"]["lambda"])):
            np.testing.assert_array_equal(a, c, err_msg=f"instance {i}, objective {k}")
