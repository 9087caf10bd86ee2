"""The optimality certificate of tests/lexopt.py, validated on the CPU before tests/test_gpu_lsi_optimality.py applies it to the GPU paths.

Accepted: the oracle-backed driver's solutions of every fixture family below in every run mode the GPU test uses (cold, deactivate_first_wrong_sign,
cycling handling, warm start from a neighbour with and without v0), every instance ending with status 0, and the reference's own stored #Solution
of tests/golden/test_01.dat — the one place where the certificate meets numbers this project did not produce.

Rejected, every case: x + 1e-6 N(0,1); the same run stopped early by max_number_of_factorizations (the largest limit whose x is more than 1e-6
from the final one); the solution of the same data with two levels swapped; the solution of instance b + 1 offered for problem b; the solution
with one active inequality moved towards its opposite bound by 1e-6.

The acceptance bounds lexopt.ACCEPT / ACCEPT_LAMBDA are 1000 x the largest accepted figure; the tests print what they measure and assert that the
bounds hold every accepted case and stay 100 x below the smallest rejected one.

The fixture families (FAMILIES, problems_of, RUN_MODES, warm_start_of) are shared with the GPU test, which imports this module."""
import os

import numpy as np
import pytest

import lexopt
from conftest import GOLDEN
from lexls_amd import problems as P

# name -> shape; 6-8 instances each, the smallest shapes that reach each kernel (see tests/test_gpu_lsi_optimality.py).  The seeds are those on
# which every run mode ends with status 0 on the oracle-backed driver and, "small" apart, the last level cannot be met: then x is pinned by the
# hierarchy (a merely feasible x certifies trivially, see pinned()).
FAMILIES = {
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True, seeds=[31001, 31002, 31004, 31005, 31006, 31007, 31008, 31009]),  # lqr_wave<41,12> / lsi_fused at its full width
    "small": dict(n=20, dims=[6, 5, 5, 6], simple_bounds=True, pinned=False, seeds=list(range(32000, 32008))),
    "general": dict(n=12, dims=[4, 5, 4, 6], simple_bounds=False, seeds=list(range(33000, 33008))),
    "wide": dict(n=57, dims=[12, 16, 16, 16, 16], simple_bounds=True, seeds=[34001, 34003, 34004, 34005, 34006, 34007]),  # the 64 x 16 instantiation
    "cols46": dict(n=45, dims=[12] * 5, simple_bounds=True, seeds=[35000, 35010, 35021, 35023, 35052, 35054]),  # 46 columns: the stage path behind the gather launch
    "duplicate": dict(n=12, dims=[4, 5, 4, 6], simple_bounds=False, seeds=[36000, 36001, 36002, 36003, 36004, 36005, 36006, 36008], special="duplicate"),
    "infeasible": dict(n=12, dims=[4, 5, 4, 6], simple_bounds=False, seeds=list(range(37000, 37008)), special="infeasible"),
}
PERTURB = 0.05  # the warm-start neighbour
RUN_MODES = {
    "cold": {},
    "first_wrong_sign": dict(deactivate_first_wrong_sign=1),
    "cycling": dict(cycling_handling_enabled=1),
}
_cache = {}


def _special(objs, kind):
    """duplicate: row 0 of level 1 repeats row 0 of level 0 with its interval moved past that row's upper bound — both end active, the second with
    a violation, and the equality problem is rank deficient.  infeasible: row 1 of level 0 repeats row 0 with a disjoint interval — level 0 cannot
    be met, v is non-zero on level 0."""
    if kind == "duplicate":
        objs[1]["A"][0] = objs[0]["A"][0]
        objs[1]["lb"][0] = objs[0]["ub"][0] + 0.5
        objs[1]["ub"][0] = objs[0]["ub"][0] + 1.0
    elif kind == "infeasible":
        objs[0]["A"][1] = objs[0]["A"][0]
        objs[0]["lb"][1] = objs[0]["ub"][0] + 1.0
        objs[0]["ub"][1] = objs[0]["ub"][0] + 1.5
    return objs


def problems_of(name, perturb=0.0):
    """the batch of a family (perturb = 0) or its warm-start neighbours; made once, shared, never modified"""
    key = ("problems", name, perturb)
    if key not in _cache:
        f = FAMILIES[name]
        _cache[key] = [_special(P.lsi_problem(seed, f["n"], f["dims"], simple_bounds=f["simple_bounds"], perturb=perturb), f.get("special"))
                       for seed in f["seeds"]]
    return _cache[key]


def split(name, a):
    return np.split(np.asarray(a), np.cumsum(FAMILIES[name]["dims"])[:-1])


def warm_start_of(oracle, name):
    """-> (guess, x0, v0), each (batch, ...): the solution of every instance's neighbour (right-hand sides perturbed by PERTURB) from the
    oracle-backed driver; equality flags are not part of a guess (the driver activates those rows itself)"""
    key = ("warm", name)
    if key not in _cache:
        f = FAMILIES[name]
        rs = [oracle.lsi_run(f["n"], p) for p in problems_of(name, PERTURB)]
        assert all(r["info"]["status"] == 0 for r in rs)
        active = np.stack([np.concatenate(r["active"]) for r in rs])
        _cache[key] = (np.where(active == 3, 0, active).astype(np.uint8), np.stack([r["x"] for r in rs]), np.stack([np.concatenate(r["v"]) for r in rs]))
    return _cache[key]


def oracle_runs(oracle, name, mode):
    """the oracle-backed driver's results of a family in one run mode (with the multipliers where the mode has them); computed once"""
    key = ("runs", name, mode)
    if key not in _cache:
        f = FAMILIES[name]
        out = []
        for b, p in enumerate(problems_of(name)):
            kw = {}
            if mode.startswith("warm"):
                guess, x0, v0 = warm_start_of(oracle, name)
                kw = dict(active_guess=split(name, guess[b]), x0=x0[b])
                if mode == "warm_v0":
                    kw["v0"] = split(name, v0[b])
            else:
                kw = dict(RUN_MODES[mode])
            r = oracle.lsi_run_debug(f["n"], p, **kw)
            if mode == "cycling":
                r["relaxed"] = sum(1 for e in r["debug"]["working_set_log"] if e["cycling_detected"])
            out.append(r)
        _cache[key] = out
    return _cache[key]


ALL_MODES = list(RUN_MODES) + ["warm", "warm_v0"]


def pinned(name):
    """more rows than variables: the last levels are in conflict and x is unique.  "small" (16 general rows, 20 variables) meets every level
    exactly; any feasible point is optimal there, every gradient is zero and so is every multiplier: its results must pass the certificate and
    the consistency checks like all others, but there is nothing the rejection families could be rejected for (the solution of the swapped
    hierarchy, for one, IS optimal)"""
    return FAMILIES[name].get("pinned", True)


# Instances (by seed) whose deactivate_first_wrong_sign run ends with status 0 at a point that is NOT optimal, with the certificate it gets.  The
# rule's scan of the fixed variables reads the multipliers of the first general rows instead of the fixed variables' own (kept from the reference,
# lexlse.h:599-600: include/lexls_hip.h, lexls_lse_sensitivity), so a simple bound can keep a multiplier of the wrong sign.  Everything else about
# these runs is asserted like for every other instance (status 0, kernel, v and working set consistent with x, stationarity of the multipliers), and
# the certificate is asserted to REJECT exactly them: a change of the rule shows here.
FIRST_WRONG_SIGN_NOT_OPTIMAL = {"ik": {31007: 0.227}, "wide": {34003: 0.0128, 34007: 0.00515}, "cols46": {35000: 0.0339}}


def not_optimal(name, mode):
    """the indices of the instances of a family that a run mode is known to leave at a non-optimal point"""
    if mode != "first_wrong_sign":
        return set()
    return {FAMILIES[name]["seeds"].index(seed) for seed in FIRST_WRONG_SIGN_NOT_OPTIMAL.get(name, {})}


def assert_not_optimal(name, b, p, x, active, lam, what):
    """a known non-optimal result: rejected by the certificate with the margin of the rejection families, and, where multipliers are returned, for
    the known reason — they are stationary, one on a simple bound has the wrong sign"""
    f = FAMILIES[name]
    t = float(lexopt.certificate(f["n"], p, x).max())
    assert t >= 100 * lexopt.ACCEPT, (what, b, t)
    assert abs(t - FIRST_WRONG_SIGN_NOT_OPTIMAL[name][f["seeds"][b]]) <= 0.01 * t, (what, b, t)
    if lam is not None:
        fig = lexopt.lambda_check(f["n"], p, x, active, lam)
        assert fig["stationarity"] <= lexopt.ACCEPT_LAMBDA and fig["own_block"] <= lexopt.EPS_ON_BOUND and fig["stray"] == 0.0, (what, b, fig)
        assert fig["wrong_sign"] > 1e-3, (what, b, fig)


def accepted_figures(oracle):
    """(certificate, lambda figures) of every accepted oracle case: {(family, mode, instance): figure}; the instances of FIRST_WRONG_SIGN_NOT_OPTIMAL
    are asserted to be rejected instead (everything else about them is asserted as for the others)"""
    if "accepted" not in _cache:
        cert, lam = {}, {}
        for name, f in FAMILIES.items():
            for mode in ALL_MODES:
                for b, (p, r) in enumerate(zip(problems_of(name), oracle_runs(oracle, name, mode))):
                    assert r["info"]["status"] == 0, (name, mode, b, r["info"])
                    if mode == "cycling":
                        assert r["relaxed"] == 0, (name, b, "a bound was relaxed: the problem solved is not the caller's")
                    lexopt.assert_consistent(lexopt.consistent(f["n"], p, r["x"], r["active"], r["v"]), (name, mode, b))
                    if b in not_optimal(name, mode):
                        assert_not_optimal(name, b, p, r["x"], r["active"], r["debug"]["lambda"], (name, mode))
                        continue
                    cert[name, mode, b] = float(lexopt.certificate(f["n"], p, r["x"]).max())
                    fig = lexopt.lambda_check(f["n"], p, r["x"], r["active"], r["debug"]["lambda"])
                    lam[name, mode, b] = fig
        _cache["accepted"] = (cert, lam)
    return _cache["accepted"]


def golden_problem():
    return lexopt.read_dat(os.path.join(GOLDEN, "test_01.dat"), one_based=True)


def test_dat_reader_reads_the_reference_fixture(oracle):
    d = golden_problem()
    assert d["n"] == 88 and [len(o["lb"]) for o in d["objectives"]] == [74, 33, 3, 2, 97]
    assert "var" in d["objectives"][0] and d["objectives"][0]["var"].min() >= 0 and d["objectives"][0]["var"].max() < 88
    assert d["solution"].shape == (88,) and d["guess"].shape == (88,)
    ref = oracle.lsi_run_dat(os.path.join(GOLDEN, "test_01.dat"))
    np.testing.assert_array_equal(d["solution"], ref["solution"])  # the same numbers the project's C++ reader finds
    r = oracle.lsi_run(88, d["objectives"])  # and the same problem: the driver reaches the stored solution from these objectives
    assert r["info"]["status"] == 0
    np.testing.assert_allclose(r["x"], d["solution"], atol=1e-9)


def test_fixtures_are_what_they_claim(oracle):
    """every instance of every family and mode ends with status 0; the families exercise what they are there for"""
    for name in FAMILIES:
        for mode in ALL_MODES:
            assert all(r["info"]["status"] == 0 for r in oracle_runs(oracle, name, mode)), (name, mode)
        cold = oracle_runs(oracle, name, "cold")
        assert all(r["info"]["iterations"] > 1 for r in cold), name  # the active-set loop has work to do
        assert all(np.abs(r["v"][-1]).max() > 1e-3 for r in cold) == pinned(name), name  # the hierarchy is in conflict: x is pinned
    assert any(r["info"]["deactivations"] > 0 for name in FAMILIES for r in oracle_runs(oracle, name, "first_wrong_sign"))
    for r in oracle_runs(oracle, "duplicate", "cold"):
        assert r["active"][0][0] != 0 and r["active"][1][0] != 0 and abs(r["v"][1][0]) > 0.4  # both copies active: rank deficient
    for r in oracle_runs(oracle, "infeasible", "cold"):
        assert abs(r["v"][0][0]) > 0.4 and abs(r["v"][0][1]) > 0.4  # level 0 cannot be met
    for name in FAMILIES:  # a warm start changes the run (otherwise the warm paths would only repeat the cold ones)
        assert any(w["info"] != c["info"] for w, c in zip(oracle_runs(oracle, name, "warm"), oracle_runs(oracle, name, "cold"))), name


def test_certificate_accepts_the_stored_solution_of_test_01():
    d = golden_problem()
    t = lexopt.certificate(d["n"], d["objectives"], d["solution"])
    print("test_01.dat #Solution: certificate per level", t)
    assert t.max() <= lexopt.ACCEPT, t


def test_certificate_accepts_every_oracle_solution(oracle):
    cert, lam = accepted_figures(oracle)
    worst = max(cert, key=cert.get)
    print("certificate, accepted: max", cert[worst], "at", worst)
    for key in ("stationarity", "own_block", "wrong_sign", "stray"):
        w = max(lam, key=lambda k: lam[k][key])
        print("lambda_check, accepted: max", key, lam[w][key], "at", w)
    assert cert[worst] <= lexopt.ACCEPT, (worst, cert[worst])
    for k, fig in lam.items():
        lexopt.assert_lambda(fig, k)


# --- rejections -----------------------------------------------------------------------------------------------------------------------------

def _noise(name, b, count, stream):
    return P.normal(FAMILIES[name]["seeds"][b], count, 9000 + stream)


def rejected_points(oracle, name):
    """{(case, instance): x} of the five rejection families for one fixture family, from its cold runs"""
    f = FAMILIES[name]
    n, probs, runs = f["n"], problems_of(name), oracle_runs(oracle, name, "cold")
    out = {}
    for b, (p, r) in enumerate(zip(probs, runs)):
        out["noise", b] = r["x"] + 1e-6 * _noise(name, b, n, 0)
        for limit in range(r["info"]["factorizations"] - 1, 0, -1):  # (the last factorization usually only confirms the optimum)
            early = oracle.lsi_run(n, p, max_number_of_factorizations=limit)
            if np.abs(early["x"] - r["x"]).max() > 1e-6:
                assert early["info"]["status"] == 2
                out["stopped_early", b] = early["x"]
                break
        i, j = len(p) - 2, len(p) - 1  # the last two levels: the ones in conflict, so their order matters
        swapped = list(p)
        swapped[i], swapped[j] = p[j], p[i]
        s = oracle.lsi_run(n, swapped)
        assert s["info"]["status"] == 0
        out["levels_swapped", b] = s["x"]
        out["neighbour", b] = runs[(b + 1) % len(runs)]["x"]
        # one active inequality moved off its bound towards the opposite one: the row with the largest multiplier, so that it matters
        L = np.abs(np.vstack(r["debug"]["lambda"]))
        act = np.concatenate(r["active"])
        L[(act != 1) & (act != 2)] = -1.0
        L[np.abs(np.concatenate(r["v"])) > 1e-9] = -1.0  # (not a violated one: moving it inwards is an improvement the bound stops nobody from making)
        row = int(np.argmax(L.max(axis=1)))
        assert L[row].max() > 1e-3
        a = np.vstack([np.asarray(A, float) for A, _, _ in lexopt.rows_of(n, p)])[row]
        out["moved_off_bound", b] = r["x"] + (1e-6 if act[row] == 1 else -1e-6) * a / (a @ a)
    return out


CASES = ["noise", "stopped_early", "levels_swapped", "neighbour", "moved_off_bound"]


def rejected_figures(oracle):
    if "rejected" not in _cache:
        out = {}
        for name, f in FAMILIES.items():
            if not pinned(name):
                continue
            for (case, b), x in rejected_points(oracle, name).items():
                out[name, case, b] = float(lexopt.certificate(f["n"], problems_of(name)[b], x).max())
        _cache["rejected"] = out
    return _cache["rejected"]


@pytest.mark.parametrize("case", CASES)
def test_certificate_rejects(oracle, case):
    rej = {k: t for k, t in rejected_figures(oracle).items() if k[1] == case}
    for name, f in FAMILIES.items():
        if not pinned(name):
            continue
        have = sum(1 for k in rej if k[0] == name)  # no instance without its case
        assert have == len(f["seeds"]), (name, case, have)
    least = min(rej, key=rej.get)
    print(case, ": smallest rejected certificate", rej[least], "at", least, "of", len(rej))
    assert rej[least] >= 100 * lexopt.ACCEPT, (least, rej[least])


def test_acceptance_bounds_are_the_measured_ones(oracle):
    """ACCEPT = 1000 x the largest accepted figure (the oracle-backed driver and test_01.dat), at least 100 x below the smallest rejected one; the
    same for the direct multiplier check"""
    cert, lam = accepted_figures(oracle)
    d = golden_problem()
    accepted = max(max(cert.values()), float(lexopt.certificate(d["n"], d["objectives"], d["solution"]).max()))
    rejected = min(rejected_figures(oracle).values())
    print("certificate: largest accepted", accepted, "smallest rejected", rejected, "ACCEPT", lexopt.ACCEPT)
    assert lexopt.MEASURED_MAX_T / 10 <= accepted <= 1.5 * lexopt.MEASURED_MAX_T and lexopt.ACCEPT == 1000 * lexopt.MEASURED_MAX_T  # (the constant is the measurement)
    assert 100 * lexopt.ACCEPT <= rejected
    lam_accepted = max(fig["stationarity"] for fig in lam.values())
    lam_rejected = min(rejected_lambda_figures(oracle).values())
    print("lambda_check: largest accepted", lam_accepted, "smallest rejected", lam_rejected, "ACCEPT_LAMBDA", lexopt.ACCEPT_LAMBDA)
    assert lexopt.MEASURED_MAX_LAMBDA / 10 <= lam_accepted <= 1.5 * lexopt.MEASURED_MAX_LAMBDA and lexopt.ACCEPT_LAMBDA == 1000 * lexopt.MEASURED_MAX_LAMBDA
    assert 100 * lexopt.ACCEPT_LAMBDA <= lam_rejected


def rejected_lambda_figures(oracle):
    """the direct multiplier check on wrong inputs: the run's multipliers with x + 1e-6 N(0,1); its x with 1e-6 N(0,1) added to the multipliers of
    the active rows; x, working set and multipliers of instance b + 1 for problem b"""
    if "rejected_lambda" not in _cache:
        out = {}
        for name, f in FAMILIES.items():
            if not pinned(name):
                continue
            runs = oracle_runs(oracle, name, "cold")
            for b, (p, r) in enumerate(zip(problems_of(name), runs)):
                L, act = np.vstack(r["debug"]["lambda"]), np.concatenate(r["active"])
                out[name, "noise_x", b] = lexopt.lambda_check(f["n"], p, r["x"] + 1e-6 * _noise(name, b, f["n"], 0), act, L)["stationarity"]
                noisy = L + 1e-6 * _noise(name, b, L.size, 1).reshape(L.shape) * (L != 0)
                out[name, "noise_lambda", b] = lexopt.lambda_check(f["n"], p, r["x"], act, noisy)["stationarity"]
                o = runs[(b + 1) % len(runs)]
                out[name, "neighbour", b] = lexopt.lambda_check(f["n"], p, o["x"], np.concatenate(o["active"]), np.vstack(o["debug"]["lambda"]))["stationarity"]
        _cache["rejected_lambda"] = out
    return _cache["rejected_lambda"]


def test_lambda_check_rejects(oracle):
    rej = rejected_lambda_figures(oracle)
    for case in ("noise_x", "noise_lambda", "neighbour"):
        sub = {k: t for k, t in rej.items() if k[1] == case}
        least = min(sub, key=sub.get)
        print(case, ": smallest rejected stationarity of the multipliers", sub[least], "at", least)
        assert sub[least] >= 100 * lexopt.ACCEPT_LAMBDA, (least, sub[least])


def test_consistency_checks_notice_a_wrong_report(oracle):
    """consistent() on tampered reports of one run: v off by 1e-6, an inactive row reported active, the wrong bound, a violated row reported inactive"""
    f, p, r = FAMILIES["small"], problems_of("small")[0], oracle_runs(oracle, "small", "cold")[0]
    act, v = np.concatenate(r["active"]), np.concatenate(r["v"])
    lexopt.assert_consistent(lexopt.consistent(f["n"], p, r["x"], act, v))
    general = np.arange(act.size) >= f["dims"][0]
    on = int(np.flatnonzero(((act == 1) | (act == 2)) & general)[0])
    off = int(np.flatnonzero((act == 0) & general)[0])
    tampered = []
    w = v.copy(); w[on] += 1e-6; tampered.append((act, w))
    a = act.copy(); a[off] = 2; tampered.append((a, v))
    a = act.copy(); a[on] = 3 - a[on]; tampered.append((a, v))
    viol = int(np.flatnonzero(v != 0)[0])
    a = act.copy(); a[viol] = 0; tampered.append((a, v))
    for a, w in tampered:
        with pytest.raises(AssertionError):
            lexopt.assert_consistent(lexopt.consistent(f["n"], p, r["x"], a, w))


# --- what the certificate found -----------------------------------------------------------------------------------------------------------------

FIRST_WRONG_SIGN_DEFECT = ("deactivate_first_wrong_sign with simple bounds can end with status 0 at a point that is not optimal: the scan of the fixed "
                           "variables reads the first general rows' multipliers (reference lexlse.h:599-600, kept on purpose: include/lexls_hip.h, "
                           "lexls_lse_sensitivity), so a simple bound keeps a wrong-sign multiplier")


@pytest.mark.xfail(strict=True, reason=FIRST_WRONG_SIGN_DEFECT)
def test_first_wrong_sign_with_simple_bounds_smallest_reproducer(oracle):
    """n = 3, dims (2, 2, 3), P.lsi_problem(2, ...): the default rule's x certifies at 9.4e-16, the first-wrong-sign rule's, also status 0, at 0.339"""
    n, p = 3, P.lsi_problem(2, 3, [2, 2, 3])
    plain, first = oracle.lsi_run(n, p), oracle.lsi_run(n, p, deactivate_first_wrong_sign=1)
    assert plain["info"]["status"] == 0 and first["info"]["status"] == 0
    assert lexopt.certificate(n, p, plain["x"]).max() <= lexopt.ACCEPT
    t = lexopt.certificate(n, p, first["x"])
    print("certificate of the first-wrong-sign run", t)
    assert t.max() <= lexopt.ACCEPT, t
