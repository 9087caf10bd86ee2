"""The conditions that make tests/test_gpu_scale.py meaningful, asserted on the cases of tests/scale_cases.py from the oracle and the dispatch
plan alone (no GPU): the invariances the GPU file states are the oracle's own, every case keeps what it drew, the scaling does change pivot
decisions, and no GPU test can pass by having dropped the problems that matter."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import scale_cases as SC
import skip_cases as S
from oracle import oracle_ctypes as oracle
from scripts import record_dispatch_table as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIVOTS = ("rank", "fcol", "totalrank", "perm")
NO_FIXED = [nm for nm in SC.NAMES if S.CASES[nm].get("nfixed") is None]
UNIFORM = [nm for nm in SC.NAMES if SC.uniform(S.CASES[nm]) and S.CASES[nm]["n"] != 100]
TOLERANCE_CASES = [nm for nm in SC.NAMES if S.CASES[nm]["contract"] in ("T", "L")]


def test_the_case_table():
    """one case per instantiation of every factorization family, by the names skip_cases carries; what is left out is what the module text says"""
    assert set(S.CASES) - set(SC.NAMES) == {"wave_reg", "mfma_one_n44"}
    assert S.CASES["mfma_one_n44"]["kernel"] == S.CASES["mfma_one"]["kernel"]
    assert len({S.CASES[nm]["kernel"] for nm in SC.NAMES}) == len(SC.NAMES) == 25
    for nm in SC.NAMES:
        assert SC.batch_of(S.CASES[nm]) == (3 if S.CASES[nm]["n"] == 100 else 19)
    assert SC.POW2_K == (-100, 100) and SC.LEVEL_RANGE == 10
    assert len(SC.runs()) == 4 * len(SC.NAMES)
    assert set(S.CONSUMER_CASES) <= set(NO_FIXED)


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_case_keeps_what_it_drew(name):
    for gen in SC.GENERATORS:
        case, c = SC.build(name, gen), S.CASES[name]
        assert np.isfinite(case["lod"]).all()
        for key, v in case["ref"].items():
            assert np.isfinite(v).all(), (gen, key)
        assert case["kept"] >= S.RETENTION * case["drawn"], (gen, case["kept"], case["drawn"])
        if c["contract"] in ("T", "L") or gen == "levels":
            assert SC._stable(c, case["lod"], case["dims"], case["fixed"]).all(), gen
        if SC.uniform(c) and len(case["dims"]) == S.BATCH:
            assert case["deficient"] == list(S.DEFICIENT)
            short = case["ref_base"]["rank"][list(S.DEFICIENT), 0]
            assert (short == S._deficient_ranks(c["n"], c["caps"])[0]).all() and (short < min(c["caps"][0], c["n"])).all(), gen
        else:
            assert case["deficient"] == []


@pytest.mark.parametrize("k", SC.POW2_K)
@pytest.mark.parametrize("name", NO_FIXED)
def test_a_power_of_two_changes_no_bit_of_the_oracle(name, k):
    """[A | b] times 2^k under the tolerance times 4^k: x, ranks, first columns, total rank and permutation are those of k = 0, bit for bit"""
    scaled, plain = SC.build(name, "pow2", k), SC.build(name, "pow2")
    assert scaled["tol"] == np.ldexp(1e-12, 2 * k) and plain["tol"] == 1e-12
    np.testing.assert_array_equal(scaled["lod"], np.ldexp(plain["lod"], k))
    big = np.abs(scaled["lod"][scaled["lod"] != 0.0])
    assert 1e-40 < big.min() and big.max() < 1e40  # squared norms stay within 1e+-80: nowhere near overflow, underflow or subnormals
    for key in PIVOTS + ("x",):
        np.testing.assert_array_equal(scaled["ref"][key].view(np.uint64 if key == "x" else np.uint32), plain["ref"][key].view(np.uint64 if key == "x" else np.uint32),
                                      err_msg=key)
    if "sens" in scaled:
        np.testing.assert_array_equal(scaled["sens"], plain["sens"])


@pytest.mark.parametrize("name", [nm for nm in SC.NAMES if nm not in NO_FIXED])
def test_pow2_with_fixed_variables_keeps_the_fixed_values(name):
    """only [A | b] is scaled, the fixed values are left alone; the GPU file takes the expectation of these cases from the oracle on the same
    scaled data, not from an invariance, so nothing is asserted about the oracle's x here beyond its pivots"""
    for k in SC.POW2_K:
        scaled, plain = SC.build(name, "pow2", k), SC.build(name, "pow2")
        assert scaled["fixed"] is plain["fixed"] and scaled["fixed"]["nfixed"].max() > 0
        np.testing.assert_array_equal(scaled["lod"], np.ldexp(plain["lod"], k))
        for key in ("rank", "fcol", "totalrank"):
            np.testing.assert_array_equal(scaled["ref"][key], plain["ref"][key], err_msg=key)


@pytest.mark.parametrize("name", SC.NAMES)
def test_level_scaling_changes_no_bit_of_the_oracles_x(name):
    case = SC.build(name, "levels")
    for key in PIVOTS:
        np.testing.assert_array_equal(case["ref"][key], case["ref_base"][key], err_msg=key)
    np.testing.assert_array_equal(case["ref"]["x"].view(np.uint64), case["ref_base"]["x"].view(np.uint64))
    rng = SC.LEVEL_RANGE_OF.get(name, SC.LEVEL_RANGE)
    assert np.abs(case["exps"]).max() <= rng
    for b in range(len(case["dims"])):
        np.testing.assert_array_equal(case["lod"][b], SC.scale_levels(case["base"][b], case["dims"][b], case["exps"][b]))
    assert (case["exps"] != 0).any(axis=1).all()  # every problem is in other units
    if len(case["dims"]) == S.BATCH:
        assert case["exps"].min() <= -rng + 2 and case["exps"].max() >= rng - 2  # the range is used


@pytest.mark.parametrize("name", UNIFORM)
def test_four_neighbours_with_four_different_exponent_rows(name):
    e = SC.build(name, "levels")["exps"]
    assert any(len({tuple(r) for r in e[i:i + 4].tolist()}) == 4 for i in range(0, len(e) - 3, 4))


@pytest.mark.parametrize("name", SC.NAMES)
def test_decades_change_pivot_decisions(name):
    """every problem's column norms of A spread over more than three decades, and in every case some problem's first pivot is another variable
    than the first pivot of its unscaled base"""
    case = SC.build(name, "decades")
    ratio = SC.column_norm_ratio(case)
    assert (ratio > 1e3).all(), ratio.min()
    for b in range(len(case["dims"])):
        np.testing.assert_array_equal(case["lod"][b], SC.scale_decades(case["base"][b], case["col"][b], case["row"][b]))
    assert 1e-3 <= case["col"].min() and case["col"].max() <= 1e3 and 1e-2 <= case["row"].min() and case["row"].max() <= 1e2
    assert (SC.first_pivot(case, case["ref"]) != SC.first_pivot(case, case["ref_base"])).any()


@pytest.mark.parametrize("name", TOLERANCE_CASES)
def test_tolerance_cases_carry_their_sensitivity(name):
    """three draws of +-1.1e-16 relative on the data, the oracle alone; it is a lower estimate of what rounding does, never zero on these data"""
    for gen in SC.GENERATORS:
        case = SC.build(name, gen)
        assert case["sens"].shape == (len(case["dims"]),) and np.isfinite(case["sens"]).all(), gen
    assert (SC.build(name, "decades")["sens"] > 0).any()


def test_guard_estimates_of_the_decades_problems():
    """the accuracy guard's estimate, computed from the oracle's factor as scripts/calibrate_guard.py does, is beyond the default threshold for
    every kept problem of qtol_guard / decades: include/lexls_hip.h's "it flags every badly scaled problem too" is what the GPU test may assert"""
    case = SC.build("qtol_guard", "decades")
    est = SC.guard_estimates(case)
    print(f"estimates {est.min():.3g} .. {est.max():.3g}")
    assert (est > S.GUARD_THRESHOLD).all(), est


def test_planned_kernels(tmp_path):
    """each case's expected kernel name is what the host-side dispatch plan (lexls_amd/csrc/lexls_dispatch.h through tests/dispatch_plan_check.cpp
    and the query lines of scripts/record_dispatch_table.py) gives for its shape, policy and switches; the rank tolerance is no input of the plan"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "dispatch_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "lexls_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    with open(R.TABLE) as f:
        cus = json.load(f)["cu_count"]
    lines = []
    for i, nm in enumerate(SC.NAMES):
        c = SC.build(nm, "decades")
        lines.append(R.query_line(dict(kind="lse", id=i, caps=c["caps"], dims=c["dims"], n=c["n"], batch=len(c["dims"]), policy=c["policy"], keep=int(c["keep"]), mode="fs",
                                       fixed=int(bool(c["fixed"])), guard=c["guard"], reg=0, qtol0=0, align8=0), cus))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(SC.NAMES)
    for nm, line in zip(SC.NAMES, out):
        assert line.split("|")[1] == S.CASES[nm]["kernel"], (nm, line)


@pytest.mark.parametrize("name", S.CONSUMER_CASES)
def test_consumer_references(name):
    """the two CPU references of every family agree on the decades data within the recorded D_CPU, from which the device tolerance follows
    (10 x, never the unit-scale TOLs); both kinds of problems occur: rank-stable ones and the two exactly rank-deficient slots"""
    case, want = SC.build(name, "decades"), SC.consumers(name)
    print(SC.consumer_summary(name))
    for fam, gap in want["gaps"].items():
        assert gap <= SC.CONSUMER_D_CPU[fam], (fam, gap)
        assert SC.CONSUMER_TOL[fam] == 10.0 * SC.CONSUMER_D_CPU[fam] and SC.CONSUMER_TOL[fam] <= 1e-6
    flags = want["flags"]
    assert flags.sum() >= len(flags) / 2 and not flags[list(S.DEFICIENT)].any()
    assert not want["GA"][flags == 0].any() and not want["TA"][:, flags == 0].any()
    assert np.abs(want["TA"][:, flags == 1]).max() > 0 and np.abs(want["XA"]).max() > 0
    assert np.isfinite(want["ln1"]).all() and np.isfinite(want["mult"]).all()


def test_consumer_tolerances_are_ten_times_the_largest_gap():
    worst = {fam: max(SC.consumers(nm)["gaps"][fam] for nm in S.CONSUMER_CASES) for fam in SC.CONSUMER_D_CPU}
    for fam, d in SC.CONSUMER_D_CPU.items():
        assert worst[fam] <= d <= 1.25 * worst[fam], (fam, worst[fam], d)  # rounded up, not padded


def test_lsi_case_is_solved_by_the_oracle_driver():
    """every instance ends PROBLEM_SOLVED (status 0) within the default limits, at least one deactivates a constraint, every general level of
    every instance is scaled by its own power of two in [-10, 10], bounds included, and level 0 stays simple bounds"""
    probs, exps = SC.lsi_problems(), SC.lsi_exponents()
    assert len(probs) == SC.LSI_INSTANCES == 6
    assert (exps[:, 0] == 0).all() and np.abs(exps).max() <= 10 and (exps[:, 1:] != 0).any(axis=1).all() and len({tuple(r) for r in exps.tolist()}) == 6
    infos = [oracle.lsi_run(SC.LSI_N, objs)["info"] for objs in probs]
    print([(i["iterations"], i["activations"], i["deactivations"]) for i in infos])
    assert all(i["status"] == 0 for i in infos)
    assert any(i["deactivations"] > 0 for i in infos)
    for i, objs in enumerate(probs):
        plain = SC.P.lsi_problem(SC.LSI_SEED + i, SC.LSI_N, SC.LSI_DIMS, simple_bounds=True)
        assert "var" in objs[0] and np.array_equal(objs[0]["lb"], plain[0]["lb"])
        for k in range(1, len(SC.LSI_DIMS)):
            for key in ("A", "lb", "ub"):
                np.testing.assert_array_equal(objs[k][key], plain[k][key] * 2.0 ** int(exps[i, k]))


def test_measured_table_is_current():
    """the MEASURED table of the module text is what `python tests/scale_cases.py` prints"""
    for nm, g, k in SC.runs():
        assert SC.summary(SC.build(nm, g, k)) in SC.__doc__, (nm, g, k)
    for nm in S.CONSUMER_CASES:
        assert SC.consumer_summary(nm) in SC.__doc__, nm
