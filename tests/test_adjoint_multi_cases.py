"""The references of the multi-cotangent adjoint agree on the CPU (tests/adjoint_multi_cases.py): per cotangent, M^T g and N^T g from unit
solves on the oracle (A) against the numpy restatement on the oracle's factor (B), the identity cotangents against M and N themselves; for the
large cases and `beyond`, (B) against the dot-product identities.  The largest discrepancy is D_CPU_MULTI, from which TOL_MULTI follows.
The host-side fit rule (lexls_lds.h: adjoint_multi_form) sends every case to the form the GPU test expects; its Python restatement
(MC.lds_bytes) agrees with it byte for byte, and the four fit_* cases sit on both sides of its two switches at n = 40.  The host-side dispatch
plan names the producers of the kept factors (MC.PRODUCERS).  No GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_multi_cases as MC
from scripts import record_dispatch_table as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {name: MC.build(name) for name in MC.NAMES + MC.FIT_NAMES}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for c in cases.values():
        print(MC.summary(c))
    print(f"D_CPU_MULTI measured {worst:.2e}, recorded {MC.D_CPU_MULTI:.2e}, TOL_MULTI {MC.TOL_MULTI:.2e}")
    assert MC.TOL_MULTI == max(10.0 * MC.D_CPU_MULTI, 1e-12) and MC.TOL_MULTI <= 1e-10
    assert max(10.0 * worst, 1e-12) <= MC.TOL_MULTI, "the references disagree by more than the recorded D_CPU_MULTI allows for: re-measure (or replace the data)"


def test_the_cotangent_sets_are_what_they_are_for(cases):
    for c in cases.values():
        R, n = c["R"], c["n"]
        assert R.shape == (c["lod"].shape[0], 65, n)
        np.testing.assert_array_equal(MC.select("1", R)[:, 0], c["g"])            # K = 1: the case's own g
        assert [MC.select(s, R).shape[1] for s in MC.SETS] == [1, 3, 64, 65, n]   # the tile edge, a second tile with one live lane, the Jacobian
        np.testing.assert_array_equal(MC.select("identity", R)[0], np.eye(n))
        for s in MC.SETS:
            assert MC.select_ref(s, c, 0).shape == (R.shape[0], MC.select(s, R).shape[1], sum(c["caps"]))
            assert MC.select_ref(s, c, 1).shape == (R.shape[0], MC.select(s, R).shape[1], n)
        # cotangent 0 of the master set is the single-cotangent case: reference (B) of adjoint_cases.py, bit for bit
        base = MC.AC.build(c["name"])["B"] if c["name"] in MC.AC.CASES else None
        if base is not None:
            np.testing.assert_array_equal(c["B_R"][0][:, 0], base[0])
            np.testing.assert_array_equal(c["B_R"][1][:, 0], base[1])


def test_the_identity_cotangents_reproduce_m_and_n(cases):
    for c in cases.values():
        if c["large"]:
            continue
        for which, mat in ((0, c["M"]), (1, c["N"])):
            np.testing.assert_array_equal(c["ref_identity"][which], mat)  # row i of the Jacobian = row i of M (of N)
            assert MC.gap(c["B_identity"][which], mat) <= MC.TOL_MULTI / 10
        assert np.abs(c["M"]).max() > 1e-3 or c["name"] == "fixed"


def test_absent_rows_and_slots_are_zero(cases):
    for c in cases.values():
        m = c["dims"].sum(axis=1)
        nf = c["fixed"]["nfixed"] if c["fixed"] else np.zeros(len(m), np.uint32)
        for s in MC.SETS:
            rhs, fixed = MC.select_ref(s, c, 0), MC.select_ref(s, c, 1)
            for b in range(len(m)):
                assert not rhs[b, :, m[b]:].any() and not fixed[b, :, nf[b]:].any(), (c["name"], s, b)


def test_beyond_is_what_it_is_for(cases):
    c = cases["beyond"]
    assert (c["ref"]["rank"] == [[150, 50], [150, 50]]).all() and (c["ref"]["totalrank"] == 200).all()
    assert c["large"] and len(c["pairs"]) == 3
    for pair in c["pairs"]:
        assert np.abs(pair[1]).max() > 1e-3
    assert MC.identities(c, c["R"], c["B_R"][0]) <= MC.TOL_MULTI / 10


def fit_check(tmp_path, shapes):
    """tests/adjoint_multi_fit_check.cpp on (n, cap) pairs -> [(form, bytes staged, bytes hbm)]"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "adjoint_multi_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "adjoint_multi_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n} {cap}\n" for n, cap in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return [(form, int(staged), int(hbm)) for form, staged, hbm in (line.split("|") for line in lines)]


def test_the_fit_rule_sends_every_case_to_its_form(cases, tmp_path):
    shapes = [(c["n"], sum(c["caps"])) for c in cases.values()]
    limit = 160 * 1024
    for (name, c), (n, cap), (form, staged, hbm) in zip(cases.items(), shapes, fit_check(tmp_path, shapes)):
        print(f"{name:<16} n={n:<4} cap={cap:<4} {form:<32} staged {staged:>7} B  state alone {hbm:>7} B")
        assert form == MC.FORMS[name], (name, form)
        assert hbm >= 8 * 65 * (n + cap) and staged >= hbm + 8 * cap * n  # the state [index][lane], ld 65; the factor's columns
        want = "solve_adjoint_multi<64,staged>" if staged <= limit else ("solve_adjoint_multi<64,hbm>" if hbm <= limit else "solve_adjoint<64> x K")
        assert form == want
        assert (MC.form(n, cap), MC.lds_bytes(n, cap, True), MC.lds_bytes(n, cap, False)) == (form, staged, hbm)  # the Python restatement
    assert MC.FORMS["ik"].endswith("staged>") and MC.FORMS["wide"].endswith("staged>") and MC.FORMS["large"].endswith("hbm>") and MC.FORMS["beyond"] == "solve_adjoint<64> x K"
    for name in ("fixed_wide", "fixed_rank_def", "fixed_ragged", "fixed_tall"):
        assert MC.FORMS[name] == MC.STAGED


def test_the_fit_cases_sit_on_both_sides_of_the_two_switches(cases, tmp_path):
    """the boundaries come from the rule (the C++ one, through the stand-alone program), not from arithmetic done by hand"""
    n, limit = MC.FIT_N, 160 * 1024
    caps = list(range(1, 400))
    rule = fit_check(tmp_path, [(n, cap) for cap in caps])
    forms = [r[0] for r in rule]
    for cap, (form, staged, hbm) in zip(caps, rule):
        assert (MC.form(n, cap), MC.lds_bytes(n, cap, True), MC.lds_bytes(n, cap, False)) == (form, staged, hbm), cap
    last_staged = max(cap for cap, f in zip(caps, forms) if f == MC.STAGED)
    last_hbm = max(cap for cap, f in zip(caps, forms) if f == MC.HBM)
    assert forms == [MC.STAGED] * last_staged + [MC.HBM] * (last_hbm - last_staged) + [MC.SINGLE] * (len(caps) - last_hbm)  # monotone: two switches
    assert MC.FIT_CAPS == dict(fit_staged_last=last_staged, fit_hbm_first=last_staged + 1, fit_hbm_last=last_hbm, fit_single_first=last_hbm + 1)
    assert [MC.FORMS[k] for k in MC.FIT_NAMES] == [MC.STAGED, MC.HBM, MC.HBM, MC.SINGLE]
    assert MC.LDS_LIMIT == limit and rule[last_staged - 1][1] <= limit < rule[last_staged][1] and rule[last_hbm - 1][2] <= limit < rule[last_hbm][2]
    print(f"n = {n}: staged up to cap {last_staged} ({rule[last_staged - 1][1]} B, then {rule[last_staged][1]} B), hbm up to cap {last_hbm} "
          f"({rule[last_hbm - 1][2]} B, then {rule[last_hbm][2]} B) of {limit} B")
    for name in MC.FIT_NAMES:
        c = cases[name]
        cap, rank = sum(c["caps"]), c["ref"]["rank"]
        assert cap == MC.FIT_CAPS[name] and c["n"] == n and c["lod"].shape == (2, n + 1, cap) and not c["fixed"] and not c["large"]
        assert (rank[:, :4] == [12, 12, 12, 4]).all() and not rank[:, 4:].any() and (c["ref"]["totalrank"] == n).all()
        # the cotangents weigh the last pivot column and the last rows that carry anything: the reference is not 0 in the last live row of the
        # last level that has rank, for the sets "3" and "65" alike, and every cotangent has weight on the variable of the last pivot column
        last_row = 4 * 12 - 1
        for st in ("3", "65"):
            ref = MC.select_ref(st, c, 0)
            assert np.abs(ref[:, :, last_row]).min() > 1e-6, (name, st)
            assert not ref[:, :, 4 * 12:].any()  # the levels behind them have no rank: exactly 0
        assert np.abs(c["R"]).min() > 0


def test_the_dispatch_plan_names_the_producers(cases, tmp_path):
    """MC.PRODUCERS (adjoint_cases.PRODUCERS and this file's cases) against the host-side dispatch plan (lexls_amd/csrc/lexls_dispatch.h through
    tests/dispatch_plan_check.cpp and the query lines of scripts/record_dispatch_table.py): every named producer is the plan's for its policy, and
    no policy gives a new case a producer that is not named.  A dispatch rule that moves fails here, before any device run"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "dispatch_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "lexls_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    with open(R.TABLE) as f:
        cus = json.load(f)["cu_count"]  # the device the recorded table stands for: wave capacity = CUs x 8
    assert set(MC.PRODUCERS) == set(cases)
    keys = [(name, policy) for name in cases for policy in range(11)]
    lines = []
    for i, (name, policy) in enumerate(keys):
        c = cases[name]
        lines.append(R.query_line(dict(kind="lse", id=i, caps=c["caps"], dims=c["dims"], n=c["n"], batch=c["lod"].shape[0], policy=policy, keep=1, mode="fs",
                                       fixed=int(bool(c["fixed"])), guard=0, reg=0, qtol0=0, align8=0), cus))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(keys)
    plan = {key: line.split("|")[1] for key, line in zip(keys, out)}
    for name, table in MC.PRODUCERS.items():
        for policy, producer in table.items():
            assert plan[(name, policy)] == producer, (name, policy, plan[(name, policy)])
    new = ["fixed_wide", "fixed_rank_def", "fixed_ragged", "fixed_tall"] + MC.FIT_NAMES
    for name in new:  # every policy that gives the shape a distinct producer is named
        assert {plan[(name, policy)] for policy in range(11)} == set(MC.PRODUCERS[name].values()), name
        print(f"{name:<16} {MC.PRODUCERS[name]}")
    assert set(MC.PRODUCERS["fixed_wide"].values()) == set(MC.PRODUCERS["fixed_tall"].values()) == {"lqr_generic<256,lds>"}
    for name in ("fixed_rank_def", "fixed_ragged"):
        assert set(MC.PRODUCERS[name].values()) == {"lqr_wave<41,12>", "lqr_generic<64,lds>", "lqr_quad<3,12,factor,fixed>"}
