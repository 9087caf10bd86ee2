"""CPU: the three references of tests/tangent_cases.py agree — (A) the differentiated dense KKT system, (B) the kernels' steps in numpy on the
oracle's factor, (C) central differences of the oracle —, forward and reverse mode are transposes of one another, the GPU tolerance follows from
the references' own gap, and the placement rule of lexls_lds.h gives what the restatement gives on both sides of each switch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tangent_cases as TC
from conftest import ROOT


@pytest.fixture(scope="module")
def cases(oracle):
    return {nm: TC.build(nm) for nm in TC.CASES + TC.FIT_NAMES}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(t["gap"] for t in cases.values())
    for t in cases.values():
        print(TC.summary(t))
    print(f"D_CPU measured {worst:.2e}, recorded {TC.D_CPU:.2e}, TOL {TC.TOL:.2e}")
    assert worst <= TC.D_CPU * 1.0001, f"(A) and (B) are {worst:.3e} apart: D_CPU in tests/tangent_cases.py is out of date"
    assert worst >= TC.D_CPU / 2, "D_CPU is recorded far above what the references show: measure it again"
    assert TC.TOL == 10.0 * TC.D_CPU and TC.TOL <= 1e-10


def test_forward_and_reverse_mode_are_transposes(cases):
    """<g, dx> == <grad_lod(g), dlod> + <N^T g, dfixed> against the references of adjoint_matrix_cases and adjoint_cases"""
    for name in TC.CASES:
        print(f"{name}: duality gap {cases[name]['dual']:.2e}")
        assert cases[name]["dual"] <= TC.TOL, name


def test_flags_and_zeros(cases):
    for name in TC.CASES:
        t = cases[name]
        np.testing.assert_array_equal(t["case"]["flags"], np.asarray(TC.FLAGS[name], np.uint8))
        for b, f in enumerate(t["case"]["flags"]):
            assert f or not (t["A"][:, b].any() or t["B"][:, b].any())
    for name in TC.FIT_NAMES:
        assert cases[name]["case"]["flags"].all(), name


def test_fixed_variables_take_their_slot_and_free_variables_stay(cases):
    t = cases["fixed"]
    case = t["case"]
    for b in range(case["lod"].shape[0]):
        nf, fidx, _ = TC.fixed_of(case, b)
        for c in range(TC.NTAN):
            np.testing.assert_array_equal(t["A"][c, b][fidx], t["dfixed"][c, b][:nf])
            np.testing.assert_array_equal(t["B"][c, b][fidx], t["dfixed"][c, b][:nf])
    assert int(case["fixed"]["nfixed"][2]) == case["n"]  # the all-fixed problem: dx is dfixed in the variables' order, nothing else
    t = cases["ragged"]
    T = t["case"]["ref"]["totalrank"]
    assert (T < t["case"]["n"]).any()
    for b in np.nonzero(T < t["case"]["n"])[0]:
        free = [i for i in range(t["case"]["n"]) if TC.AM.position(t["case"]["ref"]["perm"][b], int(T[b]), i) >= T[b]]
        assert free and not t["A"][:, b][:, free].any() and not t["B"][:, b][:, free].any()


def test_nan_behind_a_problems_own_rows_and_slots_reaches_no_reference(cases):
    for name in ("ragged", "fixed"):
        t, case = cases[name], cases[name]["case"]
        dlod, dfixed = t["dlod"].copy(), t["dfixed"].copy()
        for b in range(case["lod"].shape[0]):
            dlod[:, b, :, int(case["dims"][b].sum()):] = np.nan
            dfixed[:, b, TC.fixed_of(case, b)[0]:] = np.nan
        for b in range(case["lod"].shape[0]):
            nf, fidx, fval = TC.fixed_of(case, b)
            ref = case["ref"]
            for c in range(TC.NTAN):
                got = TC.tangent_from_factor(case, ref, b, dlod[c, b], dfixed[c, b])[0]
                np.testing.assert_array_equal(got, t["B"][c, b])


@pytest.mark.parametrize("name", ["base", "fixed", "ik"])
def test_central_differences_confirm_the_kkt_reference(oracle, name):
    gap = TC.fd_gap(name)
    print(f"{name}: central differences (h = {TC.FD_H:g}) against (A): {gap:.2e} (bound {TC.FD_BOUND:.0e})")
    assert gap <= TC.FD_BOUND


def test_lsi_references_agree_and_the_tolerance_follows_from_their_gap(oracle):
    import lsi_adjoint_matrix_cases as LM
    worst = 0.0
    for name in LM.CASES:
        t = TC.lsi_build(name)
        print(f"LexLSI {name}: flags {t['flags'].tolist()} gap {t['gap']:.2e}")
        np.testing.assert_array_equal(t["flags"], np.asarray(LM.FLAGS[name], np.uint8))
        np.testing.assert_array_equal(t["flags"], t["case"]["flags"])
        for b, f in enumerate(t["flags"]):
            assert f or not (t["A"][:, b].any() or t["B"][:, b].any())
        worst = max(worst, t["gap"])
    assert worst <= TC.LSI_D_CPU * 1.0001 and worst >= TC.LSI_D_CPU / 2, worst
    assert TC.LSI_TOL == 10.0 * TC.LSI_D_CPU and TC.LSI_TOL <= 1e-10
    t = TC.lsi_build("empty_ws")  # an empty working set: differentiable, dx = 0
    assert t["flags"][1] == 1 and not t["A"][:, 1].any() and not t["case"]["active"][1].any()


def test_lsi_central_differences_through_the_whole_driver_confirm_the_kkt_reference(oracle):
    import lsi_adjoint_matrix_cases as LM
    worst = 0.0
    for name in LM.WITH_B:
        gap, held = TC.lsi_fd_gap(name)
        print(f"LexLSI {name}: central differences against (A) {gap:.2e} (bound {TC.LSI_FD_BOUND:.1e}), working sets held: {held}")
        assert held, name
        assert gap <= TC.LSI_FD_BOUND, name
        worst = max(worst, gap)
    assert worst >= TC.LSI_GAP_C / 2 and TC.LSI_FD_BOUND <= 1e-6


def test_lsi_duality_against_the_reverse_mode_reference(oracle):
    """<g, dx> == <grad_data(g), ddata> per instance, against reference (A) of lsi_adjoint_matrix_cases"""
    import lsi_adjoint_matrix_cases as LM
    for name in LM.CASES:
        t = TC.lsi_build(name)
        case = t["case"]
        for b in range(len(t["flags"])):
            for c in range(TC.LSI_NTAN):
                terms = np.concatenate([case["g"][b] * t["A"][c, b], -case["A"][b] * t["ddata"][c, b]])
                assert abs(terms.sum()) / max(1.0, float(np.abs(terms).sum())) <= TC.LSI_TOL, (name, b, c)


def test_lsi_nan_outside_the_working_set_reaches_no_reference(oracle):
    t = TC.lsi_build("general")
    case = t["case"]
    for b in range(len(t["flags"])):
        dd = t["ddata"][:, b].copy()
        dd[:, TC.inactive_entries(case, b)] = np.nan
        got = TC.lsi_reference_instance(case["n"], case["probs"][b], case["runs"][b]["active"], case["status"][b], dd)[0]
        np.testing.assert_array_equal(got, t["A"][:, b])


def require_cxx():
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed for the stand-alone placement check (tests/tangent_fit_check.cpp)"
    return cxx


def fit_check(tmp_path, shapes):
    """tests/tangent_fit_check.cpp on (n, cap, nObj) triples -> [(placement, bytes staged, bytes lds, bytes work, work doubles, bytes rhs)]"""
    cxx = require_cxx()
    exe = str(tmp_path / "tangent_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "tangent_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n} {cap} {k}\n" for n, cap, k in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return [(f[0], *(int(v) for v in f[1:])) for f in (ln.split("|") for ln in lines)]


def test_the_placement_rule_is_the_restatement_on_both_sides_of_each_switch(tmp_path):
    """the boundaries come from the rule (the C++ one, through the stand-alone program), and no launch asks for more LDS than a workgroup may"""
    n, limit = TC.FIT_N, TC.LDS_LIMIT
    caps = list(range(1, 400))
    rule = fit_check(tmp_path, [(n, cap, (cap + 11) // 12) for cap in caps])
    for cap, (place, staged, lds, work, doubles, rhs) in zip(caps, rule):
        assert (TC.placement(n, cap), TC.lds_bytes(n, cap, TC.STAGED), TC.lds_bytes(n, cap, TC.LDS), TC.lds_bytes(n, cap, TC.WORK)) == (place, staged, lds, work), cap
        asked = {TC.STAGED: staged, TC.LDS: lds, TC.WORK: work}[place]
        assert asked <= limit and rhs <= limit, cap
        assert doubles == 64 * (n + cap) and rhs == 8 * (3 * n + cap)
    places = [r[0] for r in rule]
    for name, cap in TC.FIT_CAPS.items():
        assert places[cap - 1] == TC.PLACEMENTS[name], name
    a, b = TC.FIT_CAPS["fit_staged_last"], TC.FIT_CAPS["fit_lds_last"]
    assert places[a - 1] == TC.STAGED and places[a] == TC.LDS and places[b - 1] == TC.LDS and places[b] == TC.WORK
    assert TC.FIT_CAPS["fit_lds_first"] == a + 1 and TC.FIT_CAPS["fit_work_first"] == b + 1
    assert places == sorted(places, key=[TC.STAGED, TC.LDS, TC.WORK].index)  # monotone in cap
    # the shapes of the other cases, and shapes far beyond any switch
    shapes = [(3, 7, 3), (40, 60, 5), (70, 90, 3), (127, 165, 5), (200, 200, 2), (1000, 3000, 4), (2000, 100, 1)]
    for (nn, cap, k), (place, staged, lds, work, _, rhs) in zip(shapes, fit_check(tmp_path, shapes)):
        assert place == TC.placement(nn, cap)
        assert {TC.STAGED: staged, TC.LDS: lds, TC.WORK: work}[place] <= limit, (nn, cap)
