"""The references of the many-cotangent adjoint of the regularized LexLSE solve agree on the CPU (tests/adjoint_reg_multi_cases.py): G M_reg and
G N_reg from unit solves on the oracle (A) against adjoint_reg_from_factor one cotangent at a time (B); the largest gap is D_CPU, from which the
GPU tolerance follows.  Also: the cases sit where their docstring says on the placement rule, and the rule of lexls_lds.h and its Python
restatement agree over a grid of shapes (a stand-alone host program).  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_reg_cases as RC
import adjoint_reg_multi_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_references_agree_and_the_tolerance_follows_from_their_gap():
    worst = 0.0
    for name in XC.NAMES:
        for t in XC.types_of(name):
            g = XC.cpu_gap(name, t)
            print(f"{name:<15} type {t}  gap {g:.1e}")
            assert g <= XC.D_CPU, (name, t, g)
            worst = max(worst, g)
    print(f"D_CPU measured {worst:.2e}, recorded {XC.D_CPU:.2e}, TOL {XC.TOL:.2e}")
    assert XC.TOL == max(10.0 * XC.D_CPU, 1e-12) and XC.TOL <= 1e-10


def test_the_cases_the_sets_and_the_gates_are_there():
    assert XC.NAMES == RC.NAMES + ("edge_lds", "edge", "deep")
    for name in XC.NAMES:
        assert XC.sets_of(name)[:2] == ("identity", "3")
        assert ("65" in XC.sets_of(name)) == (name in XC.SMALL or name == "edge")
        for t in XC.types_of(name):
            assert t in RC.TYPES
        c = XC.build(name, XC.types_of(name)[0])
        f = c["factors"]
        assert f[0, 0] == 0.0 and 0.0 < abs(f[1, 1]) < 1e-15  # an exact zero at level 0 of problem 0, one below the gate at level 1 of problem 1
        assert c["G"]["identity"].shape == (c["lod"].shape[0], c["n"], c["n"]) and c["G"]["3"].shape[1] == 3
        assert np.abs(c["A"]["3"][0]).max() > 1e-3
    for name in XC.NEW:
        assert XC.build(name, 1)["lod"].shape[0] == 3
    # the first cotangent-independent check of (A): row c of the identity set is column c of M_reg
    c = XC.build("ik", 1)
    np.testing.assert_array_equal(c["A"]["identity"][0][2][:, :60], c["maps"][2][0])
    # the damping shows: M_reg differs from the undamped solve map's reference (tests/adjoint_cases.py: M^T g for the case's g)
    import adjoint_cases as AC
    assert np.abs(c["g"][2] @ c["maps"][2][0] - AC.build("ik")["A"][0][2][:60]).max() > 1e-3


def test_where_the_cases_sit_on_the_placement_rule():
    forms = {name: XC.build(name, XC.types_of(name)[0])["variant"] for name in XC.NAMES}
    for name in XC.SMALL + ("ik", "edge_lds"):
        assert forms[name] == XC.LDS, name
    assert forms["edge"] == XC.HBM and forms["deep"] == XC.HBM
    assert forms["wide"] == "solve_adjoint_reg<64,hbm> x K"  # the state alone is over the limit: the single-cotangent kernel once per cotangent
    w = RC.WIDE
    assert XC.lds_bytes(w["n"], sum(w["dims"]), len(w["dims"]), False) > XC.LDS_LIMIT
    # edge is the smallest nVar on the hbm side at its cap and nObj, edge_lds the one before it
    e = XC.NEW["edge"]
    assert XC.NEW["edge_lds"]["n"] == e["n"] - 1 and XC.NEW["edge_lds"]["dims"] == e["dims"]
    cap, nobj = sum(e["dims"]), len(e["dims"])
    assert all(XC.variant(n, cap, nobj) == XC.LDS for n in range(1, e["n"])) and XC.variant(e["n"], cap, nobj) == XC.HBM
    # deep: D reaches an order above 64 on a level that is damped for some problem (types 1, 5: W = [R | T], order nVar - Fc)
    d = XC.build("deep", 1)
    orders = [d["n"] - int(d["ref"]["fcol"][b, k]) for b in range(3) for k in range(3) if d["ref"]["rank"][b, k] > 0 and abs(d["factors"][b, k]) >= 1e-15]
    assert max(orders) > 64, orders
    assert 135000 <= XC.lds_bytes(40, 60, 5, True) <= 136000  # the IK shape: one wavefront per CU in the lds form


def fit_check(tmp_path, shapes):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "adjoint_reg_multi_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "adjoint_reg_multi_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n} {cap} {nobj}\n" for n, cap, nobj in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return [(v, int(a), int(b)) for v, a, b in (line.split("|") for line in lines)]


def test_the_header_rule_and_its_restatement_agree_over_a_grid(tmp_path):
    shapes = [(n, cap, nobj) for n in (1, 2, 3, 7, 16, 39, 40, 41, 51, 52, 53, 54, 64, 65, 70, 85, 86, 100, 128) for cap in (1, 12, 48, 60, 75, 90, 105, 106, 200)
              for nobj in (1, 2, 3, 5, 8)]
    res = fit_check(tmp_path, shapes)
    seen = set()
    for (n, cap, nobj), (name, with_m, without) in zip(shapes, res):
        assert (name, with_m, without) == (XC.variant(n, cap, nobj), XC.lds_bytes(n, cap, nobj, True), XC.lds_bytes(n, cap, nobj, False)), (n, cap, nobj)
        assert with_m + 15 >= without + 8 * RC.matrix_doubles(n, nobj)
        seen.add(name)
    assert seen == {XC.LDS, XC.HBM, "solve_adjoint_reg<64,lds> x K", "solve_adjoint_reg<64,hbm> x K"}, seen
