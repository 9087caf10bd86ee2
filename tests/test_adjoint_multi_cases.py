"""The references of the multi-cotangent adjoint agree on the CPU (tests/adjoint_multi_cases.py): per cotangent, M^T g and N^T g from unit
solves on the oracle (A) against the numpy restatement on the oracle's factor (B), the identity cotangents against M and N themselves; for the
large cases and `beyond`, (B) against the dot-product identities.  The largest discrepancy is D_CPU_MULTI, from which TOL_MULTI follows.
The host-side fit rule (lexls_lds.h: adjoint_multi_form) sends every case to the form the GPU test expects.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_multi_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {name: MC.build(name) for name in MC.NAMES}


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
        base = MC.AC.build(c["name"])["B"] if c["name"] != "beyond" else None
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


def test_the_fit_rule_sends_every_case_to_its_form(cases, tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "adjoint_multi_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "adjoint_multi_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    shapes = [(c["n"], sum(c["caps"])) for c in cases.values()]
    run = subprocess.run([exe], input="".join(f"{n} {cap}\n" for n, cap in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    limit = 160 * 1024
    for (name, c), (n, cap), line in zip(cases.items(), shapes, lines):
        form, staged, hbm = line.split("|")
        print(f"{name:<9} n={n:<4} cap={cap:<4} {form:<32} staged {int(staged):>7} B  state alone {int(hbm):>7} B")
        assert form == MC.FORMS[name], (name, line)
        assert int(hbm) >= 8 * 65 * (n + cap) and int(staged) >= int(hbm) + 8 * cap * n  # the state [index][lane], ld 65; the factor's columns
        want = "solve_adjoint_multi<64,staged>" if int(staged) <= limit else ("solve_adjoint_multi<64,hbm>" if int(hbm) <= limit else "solve_adjoint<64> x K")
        assert form == want
    assert MC.FORMS["ik"].endswith("staged>") and MC.FORMS["wide"].endswith("staged>") and MC.FORMS["large"].endswith("hbm>") and MC.FORMS["beyond"] == "solve_adjoint<64> x K"
