"""The two references of the adjoint of the regularized LexLSE solve agree on the CPU (tests/adjoint_reg_cases.py): M_reg^T g, N_reg^T g from
unit solves on the oracle (A) against the numpy reverse pass on the oracle's factor (B).  The largest discrepancy is D_CPU, from which the GPU
tolerance follows.  Also: the damped solve is affine for the served types and visibly not for the CG type 2; which form type 1 took at every
level; the host's lds/hbm rule on both sides of its switch.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_reg_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {(name, t): RC.build(name, t) for name in RC.NAMES for t in RC.types_of(name)}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for (name, t), c in cases.items():
        print(f"{name:<15} type {t}  gap {c['gap']:.1e}")
        assert c["gap"] <= RC.D_CPU, (name, t, c["gap"])
    print(f"D_CPU measured {worst:.2e}, recorded {RC.D_CPU:.2e}, TOL {RC.TOL:.2e}")
    assert RC.TOL == max(10.0 * RC.D_CPU, 1e-12) and RC.TOL <= 1e-10


def test_every_case_and_type_is_there_and_the_factors_cover_the_gate(cases):
    assert set(RC.NAMES) == {"base", "used_up", "one_row", "rank_def", "ragged", "fixed", "fixed_rank_def", "fixed_ragged", "ik", "wide"}
    assert RC.TYPES == (1, 3, 4, 5, 8, 9) and RC.types_of("wide") == (1, 5) and all(RC.types_of(n) == RC.TYPES for n in RC.NAMES if n != "wide")
    assert cases[("ik", 1)]["lod"].shape[0] == 8
    for (name, t), c in cases.items():
        f = c["factors"]
        assert f[0, 0] == 0.0 and 0.0 < abs(f[1, 1]) < 1e-15                    # an exact zero, one below the gate
        live = f[np.abs(f) >= 1e-15]
        assert live.min() >= 0.1 and live.max() <= 0.5
        assert len({tuple(row) for row in f.tolist()}) == f.shape[0]            # per-problem factors differ within the batch
        assert np.abs(c["A"][0]).max() > 1e-3
    # an undamped level in front of a damped one that reads the accumulated basis: problem 0 of every case with rank at levels 0 and 1
    for name in ("base", "one_row", "ik", "wide"):
        c = cases[(name, 1)]
        assert c["ref"]["rank"][0, 0] > 0 and c["ref"]["rank"][0, 1] > 0 and c["factors"][0, 1] > 0.05
    # the damping changes the gradient: against the unregularized references of tests/adjoint_cases.py
    import adjoint_cases as AC
    for t in RC.TYPES:
        assert np.abs(cases[("ik", t)]["A"][0] - AC.build("ik")["A"][0]).max() > 1e-3, t


def test_the_damped_solve_is_affine_for_the_served_types_and_not_for_cg():
    for name in ("base", "fixed_rank_def", "ik"):
        for t in RC.TYPES:
            for b in (0, 1, 2):
                d = RC.affine_defect(name, t, b)
                assert d <= 1e-13, (name, t, b, d)
    d = max(RC.affine_defect("ik", 2, b) for b in (2, 3))  # TIKHONOV_CG: ten CGLS iterations from x = 0 are no linear map of b
    print(f"type 2 on ik: affine defect {d:.2e}")
    assert d > 1e-8


def test_the_branch_table_of_type_1(cases):
    seen = set()
    for name in RC.NAMES:
        c = cases[(name, 1)]
        got = RC.tikhonov_branches(c["ref"], c["nf"], c["n"])
        assert got == [list(r) for r in RC.TIKHONOV_BRANCHES[name]], (name, got)
        for b, row in enumerate(got):
            for k, form in enumerate(row):
                if form != "-" and abs(c["factors"][b, k]) >= 1e-15:
                    seen.add(form)
    assert seen == {"dual", "primal"}  # both Fc + rank <= RC and its complement are reached by damped levels


def fit_check(tmp_path, shapes):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "adjoint_reg_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "adjoint_reg_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n} {cap} {nobj}\n" for n, cap, nobj in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return [(v, int(a), int(b), int(m), tuple(int(t) for t in served.split())) for v, a, b, m, served in (line.split("|") for line in lines)]


def test_the_host_rule_on_both_sides_of_its_switch(tmp_path):
    n, cap, nobj = RC.WIDE["n"], sum(RC.WIDE["dims"]), len(RC.WIDE["dims"])
    shapes = [(n - 1, cap, nobj), (n, cap, nobj), (70, cap, nobj), (40, 60, 5), (3, 7, 3)]
    res = fit_check(tmp_path, shapes)
    limit = 160 * 1024
    for (sn, scap, sobj), (variant, with_m, without, m, served) in zip(shapes, res):
        print(f"n={sn} cap={scap} nObj={sobj}: {variant} {with_m} B / {without} B, {m} doubles")
        assert served == RC.TYPES
        assert variant == ("solve_adjoint_reg<64,lds>" if with_m <= limit else "solve_adjoint_reg<64,hbm>")
        assert (variant, with_m, without, m) == (RC.variant(sn, scap, sobj), RC.lds_bytes(sn, scap, sobj, True), RC.lds_bytes(sn, scap, sobj, False),
                                                 RC.matrix_doubles(sn, sobj))  # the Python restatement
        assert with_m + 15 >= without + 8 * m and without <= limit  # (both are rounded up to 16 bytes)
        # the snapshots' share holds every level's m0 x (n - Fc) <= Fc (n - Fc) <= n^2 / 4
        assert m - 2 * sn * sn >= min(sobj, sn) * max(fc * (sn - fc) for fc in range(sn + 1))
    assert [r[0][-4:-1] for r in res] == ["lds", "hbm", "lds", "lds", "lds"]  # n = 85 | 86: the switch `wide` sits behind; 70 and the IK shape in LDS
