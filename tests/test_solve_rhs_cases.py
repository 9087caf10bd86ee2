"""The two references of lexls_lse_solve_rhs agree on the CPU (tests/solve_rhs_cases.py): the oracle solving [A | b_new] from scratch (a) against
the numpy forward pass over the oracle's kept factor (b), plain and damped.  Their largest discrepancy is D_CPU, from which the GPU tolerance
follows.  Also: the transposition identity against the numpy reverse passes, the affine defect of the CG type 2 (the refusal), the coverage of
the cases, the jvp comparison's figures, the host's placement rules on both sides of each switch.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_reg_cases as RC
import solve_rhs_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {(name, t): SC.build(name, t) for name in SC.NAMES for t in SC.types_of(name)}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for (name, t), c in cases.items():
        print(f"{name:<15} type {t}  gap {c['gap']:.1e}  transposition {c['trans']:.1e}")
        assert c["gap"] <= SC.D_CPU, (name, t, c["gap"])
    print(f"D_CPU measured {worst:.2e}, recorded {SC.D_CPU:.2e}, TOL {SC.TOL:.2e}")
    assert worst >= SC.D_CPU / 2  # the recorded figure is the measured one, rounded up — not a bound picked in advance
    assert SC.TOL == 10.0 * SC.D_CPU and SC.TOL <= 1e-10


def test_the_transposition_identity_holds_to_rounding(cases):
    for (name, t), c in cases.items():
        assert c["trans"] <= SC.D_CPU, (name, t, c["trans"])


def test_the_affine_defect_of_type_2_stays_large():
    d = max(RC.affine_defect("ik", 2, b) for b in (2, 3))
    print(f"type 2 on ik: affine defect {d:.2e}")
    assert d > 1e-8
    for t in RC.TYPES:
        assert RC.affine_defect("ik", t, 2) <= 1e-13, t


def test_the_cases_cover_what_they_are_for(cases):
    assert SC.NAMES == ("six", "used_up", "rank_def", "ragged", "fixed", "fixed_rank_def", "fixed_ragged", "ik", "mid", "wide") and SC.K == 65
    assert SC.TYPES == (0, 1, 3, 4, 5, 8, 9) and all(SC.types_of(n) == SC.TYPES for n in SC.NAMES if n not in ("mid", "wide"))
    six, ik = cases[("six", 0)], cases[("ik", 1)]
    assert six["n"] == 6 and six["caps"] == [2, 3, 2] and ik["n"] == 40 and ik["caps"] == [12] * 5 and ik["lod"].shape[0] == 8
    assert cases[("rank_def", 0)]["ref"]["rank"].tolist() == [[2, 0, 2]] * 3                     # a repeated-row level, a level of rank 0
    up = cases[("used_up", 0)]["ref"]
    assert (up["rank"][:, 2] == 0).all() and (up["fcol"][:, 2] >= up["totalrank"]).all()          # a level that finds the columns used up
    assert (cases[("ragged", 0)]["dims"] == 0).any() and len({tuple(d) for d in cases[("ragged", 0)]["dims"].tolist()}) == 4  # empty levels, per-problem dimensions
    assert cases[("fixed", 0)]["nf"].tolist() == [2, 2, 5, 1]                                     # two, all (n = 5) and one variable fixed
    for (name, t), c in cases.items():
        f = c["factors"]
        assert f[0, 0] == 0.0 and 0.0 < abs(f[1, 1]) < 1e-15                                      # a zero factor on one level, one below the gate
        assert np.abs(c["a"]).max() > 1e-3
    for t in RC.TYPES:  # the damping changes the solution
        assert np.abs(cases[("ik", t)]["a"] - cases[("ik", 0)]["a"]).max() > 1e-3, t
    # with the handle's own b and fixed values reference (b) reproduces the oracle's x, rank-deficient problems included
    for key in (("rank_def", 0), ("fixed_rank_def", 1), ("fixed", 8), ("ik", 4)):
        c = cases[key]
        ref, keep = c["ref"], c["fixed"]["fixed_val"] if c["fixed"] else np.zeros((c["lod"].shape[0], c["n"]))
        back = np.stack([SC.solve_rhs_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], c["dims"][b],
                                                  int(c["nf"][b]), SC.own_rhs(c)[b], keep[b], key[1], c["factors"][b]) for b in range(c["lod"].shape[0])])
        assert SC.rel_rows(back, ref["x"]) <= SC.D_CPU, key


def test_the_jvp_comparison_on_the_cpu():
    worst = max(SC.jvp_gap("ik", t)[0] for t in RC.TYPES)
    print(f"D_JVP measured {worst:.2e}, recorded {SC.D_JVP:.2e}, step {SC.JVP_STEP}")
    assert SC.D_JVP / 2 <= worst <= SC.D_JVP and SC.JVP_TOL == 10.0 * SC.D_JVP


def fit_check(tmp_path, shapes):
    """tests/solve_rhs_fit_check.cpp on (n, cap, nObj) triples -> [(plain variant, damped variant, bytes lds, bytes hbm, bytes work, work doubles)]"""
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed for the stand-alone placement check (tests/solve_rhs_fit_check.cpp)"
    exe = str(tmp_path / "solve_rhs_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "solve_rhs_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n} {cap} {nobj}\n" for n, cap, nobj in shapes), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(shapes)
    return [(p, r, int(a), int(b), int(c), int(d)) for p, r, a, b, c, d in (line.split("|") for line in lines)]


def test_the_host_rules_on_both_sides_of_each_switch(tmp_path):
    cap, nobj = 90, 3
    shapes = [(49, cap, nobj), (50, cap, nobj), (60, cap, nobj), (74, cap, nobj), (75, cap, nobj), (86, cap, nobj), (40, 60, 5), (6, 7, 3), (92, cap, nobj), (93, cap, nobj)]
    res = fit_check(tmp_path, shapes)
    limit = SC.LDS_LIMIT
    for (n, c, k), (plain, reg, lds, hbm, work, doubles) in zip(shapes, res):
        print(f"n={n} cap={c} nObj={k}: {plain} | {reg}  {lds} B / {hbm} B / {work} B, {doubles} work doubles")
        assert (lds, hbm, work) == tuple(SC.reg_lds_bytes(n, c, f) for f in ("lds", "hbm", "work"))  # the Python restatement
        assert reg == SC.reg_variant(n, c) and plain == SC.plain_variant(n, c)
        assert reg == ("solve_rhs_reg<64,lds>" if lds <= limit else "solve_rhs_reg<64,hbm>" if hbm <= limit else "solve_rhs_reg<64,work>")
        assert doubles == {"lds": 0, "hbm": 2 * n * n, "ork": 2 * n * n + 64 * (3 * n + c)}[reg[-4:-1]] and work <= limit
    assert [r[1].split(",")[1][:-1] for r in res] == ["lds", "hbm", "hbm", "hbm", "work", "work", "lds", "lds", "work", "work"]  # 49 | 50 and 74 | 75 at cap = 90
    assert [r[0].split(",")[1][:-1] for r in res[-2:]] == ["staged", "lds"]  # the plain rule (tangent_map_placement) switches at 92 | 93 for this cap
    assert [SC.variant(nm, 1) for nm in ("ik", "mid", "wide")] == ["solve_rhs_reg<64,lds>", "solve_rhs_reg<64,hbm>", "solve_rhs_reg<64,work>"]
