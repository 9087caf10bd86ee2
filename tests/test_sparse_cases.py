"""The conditions that make tests/test_gpu_sparse.py meaningful, asserted on the cases of tests/sparse_cases.py from the oracle and the dispatch
plan alone (no GPU)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjoint_cases as AC
import adjoint_matrix_cases as AM
import skip_cases as S
import sparse_cases as SP
from oracle import oracle_ctypes as oracle
from scripts import record_dispatch_table as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SP.cases()
IDS = [f"{nm}-{g}" for nm, g in CASES]
PER_WAVEFRONT = {"lqr_qtol<": 4, "lqr_quad<": 4, "lqr_mfma<16": 4, "lqr_mfma<32": 2}  # problems that share a wavefront, by kernel name


def test_the_case_table():
    """every family of the issue has its instantiations, by the names skip_cases carries; what is left out is what the module text says"""
    kernels = {S.CASES[nm]["kernel"] for nm in SP.NAMES}
    assert {k for k in kernels if k.startswith("lqr_qtol")} == {"lqr_qtol<3,12,shift 7>", "lqr_qtol<3,12,shift 7,guard>", "lqr_qtol<3,12,shift 7,ragged>", "lqr_qtol<3,8>",
                                                               "lqr_qtol<2,12>"}
    assert {k for k in kernels if k.startswith("lqr_mfma")} == {"lqr_mfma<32,12,n40>", "lqr_mfma<64,12>", "lqr_mfma<16,12,n40>", "lqr_mfma<32,12>"}
    assert {k for k in kernels if k.startswith("lqr_quad")} == {"lqr_quad<3,12,shift 7>", "lqr_quad<3,12,shift 7,factor>", "lqr_quad<4,16>", "lqr_quad<4,16,factor>",
                                                               "lqr_quad<4,16,fixed>", "lqr_quad<3,12,shift 7,factor,fixed>"}
    assert {k for k in kernels if k.startswith("lqr_lwave")} == {"lqr_lwave<41,12,exact>", "lqr_lwave<41,12>"}
    assert {k for k in kernels if k.startswith("lqr_wave")} == {"lqr_wave<41,12,exact>", "lqr_wave<41,12>", "lqr_wave<64,16>"}
    assert {k for k in kernels if k.startswith("lqr_generic")} == {"lqr_generic<64,lds>", "lqr_generic<256,lds>", "lqr_generic<1024,hbm>"}
    assert {k for k in kernels if k.startswith("lqr_large")} == {"lqr_large<multi-launch>", "lqr_large<step-per-pivot,mfma>"}
    assert set(SP.FULL) <= set(SP.NAMES) and set(S.CONSUMER_CASES) <= set(SP.FULL)
    assert len(CASES) == 2 * len(SP.NAMES) + 3 * len(SP.FULL)
    for nm in SP.NAMES:
        assert SP.batch_of(S.CASES[nm]) == (3 if S.CASES[nm]["n"] == 100 else 19)
        assert sum(SP.widths_of(S.CASES[nm])) == S.CASES[nm]["n"]


@pytest.mark.parametrize("name,gen", CASES, ids=IDS)
def test_rank_is_cut_at_an_exactly_zero_norm(name, gen):
    """at least a third of the problems have a level of rank below min(rows, columns left) whose rows hold exactly 0.0 in every unpivoted column
    of the oracle's factor; those columns were structural zeros of the level, and they survived the earlier levels' eliminations because every
    update term was zero: a pivot of an earlier level with a non-zero multiplier onto the level's rows has a row that is zero there"""
    case = SP.build(name, gen)
    ref, dims, n = case["ref"], case["dims"], case["n"]
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(len(dims), np.uint32)
    cut = [(b, k) for b, k in SP.cut_levels(case) if not SP.leftover(case, b, k).any()]
    assert 3 * len({b for b, _ in cut}) >= len(dims)
    for b, k in cut:
        first = np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        Fc, r, T = int(ref["fcol"][b, k]), int(ref["rank"][b, k]), int(ref["totalrank"][b])
        left = np.arange(Fc + r, n)
        assert left.size and first[k + 1] - first[k] > r
        W = ref["factor"][b].T  # W[row, column]
        for j in range(k):  # the update of level k's rows by level j: rows -= multipliers x (pivot rows of j)
            Fj, Fcj, rj = int(first[j]), int(ref["fcol"][b, j]), int(ref["rank"][b, j])
            mult = W[first[k]:first[k + 1], Fcj:Fcj + rj]
            used = np.flatnonzero((mult != 0.0).any(axis=0))
            assert not W[np.ix_(Fj + used, left)].any(), (b, k, j)
        if int(nf[b]) == 0:  # (positions follow the transpositions; the fixed columns of a problem are moved before them)
            pos = np.array([AM.position(ref["perm"][b], T, i) for i in range(n)])
            zero_vars = np.flatnonzero(np.isin(pos, left))
            assert case["structural"][b][np.ix_(zero_vars, np.arange(first[k], first[k + 1]))].all(), (b, k)


@pytest.mark.parametrize("name,gen", [(nm, g) for nm, g in CASES if any(S.CASES[nm]["kernel"].startswith(p) for p in PER_WAVEFRONT)],
                         ids=[f"{nm}-{g}" for nm, g in CASES if any(S.CASES[nm]["kernel"].startswith(p) for p in PER_WAVEFRONT)])
def test_mixed_rank_profiles_inside_a_wavefront(name, gen):
    case = SP.build(name, gen)
    per = next(v for p, v in PER_WAVEFRONT.items() if case["kernel"].startswith(p))
    rank = case["ref"]["rank"]
    assert any(len({tuple(r) for r in rank[i:i + per].tolist()}) >= 2 for i in range(0, len(rank), per))


@pytest.mark.parametrize("name,gen", [(nm, g) for nm, g in CASES if S.CASES[nm]["contract"] in ("T", "L")],
                         ids=[f"{nm}-{g}" for nm, g in CASES if S.CASES[nm]["contract"] in ("T", "L")])
def test_tolerance_contract_cases_keep_stable_problems_only(name, gen):
    case, c = SP.build(name, gen), S.CASES[name]
    assert S._stable(c, case["lod"], case["dims"], case["fixed"]).all()
    assert case["kept"] >= S.RETENTION * case["drawn"]


@pytest.mark.parametrize("name,gen", CASES, ids=IDS)
def test_oracle_results_are_finite(name, gen):
    case = SP.build(name, gen)
    assert np.isfinite(case["lod"]).all()
    for k, v in case["ref"].items():
        assert np.isfinite(v).all(), k
    if gen == "zero_rhs":
        np.testing.assert_array_equal(case["ref"]["x"], np.zeros_like(case["ref"]["x"]))
        assert not case["lod"][:, case["n"], :].any()
    if gen == "zero_level":
        zero = set()  # the levels that are zero rows altogether, A and b: first, middle and last occur in a batch of 19 (the large batch: level 0)
        for b in range(len(case["dims"])):
            first = np.concatenate([[0], np.cumsum(case["dims"][b])]).astype(int)
            zero |= {k for k in range(len(first) - 1) if first[k + 1] > first[k] and not case["lod"][b, :, first[k]:first[k + 1]].any()}
        nobj = len(case["caps"])
        assert zero == ({0, nobj // 2, nobj - 1} if len(case["dims"]) == SP.BATCH else {0})


@pytest.mark.parametrize("name", SP.FULL)
def test_signed_zeros_do_not_change_the_oracle(name):
    """perm, ranks, factor, Householder scalars and x on the data with -0.0 are value-equal to those on the same data with +0.0"""
    case, c = SP.build(name, "neg_zero"), S.CASES[name]
    minus = np.signbit(case["lod"]) & (case["lod"] == 0.0)
    assert 0.3 < minus.sum() / case["structural"].sum() < 0.7 and not (minus[:, :case["n"]] & ~case["structural"]).any()
    assert not (np.signbit(case["lod_plus"]) & (case["lod_plus"] == 0.0)).any()
    np.testing.assert_array_equal(case["lod_plus"], case["lod"])  # (as values)
    plus = S._run(c, case["lod_plus"], case["dims"], case["fixed"])
    for k in ("perm", "rank", "fcol", "totalrank", "factor", "hh", "x", "v"):
        np.testing.assert_array_equal(case["ref"][k], plus[k], err_msg=k)


def test_planned_kernels(tmp_path):
    """each case's expected kernel name is what the host-side dispatch plan (lexls_amd/csrc/lexls_dispatch.h through tests/dispatch_plan_check.cpp
    and the query lines of scripts/record_dispatch_table.py) gives for its shape, policy and switches"""
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
    for i, nm in enumerate(SP.NAMES):
        c = SP.build(nm, "limbs")
        lines.append(R.query_line(dict(kind="lse", id=i, caps=c["caps"], dims=c["dims"], n=c["n"], batch=len(c["dims"]), policy=c["policy"], keep=int(c["keep"]), mode="fs",
                                       fixed=int(bool(c["fixed"])), guard=c["guard"], reg=0, qtol0=0, align8=0), cus))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(SP.NAMES)
    for nm, line in zip(SP.NAMES, out):
        assert line.split("|")[1] == S.CASES[nm]["kernel"], (nm, line)


@pytest.mark.parametrize("gen", SP.CONSUMER_GENERATORS)
@pytest.mark.parametrize("name", S.CONSUMER_CASES)
def test_consumer_references(name, gen):
    """the references the post-factorization calls are held to agree among themselves ten times closer than the device has to: the unit solves of
    tests/adjoint_cases.py with its restatement on the oracle's factor, the KKT reference of tests/adjoint_matrix_cases.py with its own.  Levels of
    rank 0 occur; no `dead` problem is rank-stable (a zero column is never a pivot, so behind 60 rows the total rank stays below n = 40 and some
    level is short of min(rows, columns left)), the zero_level data hold both kinds"""
    case, want = SP.build(name, gen), SP.consumers(name, gen)
    B = len(case["dims"])
    assert ((case["ref"]["rank"] == 0) & (case["ref"]["fcol"] < case["n"])).any()
    gap = max(AC._rel(want["grad_rhs_A"][b] - want["grad_rhs_B"][b], want["grad_rhs_A"][b]) for b in range(B))
    assert 10.0 * gap <= AC.TOL, gap
    flags = want["flags"]
    if gen == "dead":
        assert not flags.any()
    else:
        assert 2 <= flags.sum() < B / 2  # both kinds, the rank-stable ones the fewer
    mgap = max([AC._rel(want["GA"][b] - want["GB"][b], want["GA"][b]) for b in np.flatnonzero(flags)] or [0.0])
    assert 10.0 * mgap <= AM.TOL, mgap
    assert not want["GA"][flags == 0].any()
    moved = np.abs(want["ln1"] - case["ref"]["x"]).max(axis=1)
    assert (moved[case["ref"]["totalrank"] < case["n"]] > 0).any()  # solveLeastNorm_1 has something to do


def test_lsi_case_is_solved_by_the_oracle_driver():
    """LSI_SEED is the first seed of its series at which the oracle-backed driver ends PROBLEM_SOLVED (status 0) for every instance within the
    default limits; the general levels between the bounds and the last level hold exact zeros in three of five column groups"""
    probs = SP.lsi_problems()
    assert len(probs) == SP.LSI_INSTANCES == 6
    for objs in probs:
        assert oracle.lsi_run(SP.LSI_N, objs)["info"]["status"] == 0
        assert "var" in objs[0] and not (objs[-1]["A"] == 0.0).any()
        for o in objs[1:-1]:
            assert (o["A"] == 0.0).all(axis=0).sum() == 24 and (o["A"] != 0.0).all(axis=0).sum() == 16
    ranks = {oracle.lsi_run(SP.LSI_N, objs)["info"]["total_rank"] for objs in probs}
    print(f"total ranks of the last equality problems: {sorted(ranks)}")


def test_measured_table_is_current():
    """the MEASURED table of the module text is what `python tests/sparse_cases.py` prints"""
    for nm, g in CASES:
        assert SP.summary(SP.build(nm, g)) in SP.__doc__, (nm, g)
