"""Every LexLSE factorization kernel family, the consumers of a kept factor and one LexLSI batch held to the oracle on BLOCK-SPARSE data: the
cases of tests/sparse_cases.py (what the generators are; tests/test_sparse_cases.py: the conditions that make the comparison meaningful — ranks
cut at exactly zero norms, mixed rank profiles inside a wavefront, stable problems only under the tolerance contracts — from the oracle alone).

Every equality below is an equality of VALUES, as np.testing.assert_array_equal defines it: -0.0 equals +0.0, NaN anywhere fails.  Signed zeros
are not pinned: no sentence of include/lexls_hip.h promises the sign of a zero, and the oracle's own results on data with -0.0 are only
value-equal to those with +0.0 (tests/test_sparse_cases.py).  No tolerance is defined here: contract "B" is bit for bit (ranks, first columns,
total rank, permutation, x, with the factor kept the Householder scalars and the factor over each problem's own rows), contract "T" is pivots
exact and x within test_gpu_qtol.TOL relative to max(1, |x|_inf), contract "L" is assert_tolerance_contract of tests/test_gpu_large_cases.py with
the one-ulp sensitivity measured on the oracle — all three as tests/test_gpu_lse_skip.py::assert_contract applies them.  The adjoint calls are held
to adjoint_cases.TOL and adjoint_matrix_cases.TOL against those modules' references (A).  last_kernel() is asserted in every test: none passes on
another kernel than the one it names.

MEASURED on MI355X (every test prints its figures): contract "T", largest |x - x_oracle| / max(1, |x|_inf) 4.1e-13 (qtol_8 / dead: 8.1e-10 at |x|_inf
2.0e3; qtol_ik / zero_level 1.8e-13, mfma_two / zero_level 7.3e-14) against 1e-10; contract "L" 6.7e-16, 1.3 x the one-ulp sensitivity; the guard flags 1
problem of 19 (limbs) and 0 (dead), estimates 2.5 .. 174; solve_adjoint / solve_adjoint_multi at most 1.2e-14 (TOL 1e-12), solve_adjoint_matrix at most
9.6e-14 (TOL 1.7e-12) on 3, 4 and 3 rank-stable problems of 19.  No kernel was found wrong.  A scratch build of lqr_qtol whose rank test took an
exactly zero norm for a pivot fails test_family_against_the_oracle[qtol_ik-*] (ranks) and test_two_runs_of_one_handle_give_the_same_bits[qtol_ik]."""
import numpy as np
import pytest

import adjoint_cases as AC
import adjoint_matrix_cases as AM
import skip_cases as S
import sparse_cases as SP
import test_gpu_qtol as Q
from lexls_amd import lexlsi
from test_gpu_lse_skip import PIVOTS, assert_contract, outputs

pytestmark = pytest.mark.gpu

CASES = SP.cases()
IDS = [f"{nm}-{g}" for nm, g in CASES]
TOLERANCE_CASES = [nm for nm in SP.NAMES if S.CASES[nm]["contract"] in ("T", "L")]


def handle(hip, case, guard=None):
    s = hip.BatchedLexLSE(len(case["dims"]), case["n"], case["caps"])
    s.set_kernel_policy(case["policy"])
    if case["guard"] if guard is None else guard:
        s.set_accuracy_guard(case["guard"] if guard is None else guard)
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"], f["fixed_idx"], f["fixed_val"])
    return s


def run(s, case):
    s.setProblem(case["lod"])
    s.factorize_solve(keep_factor=case["keep"])
    assert s.last_kernel() == case["kernel"]
    return outputs(s, case)


@pytest.mark.parametrize("name,gen", CASES, ids=IDS)
def test_family_against_the_oracle(hip, name, gen):
    case = SP.build(name, gen)
    s = handle(hip, case)
    o = run(s, case)
    print(f"{name} / {gen}: {s.last_kernel()}")
    assert_contract(o, case, case["ref"], np.arange(len(case["dims"])), f"{name} / {gen}", case.get("sens"))
    if gen == "zero_rhs":
        np.testing.assert_array_equal(o["x"], np.zeros_like(o["x"]))
    s.close()


@pytest.mark.parametrize("gen", ["limbs", "dead"])
def test_guard_reports_and_re_solves(hip, gen):
    """the accuracy guard in mode 2 on the guard case: the estimate meets zero diagonals — it is finite and not negative, the status is 1 or 3 and
    the count is the number of 3s; the problems it flags carry the bit-exact x, the others the tolerance contract.  Which problems it flags is not
    pinned: the estimate is one-sided"""
    case = SP.build("qtol_guard", gen)
    s = handle(hip, case, guard=2)
    o = run(s, case)
    est, st, nf = s.get_accuracy()
    flagged = st == 3
    print(f"qtol_guard / {gen}: {int(flagged.sum())} of {len(st)} flagged, estimates {est.min():.3g} .. {est.max():.3g}")
    assert np.isfinite(est).all() and (est >= 0).all()
    assert set(np.unique(st).tolist()) <= {1, 3} and nf == int(flagged.sum())
    ref = case["ref"]
    for k in PIVOTS:
        np.testing.assert_array_equal(o[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(o["x"][flagged], ref["x"][flagged], err_msg="x of a re-solved problem")
    assert np.isfinite(o["x"]).all()
    assert np.abs(o["x"] - ref["x"]).max() <= Q.TOL * max(1.0, float(np.abs(ref["x"]).max()))
    s.close()


@pytest.mark.parametrize("name", TOLERANCE_CASES)
def test_two_runs_of_one_handle_give_the_same_bits(hip, name):
    case = SP.build(name, "dead")
    s = handle(hip, case)
    first = run(s, case)
    second = run(s, case)
    for k in first:
        assert np.array_equal(first[k], second[k]), f"{name}: {k} differs between two runs of the same data"
    s.close()


@pytest.mark.parametrize("gen", SP.CONSUMER_GENERATORS)
@pytest.mark.parametrize("name", S.CONSUMER_CASES)
def test_consumers_of_a_kept_factor(hip, name, gen):
    """levels of rank 0 and columns that are never pivoted under every post-factorization call: get_v, ObjectiveSensitivity at every level,
    multipliers() and solveLeastNorm_1 equal the oracle; solve_adjoint and solve_adjoint_multi within adjoint_cases.TOL of the oracle's unit
    solves; solve_adjoint_matrix within adjoint_matrix_cases.TOL of the KKT reference on the rank-stable problems, differentiable == 0 and an
    exactly zero gradient on every other one"""
    case, want = SP.build(name, gen), SP.consumers(name, gen)
    B, nobj = len(case["dims"]), len(case["caps"])
    s = handle(hip, case)
    o = run(s, case)
    print(f"{name} / {gen}: {s.last_kernel()}")
    assert_contract(o, case, case["ref"], np.arange(B), f"{name} / {gen}")
    np.testing.assert_array_equal(s.get_v(), want["v"], err_msg="get_v")
    for k in range(nobj):
        s.setCtrType(want["types"])
        found, ctr, obj, maxabs = s.ObjectiveSensitivity(k)
        np.testing.assert_array_equal(found.astype(np.int32), want["sens"][k][:, 0], err_msg=f"found, level {k}")
        np.testing.assert_array_equal(np.where(found, ctr, 0), np.where(found, want["sens"][k][:, 1], 0), err_msg=f"ctr, level {k}")
        np.testing.assert_array_equal(np.where(found, obj, 0), np.where(found, want["sens"][k][:, 2], 0), err_msg=f"obj, level {k}")
        np.testing.assert_array_equal(maxabs, want["maxabs"][k], err_msg=f"maxabs, level {k}")
        np.testing.assert_array_equal(s.getWorkspace(), want["lam"][k], err_msg=f"multipliers, level {k}")
        np.testing.assert_array_equal(s.getCtrType(), want["marks"][k], err_msg=f"marks, level {k}")
    s.setCtrType(want["types"])
    np.testing.assert_array_equal(s.multipliers(), want["mult"], err_msg="multipliers()")
    # the adjoints
    G = want["G"]
    grad_rhs, grad_fixed = s.solve_adjoint(G[:, 0])
    assert np.isfinite(grad_rhs).all() and not grad_fixed.any()
    gap = max(AC._rel(grad_rhs[b] - want["grad_rhs_A"][b, 0], want["grad_rhs_A"][b, 0]) for b in range(B))
    multi, multi_fixed = s.solve_adjoint_multi(G)
    assert np.isfinite(multi).all() and not multi_fixed.any()
    gap_multi = max(AC._rel(multi[b, j] - want["grad_rhs_A"][b, j], want["grad_rhs_A"][b, j]) for b in range(B) for j in range(G.shape[1]))
    print(f"{name} / {gen}: solve_adjoint {gap:.2e}, solve_adjoint_multi {gap_multi:.2e} against the unit solves (TOL {AC.TOL:.1e})")
    assert gap <= AC.TOL and gap_multi <= AC.TOL
    Gm, diff = s.solve_adjoint_matrix(G[:, 0])
    np.testing.assert_array_equal(diff, want["flags"], err_msg="differentiable")
    if gen == "zero_level":
        assert diff.any() and not diff.all()  # both kinds occur
    assert np.isfinite(Gm).all()
    assert not Gm[diff == 0].any()
    mgap = max([AC._rel(Gm[b] - want["GA"][b], want["GA"][b]) for b in np.flatnonzero(diff)] or [0.0])
    print(f"{name} / {gen}: solve_adjoint_matrix {mgap:.2e} against the KKT reference on {int(diff.sum())} rank-stable problems of {B} (TOL {AM.TOL:.1e})")
    assert mgap <= AM.TOL
    s.solveLeastNorm_1()
    np.testing.assert_array_equal(s.get_x(), want["ln1"], err_msg="solveLeastNorm_1")
    s.solve()
    np.testing.assert_array_equal(s.get_x(), case["ref"]["x"], err_msg="solve() on the kept factor")
    s.close()


@pytest.mark.parametrize("path", ["persistent", "stages"])
def test_lsi_batch_with_block_sparse_levels(hip, oracle, monkeypatch, path):
    """six LexLSI instances whose general levels are block-sparse: info, x and the working set equal the oracle-backed driver's, through the
    persistent launch and through the stage path (LEXLS_LSI_NO_FUSED=1, as tests/test_gpu_lsi.py selects it)"""
    if path == "persistent":
        monkeypatch.delenv("LEXLS_LSI_NO_FUSED", raising=False)
    else:
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    probs = SP.lsi_problems()
    pk = lexlsi.pack_batch(SP.LSI_N, probs)
    srv = lexlsi.LsiBatch(SP.LSI_N, pk.dims, pk.types, len(probs))
    try:
        r = srv.run(pk)
        kernel = srv.last_kernel()
    finally:
        srv.close()
    print(f"LexLSI, {path}: {kernel}")
    assert kernel.startswith("lsi_fused<") == (path == "persistent") and kernel.startswith(("lsi_fused<", "lqr_"))
    for i, objs in enumerate(probs):
        o = oracle.lsi_run(SP.LSI_N, objs)
        assert o["info"]["status"] == 0
        assert r["info"][i] == o["info"], i
        np.testing.assert_array_equal(r["x"][i], o["x"], err_msg=str(i))
        np.testing.assert_array_equal(r["active"][i], np.concatenate(o["active"]), err_msg=str(i))
