"""Every LexLSE kernel family held to the rank threshold `tol_linear_dependence` on near-singular data (tests/rank_cases.py: one column a
combination of two others plus 1e-4 N(0,1), so that the pivot taking it has a fresh squared norm of 1e-10 .. 1e-5 — accepted at
tol_keep = 1e-13 and at the default 1e-12, a rank break at tol_drop = 1e-4; iid full-rank and exactly dependent problems in the same wavefronts).
Each case solves at tol_keep, tol_drop and the default through setParameters on ONE handle, asserts last_kernel(), and compares with the CPU
oracle at the same tolerance.  Only problems whose oracle ranks are the same a decade either side of each tolerance are in a case, so "ranks
exact" is a fair demand of the tolerance-contract kernels too.

Contract (B) kernels (lqr_quad, lqr_lwave, lqr_wave, lqr_generic, lqr_large<multi-launch>): ranks, first columns, total rank, permutation and x
bit-identical to the oracle; factor and Householder scalars too where kept.  Contract (T) kernels (lqr_qtol and its ragged and estimating
instantiations, lqr_mfma, lqr_large<step-per-pivot>): ranks, first columns, total rank and permutation exact, x finite and
|x - x_oracle|_inf / max(1, |x_oracle|_inf) <= max(1e-10, 100 x the problem's one-ulp sensitivity), measured on the oracle (include/lexls_hip.h,
contract (T); scripts/soak_qtol.py).  At tol_drop the problems are well conditioned (sensitivity <= 1e-12: tests/test_rank_cases.py) and the
plain 1e-10 applies.

What would make each test fail (each kernel's own copy of the reference's rank test `fresh < a.tol`, lexlse.h:214):
  test_qtol*, test_guard*   lqr_qtol_body.inc:480  — `a.tol` replaced by 1e-12, or `fresh` by sqrt(fresh) (every case has flipping problems
                            whose pivot lies between tol_drop^2 and tol_drop), or `j < dlev` taken for the rank test in the ragged form: ranks
                            at tol_drop come out one too high; a break one pivot early: one too low at tol_drop, full-rank neighbours unchanged
  test_mfma*                lqr_mfma_impl.h:695    — the same edits; n = 44 / 47 (a near-dependent ROW: see the test) run the third column tile behind it
  test_quad*                lqr_quad_impl.h:478    — the same edits; `cont` of one problem leaking into its wavefront neighbours shows in the mixed
                            groups of four (flipping, full-rank and exactly dependent side by side)
  test_lwave*               lqr_lwave_impl.h:298
  test_small*, test_handle* lqr_small_impl.h:411 (:526 is the lane hand-off variant, compiled out); lexls_capi.hip lexls_lse_set_tolerance: without
                            `factor_valid = false` solve() serves the old x; without dropping the prefix-reuse state the levels read back keep
                            the ranks of the old tolerance (FOUND by test_handle_state[wave-prefix-reuse]; fixed with it)
  test_generic*             lqr_generic.hip:421
  test_large*               lqr_large.hip:184 (multi-launch), :761 (launch per pivot: a batch), :1406 (pivots of a level in one launch: one problem)
A kernel that ignored `tol` altogether passes no case: every case asserts that the oracle's own ranks differ between tol_keep and tol_drop.

MEASURED on MI355X (largest (T) error / largest error over one-ulp sensitivity, per kernel, over the three tolerances):
    kernel                             largest error   largest error / one-ulp sensitivity
    lqr_qtol<3,12,shift 7>             4.75e-10        3.42      (and its estimating instantiation: the same x, bit for bit)
    lqr_qtol<3,12>                     6.61e-11        2.86
    lqr_qtol<2,12>                     4.80e-11        5.85
    lqr_qtol<3,8>                      1.05e-10        11.1
    lqr_qtol<2,8>                      1.31e-10        3.10
    lqr_qtol<2,12,ragged>              1.11e-10        6.37
    lqr_qtol<3,12,shift 7,ragged>      4.02e-11        7.30
    lqr_mfma<32,12,n40> / <16,12,n40>  4.42e-10        3.83
    lqr_mfma<64,12>                    4.42e-10        5.76
    lqr_mfma<32,12>                    1.23e-11        5.76
    lqr_large<step-per-pivot,mfma>     1.26e-11        2.48
The largest errors are at tol_keep and the default (the small pivot accepted: sensitivities up to 5e-10); at tol_drop every kernel is below
1e-12.  Ranks, first columns, total rank and permutation exact in every case; every (B) kernel bit-identical.  Kept / flip counts per case:
tests/rank_cases.py.
"""
import numpy as np
import pytest

import rank_cases as R
from lexls_amd import capi
from scripts import calibrate_guard as CG

pytestmark = pytest.mark.gpu

ORDER = ("keep", "drop", "default")


def handle(hip, case, policy, guard=None, sl=slice(None)):
    lod, dims = case["lod"][sl], case["dims"][sl]
    s = hip.BatchedLexLSE(lod.shape[0], case["n"], case["caps"])
    s.set_kernel_policy(policy)
    if guard is not None:
        s.set_accuracy_guard(guard)
    if not case["uniform"]:
        s.setObjDim(dims)
    s.setProblem(lod)
    return s


def outputs(s, keep_factor):
    r, fc, tr = s.getRanks()
    o = dict(rank=r, fcol=fc, totalrank=tr, perm=s.get_column_permutations(), x=s.get_x())
    if keep_factor:
        o.update(factor=s.get_lexqr(), hh=s.get_hh_scalars())
    return o


def assert_pivots(o, ref, ctx, sl=slice(None)):
    for k in ("rank", "fcol", "totalrank", "perm"):
        np.testing.assert_array_equal(o[k], ref[k][sl], err_msg=f"{ctx}: {k}")


def assert_bit_exact(o, ref, case, ctx, sl=slice(None)):
    assert_pivots(o, ref, ctx, sl)
    np.testing.assert_array_equal(o["x"], ref["x"][sl], err_msg=f"{ctx}: x")
    if "factor" in o:
        for b, m in enumerate(case["dims"][sl].sum(axis=1)):  # (rows beyond a problem's own are not written)
            np.testing.assert_array_equal(o["hh"][b, :m], ref["hh"][sl][b, :m], err_msg=f"{ctx}: Householder scalars of problem {b}")
            np.testing.assert_array_equal(o["factor"][b, :, :m], ref["factor"][sl][b, :, :m], err_msg=f"{ctx}: factor of problem {b}")


def assert_tolerance_contract(o, ref, sens, ctx, sl=slice(None)):
    """-> (largest error, largest error / one-ulp sensitivity)"""
    assert_pivots(o, ref, ctx, sl)
    assert np.isfinite(o["x"]).all(), ctx
    xr = ref["x"][sl]
    err = np.abs(o["x"] - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))
    ratio = float((err / np.maximum(sens[sl], 1e-300)).max())
    print(f"{ctx}: largest error {err.max():.3e}, largest error / one-ulp sensitivity {ratio:.3g}")
    bad = err > np.maximum(1e-10, 100.0 * sens[sl])
    assert not bad.any(), f"{ctx}: problems {np.flatnonzero(bad).tolist()} err {err[bad].tolist()} sensitivity {sens[sl][bad].tolist()}"
    return float(err.max()), ratio


def run_case(hip, name, policy, kernel, exact, keep_factor=False, sl=slice(None)):
    """the case at tol_keep, tol_drop and the default, one handle, setParameters between the solves"""
    case = R.build(name)
    assert case["flip"][sl].any() and not case["flip"][sl].all(), "the oracle's ranks must differ between the two tolerances for some problems only"
    s = handle(hip, case, policy, sl=sl)
    for t in ORDER:
        s.setParameters(R.TOLS[t])
        s.factorize_solve(keep_factor=keep_factor)
        assert s.last_kernel() == kernel
        ctx = f"{name} policy {policy} {s.last_kernel()} tol_{t}"
        o = outputs(s, keep_factor)
        if exact:
            assert_bit_exact(o, case["ref"][t], case, ctx, sl)
        else:
            assert_tolerance_contract(o, case["ref"][t], case["sens"][t], ctx, sl)
    return s


# ---- contract (T): lqr_qtol --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [0, 6])
def test_qtol_ik_mixed_wavefronts(hip, policy):
    """flipping, full-rank and exactly dependent problems in the same groups of four"""
    run_case(hip, "ik", policy, "lqr_qtol<3,12,shift 7>", exact=False)


@pytest.mark.parametrize("name,kernel", [("n36", "lqr_qtol<3,12>"), ("n24", "lqr_qtol<2,12>"), ("n40x8", "lqr_qtol<3,8>"), ("n24x8", "lqr_qtol<2,8>")])
def test_qtol_other_instantiations(hip, name, kernel):
    run_case(hip, name, 6, kernel, exact=False)


@pytest.mark.parametrize("name,kernel", [("ragged", "lqr_qtol<2,12,ragged>"), ("ragged_per_problem", "lqr_qtol<3,12,shift 7,ragged>")])
def test_qtol_ragged(hip, name, kernel):
    """policy 10: one hierarchy [6, 3, 12, 2] for the batch, and per-problem dimensions with empty levels"""
    run_case(hip, name, 10, kernel, exact=False)


def test_guard_estimating_instantiation(hip):
    """guard mode 1 on the IK shape: the estimating instantiation breaks ranks where the shipped one does (same x, bit for bit), and its
    status / estimate arrays follow the header: status 1 below the threshold, 2 above, flagged = number of 2s, the estimate = max over the
    ACCEPTED pivots of |raw pivot column| / |R_jj| — large where tol_keep accepts the small pivot, small again where tol_drop breaks before it"""
    case = R.build("ik")
    assert case["flip"].any() and not case["flip"].all()
    g, p = handle(hip, case, 0, guard=1), handle(hip, case, 0)
    flagged = 0
    for t in ORDER:
        for s in (g, p):
            s.setParameters(R.TOLS[t])
            s.factorize_solve(keep_factor=False)
        assert g.last_kernel() == "lqr_qtol<3,12,shift 7,guard>" and p.last_kernel() == "lqr_qtol<3,12,shift 7>"
        ctx = f"ik guard 1 {g.last_kernel()} tol_{t}"
        o = outputs(g, False)
        assert_tolerance_contract(o, case["ref"][t], case["sens"][t], ctx)
        np.testing.assert_array_equal(o["x"], p.get_x(), err_msg=ctx)
        est, st, nf = g.get_accuracy()
        assert np.isfinite(est).all() and (est > 0).all(), ctx
        assert set(np.unique(st).tolist()) <= {1, 2} and nf == int((st == 2).sum()), ctx
        assert (st[est > CG.DEFAULT_THRESHOLD] == 2).all() and (st[est < CG.DEFAULT_THRESHOLD] == 1).all(), ctx
        np.testing.assert_allclose(est, CG.estimate(case["lod"], case["caps"], case["n"], case["ref"][t]), rtol=1e-3, err_msg=ctx)
        assert nf == (0 if t == "drop" else int((st[case["flip"]] == 2).sum())), ctx  # (only an accepted small pivot is flagged here)
        flagged += nf
    assert flagged > 0, "the case does not exercise status 2"


# ---- contract (T): lqr_mfma --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,kernel", [(7, "lqr_mfma<32,12,n40>"), (8, "lqr_mfma<64,12>"), (9, "lqr_mfma<16,12,n40>")])
def test_mfma_ik_mixed_wavefronts(hip, policy, kernel):
    run_case(hip, "ik", policy, kernel, exact=False)


@pytest.mark.parametrize("policy,kernel", [(7, "lqr_mfma<32,12>"), (8, "lqr_mfma<64,12>")])
@pytest.mark.parametrize("name", ["n44", "n47"])
def test_mfma_third_column_tile(hip, name, policy, kernel):
    """n = 44 with two levels, n = 47 with one: as deep as lqr_mfma's LDS slices hold these n.  With fewer rows than variables a near-dependent
    column is never a pivot, so here the last ROW of level 0 is near-dependent: the level's twelfth pivot is the small one"""
    run_case(hip, name, policy, kernel, exact=False)


@pytest.mark.parametrize("policy", [7, 8])
def test_mfma_policies_beyond_their_lds_budget(hip, policy):
    """n = 47 with four levels of 12 rows: 16 x 12688 bytes do not fit a CU's 160 KB, policies 7 / 8 go where policy 6 sends the shape —
    the bit-exact four-per-wavefront kernel (three slots, n read from the arguments)"""
    run_case(hip, "n47x4", policy, "lqr_quad<3,12>", exact=True)


# ---- contract (B) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_factor,kernel", [(False, "lqr_quad<3,12,shift 7>"), (True, "lqr_quad<3,12,shift 7,factor>")])
def test_quad_ik_mixed_wavefronts(hip, keep_factor, kernel):
    run_case(hip, "ik", 4, kernel, exact=True, keep_factor=keep_factor)


@pytest.mark.parametrize("keep_factor", [False, True])
def test_lwave(hip, keep_factor):
    run_case(hip, "ik", 3, "lqr_lwave<41,12,exact>", exact=True, keep_factor=keep_factor)


@pytest.mark.parametrize("keep_factor", [False, True])
@pytest.mark.parametrize("name,kernel", [("ik", "lqr_wave<41,12,exact>"), ("ragged_per_problem", "lqr_wave<41,12,exact>"), ("n36", "lqr_wave<41,12>"), ("n47x4", "lqr_wave<64,16>")])
def test_small(hip, name, kernel, keep_factor):
    """the register-resident wave kernel: its three instantiations, full and ragged levels"""
    run_case(hip, name, 2, kernel, exact=True, keep_factor=keep_factor)


@pytest.mark.parametrize("keep_factor", [False, True])
def test_generic(hip, keep_factor):
    run_case(hip, "generic", 1, "lqr_generic<64,lds>", exact=True, keep_factor=keep_factor)


# ---- beyond one CU's LDS -----------------------------------------------------------------------------------------------------------------
def test_large_multi_launch_bit_exact(hip):
    run_case(hip, "large", 5, "lqr_large<multi-launch>", exact=True, keep_factor=True)


def test_large_step_per_pivot_batch(hip):
    """three problems: a launch per pivot"""
    run_case(hip, "large", 0, "lqr_large<step-per-pivot,mfma>", exact=False, keep_factor=True)


def test_large_step_per_pivot_one_problem(hip):
    """one problem: the pivots of a level inside one launch.  (The one problem flips, so run_case's 'some problems only' is checked on the batch.)"""
    case = R.build("large")
    b = int(np.flatnonzero(case["flip"])[0])
    s = handle(hip, case, 0, sl=slice(b, b + 1))
    for t in ORDER:
        s.setParameters(R.TOLS[t])
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == "lqr_large<step-per-pivot,mfma>"
        assert_tolerance_contract(outputs(s, False), case["ref"][t], case["sens"][t], f"large problem {b} {s.last_kernel()} tol_{t}", slice(b, b + 1))


# ---- handle state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,kernel,reuse", [(4, "lqr_quad<3,12,shift 7,factor>", False), (2, "lqr_wave<41,12,exact>", False), (2, "lqr_wave<41,12,exact>", True)],
                         ids=["quad", "wave", "wave-prefix-reuse"])
def test_handle_state(hip, policy, kernel, reuse):
    """lexls_lse_set_tolerance invalidates what the handle keeps (include/lexls_hip.h): after a change of the tolerance solve() without a new
    factorization is an ERROR (never the old x), the prefix-reuse state is gone (resume levels armed before the change are dropped, arming
    them after it is an error), and factorize_solve() gives what a fresh handle gives at the new tolerance, bit for bit — up, down and
    up again"""
    case = R.build("ik")
    nobj = len(case["caps"])
    assert case["flip"].any()
    s = handle(hip, case, policy)
    if reuse:
        s.set_prefix_reuse(True)
    s.setParameters(R.TOL_KEEP)
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == kernel
    assert_bit_exact(outputs(s, True), case["ref"]["keep"], case, "first solve")
    s.solve()  # same tolerance: the kept factor serves
    np.testing.assert_array_equal(s.get_x(), case["ref"]["keep"]["x"])
    for t in ("drop", "keep", "default", "drop"):
        ctx = f"{kernel} reuse {reuse}: on to tol_{t}"
        if reuse:
            assert s.prefix_reuse_ready(), ctx
            s.set_resume_levels(nobj)  # "nothing changed": true of the rows, not of the tolerance
        s.setParameters(R.TOLS[t])
        with pytest.raises(capi.LexlsError):
            s.solve()
        if reuse:
            assert not s.prefix_reuse_ready(), ctx
            with pytest.raises(capi.LexlsError):
                s.set_resume_levels(nobj)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == kernel
        got = outputs(s, True)
        fresh = handle(hip, case, policy)
        fresh.setParameters(R.TOLS[t])
        fresh.factorize_solve(keep_factor=True)
        want = outputs(fresh, True)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{ctx}: {k} differs from a fresh handle's")
        assert_bit_exact(got, case["ref"][t], case, ctx)
        if reuse:  # and at an unchanged tolerance the levels are read back as before
            assert s.prefix_reuse_ready(), ctx
            s.set_resume_levels(nobj)
            s.setParameters(R.TOLS[t])
            s.factorize_solve(keep_factor=True)
            assert_bit_exact(outputs(s, True), case["ref"][t], case, ctx + " (levels read back)")
