"""The skip mask of LexLSE (lexls_lse_set_skip; include/lexls_hip.h: "problems whose flag is non-zero are left untouched by the next factorize /
factorize_solve calls (their previous results stay valid)") held to that sentence on every factorization kernel family, on the cases of
tests/skip_cases.py (what each is for; tests/test_skip_cases.py: the conditions that make the comparison meaningful, from the oracle alone).

One handle, three runs.  Run 1 (no mask, lod1): the family's own contract against the oracle.  Run 2 (mask, lod2 — the skipped slots NaN or
valid data of another seed): the LIVE problems under the family's contract against the oracle on the composite batch, the SKIPPED problems
np.array_equal against a copy of run 1's DEVICE results, every array (a tolerance-contract kernel may differ from the oracle, not from itself).
Run 3 (mask cleared, lod3): the whole batch against the oracle — nothing is sticky.  Contracts: "B" x, ranks, first columns, total rank,
permutation bit for bit, with the factor kept the factor and the Householder scalars over each problem's own rows as well; "T" pivots and ranks
exact, x within test_gpu_qtol.TOL relative to max(1, |x|_inf) (Q.check); "L" assert_tolerance_contract of tests/test_gpu_large_cases.py.
last_kernel() is asserted after runs 1 and 2 and printed: a dispatch rule that moves makes a case fail instead of quietly testing another kernel."""
import numpy as np
import pytest

import adjoint_cases as AC
import skip_cases as S
import test_gpu_qtol as Q
from test_gpu_large_cases import assert_tolerance_contract

pytestmark = pytest.mark.gpu

NAMES = list(S.CASES)
PIVOTS = ("rank", "fcol", "totalrank", "perm")


def handle(hip, case, prefix_reuse=False):
    s = hip.BatchedLexLSE(len(case["skip"]), case["n"], case["caps"])
    s.set_kernel_policy(case["policy"])
    if case["reg"]:
        s.setRegularization(case["reg"][0], [case["reg"][1]] * len(case["caps"]))
    if case["guard"]:
        s.set_accuracy_guard(case["guard"])
    if prefix_reuse:
        s.set_prefix_reuse(True)
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"], f["fixed_idx"], f["fixed_val"])
    return s


def run(s, case, lod, mask="keep"):
    if not isinstance(mask, str):
        s.set_skip(mask)
    s.setProblem(lod)
    s.factorize_solve(keep_factor=case["keep"])
    assert s.last_kernel() == case["kernel"]
    return outputs(s, case)


def outputs(s, case):
    """a copy of every result array of the handle"""
    r, fc, tr = s.getRanks()
    o = dict(x=s.get_x(), rank=r, fcol=fc, totalrank=tr, perm=s.get_column_permutations())
    if case["keep"]:
        o.update(factor=s.get_lexqr(), hh=s.get_hh_scalars())
    if case["contract"] == "L":
        o["v"] = s.get_v()
    if case["guard"]:
        o["est"], o["status"], _ = s.get_accuracy()
    return o


def assert_contract(o, case, ref, idx, ctx, sens=None):
    """the problems `idx` of the outputs `o` hold the family's contract against the oracle's result `ref`"""
    idx = np.asarray(idx)
    if idx.size == 0:
        return
    if case["contract"] == "L":
        pseudo = dict(ref=ref, sens=sens, dims=case["dims"])
        assert_tolerance_contract({k: v[idx] for k, v in o.items()}, pseudo, ctx, idx)
        return
    for k in PIVOTS:
        np.testing.assert_array_equal(o[k][idx], ref[k][idx], err_msg=f"{ctx}: {k}")
    x, xr = o["x"][idx], ref["x"][idx]
    assert np.isfinite(x).all(), ctx
    if case["contract"] == "T":
        err = float(np.abs(x - xr).max())
        print(f"{ctx}: max|x - x_oracle| = {err:.3e}")
        assert err <= Q.TOL * max(1.0, float(np.abs(xr).max())), ctx
        return
    np.testing.assert_array_equal(x, xr, err_msg=f"{ctx}: x")
    if case["keep"]:
        for b in idx:  # (rows beyond a problem's own are not written)
            m = int(case["dims"][b].sum())
            np.testing.assert_array_equal(o["hh"][b, :m], ref["hh"][b, :m], err_msg=f"{ctx}: hh of problem {b}")
            np.testing.assert_array_equal(o["factor"][b, :, :m], ref["factor"][b, :, :m], err_msg=f"{ctx}: factor of problem {b}")


def assert_kept(o, o1, idx, ctx):
    """the problems `idx` have the bits of run 1's device results, every array"""
    for k in o1:
        for b in idx:
            assert np.array_equal(o[k][b], o1[k][b], equal_nan=True), f"{ctx}: {k} of skipped problem {b} is not what run 1 left"


def sens_of(case, which):
    return case["sens"][which] if case["contract"] == "L" else None


@pytest.mark.parametrize("variant", ["poison", "fresh"])
@pytest.mark.parametrize("name", NAMES)
def test_three_runs(hip, name, variant):
    case = S.build(name)
    everyone = np.arange(len(case["skip"]))
    s = handle(hip, case)
    o1 = run(s, case, case["lod1"])
    print(f"{name} ({variant}): {s.last_kernel()}")
    assert_contract(o1, case, case["ref1"], everyone, f"{name} run 1", sens_of(case, 1))
    o2 = run(s, case, case["lod2"][variant], case["skip"])
    assert_kept(o2, o1, case["skipped"], f"{name} run 2 ({variant})")
    assert_contract(o2, case, case["expected"], case["live"], f"{name} run 2 ({variant}), live problems", sens_of(case, "expected"))
    o3 = run(s, case, case["lod3"], None)
    assert_contract(o3, case, case["ref3"], everyone, f"{name} run 3 (mask cleared)", sens_of(case, 3))


@pytest.mark.parametrize("name", NAMES)
def test_degenerate_masks(hip, name):
    """all bytes 0: the bits of an unmasked run of the same data on a handle of the same history; all bytes 1: every output keeps run 1's bits"""
    case = S.build(name)
    B = len(case["skip"])
    s, plain = handle(hip, case), handle(hip, case)
    o1 = run(s, case, case["lod1"])
    run(plain, case, case["lod1"])
    oz = run(s, case, case["lod2"]["fresh"], np.zeros(B, np.uint8))
    op = run(plain, case, case["lod2"]["fresh"])
    print(f"{name}: {s.last_kernel()}")
    assert_kept(oz, op, np.arange(B), f"{name}, all-zero mask against no mask")
    assert_contract(oz, case, case["ref2_fresh"], case["live"], f"{name}, all-zero mask", sens_of(case, "fresh"))  # (the live slots: the stable ones of a filtered case)
    oo = run(s, case, case["lod3"], np.ones(B, np.uint8))
    assert_kept(oo, oz, np.arange(B), f"{name}, all-one mask")


@pytest.mark.parametrize("policy,kernel", [(5, "lqr_large<multi-launch>"), (0, "lqr_large<step-per-pivot,mfma>")])
def test_large_path_one_problem(hip, policy, kernel):
    """batch 1 on the large path: an all-zero mask is no mask — the dispatch of the unmasked run (the one-launch-per-level form where the unmasked
    run takes it: last_large_levels) and its bits; mask [1]: every output keeps its bits, whatever the input holds"""
    case = S.build("large_multi" if policy == 5 else "large_fast")

    def one(mask):
        s = hip.BatchedLexLSE(1, case["n"], case["caps"])
        s.set_kernel_policy(policy)
        if mask is not None:
            s.set_skip(mask)
        s.setProblem(case["lod1"][:1])
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == kernel
        return s

    plain, zero = one(None), one(np.zeros(1, np.uint8))
    print(f"policy {policy}: {plain.last_kernel()}, levels in launch / redone {plain.last_large_levels()}")
    assert zero.last_large_levels() == plain.last_large_levels()
    np.testing.assert_array_equal(zero.get_x(), plain.get_x())
    np.testing.assert_array_equal(zero.get_lexqr(), plain.get_lexqr())
    np.testing.assert_array_equal(zero.get_column_permutations(), plain.get_column_permutations())
    before = (zero.get_x(), zero.get_lexqr(), zero.get_hh_scalars(), zero.get_column_permutations(), *zero.getRanks())
    zero.set_skip(np.ones(1, np.uint8))
    zero.setProblem(np.full_like(case["lod1"][:1], np.nan))
    zero.factorize_solve(keep_factor=True)
    assert zero.last_kernel() == kernel
    after = (zero.get_x(), zero.get_lexqr(), zero.get_hh_scalars(), zero.get_column_permutations(), *zero.getRanks())
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b)


def test_two_call_form(hip):
    """factorize() then solve() under the mask, on a bit-exact family that keeps its factor (lqr_generic; where the factorization left x on its
    way, solve() has nothing to launch and reports no consumer — a solve launch on the kept factors: test_post_factor_consumers_...)"""
    case = S.build("generic_64")
    s = handle(hip, case)
    s.setProblem(case["lod1"])
    s.factorize()
    s.solve()
    assert s.last_kernel() == case["kernel"]
    o1 = outputs(s, case)
    assert_contract(o1, case, case["ref1"], np.arange(len(case["skip"])), "two calls, run 1")
    s.set_skip(case["skip"])
    s.setProblem(case["lod2"]["poison"])
    s.factorize()
    s.solve()
    assert s.last_kernel() == case["kernel"]
    print(f"two-call form: {s.last_kernel()}, solve by {s.last_consumer_kernel()!r}")
    o2 = outputs(s, case)
    assert_kept(o2, o1, case["skipped"], "two calls, run 2")
    assert_contract(o2, case, case["expected"], case["live"], "two calls, run 2, live problems")


@pytest.mark.parametrize("name", S.CONSUMER_CASES)
def test_post_factor_consumers_read_the_kept_factor(hip, name):
    """after the masked run the kept factor of a skipped problem is its old one: solve, residuals, ObjectiveSensitivity at the last level and
    multipliers() give the oracle's answers for the composite batch bit for bit (as tests/test_gpu_postfactor.py demands), solve_adjoint within
    adjoint_cases.TOL of reference (B) of tests/adjoint_cases.py"""
    case, want = S.build(name), S.consumers(name)
    s = handle(hip, case)
    run(s, case, case["lod1"])
    run(s, case, case["lod2"]["poison"], case["skip"])
    print(f"{name}: {s.last_kernel()}")
    e = case["expected"]
    s.setCtrType(want["types"])
    np.testing.assert_array_equal(s.get_v(), want["v"], err_msg="get_v")
    found, ctr, obj, maxabs = s.ObjectiveSensitivity(want["level"])
    np.testing.assert_array_equal(found.astype(np.int32), want["sens"][:, 0], err_msg="found")
    np.testing.assert_array_equal(np.where(found, ctr, 0), np.where(found, want["sens"][:, 1], 0), err_msg="ctr")
    np.testing.assert_array_equal(np.where(found, obj, 0), np.where(found, want["sens"][:, 2], 0), err_msg="obj")
    np.testing.assert_array_equal(maxabs, want["maxabs"], err_msg="maxabs")
    np.testing.assert_array_equal(s.getWorkspace(), want["lam"], err_msg="multipliers of the level")
    np.testing.assert_array_equal(s.getCtrType(), want["marks"], err_msg="marks")
    s.setCtrType(want["types"])
    np.testing.assert_array_equal(s.multipliers(), want["mult"], err_msg="multipliers()")
    grad_rhs, grad_fixed = s.solve_adjoint(want["g"])
    gap = max(AC._rel(grad_rhs[b] - want["grad_rhs"][b], want["grad_rhs"][b]) for b in range(len(case["skip"])))
    print(f"{name}: solve_adjoint against the reference from the oracle's factor {gap:.2e} (TOL {AC.TOL:.1e})")
    assert gap <= AC.TOL and not grad_fixed.any()
    s.solveLeastNorm_1()  # x now holds something else: solve() has to run on the kept factor, the skipped problems' old one included
    s.solve()
    np.testing.assert_array_equal(s.get_x(), e["x"], err_msg="solve() on the kept factor")


def test_prefix_reuse_after_a_masked_run(hip, oracle):
    """set_prefix_reuse(True) on lqr_wave: after the masked run, a further run with set_resume_levels on every problem, the previously skipped
    ones included, equals a from-scratch factorization (the check of tests/test_gpu_prefix_reuse.py::run_pair): a skipped problem's state is
    that of the run its factor comes from"""
    case = S.build("wave_exact")
    caps, n, K = case["caps"], case["n"], 2
    s = handle(hip, case, prefix_reuse=True)
    run(s, case, case["lod1"])
    assert s.prefix_reuse_ready()
    run(s, case, case["lod2"]["poison"], case["skip"])
    assert s.prefix_reuse_ready()
    print(f"prefix reuse: {s.last_kernel()}")
    lod4 = case["composite"].copy()  # the first K levels of every problem unchanged since ITS previous factorization, the levels behind them new
    lod4[:, :, sum(caps[:K]):] = case["lod3"][:, :, sum(caps[:K]):]
    s.set_skip(None)
    s.setProblem(lod4)
    s.set_resume_levels(K)
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == case["kernel"]
    got = outputs(s, case)
    scratch = handle(hip, case)
    ref = run(scratch, case, lod4)
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    o = oracle.lse_run(lod4, caps, n, nthreads=8)
    for k in PIVOTS + ("x",):
        np.testing.assert_array_equal(got[k], o[k], err_msg=k)


# ---- the accuracy guard under the mask ------------------------------------------------------------------------------------------------------
def guard_outputs(s):
    r, fc, tr = s.getRanks()
    est, status, nf = s.get_accuracy()
    assert nf == int((status >= 2).sum())
    return dict(x=s.get_x(), rank=r, fcol=fc, totalrank=tr, perm=s.get_column_permutations(), est=est, status=status)


def guard_run1(hip, g):
    s = hip.BatchedLexLSE(S.BATCH, S.GUARD_N, S.IK)
    s.set_kernel_policy(6)
    s.set_accuracy_guard(2)
    s.setProblem(g["lod1"])
    s.factorize_solve(keep_factor=False)
    assert s.last_kernel() == "lqr_qtol<3,12,shift 7,guard>"
    o1 = guard_outputs(s)
    flagged = np.zeros(S.BATCH, bool)
    flagged[S.GUARD_FLAGGED_RUN1] = True
    np.testing.assert_array_equal(o1["status"], np.where(flagged, 3, 1))
    for k in PIVOTS + ("x",):  # the flagged problem carries the bit-exact answer
        np.testing.assert_array_equal(o1[k][flagged], g["ref1"][k][flagged], err_msg=k)
    return s, o1


def test_guard_mode2_under_the_mask(hip):
    """a skipped problem that was flagged and re-solved in run 1 (the list of the re-solve names it again: only the indirect kernel's mask test keeps
    it from being solved on its new input) and a skipped problem whose fresh lod2 data would be flagged: x, pivots, estimate and status of both
    keep run 1's bits; live flagged problems carry the bit-exact answer, the other live ones the tolerance contract"""
    g = S.guard_case()
    s, o1 = guard_run1(hip, g)
    s.set_skip(g["skip"])
    s.setProblem(g["lod2"])
    s.factorize_solve(keep_factor=False)
    assert s.last_kernel() == "lqr_qtol<3,12,shift 7,guard>"
    o2 = guard_outputs(s)
    skipped = np.flatnonzero(g["skip"])
    assert_kept(o2, o1, skipped, "guard mode 2, run 2")
    assert o2["status"][S.GUARD_FLAGGED_RUN1] == 3 and o2["status"][S.GUARD_WOULD_FLAG] == 1
    live_flagged = np.asarray(S.GUARD_LIVE_FLAGGED)
    live_plain = np.setdiff1d(np.flatnonzero(g["skip"] == 0), live_flagged)
    assert (o2["status"][live_flagged] == 3).all() and (o2["status"][live_plain] == 1).all()
    e = g["expected"]
    for k in PIVOTS + ("x",):
        np.testing.assert_array_equal(o2[k][live_flagged], e[k][live_flagged], err_msg=f"{k} of a re-solved live problem")
    for k in PIVOTS:
        np.testing.assert_array_equal(o2[k][live_plain], e[k][live_plain], err_msg=k)
    assert np.abs(o2["x"][live_plain] - e["x"][live_plain]).max() <= Q.TOL * max(1.0, float(np.abs(e["x"][live_plain]).max()))


def test_guard_report_of_a_skipped_problem_on_a_bit_exact_plan(hip):
    """include/lexls_hip.h, lexls_lse_get_accuracy: "Under a skip mask (lexls_lse_set_skip) the report of a skipped problem is KEPT: estimate and
    status stay those of the factorization that produced its results, on the estimating kernel and on a bit-exact plan alike".  Guard on, run 2
    under policy 5: the live problems report status 0 and estimate 0 and carry the oracle's bits, the skipped ones keep run 1's report and results"""
    g = S.guard_case()
    s, o1 = guard_run1(hip, g)
    s.set_kernel_policy(5)
    s.set_skip(g["skip"])
    s.setProblem(g["lod2"])
    s.factorize_solve(keep_factor=False)
    assert s.last_kernel() == "lqr_quad<3,12,shift 7>"
    o2 = guard_outputs(s)
    skipped, live = np.flatnonzero(g["skip"]), np.flatnonzero(g["skip"] == 0)
    assert_kept(o2, o1, skipped, "guard on a bit-exact plan, run 2")
    assert (o1["est"][skipped] > 0).all()  # (there is a report to keep)
    assert not o2["status"][live].any() and not o2["est"][live].any()
    for k in PIVOTS + ("x",):
        np.testing.assert_array_equal(o2[k][live], g["expected"][k][live], err_msg=k)
