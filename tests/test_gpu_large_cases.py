"""The large path (lexls_amd/csrc/lqr_large.hip) held to the CPU oracle on both sides of the switches of its kernels and launchers, on the
cases of tests/large_cases.py (what each is for; tests/test_large_cases.py: which side of which switch, asserted from the constants).  Every
case is a small batch whose problem 0 is also solved alone, so the same data go through the launch per pivot (fast_step: a batch, and one
problem under LEXLS_LARGE_PERSIST = 0 / 2) and through the pivots of a level in one launch (fast_level_persist: one problem, default).

Policy 5, lqr_large<multi-launch>, contract (B): ranks, first columns, total rank, permutation, Householder scalars, factor, x and get_v() bit for
bit.  Policy 0, lqr_large<step-per-pivot,mfma>, contract (T) as tests/test_gpu_rank_tolerance.py holds it: pivots and ranks exact, x finite and
|x - x_oracle|_inf / max(1, |x_oracle|_inf) <= max(1e-10, 100 x the problem's one-ulp sensitivity measured on the oracle); factor, Householder
scalars and get_v() within 1e-10 of the oracle's relative to the largest entry of the quantity (never below 1), as check_large of
tests/test_gpu_parity.py compares them.  lexls_lse_last_large_levels tells the one-launch form from its fall-back: under
LEXLS_LARGE_PERSIST = 1 every level reached is committed inside its launch and none is redone (n1030: no form fits G = 258 workgroups, both
counts 0), under 2 every level reached is redone, under 0 and for a batch both counts are 0.

What would make which case fail (one-token slips in lqr_large.hip and lqr_large_plan.h, by reasoning; the constants are lqr_large_plan.h's):
    fast_step, tail loop of the dot product `i = lane + 64u * FRC` -> `64u * (FRC + 1)`  rows 256 .. 319 leave the dot product: rows1030, rows1024, rows257 (R = 257),
                                        rows330 — batches and modes 0 / 2 (x off by O(1); the tail loop of the update likewise: rows of the trailing columns not updated)
    fast_step, second search loop (beyond NCAND = kStepCandWindow / FNT candidates per thread) `k < n` -> `k < 1024`  columns 1024 .. 1029 are never candidates:
                                        n1030's first pivots (permutation); `p < bp` -> `p <= bp` in that loop: the tie 1000 / 1027 goes to the later position
    large_pivot, search loop `k += NTP` second trip dropped: n1030 under policy 5 (permutation); its column staging / column swap loops `i += NTP`: rows1030
                                        under policy 5 (rows 1024 .. 1029 leave the norm / the reflector)
    fast_level_persist, one-by-one granule loop `i = tid + CR * NT` -> `(CR + 1) * NT`  rows 256 .. 511 of the pivot column are not fetched: rows257, rows330, rows1024,
                                        rows1030 alone under mode 1; `i += NT` -> `i += 2 * NT`: rows1024 / rows1030 only
    persist_within_limits `G > kPersistMaxG` with kPersistMaxG 256 -> 512  n1030 alone would run a form whose polls hold 4 x 64 records: the counters (in_launch 0 expected)
    plan_level `level_max <= kTrsmColsMax` -> `<`  rows1024 would take large_trsm: same numbers, so only a fault in it would show — the boundary is pinned
                                        from the other side by kTrsmColsMax 1024 -> 1030: rows1030 would launch large_trsm_cols with 1088 threads (launch error)
    large_trsm (never run before)        any slip: rows1030 under both policies (the rows below level 0 feed level 1's ranks and x)
    plan_level level_end_grid `(rows_max + kLevelEndRows - 1) / kLevelEndRows` -> `rows_max / kLevelEndRows`, or fast_level_end's stride `gridDim.x * 256` -> `256`
                                        rows1030 / rows1024 (rows beyond 1024 not copied)
    plan_level gemm_grid[1] `(n + GBN) / GBN` -> `(n + GBN - 1) / GBN`  edges128 loses the right-hand side column (n + 1 = 129): x; edges127 pins the exact fit
    plan_level trsm_grid `(rows_max + TRB - 1) / TRB` -> `rows_max / TRB`  the 65th row below level 0 of edges127 / edges128; TCH chunks: ranks 17 and 5 there
    read_all_exhausted `!host[b].exhausted` -> `host[b].exhausted`  rows1030 / rows330 batches: level 1 of the live problems is never factorized (ranks)
    counters                            mode 1 silently falling back (abort on every level) gives redone > 0; mode 2 not aborting gives in_launch > 0
    fast_workspace_layout, a piece short (st[1] taking one record for the batch, E taking maxdim x n, the column buffer one granule per row short) or
                                        FastWorkspace::clear_end short of the column buffer: tests/test_large_plan.py on the CPU; on the GPU test_workspace_reuse — the third
                                        solve runs in a work space that holds the second's records, tags and essential parts at other offsets

MEASURED on MI355X (policy 0; error = |x - x_oracle|_inf / max(1, |x_oracle|_inf), largest over the case's problems; ratio = error / one-ulp
sensitivity; every bit-exact comparison under policy 5 held):
    case       batch, a launch per pivot    one problem, mode 0 / 2      one problem, mode 1 (in_launch, redone)
    rows1030   7.303e-16  ratio 1.62        7.303e-16  ratio 1           1.082e-15  ratio 1.49   (2, 0)
    rows1024   1.166e-15  ratio 1.47        1.166e-15  ratio 1.47        9.714e-16  ratio 1.23   (2, 0)
    n1030      9.576e-16  ratio 0.917       9.159e-16  ratio 0.917       9.159e-16  ratio 0.917  (0, 0)
    rows257    5.322e-14  ratio 1.62        1.166e-15  ratio 1.62        1.374e-15  ratio 1.9    (3, 0)
    rows330    5.759e-16  ratio 1.36        5.274e-16  ratio 1.36        4.441e-16  ratio 1.14   (1, 0)
    edges127   3.157e-16  ratio 1.2         1.943e-16  ratio 0.389       2.220e-16  ratio 0.444  (4, 0)
    edges128   6.939e-16  ratio 1.67        1.249e-16  ratio 0.533       2.359e-16  ratio 1.01   (4, 0)
A problem alone under mode 0 / 2 gives the x it gives inside its batch, bit for bit (not asserted: both are held to the contract).
"""
import numpy as np
import pytest

import large_cases as L

pytestmark = pytest.mark.gpu

MULTI, FAST = "lqr_large<multi-launch>", "lqr_large<step-per-pivot,mfma>"
NAMES = list(L.CASES)


def solve(hip, case, policy, sl):
    lod, dims = case["lod"][sl], case["dims"][sl]
    s = hip.BatchedLexLSE(lod.shape[0], case["n"], case["caps"])
    s.set_kernel_policy(policy)
    s.setObjDim(dims)
    s.setProblem(lod)
    s.factorize_solve(keep_factor=True)
    return s


def outputs(s):
    r, fc, tr = s.getRanks()
    return dict(rank=r, fcol=fc, totalrank=tr, perm=s.get_column_permutations(), x=s.get_x(), factor=s.get_lexqr(), hh=s.get_hh_scalars(), v=s.get_v())


def assert_pivots(o, ref, ctx, sl):
    for k in ("rank", "fcol", "totalrank", "perm"):
        np.testing.assert_array_equal(o[k], ref[k][sl], err_msg=f"{ctx}: {k}")


def assert_bit_exact(o, case, ctx, sl):
    ref = case["ref"]
    assert_pivots(o, ref, ctx, sl)
    np.testing.assert_array_equal(o["x"], ref["x"][sl], err_msg=f"{ctx}: x")
    for b, m in enumerate(case["dims"][sl].sum(axis=1)):  # (rows beyond a problem's own are not written)
        for k in ("hh", "v"):
            np.testing.assert_array_equal(o[k][b, :m], ref[k][sl][b, :m], err_msg=f"{ctx}: {k} of problem {b}")
        np.testing.assert_array_equal(o["factor"][b, :, :m], ref["factor"][sl][b, :, :m], err_msg=f"{ctx}: factor of problem {b}")


def assert_tolerance_contract(o, case, ctx, sl, ref=None, sens=None):
    """contract (T) against `ref` (default: the oracle's result) -> (largest error of x, largest error / one-ulp sensitivity)"""
    ref = case["ref"] if ref is None else ref
    sens = case["sens"][sl] if sens is None else sens
    assert_pivots(o, ref, ctx, sl)
    assert np.isfinite(o["x"]).all(), ctx
    xr = ref["x"][sl]
    err = np.abs(o["x"] - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))
    ratio = float((err / np.maximum(sens, 1e-300)).max())
    print(f"{ctx}: largest error {err.max():.3e}, largest error / one-ulp sensitivity {ratio:.3g}")
    bad = err > np.maximum(1e-10, 100.0 * sens)
    assert not bad.any(), f"{ctx}: problems {np.flatnonzero(bad).tolist()} err {err[bad].tolist()} sensitivity {sens[bad].tolist()}"
    for b, m in enumerate(case["dims"][sl].sum(axis=1)):  # factor magnitudes, Householder scalars, residuals: as check_large (tests/test_gpu_parity.py)
        for k, a, r in (("factor", o["factor"][b, :, :m], ref["factor"][sl][b, :, :m]), ("hh", o["hh"][b, :m], ref["hh"][sl][b, :m]), ("v", o["v"][b, :m], ref["v"][sl][b, :m])):
            assert np.abs(a - r).max() <= 1e-10 * max(1.0, float(np.abs(r).max())), f"{ctx}: {k} of problem {b}: {np.abs(a - r).max():.3e}"
    return float(err.max()), ratio


ONE, ALL = slice(0, 1), slice(None)


# ---- policy 5: bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_multi_launch_one_problem(hip, name):
    case = L.build(name)
    s = solve(hip, case, 5, ONE)
    assert s.last_kernel() == MULTI
    assert_bit_exact(outputs(s), case, f"{name} policy 5, problem 0 alone", ONE)
    assert s.last_large_levels() == (0, 0)


@pytest.mark.parametrize("name", NAMES)
def test_multi_launch_batch(hip, name):
    """the batch against the oracle, and every problem of it against its stand-alone solve on the same path"""
    case = L.build(name)
    s = solve(hip, case, 5, ALL)
    assert s.last_kernel() == MULTI
    o = outputs(s)
    assert_bit_exact(o, case, f"{name} policy 5, batch", ALL)
    for b in range(1, case["lod"].shape[0]):  # (problem 0 alone: test_multi_launch_one_problem, against the same oracle result)
        alone = solve(hip, case, 5, slice(b, b + 1))
        assert alone.last_kernel() == MULTI
        oa = outputs(alone)
        m = int(case["dims"][b].sum())
        for k in ("rank", "fcol", "totalrank", "perm", "x"):
            np.testing.assert_array_equal(oa[k][0], o[k][b], err_msg=f"{name} problem {b} alone / in the batch: {k}")
        for k in ("hh", "v"):
            np.testing.assert_array_equal(oa[k][0, :m], o[k][b, :m], err_msg=f"{name} problem {b} alone / in the batch: {k}")
        np.testing.assert_array_equal(oa["factor"][0, :, :m], o["factor"][b, :, :m], err_msg=f"{name} problem {b} alone / in the batch: factor")


# ---- policy 0: a launch per pivot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_step_per_pivot_batch(hip, monkeypatch, name):
    """the batch under the contract, and every problem of it against its stand-alone solve on the same path (a launch per pivot:
    LEXLS_LARGE_PERSIST = 0 for the single problems)"""
    case = L.build(name)
    s = solve(hip, case, 0, ALL)
    assert s.last_kernel() == FAST
    assert s.last_large_levels() == (0, 0)  # (a batch never takes the one-launch form)
    o = outputs(s)
    assert_tolerance_contract(o, case, f"{name} policy 0, batch", ALL)
    monkeypatch.setenv("LEXLS_LARGE_PERSIST", "0")
    for b in range(case["lod"].shape[0]):
        sl = slice(b, b + 1)
        alone = solve(hip, case, 0, sl)
        assert alone.last_kernel() == FAST and alone.last_large_levels() == (0, 0)
        oa = outputs(alone)
        assert_tolerance_contract(oa, case, f"{name} policy 0, problem {b} alone (a launch per pivot)", sl)
        assert_tolerance_contract(oa, case, f"{name} policy 0, problem {b} alone against the batch's", sl, ref=o, sens=case["sens"][sl])


@pytest.mark.parametrize("mode", ["0", "2"])
@pytest.mark.parametrize("name", NAMES)
def test_one_problem_launch_per_pivot(hip, monkeypatch, name, mode):
    """LEXLS_LARGE_PERSIST = 0: never the one-launch form; 2: its abort flag raised before every launch, every level reached redone"""
    monkeypatch.setenv("LEXLS_LARGE_PERSIST", mode)
    case = L.build(name)
    s = solve(hip, case, 0, ONE)
    assert s.last_kernel() == FAST
    assert_tolerance_contract(outputs(s), case, f"{name} policy 0, problem 0 alone, mode {mode}", ONE)
    in_launch, redone = s.last_large_levels()
    assert in_launch == 0
    assert redone == (0 if mode == "0" or name == "n1030" else L.levels_reached(case))


# ---- policy 0: the pivots of a level in one launch (kept LAST in this file: the one-by-one granule loop of fast_level_persist runs here) ----
@pytest.mark.parametrize("name", NAMES)
def test_one_problem_in_launch(hip, monkeypatch, name):
    """LEXLS_LARGE_PERSIST = 1 (the default): every level reached is committed by its launch, none is redone; n1030: no form fits, both 0"""
    monkeypatch.setenv("LEXLS_LARGE_PERSIST", "1")
    case = L.build(name)
    s = solve(hip, case, 0, ONE)
    assert s.last_kernel() == FAST
    assert_tolerance_contract(outputs(s), case, f"{name} policy 0, problem 0 alone, mode 1", ONE)
    in_launch, redone = s.last_large_levels()
    print(f"{name}: in_launch {in_launch} redone {redone}")
    assert redone == 0
    if name == "n1030":
        assert in_launch == 0
    else:
        assert in_launch == L.levels_reached(case) > 0


# ---- one handle, three shapes: the work space grows, then is reused under a smaller layout ----
@pytest.mark.parametrize("batch", [1, 2])
def test_workspace_reuse(hip, monkeypatch, batch):
    """One handle with n = 60 and capacities [330, 100] solves level dimensions [300, 100], [330, 70] and [300, 100] again (tests/large_cases.py,
    REUSE): the work space is allocated for the first, grows for the second (largest level 330) and is kept for the third, whose layout
    (fast_workspace_layout) is the first's again inside the larger allocation — every piece at an exact offset, nothing of the slack the sum
    formula used to add.  Batch 1 takes the pivots of a level in one launch (the records, tags and column granules of the solve before are
    cleared by the layout's range), batch 2 a launch per pivot.  Every result under contract (T) against the oracle; tests/test_large_cases.py
    asserts on the CPU that all of them are planned lqr_large<step-per-pivot,mfma> and that 100 x sensitivity < 1e-10."""
    monkeypatch.setenv("LEXLS_LARGE_PERSIST", "1")
    sl = slice(0, batch)
    first = L.build("reuse300")
    s = hip.BatchedLexLSE(batch, first["n"], first["caps"])
    s.set_kernel_policy(0)
    for step, name in enumerate(("reuse300", "reuse330", "reuse300")):
        case = L.build(name)
        s.setObjDim(case["dims"][sl])
        s.setProblem(case["lod"][sl])
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == FAST
        assert_tolerance_contract(outputs(s), case, f"work-space reuse, batch {batch}, solve {step} ({name})", sl)
        assert s.last_large_levels() == ((L.levels_reached(case), 0) if batch == 1 else (0, 0))
