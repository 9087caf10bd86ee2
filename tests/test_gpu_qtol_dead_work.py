"""lqr_qtol with the row broadcast of the Gauss elimination folded into the fma (lexls_amd/csrc/lqr_qtol_impl.h: qt_gauss_dpp, v_fmac_f64_dpp
row_newbcast) in the elimination steps with one or two live slots.  The cases are those in which such steps meet something other than the
bench batch: a partly filled wavefront, problems of one wavefront whose finished pivots end at different columns (a row with fewer pivots than
the wavefront's maximum runs the folded steps on the zeros of the x block as U'), a level of rank 0, the two-slot instantiation (every step
folded), the eight-row operand lists, the ragged and the estimating instantiations of the same body.  The level end and the level start are
as they were.  Acceptance = tests/test_gpu_qtol.py::check / tests/test_gpu_qtol_ragged.py::check (contract (T) of include/lexls_hip.h):
column permutation, ranks, first columns and total rank EXACT, x within 1e-10 relative to max(1, |x|_inf).  Every constructed problem's
ranks are asserted on the oracle's result, so a construction that misses its purpose fails here, without a GPU result involved."""
import numpy as np
import pytest

import test_gpu_qtol as Q
import test_gpu_qtol_ragged as R
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

N, DIMS = 40, [12] * 5
FULL = [12, 12, 12, 4, 0]


def deficient_level1(lod, b, seed):
    """level 1 of problem b: two duplicated rows and three rows that are combinations of level-0 rows -> rank 7 (rows along the last axis)"""
    lod[b, :, 13] = lod[b, :, 12]
    lod[b, :, 15] = lod[b, :, 14]
    g = P.normal(seed, 3 * 12).reshape(3, 12)
    lod[b, :, 16:19] = lod[b, :, 0:12] @ g.T


def mixed_rank_batch():
    lod = P.lse_batch(31000, 8, N, DIMS)
    for b in (1, 6):
        deficient_level1(lod, b, 31100 + b)
    return lod


def rank0_batch():
    lod = P.lse_batch(32000, 4, N, DIMS)
    lod[2, :, 12:24] = lod[2, :, 0:12]  # level 1 repeats level 0: rank 0
    return lod


def test_bench_instantiation_partly_filled_wavefront(hip, oracle):
    _, ref = Q.check(hip, oracle, P.lse_batch(30000, 5, N, DIMS))
    assert (ref["rank"] == FULL).all()


def test_mixed_ranks_inside_one_wavefront(hip, oracle):
    """problems 1 and 6 (one per wavefront) have a level 1 of rank 7: their first columns at levels 2 and 3 are 19 and 31 against 24 and 36, their
    ranks at level 3 are 9 and 4.  The wavefront eliminates up to its largest first column: in the folded steps 19 .. 23 (level 2) and 31 .. 35
    (level 3) one row of the wavefront has no pivot and must come through unchanged"""
    lod = mixed_rank_batch()
    _, ref = Q.check(hip, oracle, lod)
    want = np.tile(np.array(FULL), (8, 1))
    want[[1, 6]] = [12, 7, 12, 9, 0]
    np.testing.assert_array_equal(ref["rank"], want)


def test_level_of_rank_zero_in_one_problem_of_the_quad(hip, oracle):
    _, ref = Q.check(hip, oracle, rank0_batch())
    want = np.tile(np.array(FULL), (4, 1))
    want[2] = [12, 0, 12, 12, 4]
    np.testing.assert_array_equal(ref["rank"], want)


def test_two_slot_instantiation(hip, oracle):
    """<2,12,0,0>: every elimination step has one or two slots"""
    dims = [12] * 3
    _, ref = Q.check(hip, oracle, P.lse_batch(33000, 4, 24, dims), dims, expect="lqr_qtol<2,12>", n=24)
    assert (ref["rank"] == [12, 12, 0]).all()


def test_levels_of_eight_rows(hip, oracle):
    """<3,8,0,0>: the eight-row operand lists of the folded elimination"""
    dims = [8] * 5
    _, ref = Q.check(hip, oracle, P.lse_batch(34000, 4, N, dims), dims, expect="lqr_qtol<3,8>", n=N)
    assert (ref["rank"] == [8] * 5).all()


def test_ragged_uniform_hierarchy(hip, oracle):
    dims = [5, 12, 7, 12, 9]
    _, ref = R.check(hip, oracle, P.lse_batch(35000, 4, N, dims), dims, N, expect="lqr_qtol<3,12,shift 7,ragged>")
    assert (ref["rank"] == [5, 12, 7, 12, 4]).all()


def test_ragged_per_problem_dims_with_empty_levels(hip, oracle):
    dims = np.array([[0, 12, 5, 12, 11], [12, 0, 12, 12, 4], [7, 3, 1, 0, 12], [1, 12, 12, 2, 9]], np.uint32)
    lod = R.per_problem_batch(36000, 4, N, dims, 60)
    _, ref = R.check(hip, oracle, lod, dims, N, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")
    np.testing.assert_array_equal(ref["rank"], [[0, 12, 5, 12, 11], [12, 0, 12, 12, 4], [7, 3, 1, 0, 12], [1, 12, 12, 2, 9]])


def test_accuracy_guard_instantiation(hip, oracle):
    """the first case on the estimating instantiation (same body): contract against the oracle, and the same results as the plain kernel"""
    lod = P.lse_batch(30000, 5, N, DIMS)
    ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
    plain = Q.solve(hip, lod)
    g = hip.BatchedLexLSE(5, N, DIMS)
    g.set_accuracy_guard(1)
    g.setProblem(lod)
    g.factorize_solve(keep_factor=False)
    assert g.last_kernel() == "lqr_qtol<3,12,shift 7,guard>"
    r, fc, tr = g.getRanks()
    np.testing.assert_array_equal(r, ref["rank"])
    np.testing.assert_array_equal(fc, ref["fcol"])
    np.testing.assert_array_equal(tr, ref["totalrank"])
    np.testing.assert_array_equal(g.get_column_permutations(), ref["perm"])
    x = g.get_x()
    assert np.isfinite(x).all()
    assert np.abs(x - ref["x"]).max() <= Q.TOL * max(1.0, float(np.abs(ref["x"]).max()))
    np.testing.assert_array_equal(x, plain.get_x())
