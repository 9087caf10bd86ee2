"""lqr_qtol with level 0 peeled out of the level loop (lexls_amd/csrc/lqr_qtol_body.inc): level 0 is a straight-line section on its own block,
the loop runs the levels behind it on a block local to the iteration.  The cases are the smallest at which that boundary can go wrong: no
level behind level 0 at all, a level 0 that is rank deficient or all zero (level 1 then starts with every slot live inside the loop and
eliminates by fewer than nine pivots, or none), rows of one wavefront that cross the boundary in different states (exhausted, skipped),
the other instantiations, the ragged form with an empty level 0, the estimating form.  Acceptance = tests/test_gpu_qtol.py::check /
tests/test_gpu_qtol_ragged.py::check (contract (T) of include/lexls_hip.h): column permutation, ranks, first columns and total rank EXACT, x
within 1e-10 relative to max(1, |x|_inf).  The ranks every constructed problem is meant to have are asserted on the oracle's result."""
import numpy as np
import pytest

import test_gpu_qtol as Q
import test_gpu_qtol_ragged as R
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

N = 40


def deficient_level0_batch(seed, batch, n, dims, r0):
    """level 0 with exactly r0 new directions, the levels behind it full (the reference's generator)"""
    ranks = [r0] + [d for d in dims[1:]]
    return np.stack([P.rank_deficient_problem(seed + b, n, dims, ranks) for b in range(batch)])


def duplicated_level0_batch(seed, batch, n, dims, distinct):
    """level 0 has `distinct` different columns, every other column of it an exact copy of one of them (the right-hand side is its own)"""
    lod = P.lse_batch(seed, batch, n, dims)
    for j in range(distinct, n):
        lod[:, j, :dims[0]] = lod[:, j % distinct, :dims[0]]
    return lod


def mixed_batch():
    """n = 20, three levels of 12 rows: problems 0 and 2 have a full level 0 (12, 8, 0: the columns are exhausted in level 1), problems 1 and 3
    one of rank 4 (4, 12, 4)"""
    dims = [12] * 3
    lod = P.lse_batch(41000, 4, 20, dims)
    lod[[1, 3]] = deficient_level0_batch(41100, 4, 20, dims, 4)[[1, 3]]
    return lod, dims


# ---- 1. no level behind level 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,expect", [(40, "lqr_qtol<3,12,shift 7>"), (8, "lqr_qtol<2,12>")])
@pytest.mark.parametrize("batch", [1, 3, 4, 5])
def test_single_level(hip, oracle, n, expect, batch):
    """nObj = 1: the loop never runs; rows beyond the batch idle; with n = 8 level 0 exhausts the columns"""
    _, ref = Q.check(hip, oracle, P.lse_batch(40000 + 10 * n + batch, batch, n, [12]), [12], expect=expect, n=n)
    assert (ref["rank"] == [min(n, 12)]).all()


# ---- 2. rank-deficient level 0 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0", [5, 0])
def test_rank_deficient_level0(hip, oracle, r0):
    """level 1 starts at column r0 < 16 - 7: factor_level<0> inside the loop, its elimination runs r0 steps"""
    dims = [12] * 3
    _, ref = Q.check(hip, oracle, deficient_level0_batch(42000 + r0, 8, N, dims, r0), dims)
    assert (ref["rank"] == [r0, 12, 12]).all()


def test_level0_of_duplicated_columns(hip, oracle):
    dims = [12] * 3
    _, ref = Q.check(hip, oracle, duplicated_level0_batch(43000, 8, N, dims, 5), dims)
    assert (ref["rank"] == [5, 12, 12]).all()


# ---- 3. rows of one wavefront in different states -----------------------------------------------------------------------------------------
def test_mixed_exhaustion_inside_one_wavefront(hip, oracle):
    lod, dims = mixed_batch()
    _, ref = Q.check(hip, oracle, lod, dims, expect="lqr_qtol<2,12>", n=20)
    np.testing.assert_array_equal(ref["rank"], [[12, 8, 0], [4, 12, 4], [12, 8, 0], [4, 12, 4]])


def test_skipped_problem_inside_the_quad(hip, oracle):
    """problem 2 is skipped in the second run: its results stay those of the first run, the other three are those of the new data"""
    lod, dims = mixed_batch()
    s, _ = Q.check(hip, oracle, lod, dims, expect="lqr_qtol<2,12>", n=20)
    x0, perm0, r0 = s.get_x().copy(), s.get_column_permutations().copy(), s.getRanks()[0].copy()
    lod2 = lod[[1, 0, 3, 2]].copy()
    ref = oracle.lse_run(lod2, dims, 20, nthreads=8)
    s.set_skip(np.array([0, 0, 1, 0], np.uint8))
    s.setProblem(lod2)
    s.factorize_solve(keep_factor=False)
    assert s.last_kernel() == "lqr_qtol<2,12>"
    x, perm, r = s.get_x(), s.get_column_permutations(), s.getRanks()[0]
    np.testing.assert_array_equal(x[2], x0[2])
    np.testing.assert_array_equal(perm[2], perm0[2])
    np.testing.assert_array_equal(r[2], r0[2])
    keep = [0, 1, 3]
    np.testing.assert_array_equal(r[keep], ref["rank"][keep])
    np.testing.assert_array_equal(perm[keep], ref["perm"][keep])
    assert np.abs(x[keep] - ref["x"][keep]).max() <= Q.TOL * max(1.0, float(np.abs(ref["x"][keep]).max()))


# ---- 4. the other instantiations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dims,expect", [(40, [8] * 5, "lqr_qtol<3,8>"), (24, [12] * 5, "lqr_qtol<2,12>"), (33, [12] * 5, "lqr_qtol<3,12>")])
def test_other_instantiations(hip, oracle, n, dims, expect):
    Q.check(hip, oracle, P.lse_batch(44000 + n, 8, n, dims), dims, expect=expect, n=n)


# ---- 5. ragged form -----------------------------------------------------------------------------------------------------------------------
def test_ragged_empty_and_short_level0(hip, oracle):
    """policy 10: level 0 of 0, 1 and 12 rows in one wavefront, an empty level in the middle, an odd leading dimension"""
    dims = np.array([[0, 12, 0, 12, 11], [1, 12, 0, 12, 12], [12, 5, 0, 12, 3], [0, 0, 11, 7, 12],
                     [12, 12, 0, 12, 12], [1, 0, 0, 12, 9], [0, 12, 11, 0, 12], [12, 1, 0, 1, 12]], np.uint32)
    caps = [12, 12, 11, 12, 12]  # 59 rows: the leading dimension is the sum of the capacities
    lod = R.per_problem_batch(45000, 8, N, dims, sum(caps))
    _, ref = R.check(hip, oracle, lod, dims, N, maxdim=caps, expect="lqr_qtol<3,12,shift 7,ragged>")
    np.testing.assert_array_equal(ref["rank"][:, 0], dims[:, 0])


# ---- 6. accuracy guard on -----------------------------------------------------------------------------------------------------------------
def test_accuracy_guard_instantiation(hip, oracle):
    dims = [12] * 5
    lod = P.lse_batch(46000, 8, N, dims)
    ref = oracle.lse_run(lod, dims, N, nthreads=8)
    plain = Q.solve(hip, lod)
    g = hip.BatchedLexLSE(8, N, dims)
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
