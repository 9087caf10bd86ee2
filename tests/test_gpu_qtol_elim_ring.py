"""lqr_qtol's ring of image rows (lexls_amd/csrc/lqr_qtol_body.inc, RING_D / RING_W): the elimination of a level's rows by the finished levels
requests the image row of a finished pivot three steps (steps with one or two live slots) or two steps (more live slots) in front of its
use, the first ones at the level head, without asking whether the wavefront has that many finished pivots.  The cases are the smallest at
which that can go wrong: one wavefront and a wavefront with absent problems, finished levels of fewer pivots than the ring is deep (rank 0, 1,
2) beside full ones in one wavefront and as the whole wavefront's, a wavefront that takes the retiring form of level 2 beside one that does
not, every instantiation that carries the ring, and the ragged form with an empty level and a one-row level.
Acceptance = tests/test_gpu_qtol.py::check (contract (T) of include/lexls_hip.h): column permutation, ranks, first columns and total rank
EXACT, x within 1e-10 relative to max(1, |x|_inf); check asserts through last_kernel() that the intended instantiation ran.  What a
constructed problem is built for is asserted on the oracle's result."""
import numpy as np
import pytest

import test_gpu_qtol as Q
import test_gpu_qtol_ragged as R
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

N, DIMS, MD = Q.N, Q.DIMS, 12


def level_of_rank(lod, b, k, r, md=MD):
    """level k of problem b gets exactly r different rows: none (a level of zeros) or its first r, repeated down the level — right-hand side
    included, so the repeated equations agree"""
    rows = slice(k * md, (k + 1) * md)
    if r == 0:
        lod[b, :, rows] = 0.0
    else:
        lod[b, :, rows] = lod[b, :, k * md:k * md + r][:, np.arange(md) % r]


@pytest.mark.parametrize("batch", [4, 6])
def test_one_wavefront_and_absent_problems(hip, oracle, batch):
    """the product instantiation on full-rank problems: one wavefront; a second one with two problems beyond the batch"""
    _, ref = Q.check(hip, oracle, P.lse_batch(52000 + batch, batch, N, DIMS))
    assert (ref["rank"] == [12, 12, 12, 4, 0]).all()


def test_finished_levels_shorter_than_the_ring(hip, oracle):
    """wavefront 0: level 0 of rank 0, 1, 2 and 12 side by side — level 1 runs twelve elimination steps, three problems meet the zeros of the x
    block in most of them.  Wavefront 1: level 0 of rank 1 in all four problems — level 1 has ONE step, the head's requests for the pivots 1
    and 2 are never used — then level 1 of rank 2: three steps in level 2.  Wavefront 2: level 0 empty everywhere (no step at all in level 1),
    level 1 of rank 2 (two steps, fewer than the ring is deep).  Wavefront 3: ranks 12, 0, 1, 2 in level 1 behind a full level 0"""
    lod = P.lse_batch(52100, 16, N, DIMS)
    for b, r in zip(range(0, 4), (0, 1, 2, 12)):
        if r < MD:
            level_of_rank(lod, b, 0, r)
    for b in range(4, 8):
        level_of_rank(lod, b, 0, 1)
        level_of_rank(lod, b, 1, 2)
    for b in range(8, 12):
        level_of_rank(lod, b, 0, 0)
        level_of_rank(lod, b, 1, 2)
    for b, r in zip(range(12, 16), (12, 0, 1, 2)):
        if r < MD:
            level_of_rank(lod, b, 1, r)
    _, ref = Q.check(hip, oracle, lod)
    np.testing.assert_array_equal(ref["rank"][:4, 0], [0, 1, 2, 12])
    np.testing.assert_array_equal(ref["fcol"][:4, 1], [0, 1, 2, 12])
    assert (ref["rank"][4:8, :2] == [1, 2]).all() and (ref["fcol"][4:8, 2] == 3).all()
    assert (ref["rank"][8:12, :2] == [0, 2]).all() and (ref["fcol"][8:12, 2] == 2).all()
    np.testing.assert_array_equal(ref["rank"][12:, 1], [12, 0, 1, 2])
    np.testing.assert_array_equal(ref["fcol"][12:, 2], [24, 12, 13, 14])


def test_level2_starts_at_different_columns(hip, oracle):
    """problem 1 has a level 0 of rank 11: its level 2 starts at column 23, its wavefront does not take the retiring form of level 2 and
    eliminates level 2's rows by 24 pivots for the other three's sake; the second wavefront retires.  The other three problems of the first
    wavefront give bit for bit what they give beside a full-rank problem 1"""
    full = P.lse_batch(52200, 8, N, DIMS)
    lod = full.copy()
    level_of_rank(lod, 1, 0, 11)
    s, ref = Q.check(hip, oracle, lod)
    np.testing.assert_array_equal(ref["fcol"][:, 2], [24, 23, 24, 24, 24, 24, 24, 24])
    t, _ = Q.check(hip, oracle, full)
    keep = [0, 2, 3, 4, 5, 6, 7]
    np.testing.assert_array_equal(s.get_x()[keep], t.get_x()[keep])
    np.testing.assert_array_equal(s.get_column_permutations()[keep], t.get_column_permutations()[keep])


@pytest.mark.parametrize("n,md,nobj,expect", [(36, 12, 4, "lqr_qtol<3,12>"), (24, 12, 3, "lqr_qtol<2,12>"), (40, 8, 6, "lqr_qtol<3,8>"), (24, 8, 4, "lqr_qtol<2,8>")])
def test_other_instantiations(hip, oracle, n, md, nobj, expect):
    """the instantiations that read n from the arguments, twelve and eight rows, three and two slots (three from n = 32 on): six problems (a
    wavefront with two absent ones), of which problem 1 has a level 0 of rank 1, problem 2 an empty one and problem 4 a level 1 of rank 2"""
    dims = [md] * nobj
    lod = P.lse_batch(52300 + 10 * n + md, 6, n, dims)
    level_of_rank(lod, 1, 0, 1, md)
    level_of_rank(lod, 2, 0, 0, md)
    level_of_rank(lod, 4, 1, 2, md)
    _, ref = Q.check(hip, oracle, lod, dims, expect=expect, n=n)
    np.testing.assert_array_equal(ref["rank"][[1, 2], 0], [1, 0])
    assert ref["rank"][4, 1] == 2 and (ref["rank"][[0, 3, 5], 0] == md).all()


@pytest.mark.parametrize("dims", [[12, 0, 12, 12, 12], [1, 3, 12, 12, 12]])
def test_ragged_empty_and_one_row_levels(hip, oracle, dims):
    """the ragged form (kernel policy 10), one hierarchy for the batch: an empty level; a one-row level in front (one finished pivot when level
    1 starts, four when level 2 does)"""
    R.check(hip, oracle, P.lse_batch(52400 + sum(dims), 6, N, dims), dims, N, expect="lqr_qtol<3,12,shift 7,ragged>")


def test_ragged_levels_differ_inside_a_wavefront(hip, oracle):
    """per-problem dimensions: an empty level, a one-row level and full levels side by side in one wavefront; two problems in the second"""
    dims = np.array([[12, 0, 12, 12, 12], [1, 3, 12, 12, 12], [12, 12, 12, 12, 12], [0, 1, 2, 12, 12], [2, 12, 0, 1, 12], [12, 12, 12, 12, 12]], np.uint32)
    R.check(hip, oracle, R.per_problem_batch(52500, 6, N, dims, 60), dims, N, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")
