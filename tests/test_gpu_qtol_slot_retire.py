"""lqr_qtol's slot retirement (lexls_amd/csrc/lqr_qtol_body.inc, RETIRE): a level that starts with two live slots, the lower holding one live
column per problem, drops that slot behind its first pivot step — the lone column moves into the register place of the step's pivot.  On the
IK shape (n = 40, five levels of 12 rows, the shift-7 instantiation) that is level 2, which starts at column 24.  The cases are the smallest
at which the move can go wrong: the lone column wins the first step (no move), wins last or never, a wavefront that must not take the path
(a problem of it starts level 2 elsewhere; rows beyond the batch), a level that stops on the rank test behind the move, a level without
work (no pivot at all: no move, the slot's maps are stored by the level end), alone and beside problems that do move.
Acceptance = tests/test_gpu_qtol.py::check (contract (T) of include/lexls_hip.h): column permutation, ranks, first columns and total rank
EXACT, x within 1e-10 relative to max(1, |x|_inf).  What every constructed problem is built for is asserted on the oracle's result."""
import numpy as np
import pytest

import test_gpu_qtol as Q
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

N, DIMS, MD = Q.N, Q.DIMS, 12
FC2 = 2 * MD  # level 2's first column when the levels above are full: place (24 + 7) = lane 15 of slot 1
L2 = slice(2 * MD, 3 * MD)  # level 2's rows


def columns_at_positions(perm, steps):
    """physical column at every position after the first `steps` pivot steps (perm[P]: the position swapped to the front at step P)"""
    phys = np.arange(N)
    for p in range(steps):
        q = int(perm[p])
        phys[p], phys[q] = phys[q], phys[p]
    return phys


def pivots_of_steps(perm, lo, hi):
    """physical columns chosen at the pivot steps lo .. hi-1"""
    phys = columns_at_positions(perm, lo)
    out = []
    for p in range(lo, hi):
        q = int(perm[p])
        out.append(int(phys[q]))
        phys[p], phys[q] = phys[q], phys[p]
    return out


def scaled_lone_column(oracle, seed, batch, factor, reduced=False):
    """the lone column times `factor` in level 2's rows.  reduced: what is scaled is the column as level 2 factorises it, that is behind the
    elimination by the pivots of the levels 0 and 1 — a_c - A_S w with S those 24 pivot columns and w = A01_S^-1 A01_c from the rows above;
    the part A_S w, which comes from the other columns' entries and which scaling the raw entries leaves as large as it was, stays"""
    lod = P.lse_batch(seed, batch, N, DIMS)
    ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
    assert (ref["rank"][:, :2] == MD).all()
    lone = []
    for b in range(batch):
        phys = columns_at_positions(ref["perm"][b], FC2)
        c, S = int(phys[FC2]), phys[:FC2]
        lone.append(c)
        if reduced:
            w = np.linalg.solve(lod[b, S, :FC2].T, lod[b, c, :FC2])
            through = w @ lod[b, S, L2]
            lod[b, c, L2] = through + factor * (lod[b, c, L2] - through)
        else:
            lod[b, c, L2] *= factor
    return lod, lone


def against_bit_exact_kernel(hip, s, lod):
    """the bit-exact kernel of the same mapping (kernel policy 4): same pivots, x within the tolerance"""
    e = Q.solve(hip, lod, policy=4)
    assert e.last_kernel() == "lqr_quad<3,12,shift 7>"
    np.testing.assert_array_equal(e.get_column_permutations(), s.get_column_permutations())
    np.testing.assert_array_equal(e.getRanks()[0], s.getRanks()[0])
    assert np.abs(e.get_x() - s.get_x()).max() <= Q.TOL * max(1.0, float(np.abs(e.get_x()).max()))


def test_two_wavefronts(hip, oracle):
    """batch 8, iid N(0,1): both wavefronts retire slot 1 in level 2"""
    lod = P.lse_batch(47000, 8, N, DIMS)
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"] == [12, 12, 12, 4, 0]).all() and (ref["fcol"][:, 2] == FC2).all()
    against_bit_exact_kernel(hip, s, lod)


def test_partly_empty_wavefront(hip, oracle):
    """batch 5: the second wavefront holds one problem — it does not take the path (three of its rows do not work)"""
    lod = P.lse_batch(47100, 5, N, DIMS)
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"] == [12, 12, 12, 4, 0]).all()
    against_bit_exact_kernel(hip, s, lod)


def test_lone_column_wins_the_first_step(hip, oracle):
    """the lone column, 1e3 times larger in level 2's rows, is level 2's first pivot: nothing moves, slot 1 is simply dead"""
    lod, lone = scaled_lone_column(oracle, 47200, 8, 1e3)
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"] == [12, 12, 12, 4, 0]).all()
    for b, c in enumerate(lone):
        assert int(ref["perm"][b, FC2]) == FC2 and pivots_of_steps(ref["perm"][b], FC2, FC2 + 1) == [c]
    against_bit_exact_kernel(hip, s, lod)


def test_lone_column_wins_last_or_never(hip, oracle):
    """the lone column, 1e-3 times smaller in level 2's rows as the level factorises them, is not among level 2's first eleven pivots: it
    lives in its new place through every step of the level.  (Scaling its raw entries does not do that: the elimination by the levels
    above adds the other columns' entries to it, and it is chosen early all the same — the assertion below fails on such data.)"""
    lod, lone = scaled_lone_column(oracle, 47300, 8, 1e-3, reduced=True)
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"] == [12, 12, 12, 4, 0]).all()
    for b, c in enumerate(lone):
        assert c not in pivots_of_steps(ref["perm"][b], FC2, FC2 + MD - 1)
    against_bit_exact_kernel(hip, s, lod)


def test_one_problem_starts_level2_elsewhere(hip, oracle):
    """problem 1 has a level 0 of rank 11 (two equal rows): its level 2 starts at column 23, its wavefront keeps the unretired path, the
    second wavefront retires.  The other three problems of the first wavefront give bit for bit what they give beside a full-rank
    problem 1, where their wavefront retires the slot: the two paths agree exactly"""
    full = P.lse_batch(47400, 8, N, DIMS)
    lod = full.copy()
    lod[1, :, 1] = lod[1, :, 0]
    s, ref = Q.check(hip, oracle, lod)
    np.testing.assert_array_equal(ref["rank"][1], [11, 12, 12, 5, 0])
    assert (np.delete(ref["rank"], 1, axis=0) == [12, 12, 12, 4, 0]).all()
    t = Q.solve(hip, full)
    keep = [0, 2, 3, 4, 5, 6, 7]
    np.testing.assert_array_equal(s.get_x()[keep], t.get_x()[keep])
    np.testing.assert_array_equal(s.get_column_permutations()[keep], t.get_column_permutations()[keep])
    np.testing.assert_array_equal(s.getRanks()[0][keep], t.getRanks()[0][keep])


def test_rank_deficient_level2(hip, oracle):
    """level 2 has seven different rows (the last five repeat the first five): it stops on the rank test behind the move; level 3 starts
    at column 31 and takes the nine columns left"""
    lod = P.lse_batch(47500, 8, N, DIMS)
    lod[:, :, 2 * MD + 7:3 * MD] = lod[:, :, 2 * MD:2 * MD + 5]
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"] == [12, 12, 7, 9, 0]).all() and (ref["fcol"][:, 3] == FC2 + 7).all()
    against_bit_exact_kernel(hip, s, lod)


def test_level2_without_work(hip, oracle):
    """level 2 all zero — in every problem of the first wavefront, in one problem of the second (beside three that move their lone
    column): no pivot, no move; level 3 then starts at column 24 itself and retires the slot"""
    lod = P.lse_batch(47600, 8, N, DIMS)
    empty = [0, 1, 2, 3, 5]
    lod[empty, :, L2] = 0.0
    s, ref = Q.check(hip, oracle, lod)
    assert (ref["rank"][empty] == [12, 12, 0, 12, 4]).all() and (ref["fcol"][empty, 3] == FC2).all()
    assert (np.delete(ref["rank"], empty, axis=0) == [12, 12, 12, 4, 0]).all()
    against_bit_exact_kernel(hip, s, lod)
