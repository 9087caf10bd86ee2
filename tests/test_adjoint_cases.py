"""The two references of the adjoint of the LexLSE solve agree on the CPU (tests/adjoint_cases.py): M^T g, N^T g from unit solves on the
oracle (A) against the numpy restatement of the kernel's steps on the oracle's factor (B); for the large cases (B) against three dot-product
identities on oracle forward solves.  The largest discrepancy is D_CPU, from which the GPU tolerance follows.  No GPU."""
import numpy as np
import pytest

import adjoint_cases as AC


@pytest.fixture(scope="module")
def cases():
    return {name: AC.build(name) for name in AC.CASES}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for c in cases.values():
        print(AC.summary(c))
    print(f"D_CPU measured {worst:.2e}, recorded {AC.D_CPU:.2e}, TOL {AC.TOL:.2e}")
    assert AC.TOL == max(10.0 * AC.D_CPU, 1e-12) and AC.TOL <= 1e-10
    assert max(10.0 * worst, 1e-12) <= AC.TOL, "the references disagree by more than the recorded D_CPU allows for: re-measure (or replace the data)"


def test_every_case_is_what_it_is_for(cases):
    rank = {k: c["ref"]["rank"] for k, c in cases.items()}
    n = {k: c["n"] for k, c in cases.items()}
    assert (rank["base"].sum(axis=1) == n["base"]).all()
    assert (rank["used_up"][:, 0] + rank["used_up"][:, 1] == n["used_up"]).all() and (rank["used_up"][:, 2] == 0).all()  # used up before the last level
    assert (rank["one_row"][:, 0] == 1).all() and cases["one_row"]["caps"][0] == 1                                      # R == 1: no reflector
    assert (cases["one_row"]["ref"]["hh"][:, 0] == 0).all()
    assert (rank["rank_def"] == [2, 0, 2]).all()                                                                        # a rank-0 level, rank < dim
    assert (cases["ragged"]["dims"] == 0).any() and (cases["ragged"]["dims"].sum(axis=1) < sum(cases["ragged"]["caps"])).any()
    f = cases["fixed"]
    assert f["fixed"]["nfixed"].tolist() == [2, 2, 5, 1] and f["fixed"]["fixed_idx"][0, :2].tolist() == [1, 0]
    assert (rank["fixed"][2] == 0).all() and f["ref"]["totalrank"][2] == 5                                              # the all-fixed early return
    assert n["wide"] > 64 and n["large"] > 64 and cases["wide"]["large"] and cases["large"]["large"]
    assert (rank["large"] == [[17, 1, 0, 5, 10], [9, 0, 0, 16, 8]]).all()


def test_the_fixed_cases_meet_the_other_edges(cases):
    """what fixed_wide, fixed_rank_def, fixed_ragged and fixed_tall are named for, from the oracle's rank / fcol / totalrank"""
    def of(name):
        c = cases[name]
        r = c["ref"]
        return c, c["fixed"]["nfixed"].astype(int), r["rank"].astype(int), r["fcol"].astype(int), r["totalrank"].astype(int), c["dims"].sum(axis=1).astype(int)

    for name in ("fixed_wide", "fixed_rank_def", "fixed_ragged", "fixed_tall"):
        c, nf, rank, fcol, T, m = of(name)
        assert c["A"] is not None and not c["large"]                       # reference (A): the unit solves
        np.testing.assert_array_equal(fcol[:, 0], nf)                      # the pivot columns start behind the fixed ones ...
        np.testing.assert_array_equal(T, nf + rank.sum(axis=1))            # ... and end at T
        for b in range(len(nf)):
            assert sorted(c["fixed"]["fixed_idx"][b, :nf[b]].tolist()) == sorted(set(c["fixed"]["fixed_idx"][b, :nf[b]].tolist()))
            if nf[b]:
                assert np.abs(AC.expected(c)[1][b, :nf[b]]).max() > 1e-2, (name, b)  # grad_fixed is not 0: step (d) has something to get wrong

    c, nf, rank, fcol, T, m = of("fixed_wide")
    assert c["n"] > 64 and nf.tolist() == [6, 9, 0]                        # nfixed == 0 beside nfixed > 0; pivot columns [nf, T) at n > 64
    assert nf[0] > 4 and nf[1] > 8                                         # step (d): a second and a third group of AU = 4 columns
    assert (m > 64).all() and (T == c["n"]).all()                          # column_dot makes a second trip; every column is a pivot or fixed
    assert (rank == [[20, 40, 4], [20, 40, 1], [20, 40, 10]]).all()
    assert np.abs(AC.expected(c)[0][:, 64:]).min(axis=1).min() > 0         # cb is live behind row 64
    assert [c["fixed"]["fixed_idx"][b, :nf[b]].tolist() for b in range(3)] == [AC.WIDE_ORDER[:6], AC.WIDE_ORDER[:9], []]
    assert sorted(AC.WIDE_ORDER) == list(range(70))

    c, nf, rank, fcol, T, m = of("fixed_rank_def")
    assert nf.tolist() == [2, 1, 3] and (rank == [2, 0, 2]).all()          # a rank-0 level, rank < dim, behind fixed columns
    assert len(set(T.tolist())) == 3 and (T <= c["n"]).all()               # another T per problem
    assert (rank < c["dims"]).all()

    c, nf, rank, fcol, T, m = of("fixed_ragged")
    assert nf.tolist() == [2, 0, 4, 1] and (c["dims"] == AC.RAGGED_DIMS).all() and (c["dims"] == 0).any()
    assert (c["dims"][nf > 0] == 0).any()                                  # an empty level in a problem with fixed variables
    assert c["n"] - nf[2] == 1 and rank[2].tolist() == [1, 0, 0]           # one free variable
    assert ((fcol >= T[:, None]) & (c["dims"] > 0) & (nf[:, None] > 0)).any()  # a level with rows finds the columns used up
    assert (rank == [[2, 1, 0], [2, 0, 2], [1, 0, 0], [0, 3, 1]]).all()

    c, nf, rank, fcol, T, m = of("fixed_tall")
    assert nf.tolist() == [5, 7] and c["caps"] == [70, 30] and (m == 100).all()  # reflectors over 70 rows, step (d) over 100
    assert (rank[:, 0] == c["n"] - nf).all() and (rank[:, 1] == 0).all() and (fcol[:, 1] == c["n"]).all()  # the columns are gone
    assert (c["ref"]["hh"][:, :5] != 0).all()                              # the reflectors over 70, 69, ... rows exist


def test_absent_rows_and_slots_are_zero_and_the_rest_is_not(cases):
    for c in cases.values():
        grad_rhs, grad_fixed = AC.expected(c)
        m = c["dims"].sum(axis=1)
        nf = c["fixed"]["nfixed"] if c["fixed"] else np.zeros(len(m), np.uint32)
        for b in range(len(m)):
            assert not grad_rhs[b, m[b]:].any() and not grad_fixed[b, nf[b]:].any()
            assert np.abs(grad_rhs[b, :m[b]]).max() > 1e-3 or nf[b] == c["n"], (c["name"], b)
            if nf[b]:
                assert np.abs(grad_fixed[b, :nf[b]]).min() > 1e-6, (c["name"], b)
    f = cases["fixed"]
    np.testing.assert_array_equal(AC.expected(f)[0][2], 0.0)  # every variable fixed: x does not depend on b ...
    np.testing.assert_allclose(AC.expected(f)[1][2, :5], f["g"][2, [2, 0, 4, 1, 3]], rtol=0, atol=1e-15)  # ... and x[idx[j]] = value j


def test_the_large_cases_hold_their_identities(cases):
    for name in ("wide", "large"):
        c = cases[name]
        assert len(c["pairs"]) == 3
        for pair in c["pairs"]:
            assert np.abs(pair[1]).max() > 1e-3
            assert AC.identity_gap(pair, c["g"], c["B"][0]) <= AC.TOL / 10
