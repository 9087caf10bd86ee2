"""The two references of the gradient of the LexLSE solve with respect to the matrix agree on the CPU (tests/adjoint_matrix_cases.py): the dense
KKT solve on the original data (A) against the numpy restatement of the kernels' steps on the oracle's factor (B).  The largest discrepancy is
D_CPU, from which the GPU tolerance follows.  The restated solve map is the transpose of the restated adjoint, the flags follow from the oracle's
ranks by the rule, and central differences of the oracle confirm (A) to their own accuracy.  No GPU."""
import numpy as np
import pytest

import adjoint_cases as AC
import adjoint_matrix_cases as AM


@pytest.fixture(scope="module")
def cases():
    return {name: AM.build(name) for name in AM.CASES}


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for c in cases.values():
        print(AM.summary(c))
    print(f"D_CPU measured {worst:.2e}, recorded {AM.D_CPU:.2e}, TOL {AM.TOL:.2e}")
    assert AM.TOL == max(10.0 * AM.D_CPU, 1e-12) and AM.TOL <= 1e-10
    assert max(10.0 * worst, 1e-12) <= AM.TOL, "the references disagree by more than the recorded D_CPU allows for: re-measure (or replace the data)"


def test_the_flags_follow_from_the_ranks_and_equal_the_literals(cases):
    assert set(AM.FLAGS) == set(AM.CASES) == set(AM.PRODUCERS)
    for name, c in cases.items():
        assert c["flags"].tolist() == AM.FLAGS[name], name
        n = c["n"]
        for b in range(len(c["flags"])):  # the rule once more, spelled out
            nf, rank, fcol, dims = int(c["nf"][b]), c["ref"]["rank"][b], c["ref"]["fcol"][b], c["dims"][b]
            want = 1 if nf >= n else int(all(int(rank[k]) == min(int(dims[k]), max(n - int(fcol[k]), 0)) for k in range(len(dims))))
            assert c["flags"][b] == want, (name, b)


def test_every_case_is_what_it_is_for(cases):
    rank = {k: c["ref"]["rank"] for k, c in cases.items()}
    assert (rank["ik"] == [12, 12, 12, 4, 0]).all() and cases["ik"]["n"] == 40
    assert (rank["rank_def"] == [2, 0, 2]).all() and (rank["fixed_rank_def"] == [2, 0, 2]).all() and cases["fixed_rank_def"]["nf"].tolist() == [2, 1, 3]
    assert (rank["mixed"] == [[3, 3, 1], [2, 0, 2]]).all()                                    # rank-stable beside rank-deficient
    assert (rank["used_up"][:, 2] == 0).all() and (rank["one_row"][:, 0] == 1).all()
    r = cases["ragged"]
    assert (r["ref"]["totalrank"] < r["n"]).sum() == 2 and (r["dims"].sum(axis=1) < sum(r["caps"])).any()  # free variables; absent rows
    f = cases["fixed"]
    assert f["nf"].tolist() == [2, 2, 5, 1] and not f["A"][2, :f["n"]].any()                   # every variable fixed: no gradient of A ...
    assert not f["A"][2].any()                                                                # ... and x does not depend on b either
    t = cases["fixed_tall"]
    assert t["caps"] == [70, 30] and (t["ref"]["hh"][:, :5] != 0).all() and (rank["fixed_tall"][:, 1] == 0).all()
    assert cases["wide"]["n"] > 64 and (cases["wide"]["dims"].sum(axis=1) > 64).all()
    for name, c in cases.items():
        m = c["dims"].sum(axis=1)
        for b in range(len(m)):
            assert not c["A"][b, :, m[b]:].any() and not c["B"][b, :, m[b]:].any()            # rows behind a problem's own
            if not c["flags"][b]:
                assert not c["A"][b].any() and not c["B"][b].any()
            elif c["nf"][b] < c["n"]:
                assert np.abs(c["A"][b, :c["n"]]).max() > 1e-3, (name, b)                     # there is a gradient to get wrong


def test_the_lambda_term_is_live(cases):
    """the second term of the formula matters wherever level k* has a residual: (B) without it misses (A) by far more than TOL"""
    for name in ("base", "used_up", "ik", "wide", "fixed_tall"):
        c = cases[name]
        G, u, lam, y = AM.reference_from_factor(c, c["ref"], 0)
        assert np.abs(np.outer(u, lam)).max() > 1e-3, name
        assert AC._rel(c["A"][0, :c["n"]] + np.outer(c["ref"]["x"][0], y), c["A"][0]) > 1e-4, name


def test_apply_solve_map_is_the_transpose_of_the_adjoint_and_matches_unit_solves(cases):
    for name, c in cases.items():
        assert c["dual"] <= AM.TOL / 10, (name, c["dual"])
    for name in ("base", "fixed"):
        c = cases[name]
        cols = AM.unit_solve_columns(c)
        for b in range(cols.shape[0]):
            r = c["ref"]
            got = np.stack([AM.apply_solve_map(r["factor"][b].T, r["hh"][b], r["perm"][b], r["rank"][b], r["fcol"][b], r["totalrank"][b], c["dims"][b],
                                               int(c["nf"][b]), e) for e in np.eye(cols.shape[2])], axis=1)
            assert AC._rel(got - cols[b], cols[b]) <= AM.TOL / 10, (name, b)


@pytest.mark.parametrize("name", ["base", "one_row", "ik"])
def test_central_differences_of_the_oracle_confirm_the_kkt_reference(name):
    gap = AM.fd_gap(name)
    print(f"{name}: {len(AM.fd_entries(name))} entries, central differences (h = {AM.FD_H:g}) against (A): {gap:.2e} (bound {AM.FD_BOUND:.0e})")
    assert gap <= AM.FD_BOUND
