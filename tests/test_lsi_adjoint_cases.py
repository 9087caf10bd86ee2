"""The two references of the gradients of LexLSI solutions with respect to the bounds agree on the CPU (tests/lsi_adjoint_cases.py): (A) the
adjoint of the final equality problem of the oracle's working set, scattered to constraint order, against (B) differences through the whole oracle
LexLSI driver under three bound perturbations per case.  The largest discrepancy is D_CPU, from which the GPU tolerance follows.  No GPU."""
import numpy as np
import pytest

import adjoint_cases as AC
import lsi_adjoint_cases as LC


@pytest.fixture(scope="module")
def cases():
    return {name: LC.build(name) for name in LC.CASES}


def test_every_perturbed_solve_keeps_status_and_working_set(cases):
    """the condition under which (B) is exact: no instance is left out"""
    for c in cases.values():
        assert (c["status"] == LC.SOLVED).all(), c["name"]
        assert c["held"], f"{c['name']}: a perturbed solve left the working set of the unperturbed one (or did not end PROBLEM_SOLVED)"
        assert len(c["pairs"]) == 3 and all(np.abs(p[2]).max() > 1e-6 for p in c["pairs"]), c["name"]


def test_the_references_agree_and_the_tolerance_follows_from_their_gap(cases):
    worst = max(c["gap"] for c in cases.values())
    for c in cases.values():
        print(LC.summary(c))
    print(f"D_CPU measured {worst:.2e}, recorded {LC.D_CPU:.2e}, TOL {LC.TOL:.2e}")
    assert LC.TOL == max(10.0 * LC.D_CPU, 1e-12) and LC.TOL <= 1e-10
    assert max(10.0 * worst, 1e-12) <= LC.TOL, "the references disagree by more than the recorded D_CPU allows for: re-measure (or replace the data)"
    for c in cases.values():
        glb, gub = c["A"]
        for dlb, dub, dx in c["pairs"]:
            assert AC.identity_gap((np.hstack([dlb, dub]), dx), c["g"], np.hstack([glb, gub])) <= LC.TOL / 10, c["name"]


def test_zeros_outside_the_working_set_and_the_routing_by_type(cases):
    for c in cases.values():
        glb, gub = c["A"]
        act = c["active"]
        assert not glb[act != LC.LB].any(), c["name"]              # grad_lb lives on CTR_ACTIVE_LB alone
        assert not gub[(act != LC.UB) & (act != LC.EQ)].any(), c["name"]  # grad_ub on CTR_ACTIVE_UB and CTR_ACTIVE_EQ
        assert not glb[act == 0].any() and not gub[act == 0].any()
        assert set(np.unique(act)) <= {0, LC.LB, LC.UB, LC.EQ}
    # across the cases every type occurs, with values that are not zero
    act = np.concatenate([c["active"].ravel() for c in cases.values()])
    glb = np.concatenate([c["A"][0].ravel() for c in cases.values()])
    gub = np.concatenate([c["A"][1].ravel() for c in cases.values()])
    assert np.abs(glb[act == LC.LB]).max() > 1e-3 and np.abs(gub[act == LC.UB]).max() > 1e-3 and np.abs(gub[act == LC.EQ]).max() > 1e-3


def test_every_case_is_what_it_is_named_for(cases):
    sb = cases["small_sb"]
    assert "var" in sb["probs"][0][0] and sb["n"] == 4 and sb["dims"].tolist() == [4, 2, 2] and len(sb["probs"]) == 4
    assert (sb["active"][:, :4] != 0).any(), "no active simple bound"
    assert np.abs(np.where(sb["active"][:, :4] != 0, sb["A"][0][:, :4] + sb["A"][1][:, :4], 0.0)).max() > 1e-3  # grad_fixed reaches the bounds
    ge = cases["general"]
    assert all("A" in o for o in ge["probs"][0]) and ge["n"] == 5 and ge["dims"].tolist() == [3, 2, 3]
    rd = cases["rank_def"]
    for b, objs in enumerate(rd["probs"]):
        assert np.array_equal(objs[0]["A"][0], objs[1]["A"][0])
        assert rd["active"][b, 0] == LC.EQ and rd["active"][b, 3] == LC.EQ  # both copies are in the working set ...
    nact = np.stack([[np.count_nonzero(a) for a in r["active"]] for r in rd["runs"]])
    assert (rd["ranks"][:, 1] < nact[:, 1]).all()                           # ... and level 1 has fewer ranks than rows
    em = cases["empty_ws"]
    for b in LC.CASES["empty_ws"]["empty"]:
        assert not em["active"][b].any() and not em["runs"][b]["x"].any()
        assert not em["A"][0][b].any() and not em["A"][1][b].any()
    assert em["active"][0].any() and em["active"][2].any()
    ik = cases["ik"]
    assert ik["n"] == 40 and ik["dims"].tolist() == [12] * 5 and len(ik["probs"]) == 8 and "var" in ik["probs"][0][0]


def test_the_budget_case_has_both_kinds_of_instances():
    bd = LC.build_budget()
    wide = list(LC.BUDGET["wide"])
    rest = [b for b in range(LC.BUDGET["batch"]) if b not in wide]
    assert (bd["status"][wide] == LC.SOLVED).all() and (bd["status"][rest] == 2).all()  # MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED
    for b in rest:
        assert not bd["A"][0][b].any() and not bd["A"][1][b].any()
        assert bd["active"][b].any()  # a working set, but not a solved one: zeros are the status rule's, not an empty set's
    for b in wide:
        assert np.abs(bd["A"][1][b]).max() > 1e-3


def test_the_tile_case_has_active_rows_on_both_sides_of_the_tile_edge():
    tl = LC.build_tile()
    total = int(tl["dims"].sum())
    assert LC.ADJ_TILE < total < 2 * LC.ADJ_TILE and tl["active"].shape == (2, total) and (tl["status"] == LC.SOLVED).all()
    eq = [4 + r for r in LC.TILE["equalities"]]  # user rows of the two equalities of the second objective
    assert eq[0] < LC.ADJ_TILE < eq[1]
    glb, gub = tl["A"]
    for b in range(2):
        rows = np.flatnonzero(tl["active"][b])
        assert set(eq) <= set(rows.tolist()) and set(rows.tolist()) <= set(range(4)) | set(eq) | {total - 2, total - 1}  # the far inequalities stay out
        assert (tl["active"][b, eq] == LC.EQ).all() and (np.abs(gub[b, eq]) > 1e-3).all()                         # values on both sides of row 1024
        assert not glb[b, tl["active"][b] != LC.LB].any() and not gub[b, (tl["active"][b] != LC.UB) & (tl["active"][b] != LC.EQ)].any()
    assert (tl["active"][:, :4] != 0).any() and np.abs(gub[:, total - 2:]).max() > 1e-3  # a simple bound (grad_fixed) and the last tile's last rows
