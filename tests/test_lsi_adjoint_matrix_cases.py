"""The references of tests/lsi_adjoint_matrix_cases.py held to each other on the CPU (the oracle and numpy alone): (A) against the central
differences (B) on every case with a (B), the flags, D_CPU re-measured, and the exact zeros of (A) itself."""
import numpy as np
import pytest

import adjoint_matrix_cases as MC
import lsi_adjoint_cases as LC
import lsi_adjoint_matrix_cases as XC


@pytest.mark.parametrize("name", XC.WITH_B)
def test_reference_a_against_central_differences(name):
    case = XC.build(name)
    assert case["held"], f"{name}: a perturbed solve left the working set (shrink DIRECTION_SCALE[{name!r}])"
    flagged = np.flatnonzero(case["flags"])
    assert flagged.size  # (B) covers every flag-1 instance of the case
    for b in flagged:
        ip = float(case["A"][b] @ case["dD"][b])
        gap = abs(case["fd"][b] - ip) / max(1.0, float(np.abs(case["A"][b] * case["dD"][b]).sum()))
        print(f"{name}[{b}]: fd {case['fd'][b]:+.9e}  <grad_data, dD> {ip:+.9e}  gap {gap:.1e} (FD_BOUND {XC.FD_BOUND:.1e})")
        assert gap <= XC.FD_BOUND, (name, b, gap)
        assert (case["dD"][b] != 0).all()  # the direction moves all data, inactive rows included
    assert case["gapB"] <= XC.GAP_B * 1.0000001  # the table's figure is the largest measured


def test_the_bound_on_b_follows_from_the_measurement():
    assert XC.FD_BOUND == min(10.0 * XC.GAP_B, 1e-6) and XC.FD_BOUND <= 1e-6
    assert XC.FD_H == MC.FD_H and XC.FD_BOUND != MC.FD_BOUND


@pytest.mark.parametrize("name", XC.CASES)
def test_flags(name):
    """the literals, the rule on the oracle's ranks of the final problems, and what the issue says of each case"""
    case = XC.build(name)
    assert case["flags"].tolist() == XC.FLAGS[name]
    for b, flag in enumerate(case["flags"]):
        assert flag == 0 or case["status"][b] == LC.SOLVED
    if name == "rank_def":
        assert [np.asarray(r).tolist() for r in case["ranks"][1:]] == [[3, 1, 1]] * 3 and (case["status"] == LC.SOLVED).all()
    if name == "budget":
        assert case["status"].tolist() == [0, 2, 0, 2, 0, 2]
    if name == "empty_ws":
        assert not case["active"][1].any() and not case["active"][3].any() and case["active"][0].any()
    if name == "ik":
        assert [12, 10, 11, 5] in [np.asarray(r).tolist() for r in case["ranks"]]
    if name == "mixed":
        assert (case["flags"][:-1] != case["flags"][1:]).all()  # the flags differ between neighbours
    if name == "tile":
        rows = [np.flatnonzero(a) for a in case["active"]]
        assert case["active"].shape[1] == 1036 and all((r < LC.ADJ_TILE).any() and (r > LC.ADJ_TILE).any() for r in rows)


def test_d_cpu_and_tol():
    worst = max(XC.build(name)["d"] for name in XC.CASES)
    print(f"D_CPU re-measured {worst:.3e} (the file has {XC.D_CPU:.3e})")
    assert worst <= XC.D_CPU * 1.01 and worst >= XC.D_CPU / 2  # the figure in the file is the measured one
    assert XC.TOL == max(10.0 * XC.D_CPU, 1e-12) and XC.TOL <= 1e-10


@pytest.mark.parametrize("name", XC.CASES)
def test_exact_zeros_of_reference_a(name):
    """every flag-0 slice is all zeros; every row outside W is all zeros; a flag-1 instance with a working set carries something"""
    case = XC.build(name)
    for b, flag in enumerate(case["flags"]):
        parts, nonzero = XC.split(case, case["A"][b])
        if not flag:
            assert not case["A"][b].any(), (name, b)
            continue
        active = case["active"][b] != 0
        assert not nonzero[~active].any(), (name, b)
        assert nonzero.any() == active.any(), (name, b)  # (rows of W behind the last level of non-zero rank do not touch x: zeros there too)
        # the type rule: the bound column a row does not sit at is zero
        lb, ub = np.concatenate([p["lb"] for p in parts]), np.concatenate([p["ub"] for p in parts])
        assert not lb[case["active"][b] != LC.LB].any() and not ub[(case["active"][b] != LC.UB) & (case["active"][b] != LC.EQ)].any()


def test_bound_columns_are_the_bounds_adjoint():
    """the bound columns of (A) against the reference of lsi_adjoint_cases (unit solves on the oracle): two formations of the same numbers"""
    for name in ("small_sb", "general", "empty_ws", "ik"):
        case, lc = XC.build(name), LC.build(name)
        np.testing.assert_array_equal(case["active"], lc["active"])
        for b in range(len(case["probs"])):
            # lsi_adjoint_cases has its own g: the identity is linear in g, so compare through the case's own gradient of the same g
            glb, gub, _ = LC.reference_a(case["n"], [case["probs"][b]], [case["runs"][b]["active"]], [case["status"][b]], case["g"][b][None])
            parts, _ = XC.split(case, case["A"][b])
            lb, ub = np.concatenate([p["lb"] for p in parts]), np.concatenate([p["ub"] for p in parts])
            scale = max(1.0, float(np.abs(glb).max()), float(np.abs(gub).max()))
            assert np.abs(lb - glb[0]).max() / scale <= XC.TOL and np.abs(ub - gub[0]).max() / scale <= XC.TOL, (name, b)
