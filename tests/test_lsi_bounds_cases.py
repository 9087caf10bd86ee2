"""The references of tests/lsi_bounds_cases.py against each other, on the CPU: (A), the final equality problem re-formed from scratch with the new
bounds, against (B), x_run + M (b_new - b_run) from unit solves on the run's problem; the semantic check through the oracle's whole LexLSI driver;
the violation of the large perturbation; the run's own bounds.  The largest (A)-(B) gap is D_CPU, from which the GPU tolerance follows.  No GPU."""
import numpy as np
import pytest

import lsi_bounds_cases as BC


def rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def test_tolerance_follows_from_the_measured_discrepancy():
    worst = 0.0
    for name in BC.CASES:
        case = BC.build(name)
        print(BC.summary(case))
        worst = max(worst, case["gap"])
    print(f"D_CPU measured {worst:.2e}, recorded {BC.D_CPU:.2e}, TOL {BC.TOL:.2e}")
    assert BC.TOL == 10.0 * BC.D_CPU and BC.TOL <= 1e-10
    assert worst <= BC.D_CPU, "the references disagree by more than the recorded D_CPU: re-measure (or replace the data)"
    assert worst >= 0.1 * BC.D_CPU, "the recorded D_CPU is far above what the references show: re-measure"


@pytest.mark.parametrize("name", BC.CASES)
def test_small_perturbations_keep_the_working_set_and_the_driver_agrees_with_a(name):
    """asserted, never skipped: the oracle's driver run from scratch on the first N_SEM small bound sets ends PROBLEM_SOLVED on the run's working
    set for every solved instance, and its x is (A)'s within TOL"""
    case = BC.build(name)
    assert case["held"], name
    print(f"{name}: driver against (A) {case['sem_gap']:.2e} (TOL {BC.TOL:.1e})")
    assert case["sem_gap"] <= BC.TOL, name
    assert (case["status"] == BC.SOLVED).any()


@pytest.mark.parametrize("name", BC.CASES)
def test_own_bounds_large_perturbation_and_stopped_instances(name):
    case = BC.build(name)
    solved = case["status"] == BC.SOLVED
    for i in np.flatnonzero(solved):
        assert rel(case["A"][0, i], case["x_run"][i]) <= BC.TOL, (name, i)  # with the run's own bounds x is the run's x
        assert case["violation"][-1, i] > 0.0, (name, i)                    # the large perturbation leaves the region
    assert not case["A"][:, ~solved].any() and not case["violation"][:, ~solved].any()
    empty = [i for i in np.flatnonzero(solved) if not case["active"][i].any()]
    assert not case["A"][:, empty].any()
    if name == "empty_ws":
        assert empty == [1, 3] and (case["violation"][-1, empty] > 0.0).all()  # measured against x = 0
    if name == "budget":
        assert case["status"].tolist() == [0, 2, 0, 2, 0, 2]


def test_the_cases_reach_what_they_are_for():
    types = set()
    for name in BC.CASES:
        types |= set(np.unique(BC.build(name)["active"]).tolist())
    assert {1, 2, 3} <= types  # CTR_ACTIVE_LB, _UB, _EQ
    for name in ("sb3", "ik", "rows"):  # active simple bounds: fixed variables
        case = BC.build(name)
        assert case["active"][:, :int(case["dims"][0])].any(), name
    assert int(BC.build("rows")["dims"].sum()) > 64
    ranks = BC.LC.build("rank_def")["ranks"]
    dims = np.stack([BC.LC.final_problem(5, objs, r["active"])[1] for objs, r in zip(BC.build("rank_def")["probs"], BC.build("rank_def")["runs"])])
    assert (ranks < dims).any()  # a level of rank < rows


def test_violation_definition_on_a_hand_made_instance():
    objs = [dict(var=np.array([1], np.uint32), lb=np.array([0.5]), ub=np.array([2.0])),
            dict(A=np.array([[1.0, 1.0], [1.0, -1.0]]), lb=np.array([0.0, 3.0]), ub=np.array([1.0, 2.0]))]
    x = np.array([2.0, 0.25])
    # simple bound: lb - x[1] = 0.25; row 0: a.x - ub = 1.25; row 1: lb - ub = 1 and lb - a.x = 1.25
    assert BC.violation_of(2, objs, x) == 1.25
    assert BC.violation_of(2, objs, x, counts=[1, 0]) == 0.25
    assert BC.violation_of(2, objs, x, counts=[0, 0]) == 0.0
    assert 0.0 < BC.violation_bound(2, objs, x) < 1e-15
