"""The conditions on the near-singular cases of tests/rank_cases.py, from the CPU oracle alone: the GPU tests of
tests/test_gpu_rank_tolerance.py compare kernels with what these cases keep, so a case that kept nothing — or nothing that flips — would let
them pass on anything.  Conditions, not measurements: the measured figures are in the docstring of tests/rank_cases.py."""
import numpy as np
import pytest

import rank_cases as R


@pytest.fixture(scope="module", params=list(R.CASES))
def case(request):
    return R.build(request.param)


def test_tolerances_straddle_the_data():
    assert R.TOL_KEEP < R.DELTA ** 2 < R.TOL_DROP
    assert R.TOL_KEEP != R.TOL_DEFAULT != R.TOL_DROP  # a kernel that reads the default instead of the handle's value meets another one
    assert R.TOL_DEFAULT * R.FACTOR < R.DELTA ** 2


def test_shapes_have_as_many_rows_as_variables():
    """a hierarchy with fewer rows than variables never flips (n = 30, [9, 12, 5]: 0 flips of 64)"""
    for name, c in R.CASES.items():
        if c.get("near_row"):  # (a near-dependent row instead: it is a pivot of its own level whatever n)
            continue
        rows = c["per_problem"].sum(axis=1).min() if c.get("per_problem") is not None else sum(c["dims"])
        assert rows >= c["n"], name


def test_keeps_at_least_half(case):
    print(R.summary(case))
    assert case["drawn"] - case["dropped"] == len(case["flip"])
    assert 2 * len(case["flip"]) >= case["drawn"]


def test_at_least_a_quarter_flips_and_one_does_not(case):
    flips = int(case["flip"].sum())
    assert 4 * flips >= len(case["flip"])
    assert flips < len(case["flip"])
    # what flips is what was built to flip; the iid problems keep their ranks, and so do the exactly dependent ones (their breaks are at
    # ~1e-30 under every tolerance)
    assert case["flip"][case["kind"] == 0].all()
    assert not case["flip"][case["kind"] == 2].any()
    assert (~case["flip"][case["kind"] == 1]).any()


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "large"])  # (large: three problems, a workgroup each — no group of four)
def test_flipping_and_steady_problems_share_a_group_of_four(name):
    assert R.build(name)["mixed_groups"] >= 1


def test_mixed_case_has_all_three_kinds_side_by_side():
    case = R.build("ik")
    kinds = [set(case["kind"][i:i + 4].tolist()) for i in range(0, len(case["kind"]) - 3, 4)]
    assert sum(1 for k in kinds if k == {0, 1, 2}) >= 4


def test_kept_problems_are_stable(case):
    """same ranks and first columns a decade either side of each tolerance: a kernel's rounding of a fresh norm cannot move a rank"""
    for t, tol in R.TOLS.items():
        for f in (1.0 / R.FACTOR, R.FACTOR):
            o = R._run(case["name"], case["lod"], case["dims"], tol * f)
            np.testing.assert_array_equal(o["rank"], case["ref"][t]["rank"], err_msg=f"{t} x {f}")
            np.testing.assert_array_equal(o["fcol"], case["ref"][t]["fcol"], err_msg=f"{t} x {f}")


def test_threshold_is_on_the_squared_norm(case):
    """some flipping problem's pivot lies between tol_drop^2 and tol_drop: compared by its norm it would survive tol_drop"""
    assert case["norm_sensitive"] >= 1
    s = case["smallest_pivot_sq"]
    assert (s[case["flip"]] < R.TOL_DROP / R.FACTOR).all() and (s > R.TOL_DEFAULT * R.FACTOR).all()


def test_tol_drop_leaves_well_conditioned_problems(case):
    """with the small pivot gone x is determined to far better than contract (T)'s 1e-10: the plain bound applies there"""
    assert case["sens"]["drop"].max() <= 1e-12
    assert np.isfinite(case["ref"]["keep"]["x"]).all() and np.isfinite(case["ref"]["drop"]["x"]).all()
    assert (case["ref"]["keep"]["totalrank"] >= case["ref"]["drop"]["totalrank"]).all()
