"""The conditions on the cases of tests/postfactor_cases.py, from the CPU oracle alone: tests/test_gpu_postfactor.py compares the
post-factorization kernels with what these cases carry, so a case whose multipliers are all zero, whose least-norm solution is the basic one or
whose scan always stops at the same level would let them pass on anything — and at these sizes the oracle has no other judge, so it is held
to the mathematics here.  Conditions, not measurements: the measured figures are in the docstring of tests/postfactor_cases.py."""
import numpy as np
import pytest

import postfactor_cases as C


@pytest.fixture(scope="module", params=list(C.CASES))
def case(request):
    return C.build(request.param)


def test_docstring_table_is_what_the_module_measures(case):
    print(C.summary(case))
    assert C.summary(case) in C.__doc__


def test_shapes_cross_the_boundaries_they_are_for():
    c = C.CASES
    for name in ("n63", "n64", "n65"):  # sweepable but for n: levels <= 16 rows, <= 8 objectives, more rows than variables
        assert max(c[name]["dims"]) <= 16 and len(c[name]["dims"]) <= 8 and sum(c[name]["dims"]) > c[name]["n"]
    assert [c[k]["n"] for k in ("n63", "n64", "n65")] == [63, 64, 65]
    assert max(c["row17"]["dims"]) == 17 and len(c["row17"]["dims"]) <= 8 and c["row17"]["n"] <= 64 and sum(c["row17"]["dims"]) > c["row17"]["n"]
    assert len(c["obj9"]["dims"]) == 9 and max(c["obj9"]["dims"]) <= 16 and c["obj9"]["n"] <= 64 and sum(c["obj9"]["dims"]) > c["obj9"]["n"]

    def staged(name, batch=None):  # launch_sensitivity's lds_staged
        n, cap = c[name]["n"], sum(c[name]["dims"])
        return 8 * (2 * n + cap + 2) + 64 + 16 + 8 * ((cap | 1) * (n + 1) + cap) + ((cap + n + 15) & ~15)
    assert staged("large") > 160 * 1024 and c["large"]["batch"] == 1 and c["large"]["dims"] == [115, 115] and c["large"]["n"] == 100
    assert 64 * 1024 + 4096 < staged("staged") <= 160 * 1024 - 4096 and c["staged"]["batch"] <= 8  # (4 KB either way: SensState's size is the kernel's business)
    assert staged("tiny") <= 40 * 1024 and c["tiny"]["n"] <= 5 and c["tiny"]["batch"] == 1025
    assert sum(c["blocks"]["dims"]) > 200 and c["blocks"]["n"] > 2 * 64 + 1 and c["blocks"]["batch"] == 3


def test_blocked_solve_meets_every_loop():
    """level ranks on both sides of the 64-row blocks, and columns of the levels below (acc) that run the 64-wide loop, the 16-wide loop and the
    scalar tail of solve_generic_kernel<256>"""
    case = C.build("blocks")
    for b in range(case["lod"].shape[0]):
        ranks = case["rank"][b].tolist()
        assert {64, 65, 1} <= set(ranks)
        assert max(ranks) >= 129 or sum(sorted(ranks)[-2:]) > 128
        acc, loops = 0, set()
        for r in reversed(ranks):
            if r:
                loops |= {w for w, runs in ((64, acc >= 64), (16, acc % 64 >= 16), (1, acc % 16 > 0)) if runs}
                acc += r
        assert loops == {64, 16, 1}, (ranks, loops)
        blocks = {(r - 1) // 64 + 1 for r in ranks if r}  # 64-row blocks of a level's triangular solve
        assert 1 in blocks and 2 in blocks
        assert any(r > 64 and r % 64 == 1 for r in ranks) and any(r % 64 == 0 for r in ranks if r)  # a partial block of one row, a full one


def test_ragged_case_reaches_both_ends_of_least_norm():
    case = C.build("ragged")
    nf, dims, n = case["fixed"]["nfixed"], case["dims"], case["n"]
    assert (dims == 0).any() and (nf == dims[:, 0] + 1).any() and (nf == n).any() and (nf == 0).any()
    b = int(np.flatnonzero(nf == n)[0])
    assert case["totalrank"][b] == n and not case["rank"][b].any()  # nVarRank = 0 and nVarFree = 0
    np.testing.assert_array_equal(np.sort(case["x"][b]), np.sort(case["fixed"]["fixed_val"][b]))
    assert (case["rank"][dims == 0] == 0).all()


def test_a_free_variables(case):
    """(a) at least half of the problems have free variables (ranks of the levels + nfixed < n), and solveLeastNorm_1 moves each of those by more than 1e-3 somewhere"""
    free = case["free"]
    if case["name"] != "ragged":  # (built for the nVarFree == 0 end)
        assert 2 * int(free.sum()) >= len(free)
    assert free.any() and (case["ln1_moves"][free] > 1e-3).all()


def test_least_norm_group_covers_the_orders_of_the_spd_solve():
    """from the oracle's ranks alone: every listed nVarFree occurs, and in EVERY problem of the group solveLeastNorm_2 and _3 each move some entry
    of x by more than 1e-3 (condition (a): a routine that does nothing cannot pass); fixed variables occur"""
    seen = set()
    for name in C.LEAST_NORM_CASES:
        ln = C.build_least_norm(name)
        print(C.summary_least_norm(ln))
        assert C.summary_least_norm(ln) in C.__doc__
        np.testing.assert_array_equal(ln["nvarfree"], ln["n"] - ln["fixed"]["nfixed"].astype(int) - ln["rank"].sum(axis=1).astype(int))
        assert (ln["nvarfree"] > 0).all() and (ln["fixed"]["nfixed"] > 0).any()
        for key in ("ln2", "ln3"):
            assert np.isfinite(ln[key]).all()
            assert (np.abs(ln[key] - ln["x"]).max(axis=1) > 1e-3).all(), (name, key)
        assert C._rel(np.abs(ln["ln2"] - ln["ln3"]).max(), ln["ln2"]) <= C.BOUND_X  # (of condition (c))
        seen |= set(ln["nvarfree"].tolist())
    assert set(C.LEAST_NORM_ORDERS) <= seen, seen
    assert C.LEAST_NORM_ORDERS == (1, 15, 16, 17, 48, 64, 65)


def test_b_multipliers_are_not_vacuous(case):
    """(b) non-zero multipliers at two objectives at least, found and not found, CORRECT_SIGN marks, a scan that stops at more than one level"""
    assert len(case["nonzero_objectives"]) >= 2
    assert (case["found"] == 1).any() and (case["found"] == 0).any()
    sens, _, _, marks, stopped = case["scan"]
    assert (marks == C.CORRECT).any() and any((m == C.CORRECT).any() for m in case["marks"])
    last = len(case["caps"]) - 1
    if case["name"] == "large":  # (one problem)
        assert sens[0, 0] == 1
    else:
        assert len(set(stopped.tolist())) > 1
        assert (stopped < last).any() and (stopped == last).any()  # some stop, some run to the end
    mask, _, _, _, verdict = case["collect"]
    assert mask[:, case["n"]:].any() and (verdict[:, 1] > 1).any()  # the collected sets are sets


def test_c_oracle_agrees_with_the_mathematics(case):
    """(c) stationarity, lambda_k = residual of level k (1e-12); get_v = A x - b, the three least-norm solutions, x against the null space (1e-10):
    each relative to max(1, largest magnitude of the quantity)"""
    a = case["authority"]
    assert a["stat"] <= C.BOUND_DUAL and a["lam_v"] <= C.BOUND_DUAL, a
    assert a["v"] <= C.BOUND_X and a["ln"] <= C.BOUND_X and a["orth"] <= C.BOUND_X, a
    for k in ("x", "v", "ln1", "ln2", "ln3", "mult"):
        assert np.isfinite(case[k]).all(), k


def test_a_smaller_batch_is_a_prefix_of_a_larger_one():
    """tiny runs at 4 CUs + 1 problems and again at 8: same problems, same oracle results"""
    big, small = C.build("tiny"), C.build("tiny", 8)
    for k in ("lod", "types", "x", "v", "mult", "ln1", "ln2", "ln3"):
        np.testing.assert_array_equal(small[k], big[k][:8], err_msg=k)
    for i in range(5):
        np.testing.assert_array_equal(small["scan"][i], big["scan"][i][:8])
