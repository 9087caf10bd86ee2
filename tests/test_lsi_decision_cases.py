"""The conditions that make tests/test_gpu_lsi_decisions.py meaningful, asserted on the batches of tests/lsi_decision_cases.py from the
oracle-backed driver alone (no GPU): the twins do tie, in both list orders and inside one lane; every parameter set changes decisions; the scaled
batches end as the module says, the long runs included; the new row kinds are accepted and the row nothing can satisfy ends active and violated.
They are conditions, not measurements: the module's table holds the figures, and its seed rule names the batches for which they hold."""
import numpy as np
import pytest

import lsi_decision_cases as D
from lexls_amd import problems as P
from oracle import oracle_ctypes as oracle

HALF, QUARTER = D.BATCH // 2, D.BATCH // 4


def test_the_case_table():
    assert D.BATCH == 8 and D.MAX_FACTORIZATIONS == 200 and D.LOG_CAPACITY > D.MAX_FACTORIZATIONS
    assert {k: (s["n"], s["dims"], s["simple_bounds"]) for k, s in D.SHAPES.items()} == {
        "general": (12, [4, 5, 4, 6], False), "ik": (40, [12] * 5, True), "wide": (57, [12, 16, 16, 16, 16], True), "cols46": (45, [12] * 5, True),
        "tall": (8, [4, 72, 4], False)}
    assert sum(D.SHAPES["wide"]["dims"]) == 76
    assert D.FAMILIES == ["twins", "tol_wrong_sign_1e-1", "tol_correct_sign_1e-1", "tol_linear_dependence_1e-1", "tol_feasibility_1e-1", "decades", "pow2_up",
                          "pow2_down", "kinds"]
    assert list(D.DROPPED_SETS) == ["tol_wrong_sign_0"] and not D.DROPPED_KINDS
    for shape, s in D.SHAPES.items():
        want = ["same", "cross", "reversed", "mirror"] + (["unit"] if s["simple_bounds"] else []) + (["lane_a", "lane_b"] if shape == "tall" else [])
        assert D.kinds_of(shape) == want
        rows = [r for pair in D.pairs_of(shape).values() for r in pair]
        assert len(set(rows)) == len(rows), shape  # no row in two pairs
        assert all(k < len(s["dims"]) - 1 and r < s["dims"][k] for k, r in rows), shape  # the last level is left alone
    first = D.SHAPES["tall"]["dims"][0]
    for kind in D.SAME_LANE:  # the same lane of a 64-wide scan over all rows of the instance
        (ka, ra), (kb, rb) = D.pairs_of("tall")[kind]
        assert ka == kb == 1 and abs(ra - rb) == 64 and (first + ra) % 64 == (first + rb) % 64


@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_generators_change_what_they_say(shape):
    s = D.SHAPES[shape]
    seed = D.start_of("twins", shape)
    plain = D.base_problem(shape, seed)
    t = D.generate("twins", shape, seed)
    for kind, ((ko, ro), (kc, rc)) in D.pairs_of(shape).items():
        if kind == "unit":
            e = np.zeros(s["n"])
            e[int(t[0]["var"][ro])] = 1.0
            np.testing.assert_array_equal(t[kc]["A"][rc], e)
            assert (t[kc]["lb"][rc], t[kc]["ub"][rc]) == (t[0]["lb"][ro], t[0]["ub"][ro]) == (-D.UNIT_BOUND, D.UNIT_BOUND)
        elif kind == "mirror":
            np.testing.assert_array_equal(t[kc]["A"][rc], -t[ko]["A"][ro])
            assert (t[kc]["lb"][rc], t[kc]["ub"][rc]) == (-t[ko]["ub"][ro], -t[ko]["lb"][ro])
        else:
            np.testing.assert_array_equal(t[kc]["A"][rc], t[ko]["A"][ro])
            assert (t[kc]["lb"][rc], t[kc]["ub"][rc]) == (t[ko]["lb"][ro], t[ko]["ub"][ro])
            np.testing.assert_array_equal(t[ko]["A"][ro], plain[ko]["A"][ro])  # the source is P.lsi_problem's row
    np.testing.assert_array_equal(t[-1]["A"], plain[-1]["A"])
    for family in D.TOLERANCES:
        for a, b in zip(D.generate(family, shape, seed), plain):
            assert all(np.array_equal(a[k], b[k]) for k in b)
    for family, k in (("pow2_up", 20), ("pow2_down", -20)):
        for a, b in zip(D.generate(family, shape, seed), plain):
            for key in b:
                np.testing.assert_array_equal(a[key], b[key] if "var" in b else np.ldexp(b[key], k))
    d = D.generate("decades", shape, seed)
    col, row = D.decade_scales(seed, s["n"], sum(s["dims"]))
    assert 1e-2 <= min(col.min(), row.min()) and max(col.max(), row.max()) <= 1e2 and col.max() / col.min() > 1e2
    if s["simple_bounds"]:
        np.testing.assert_array_equal(d[0]["ub"], 1.0 / col[plain[0]["var"]])
    np.testing.assert_array_equal(d[-1]["lb"], d[-1]["ub"])
    np.testing.assert_allclose(d[1]["A"][0, 3], plain[1]["A"][0, 3] * col[3] * row[s["dims"][0]], rtol=1e-15)
    kd = D.generate("kinds", shape, seed)
    for k in D.general_levels(shape):
        o = kd[k]
        assert o["lb"][0] == o["ub"][0] == plain[k]["lb"][0] and o["ub"][1] == 1e10 and o["lb"][2] == -1e10 and o["lb"][1] == plain[k]["lb"][1]
        assert not o["A"][3].any() and o["lb"][3] < 0.0 < o["ub"][3]
        if s["dims"][k] >= 5:
            assert not o["A"][4].any() and 0.0 < o["lb"][4] < o["ub"][4]
    assert (shape, len(D.unsatisfiable_rows(shape))) in {("general", 1), ("ik", 3), ("wide", 3), ("cols46", 3), ("tall", 1)}
    np.testing.assert_array_equal(kd[-1]["A"], plain[-1]["A"])


@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_twins_tie_on_the_oracle(shape):
    """status 0 everywhere; every pair kind has a virgin tie in at least half of the instances; the reversed kind shows both outcomes over the batch;
    the same-lane kinds tie in at least 4 of 8 tall instances"""
    assert D.statuses("twins", shape) == [0] * D.BATCH
    t = D.tie_counts(shape)
    print(shape, t)
    for kind, c in t.items():
        assert c["instances"] >= HALF, (kind, c)
    assert t["reversed"]["low"] > 0 and t["reversed"]["high"] > 0, t["reversed"]
    if shape == "tall":
        for kind in D.SAME_LANE:
            assert t[kind]["instances"] >= 4, (kind, t[kind])
        assert sum(t[k]["low"] for k in D.SAME_LANE) > 0 and sum(t[k]["high"] for k in D.SAME_LANE) > 0  # inside the lane, too, the list's order and the index order differ
    assert max(len(o["log"]) for o in D.refs("twins", shape)) <= D.LOG_CAPACITY
    for mode in ("first_wrong_sign", "warm"):  # the further paths of the GPU file: compared whatever they do; that they tie is measured, not required
        print(shape, mode, D.statuses("twins", shape, mode), {k: c["instances"] for k, c in D.tie_counts(shape, mode).items()})
    cold, warm = D.refs("twins", shape), D.refs("twins", shape, "warm")
    assert any(w["info"] != c["info"] for w, c in zip(warm, cold)), "the warm start changes no run"


def test_the_replay_counts_what_it_says():
    pairs = {"p": ((1, 0), (1, 3))}
    add = lambda k, r, t=1: dict(obj_index=k, ctr_index=r, ctr_type=t, alpha_or_lambda=0.5)
    r = D.replay([add(1, 3), add(1, 0)], pairs)["p"]
    assert (r["virgin"], r["later"], r["first"]) == (1, 0, "high")  # the second ADD finds its partner active: no tie
    r = D.replay([add(1, 0), add(1, 0, 0), add(1, 3)], pairs)["p"]
    assert (r["virgin"], r["later"], r["first"]) == (1, 1, "low")  # row 3 joins while row 0 is inactive again, but row 0 has a past
    r = D.replay([add(0, 0), add(1, 1, 2)], pairs)["p"]
    assert (r["virgin"], r["later"], r["first"]) == (0, 0, None)


@pytest.mark.parametrize("family", list(D.TOLERANCES))
def test_every_parameter_set_changes_decisions(family):
    """log or final working set differ from the default run in at least 2 of 8 instances of at least one shape; exactly one parameter is off its default"""
    assert len(D.params_of(family)) == 1
    (key, value), = D.params_of(family).items()
    from lexls_amd.lexlsi import PARAM_DEFAULTS, PARAM_KEYS
    assert value != PARAM_DEFAULTS[PARAM_KEYS.index(key)]
    counts = {shape: len(D.changed(family, shape)) for shape in D.SHAPES}
    print(family, counts)
    assert max(counts.values()) >= 2, counts


def test_the_dropped_parameter_set_changes_nothing():
    for family in D.DROPPED_SETS:
        assert not any(D.changed(family, shape) for shape in D.SHAPES), family


@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_scaled_batches_end_as_the_module_says(shape):
    for family in D.SCALED:
        st = D.statuses(family, shape)  # (an input error would have raised)
        print(family, shape, st, [len(o["log"]) for o in D.refs(family, shape)])
        assert set(st) <= {0, D.AT_THE_LIMIT}, (family, st)
        if family == "pow2_down":
            assert st.count(D.AT_THE_LIMIT) >= QUARTER, (family, st)
            assert max(o["info"]["factorizations"] for o in D.refs(family, shape)) == D.MAX_FACTORIZATIONS
        else:
            assert st.count(0) >= HALF, (family, st)
        assert max(len(o["log"]) for o in D.refs(family, shape)) <= D.LOG_CAPACITY


@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_row_kinds_on_the_oracle(shape):
    rs = D.refs("kinds", shape)
    solved = [o for o in rs if o["info"]["status"] == 0]
    assert len(solved) >= HALF
    for o in solved:
        for k, r in D.unsatisfiable_rows(shape):
            assert o["active"][k][r] != 0 and o["v"][k][r] != 0.0, (k, r)
        for k in D.general_levels(shape):
            assert o["active"][k][0] == 3  # the equality row inside a middle level is active as an equality
    assert D.kinds_hold(shape)


@pytest.mark.parametrize("family", D.FAMILIES)
def test_the_plain_run_is_the_debug_run(family):
    """the GPU file takes results and logs from oracle.lsi_run_debug; oracle.lsi_run, the entry the issue names, gives the same bits"""
    for shape, s in D.SHAPES.items():
        for p, o in zip(D.problems(family, shape), D.refs(family, shape)):
            r = oracle.lsi_run(s["n"], p, **D.params_of(family))
            assert r["info"] == o["info"]
            for key in ("active", "v"):
                np.testing.assert_array_equal(np.concatenate(r[key]), np.concatenate(o[key]))
            np.testing.assert_array_equal(r["x"], o["x"])


def test_the_seed_rule_is_followed():
    """every (family, shape) starts at the first member of its series for which its condition holds"""
    for family in D.FAMILIES:
        for shape in D.SHAPES:
            base = D.BASE + 1000 * list(D.SHAPES).index(shape)
            j = D.STARTS.get((family, shape), 0)
            assert D.start_of(family, shape) == base + 100 * j
            assert D.holds(family, shape), (family, shape)
            assert not any(D.holds(family, shape, base + 100 * i) for i in range(j)), (family, shape)
    assert P.lsi_problem(D.BASE, 12, [4, 5, 4, 6], simple_bounds=False)[0]["A"].shape == (4, 12)
