"""The conditions that make tests/test_gpu_lse_skip.py meaningful, asserted on the cases of tests/skip_cases.py from the oracle alone (no GPU)."""
import numpy as np
import pytest

import skip_cases as S

NAMES = list(S.CASES)
PIVOTS = ("rank", "fcol", "totalrank", "perm")


@pytest.mark.parametrize("name", NAMES)
def test_fresh_variant_tells_kept_bits_from_new_data(name):
    """every skipped problem's oracle result on the fresh lod2 differs from its result on lod1 in x and in the column permutation"""
    case = S.build(name)
    for b in case["skipped"]:
        assert (case["ref2_fresh"]["x"][b] != case["ref1"]["x"][b]).any(), b
        assert (case["ref2_fresh"]["perm"][b] != case["ref1"]["perm"][b]).any(), b


@pytest.mark.parametrize("name", NAMES)
def test_poison_variant(name):
    case = S.build(name)
    skip = case["skip"] != 0
    assert np.isnan(case["lod2"]["poison"][skip]).all()
    assert np.isfinite(case["lod2"]["poison"][~skip]).all() and np.isfinite(case["lod2"]["fresh"]).all()
    for k, v in case["expected"].items():
        assert np.isfinite(v).all(), k
    # the two variants differ in the skipped slots only, and the composite batch is lod1 there
    np.testing.assert_array_equal(case["lod2"]["poison"][~skip], case["lod2"]["fresh"][~skip])
    np.testing.assert_array_equal(case["composite"][skip], case["lod1"][skip])
    np.testing.assert_array_equal(case["composite"][~skip], case["lod2"]["fresh"][~skip])
    for k in PIVOTS + ("x",):
        np.testing.assert_array_equal(case["expected"][k][skip], case["ref1"][k][skip])


@pytest.mark.parametrize("name", NAMES)
def test_live_problems_change_between_the_runs(name):
    case = S.build(name)
    for b in case["live"]:
        assert (case["expected"]["x"][b] != case["ref1"]["x"][b]).any() and (case["expected"]["perm"][b] != case["ref1"]["perm"][b]).any(), b
        assert (case["ref3"]["x"][b] != case["expected"]["x"][b]).any(), b
    for b in case["deficient"]:  # the rank-deficient live members are what they are meant to be
        assert case["expected"]["rank"][b, 0] == max(1, case["caps"][0] - 3) and case["ref1"]["rank"][b, 0] == min(case["caps"][0], case["n"])


def test_mask_layout():
    """every group of four and every pair the layout is for is in the mask, at its place"""
    skip = S.build("qtol_ik")["skip"]
    assert len(skip) == S.BATCH == 19 and sorted(np.flatnonzero(skip)) == [0, 5, 6, 7, 8, 9, 10, 11, 14, 18]
    for what, (first, bits) in S.QUADS.items():
        assert first % 4 == 0 and tuple(skip[first:first + 4]) == bits, what
    for what, (first, bits) in S.PAIRS.items():
        assert first % 2 == 0 and tuple(skip[first:first + 2]) == bits, what
    assert len(skip) % 4 == 3  # the tail group leaves one quarter of the last wavefront idle
    for name in NAMES:
        case = S.build(name)
        if len(case["skip"]) == S.BATCH:
            np.testing.assert_array_equal(case["skip"], skip)
        else:
            assert case["skip"].tolist() == [0, 1, 0] and case["n"] == 100  # the large shape: the middle problem
        assert set(case["deficient"]) <= set(case["live"].tolist())


@pytest.mark.parametrize("name", [n for n in NAMES if S.CASES[n]["contract"] in ("T", "L")])
def test_tolerance_contract_cases_keep_stable_problems_only(name):
    case, c = S.build(name), S.CASES[name]
    for lod in (case["lod1"], case["composite"], case["lod2"]["fresh"], case["lod3"]):
        assert S._stable(c, lod, case["dims"], case["fixed"]).all()
    assert case["kept"] >= S.RETENTION * case["drawn"]
    assert case["redrawn_skipped"] == 0  # never a skipped one


def test_every_family_has_a_case():
    kernels = {c["kernel"] for c in S.CASES.values()}
    for family in ("lqr_qtol<", "lqr_mfma<", "lqr_quad<", "lqr_lwave<", "lqr_wave<", "lqr_generic<", "lqr_large<multi-launch>", "lqr_large<step-per-pivot,mfma>"):
        assert any(k.startswith(family) for k in kernels), family
    assert {S.CASES[n]["policy"] for n in NAMES if S.CASES[n]["kernel"].startswith("lqr_mfma")} == {7, 8, 9}
    for name in S.CONSUMER_CASES:
        assert S.CASES[name]["keep"] and S.CASES[name]["contract"] == "B" and "nfixed" not in S.CASES[name]
    for c in S.CASES.values():  # the size limit of a parametrized GPU test
        assert (c.get("batch", S.BATCH) <= 19 and c["n"] <= 47) or (c["batch"] == 3 and c["n"] == 100)


def test_guard_case_is_what_it_says():
    """from the calibration script's estimate (oracle only): which problems the guard flags in run 1, on the fresh lod2 and on the composite batch"""
    g = S.guard_case()
    flag1, flag2, flag_e = g["est1"] >= S.GUARD_THRESHOLD, g["est2"] >= S.GUARD_THRESHOLD, g["est_expected"] >= S.GUARD_THRESHOLD
    assert np.flatnonzero(flag1).tolist() == [S.GUARD_FLAGGED_RUN1]
    assert sorted(np.flatnonzero(flag2).tolist()) == sorted([S.GUARD_WOULD_FLAG, *S.GUARD_LIVE_FLAGGED])
    assert sorted(np.flatnonzero(flag_e).tolist()) == sorted([S.GUARD_FLAGGED_RUN1, *S.GUARD_LIVE_FLAGGED])
    assert g["skip"][S.GUARD_FLAGGED_RUN1] and g["skip"][S.GUARD_WOULD_FLAG] and not g["skip"][list(S.GUARD_LIVE_FLAGGED)].any()
    # estimates well away from the threshold on both sides: the kernel's rounding of an estimate cannot move a flag
    for est in (g["est1"], g["est2"]):
        assert not ((est > S.GUARD_THRESHOLD / 2) & (est < S.GUARD_THRESHOLD * 2)).any()
