"""The kernels that run AFTER the factor lands in HBM (solve_generic, residual, sensitivity<64,staged|hbm>, the two sweeps, leastnorm 1 / 2 / 3)
against the oracle, bit for bit, on the cases of tests/postfactor_cases.py: shapes on both sides of every switch of their launchers, every
l-QR kernel as the producer of the factor they read.  What makes a case worth comparing (free variables, non-zero multipliers, candidates
found and not found, scans that stop at different levels, the oracle's own agreement with the mathematics) is asserted on the CPU by
tests/test_postfactor_cases.py.  Every case names the producer (last_kernel) and the consumer variants (last_consumer_kernel) it was built
to reach: a dispatch rule that moves makes the case fail instead of quietly testing something else."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime — the CU count below comes from torch)

import postfactor_cases as PC
from lexls_amd import capi
from test_gpu_parity import assert_factor_equal

pytestmark = pytest.mark.gpu

STAGED, HBM, PER_OBJECTIVE = "sensitivity<64,staged>", "sensitivity<64,hbm>", "multipliers<per-objective>"


def sweep(md, collect=False):
    return f"sensitivity_sweep<{md},collect>" if collect else f"sensitivity_sweep<{md}>"


def handle(hip, case, policy=None, regularized=False):
    s = hip.BatchedLexLSE(case["lod"].shape[0], case["n"], case["caps"])
    if policy is not None:
        s.set_kernel_policy(policy)
    if regularized:
        s.setRegularization(1, [0.0] * len(case["caps"]))  # the null-space basis solveLeastNorm_3 needs (lexlse.h:1217-1221), x as without
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"], f["fixed_idx"], f["fixed_val"], f["fixed_type"])
    s.setProblem(case["lod"])
    s.setCtrType(case["types"])
    return s


def reset_types(s, case):
    """the activation types as given: every oracle result starts from them, the handle keeps the marks of the call before"""
    s.setCtrType(case["types"])
    if case["fixed"]:
        capi.check(capi.lib().lexls_lse_set_fixed_type(s._h, case["fixed"]["fixed_type"].ctypes.data_as(C.POINTER(C.c_uint8))))


def check_consumers(hip, s, case, sens_kernel, collect_kernel, mult_kernel, ctx=""):
    """every post-factorization call on the factor `s` holds against the oracle's results in `case`; returns what the calls gave"""
    n, nobj = case["n"], len(case["caps"])
    m = case["dims"].sum(axis=1)
    solve_kernel = "solve_generic<64>" if n + 1 <= 64 else "solve_generic<256>"
    got = {}
    np.testing.assert_array_equal(s.get_x(), case["x"], err_msg=ctx + "x")
    v = s.get_v()
    assert s.last_consumer_kernel() == "residual<64>"
    for b in range(len(m)):
        np.testing.assert_array_equal(v[b, :m[b]], case["v"][b, :m[b]], err_msg=ctx + f"v of problem {b}")
    got["v"] = [v[b, :m[b]] for b in range(len(m))]
    for k in range(nobj):
        reset_types(s, case)
        found, ctr, obj, maxabs = s.ObjectiveSensitivity(k, PC.TOLW, PC.TOLC)
        assert s.last_consumer_kernel() == sens_kernel, ctx
        want = case["sens"][k]
        np.testing.assert_array_equal(found.astype(np.int32), want[:, 0], err_msg=ctx + f"found, level {k}")
        np.testing.assert_array_equal(np.where(found, ctr, 0), np.where(found, want[:, 1], 0), err_msg=ctx + f"ctr, level {k}")
        np.testing.assert_array_equal(np.where(found, obj, 0), np.where(found, want[:, 2], 0), err_msg=ctx + f"obj, level {k}")
        np.testing.assert_array_equal(maxabs, case["maxabs"][k], err_msg=ctx + f"maxabs, level {k}")
        np.testing.assert_array_equal(s.getWorkspace(), case["lam"][k], err_msg=ctx + f"multipliers, level {k}")
        np.testing.assert_array_equal(s.getCtrType(), case["marks"][k], err_msg=ctx + f"marks, level {k}")
    # the scan from level 0 against the oracle's level loop
    sens, maxabs_ref, lam, marks, _ = case["scan"]
    reset_types(s, case)
    s.setSensitivityScan(True)
    found, ctr, obj, maxabs = s.ObjectiveSensitivity(0, PC.TOLW, PC.TOLC)
    s.setSensitivityScan(False)
    assert s.last_consumer_kernel() == sens_kernel, ctx
    np.testing.assert_array_equal(np.stack([found.astype(np.int32), ctr, obj], 1), sens, err_msg=ctx + "scan: verdict")
    np.testing.assert_array_equal(maxabs, maxabs_ref, err_msg=ctx + "scan: maxabs")
    np.testing.assert_array_equal(s.getWorkspace(), lam, err_msg=ctx + "scan: multipliers")
    np.testing.assert_array_equal(s.getCtrType(), marks, err_msg=ctx + "scan: marks")
    got["scan"] = (found, ctr, obj, maxabs, s.getWorkspace(), s.getCtrType())
    # the collecting overload at one level, with its wrong-sign set
    reset_types(s, case)
    nonempty, entries, obj = s.sensitivity_collect(case["collect_level"], PC.TOLW, PC.TOLC)
    assert s.last_consumer_kernel() == collect_kernel, ctx
    have = (s.wrong_sign(), s.getCtrType(), s.getFixedType(), s.getWorkspace(), np.stack([nonempty.astype(np.int32), entries, obj], 1))
    for name, g, w in zip(("set", "constraint types", "fixed types", "multipliers", "verdict"), have, case["collect"]):
        if name == "fixed types" and not case["fixed"]:
            continue
        np.testing.assert_array_equal(g, w, err_msg=ctx + f"collect: {name}")
    got["collect"] = have
    reset_types(s, case)
    got["mult"] = s.multipliers()
    assert s.last_consumer_kernel() == mult_kernel, ctx
    np.testing.assert_array_equal(got["mult"], case["mult"], err_msg=ctx + "multipliers()")
    np.testing.assert_array_equal(s.getCtrType(), case["types"], err_msg=ctx + "multipliers() leaves the types alone")
    for opt, fn in ((1, s.solveLeastNorm_1), (2, s.solveLeastNorm_2)):
        fn()
        assert s.last_consumer_kernel() == f"leastnorm_{opt}<64>"
        got[f"ln{opt}"] = s.get_x()
        np.testing.assert_array_equal(got[f"ln{opt}"], case[f"ln{opt}"], err_msg=ctx + f"solveLeastNorm_{opt}")
        s.solve()  # d_x holds a least-norm solution: solve() has to run, and gives the basic solution back
        assert s.last_consumer_kernel() == solve_kernel, ctx
        np.testing.assert_array_equal(s.get_x(), case["x"], err_msg=ctx + f"solve() after solveLeastNorm_{opt}")
    return got


def check_least_norm_3(hip, case, policy=None):
    """solveLeastNorm_3 on a second handle: regularization type 1 with zero factors accumulates the null-space basis and changes nothing else"""
    s = handle(hip, case, policy, regularized=True)
    s.factorize()
    s.solveLeastNorm_3()
    assert s.last_consumer_kernel() == "leastnorm_3<64>"
    np.testing.assert_array_equal(s.get_x(), case["ln3"], err_msg="solveLeastNorm_3")
    s.solve()
    assert s.last_consumer_kernel() == ("solve_generic<64>" if case["n"] + 1 <= 64 else "solve_generic<256>")
    np.testing.assert_array_equal(s.get_x(), case["x"], err_msg="solve() after solveLeastNorm_3")
    s.close()


# case -> producer under its policy (automatic where the case names none), kernels of ObjectiveSensitivity, sensitivity_collect, multipliers()
SIZE_CASES = {
    "n63": ("lqr_quad<4,16,factor>", sweep(16), sweep(16, True), "multipliers_sweep<16>"),       # 72 rows: a left-looking kernel; n <= 64: swept
    "n64": ("lqr_generic<256,lds>", sweep(16), sweep(16, True), "multipliers_sweep<16>"),        # 65 columns: no wave kernel; n <= 64: swept
    "n65": ("lqr_generic<256,lds>", STAGED, STAGED, PER_OBJECTIVE),                              # n = 65: not swept
    "row17": ("lqr_generic<64,lds>", STAGED, STAGED, PER_OBJECTIVE),                             # a 17-row level: not swept
    "obj9": ("lqr_wave<41,12>", STAGED, STAGED, PER_OBJECTIVE),                                  # 9 objectives: not swept
    "blocks": ("lqr_large<multi-launch>", HBM, HBM, PER_OBJECTIVE),                              # 206 x 151 x 8 B staged > 160 KB
    "large": ("lqr_large<multi-launch>", HBM, HBM, PER_OBJECTIVE),                               # 231 x 101 x 8 B staged > 160 KB
    "staged": ("lqr_generic<256,lds>", STAGED, STAGED, PER_OBJECTIVE),                           # 64 KB < 101 x 89 x 8 B <= 160 KB: set_lds
    "ragged": ("lqr_wave<41,12,exact>", sweep(12), sweep(12, True), "multipliers_sweep<12>"),
}


@pytest.mark.parametrize("name", list(SIZE_CASES))
def test_consumers_beyond_the_small_shapes(hip, oracle, name):
    case = PC.build(name)
    producer, sens_kernel, collect_kernel, mult_kernel = SIZE_CASES[name]
    s = handle(hip, case, case["policy"])
    if name == "blocks":  # factorize() and solve() separately: the multi-launch path leaves x to solve_generic_kernel<256>
        s.factorize()
        assert s.last_consumer_kernel() == ""
        s.solve()
        assert s.last_consumer_kernel() == "solve_generic<256>"
    else:
        s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == producer
    assert_factor_equal(s, case["basic"], case["dims"], case["n"])
    check_consumers(hip, s, case, sens_kernel, collect_kernel, mult_kernel)
    s.close()
    check_least_norm_3(hip, case)


def test_hbm_resident_generic_factor_under_the_consumers(hip, oracle):
    """policy 1 on the n = 100 case: the generic kernel that never holds the problem in LDS as the producer"""
    case = PC.build("large")
    s = handle(hip, case, 1)
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == "lqr_generic<1024,hbm>"
    assert_factor_equal(s, case["basic"], case["dims"], case["n"])
    check_consumers(hip, s, case, HBM, HBM, PER_OBJECTIVE)
    s.close()


def test_unstaged_sensitivity_kernel_chosen_by_batch_size(hip, oracle):
    """n = 3 at 4 CUs + 1 problems: neither the sweep nor the staged kernel takes a batch beyond four problems per CU; the same data at batch 8
    go to the sweep, and the first 8 results of the big batch are those"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big, small = PC.build("tiny", 4 * cus + 1), PC.build("tiny", 8)
    got = {}
    for case, sens_kernel, collect_kernel in ((big, HBM, HBM), (small, sweep(12), sweep(12, True))):
        s = handle(hip, case)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == "lqr_quad<1,12,factor>"
        assert_factor_equal(s, case["basic"], case["dims"], case["n"])
        got[len(case["x"])] = check_consumers(hip, s, case, sens_kernel, collect_kernel, "multipliers_sweep<12>", ctx=f"batch {len(case['x'])}: ")
        s.close()
    for key in ("mult", "ln1", "ln2"):
        np.testing.assert_array_equal(got[8][key], got[4 * cus + 1][key][:8], err_msg=key)
    for key in ("scan", "collect"):
        for g8, gbig in zip(got[8][key], got[4 * cus + 1][key]):
            np.testing.assert_array_equal(g8, gbig[:8], err_msg=key)
    check_least_norm_3(hip, small)


# the producer matrix: policy -> kernel (wide: policy 3 finds no left-looking instantiation and takes policy 0's kernel)
PRODUCERS = {
    "ik": {0: "lqr_wave<41,12,exact>", 3: "lqr_lwave<41,12,exact>", 4: "lqr_quad<3,12,shift 7,factor>", 1: "lqr_generic<64,lds>"},
    "wide": {0: "lqr_wave<64,16>", 4: "lqr_quad<4,16,factor>", 1: "lqr_generic<64,lds>"},
}


@pytest.mark.parametrize("name", list(PRODUCERS))
def test_every_producer_feeds_every_consumer_the_same_bits(hip, oracle, name):
    """fac, hh, perm, rank and fcol of every l-QR kernel under the whole consumer list: the same outputs whoever wrote the factor — the padding
    behind a problem's rows and the ranks of levels nobody entered included, which assert_factor_equal does not look at"""
    case = PC.build(name)
    md = 12 if max(case["caps"]) <= 12 else 16
    first = None
    for policy, producer in PRODUCERS[name].items():
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        assert_factor_equal(s, case["basic"], case["dims"], case["n"])
        got = check_consumers(hip, s, case, sweep(md), sweep(md, True), f"multipliers_sweep<{md}>", ctx=f"{producer}: ")
        s.close()
        if first is None:
            first = got
        for key in ("mult", "ln1", "ln2"):
            np.testing.assert_array_equal(got[key], first[key], err_msg=f"{producer}: {key}")
        for key in ("v", "scan", "collect"):
            for g, f in zip(got[key], first[key]):
                np.testing.assert_array_equal(g, f, err_msg=f"{producer}: {key}")
    check_least_norm_3(hip, case)


@pytest.mark.parametrize("name", list(PC.LEAST_NORM_CASES))
def test_least_norm_orders_of_the_spd_solve(hip, oracle, name):
    """solveLeastNorm_2 and _3 with nVarFree = 1, on both sides of 16, at 48 and on both sides of 64 — the panel edges and the switch of spd_solve
    (tests/postfactor_cases.py: the least-norm group) —, bit for bit"""
    case = PC.build_least_norm(name)
    s = handle(hip, case)
    s.factorize_solve(keep_factor=True)
    np.testing.assert_array_equal(s.getRanks()[0], case["rank"])
    np.testing.assert_array_equal(s.get_x(), case["x"])
    s.solveLeastNorm_2()
    assert s.last_consumer_kernel() == "leastnorm_2<64>"
    np.testing.assert_array_equal(s.get_x(), case["ln2"], err_msg="solveLeastNorm_2")
    s.close()
    check_least_norm_3(hip, case)


def test_consumer_name_follows_the_factor(hip, oracle):
    """"" until a consumer launches on the current factor; a solve() the factorization kernel answered already launches nothing"""
    case = PC.build("ik")
    s = handle(hip, case)
    assert s.last_consumer_kernel() == ""
    s.factorize()
    s.solve()
    assert s.last_consumer_kernel() == ""
    np.testing.assert_array_equal(s.get_x(), case["x"])
    s.get_v()
    assert s.last_consumer_kernel() == "residual<64>"
    s.factorize_solve(keep_factor=True)
    assert s.last_consumer_kernel() == ""
    buf = C.create_string_buffer(8)
    s.get_v()
    capi.check(capi.lib().lexls_lse_last_consumer_kernel(s._h, buf, C.c_size_t(8)))
    assert buf.value == b"residua"  # cut to len - 1 characters, NUL-terminated
    assert capi.lib().lexls_lse_last_consumer_kernel(s._h, None, C.c_size_t(8)) == 1  # LEXLS_ERR_INVALID
    s.close()
