"""The regularization family (lexls_amd/csrc/lexls_regularize.h) against the oracle, bit for bit, on the cases of tests/reg_cases.py: both sides
of every placement of the wave kernels' work matrix and null-space basis, the panel edges of the one-wavefront Cholesky, the workgroup Cholesky
and the one-thread CG reductions of lqr_generic<256 | 1024>, both exits of the CG loop, both sides of the conditioning-dependent factor, type 7
with its by-products.  What makes a case stand where it is said to stand is asserted on the CPU by tests/test_reg_cases.py; here every run names
the kernel (last_kernel) and the placement (last_reg_placement) it was built to reach: a dispatch or placement rule that moves makes the case
fail instead of quietly testing something else."""
import ctypes as C

import numpy as np
import pytest

import reg_cases as RC
from factor_checks import assert_factor_equal
from lexls_amd import capi

pytestmark = pytest.mark.gpu


def handle(hip, case, reg_type, cap=10, policy=None, problems=slice(None)):
    """the case (or the problems `problems` of it) on a fresh handle, regularization and all"""
    lod, dims, fac = case["lod"][problems], case["dims"][problems], case["fac"][problems]
    s = hip.BatchedLexLSE(lod.shape[0], case["n"], case["caps"])
    if policy is not None:
        s.set_kernel_policy(policy)
    s.setRegularization(reg_type, fac, variable_factor=case["var_reg"], cg_iterations=cap)
    if (dims != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(dims)
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"][problems], f["fixed_idx"][problems], f["fixed_val"][problems])
    s.setProblem(lod)
    return s


def check(s, case, ref, reg_type, problems=slice(None), ctx=""):
    """x, ranks, first columns, permutations, Householder scalars, the kept factor (type 7: X_mu and residual_mu) are the oracle's bits"""
    ref = {k: v[problems] for k, v in ref.items()}
    np.testing.assert_array_equal(s.get_x(), ref["x"], err_msg=ctx + "x")
    assert_factor_equal(s, ref, case["dims"][problems], case["n"])
    if reg_type == 7:
        xm, _, rm = s.get_mu()
        np.testing.assert_array_equal(xm, ref["x_mu"], err_msg=ctx + "X_mu")
        np.testing.assert_array_equal(rm, ref["residual_mu"], err_msg=ctx + "residual_mu")
    return s.get_x(), s.get_lexqr()


PAIRS = [(nm, t) for nm, c in RC.CASES.items() for t in c["types"]]


@pytest.mark.parametrize("name,reg_type", PAIRS, ids=[f"{nm}-type{t}" for nm, t in PAIRS])
def test_regularized_case_is_the_oracle_s_bits(hip, oracle, name, reg_type):
    case = RC.build(name)
    kernel, window, basis = RC.PLAN[name][reg_type]
    B = case["lod"].shape[0]
    for cap in (case["cg_caps"] if reg_type in (2, 6) else (10,)):
        ref = case["ref"][(reg_type, cap)]
        ctx = f"{name}, type {reg_type}, cap {cap}: "
        s = handle(hip, case, reg_type, cap)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == kernel, ctx
        assert s.last_reg_placement() == (window, bool(basis)), ctx
        x, fac = check(s, case, ref, reg_type, ctx=ctx)
        s.close()
        if name in RC.WAVE_CASES:  # the same bits from the generic kernel, which keeps every piece in HBM
            g = handle(hip, case, reg_type, cap, policy=1)
            g.factorize_solve(keep_factor=True)
            assert g.last_kernel() == RC.POLICY_1, ctx
            assert g.last_reg_placement() == (0, False), ctx
            check(g, case, ref, reg_type, ctx=ctx + "policy 1: ")
            g.close()
        for b in range(B):  # a batch with per-problem factors gives the bits of batch-of-one runs
            one = handle(hip, case, reg_type, cap, problems=slice(b, b + 1))
            one.factorize_solve(keep_factor=True)
            x1, f1 = check(one, case, ref, reg_type, problems=slice(b, b + 1), ctx=ctx + f"problem {b} alone: ")
            m = int(case["dims"][b].sum())
            np.testing.assert_array_equal(x1[0], x[b])
            np.testing.assert_array_equal(f1[0][:, :m], fac[b][:, :m])
            one.close()


def test_placement_follows_the_last_factorization(hip, oracle):
    """(0, False) before any factorization, on the generic kernel and without regularization; the wave kernel's own placement in between"""
    case = RC.build("p41_22")
    s = handle(hip, case, 1)
    assert s.last_reg_placement() == (0, False)
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == RC.W41 and s.last_reg_placement() == (22, True)
    s.factorize()  # (factorize alone launches the same kernel)
    assert s.last_reg_placement() == (22, True)
    s.setRegularization(3, case["fac"])
    s.factorize_solve(keep_factor=True)
    assert s.last_reg_placement() == (12, True)
    np.testing.assert_array_equal(s.get_x(), case["ref"][(3, 10)]["x"])
    s.setRegularization(0)
    s.factorize_solve(keep_factor=True)
    assert not s.last_kernel().endswith("regularized>") and s.last_reg_placement() == (0, False)
    np.testing.assert_array_equal(s.get_x(), case["plain"]["x"])
    s.setRegularization(1, case["fac"])
    s.set_kernel_policy(1)
    s.factorize_solve(keep_factor=True)
    assert s.last_kernel() == RC.POLICY_1 and s.last_reg_placement() == (0, False)
    w = C.c_uint32(7)
    assert capi.lib().lexls_lse_last_reg_placement(s._h, C.byref(w), None) == 1  # LEXLS_ERR_INVALID
    assert capi.lib().lexls_lse_last_reg_placement(None, C.byref(w), C.byref(w)) == 1
    s.close()
