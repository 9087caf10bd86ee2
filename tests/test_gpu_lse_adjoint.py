"""The adjoint of the LexLSE solve on the device (lexls_lse_solve_adjoint*, solve_adjoint_kernel) against the references of
tests/adjoint_cases.py, within AC.TOL (derived there from the references' own disagreement on the CPU, never from the device's figures):
reference (A), M^T g and N^T g from unit solves on the oracle; for the two large cases reference (B) plus the dot-product identities.
Every producer of a kept factor the shape allows is named (last_kernel), so a dispatch rule that moves makes the case fail instead of
quietly testing something else."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
from lexls_amd import capi
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
CONSUMER = "solve_adjoint<64>"
PRODUCERS = AC.PRODUCERS  # case -> kernel policy -> the producer of the kept factor, as the host-side dispatch plan names it


def handle(hip, case, policy=None):
    s = hip.BatchedLexLSE(case["lod"].shape[0], case["n"], case["caps"])
    if policy is not None:
        s.set_kernel_policy(policy)
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"], f["fixed_idx"], f["fixed_val"])
    s.setProblem(case["lod"])
    return s


def gap(got, ref):
    """largest error per problem, relative to max(1, largest magnitude of the problem's reference)"""
    return max(float(np.abs(got[b] - ref[b]).max()) / max(1.0, float(np.abs(ref[b]).max())) for b in range(len(ref)))


def device_form(s, g, with_fixed=True):
    B, n, cap = g.shape[0], s.nVar, s.cap
    d_g = torch.from_numpy(np.array(g, np.float64)).cuda()
    d_rhs = torch.full((B, cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda") if with_fixed else None
    s.solve_adjoint_device(d_g, d_rhs, d_fixed)
    s.synchronize()
    return d_rhs.cpu().numpy(), d_fixed.cpu().numpy() if with_fixed else None


@pytest.mark.parametrize("name", list(PRODUCERS))
def test_device_adjoint_within_tol_of_the_reference(hip, oracle, name):
    case = AC.build(name)
    ref_rhs, ref_fixed = AC.expected(case)
    m = case["dims"].sum(axis=1)
    first = None
    for policy, producer in PRODUCERS[name].items():
        ctx = f"{name} on {producer}: "
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.get_v())
        grad_rhs, grad_fixed = s.solve_adjoint(case["g"])
        assert s.last_consumer_kernel() == CONSUMER
        e_rhs, e_fixed = gap(grad_rhs, ref_rhs), gap(grad_fixed, ref_fixed)
        ids = [AC.identity_gap(pair, case["g"], grad_rhs) for pair in case["pairs"]]
        print(f"{ctx}grad_rhs {e_rhs:.2e} grad_fixed {e_fixed:.2e} identities {['%.1e' % i for i in ids]} (TOL {AC.TOL:.1e})")
        assert e_rhs <= AC.TOL and e_fixed <= AC.TOL, ctx + f"{e_rhs:.3e} {e_fixed:.3e}"
        if case["large"]:
            assert len(ids) == 3 and max(ids) <= AC.TOL, ctx + str(ids)
        nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(len(m), np.uint32)
        for b in range(len(m)):  # rows behind a problem's own, slots behind its fixed variables: exactly 0
            assert not grad_rhs[b, m[b]:].any() and not grad_fixed[b, nf[b]:].any(), ctx + f"problem {b}"
        # the same bits from a second run, from the device form (with and without grad_fixed), and whoever wrote the (bit-identical) factor
        again = s.solve_adjoint(case["g"])
        np.testing.assert_array_equal(again[0], grad_rhs, err_msg=ctx + "second run")
        np.testing.assert_array_equal(again[1], grad_fixed, err_msg=ctx + "second run")
        d_rhs, d_fixed = device_form(s, case["g"])
        assert s.last_consumer_kernel() == CONSUMER
        np.testing.assert_array_equal(d_rhs, grad_rhs, err_msg=ctx + "device form")
        np.testing.assert_array_equal(d_fixed, grad_fixed, err_msg=ctx + "device form")
        np.testing.assert_array_equal(device_form(s, case["g"], with_fixed=False)[0], grad_rhs, err_msg=ctx + "device form without grad_fixed")
        if first is None:
            first = (grad_rhs, grad_fixed)
        np.testing.assert_array_equal(grad_rhs, first[0], err_msg=ctx + "against the first producer")
        np.testing.assert_array_equal(grad_fixed, first[1], err_msg=ctx + "against the first producer")
        # x, the factor and get_v are what they were
        after = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.get_v())
        for a, b_, what in zip(after, before, ("x", "factor", "hh", "v")):
            np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
        s.close()


def sentinels(s):
    return np.full((s.batch, s.cap), 7.0), np.full((s.batch, s.nVar), 7.0)


def get_adjoint_rc(s, rhs, fixed):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    return capi.lib().lexls_lse_get_adjoint(s._h, p(rhs), p(fixed))


def solve_adjoint_rc(s, g):
    return capi.lib().lexls_lse_solve_adjoint(s._h, None if g is None else g.ctypes.data_as(C.POINTER(C.c_double)))


def device_rc(s, g):
    """(return code of the device form on sentinel-filled outputs, whether the outputs still hold the sentinels)"""
    d_g = None if g is None else torch.from_numpy(np.array(g, np.float64)).cuda()
    d_rhs = torch.full((s.batch, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((s.batch, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    rc = capi.lib().lexls_lse_solve_adjoint_device(s._h, None if d_g is None else C.c_void_p(d_g.data_ptr()), C.c_void_p(d_rhs.data_ptr()), C.c_void_p(d_fixed.data_ptr()))
    s.synchronize()
    return rc, bool((d_rhs == 7.0).all() and (d_fixed == 7.0).all())


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    case = AC.build("ik")
    g = np.ascontiguousarray(case["g"])
    s = handle(hip, case)
    rhs, fixed = sentinels(s)

    def refused(code):
        assert solve_adjoint_rc(s, g) == code
        assert device_rc(s, g) == (code, True)
        assert get_adjoint_rc(s, rhs, fixed) == INVALID  # (never UNSUPPORTED: there is nothing to return)
        assert (rhs == 7.0).all() and (fixed == 7.0).all()

    refused(INVALID)                                   # no factorization yet
    assert solve_adjoint_rc(s, g) == INVALID and b"kept" in capi.lib().lexls_last_error()
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    assert solve_adjoint_rc(s, None) == INVALID         # null g, with a factor in place
    assert device_rc(s, None) == (INVALID, True)
    assert capi.lib().lexls_lse_solve_adjoint_device(s._h, C.c_void_p(8), None, None) == INVALID  # null d_grad_rhs (refused before d_g is read)
    assert get_adjoint_rc(s, rhs, fixed) == INVALID     # nothing computed yet
    assert (rhs == 7.0).all() and (fixed == 7.0).all()

    want = s.solve_adjoint(g)
    assert get_adjoint_rc(s, rhs, None) == 0 and get_adjoint_rc(s, None, fixed) == 0  # either output may be NULL
    np.testing.assert_array_equal(rhs, want[0])
    np.testing.assert_array_equal(fixed, want[1])
    rhs, fixed = sentinels(s)
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert get_adjoint_rc(s, rhs, fixed) == INVALID
    assert solve_adjoint_rc(s, g) == 0 and get_adjoint_rc(s, rhs, fixed) == 0
    np.testing.assert_array_equal(rhs, want[0])
    rhs, fixed = sentinels(s)
    s.setProblem(case["lod"])                          # a call that invalidates the factor
    refused(INVALID)

    s.setRegularization(1, [1e-3] * len(case["caps"]))  # a regularized factorization: the damping rewrites the right-hand side
    s.factorize_solve(keep_factor=True)
    assert solve_adjoint_rc(s, g) == UNSUPPORTED
    assert b"regularization_type" in capi.lib().lexls_last_error()
    assert device_rc(s, g) == (UNSUPPORTED, True)
    assert get_adjoint_rc(s, rhs, fixed) == INVALID
    assert (rhs == 7.0).all() and (fixed == 7.0).all()
    s.close()


def torch_problem(hip, n=4, dims=(2, 2, 2), batch=2, seed=20290201):
    lod = torch.from_numpy(P.lse_batch(seed, batch, n, list(dims))).cuda()
    return hip.BatchedLexLSE(batch, n, list(dims)), lod


def test_solve_rhs_gradcheck(hip, oracle):
    """n = 4, dims (2, 2, 2), batch 2.  The map is affine, so central differences are exact up to the rounding of x over the step: with
    eps = 1e-6 and errors of x around 1e-15 (2 x 4 triangles of iid data) that is some 1e-9, against atol = rtol = 1e-6"""
    from lexls_amd.torch_adjoint import SolveRhs
    s, lod = torch_problem(hip)
    n = s.nVar
    rhs = lod[:, n, :].clone().requires_grad_(True)
    x = SolveRhs.apply(rhs, s, lod)
    ref = oracle.lse_run(lod.cpu().numpy(), [2, 2, 2], n)
    assert float(np.abs(x.detach().cpu().numpy() - ref["x"]).max()) <= 1e-10
    assert x.requires_grad and x.data_ptr() != s.device_ptr("x")  # a new tensor, not the handle's array
    assert torch.autograd.gradcheck(lambda r: SolveRhs.apply(r, s, lod), (rhs,), eps=1e-6, atol=1e-6, rtol=1e-6)
    (x * x).sum().backward()
    want = s.solve_adjoint(2.0 * x.detach().cpu().numpy())[0]
    np.testing.assert_array_equal(rhs.grad.cpu().numpy(), want)  # the host form on the same factor: the same bits
    s.close()


def test_solve_rhs_refuses_a_matrix_that_requires_grad(hip):
    from lexls_amd.torch_adjoint import SolveRhs
    s, lod = torch_problem(hip)
    rhs = lod[:, s.nVar, :].clone().requires_grad_(True)
    lod.requires_grad_(True)
    with pytest.raises(ValueError, match="no derivatives with respect to A"):
        SolveRhs.apply(rhs, s, lod)
    s.close()
