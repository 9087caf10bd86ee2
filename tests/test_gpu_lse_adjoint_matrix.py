"""The gradient of the LexLSE solve with respect to the matrix on the device (lexls_lse_solve_adjoint_matrix*, apply_solve_map_kernel,
adjoint_matrix_kernel) against reference (A) of tests/adjoint_matrix_cases.py — the dense KKT solve on the original data — within AM.TOL
(derived there from the two references' own disagreement on the CPU, never from the device's figures).  Every producer of a kept factor the
shape allows is named (last_kernel), so a dispatch rule that moves makes the case fail instead of quietly testing something else."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_matrix_cases as AM
from lexls_amd import capi
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
CONSUMER = "solve_adjoint_matrix<64>"
_dp, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


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


def device_form(s, g, with_flags=True):
    d_g = torch.from_numpy(np.array(g, np.float64)).cuda()
    d_G = torch.full((s.batch, s.nVar + 1, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((s.batch,), 7, dtype=torch.uint8, device="cuda") if with_flags else None
    s.solve_adjoint_matrix_device(d_g, d_G, d_f)
    s.synchronize()
    return d_G.cpu().numpy(), d_f.cpu().numpy() if with_flags else None


def observable_state(s):
    """what lexls_lse_get_multipliers, get_v and get_lambda answer: (return code, bytes) each, into sentinel-filled buffers"""
    out = []
    for fn, shape in ((capi.lib().lexls_lse_get_multipliers, (s.batch, s.nObj, s.nVar + s.cap)), (capi.lib().lexls_lse_get_v, (s.batch, s.cap)),
                      (capi.lib().lexls_lse_get_lambda, (s.batch, s.nVar + s.cap))):
        buf = np.full(shape, 7.0)
        out.append((fn(s._h, buf.ctypes.data_as(_dp)), buf.tobytes()))
    return out


@pytest.mark.parametrize("name", AM.CASES)
def test_device_gradient_within_tol_of_the_kkt_reference(hip, oracle, name):
    case = AM.build(name)
    ref, flags = case["A"], np.asarray(AM.FLAGS[name], np.uint8)
    np.testing.assert_array_equal(case["flags"], flags)  # the rule on the oracle's ranks gives the literals
    m = case["dims"].sum(axis=1)
    for policy, producer in AM.PRODUCERS[name].items():
        ctx = f"{name} on {producer}: "
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        if name in ("ik", "fixed"):  # something to keep: the multipliers, the residuals and a removal search of this factor
            s.multipliers()
            s.get_v()
            assert capi.lib().lexls_lse_sensitivity(s._h, None, C.c_int32(0), C.c_double(1e-8), C.c_double(1e-12)) == 0
        before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.getCtrType(), s.getFixedType())
        state = observable_state(s)
        G, diff = s.solve_adjoint_matrix(case["g"])
        assert s.last_consumer_kernel() == CONSUMER
        np.testing.assert_array_equal(diff, flags, err_msg=ctx + "flags")
        e = gap(G, ref)
        grad_rhs = s.solve_adjoint(case["g"])[0]
        e_rhs = max(float(np.abs(G[b, case["n"]] - grad_rhs[b]).max()) / max(1.0, float(np.abs(grad_rhs[b]).max())) for b in range(len(m)) if flags[b])\
            if flags.any() else 0.0
        print(f"{ctx}G {e:.2e}  column n against solve_adjoint {e_rhs:.2e} (TOL {AM.TOL:.1e})")
        assert e <= AM.TOL and e_rhs <= AM.TOL, ctx + f"{e:.3e} {e_rhs:.3e}"
        for b in range(len(m)):  # problems without a derivative and rows behind a problem's own: exactly 0
            assert not G[b, :, m[b]:].any(), ctx + f"problem {b}: rows behind its own"
            assert flags[b] or not G[b].any(), ctx + f"problem {b}: flagged 0, gradient not zero"
        # the same bits from a second run and from the device form, with and without the flags
        again = s.solve_adjoint_matrix(case["g"])
        np.testing.assert_array_equal(again[0], G, err_msg=ctx + "second run")
        np.testing.assert_array_equal(again[1], diff, err_msg=ctx + "second run")
        d_G, d_f = device_form(s, case["g"])
        assert s.last_consumer_kernel() == CONSUMER
        np.testing.assert_array_equal(d_G, G, err_msg=ctx + "device form")
        np.testing.assert_array_equal(d_f, diff, err_msg=ctx + "device form")
        np.testing.assert_array_equal(device_form(s, case["g"], with_flags=False)[0], G, err_msg=ctx + "device form without flags")
        # x, the factor, the activation types and what the other getters answer are what they were
        after = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.getCtrType(), s.getFixedType())
        for a, b_, what in zip(after, before, ("x", "factor", "hh", "ctr_type", "fixed_type")):
            np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
        assert observable_state(s) == state, ctx + "get_multipliers / get_v / get_lambda answer differently"
        s.close()


@pytest.mark.parametrize("name", ["base", "fixed", "wide"])
def test_apply_solve_map_reproduces_the_unit_solves(hip, oracle, name):
    case = AM.build(name)
    cols = AM.unit_solve_columns(case)  # (batch, n, cap)
    B, n, cap = cols.shape
    for policy, producer in AM.PRODUCERS[name].items():
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        d_rhs = torch.eye(cap, dtype=torch.float64, device="cuda")[:, None, :].expand(cap, B, cap).contiguous()
        d_out = torch.full((cap, B, n), 7.0, dtype=torch.float64, device="cuda")
        for i in range(cap):
            assert capi.lib().lexls_internal_apply_solve_map(s._h, C.c_void_p(d_rhs[i].data_ptr()), C.c_void_p(d_out[i].data_ptr())) == 0
        s.synchronize()
        got = d_out.cpu().numpy().transpose(1, 2, 0)
        e = gap(got, cols)
        print(f"{name} on {producer}: M by apply_solve_map against the oracle's unit solves {e:.2e} (TOL {AM.TOL:.1e})")
        assert e <= AM.TOL
        s.close()


def rc_host(s, g):
    return capi.lib().lexls_lse_solve_adjoint_matrix(s._h, None if g is None else g.ctypes.data_as(_dp))


def rc_get(s, G, f):
    return capi.lib().lexls_lse_get_adjoint_matrix(s._h, None if G is None else G.ctypes.data_as(_dp), None if f is None else f.ctypes.data_as(_u8p))


def rc_device(s, g):
    """(return code of the device form on sentinel-filled outputs, whether the outputs still hold the sentinels)"""
    d_g = None if g is None else torch.from_numpy(np.array(g, np.float64)).cuda()
    d_G = torch.full((s.batch, s.nVar + 1, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((s.batch,), 7, dtype=torch.uint8, device="cuda")
    rc = capi.lib().lexls_lse_solve_adjoint_matrix_device(s._h, None if d_g is None else C.c_void_p(d_g.data_ptr()), C.c_void_p(d_G.data_ptr()), C.c_void_p(d_f.data_ptr()))
    s.synchronize()
    return rc, bool((d_G == 7.0).all() and (d_f == 7).all())


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    case = AM.build("ik")
    g = np.ascontiguousarray(case["g"])
    s = handle(hip, case)
    sentinels = lambda: (np.full((s.batch, s.nVar + 1, s.cap), 7.0), np.full(s.batch, 7, np.uint8))  # noqa: E731
    G, f = sentinels()

    def refused(code):
        assert rc_host(s, g) == code
        assert rc_device(s, g) == (code, True)
        assert rc_get(s, G, f) == INVALID  # (never UNSUPPORTED: there is nothing to return)
        assert (G == 7.0).all() and (f == 7).all()

    refused(INVALID)                                   # no factorization yet
    assert rc_host(s, g) == INVALID and b"kept" in capi.lib().lexls_last_error()
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    assert rc_host(s, None) == INVALID                 # null g, with a factor in place
    assert rc_device(s, None) == (INVALID, True)
    assert capi.lib().lexls_lse_solve_adjoint_matrix_device(s._h, C.c_void_p(8), None, None) == INVALID  # null d_grad_lod (refused before d_g is read)
    assert rc_get(s, G, f) == INVALID                  # nothing computed yet
    s.solveLeastNorm_1()                               # x is no longer the basic solution of the factor
    refused(INVALID)
    assert rc_host(s, g) == INVALID and b"no x belongs" in capi.lib().lexls_last_error()
    s.solve()

    want = s.solve_adjoint_matrix(g)
    assert rc_get(s, G, None) == 0 and rc_get(s, None, f) == 0  # either output may be NULL
    np.testing.assert_array_equal(G, want[0])
    np.testing.assert_array_equal(f, want[1])
    G, f = sentinels()
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert rc_get(s, G, f) == INVALID
    assert rc_host(s, g) == 0 and rc_get(s, G, f) == 0
    np.testing.assert_array_equal(G, want[0])
    G, f = sentinels()
    s.setProblem(case["lod"])                          # a call that invalidates the factor
    refused(INVALID)

    s.setRegularization(1, [1e-3] * len(case["caps"]))  # a regularized factorization
    s.factorize_solve(keep_factor=True)
    assert rc_host(s, g) == UNSUPPORTED
    assert b"regularization_type" in capi.lib().lexls_last_error()
    assert rc_device(s, g) == (UNSUPPORTED, True)
    assert rc_get(s, G, f) == INVALID
    assert (G == 7.0).all() and (f == 7).all()
    s.close()


def test_solve_lod_backward_is_the_c_abi_result_and_a_directional_derivative(hip, oracle):
    """`base` through torch: backward returns the bits of lexls_lse_solve_adjoint_matrix on the same factor, and <G, D> for a drawn direction D of
    unit Frobenius norm per problem is the oracle's (g.x(A + h D) - g.x(A - h D)) / 2h within AM.FD_BOUND (the central differences' own error,
    measured on the CPU in adjoint_matrix_cases; relative to max(1, largest |G| of the problem))"""
    from lexls_amd.torch_adjoint import solve_lod
    case = AM.build("base")
    B, n, cap = case["lod"].shape[0], case["n"], case["lod"].shape[2]
    s = hip.BatchedLexLSE(B, n, case["caps"])
    lod = torch.from_numpy(np.array(case["lod"])).cuda().requires_grad_(True)
    g = torch.from_numpy(np.array(case["g"])).cuda()
    x = solve_lod(s, lod)
    assert float(np.abs(x.detach().cpu().numpy() - case["ref"]["x"]).max()) <= 1e-10
    (g * x).sum().backward()
    G = lod.grad.cpu().numpy()
    assert s.differentiable.cpu().numpy().tolist() == AM.FLAGS["base"]
    want, _ = s.solve_adjoint_matrix(case["g"])
    np.testing.assert_array_equal(G, want)
    D = P.normal(AM.CASE_SEED("base") + 333, B * (n + 1) * cap).reshape(B, n + 1, cap)
    D /= np.sqrt((D * D).sum(axis=(1, 2)))[:, None, None]
    xp = AM.run_oracle(case, case["lod"] + AM.FD_H * D)["x"]
    xm = AM.run_oracle(case, case["lod"] - AM.FD_H * D)["x"]
    fd = ((xp - xm) * case["g"]).sum(axis=1) / (2 * AM.FD_H)
    got = (G * D).sum(axis=(1, 2))
    err = np.abs(got - fd) / np.maximum(1.0, np.abs(case["A"]).max(axis=(1, 2)))
    print(f"directional derivative: device {got} central differences {fd} gap {err.max():.2e} (bound {AM.FD_BOUND:.0e})")
    assert err.max() <= AM.FD_BOUND
    s.close()
