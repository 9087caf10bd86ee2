"""The adjoint of the regularized LexLSE solve on the device (lexls_lse_solve_adjoint* after a factorization with regularization type 1, 3, 4, 5, 8
or 9: solve_adjoint_reg_kernel) against reference (A) of tests/adjoint_reg_cases.py — M_reg^T g and N_reg^T g from unit solves on the oracle —
within RC.TOL (derived there from the references' own disagreement on the CPU, never from the device's figures).  The variant is named
(last_consumer_kernel), and so is the producer of the kept factor where the dispatch plan's answer is part of what the case is for."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
import adjoint_reg_cases as RC
from lexls_amd import capi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
G64, W41 = "lqr_generic<64,lds>", "lqr_wave<41,12,regularized>"
# case -> kernel policy (None: automatic) -> the producer of the regularized factor as the host-side dispatch plan names it (None: whatever the
# plan gives the per-problem dimensions, printed).  Policy 1 is the generic kernel with one wavefront; automatic dispatch gives the small shapes
# and the IK shape the regularized register-resident kernel
POLICIES = {name: {None: W41, 1: G64} for name in RC.NAMES}
POLICIES["ragged"] = POLICIES["fixed_ragged"] = {None: None, 1: G64}
POLICIES["wide"] = {None: "lqr_generic<256,lds>"}


def handle(hip, case, reg_type, policy=None, factors=None, variable=0.0):
    s = hip.BatchedLexLSE(case["lod"].shape[0], case["n"], case["caps"])
    if policy is not None:
        s.set_kernel_policy(policy)
    if (case["dims"] != np.asarray(case["caps"], np.uint32)).any():
        s.setObjDim(case["dims"])
    f = case["fixed"]
    if f:
        s.fixVariables(f["nfixed"], f["fixed_idx"], f["fixed_val"])
    s.setProblem(case["lod"])
    if reg_type:
        s.setRegularization(reg_type, case["factors"] if factors is None else factors, variable)
    s.set_adjoint_regularized(True)
    return s


def gap(got, ref):
    return max(float(np.abs(got[b] - ref[b]).max()) / max(1.0, float(np.abs(ref[b]).max())) for b in range(len(ref)))


def device_form(s, g, with_fixed=True):
    B, n, cap = g.shape[0], s.nVar, s.cap
    d_g = torch.from_numpy(np.array(g, np.float64)).cuda()
    d_rhs = torch.full((B, cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda") if with_fixed else None
    s.solve_adjoint_device(d_g, d_rhs, d_fixed)
    s.synchronize()
    return d_rhs.cpu().numpy(), d_fixed.cpu().numpy() if with_fixed else None


@pytest.mark.parametrize("name", RC.NAMES)
def test_device_adjoint_within_tol_of_the_unit_solves(hip, oracle, name):
    worst = {}
    for reg_type in RC.types_of(name):
        case = RC.build(name, reg_type)
        ref_rhs, ref_fixed = case["A"]
        m, nf = case["dims"].sum(axis=1), case["nf"]
        variant = RC.variant(case["n"], sum(case["caps"]), len(case["caps"]))
        assert variant.endswith("hbm>") == (name == "wide")
        first = None
        for policy, producer in POLICIES[name].items():
            s = handle(hip, case, reg_type, policy)
            s.factorize_solve(keep_factor=True)
            ctx = f"{name} type {reg_type} on {s.last_kernel()}: "
            assert s.last_kernel().startswith("lqr_") and (producer is None or s.last_kernel() == producer), ctx
            assert float(np.abs(s.get_x() - case["ref"]["x"]).max()) <= 1e-10 * max(1.0, float(np.abs(case["ref"]["x"]).max())), ctx + "the forward solve"
            before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
            grad_rhs, grad_fixed = s.solve_adjoint(case["g"])
            assert s.last_consumer_kernel() == variant, ctx
            e_rhs, e_fixed = gap(grad_rhs, ref_rhs), gap(grad_fixed, ref_fixed)
            worst[reg_type] = max(worst.get(reg_type, 0.0), e_rhs, e_fixed)
            print(f"{ctx}grad_rhs {e_rhs:.2e} grad_fixed {e_fixed:.2e} (TOL {RC.TOL:.1e})")
            assert e_rhs <= RC.TOL and e_fixed <= RC.TOL, ctx + f"{e_rhs:.3e} {e_fixed:.3e}"
            for b in range(len(m)):  # rows behind a problem's own, slots behind its fixed variables: exactly 0
                assert not grad_rhs[b, m[b]:].any() and not grad_fixed[b, nf[b]:].any(), ctx + f"problem {b}"
            again = s.solve_adjoint(case["g"])  # the same bits from a second run and from the device form
            np.testing.assert_array_equal(again[0], grad_rhs, err_msg=ctx + "second run")
            np.testing.assert_array_equal(again[1], grad_fixed, err_msg=ctx + "second run")
            d_rhs, d_fixed = device_form(s, case["g"])
            assert s.last_consumer_kernel() == variant
            np.testing.assert_array_equal(d_rhs, grad_rhs, err_msg=ctx + "device form")
            np.testing.assert_array_equal(d_fixed, grad_fixed, err_msg=ctx + "device form")
            np.testing.assert_array_equal(device_form(s, case["g"], with_fixed=False)[0], grad_rhs, err_msg=ctx + "device form without grad_fixed")
            if first is None:
                first = (grad_rhs, grad_fixed)
            np.testing.assert_array_equal(grad_rhs, first[0], err_msg=ctx + "against the first producer")  # (the A side of the factor is bit-identical)
            np.testing.assert_array_equal(grad_fixed, first[1], err_msg=ctx + "against the first producer")
            for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
                np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
            s.close()
    print(f"{name}: largest device error per type {({t: '%.1e' % e for t, e in worst.items()})}")


def device_rc(s, g):
    d_g = torch.from_numpy(np.array(g, np.float64)).cuda()
    d_rhs = torch.full((s.batch, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((s.batch, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    rc = capi.lib().lexls_lse_solve_adjoint_device(s._h, C.c_void_p(d_g.data_ptr()), C.c_void_p(d_rhs.data_ptr()), C.c_void_p(d_fixed.data_ptr()))
    s.synchronize()
    return rc, bool((d_rhs == 7.0).all() and (d_fixed == 7.0).all())


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_the_unserved_regularizations_are_refused_with_the_outputs_untouched(hip, oracle):
    case = RC.build("base", 1)
    g = np.ascontiguousarray(case["g"])
    lib = capi.lib()
    for reg_type, variable, word in ((2, 0.0, b"regularization_type 2"), (6, 0.0, b"regularization_type 6"), (7, 0.0, b"regularization_type 7"),
                                     (1, 0.5, b"variable_regularization_factor"), (3, 0.5, b"variable_regularization_factor")):
        s = handle(hip, case, reg_type, policy=1, factors=np.full(len(case["caps"]), 0.2), variable=variable)
        s.factorize_solve(keep_factor=True)
        rhs, fixed = np.full((s.batch, s.cap), 7.0), np.full((s.batch, s.nVar), 7.0)
        assert lib.lexls_lse_solve_adjoint(s._h, ptr(g)) == UNSUPPORTED, (reg_type, variable)
        assert word in lib.lexls_last_error(), lib.lexls_last_error()
        assert device_rc(s, g) == (UNSUPPORTED, True)
        assert lib.lexls_lse_get_adjoint(s._h, ptr(rhs), ptr(fixed)) == INVALID  # (there is nothing to return)
        assert (rhs == 7.0).all() and (fixed == 7.0).all()
        assert "adjoint" not in s.last_consumer_kernel()
        s.close()


def test_a_handle_that_did_not_switch_it_on_is_refused_as_before(hip, oracle):
    case = RC.build("base", 1)
    g = np.ascontiguousarray(case["g"])
    lib = capi.lib()
    s = handle(hip, case, 1, policy=1)
    s.set_adjoint_regularized(False)
    s.factorize_solve(keep_factor=True)
    assert lib.lexls_lse_solve_adjoint(s._h, ptr(g)) == UNSUPPORTED
    assert b"regularization_type" in lib.lexls_last_error() and b"lexls_lse_set_adjoint_regularized" in lib.lexls_last_error()
    assert device_rc(s, g) == (UNSUPPORTED, True)
    s.set_adjoint_regularized(True)  # (no new factorization needed: the switch is about the call, not about the factor)
    got = s.solve_adjoint(case["g"])
    assert gap(got[0], case["A"][0]) <= RC.TOL
    assert lib.lexls_lse_set_adjoint_regularized(None, 1) == INVALID
    s.close()


def test_many_cotangents_and_the_matrix_gradient_stay_refused_under_type_1(hip, oracle):
    case = RC.build("base", 1)
    lib = capi.lib()
    s = handle(hip, case, 1, policy=1)
    s.factorize_solve(keep_factor=True)
    G = np.ascontiguousarray(np.repeat(case["g"][:, None, :], 3, axis=1))
    assert lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), 3) == UNSUPPORTED
    assert b"regularization_type" in lib.lexls_last_error() and b"single-cotangent" in lib.lexls_last_error()
    d_G = torch.from_numpy(np.array(G)).cuda()
    d_rhs = torch.full((s.batch, 3, s.cap), 7.0, dtype=torch.float64, device="cuda")
    assert lib.lexls_lse_solve_adjoint_multi_device(s._h, C.c_void_p(d_G.data_ptr()), 3, C.c_void_p(d_rhs.data_ptr()), None) == UNSUPPORTED
    g = np.ascontiguousarray(case["g"])
    assert lib.lexls_lse_solve_adjoint_matrix(s._h, ptr(g)) == UNSUPPORTED
    assert b"regularization_type" in lib.lexls_last_error() and b"single-cotangent" in lib.lexls_last_error()
    d_g = torch.from_numpy(np.array(g)).cuda()
    d_lod = torch.full((s.batch, s.nVar + 1, s.cap), 7.0, dtype=torch.float64, device="cuda")
    assert lib.lexls_lse_solve_adjoint_matrix_device(s._h, C.c_void_p(d_g.data_ptr()), C.c_void_p(d_lod.data_ptr()), None) == UNSUPPORTED
    s.synchronize()
    assert bool((d_rhs == 7.0).all()) and bool((d_lod == 7.0).all())
    with pytest.raises(Exception):
        s.solve_adjoint_multi(G)
    s.close()


@pytest.mark.parametrize("name", ["base", "fixed", "ik"])
def test_without_regularization_the_plain_kernel_answers_with_a_plain_handles_bits(hip, oracle, name):
    """reg_type == 0 on a handle that ran regularized before: the variant is the unregularized kernel's, the bits are those of a handle of the same
    build that never saw a regularization (nothing of the damped pass is left behind), and they are within tests/adjoint_cases.py's tolerance of
    its reference.  (That the unregularized kernel's device code is the parent's is a statement about the build, not checked here.)"""
    case = AC.build(name)
    plain = handle(hip, case, 0)
    plain.factorize_solve(keep_factor=True)
    want = plain.solve_adjoint(case["g"])
    assert plain.last_consumer_kernel() == "solve_adjoint<64>"
    assert gap(want[0], AC.expected(case)[0]) <= AC.TOL and gap(want[1], AC.expected(case)[1]) <= AC.TOL
    s = handle(hip, case, 1, factors=RC.factors(case["lod"].shape[0], len(case["caps"])))
    s.factorize_solve(keep_factor=True)
    damped = s.solve_adjoint(case["g"])
    assert s.last_consumer_kernel() == "solve_adjoint_reg<64,lds>" and np.abs(damped[0] - want[0]).max() > 1e-6
    s.setRegularization(0)
    s.factorize_solve(keep_factor=True)
    got = s.solve_adjoint(case["g"])
    assert s.last_consumer_kernel() == "solve_adjoint<64>"
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    plain.close()
    s.close()


def test_solve_rhs_backward_under_type_1_is_the_c_abi_result(hip, oracle):
    from lexls_amd.torch_adjoint import SolveRhs
    case = RC.build("one_row", 1)
    s = handle(hip, case, 1)  # (the handle has the damped adjoint switched on: SolveRhs leaves that to the caller)
    lod = torch.from_numpy(np.array(case["lod"])).cuda()
    rhs = lod[:, s.nVar, :].clone().requires_grad_(True)
    x = SolveRhs.apply(rhs, s, lod)
    assert float(np.abs(x.detach().cpu().numpy() - case["ref"]["x"]).max()) <= 1e-10
    g = torch.from_numpy(np.array(case["g"])).cuda()
    (x * g).sum().backward()
    assert s.last_consumer_kernel() == "solve_adjoint_reg<64,lds>"
    want = s.solve_adjoint(case["g"])[0]
    np.testing.assert_array_equal(rhs.grad.cpu().numpy(), want)  # the host form on the same factor: the same bits
    assert gap(want, case["A"][0]) <= RC.TOL
    s.close()
