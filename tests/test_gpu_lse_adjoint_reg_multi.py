"""The many-cotangent adjoint of the regularized LexLSE solve on the device (lexls_lse_solve_adjoint_multi* after a factorization with
regularization type 1, 3, 4, 5, 8 or 9 on a handle with lexls_lse_set_adjoint_regularized_multi: solve_adjoint_reg_multi_kernel, lane =
cotangent) against reference (A) of tests/adjoint_reg_multi_cases.py — G M_reg and G N_reg from unit solves on the oracle — within XC.TOL
(derived there from the references' own disagreement on the CPU, never from the device's figures).  The variant the placement rule takes is
named (last_consumer_kernel); the independence contract is held bit for bit; the refusals leave the outputs alone."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
import adjoint_reg_cases as RC
import adjoint_reg_multi_cases as XC
from lexls_amd import capi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
G64, W41 = "lqr_generic<64,lds>", "lqr_wave<41,12,regularized>"
# the producers of tests/test_gpu_lse_adjoint_reg.py (automatic and policy 1; None: whatever the dispatch plan gives, printed)
POLICIES = {name: {None: W41, 1: G64} for name in RC.NAMES}
POLICIES["ragged"] = POLICIES["fixed_ragged"] = {None: None, 1: G64}
POLICIES["wide"] = {None: "lqr_generic<256,lds>"}
for _name in XC.NEW:
    POLICIES[_name] = {None: None, 1: None}


def handle(hip, case, reg_type, policy=None, factors=None, variable=0.0, multi=True, single=False):
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
    s.set_adjoint_regularized_multi(multi)
    s.set_adjoint_regularized(single)
    return s


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def host_form(s, G):
    """lexls_lse_solve_adjoint_multi + lexls_lse_get_adjoint_multi through the C ABI (K = 1 included)"""
    G = np.ascontiguousarray(G, np.float64)
    K = G.shape[1]
    capi.check(capi.lib().lexls_lse_solve_adjoint_multi(s._h, ptr(G), K))
    rhs, fixed = np.full((s.batch, K, s.cap), 7.0), np.full((s.batch, K, s.nVar), 7.0)
    capi.check(capi.lib().lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)))
    return rhs, fixed


def device_form(s, G, with_fixed=True):
    K = G.shape[1]
    d_G = torch.from_numpy(np.array(G, np.float64)).cuda()
    d_rhs = torch.full((s.batch, K, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((s.batch, K, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    capi.check(capi.lib().lexls_lse_solve_adjoint_multi_device(s._h, C.c_void_p(d_G.data_ptr()), K, C.c_void_p(d_rhs.data_ptr()),
                                                                C.c_void_p(d_fixed.data_ptr()) if with_fixed else None))
    s.synchronize()
    if not with_fixed:
        assert bool((d_fixed == 7.0).all()), "grad_fixed was not wanted and was written"
    return d_rhs.cpu().numpy(), d_fixed.cpu().numpy() if with_fixed else None


@pytest.mark.parametrize("name", XC.NAMES)
def test_every_set_within_tol_of_the_unit_solves(hip, oracle, name):
    worst = {}
    for reg_type in XC.types_of(name):
        case = XC.build(name, reg_type)
        m, nf = case["dims"].sum(axis=1), case["nf"]
        first = {}
        for policy, producer in POLICIES[name].items():
            s = handle(hip, case, reg_type, policy)
            s.factorize_solve(keep_factor=True)
            ctx = f"{name} type {reg_type} on {s.last_kernel()}: "
            assert s.last_kernel().startswith("lqr_") and (producer is None or s.last_kernel() == producer), ctx
            assert float(np.abs(s.get_x() - case["ref"]["x"]).max()) <= 1e-10 * max(1.0, float(np.abs(case["ref"]["x"]).max())), ctx + "the forward solve"
            before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
            for st, G in case["G"].items():
                rhs, fixed = host_form(s, G)
                assert s.last_consumer_kernel() == case["variant"], ctx + s.last_consumer_kernel()
                e_rhs, e_fixed = XC.gap(rhs, case["A"][st][0]), XC.gap(fixed, case["A"][st][1])
                worst[reg_type] = max(worst.get(reg_type, 0.0), e_rhs, e_fixed)
                print(f"{ctx}K = {st}: grad_rhs {e_rhs:.2e} grad_fixed {e_fixed:.2e} (TOL {XC.TOL:.1e})")
                assert e_rhs <= XC.TOL and e_fixed <= XC.TOL, ctx + f"K = {st}: {e_rhs:.3e} {e_fixed:.3e}"
                for b in range(len(m)):  # rows behind a problem's own, slots behind its fixed variables: exactly 0
                    assert not rhs[b, :, m[b]:].any() and not fixed[b, :, nf[b]:].any(), ctx + f"problem {b}"
                if st in first:  # (the A side of the factor is bit-identical behind every producer)
                    np.testing.assert_array_equal(rhs, first[st][0], err_msg=ctx + "against the first producer")
                    np.testing.assert_array_equal(fixed, first[st][1], err_msg=ctx + "against the first producer")
                first.setdefault(st, (rhs, fixed))
            d_rhs, d_fixed = device_form(s, case["G"]["3"])
            np.testing.assert_array_equal(d_rhs, first["3"][0], err_msg=ctx + "device form")
            np.testing.assert_array_equal(d_fixed, first["3"][1], err_msg=ctx + "device form")
            for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
                np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
            s.close()
    print(f"{name}: largest device error per type {({t: '%.1e' % e for t, e in worst.items()})}")


@pytest.mark.parametrize("name", ["base", "fixed_rank_def", "ik", "edge"])
def test_a_cotangent_is_independent_of_its_company_bit_for_bit(hip, oracle, name):
    """ncot = 1, 3, 64, 65 (65 crosses the tile edge); alone, elsewhere, among others; a second run; the device form, with and without grad_fixed.
    (edge: the hbm form, whose matrices live in a work buffer per tile.)"""
    case = XC.build(name, 1)
    s = handle(hip, case, 1)
    s.factorize_solve(keep_factor=True)
    B, n = case["lod"].shape[0], case["n"]
    R = XC.P.normal(20330400, B * 65 * n).reshape(B, 65, n)
    base = host_form(s, R)
    assert s.last_consumer_kernel() == case["variant"]

    def same(got, cols, what):
        for w in (0, 1):
            if got[w] is not None:
                np.testing.assert_array_equal(got[w], base[w][:, cols], err_msg=f"{name}: {what} ({('grad_rhs', 'grad_fixed')[w]})")

    same(host_form(s, R), slice(None), "a second run")
    same(device_form(s, R), slice(None), "the device form")
    same(device_form(s, R, with_fixed=False), slice(None), "the device form without grad_fixed")
    for c in (0, 5, 63, 64):  # alone: ncot = 1, lane 0 of tile 0
        same(host_form(s, R[:, c:c + 1]), [c], f"cotangent {c} alone")
    same(host_form(s, R[:, :3]), [0, 1, 2], "the first three")
    same(host_form(s, R[:, :64]), slice(0, 64), "one full tile")
    same(host_form(s, R[:, 1:65]), slice(1, 65), "one full tile, every cotangent a lane further down")
    c = 7  # at positions 0, 63 and 64 of a K = 65 set: first lane, last lane, a second tile
    for position in (0, 63, 64):
        order = np.arange(65)
        order[[position, c]] = order[[c, position]]
        same(host_form(s, R[:, order]), order, f"cotangent {c} at position {position}")
    other = R.copy()  # among different neighbours: every other cotangent replaced
    other[:, np.arange(65) != c] = XC.P.normal(20330401, B * 64 * n).reshape(B, 64, n)
    got = host_form(s, other)
    np.testing.assert_array_equal(got[0][:, c], base[0][:, c])
    np.testing.assert_array_equal(got[1][:, c], base[1][:, c])
    s.close()


@pytest.mark.parametrize("name", ["base", "fixed_rank_def", "ik", "deep", "wide"])
def test_within_tol_of_the_single_cotangent_call_on_the_same_factor(hip, oracle, name):
    """tolerance, not bits (the summation order differs); both switches on"""
    for reg_type in XC.types_of(name):
        case = XC.build(name, reg_type)
        s = handle(hip, case, reg_type, single=True)
        s.factorize_solve(keep_factor=True)
        G = case["G"]["3"]
        rhs, fixed = host_form(s, G)
        assert s.last_consumer_kernel() == case["variant"]
        worst = 0.0
        for c in range(G.shape[1]):
            one = s.solve_adjoint(G[:, c])
            assert s.last_consumer_kernel() == RC.variant(case["n"], sum(case["caps"]), len(case["caps"]))
            worst = max(worst, XC.gap(rhs[:, c], one[0]), XC.gap(fixed[:, c], one[1]))
            if case["variant"].endswith("x K"):  # the fall-back form IS the single-cotangent kernel: bits
                np.testing.assert_array_equal(rhs[:, c], one[0]), np.testing.assert_array_equal(fixed[:, c], one[1])
        print(f"{name} type {reg_type}: multi against the single-cotangent call {worst:.2e} (TOL {XC.TOL:.1e})")
        assert worst <= XC.TOL
        s.close()


def multi_rc(s, G):
    """both forms through the C ABI on outputs pre-filled with 7.0 -> (rc host, rc device, outputs untouched)"""
    lib = capi.lib()
    G = np.ascontiguousarray(G)
    K = G.shape[1]
    rc_host = lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), K)
    err = lib.lexls_last_error()
    rhs, fixed = np.full((s.batch, K, s.cap), 7.0), np.full((s.batch, K, s.nVar), 7.0)
    assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)) == INVALID  # (there is nothing to return)
    d_G = torch.from_numpy(np.array(G)).cuda()
    d_rhs = torch.full((s.batch, K, s.cap), 7.0, dtype=torch.float64, device="cuda")
    d_fixed = torch.full((s.batch, K, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    rc_dev = lib.lexls_lse_solve_adjoint_multi_device(s._h, C.c_void_p(d_G.data_ptr()), K, C.c_void_p(d_rhs.data_ptr()), C.c_void_p(d_fixed.data_ptr()))
    s.synchronize()
    untouched = bool((rhs == 7.0).all() and (fixed == 7.0).all() and (d_rhs == 7.0).all() and (d_fixed == 7.0).all())
    return rc_host, rc_dev, untouched, err


def test_the_refusals_name_their_reason_and_leave_the_outputs_alone(hip, oracle):
    case = XC.build("base", 1)
    G = case["G"]["3"]
    # the switch off (the single-cotangent switch on does not open the multi calls)
    s = handle(hip, case, 1, policy=1, multi=False, single=True)
    s.factorize_solve(keep_factor=True)
    rc_host, rc_dev, untouched, err = multi_rc(s, G)
    assert (rc_host, rc_dev, untouched) == (UNSUPPORTED, UNSUPPORTED, True)
    assert b"regularization_type" in err and b"lexls_lse_set_adjoint_regularized_multi" in err, err
    assert "adjoint" not in s.last_consumer_kernel()
    s.set_adjoint_regularized_multi(True)  # (no new factorization needed: the switch is about the call, not about the factor)
    got = host_form(s, G)
    assert XC.gap(got[0], case["A"]["3"][0]) <= XC.TOL
    s.close()
    # the switch on: types 2, 6, 7 and a variable factor
    for reg_type, variable, word in ((2, 0.0, b"regularization_type 2"), (6, 0.0, b"regularization_type 6"), (7, 0.0, b"regularization_type 7"),
                                     (1, 0.5, b"variable_regularization_factor"), (3, 0.5, b"variable_regularization_factor")):
        s = handle(hip, case, reg_type, policy=1, factors=np.full(len(case["caps"]), 0.2), variable=variable)
        s.factorize_solve(keep_factor=True)
        rc_host, rc_dev, untouched, err = multi_rc(s, G)
        assert (rc_host, rc_dev, untouched) == (UNSUPPORTED, UNSUPPORTED, True), (reg_type, variable)
        assert word in err, err
        assert "adjoint" not in s.last_consumer_kernel()
        with pytest.raises(Exception):
            s.jacobian_device()
        s.close()


def test_the_new_switch_opens_neither_the_single_call_nor_the_matrix_gradient(hip, oracle):
    case = XC.build("base", 1)
    lib = capi.lib()
    s = handle(hip, case, 1, policy=1, multi=True, single=False)
    s.factorize_solve(keep_factor=True)
    g = np.ascontiguousarray(case["g"])
    assert lib.lexls_lse_solve_adjoint(s._h, ptr(g)) == UNSUPPORTED
    assert b"lexls_lse_set_adjoint_regularized" in lib.lexls_last_error()
    assert lib.lexls_lse_solve_adjoint_matrix(s._h, ptr(g)) == UNSUPPORTED
    s.set_adjoint_regularized(True)
    assert lib.lexls_lse_solve_adjoint_matrix(s._h, ptr(g)) == UNSUPPORTED
    # the Python method sends one cotangent to the multi entry while the single switch is off
    s.set_adjoint_regularized(False)
    one = s.solve_adjoint_multi(case["G"]["3"][:, :1])
    assert s.last_consumer_kernel() == case["variant"]
    np.testing.assert_array_equal(one[0], host_form(s, case["G"]["3"])[0][:, :1])
    s.close()


@pytest.mark.parametrize("name", ["base", "fixed", "ik"])
def test_without_regularization_both_switches_change_nothing(hip, oracle, name):
    """reg_type == 0 on a handle with both switches on that ran regularized before: the variant and the bits are those of a plain handle"""
    import adjoint_multi_cases as MC
    case = AC.build(name)
    B, n = case["lod"].shape[0], case["n"]
    G = XC.P.normal(20330402, B * 5 * n).reshape(B, 5, n)
    plain = handle(hip, case, 0, multi=False)
    plain.factorize_solve(keep_factor=True)
    want = host_form(plain, G)
    assert plain.last_consumer_kernel() == MC.STAGED
    damped = dict(case, factors=RC.factors(B, len(case["caps"])))
    s = handle(hip, damped, 1, single=True)
    s.factorize_solve(keep_factor=True)
    got = host_form(s, G)
    assert s.last_consumer_kernel() == XC.LDS and np.abs(got[0] - want[0]).max() > 1e-6
    s.setRegularization(0)
    s.factorize_solve(keep_factor=True)
    got = host_form(s, G)
    assert s.last_consumer_kernel() == MC.STAGED
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    plain.close()
    s.close()


def test_the_jacobian_of_a_damped_ik_handle_is_m_reg(hip, oracle):
    from lexls_amd.torch_adjoint import jacobian_rhs
    case = XC.build("ik", 1)
    s = handle(hip, case, 1)
    s.factorize_solve(keep_factor=True)
    dx_db, dx_dfixed = s.jacobian_device()
    s.synchronize()
    assert s.last_consumer_kernel() == XC.LDS
    J = dx_db.cpu().numpy()
    for b, (M, _) in enumerate(case["maps"]):
        e = float(np.abs(J[b][:, :M.shape[1]] - M).max()) / max(1.0, float(np.abs(M).max()))
        assert e <= XC.TOL, (b, e)
        assert not J[b][:, M.shape[1]:].any()
    assert not dx_dfixed.cpu().numpy().any()  # (no fixed variables in this case)
    again = jacobian_rhs(s)
    s.synchronize()
    np.testing.assert_array_equal(again[0].cpu().numpy(), J)
    s.close()
