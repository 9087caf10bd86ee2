"""Gradients of batched LexLSI solutions with respect to the bounds for many cotangents per pass (lexls_lsi_batch_solve_adjoint_multi(_device),
lsi_adjoint_scatter_multi_kernel, LsiBatch.solve_adjoint_multi / jacobian_bounds_device) on the cases of tests/lsi_adjoint_cases.py: every
instance and cotangent within that file's TOL of K calls of solve_adjoint_device with the exact zeros at the same entries; the status, mask
and call-order rules; the Jacobian against (B)'s bound perturbations of size PERTURB; the error rules."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_cases as LC
from lexls_amd import capi
from lexls_amd import problems as P
from test_gpu_lsi_adjoint import SENTINEL, rel, solve, upload

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
DP = C.POINTER(C.c_double)


def cotangents(case, K):
    """(batch, K, n): the case's own g first, the rest iid normal"""
    B, n = case["g"].shape
    G = P.normal(20300901 + K, B * K * n).reshape(B, K, n)
    G[:, 0] = case["g"]
    return G


def host_form(b, G, total, fill=None):
    """lexls_lsi_batch_solve_adjoint_multi through the C ABI (K = 1 included) on outputs that hold `fill`"""
    G = np.ascontiguousarray(G, np.float64)
    glb, gub = (np.full((G.shape[0], G.shape[1], total), SENTINEL if fill is None else fill) for _ in range(2))
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_multi(b._h, G.ctypes.data_as(DP), G.shape[1], glb.ctypes.data_as(DP), gub.ctypes.data_as(DP)))
    return glb, gub


def device_form(b, G, total):
    d_G = torch.from_numpy(np.array(G, np.float64)).cuda()
    d_lb, d_ub = (torch.full((G.shape[0], G.shape[1], total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_multi_device(b._h, C.c_void_p(d_G.data_ptr()), G.shape[1], C.c_void_p(d_lb.data_ptr()),
                                                                     C.c_void_p(d_ub.data_ptr())))
    torch.cuda.synchronize()
    return d_lb.cpu().numpy(), d_ub.cpu().numpy()


def single_calls(b, G):
    """K calls of the existing solve_adjoint_device, stacked (batch, K, total)"""
    out = [b.solve_adjoint_device(torch.from_numpy(np.ascontiguousarray(G[:, c])).cuda()) for c in range(G.shape[1])]
    return np.stack([o[0].cpu().numpy() for o in out], axis=1), np.stack([o[1].cpu().numpy() for o in out], axis=1)


def assert_close_with_the_same_zeros(got, ref, what):
    worst = 0.0
    for w in (0, 1):
        for i in range(ref[w].shape[0]):  # every instance against its own magnitude
            worst = max(worst, rel(got[w][i], ref[w][i]))
        np.testing.assert_array_equal(got[w] == 0.0, ref[w] == 0.0, err_msg=what + ": the exact zeros sit elsewhere")
    print(f"{what}: against K single-cotangent calls {worst:.2e} (TOL {LC.TOL:.0e})")
    assert worst <= LC.TOL, what


@pytest.mark.parametrize("name", list(LC.CASES))
def test_cases_against_k_single_calls_and_bit_equality(hip, name):
    case = LC.build(name)
    n = case["n"]
    b, x, active, v, status = solve("run", case["probs"], n)
    np.testing.assert_array_equal(active, case["active"])
    total = active.shape[1]
    base = None
    sets = {"3": cotangents(case, 3), "65": cotangents(case, 65), "identity": np.ascontiguousarray(np.broadcast_to(np.eye(n), (len(case["probs"]), n, n)))}
    for K, G in sets.items():
        got = host_form(b, G, total)
        assert_close_with_the_same_zeros(got, single_calls(b, G), f"{name}, K = {K}")
        again, dev = host_form(b, G, total), device_form(b, G, total)
        for w in (0, 1):
            np.testing.assert_array_equal(again[w], got[w]), np.testing.assert_array_equal(dev[w], got[w])
        if K == "65":
            base = (G, got)
    G, got = base
    # reference (A) of the case for its own g, which is cotangent 0; the working set's types decide where the zeros are
    assert rel(got[0][:, 0], case["A"][0]) <= LC.TOL and rel(got[1][:, 0], case["A"][1]) <= LC.TOL
    act = case["active"]
    assert not got[0][:, 0][act != LC.LB].any() and not got[1][:, 0][(act != LC.UB) & (act != LC.EQ)].any()
    # independence, bit for bit: alone, and in a permuted set; one output alone
    for c in (0, 63, 64):
        alone = host_form(b, G[:, c:c + 1], total)
        np.testing.assert_array_equal(alone[0][:, 0], got[0][:, c]), np.testing.assert_array_equal(alone[1][:, 0], got[1][:, c])
    order = np.random.default_rng(20300902).permutation(65)
    perm = host_form(b, G[:, order], total)
    np.testing.assert_array_equal(perm[0], got[0][:, order]), np.testing.assert_array_equal(perm[1], got[1][:, order])
    only = np.full_like(got[1], SENTINEL)
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_multi(b._h, np.ascontiguousarray(G).ctypes.data_as(DP), 65, None, only.ctypes.data_as(DP)))
    np.testing.assert_array_equal(only, got[1])
    # call orders: get_lambda and solve_adjoint behind the multi form reuse its factor; on a fresh batch in front of it they give equal bits
    lam_after = b.lambda_array()
    one_after = b.solve_adjoint(case["g"])
    np.testing.assert_array_equal(host_form(b, G, total)[0], got[0])
    b.close()
    b, x2, _, _, _ = solve("run", case["probs"], n)
    lam_before = b.lambda_array()
    one_before = b.solve_adjoint(case["g"])
    fresh = host_form(b, G, total)
    np.testing.assert_array_equal(lam_before, lam_after)
    np.testing.assert_array_equal(one_before[0], one_after[0]), np.testing.assert_array_equal(one_before[1], one_after[1])
    np.testing.assert_array_equal(fresh[0], got[0]), np.testing.assert_array_equal(fresh[1], got[1])
    np.testing.assert_array_equal(b.lambda_array(), lam_before)
    np.testing.assert_array_equal(x2, x)
    b.close()


@pytest.mark.parametrize("entry", ["run", "run_device", "enqueue"])
def test_entries(hip, entry):
    case = LC.build("ik")
    b, _, active, _, _ = solve(entry, case["probs"], case["n"])
    np.testing.assert_array_equal(active, case["active"])
    G = cotangents(case, 5)
    got = host_form(b, G, active.shape[1])
    assert_close_with_the_same_zeros(got, single_calls(b, G), f"ik, {entry}")
    assert rel(got[0][:, 0], case["A"][0]) <= LC.TOL and rel(got[1][:, 0], case["A"][1]) <= LC.TOL
    b.close()


@pytest.mark.parametrize("entry", ["run", "run_device"])
def test_status_rule(hip, entry):
    """cold, max_number_of_factorizations = 1: all-zero rows, for every cotangent, in the instances the budget stopped"""
    bd = LC.build_budget()
    b, _, active, _, status = solve(entry, bd["probs"], bd["n"], max_number_of_factorizations=1)
    np.testing.assert_array_equal(status, bd["status"])
    G = cotangents(bd, 5)
    glb, gub = host_form(b, G, active.shape[1])
    stopped = bd["status"] != LC.SOLVED
    assert stopped.any() and (~stopped).any() and active[stopped].any()
    assert not glb[stopped].any() and not gub[stopped].any()
    assert np.abs(gub[~stopped]).max() > 1e-3
    assert rel(glb[:, 0], bd["A"][0]) <= LC.TOL and rel(gub[:, 0], bd["A"][1]) <= LC.TOL
    b.close()


def test_instance_mask(hip):
    """skipped instances keep their sentinels in all K rows of both outputs and both forms; the others carry the bits of the unmasked run"""
    from lexls_amd import lexlsi
    case = LC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    G = cotangents(case, 5)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full = device_form(b, G, pk.total)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    dev, hst = device_form(b, G, pk.total), host_form(b, G, pk.total)
    py = b.solve_adjoint_multi_device(torch.from_numpy(G).cuda(), *(torch.full((pk.batch, 5, pk.total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)))
    for got in (dev, hst, [t.cpu().numpy() for t in py]):
        for w in (0, 1):
            assert (got[w][mask == 0] == SENTINEL).all()
            np.testing.assert_array_equal(got[w][mask == 1], full[w][mask == 1])
    b.set_instance_mask(None)
    b.close()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_jacobian_against_the_bound_perturbations(hip, name):
    """x is affine in the bounds while the working set holds (asserted for these perturbations on the CPU): x(lb1, ub1) - x(lb0, ub0) =
    dx/dlb (lb1 - lb0) + dx/dub (ub1 - ub0) on the solved instances, up to rounding"""
    from lexls_amd.torch_adjoint import jacobian_bounds
    case = LC.build(name)
    assert case["held"]
    b, _, active, _, status = solve("run_device", case["probs"], case["n"])
    J_lb, J_ub = (t.cpu().numpy() for t in b.jacobian_bounds_device())
    assert J_lb.shape == (len(case["probs"]), case["n"], active.shape[1]) == J_ub.shape
    worst = 0.0
    for dlb, dub, dx in case["pairs"]:
        assert 0 < np.abs(dlb).max() <= 10 * LC.PERTURB
        for i in np.flatnonzero(status == LC.SOLVED):
            terms = np.hstack([J_lb[i] * dlb[i], J_ub[i] * dub[i]])  # (n, 2 total)
            scale = max(1.0, float(np.abs(terms).sum(axis=1).max()), float(np.abs(dx[i]).max()))
            worst = max(worst, float(np.abs(terms.sum(axis=1) - dx[i]).max()) / scale)
    print(f"{name}: Jacobian against the perturbations of size {LC.PERTURB:g}: {worst:.2e} (TOL {LC.TOL:.0e})")
    assert worst <= LC.TOL
    again = jacobian_bounds(b)
    np.testing.assert_array_equal(again[0].cpu().numpy(), J_lb), np.testing.assert_array_equal(again[1].cpu().numpy(), J_ub)
    b.close()


def test_error_rules(hip):
    """each refusal comes with the outputs left alone"""
    from lexls_amd import lexlsi
    case = LC.build("ik")
    n, K = case["n"], 3
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib = capi.lib()
    G = cotangents(case, K)
    glb, gub = (np.full((pk.batch, K, pk.total), SENTINEL) for _ in range(2))
    d_G = torch.from_numpy(G).cuda()
    d_lb, d_ub = (torch.full((pk.batch, K, pk.total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))
    p = lambda a: a.ctypes.data_as(DP)  # noqa: E731
    v = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def untouched():
        torch.cuda.synchronize()
        return (glb == SENTINEL).all() and (gub == SENTINEL).all() and bool((d_lb == SENTINEL).all()) and bool((d_ub == SENTINEL).all())

    def both(code, needle=None, ncot=K):
        assert lib.lexls_lsi_batch_solve_adjoint_multi(b._h, p(G), ncot, p(glb), p(gub)) == code
        if needle:
            assert needle in lib.lexls_last_error(), lib.lexls_last_error()
        assert lib.lexls_lsi_batch_solve_adjoint_multi_device(b._h, v(d_G), ncot, v(d_lb), v(d_ub)) == code
        assert untouched()

    both(INVALID, b"no completed")  # before any run
    data, var = upload(pk)
    b.enqueue_device(data, var_index=var)
    both(INVALID, b"waiting for lexls_lsi_batch_finish")  # a pending enqueue
    b.finish()
    b.run(pk, cycling_handling_enabled=1)
    both(UNSUPPORTED, b"cycling handling")
    b.run(pk, regularization_factors=np.array([0, 0.1, 0.1, 0.1, 0.1]), regularization_type=1, max_number_of_factorizations=40)
    both(UNSUPPORTED, b"regularized run")
    b.run(pk)
    both(INVALID, b"ncot == 0", ncot=0)
    assert lib.lexls_lsi_batch_solve_adjoint_multi(b._h, None, K, p(glb), p(gub)) == INVALID and b"null G" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_multi(b._h, p(G), K, None, None) == INVALID and b"both outputs" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_multi_device(b._h, None, K, v(d_lb), v(d_ub)) == INVALID
    assert lib.lexls_lsi_batch_solve_adjoint_multi_device(b._h, v(d_G), K, None, None) == INVALID
    assert untouched()
    # and the plain run behind them is served: the sentinels go
    assert lib.lexls_lsi_batch_solve_adjoint_multi(b._h, p(G), K, p(glb), p(gub)) == 0
    assert lib.lexls_lsi_batch_solve_adjoint_multi_device(b._h, v(d_G), K, v(d_lb), v(d_ub)) == 0
    torch.cuda.synchronize()
    assert not (glb == SENTINEL).any() and not (gub == SENTINEL).any()
    np.testing.assert_array_equal(d_lb.cpu().numpy(), glb), np.testing.assert_array_equal(d_ub.cpu().numpy(), gub)
    b.close()
