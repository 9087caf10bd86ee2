"""Gradients of batched LexLSI solutions with respect to the bounds on the device (lexls_lsi_batch_solve_adjoint(_device), LsiBatch.solve_adjoint,
torch_adjoint.SolveBounds) against the references of tests/lsi_adjoint_cases.py: reference (A) within TOL, the dot-product identities of (B),
bit-equality between the forms and the orders of calls, the status, mask and row-count rules, the error rules, gradcheck."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
import lsi_adjoint_cases as LC
from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SENTINEL = 7.25


def rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def upload(pk):
    data = torch.from_numpy(pk.data).cuda()
    var = None if pk.var_index is None else torch.from_numpy(pk.var_index.astype(np.int32)).cuda()
    return data, var


def solve(entry, probs, n, batch_obj=None, **params):
    """the problems through one of the three entries -> (LsiBatch, x, active, v, status) as numpy"""
    from lexls_amd import lexlsi
    pk = lexlsi.pack_batch(n, probs)
    b = batch_obj or lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    if entry == "run":
        r = b.run(pk, **params)
        return b, r["x"], r["active"], r["v"], np.asarray([r["info"][i]["status"] for i in range(pk.batch)])
    data, var = upload(pk)
    if entry == "run_device":
        r = b.run_device(data, var_index=var, **params)
    else:
        r = b.enqueue_device(data, var_index=var, **params)
        b.finish()
    torch.cuda.synchronize()
    return b, r["x"].cpu().numpy(), r["active"].cpu().numpy(), r["v"].cpu().numpy(), r["info"].cpu().numpy()[:, 0]


def assert_reference(case, glb, gub, what):
    """within TOL of (A), exact zeros outside the working set, and the identities of (B)"""
    ra, rb = case["A"]
    print(f"{what}: gap to (A) {max(rel(glb, ra), rel(gub, rb)):.2e} (TOL {LC.TOL:.0e})")
    assert rel(glb, ra) <= LC.TOL and rel(gub, rb) <= LC.TOL, what
    act = case["active"]
    assert not glb[act != LC.LB].any() and not gub[(act != LC.UB) & (act != LC.EQ)].any(), what
    for dlb, dub, dx in case.get("pairs", ()):
        gap = AC.identity_gap((np.hstack([dlb, dub]), dx), case["g"], np.hstack([glb, gub]))
        print(f"{what}: identity gap {gap:.2e}")
        assert gap <= LC.TOL, what


@pytest.mark.parametrize("name", list(LC.CASES))
def test_cases_against_the_references_and_bit_equality(hip, name):
    case = LC.build(name)
    b, x, active, v, status = solve("run", case["probs"], case["n"])
    np.testing.assert_array_equal(active, case["active"])  # the run is the oracle's (tests/test_gpu_lsi.py checks it in depth)
    np.testing.assert_array_equal(status, case["status"])
    glb, gub = b.solve_adjoint(case["g"])
    assert_reference(case, glb, gub, name)
    # the same bits: a second call, another g in between, the device form, one output alone
    b.solve_adjoint(2.0 * case["g"] + 1.0)
    glb2, gub2 = b.solve_adjoint(case["g"])
    np.testing.assert_array_equal(glb2, glb), np.testing.assert_array_equal(gub2, gub)
    dlb, dub = b.solve_adjoint_device(torch.from_numpy(case["g"].copy()).cuda())
    np.testing.assert_array_equal(dlb.cpu().numpy(), glb), np.testing.assert_array_equal(dub.cpu().numpy(), gub)
    from lexls_amd import capi
    only = np.full_like(glb, SENTINEL)
    g = np.ascontiguousarray(case["g"])
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint(b._h, g.ctypes.data_as(C.POINTER(C.c_double)), None, only.ctypes.data_as(C.POINTER(C.c_double))))
    np.testing.assert_array_equal(only, gub)
    # get_lambda after the adjoint (the kept factor is reused) against get_lambda before it on a fresh batch, and the adjoint behind it
    lam_after = b.lambda_array()
    glb3, gub3 = b.solve_adjoint(case["g"])
    np.testing.assert_array_equal(glb3, glb), np.testing.assert_array_equal(gub3, gub)
    b.close()
    b, x2, active2, v2, _ = solve("run", case["probs"], case["n"])
    lam_before = b.lambda_array()
    glb4, gub4 = b.solve_adjoint(case["g"])
    np.testing.assert_array_equal(lam_before, lam_after)
    np.testing.assert_array_equal(glb4, glb), np.testing.assert_array_equal(gub4, gub)
    np.testing.assert_array_equal(b.lambda_array(), lam_before)
    np.testing.assert_array_equal(x2, x), np.testing.assert_array_equal(active2, active), np.testing.assert_array_equal(v2, v)
    b.close()


def test_device_results_are_not_touched(hip):
    """x, active, v and lambda of a run_device run stay as they are"""
    from lexls_amd import lexlsi
    case = LC.build("small_sb")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    r = b.run_device(data, var_index=var, with_lambda=True)
    keep = {k: t.clone() for k, t in r.items()}
    glb, gub = b.solve_adjoint_device(torch.from_numpy(case["g"].copy()).cuda())
    assert_reference(case, glb.cpu().numpy(), gub.cpu().numpy(), "small_sb, run_device")
    for k, t in r.items():
        assert torch.equal(t, keep[k]), k
    np.testing.assert_array_equal(b.lambda_array(), keep["lambda"].cpu().numpy())
    b.close()


@pytest.mark.parametrize("entry,fused", [("run", True), ("run_device", True), ("enqueue", True), ("run_device", False)])
def test_entries_and_launch_paths(hip, monkeypatch, entry, fused):
    """the IK shape through every entry; the persistent launch and the lock-step stages, named by last_kernel()"""
    if not fused:
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    case = LC.build("ik")
    b, x, active, v, status = solve(entry, case["probs"], case["n"])
    kernel = b.last_kernel()
    assert kernel.startswith("lsi_fused<") if fused else (not kernel.startswith("lsi_fused<") and kernel not in ("host", "")), kernel
    np.testing.assert_array_equal(active, case["active"])
    glb, gub = b.solve_adjoint(case["g"])
    assert_reference(case, glb, gub, f"ik, {entry}, {kernel}")
    b.close()


@pytest.mark.parametrize("entry", ["run", "run_device"])
def test_status_rule(hip, entry):
    """cold, max_number_of_factorizations = 1: exact zeros in every row of the instances the budget stopped, values in the others"""
    bd = LC.build_budget()
    assert (bd["status"] != LC.SOLVED).any() and (bd["status"] == LC.SOLVED).any()
    b, _, active, _, status = solve(entry, bd["probs"], bd["n"], max_number_of_factorizations=1)
    np.testing.assert_array_equal(status, bd["status"])
    np.testing.assert_array_equal(active, bd["active"])
    glb, gub = (np.full((len(bd["probs"]), active.shape[1]), SENTINEL) for _ in range(2))
    from lexls_amd import capi
    dp = C.POINTER(C.c_double)
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint(b._h, np.ascontiguousarray(bd["g"]).ctypes.data_as(dp), glb.ctypes.data_as(dp), gub.ctypes.data_as(dp)))
    stopped = bd["status"] != LC.SOLVED
    assert not glb[stopped].any() and not gub[stopped].any() and active[stopped].any()
    assert np.abs(gub[~stopped]).max() > 1e-3
    assert_reference(bd, glb, gub, f"budget, {entry}")
    b.close()


def test_instance_mask(hip):
    """skipped instances keep their sentinels in both outputs and both forms; the others carry the bits of the unmasked run"""
    from lexls_amd import lexlsi
    case = LC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g = torch.from_numpy(case["g"].copy()).cuda()
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full = [t.cpu().numpy() for t in b.solve_adjoint_device(g)]
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    out = [torch.full((pk.batch, pk.total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)]
    b.solve_adjoint_device(g, out[0], out[1])
    host = [np.full((pk.batch, pk.total), SENTINEL) for _ in range(2)]
    dp = C.POINTER(C.c_double)
    from lexls_amd import capi
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint(b._h, np.ascontiguousarray(case["g"]).ctypes.data_as(dp), host[0].ctypes.data_as(dp), host[1].ctypes.data_as(dp)))
    for got, hst, ref in zip(out, host, full):
        got = got.cpu().numpy()
        assert (got[mask == 0] == SENTINEL).all() and (hst[mask == 0] == SENTINEL).all()
        np.testing.assert_array_equal(got[mask == 1], ref[mask == 1])
        np.testing.assert_array_equal(hst[mask == 1], ref[mask == 1])
    b.set_instance_mask(None)
    b.close()


def test_instance_obj_dims(hip):
    """rows that are absent under set_instance_obj_dims are exactly 0; an instance with its full counts carries the bits of the plain run"""
    from lexls_amd import lexlsi
    case = LC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g = torch.from_numpy(case["g"].copy()).cuda()
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full = [t.cpu().numpy() for t in b.solve_adjoint_device(g)]
    counts = np.tile(pk.dims.astype(np.int32), (pk.batch, 1))
    counts[1] = [12, 7, 12, 0, 12]
    counts[5] = [3, 12, 5, 12, 12]
    b.set_instance_obj_dims(torch.from_numpy(counts).cuda())
    r = b.run_device(data, var_index=var)
    active = r["active"].cpu().numpy()
    status = r["info"].cpu().numpy()[:, 0]
    got = [t.cpu().numpy() for t in b.solve_adjoint_device(g)]
    first = np.concatenate([[0], np.cumsum(pk.dims)]).astype(int)
    absent = np.zeros((pk.batch, pk.total), bool)
    for i in (1, 5):
        for k in range(len(pk.dims)):
            absent[i, first[k] + counts[i, k]:first[k + 1]] = True
    assert absent.any() and not got[0][absent].any() and not got[1][absent].any() and not active[absent].any()
    assert not got[0][active != LC.LB].any() and not got[1][(active != LC.UB) & (active != LC.EQ)].any()
    for i in range(pk.batch):
        if i not in (1, 5):
            np.testing.assert_array_equal(got[0][i], full[0][i]), np.testing.assert_array_equal(got[1][i], full[1][i])
        elif status[i] == LC.SOLVED:
            assert np.abs(got[0][i]).max() + np.abs(got[1][i]).max() > 1e-6
    b.set_instance_obj_dims(None)
    b.close()


def test_error_rules(hip):
    """each refusal comes with the outputs left alone"""
    from lexls_amd import capi, lexlsi
    case = LC.build("ik")
    n = case["n"]
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib, dp = capi.lib(), C.POINTER(C.c_double)
    g = np.array(case["g"])
    glb, gub = np.full((pk.batch, pk.total), SENTINEL), np.full((pk.batch, pk.total), SENTINEL)
    d_g = torch.from_numpy(g).cuda()
    d_lb, d_ub = (torch.full((pk.batch, pk.total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))

    def both(code, needle=None):
        assert lib.lexls_lsi_batch_solve_adjoint(b._h, g.ctypes.data_as(dp), glb.ctypes.data_as(dp), gub.ctypes.data_as(dp)) == code
        if needle:
            assert needle in lib.lexls_last_error(), lib.lexls_last_error()
        assert lib.lexls_lsi_batch_solve_adjoint_device(b._h, C.c_void_p(d_g.data_ptr()), C.c_void_p(d_lb.data_ptr()), C.c_void_p(d_ub.data_ptr())) == code
        torch.cuda.synchronize()
        assert (glb == SENTINEL).all() and (gub == SENTINEL).all() and bool((d_lb == SENTINEL).all()) and bool((d_ub == SENTINEL).all())

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
    assert lib.lexls_lsi_batch_solve_adjoint(b._h, None, glb.ctypes.data_as(dp), gub.ctypes.data_as(dp)) == INVALID and b"null g" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint(b._h, g.ctypes.data_as(dp), None, None) == INVALID and b"both outputs" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_device(b._h, None, C.c_void_p(d_lb.data_ptr()), C.c_void_p(d_ub.data_ptr())) == INVALID
    assert lib.lexls_lsi_batch_solve_adjoint_device(b._h, C.c_void_p(d_g.data_ptr()), None, None) == INVALID
    assert (glb == SENTINEL).all() and (gub == SENTINEL).all() and bool((d_lb == SENTINEL).all()) and bool((d_ub == SENTINEL).all())
    # and the plain run behind them is served: the sentinels go
    assert lib.lexls_lsi_batch_solve_adjoint(b._h, g.ctypes.data_as(dp), glb.ctypes.data_as(dp), gub.ctypes.data_as(dp)) == 0
    assert lib.lexls_lsi_batch_solve_adjoint_device(b._h, C.c_void_p(d_g.data_ptr()), C.c_void_p(d_lb.data_ptr()), C.c_void_p(d_ub.data_ptr())) == 0
    torch.cuda.synchronize()
    assert not (glb == SENTINEL).any() and not (gub == SENTINEL).any()
    np.testing.assert_array_equal(d_lb.cpu().numpy(), glb), np.testing.assert_array_equal(d_ub.cpu().numpy(), gub)
    b.close()


def range_problems(count, n=4, dims=(4, 2, 2), seed0=20300701):
    """lsi_problem with the last level's equalities opened to ranges: every bound can move on its own"""
    out = []
    for i in range(count):
        objs = P.lsi_problem(seed0 + i, n, dims)
        w = 0.2 + P.uniform(seed0 + 100 + i, dims[-1])
        objs[-1]["lb"], objs[-1]["ub"] = objs[-1]["lb"] - w, objs[-1]["ub"] + w
        out.append(objs)
    return out


def test_solve_bounds_gradcheck(hip):
    """torch.autograd.gradcheck on SolveBounds, n = 4, batch 2; the working set holds under every perturbation (asserted on `active`)"""
    from lexls_amd import lexlsi
    from lexls_amd.torch_adjoint import SolveBounds, solve_bounds
    n, probs = 4, range_problems(2)
    pk = lexlsi.pack_batch(n, probs)
    data, var = upload(pk)
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lb0, ub0 = (np.stack(a) for a in zip(*(LC.bounds_of(o) for o in probs)))
    lb, ub = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (lb0, ub0))
    seen = []

    def fn(lo, hi):
        out = {}
        x = solve_bounds(lo, hi, b, data, var_index=var, out=out)
        seen.append((out["active"].clone(), out["info"][:, 0].clone()))
        return x

    x = fn(lb, ub)
    base_active = seen[0][0]
    assert bool(base_active.any()) and bool((seen[0][1] == LC.SOLVED).all())
    ref = [LC.oracle.lsi_run(n, o) for o in probs]
    np.testing.assert_array_equal(base_active.cpu().numpy(), np.stack([np.concatenate(r["active"]) for r in ref]))
    x.sum().backward()
    assert lb.grad is not None and ub.grad is not None and bool((lb.grad != 0).any() or (ub.grad != 0).any())
    assert torch.autograd.gradcheck(fn, (lb, ub), eps=1e-6, atol=1e-7, rtol=1e-7, check_undefined_grad=False, check_batched_grad=False)
    assert len(seen) > 2 * lb.numel()
    for active, status in seen:
        assert torch.equal(active, base_active) and bool((status == LC.SOLVED).all())
    with pytest.raises(ValueError, match="no derivatives with respect to A"):
        SolveBounds.apply(lb, ub, b, data.clone().requires_grad_(True), var, None, None, None, None)
    b.close()
