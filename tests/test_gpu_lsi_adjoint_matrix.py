"""Gradients of batched LexLSI solutions with respect to the constraint data on the device (lexls_lsi_batch_solve_adjoint_matrix(_device),
LsiBatch.solve_adjoint_matrix, torch_adjoint.solve_data) against reference (A) of tests/lsi_adjoint_matrix_cases.py within its TOL: the flags,
the exact zeros as bits, the bound columns against solve_adjoint, bit-equality between the forms and the orders of calls with the final problems
factorized once, the mask, row-count and error rules, a batch split into groups."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_matrix_cases as XC
from test_gpu_lsi_adjoint import solve, upload

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = 1, 3
SENTINEL, FLAG_SENTINEL = 7.25, 9
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
GROUPS_SWITCH = "LEXLS_LSI_GROUPS"


def rel_rows(got, ref):
    """the largest gap, per instance relative to max(1, largest magnitude of the reference)"""
    return max(float(np.abs(got[b] - ref[b]).max()) / max(1.0, float(np.abs(ref[b]).max())) for b in range(len(ref)))


def host_form(b, g, per_data, with_flags=True):
    """the C call itself into outputs that hold sentinels -> (grad_data, flags)"""
    from lexls_amd import capi
    g = np.ascontiguousarray(g)
    out, flags = np.full((g.shape[0], per_data), SENTINEL), np.full(g.shape[0], FLAG_SENTINEL, np.uint8)
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_matrix(b._h, g.ctypes.data_as(DP), out.ctypes.data_as(DP), flags.ctypes.data_as(BP) if with_flags else None))
    return out, flags


def device_form(b, g, per_data):
    out = torch.full((g.shape[0], per_data), SENTINEL, dtype=torch.float64, device="cuda")
    flags = torch.full((g.shape[0],), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    b.solve_adjoint_matrix_device(torch.from_numpy(np.array(g)).cuda(), out, flags)
    return out.cpu().numpy(), flags.cpu().numpy()


def assert_reference(case, got, flags, what):
    """the flags of (A), (A) within TOL, and the zeros as bits: flag-0 and stopped instances whole, rows outside W"""
    np.testing.assert_array_equal(flags, case["flags"], err_msg=what)
    assert flags.tolist() == XC.FLAGS[case["name"]], what
    gap = rel_rows(got, case["A"])
    print(f"{what}: gap to (A) {gap:.2e} (TOL {XC.TOL:.0e})")
    assert gap <= XC.TOL, what
    for i in range(len(flags)):
        if not flags[i] or case["status"][i] != XC.SOLVED:
            assert not got[i].any(), (what, i)
        _, nonzero = XC.split(case, got[i])
        assert not nonzero[case["active"][i] == 0].any(), (what, i)
    assert not (got == SENTINEL).any(), what


@pytest.mark.parametrize("name", XC.CASES)
def test_cases_against_reference_a_both_forms(hip, name):
    case = XC.build(name)
    b, x, active, v, status = solve("run", case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"])  # the run is the oracle's
    np.testing.assert_array_equal(status, case["status"])
    per_data = case["A"].shape[1]
    assert b.per_data == per_data
    got, flags = host_form(b, case["g"], per_data)
    assert_reference(case, got, flags, f"{name}, host form")
    dev, dflags = device_form(b, case["g"], per_data)
    np.testing.assert_array_equal(dev, got), np.testing.assert_array_equal(dflags, flags)  # the two forms: the same bits
    again, _ = host_form(b, case["g"], per_data, with_flags=False)  # the flags are optional
    np.testing.assert_array_equal(again, got)
    # the bound columns of the flag-1 instances are solve_adjoint's
    glb, gub = b.solve_adjoint(case["g"])
    for i in np.flatnonzero(flags):
        parts = b.split_grad_data(got[i])
        lb, ub = np.concatenate([p["lb"] for p in parts]), np.concatenate([p["ub"] for p in parts])
        scale = max(1.0, float(np.abs(glb[i]).max()), float(np.abs(gub[i]).max()))
        assert np.abs(lb - glb[i]).max() / scale <= XC.TOL and np.abs(ub - gub[i]).max() / scale <= XC.TOL, (name, i)
        np.testing.assert_array_equal(lb != 0, glb[i] != 0), np.testing.assert_array_equal(ub != 0, gub[i] != 0)
    if name in ("rank_def", "mixed"):  # solve_adjoint still gives a solved, not rank-stable instance its bound gradients
        assert any(np.abs(gub[i]).max() > 1e-6 for i in np.flatnonzero(flags == 0))
    b.close()


@pytest.mark.parametrize("entry", ["run", "run_device", "enqueue"])
@pytest.mark.parametrize("name", ["mixed", "budget", "small_sb"])
def test_flags_and_values_on_every_entry(hip, entry, name):
    case = XC.build(name)
    b, _, active, _, status = solve(entry, case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"]), np.testing.assert_array_equal(status, case["status"])
    got, flags = device_form(b, case["g"], case["A"].shape[1])
    assert_reference(case, got, flags, f"{name}, {entry}")
    b.close()


def test_call_orders_share_one_factorization_and_change_nothing(hip):
    """lambdas -> matrix -> solve_adjoint; matrix -> lambdas; matrix twice: every output bit-equal across the orders, x / active / v untouched,
    the final problems factorized once per run"""
    from lexls_amd import lexlsi
    case = XC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g, per_data = case["g"], case["A"].shape[1]
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    groups = 1
    results = []
    for order in ("lam,mat,adj", "mat,lam", "mat,mat", "adj,mat,lam"):
        r = b.run_device(data, var_index=var)
        groups = b.stats()["groups"]
        keep = {k: t.clone() for k, t in r.items()}
        count0 = b.final_factorizations()
        out = {}
        for step in order.split(","):
            if step == "lam":
                out["lam"] = b.lambda_array()
            elif step == "adj":
                out["adj"] = b.solve_adjoint(g)
            elif "mat" in out:
                second = device_form(b, g, per_data)
                np.testing.assert_array_equal(second[0], out["mat"][0]), np.testing.assert_array_equal(second[1], out["mat"][1])
            else:
                out["mat"] = device_form(b, g, per_data)
            assert b.final_factorizations() == count0 + groups, (order, step)  # once, at the first call behind the run
        for k, t in r.items():
            assert torch.equal(t, keep[k]), (order, k)
        results.append(out)
    assert_reference(case, *results[0]["mat"], "ik, call orders")
    for out in results[1:]:
        for k, val in out.items():
            ref = next(o[k] for o in results if k in o)
            for a, a0 in zip(val if isinstance(val, tuple) else (val,), ref if isinstance(ref, tuple) else (ref,)):
                np.testing.assert_array_equal(a, a0, err_msg=k)
    b.close()


def test_instance_mask(hip):
    """skipped instances keep their sentinels in slice and flag, in both forms; the others carry the bits of the unmasked call"""
    from lexls_amd import lexlsi
    case = XC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    per_data = case["A"].shape[1]
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full, full_flags = device_form(b, case["g"], per_data)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    for form in (device_form, host_form):
        got, flags = form(b, case["g"], per_data)
        assert (got[mask == 0] == SENTINEL).all() and (flags[mask == 0] == FLAG_SENTINEL).all(), form.__name__
        np.testing.assert_array_equal(got[mask == 1], full[mask == 1]), np.testing.assert_array_equal(flags[mask == 1], full_flags[mask == 1])
    b.set_instance_mask(None)
    b.close()


def test_instance_obj_dims(hip):
    """rows that are absent under set_instance_obj_dims are exact zeros; an instance with its full counts carries the bits of the plain run"""
    from lexls_amd import lexlsi
    case = XC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    per_data = case["A"].shape[1]
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full, _ = device_form(b, case["g"], per_data)
    counts = np.tile(pk.dims.astype(np.int32), (pk.batch, 1))
    counts[1] = [12, 7, 12, 0, 12]
    counts[5] = [3, 12, 5, 12, 12]
    b.set_instance_obj_dims(torch.from_numpy(counts).cuda())
    r = b.run_device(data, var_index=var)
    active = r["active"].cpu().numpy()
    got, flags = device_form(b, case["g"], per_data)
    first = np.concatenate([[0], np.cumsum(pk.dims)]).astype(int)
    for i in range(pk.batch):
        _, nonzero = XC.split(case, got[i])
        assert not nonzero[active[i] == 0].any(), i
        if i in (1, 5):
            for k in range(len(pk.dims)):
                assert not nonzero[first[k] + counts[i, k]:first[k + 1]].any(), (i, k)
            assert not flags[i] or nonzero.any()
        else:
            np.testing.assert_array_equal(got[i], full[i])
    b.set_instance_obj_dims(None)
    b.close()


def test_error_rules(hip):
    """each refusal comes with the outputs left alone"""
    from lexls_amd import capi, lexlsi
    case = XC.build("ik")
    n, per_data = case["n"], case["A"].shape[1]
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib = capi.lib()
    g = np.array(case["g"])
    out, flags = np.full((pk.batch, per_data), SENTINEL), np.full(pk.batch, FLAG_SENTINEL, np.uint8)
    d_g = torch.from_numpy(g).cuda()
    d_out = torch.full((pk.batch, per_data), SENTINEL, dtype=torch.float64, device="cuda")
    d_flags = torch.full((pk.batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    host = lambda g_, o_, f_: lib.lexls_lsi_batch_solve_adjoint_matrix(b._h, g_, o_, f_)  # noqa: E731
    device = lambda g_, o_, f_: lib.lexls_lsi_batch_solve_adjoint_matrix_device(b._h, g_, o_, f_)  # noqa: E731
    hp = (g.ctypes.data_as(DP), out.ctypes.data_as(DP), flags.ctypes.data_as(BP))
    dp = (C.c_void_p(d_g.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(d_flags.data_ptr()))

    def untouched():
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and (flags == FLAG_SENTINEL).all() and bool((d_out == SENTINEL).all()) and bool((d_flags == FLAG_SENTINEL).all())

    def both(code, needle):
        assert host(*hp) == code and needle in lib.lexls_last_error(), lib.lexls_last_error()
        assert device(*dp) == code and needle in lib.lexls_last_error(), lib.lexls_last_error()
        untouched()

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
    assert host(None, hp[1], hp[2]) == INVALID and b"null g" in lib.lexls_last_error()
    assert host(hp[0], None, hp[2]) == INVALID and b"null grad_data" in lib.lexls_last_error()
    assert device(None, dp[1], dp[2]) == INVALID and b"null g" in lib.lexls_last_error()
    assert device(dp[0], None, dp[2]) == INVALID and b"null grad_data" in lib.lexls_last_error()
    untouched()
    # and the plain run behind them is served: the sentinels go, the two forms agree
    assert host(*hp) == 0 and device(*dp) == 0
    torch.cuda.synchronize()
    assert_reference(case, out, flags, "ik, behind the refusals")
    np.testing.assert_array_equal(d_out.cpu().numpy(), out), np.testing.assert_array_equal(d_flags.cpu().numpy(), flags)
    b.close()


def collect():
    """the ik batch plain and under a mask, mixed, and budget (stopped instances in the groups' last positions) -> {name: array}, in whatever
    number of groups this process's environment asks for"""
    from lexls_amd import lexlsi
    out = {}
    for name, mask in (("ik", None), ("ik", [1, 0, 1, 1, 0, 0, 0, 0]), ("mixed", None), ("budget", None)):
        case = XC.build(name)
        pk = lexlsi.pack_batch(case["n"], case["probs"])
        data, var = upload(pk)
        b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
        b.set_instance_mask(None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).cuda())
        b.run_device(data, var_index=var, **case["params"])
        key = name + ("_mask" if mask else "")
        out[f"{key}.groups"] = np.asarray(b.stats()["groups"])
        out[f"{key}.device"], out[f"{key}.device_flags"] = device_form(b, case["g"], case["A"].shape[1])
        out[f"{key}.host"], out[f"{key}.host_flags"] = host_form(b, case["g"], case["A"].shape[1])
        b.set_instance_mask(None)
        b.close()
    return out


def child_collect(path):
    np.savez(path, **collect())


@pytest.mark.parametrize("groups", [2, 3])
def test_a_batch_split_into_groups_has_the_bits_of_the_one_group_run(hip, monkeypatch, tmp_path, groups):
    """LEXLS_LSI_GROUPS is read when a batch is created: the split run is a child process under a time limit of its own"""
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    ref = collect()
    assert int(ref["ik.groups"]) == 1
    assert_reference(XC.build("ik"), ref["ik.device"], ref["ik.device_flags"], "ik, one group")
    assert_reference(XC.build("mixed"), ref["mixed.host"], ref["mixed.host_flags"], "mixed, one group")
    path = str(tmp_path / "groups.npz")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_adjoint_matrix as m; m.child_collect({path!r})"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{GROUPS_SWITCH: str(groups)}), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    assert set(got) == set(ref)
    for k in ref:
        if k.endswith(".groups"):
            assert int(got[k]) == groups, (k, int(got[k]))
        else:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{groups} groups: {k}")


def test_solve_data_autograd(hip):
    """torch.autograd.grad of <g, x> through solve_data is solve_adjoint_matrix_device's output bit for bit; a second backward after an
    intervening run repeats the forward"""
    from lexls_amd import lexlsi
    from lexls_amd.torch_adjoint import SolveBounds, solve_data
    case = XC.build("mixed")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g = torch.from_numpy(case["g"].copy()).cuda()
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    leaf = data.clone().requires_grad_(True)
    out = {}
    x = solve_data(b, leaf, var_index=var, out=out)
    np.testing.assert_array_equal(out["active"].cpu().numpy(), case["active"])
    (grad,) = torch.autograd.grad((g * x).sum(), leaf, retain_graph=True)
    flags = b.differentiable.cpu().numpy()
    direct, dflags = b.solve_adjoint_matrix_device(g)
    assert torch.equal(grad, direct) and flags.tolist() == XC.FLAGS["mixed"] == dflags.cpu().numpy().tolist()
    assert_reference(case, grad.cpu().numpy(), flags, "mixed, solve_data")
    # another run in between (other data: instance 0's problems everywhere), then backward again: the forward run is repeated first
    serial = b._run_serial
    b.run_device(data[[0, 0, 0, 0]].contiguous(), var_index=var)
    (grad2,) = torch.autograd.grad((g * x).sum(), leaf)
    assert b._run_serial == serial + 2 and torch.equal(grad2, direct)
    with pytest.raises(ValueError, match="solve_data"):
        SolveBounds.apply(torch.zeros(pk.batch, pk.total, dtype=torch.float64, device="cuda"), torch.zeros(pk.batch, pk.total, dtype=torch.float64, device="cuda"),
                          b, leaf, var, None, None, None, None)
    b.close()
