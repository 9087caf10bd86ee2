"""Forward-mode tangents of batched LexLSI solutions with respect to the constraint data on the device (lexls_lsi_batch_solve_tangent(_device),
LsiBatch.solve_tangent, torch_adjoint.jvp_data) against reference (A) of tests/tangent_cases.py — the differentiated dense KKT system of the
final equality problem, on the instances of tests/lsi_adjoint_matrix_cases.py — within TC.LSI_TOL: the flags, the exact zeros as bits, the
empty working set, bit-equality between the forms and the orders of calls with the final problems factorized once, the mask, row-count, NaN
and error rules."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_matrix_cases as XC
import tangent_cases as TC
from test_gpu_lsi_adjoint import solve, upload

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SENTINEL, FLAG_SENTINEL = 7.25, 9
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
K = TC.LSI_NTAN
HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS_SWITCH = "LEXLS_LSI_GROUPS"


def host_form(b, ddata, with_flags=True):
    """the C call itself into outputs that hold sentinels -> (dx, flags)"""
    from lexls_amd import capi
    ddata = np.ascontiguousarray(ddata)
    dx, flags = np.full(ddata.shape[:2] + (b.nvar,), SENTINEL), np.full(ddata.shape[1], FLAG_SENTINEL, np.uint8)
    capi.check(capi.lib().lexls_lsi_batch_solve_tangent(b._h, ddata.ctypes.data_as(DP), ddata.shape[0], dx.ctypes.data_as(DP),
                                                        flags.ctypes.data_as(BP) if with_flags else None))
    return dx, flags


def device_form(b, ddata):
    dx = torch.full(tuple(ddata.shape[:2]) + (b.nvar,), SENTINEL, dtype=torch.float64, device="cuda")
    flags = torch.full((ddata.shape[1],), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    b.solve_tangent_device(torch.from_numpy(np.array(ddata)).cuda(), dx, flags)
    return dx.cpu().numpy(), flags.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_reference(t, got, flags, what):
    """the flags of (A), (A) within LSI_TOL, exact zeros as bits for flag-0 and stopped instances and for empty working sets"""
    case = t["case"]
    np.testing.assert_array_equal(flags, t["flags"], err_msg=what)
    assert flags.tolist() == XC.FLAGS[case["name"]], what
    ref = t["A"][:got.shape[0]]
    gap = max(float(np.abs(got[c, i] - ref[c, i]).max()) / max(1.0, float(np.abs(ref[c, i]).max())) for c in range(ref.shape[0]) for i in range(ref.shape[1]))
    print(f"{what}: gap to (A) {gap:.2e} (TOL {TC.LSI_TOL:.1e})")
    assert gap <= TC.LSI_TOL, what
    for i in range(len(flags)):
        if not flags[i] or case["status"][i] != XC.SOLVED or not case["active"][i].any():
            assert not bits(got[:, i]).any(), (what, i)
    assert not (got == SENTINEL).any(), what


@pytest.mark.parametrize("name", XC.CASES)
def test_cases_against_reference_a_both_forms(hip, name):
    t = TC.lsi_build(name, K, False)
    case = t["case"]
    b, x, active, v, status = solve("run", case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"])  # the run is the oracle's
    np.testing.assert_array_equal(status, case["status"])
    assert b.per_data == t["ddata"].shape[2]
    got, flags = host_form(b, t["ddata"])
    assert_reference(t, got, flags, f"{name}, host form")
    dev, dflags = device_form(b, t["ddata"])
    np.testing.assert_array_equal(bits(dev), bits(got)), np.testing.assert_array_equal(dflags, flags)  # the two forms: the same bits
    again, _ = host_form(b, t["ddata"], with_flags=False)  # the flags are optional
    np.testing.assert_array_equal(bits(again), bits(got))
    one, oflags = b.solve_tangent(t["ddata"][0])  # a single direction without the leading axis
    assert one.shape == (len(flags), case["n"])
    np.testing.assert_array_equal(oflags, flags)
    assert max(float(np.abs(one[i] - t["A"][0, i]).max()) / max(1.0, float(np.abs(t["A"][0, i]).max())) for i in range(len(flags))) <= TC.LSI_TOL
    if name == "empty_ws":  # an empty working set is differentiable with dx = 0
        assert flags[1] == 1 and flags[3] == 1 and not bits(got[:, [1, 3]]).any()
    # NaN in the rows outside the working set changes nothing
    dd = t["ddata"].copy()
    for i in range(len(flags)):
        dd[:, i, TC.inactive_entries(case, i)] = np.nan
    nan_dx, nan_flags = device_form(b, dd)
    np.testing.assert_array_equal(bits(nan_dx), bits(got)), np.testing.assert_array_equal(nan_flags, flags)
    # forward and reverse mode of the device are transposes: <g, dx> == <grad_data(g), ddata>
    grad, gflags = b.solve_adjoint_matrix(case["g"])
    np.testing.assert_array_equal(gflags, flags)
    for i in np.flatnonzero(flags):
        for c in range(K):
            act = ~TC.inactive_entries(case, i)
            terms = np.concatenate([case["g"][i] * got[c, i], -grad[i][act] * t["ddata"][c, i][act]])
            assert abs(terms.sum()) / max(1.0, float(np.abs(terms).sum())) <= TC.LSI_TOL, (name, i, c)
    b.close()


@pytest.mark.parametrize("entry", ["run", "run_device", "enqueue"])
@pytest.mark.parametrize("name", ["mixed", "budget", "small_sb"])
def test_flags_and_values_on_every_entry(hip, entry, name):
    t = TC.lsi_build(name, K, False)
    case = t["case"]
    b, _, active, _, status = solve(entry, case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"]), np.testing.assert_array_equal(status, case["status"])
    got, flags = device_form(b, t["ddata"])
    assert_reference(t, got, flags, f"{name}, {entry}")
    b.close()


def test_call_orders_share_one_factorization_and_change_nothing(hip):
    """the tangent before, between and after lambdas, solve_adjoint and solve_adjoint_matrix: every output bit-equal across the orders, x / active /
    v untouched, the final problems factorized once per run"""
    from lexls_amd import lexlsi
    t = TC.lsi_build("ik", K, False)
    case = t["case"]
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g = case["g"]
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    results = []
    for order in ("tan,lam,mat,adj", "lam,tan,tan", "mat,tan,lam", "adj,tan,mat", "tan,mat"):
        r = b.run_device(data, var_index=var)
        groups = b.stats()["groups"]
        keep = {k: v.clone() for k, v in r.items()}
        count0 = b.final_factorizations()
        out = {}
        for step in order.split(","):
            if step == "lam":
                val = (b.lambda_array(),)
            elif step == "adj":
                val = b.solve_adjoint(g)
            elif step == "mat":
                val = b.solve_adjoint_matrix(g)
            else:
                val = device_form(b, t["ddata"])
            if step in out:
                for a, a0 in zip(val, out[step]):
                    np.testing.assert_array_equal(a, a0, err_msg=f"{order}: {step} twice")
            out[step] = val
            assert b.final_factorizations() == count0 + groups, (order, step)  # once, at the first call behind the run
        for k, v in r.items():
            assert torch.equal(v, keep[k]), (order, k)
        results.append(out)
    assert_reference(t, *results[0]["tan"], "ik, call orders")
    for out in results[1:]:
        for k, val in out.items():
            ref = next(o[k] for o in results if k in o)
            for a, a0 in zip(val, ref):
                np.testing.assert_array_equal(a, a0, err_msg=k)
    b.close()


def test_instance_mask(hip):
    """skipped instances keep their sentinels in rows and flag, in both forms; the others carry the bits of the unmasked call"""
    from lexls_amd import lexlsi
    t = TC.lsi_build("ik", K, False)
    case = t["case"]
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full, full_flags = device_form(b, t["ddata"])
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    for form in (device_form, host_form):
        got, flags = form(b, t["ddata"])
        assert (got[:, mask == 0] == SENTINEL).all() and (flags[mask == 0] == FLAG_SENTINEL).all(), form.__name__
        np.testing.assert_array_equal(bits(got[:, mask == 1]), bits(full[:, mask == 1]))
        np.testing.assert_array_equal(flags[mask == 1], full_flags[mask == 1])
    b.set_instance_mask(None)
    b.close()


def test_instance_obj_dims(hip):
    """rows that are absent under set_instance_obj_dims are never read (NaN there changes nothing); an instance with its full counts carries
    the bits of the plain run"""
    from lexls_amd import lexlsi
    t = TC.lsi_build("ik", K, False)
    case = t["case"]
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    full, _ = device_form(b, t["ddata"])
    counts = np.tile(pk.dims.astype(np.int32), (pk.batch, 1))
    counts[1] = [12, 7, 12, 0, 12]
    counts[5] = [3, 12, 5, 12, 12]
    b.set_instance_obj_dims(torch.from_numpy(counts).cuda())
    r = b.run_device(data, var_index=var)
    active = r["active"].cpu().numpy()
    got, flags = device_form(b, t["ddata"])
    first = np.concatenate([[0], np.cumsum(pk.dims)]).astype(int)
    for i in range(pk.batch):
        if i in (1, 5):
            for k in range(len(pk.dims)):
                assert not active[i, first[k] + counts[i, k]:first[k + 1]].any(), (i, k)  # an absent row is never in the working set
        else:
            np.testing.assert_array_equal(bits(got[:, i]), bits(full[:, i]))
    dd = t["ddata"].copy()
    lay, _ = XC.layout(case["n"], case["probs"][0])
    for i in (1, 5):
        for k, (off, dm, w) in enumerate(lay):
            for j in range(w):
                dd[:, i, off + j * dm + counts[i, k]:off + (j + 1) * dm] = np.nan
    nan_dx, nan_flags = device_form(b, dd)
    np.testing.assert_array_equal(bits(nan_dx), bits(got)), np.testing.assert_array_equal(nan_flags, flags)
    b.set_instance_obj_dims(None)
    b.close()


def test_error_rules(hip):
    """each refusal comes with the outputs left alone"""
    from lexls_amd import capi, lexlsi
    t = TC.lsi_build("ik", K, False)
    case = t["case"]
    n = case["n"]
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib = capi.lib()
    dd = np.array(t["ddata"])
    out, flags = np.full((K, pk.batch, n), SENTINEL), np.full(pk.batch, FLAG_SENTINEL, np.uint8)
    d_dd = torch.from_numpy(dd).cuda()
    d_out = torch.full((K, pk.batch, n), SENTINEL, dtype=torch.float64, device="cuda")
    d_flags = torch.full((pk.batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    host = lambda i_, k_, o_, f_: lib.lexls_lsi_batch_solve_tangent(b._h, i_, k_, o_, f_)  # noqa: E731
    device = lambda i_, k_, o_, f_: lib.lexls_lsi_batch_solve_tangent_device(b._h, i_, k_, o_, f_)  # noqa: E731
    hp = (dd.ctypes.data_as(DP), K, out.ctypes.data_as(DP), flags.ctypes.data_as(BP))
    dp = (C.c_void_p(d_dd.data_ptr()), K, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_flags.data_ptr()))

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
    assert host(None, K, hp[2], hp[3]) == INVALID and b"null ddata" in lib.lexls_last_error()
    assert host(hp[0], K, None, hp[3]) == INVALID and b"null dx" in lib.lexls_last_error()
    assert host(hp[0], 0, hp[2], hp[3]) == INVALID and b"ntan == 0" in lib.lexls_last_error()
    assert device(None, K, dp[2], dp[3]) == INVALID and b"null ddata" in lib.lexls_last_error()
    assert device(dp[0], K, None, dp[3]) == INVALID and b"null dx" in lib.lexls_last_error()
    assert device(dp[0], 0, dp[2], dp[3]) == INVALID and b"ntan == 0" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_tangent(None, hp[0], K, hp[2], hp[3]) == INVALID
    untouched()
    # and the plain run behind them is served: the sentinels go, the two forms agree
    assert host(*hp) == 0 and device(*dp) == 0
    torch.cuda.synchronize()
    assert_reference(t, out, flags, "ik, behind the refusals")
    np.testing.assert_array_equal(bits(d_out.cpu().numpy()), bits(out)), np.testing.assert_array_equal(d_flags.cpu().numpy(), flags)
    b.close()


def test_jvp_data_is_solve_tangent_device(hip):
    from lexls_amd import lexlsi
    from lexls_amd.torch_adjoint import jvp_data
    t = TC.lsi_build("mixed", K, False)
    case = t["case"]
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    d_dd = torch.from_numpy(np.array(t["ddata"])).cuda()
    out = {}
    x, dx = jvp_data(b, data, d_dd, var_index=var, out=out)
    np.testing.assert_array_equal(out["active"].cpu().numpy(), case["active"])
    assert b.differentiable.cpu().numpy().tolist() == XC.FLAGS["mixed"]
    direct, dflags = b.solve_tangent_device(d_dd)
    assert torch.equal(dx, direct) and torch.equal(dflags, b.differentiable)
    assert_reference(t, dx.cpu().numpy(), dflags.cpu().numpy(), "mixed, jvp_data")
    x1, dx1 = jvp_data(b, data, d_dd[0], var_index=var)  # one direction without the leading axis
    assert tuple(dx1.shape) == (pk.batch, case["n"]) and torch.equal(x1, x)
    np.testing.assert_array_equal(bits(dx1.cpu().numpy()), bits(b.solve_tangent_device(d_dd[:1])[0][0].cpu().numpy()))
    b.close()


def collect():
    """the ik batch plain and under a mask, mixed, and budget -> {name: array}, in whatever number of groups this process's environment asks for"""
    from lexls_amd import lexlsi
    out = {}
    for name, mask in (("ik", None), ("ik", [1, 0, 1, 1, 0, 0, 0, 0]), ("mixed", None), ("budget", None)):
        t = TC.lsi_build(name, K, False)
        case = t["case"]
        pk = lexlsi.pack_batch(case["n"], case["probs"])
        data, var = upload(pk)
        b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
        b.set_instance_mask(None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).cuda())
        b.run_device(data, var_index=var, **case["params"])
        key = name + ("_mask" if mask else "")
        out[f"{key}.groups"] = np.asarray(b.stats()["groups"])
        out[f"{key}.device"], out[f"{key}.device_flags"] = device_form(b, t["ddata"])
        out[f"{key}.host"], out[f"{key}.host_flags"] = host_form(b, t["ddata"])
        b.set_instance_mask(None)
        b.close()
    return out


def child_collect(path):
    np.savez(path, **collect())


def test_a_batch_split_into_groups_has_the_bits_of_the_one_group_run(hip, monkeypatch, tmp_path):
    """LEXLS_LSI_GROUPS is read when a batch is created: the split run is a child process under a time limit of its own"""
    groups = 3
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    ref = collect()
    assert int(ref["ik.groups"]) == 1
    assert_reference(TC.lsi_build("ik", K, False), ref["ik.device"], ref["ik.device_flags"], "ik, one group")
    path = str(tmp_path / "groups.npz")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_tangent as m; m.child_collect({path!r})"
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
