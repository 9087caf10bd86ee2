"""Re-solving batched LexLSI working sets on new bounds on the device (lexls_lsi_batch_solve_bounds(_device), LsiBatch.solve_bounds,
torch_adjoint.solve_new_bounds) against reference (A) of tests/lsi_bounds_cases.py — the final equality problem re-formed from scratch with the new
bounds, solved by the oracle — within BC.TOL; the violation against numpy's evaluation of the header's definition on the device's own x within the
derived rounding bound (BC.violation_bound); valid and the exact zeros as bits; bit-independence of a bound set from K, position and company;
bit-equality of the forms; the mask, row-count, NaN, sharing and error rules; the gradients of the torch operation.

MEASURED on the device (the figures the assertions print): x against (A) at most 6.4e-15 (ik; 1.3e-15 or less on the other cases) under
TOL = 6e-14; the violation at most 0.61 of its derived bound (rank_def, K = 64)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_cases as LC
import lsi_bounds_cases as BC
from test_gpu_lsi_adjoint import solve, upload

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
SENTINEL, FLAG_SENTINEL = 7.25, 9
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS_SWITCH = "LEXLS_LSI_GROUPS"
# the bound sets of a call with K sets (indices into the case's K_ALL): set 5 is first of two and fifth of 65, the large set (K_ALL - 1) second of two
# and last of 65, in the second tile of 64
SETS = {1: [0], 2: [5, BC.K_ALL - 1], 64: list(range(64)), 65: list(range(1, BC.K_ALL))}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bounds_of(case, sets):
    return np.ascontiguousarray(case["lb"][sets]), np.ascontiguousarray(case["ub"][sets])


def host_form(b, lb, ub, with_optional=True):
    """the C call itself into outputs that hold sentinels -> (x, violation, valid)"""
    from lexls_amd import capi
    K, batch = lb.shape[:2]
    x, viol, valid = np.full((K, batch, b.nvar), SENTINEL), np.full((K, batch), SENTINEL), np.full(batch, FLAG_SENTINEL, np.uint8)
    capi.check(capi.lib().lexls_lsi_batch_solve_bounds(b._h, lb.ctypes.data_as(DP), ub.ctypes.data_as(DP), K, x.ctypes.data_as(DP),
                                                       viol.ctypes.data_as(DP) if with_optional else None, valid.ctypes.data_as(BP) if with_optional else None))
    return x, viol, valid


def device_form(b, lb, ub):
    K, batch = lb.shape[:2]
    x = torch.full((K, batch, b.nvar), SENTINEL, dtype=torch.float64, device="cuda")
    viol = torch.full((K, batch), SENTINEL, dtype=torch.float64, device="cuda")
    valid = torch.full((batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    b.solve_bounds_device(torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda(), x, viol, valid)
    return x.cpu().numpy(), viol.cpu().numpy(), valid.cpu().numpy()


def assert_reference(case, sets, x, viol, valid, what, counts=None, instances=None):
    """valid, x within TOL of (A), the violation within the derived bound of numpy's on the device's own x, exact zeros as bits"""
    n, status = case["n"], case["status"]
    lb, ub = bounds_of(case, sets)
    gap = vgap = 0.0
    for i in (range(len(status)) if instances is None else instances):
        assert valid[i] == (1 if status[i] == BC.SOLVED else 0), (what, i)
        if status[i] != BC.SOLVED or not case["active"][i].any():
            assert not bits(x[:, i]).any(), (what, i)  # stopped by its budget, or an empty working set: exact zeros
        if status[i] != BC.SOLVED:
            assert not bits(viol[:, i]).any(), (what, i)
            continue
        for c, s in enumerate(sets):
            if counts is None:
                ref = case["A"][s, i]
                gap = max(gap, float(np.abs(x[c, i] - ref).max()) / max(1.0, float(np.abs(ref).max())))
            objs = LC.with_bounds(case["probs"][i], lb[c, i], ub[c, i])
            cnt = None if counts is None else counts[i]
            want, bound = BC.violation_of(n, objs, x[c, i], cnt), BC.violation_bound(n, objs, x[c, i], cnt)
            vgap = max(vgap, abs(viol[c, i] - want) / bound)
            assert abs(viol[c, i] - want) <= bound, (what, i, s, viol[c, i], want, bound)
    print(f"{what}: K {len(sets)}  x against (A) {gap:.2e} (TOL {BC.TOL:.1e})  violation against numpy {vgap:.2f} of its bound")
    assert gap <= BC.TOL, what
    assert not (x == SENTINEL).any() and not (viol == SENTINEL).any(), what


@pytest.mark.parametrize("name", BC.CASES)
def test_cases_against_reference_a_every_k_both_forms(hip, name):
    case = BC.build(name)
    b, x_run, active, _, status = solve("run", case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"])  # the run is the oracle's
    np.testing.assert_array_equal(status, case["status"])
    out = {}
    for K, sets in SETS.items():
        lb, ub = bounds_of(case, sets)
        out[K] = host_form(b, lb, ub)
        assert_reference(case, sets, *out[K], f"{name}, host form")
        assert b.last_consumer_kernel() == ("lsi_bounds_check<lds>" if case["n"] <= 46 else "lsi_bounds_check<hbm>")
        dev = device_form(b, lb, ub)
        for a, a0 in zip(dev, out[K]):  # the two forms: the same bits
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(a0) if a0.dtype == np.float64 else a0)
    # the run's own bounds give the run's x (K = 1: set 0)
    for i in np.flatnonzero(status == BC.SOLVED):
        assert float(np.abs(out[1][0][0, i] - x_run[i]).max()) / max(1.0, float(np.abs(x_run[i]).max())) <= BC.TOL, (name, i)
    # a bound set does not depend on K, on its position or on its company, bit for bit
    for s in SETS[2]:
        np.testing.assert_array_equal(bits(out[2][0][SETS[2].index(s)]), bits(out[65][0][SETS[65].index(s)]), err_msg=f"x of set {s}")
        np.testing.assert_array_equal(bits(out[2][1][SETS[2].index(s)]), bits(out[65][1][SETS[65].index(s)]), err_msg=f"violation of set {s}")
    for s in range(1, 64):
        np.testing.assert_array_equal(bits(out[64][0][s]), bits(out[65][0][s - 1]))
        np.testing.assert_array_equal(bits(out[64][1][s]), bits(out[65][1][s - 1]))
    # again, and without the optional outputs: the same bits; the Python form of a single set without the leading axis
    lb, ub = bounds_of(case, SETS[65])
    again = host_form(b, lb, ub, with_optional=False)
    np.testing.assert_array_equal(bits(again[0]), bits(out[65][0]))
    assert (again[1] == SENTINEL).all() and (again[2] == FLAG_SENTINEL).all()
    one = b.solve_bounds(case["lb"][0], case["ub"][0])
    assert one[0].shape == (len(status), case["n"]) and one[1].shape == (len(status),)
    np.testing.assert_array_equal(bits(one[0]), bits(out[1][0][0])), np.testing.assert_array_equal(bits(one[1]), bits(out[1][1][0]))
    b.close()


@pytest.mark.parametrize("entry", ["run_device", "enqueue"])
@pytest.mark.parametrize("name", ["sb3", "budget", "empty_ws"])
def test_the_device_entries(hip, entry, name):
    case = BC.build(name)
    b, _, active, _, status = solve(entry, case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"]), np.testing.assert_array_equal(status, case["status"])
    sets = SETS[2]
    assert_reference(case, sets, *device_form(b, *bounds_of(case, sets)), f"{name}, {entry}")
    b.close()


def test_sharing_the_final_factor(hip):
    """behind get_lambda or solve_adjoint nothing is factorized; in front of them it is factorized once; the multipliers answer as before"""
    from lexls_amd import lexlsi
    case = BC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    g = LC.build("ik")["g"]
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    lb, ub = bounds_of(case, SETS[2])
    results = []
    for order in ("lam,bnd,lam", "adj,bnd,bnd,adj", "bnd,lam,adj"):
        r = b.run_device(data, var_index=var)
        keep = {k: v.clone() for k, v in r.items()}
        groups, count0, out = b.stats()["groups"], b.final_factorizations(), {}
        for step in order.split(","):
            val = (b.lambda_array(),) if step == "lam" else b.solve_adjoint(g) if step == "adj" else device_form(b, lb, ub)
            for a, a0 in zip(val, out.get(step, val)):
                np.testing.assert_array_equal(a, a0, err_msg=f"{order}: {step} twice")
            out[step] = val
            assert b.final_factorizations() == count0 + groups, (order, step)
        for k, v in r.items():
            assert torch.equal(v, keep[k]), (order, k)
        results.append(out)
    for out in results[1:]:
        for k, val in out.items():
            for a, a0 in zip(val, next(o[k] for o in results if k in o)):
                np.testing.assert_array_equal(a, a0, err_msg=k)
    assert_reference(case, SETS[2], *results[0]["bnd"], "ik, call orders")
    b.close()


def test_instance_mask(hip):
    """skipped instances keep their sentinels in all three outputs, in both forms; the others carry the bits of the unmasked call"""
    from lexls_amd import lexlsi
    case = BC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    lb, ub = bounds_of(case, SETS[2])
    full = device_form(b, lb, ub)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    for form in (device_form, host_form):
        x, viol, valid = form(b, lb, ub)
        assert (x[:, mask == 0] == SENTINEL).all() and (viol[:, mask == 0] == SENTINEL).all() and (valid[mask == 0] == FLAG_SENTINEL).all(), form.__name__
        np.testing.assert_array_equal(bits(x[:, mask == 1]), bits(full[0][:, mask == 1]))
        np.testing.assert_array_equal(bits(viol[:, mask == 1]), bits(full[1][:, mask == 1]))
        np.testing.assert_array_equal(valid[mask == 1], full[2][mask == 1])
    b.set_instance_mask(None)
    b.close()


def test_instance_obj_dims(hip):
    """NaN in the absent rows of lb / ub reaches nothing; the violation is taken over the present rows; an instance with its full counts carries
    the bits of the plain run"""
    from lexls_amd import lexlsi
    case = BC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    sets = SETS[2]
    lb, ub = bounds_of(case, sets)
    full = device_form(b, lb, ub)
    counts = np.tile(pk.dims.astype(np.int32), (pk.batch, 1))
    counts[1] = [12, 7, 12, 0, 12]
    counts[5] = [3, 12, 5, 12, 12]
    b.set_instance_obj_dims(torch.from_numpy(counts).cuda())
    r = b.run_device(data, var_index=var)
    assert (r["info"].cpu().numpy()[:, 0] == BC.SOLVED).all()
    got = device_form(b, lb, ub)
    first = np.concatenate([[0], np.cumsum(pk.dims)]).astype(int)
    lbn, ubn = lb.copy(), ub.copy()
    for i in (1, 5):
        for k in range(len(pk.dims)):
            lbn[:, i, first[k] + counts[i, k]:first[k + 1]] = np.nan
            ubn[:, i, first[k] + counts[i, k]:first[k + 1]] = np.nan
    nan = device_form(b, lbn, ubn)
    for a, a0 in zip(nan, got):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(a0) if a0.dtype == np.float64 else a0)
    for i in range(pk.batch):
        if i not in (1, 5):
            np.testing.assert_array_equal(bits(got[0][:, i]), bits(full[0][:, i])), np.testing.assert_array_equal(bits(got[1][:, i]), bits(full[1][:, i]))
    assert_reference(case, sets, *got, "ik, row counts", counts=counts, instances=(1, 5))  # (the violation alone: (A) knows the full instances)
    b.set_instance_obj_dims(None)
    b.close()


def test_error_rules(hip):
    """each refusal comes before any device work, with the outputs left alone"""
    from lexls_amd import capi, lexlsi
    case = BC.build("ik")
    n, K = case["n"], 2
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib = capi.lib()
    lb, ub = bounds_of(case, SETS[2])
    x, viol, valid = np.full((K, pk.batch, n), SENTINEL), np.full((K, pk.batch), SENTINEL), np.full(pk.batch, FLAG_SENTINEL, np.uint8)
    d_lb, d_ub = torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda()
    d_x = torch.full((K, pk.batch, n), SENTINEL, dtype=torch.float64, device="cuda")
    d_viol = torch.full((K, pk.batch), SENTINEL, dtype=torch.float64, device="cuda")
    d_valid = torch.full((pk.batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    host = lambda *a: lib.lexls_lsi_batch_solve_bounds(b._h, *a)  # noqa: E731
    device = lambda *a: lib.lexls_lsi_batch_solve_bounds_device(b._h, *a)  # noqa: E731
    hp = [lb.ctypes.data_as(DP), ub.ctypes.data_as(DP), K, x.ctypes.data_as(DP), viol.ctypes.data_as(DP), valid.ctypes.data_as(BP)]
    dp = [C.c_void_p(d_lb.data_ptr()), C.c_void_p(d_ub.data_ptr()), K, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_viol.data_ptr()), C.c_void_p(d_valid.data_ptr())]

    def untouched():
        torch.cuda.synchronize()
        assert (x == SENTINEL).all() and (viol == SENTINEL).all() and (valid == FLAG_SENTINEL).all()
        assert bool((d_x == SENTINEL).all()) and bool((d_viol == SENTINEL).all()) and bool((d_valid == FLAG_SENTINEL).all())

    def both(code, needle):
        assert host(*hp) == code and needle in lib.lexls_last_error(), lib.lexls_last_error()
        assert device(*dp) == code and needle in lib.lexls_last_error(), lib.lexls_last_error()
        untouched()

    def swapped(args, at, val):
        return [val if j == at else a for j, a in enumerate(args)]

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
    for form, args in ((host, hp), (device, dp)):
        for at, val, needle in ((0, None, b"null lb / ub"), (1, None, b"null lb / ub"), (3, None, b"null x"), (2, 0, b"nrhs == 0"), (2, 65536, b"more than 65535")):
            assert form(*swapped(args, at, val)) == INVALID and needle in lib.lexls_last_error(), (at, lib.lexls_last_error())
    assert lib.lexls_lsi_batch_solve_bounds(None, *hp) == INVALID
    untouched()
    # and the plain run behind them is served: the sentinels go, the two forms agree
    assert host(*hp) == 0 and device(*dp) == 0
    torch.cuda.synchronize()
    assert_reference(case, SETS[2], x, viol, valid, "ik, behind the refusals")
    np.testing.assert_array_equal(bits(d_x.cpu().numpy()), bits(x)), np.testing.assert_array_equal(bits(d_viol.cpu().numpy()), bits(viol))
    np.testing.assert_array_equal(d_valid.cpu().numpy(), valid)
    b.close()


def test_solve_new_bounds_gradients(hip):
    """x is differentiable in lb and ub through one multi-cotangent adjoint call: its bits, and the oracle's M^T g within the adjoint tests'
    tolerance; violation is not differentiable"""
    from lexls_amd import lexlsi
    from lexls_amd.torch_adjoint import solve_new_bounds
    ref = LC.build("small_sb")
    case_lb, case_ub = zip(*(LC.bounds_of(objs) for objs in ref["probs"]))
    pk = lexlsi.pack_batch(ref["n"], ref["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(ref["n"], pk.dims, pk.types, pk.batch)
    r = b.run_device(data, var_index=var)
    np.testing.assert_array_equal(r["active"].cpu().numpy(), ref["active"])
    K = 3
    lb = torch.from_numpy(np.tile(np.stack(case_lb), (K, 1, 1))).cuda().requires_grad_(True)
    ub = torch.from_numpy(np.tile(np.stack(case_ub), (K, 1, 1))).cuda().requires_grad_(True)
    x, viol = solve_new_bounds(b, lb, ub)
    assert x.requires_grad and not viol.requires_grad and b.valid.cpu().numpy().tolist() == [1] * pk.batch
    scale = torch.arange(1, K + 1, dtype=torch.float64, device="cuda")[:, None, None]
    G = scale * torch.from_numpy(np.array(ref["g"])).cuda()[None]  # cotangent c = (c + 1) g
    x.backward(G)
    direct_lb, direct_ub = b.solve_adjoint_multi_device(G.transpose(0, 1).contiguous())
    assert torch.equal(lb.grad, direct_lb.transpose(0, 1)) and torch.equal(ub.grad, direct_ub.transpose(0, 1))
    for c in range(K):
        for got, want in ((lb.grad[c].cpu().numpy(), ref["A"][0]), (ub.grad[c].cpu().numpy(), ref["A"][1])):
            assert float(np.abs(got - (c + 1) * want).max()) / max(1.0, float(np.abs((c + 1) * want).max())) <= LC.TOL, c
    x1, v1 = solve_new_bounds(b, lb[0].detach(), ub[0].detach())  # one set without the leading axis
    assert tuple(x1.shape) == (pk.batch, ref["n"]) and tuple(v1.shape) == (pk.batch,)
    b.close()


def collect():
    """ik plain and under a mask, sb3 and budget -> {name: array}, in whatever number of groups this process's environment asks for"""
    from lexls_amd import lexlsi
    out = {}
    for name, mask in (("ik", None), ("ik", [1, 0, 1, 1, 0, 0, 0, 0]), ("sb3", None), ("budget", None)):
        case = BC.build(name)
        pk = lexlsi.pack_batch(case["n"], case["probs"])
        data, var = upload(pk)
        b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
        b.set_instance_mask(None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).cuda())
        b.run_device(data, var_index=var, **case["params"])
        key = name + ("_mask" if mask else "")
        out[f"{key}.groups"] = np.asarray(b.stats()["groups"])
        lb, ub = bounds_of(case, SETS[65])
        for form in (device_form, host_form):
            for part, a in zip(("x", "violation", "valid"), form(b, lb, ub)):
                out[f"{key}.{form.__name__}.{part}"] = a
        b.set_instance_mask(None)
        b.close()
    return out


def child_collect(path):
    np.savez(path, **collect())


def test_a_batch_split_into_groups_has_the_bits_of_the_one_group_run(hip, monkeypatch, tmp_path):
    """LEXLS_LSI_GROUPS is read when a batch is created: the split run is a child process under a time limit of its own"""
    groups = 2
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    ref = collect()
    assert int(ref["ik.groups"]) == 1
    path = str(tmp_path / "groups.npz")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_solve_bounds as m; m.child_collect({path!r})"
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
