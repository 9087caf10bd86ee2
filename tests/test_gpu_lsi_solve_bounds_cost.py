"""The per-objective cost of new bounds on the final working sets (lexls_lsi_batch_solve_bounds_cost(_device), LsiBatch.solve_bounds(with_cost=True),
lexls_amd/csrc/lsi_final.h: lsi_bounds_check_kernel<placement, true>) on the cases of tests/lsi_bounds_cases.py and one more of their kind, n20 (n = 20, simple bounds
(6) + general (5, 5, 6)): cost against numpy on the device's own x within a computable forward bound; x and violation the bits of
lexls_lsi_batch_solve_bounds_device; violation^2 >= every d_r^2; independence of K, position and company, run-to-run and host = device as bits;
exact zeros for instances stopped by their budget, sentinels kept under the mask, NaN in absent rows unread; the final factor shared; the
refusals; lex_argmin on the device's costs.

The bound.  cost_k = sum_r d_r^2, d_r = max(lb - a.x, a.x - ub, 0).  The device's a.x is an fma chain of nVar terms: |e_r| <= g sum_j |a_rj x_j|, and
the subtraction adds an ulp of the bound, so d_r moves by at most e_r = g sum_j |a_rj x_j| + ulp; d_r^2 by 2 |d_r| e_r + e_r^2; the ordered sum of
rows_k squares by g cost.  With g = (nVar + rows_k) 2^-52:   |delta| <= 4 g sum_r |d_r| sum_j |a_rj x_j| + g cost  +  sum_r e_r^2.
The last term is second order (1e-30 and below here) and is kept because an ACTIVE row sits on its bound to rounding: numpy may see d_r = 0 where
the device sees one ulp, and then the first-order terms of that row are 0 while the costs differ by an ulp squared.

MEASURED on the device (the figures the assertions print): the cost at most 0.07 of its bound (sb3; 0.02 or less on the other cases)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_cases as LC
import lsi_bounds_cases as BC
from test_gpu_lsi_adjoint import solve, upload
from test_gpu_lsi_solve_bounds import FLAG_SENTINEL, SENTINEL, SETS, bits, bounds_of
from test_gpu_lsi_solve_bounds import device_form as plain_device_form

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
BC.OWN.setdefault("n20", dict(n=20, dims=(6, 5, 5, 6), simple=True, batch=4, seed=20350101))  # (not in BC.CASES: the other files do not run it)
CASES = ("n20", "ik", "sb3", "lds46", "hbm47", "budget", "empty_ws")


def host_form(b, lb, ub, with_x=True):
    """the C call itself into outputs that hold sentinels -> (x, violation, valid, cost)"""
    from lexls_amd import capi
    K, batch = lb.shape[:2]
    x, viol, valid = np.full((K, batch, b.nvar), SENTINEL), np.full((K, batch), SENTINEL), np.full(batch, FLAG_SENTINEL, np.uint8)
    cost = np.full((K, batch, len(b.dims)), SENTINEL)
    capi.check(capi.lib().lexls_lsi_batch_solve_bounds_cost(b._h, lb.ctypes.data_as(DP), ub.ctypes.data_as(DP), K, x.ctypes.data_as(DP) if with_x else None,
                                                            viol.ctypes.data_as(DP), cost.ctypes.data_as(DP), valid.ctypes.data_as(BP)))
    return x, viol, valid, cost


def device_form(b, lb, ub):
    K, batch = lb.shape[:2]
    x = torch.full((K, batch, b.nvar), SENTINEL, dtype=torch.float64, device="cuda")
    viol = torch.full((K, batch), SENTINEL, dtype=torch.float64, device="cuda")
    valid = torch.full((batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    cost = torch.full((K, batch, len(b.dims)), SENTINEL, dtype=torch.float64, device="cuda")
    out = b.solve_bounds_device(torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda(), x, viol, valid, cost=cost)
    assert len(out) == 4 and out[3] is cost
    return x.cpu().numpy(), viol.cpu().numpy(), valid.cpu().numpy(), cost.cpu().numpy()


def cost_of(n, objs, x, counts=None):
    """per objective (cost, bound, largest d_r) of the header's definition in numpy for ONE instance and ONE x (a.x in extended precision)"""
    out = []
    for k, o in enumerate(objs):
        m = len(o["lb"]) if counts is None else int(counts[k])
        if "var" in o:
            ax, mag = x[o["var"][:m].astype(int)], np.abs(x[o["var"][:m].astype(int)])
        else:
            ax, mag = BC._fma_rows(o["A"][:m], x), np.abs(o["A"][:m]) @ np.abs(x)
        lb, ub = o["lb"][:m], o["ub"][:m]
        d = np.maximum(np.maximum(lb - ax, ax - ub), 0.0)
        cost, g = float((d * d).sum()), (n + m) * 2.0 ** -52
        e = g * mag + np.maximum(np.spacing(np.abs(lb)), np.spacing(np.abs(ub)))
        out.append((cost, 4 * g * float((d * mag).sum()) + g * cost + float((e * e).sum()), float(d.max()) if m else 0.0))
    return out


def assert_cost(case, sets, x, viol, valid, cost, what, counts=None, instances=None):
    status, n = case["status"], case["n"]
    lb, ub = bounds_of(case, sets)
    worst = 0.0
    for i in (range(len(status)) if instances is None else instances):
        if status[i] != BC.SOLVED:
            assert valid[i] == 0 and not bits(cost[:, i]).any(), (what, i)  # stopped by its budget: exact zeros
            continue
        for c in range(len(sets)):
            objs = LC.with_bounds(case["probs"][i], lb[c, i], ub[c, i])
            for k, (want, bound, dmax) in enumerate(cost_of(n, objs, x[c, i], None if counts is None else counts[i])):
                delta = abs(cost[c, i, k] - want)
                worst = max(worst, delta / bound if bound else 0.0)
                assert delta <= bound, (what, i, sets[c], k, cost[c, i, k], want, bound)
                assert viol[c, i] ** 2 >= dmax * dmax * (1 - 2.0 ** -50) - bound, (what, i, sets[c], k)  # violation^2 >= every d_r^2
    print(f"{what}: K {len(sets)}  cost against numpy on the device's x: {worst:.2f} of its bound")
    assert not (cost == SENTINEL).any(), what


@pytest.mark.parametrize("name", CASES)
def test_cost_every_k_both_forms_and_the_bit_rules(hip, name):
    case = BC.build(name)
    assert case["held"]
    b, _, active, _, status = solve("run", case["probs"], case["n"], **case["params"])
    np.testing.assert_array_equal(active, case["active"])  # the run is the oracle's
    np.testing.assert_array_equal(status, case["status"])
    out = {}
    plain_device_form(b, *bounds_of(case, SETS[1]))  # (the final factor of the run is formed here)
    count0 = b.final_factorizations()
    for K, sets in SETS.items():
        lb, ub = bounds_of(case, sets)
        out[K] = host_form(b, lb, ub)
        assert b.last_consumer_kernel() == ("lsi_bounds_cost<lds>" if case["n"] <= 46 else "lsi_bounds_cost<hbm>")
        assert_cost(case, sets, *out[K], f"{name}, host form")
        for form in (device_form, host_form):  # host = device, and run to run
            for a, a0 in zip(form(b, lb, ub), out[K]):
                np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(a0) if a0.dtype == np.float64 else a0, err_msg=form.__name__)
        plain = plain_device_form(b, lb, ub)  # x, violation and valid are lexls_lsi_batch_solve_bounds_device's
        assert b.last_consumer_kernel().startswith("lsi_bounds_check<")
        for a, a0 in zip(plain, out[K][:3]):
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(a0) if a0.dtype == np.float64 else a0)
        assert b.final_factorizations() == count0  # the final factor is shared: nothing is formed or factorized again
        nox = host_form(b, lb, ub, with_x=False)  # x not wanted
        assert (nox[0] == SENTINEL).all()
        np.testing.assert_array_equal(bits(nox[3]), bits(out[K][3])), np.testing.assert_array_equal(bits(nox[1]), bits(out[K][1]))
    # a bound set's cost does not depend on K, on its position or on its company, bit for bit
    for s in SETS[2]:
        np.testing.assert_array_equal(bits(out[2][3][SETS[2].index(s)]), bits(out[65][3][SETS[65].index(s)]), err_msg=f"cost of set {s}")
    for s in range(1, 64):
        np.testing.assert_array_equal(bits(out[64][3][s]), bits(out[65][3][s - 1]))
    one = b.solve_bounds(case["lb"][0], case["ub"][0], with_cost=True)
    assert len(one) == 4 and one[3].shape == (len(status), len(case["dims"]))
    np.testing.assert_array_equal(bits(one[3]), bits(out[1][3][0]))
    assert len(b.solve_bounds(case["lb"][0], case["ub"][0])) == 3  # the old return shape
    b.close()


def test_instance_mask_and_obj_dims(hip):
    """skipped instances keep their sentinels in all four outputs, in both forms; NaN bounds in absent rows reach nothing, and the cost is taken
    over the present rows"""
    from lexls_amd import lexlsi
    case = BC.build("ik")
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    data, var = upload(pk)
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.run_device(data, var_index=var)
    sets = SETS[2]
    lb, ub = bounds_of(case, sets)
    full = device_form(b, lb, ub)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    b.set_instance_mask(torch.from_numpy(mask).cuda())
    b.run_device(data, var_index=var)
    for form in (device_form, host_form):
        got = form(b, lb, ub)
        assert (got[3][:, mask == 0] == SENTINEL).all() and (got[0][:, mask == 0] == SENTINEL).all() and (got[2][mask == 0] == FLAG_SENTINEL).all(), form.__name__
        np.testing.assert_array_equal(bits(got[3][:, mask == 1]), bits(full[3][:, mask == 1]))
    b.set_instance_mask(None)
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
    for a, a0 in zip(device_form(b, lbn, ubn), got):
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(a0) if a0.dtype == np.float64 else a0)
    assert not bits(got[3][:, 1, 3]).any()  # an objective without rows costs nothing
    for i in range(pk.batch):
        if i not in (1, 5):
            np.testing.assert_array_equal(bits(got[3][:, i]), bits(full[3][:, i]))
    assert_cost(case, sets, *got, "ik, row counts", counts=counts, instances=(1, 5))
    b.set_instance_obj_dims(None)
    b.close()


def test_error_rules(hip):
    """the refusals of lexls_lsi_batch_solve_bounds, a null cost in the place of a null x, each before any device work with the outputs left alone"""
    from lexls_amd import capi, lexlsi
    case = BC.build("ik")
    n, K = case["n"], 2
    pk = lexlsi.pack_batch(n, case["probs"])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    lib = capi.lib()
    lb, ub = bounds_of(case, SETS[2])
    shapes = ((K, pk.batch, n), (K, pk.batch), (K, pk.batch, len(pk.dims)))
    x, viol, cost = (np.full(s, SENTINEL) for s in shapes)
    valid = np.full(pk.batch, FLAG_SENTINEL, np.uint8)
    d_lb, d_ub = torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda()
    d_x, d_viol, d_cost = (torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for s in shapes)
    d_valid = torch.full((pk.batch,), FLAG_SENTINEL, dtype=torch.uint8, device="cuda")
    host = lambda *a: lib.lexls_lsi_batch_solve_bounds_cost(b._h, *a)  # noqa: E731
    device = lambda *a: lib.lexls_lsi_batch_solve_bounds_cost_device(b._h, *a)  # noqa: E731
    hp = [lb.ctypes.data_as(DP), ub.ctypes.data_as(DP), K, x.ctypes.data_as(DP), viol.ctypes.data_as(DP), cost.ctypes.data_as(DP), valid.ctypes.data_as(BP)]
    dp = [C.c_void_p(t.data_ptr()) for t in (d_lb, d_ub)] + [K] + [C.c_void_p(t.data_ptr()) for t in (d_x, d_viol, d_cost, d_valid)]

    def untouched():
        torch.cuda.synchronize()
        assert all((a == SENTINEL).all() for a in (x, viol, cost)) and (valid == FLAG_SENTINEL).all()
        assert all(bool((t == SENTINEL).all()) for t in (d_x, d_viol, d_cost)) and bool((d_valid == FLAG_SENTINEL).all())

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
        for at, val, needle in ((0, None, b"null lb / ub"), (1, None, b"null lb / ub"), (5, None, b"null cost"), (2, 0, b"nrhs == 0"), (2, 65536, b"more than 65535")):
            assert form(*swapped(args, at, val)) == INVALID and needle in lib.lexls_last_error(), (at, lib.lexls_last_error())
    assert lib.lexls_lsi_batch_solve_bounds_cost(None, *hp) == INVALID
    untouched()
    assert host(*hp) == 0 and device(*dp) == 0  # and the plain run behind them is served: the sentinels go, the two forms agree
    torch.cuda.synchronize()
    assert_cost(case, SETS[2], x, viol, valid, cost, "ik, behind the refusals")
    np.testing.assert_array_equal(bits(d_cost.cpu().numpy()), bits(cost))
    b.close()


def test_lex_argmin_picks_the_runs_own_bounds_among_tightened_ones(hip):
    """candidates: the run's own bounds at index 3 among sets that TIGHTEN one active bound of the top objective, each by another amount.  Every
    candidate's region of level 0 lies inside the run's own, so no candidate can do lexicographically better than the run's optimum"""
    from lexls_amd.lexlsi import lex_argmin
    case = BC.build("ik")
    b, _, active, _, status = solve("run", case["probs"], case["n"], **case["params"])
    B, K, own = len(status), 6, 3
    lb, ub = np.repeat(case["lb"][:1], K, axis=0).copy(), np.repeat(case["ub"][:1], K, axis=0).copy()
    dim0, picked = int(case["dims"][0]), []
    for i in range(B):
        rows = np.flatnonzero((case["active"][i, :dim0] == 1) | (case["active"][i, :dim0] == 2))  # CTR_ACTIVE_LB, CTR_ACTIVE_UB
        if status[i] != BC.SOLVED or not rows.size:
            continue
        r, picked = int(rows[0]), picked + [i]
        for c in range(K):
            step = 0.0 if c == own else 0.05 * (c + 1)
            if case["active"][i, r] == 1:  # CTR_ACTIVE_LB: the lower bound moves up (the upper one with it where it would cross)
                lb[c, i, r] += step
                ub[c, i, r] = max(ub[c, i, r], lb[c, i, r])
            else:
                ub[c, i, r] -= step
                lb[c, i, r] = min(lb[c, i, r], ub[c, i, r])
    assert picked
    _, _, valid, cost = b.solve_bounds(lb, ub, with_cost=True)
    best = lex_argmin(cost, 1e-9)
    assert best.shape == (B,) and (best[picked] == own).all(), (picked, best, cost[:, picked[0]])
    d_best = lex_argmin(torch.from_numpy(cost).cuda(), 1e-9)
    np.testing.assert_array_equal(d_best.cpu().numpy(), best)
    # level order before magnitude, on a hand-made array (K = 2, one instance): a little more at level 0 loses to much more at level 1
    made = np.array([[[1.0, 100.0, 0.0]], [[1.5, 0.0, 0.0]]])
    assert lex_argmin(made, 0.1).tolist() == [0] and lex_argmin(torch.from_numpy(made).cuda(), 0.1).tolist() == [0]
    assert lex_argmin(made, 1.0).tolist() == [1]  # (inside the caller's tie window level 0 does not decide)
    b.close()
