"""lexls_lse_residual_rhs* on the device — get_v() and the cost per level for K new right-hand sides and fixed values on a kept factor
(lexls_amd/csrc/lse_adjoint.hip: solve_rhs_front_kernel + residual_rhs_kernel) — against the oracle solving [A | b_new] from scratch (its get_v)
and, independently, against A x - b on the original data with the x of the same call.  Tolerance: SC.TOL, the one tests/test_gpu_lse_solve_rhs.py
holds x to (derived in tests/solve_rhs_cases.py on the CPU), relative to max(1, |b|_inf, |A|_inf |x|_inf) of the problem and right-hand side: v
inherits x's error through A.  cost against numpy's sum of squares of the returned v within 2 cap 2^-52 relative, the forward bound of an ordered
sum.  Shapes: the case generators and the producer list of that file; K = 1, 2, 64 (a full tile), 65 (a second tile).

MEASURED on the device (the figures the assertions print): v against the oracle's get_v at most 3.3e-16 of the scale, under TOL = 2.4e-12."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
import adjoint_reg_cases as RC
import solve_rhs_cases as SC
from lexls_amd import capi, problems as P
from test_gpu_lse_adjoint_matrix import observable_state
from test_gpu_lse_adjoint_reg import handle

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
KS = (1, 2, 64, 65)
K = 65
_dp = C.POINTER(C.c_double)
# n8: n = 8, (3, 3, 4), a rank-deficient middle level, two fixed variables; ik: the project's shape (ranks 12, 12, 12, 4, 0); ragged: per-problem
# dimensions with empty levels; fixed: a problem with EVERY variable fixed among them; rank_def: a level of rank 0
NAMES = ("n8", "ik", "ragged", "fixed", "rank_def")
POLICIES = {"n8": AC.SMALL_FIXED, "ik": AC.PRODUCERS["ik"], "ragged": AC.SMALL, "fixed": AC.SMALL_FIXED, "rank_def": AC.SMALL}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def draw(name):
    if name != "n8":
        return SC.draw(name)
    n, caps, B, seed = 8, [3, 3, 4], 3, 20340101
    lod = np.stack([P.rank_deficient_problem(seed + b, n, caps, [3, 1, 4]) for b in range(B)])
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b, pair in enumerate([[5, 2], [0, 7], [3, 1]]):
        idx[b, :2], val[b, :2] = pair, P.normal(seed + 500 + b, n)[:2]
    case = dict(name=name, n=n, caps=caps, lod=lod, dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), large=False,
                fixed=dict(nfixed=np.full(B, 2, np.uint32), fixed_idx=idx, fixed_val=val), g=P.normal(seed + 900, B * n).reshape(B, n))
    case["factors"] = RC.factors(B, len(caps))
    case["rhs"] = P.normal(seed + 1, K * B * sum(caps)).reshape(K, B, sum(caps))
    case["fixed_new"] = P.normal(seed + 2, K * B * n).reshape(K, B, n)
    case["nf"] = case["fixed"]["nfixed"]
    return case


@functools.lru_cache(maxsize=None)
def build(name):
    """the case, and per (right-hand side, problem) the oracle's run from scratch: v, x (K, batch, .), rank (batch, nObj: A's alone), and the scale
    max(1, |b|_inf, |A|_inf |x|_inf) the tolerance is relative to.  Computed once, shared, read-only"""
    case = draw(name)
    B, n = case["lod"].shape[0], case["n"]
    runs = [RC._run_one(case, b, 0, np.ascontiguousarray(case["rhs"][:, b]), np.ascontiguousarray(case["fixed_new"][:, b])) for b in range(B)]
    case["v"] = np.stack([r["v"] for r in runs], axis=1)
    case["x"] = np.stack([r["x"] for r in runs], axis=1)
    case["rank"] = np.stack([r["rank"][0] for r in runs])
    for b in range(B):
        assert (runs[b]["rank"] == runs[b]["rank"][0]).all()  # pivots and ranks come from A alone
    m = case["dims"].sum(axis=1)
    scale = np.ones((K, B))
    for b in range(B):
        A = case["lod"][b, :n, :m[b]].T
        a_inf = float(np.abs(A).sum(axis=1).max()) if m[b] else 0.0
        for c in range(K):
            scale[c, b] = max(1.0, float(np.abs(case["rhs"][c, b, :m[b]]).max()) if m[b] else 0.0, a_inf * float(np.abs(case["x"][c, b]).max()))
    case["scale"], case["m"] = scale, m
    for arr in (case["lod"], case["dims"], case["rhs"], case["fixed_new"], case["v"], case["x"], case["rank"], scale, *case["fixed"].values()):
        arr.setflags(write=False)
    return case


def plain_variant(case):
    return SC.plain_variant(case["n"], sum(case["caps"])).replace("solve_rhs", "residual_rhs")


def device_form(s, rhs, fixed, want=("x", "v", "cost")):
    d_rhs = torch.from_numpy(np.array(rhs, np.float64)).cuda()
    d_fixed = None if fixed is None else torch.from_numpy(np.array(fixed, np.float64)).cuda()
    lead = tuple(rhs.shape[:-1])
    out = {"x": torch.full(lead + (s.nVar,), 7.0, dtype=torch.float64, device="cuda"), "v": torch.full(lead + (s.cap,), 7.0, dtype=torch.float64, device="cuda"),
           "cost": torch.full(lead + (s.nObj,), 7.0, dtype=torch.float64, device="cuda")}
    s.residual_rhs_device(d_rhs, fixed=d_fixed, **{k: (out[k] if k in want else None) for k in out})
    s.synchronize()
    return {k: out[k].cpu().numpy() for k in out}


def solve_rhs_device(s, rhs, fixed):
    d_x = torch.full(tuple(rhs.shape[:-1]) + (s.nVar,), 7.0, dtype=torch.float64, device="cuda")
    s.solve_rhs_device(torch.from_numpy(np.array(rhs, np.float64)).cuda(), d_x, torch.from_numpy(np.array(fixed, np.float64)).cuda())
    s.synchronize()
    return d_x.cpu().numpy()


def check_values(case, ctx, v, cost, x, k):
    """v against the oracle's get_v and against A x - b; cost against numpy on v; exact zeros at levels of full row rank and behind the rows.
    Returns the largest deviation of v from the oracle, in units of the scale"""
    B, n, m, dims = case["lod"].shape[0], case["n"], case["m"], case["dims"]
    worst = 0.0
    for b in range(B):
        A, F = case["lod"][b, :n, :m[b]].T, np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        assert not v[:, b, m[b]:].any(), ctx + "rows behind the problem's own are not zero"
        for c in range(k):
            sc = case["scale"][c, b]
            e_or = float(np.abs(v[c, b, :m[b]] - case["v"][c, b, :m[b]]).max()) / sc if m[b] else 0.0
            e_ax = float(np.abs(v[c, b, :m[b]] - (A @ x[c, b] - case["rhs"][c, b, :m[b]])).max()) / sc if m[b] else 0.0
            worst = max(worst, e_or)
            assert e_or <= SC.TOL and e_ax <= SC.TOL, ctx + f"problem {b} rhs {c}: v against the oracle {e_or:.3e}, against A x - b {e_ax:.3e}"
            for lv in range(dims.shape[1]):
                rows = v[c, b, F[lv]:F[lv + 1]]
                want = float((rows * rows).sum())
                assert abs(cost[c, b, lv] - want) <= 2 * case["lod"].shape[2] * 2.0 ** -52 * want, ctx + f"cost of level {lv}: {cost[c, b, lv]!r} against {want!r}"
                if case["rank"][b, lv] == dims[b, lv]:
                    assert not rows.any() and cost[c, b, lv] == 0.0, ctx + f"level {lv} of full row rank: v and cost must be exact zeros"
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_v_and_cost_within_tol_of_the_oracle_and_bit_rules(hip, oracle, name):
    case = build(name)
    rhs, fixed = case["rhs"], case["fixed_new"]
    B, m, nf = case["lod"].shape[0], case["m"], case["nf"]
    for policy, producer in POLICIES[name].items():
        s = handle(hip, case, 0, policy)
        s.factorize_solve(keep_factor=True)
        s.multipliers()
        ctx = f"{name} on {s.last_kernel()}: "
        assert s.last_kernel().startswith("lqr_") and (name == "n8" or s.last_kernel() == producer), ctx
        some_free = nf < case["n"]  # (a problem with every variable fixed is not factorized: its ranks are not read)
        np.testing.assert_array_equal(s.getRanks()[0][some_free], case["rank"][some_free], err_msg=ctx + "ranks")
        kept_x = s.solve_rhs(rhs[:2], fixed[:2])
        before = (s.get_x(), s.get_v(), s.getWorkspace(), s.get_lexqr(), s.get_hh_scalars())
        state = observable_state(s)
        res = {}
        for k in KS:
            dev = device_form(s, rhs[:k], fixed[:k])
            assert s.last_consumer_kernel() == plain_variant(case), ctx + s.last_consumer_kernel()
            e = check_values(case, ctx + f"K={k} ", dev["v"], dev["cost"], dev["x"], k)
            print(f"{ctx}K={k} v against the oracle's get_v {e:.2e} of the scale (TOL {SC.TOL:.1e})")
            np.testing.assert_array_equal(bits(dev["x"]), bits(solve_rhs_device(s, rhs[:k], fixed[:k])), err_msg=ctx + f"K={k}: d_x is not solve_rhs_device's")
            v, cost = s.residual_rhs(rhs[:k], fixed[:k])
            np.testing.assert_array_equal(bits(v), bits(dev["v"]), err_msg=ctx + f"K={k} host form, v")
            np.testing.assert_array_equal(bits(cost), bits(dev["cost"]), err_msg=ctx + f"K={k} host form, cost")
            again = device_form(s, rhs[:k], fixed[:k], want=("v", "cost"))  # a second run, and without d_x
            np.testing.assert_array_equal(bits(again["v"]), bits(v), err_msg=ctx + f"K={k} second run")
            np.testing.assert_array_equal(bits(again["cost"]), bits(cost), err_msg=ctx + f"K={k} second run")
            assert (again["x"] == 7.0).all()
            res[k] = (v, cost)
        # independence: positions 0, 1, 63, 64 across nrhs 2, 64, 65 and in other company (K = 1 runs the same lane kernel for v and cost)
        for what in (0, 1):
            np.testing.assert_array_equal(bits(res[65][what][:64]), bits(res[64][what]), err_msg=ctx + "64 of 65")
            np.testing.assert_array_equal(bits(res[64][what][:2]), bits(res[2][what]), err_msg=ctx + "2 of 64")
            np.testing.assert_array_equal(bits(res[2][what][:1]), bits(res[1][what]), err_msg=ctx + "1 of 2")
        rev = s.residual_rhs(rhs[:64][::-1], fixed[:64][::-1])  # position 0 <-> 63
        pair = s.residual_rhs(rhs[[64, 0]], fixed[[64, 0]])     # the second tile's lane 0 at position 0, position 0 at 1
        moved = s.residual_rhs(rhs[np.r_[1:65, 0]], fixed[np.r_[1:65, 0]])  # position 0 at 64, 64 at 63
        for what in (0, 1):
            np.testing.assert_array_equal(bits(rev[what][::-1]), bits(res[64][what]), err_msg=ctx + "reversed order")
            np.testing.assert_array_equal(bits(pair[what]), bits(res[65][what][[64, 0]]), err_msg=ctx + "two of 65 on their own")
            np.testing.assert_array_equal(bits(moved[what]), bits(res[65][what][np.r_[1:65, 0]]), err_msg=ctx + "rotated by one")
        # NaN in the rows behind a problem's own and in the slots behind nfixed: never read
        nan_rhs, nan_fixed = rhs[:2].copy(), fixed[:2].copy()
        for b in range(B):
            nan_rhs[:, b, int(m[b]):] = np.nan
            nan_fixed[:, b, int(nf[b]):] = np.nan
        nan = device_form(s, nan_rhs, nan_fixed)
        for key, want in (("v", res[2][0]), ("cost", res[2][1]), ("x", kept_x)):
            np.testing.assert_array_equal(bits(nan[key]), bits(want), err_msg=ctx + "NaN in unread entries reached " + key)
        # consistency: the handle's own b and fixed values give get_v(); a 2-D rhs is K = 1
        own_v, own_cost = s.residual_rhs(SC.own_rhs(case))
        assert own_v.shape == (B, s.cap) and own_cost.shape == (B, s.nObj)
        for b in range(B):
            sc = max(1.0, float(np.abs(SC.own_rhs(case)[b, :m[b]]).max()) if m[b] else 0.0,
                     float(np.abs(case["lod"][b, :case["n"], :m[b]]).sum(axis=0).max() if m[b] else 0.0) * float(np.abs(before[0][b]).max()))
            e = float(np.abs(own_v[b] - before[1][b]).max()) / sc
            print(f"{ctx}own right-hand side against get_v, problem {b}: {e:.2e}")
            assert e <= SC.TOL, ctx + f"own right-hand side {e:.3e}"
        # no side effects
        after = (s.get_x(), s.get_v(), s.getWorkspace(), s.get_lexqr(), s.get_hh_scalars())
        for a, b_, what in zip(after, before, ("x", "v", "workspace", "factor", "hh")):
            np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
        assert observable_state(s) == state, ctx + "get_multipliers / get_v / get_lambda answer differently"
        buf = np.full((2, B, s.nVar), 7.0)
        assert capi.lib().lexls_lse_get_solve_rhs(s._h, buf.ctypes.data_as(_dp)) == 0
        np.testing.assert_array_equal(bits(buf), bits(kept_x), err_msg=ctx + "get_solve_rhs")
        s.close()


@pytest.mark.parametrize("name", ["n8", "ik"])
def test_placements_lds_and_work_run_and_give_the_staged_bits(hip, oracle, name, monkeypatch):
    """every case sits on the staged side of tangent_map_placement's switches, so LEXLS_TANGENT_PLACEMENT moves the shape down the list as
    tests/test_gpu_lse_solve_rhs.py does: residual_rhs_kernel<64, 1 | 2> and the state offset of the work form run here"""
    case = build(name)
    s = handle(hip, case, 0)
    s.factorize()  # factorize() alone is enough: no x of the current factor is needed
    want = device_form(s, case["rhs"], case["fixed_new"])
    assert s.last_consumer_kernel() == "residual_rhs<64,staged>"
    for env in ("lds", "work"):
        monkeypatch.setenv("LEXLS_TANGENT_PLACEMENT", env)
        for k in (1, 2, 65):
            got = device_form(s, case["rhs"][:k], case["fixed_new"][:k])
            assert s.last_consumer_kernel() == f"residual_rhs<64,{env}>"
            check_values(case, f"{name} {env} K={k} ", got["v"], got["cost"], got["x"], k)
            for key in ("v", "cost") + (("x",) if k > 1 else ()):
                np.testing.assert_array_equal(bits(got[key]), bits(want[key][:k]), err_msg=f"{name}: {env} K={k} {key}")
            np.testing.assert_array_equal(bits(got["x"]), bits(solve_rhs_device(s, case["rhs"][:k], case["fixed_new"][:k])), err_msg=f"{name}: {env} K={k} d_x")
        monkeypatch.delenv("LEXLS_TANGENT_PLACEMENT")
    s.close()


def test_fixed_none_means_the_handles_values(hip, oracle):
    case = build("fixed")
    s = handle(hip, case, 0)
    s.factorize_solve(keep_factor=True)
    held = np.repeat(case["fixed"]["fixed_val"][None], 2, axis=0)
    for a, b in zip(s.residual_rhs(case["rhs"][:2]), s.residual_rhs(case["rhs"][:2], held)):
        np.testing.assert_array_equal(bits(a), bits(b))
    s.close()


def rc_calls(s, rhs, k, outputs=True):
    """(return code of the host form, of the device form, whether the device outputs still hold the sentinels)"""
    rc_h = capi.lib().lexls_lse_residual_rhs(None if s is None else s._h, None if rhs is None else rhs.ctypes.data_as(_dp), None, k)
    d_in = None if rhs is None else torch.from_numpy(np.array(rhs, np.float64)).cuda()
    outs = [torch.full((2, 8, 64), 7.0, dtype=torch.float64, device="cuda") for _ in range(3)]  # (a refused call writes nothing)
    rc_d = capi.lib().lexls_lse_residual_rhs_device(None if s is None else s._h, None if d_in is None else C.c_void_p(d_in.data_ptr()), None, k,
                                                    *[C.c_void_p(o.data_ptr()) if outputs else None for o in outs])
    torch.cuda.synchronize()
    return rc_h, rc_d, all(bool((o == 7.0).all()) for o in outs)


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    case = build("ik")
    rhs = np.ascontiguousarray(case["rhs"][:2])
    s = handle(hip, case, 0)
    v, cost = np.full((2, s.batch, s.cap), 7.0), np.full((2, s.batch, s.nObj), 7.0)

    def rc_get():
        return capi.lib().lexls_lse_get_residual_rhs(s._h, v.ctypes.data_as(_dp), cost.ctypes.data_as(_dp))

    def refused(code, k=2, r=rhs):
        assert rc_calls(s, r, k) == (code, code, True)
        assert rc_get() == INVALID and (v == 7.0).all() and (cost == 7.0).all()

    assert rc_calls(None, rhs, 2) == (INVALID, INVALID, True)  # null handle
    refused(INVALID)                                   # no factorization yet
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    refused(INVALID, r=None)                           # null rhs
    refused(INVALID, k=0)                              # nrhs == 0
    refused(INVALID, k=65536)                          # nrhs > 65535 (refused before anything is read)
    assert rc_calls(s, rhs, 2, outputs=False)[1:] == (INVALID, True)  # all outputs null
    assert capi.lib().lexls_lse_get_residual_rhs(s._h, None, None) == INVALID
    want = s.residual_rhs(rhs)
    assert rc_get() == 0
    np.testing.assert_array_equal(v, want[0])
    np.testing.assert_array_equal(cost, want[1])
    v[:], cost[:] = 7.0, 7.0
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert rc_get() == INVALID and (v == 7.0).all()
    s.setRegularization(1, [1e-3] * len(case["caps"]), 0.0)  # a type-1 damped factorization: solve_rhs serves it, this call does not
    s.factorize_solve(keep_factor=True)
    assert capi.lib().lexls_lse_residual_rhs(s._h, rhs.ctypes.data_as(_dp), None, 2) == UNSUPPORTED
    assert b"regularization_type != 0" in capi.lib().lexls_last_error()  # the message names the condition
    refused(UNSUPPORTED)
    s.solve_rhs(rhs)
    s.close()
