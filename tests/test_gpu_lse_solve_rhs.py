"""lexls_lse_solve_rhs* on the device — new right-hand sides and fixed values on a kept factor, plain (solve_rhs_front_kernel +
apply_solve_map_kernel / apply_solve_map_multi_kernel) and damped (apply_solve_map_reg_multi_kernel) — against reference (a) of
tests/solve_rhs_cases.py, the oracle solving [A | b_new] from scratch, within SC.TOL (derived there from the two references' own disagreement on
the CPU, never from the device's figures).  Every producer of a kept factor the shape allows is named (last_kernel), and so is the variant that
served the call (last_consumer_kernel).  K = 1 (plain: the single-vector kernel), 2, 64 (a full tile), 65 (a second tile)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_cases as AC
import solve_rhs_cases as SC
from lexls_amd import capi
from test_gpu_lse_adjoint_matrix import observable_state
from test_gpu_lse_adjoint_reg import POLICIES as REG_POLICIES, handle

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
KS = (1, 2, 64, 65)
_dp = C.POINTER(C.c_double)
PLAIN_POLICIES = {name: AC.PRODUCERS.get(name, AC.SMALL) for name in SC.NAMES}
PLAIN_POLICIES["mid"] = PLAIN_POLICIES["wide"] = {None: None}  # (whatever the plan gives these shapes, printed)
REG = dict(REG_POLICIES, six=REG_POLICIES["base"], mid={None: None})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def device_form(s, rhs, fixed):
    d_rhs = torch.from_numpy(np.array(rhs, np.float64)).cuda()
    d_fixed = None if fixed is None else torch.from_numpy(np.array(fixed, np.float64)).cuda()
    d_x = torch.full(tuple(rhs.shape[:-1]) + (s.nVar,), 7.0, dtype=torch.float64, device="cuda")
    s.solve_rhs_device(d_rhs, d_x, d_fixed)
    s.synchronize()
    return d_x.cpu().numpy()


def check_case(hip, name, reg_type):
    case = SC.build(name, reg_type)
    ref, rhs, fixed = case["a"], case["rhs"], case["fixed_new"]
    B, n = case["lod"].shape[0], case["n"]
    m, nf = case["dims"].sum(axis=1), case["nf"]
    worst = 0.0
    for policy, producer in (REG[name] if reg_type else PLAIN_POLICIES[name]).items():
        s = handle(hip, case, reg_type, policy)
        s.factorize_solve(keep_factor=True)
        ctx = f"{name} type {reg_type} on {s.last_kernel()}: "
        assert s.last_kernel().startswith("lqr_") and (producer is None or s.last_kernel() == producer), ctx
        if not reg_type:
            s.multipliers()  # something to keep besides x and v
        g_rhs, g_fixed = s.solve_adjoint(case["g"])
        before = (s.get_x(), s.get_v(), s.getWorkspace(), s.get_lexqr(), s.get_hh_scalars())
        state, adj = observable_state(s), s.solve_adjoint(case["g"])
        results = {}
        for K in KS:
            x = s.solve_rhs(rhs[:K], fixed[:K])
            assert s.last_consumer_kernel() == SC.variant(case, reg_type, K), ctx + s.last_consumer_kernel()
            e = SC.rel_rows(x, ref[:K])
            worst = max(worst, e)
            print(f"{ctx}K={K} x against (a) {e:.2e} (TOL {SC.TOL:.1e})")
            assert e <= SC.TOL, ctx + f"K={K}: {e:.3e}"
            np.testing.assert_array_equal(bits(device_form(s, rhs[:K], fixed[:K])), bits(x), err_msg=ctx + f"K={K} device form")
            np.testing.assert_array_equal(bits(s.solve_rhs(rhs[:K], fixed[:K])), bits(x), err_msg=ctx + f"K={K} second run")
            results[K] = x
        # independence: the 64 in reverse order; two of them embedded in a call of 65 (the second tile's lane 0 among them)
        rev = s.solve_rhs(rhs[:64][::-1], fixed[:64][::-1])
        np.testing.assert_array_equal(bits(rev[::-1]), bits(results[64]), err_msg=ctx + "reversed order")
        np.testing.assert_array_equal(bits(results[65][:64]), bits(results[64]), err_msg=ctx + "64 of 65")
        pair = s.solve_rhs(rhs[[64, 5]], fixed[[64, 5]])
        np.testing.assert_array_equal(bits(pair), bits(results[65][[64, 5]]), err_msg=ctx + "two of 65 on their own")
        # NaN in the rows behind a problem's own and in the slots behind nfixed: never read
        nan_rhs, nan_fixed = rhs[:2].copy(), fixed[:2].copy()
        for b in range(B):
            nan_rhs[:, b, int(m[b]):] = np.nan
            nan_fixed[:, b, int(nf[b]):] = np.nan
        np.testing.assert_array_equal(bits(s.solve_rhs(nan_rhs, nan_fixed)), bits(results[2]), err_msg=ctx + "NaN in unread entries")
        # round trip: the handle's own b and fixed values reproduce get_x(), rank-deficient problems included; a 2-D rhs is K = 1
        own = SC.own_rhs(case)
        for back in (s.solve_rhs(own), s.solve_rhs(np.stack([own, own]))[1]):
            e = SC.rel_rows(back, before[0])
            print(f"{ctx}round trip {e:.2e}")
            assert back.shape == (B, n) and e <= SC.TOL, ctx + f"round trip {e:.3e}"
        # transposition on the device: <g, x(b, f)> = <M^T g, b> + <N^T g, f> with the existing adjoint kernels
        for c in range(4):
            for b in range(B):
                terms = np.concatenate([case["g"][b] * results[65][c, b], -g_rhs[b, :m[b]] * rhs[c, b, :m[b]], -g_fixed[b, :nf[b]] * fixed[c, b, :nf[b]]])
                d = abs(terms.sum()) / max(1.0, float(np.abs(terms).sum()))
                assert d <= SC.TOL, ctx + f"transposition {d:.3e}"
        # no side effects
        after = (s.get_x(), s.get_v(), s.getWorkspace(), s.get_lexqr(), s.get_hh_scalars())
        for a, b_, what in zip(after, before, ("x", "v", "workspace", "factor", "hh")):
            np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
        assert observable_state(s) == state, ctx + "get_multipliers / get_v / get_lambda answer differently"
        got = capi.lib().lexls_lse_get_adjoint
        buf_r, buf_f = np.full((B, s.cap), 7.0), np.full((B, n), 7.0)
        assert got(s._h, buf_r.ctypes.data_as(_dp), buf_f.ctypes.data_as(_dp)) == 0
        np.testing.assert_array_equal(bits(buf_r), bits(adj[0]), err_msg=ctx + "get_adjoint")
        np.testing.assert_array_equal(bits(buf_f), bits(adj[1]), err_msg=ctx + "get_adjoint")
        s.close()
    return worst


@pytest.mark.parametrize("name", SC.NAMES)
def test_plain_factors_within_tol_of_the_oracle(hip, oracle, name):
    print(f"{name}: largest device error {check_case(hip, name, 0):.1e}")


@pytest.mark.parametrize("name", SC.NAMES)
def test_damped_factors_within_tol_of_the_oracle(hip, oracle, name):
    worst = {t: check_case(hip, name, t) for t in SC.types_of(name) if t}
    print(f"{name}: largest device error per type {({t: '%.1e' % e for t, e in worst.items()})}")


@pytest.mark.parametrize("name", ["ik", "fixed", "fixed_rank_def", "wide"])
def test_plain_placements_lds_and_work_run_and_give_the_staged_bits(hip, oracle, name, monkeypatch):
    """Every plain case sits on the staged side of tangent_map_placement's switches (n = 92 | 93 at cap = 90), so LEXLS_TANGENT_PLACEMENT moves
    the shape down the list, as tests/test_gpu_lse_tangent.py does: apply_solve_map_multi_kernel<64, 1 | 2, false>, the work term of
    solve_rhs_work_bytes and the state offset handed to the work form run here.  Named, within TOL of reference (a), the staged form's bits."""
    case = SC.build(name, 0)
    s = handle(hip, case, 0)
    s.factorize()
    want = s.solve_rhs(case["rhs"], case["fixed_new"])
    assert s.last_consumer_kernel() == "solve_rhs<64,staged>"
    for env in ("lds", "work"):
        monkeypatch.setenv("LEXLS_TANGENT_PLACEMENT", env)
        for K in (2, 65):
            got = s.solve_rhs(case["rhs"][:K], case["fixed_new"][:K])
            assert s.last_consumer_kernel() == f"solve_rhs<64,{env}>"
            e = SC.rel_rows(got, case["a"][:K])
            print(f"{name} {env} K={K}: x against (a) {e:.2e}")
            assert e <= SC.TOL
            np.testing.assert_array_equal(bits(got), bits(want[:K]), err_msg=f"{name}: {env} K={K}")
            np.testing.assert_array_equal(bits(device_form(s, case["rhs"][:K], case["fixed_new"][:K])), bits(got), err_msg=f"{name}: {env} K={K} device form")
        monkeypatch.delenv("LEXLS_TANGENT_PLACEMENT")
        np.testing.assert_array_equal(bits(s.solve_rhs(case["rhs"][:2], case["fixed_new"][:2])), bits(want[:2]))  # (a smaller request after a larger one)
    s.close()


def test_the_damped_cases_sit_on_every_side_of_the_damped_rule():
    """no device work: the three damped forms are named per case in check_case; this pins which case is on which side (ik lds, mid hbm, wide work)"""
    assert [SC.variant(nm, 1).split(",")[1][:-1] for nm in ("ik", "mid", "wide")] == ["lds", "hbm", "work"]
    n, cap = SC.OWN["mid"]["n"], sum(SC.OWN["mid"]["dims"])
    assert SC.reg_variant(49, cap).endswith("lds>") and SC.reg_variant(50, cap).endswith("hbm>") and SC.reg_variant(74, cap).endswith("hbm>")
    assert SC.reg_variant(75, cap).endswith("work>") and 50 <= n <= 74


@pytest.mark.parametrize("name,reg_type", [("ik", 1), ("fixed", 8), ("rank_def", 3)])
def test_forced_forms_give_the_same_bits(hip, oracle, name, reg_type, monkeypatch):
    """LEXLS_SOLVE_RHS_REG_FORM moves a shape down the list: the same dfma chains, only the place of the matrices and the per-lane vectors differs"""
    case = SC.build(name, reg_type)
    s = handle(hip, case, reg_type)
    s.factorize()  # factorize() alone is enough: no x of the current factor is needed
    want = s.solve_rhs(case["rhs"], case["fixed_new"])
    assert s.last_consumer_kernel() == "solve_rhs_reg<64,lds>"
    assert SC.rel_rows(want, case["a"]) <= SC.TOL
    for env in ("hbm", "work"):
        monkeypatch.setenv("LEXLS_SOLVE_RHS_REG_FORM", env)
        got = s.solve_rhs(case["rhs"], case["fixed_new"])
        assert s.last_consumer_kernel() == f"solve_rhs_reg<64,{env}>"
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{name}: {env}")
    s.close()


def test_fixed_none_means_the_handles_values(hip, oracle):
    for reg_type in (0, 1):
        case = SC.build("fixed", reg_type)
        s = handle(hip, case, reg_type)
        s.factorize_solve(keep_factor=True)
        held = np.repeat(case["fixed"]["fixed_val"][None], 2, axis=0)
        np.testing.assert_array_equal(bits(s.solve_rhs(case["rhs"][:2])), bits(s.solve_rhs(case["rhs"][:2], held)))
        s.close()


def rc_calls(s, rhs, K, with_x=True):
    """(return code of the host form, return code of the device form, whether the device output still holds the sentinels)"""
    rc_h = capi.lib().lexls_lse_solve_rhs(s._h, None if rhs is None else rhs.ctypes.data_as(_dp), None, K)
    d_in = None if rhs is None else torch.from_numpy(np.array(rhs, np.float64)).cuda()
    d_x = torch.full((min(max(K, 1), 2), s.batch, s.nVar), 7.0, dtype=torch.float64, device="cuda")  # (a refused call writes nothing: two rows do)
    rc_d = capi.lib().lexls_lse_solve_rhs_device(s._h, None if d_in is None else C.c_void_p(d_in.data_ptr()), None, K, C.c_void_p(d_x.data_ptr()) if with_x else None)
    s.synchronize()
    return rc_h, rc_d, bool((d_x == 7.0).all())


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    case = SC.build("ik", 0)
    rhs = np.ascontiguousarray(case["rhs"][:2])
    s = handle(hip, case, 0)
    x = np.full((2, s.batch, s.nVar), 7.0)

    def rc_get():
        return capi.lib().lexls_lse_get_solve_rhs(s._h, x.ctypes.data_as(_dp))

    def refused(code, K=2, r=rhs):
        assert rc_calls(s, r, K) == (code, code, True)
        assert rc_get() == INVALID and (x == 7.0).all()

    refused(INVALID)                                   # no factorization yet
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    refused(INVALID, r=None)                           # null rhs
    refused(INVALID, K=0)                              # nrhs == 0
    refused(INVALID, K=65536)                          # nrhs > 65535 (refused before anything is read: the two right-hand sides suffice)
    assert capi.lib().lexls_lse_solve_rhs(s._h, rhs.ctypes.data_as(_dp), None, 65536) == INVALID and b"nrhs > 65535" in capi.lib().lexls_last_error()
    assert rc_calls(s, rhs, 2, with_x=False)[1:] == (INVALID, True)  # null d_x
    want = s.solve_rhs(rhs)
    assert rc_get() == 0
    np.testing.assert_array_equal(x, want)
    x[:] = 7.0
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert rc_get() == INVALID and (x == 7.0).all()
    nobj = len(case["caps"])
    for reg_type, variable, word in ((2, 0.0, b"regularization_type 2"), (6, 0.0, b"regularization_type 6"), (7, 0.0, b"regularization_type 7"),
                                     (1, 0.5, b"variable_regularization_factor")):
        s.setRegularization(reg_type, [1e-3] * nobj, variable)
        s.factorize_solve(keep_factor=True)
        assert capi.lib().lexls_lse_solve_rhs(s._h, rhs.ctypes.data_as(_dp), None, 2) == UNSUPPORTED
        assert word in capi.lib().lexls_last_error()  # the message names the condition
        refused(UNSUPPORTED)
    s.close()


def test_torch_solve_rhs_and_jvp_rhs(hip, oracle):
    from lexls_amd.torch_adjoint import jvp_rhs, solve_new_rhs as solve_rhs
    case = SC.build("ik", 1)
    B, n = case["lod"].shape[0], case["n"]
    s = handle(hip, case, 1)
    s.set_adjoint_regularized_multi(True)
    s.factorize_solve(keep_factor=True)
    rhs = torch.from_numpy(np.array(case["rhs"][:3])).cuda().requires_grad_(True)
    x = solve_rhs(s, rhs)
    s.synchronize()
    np.testing.assert_array_equal(bits(x.detach().cpu().numpy()), bits(s.solve_rhs(case["rhs"][:3])))
    w = torch.from_numpy(np.array(case["fixed_new"][:3])).cuda()  # any cotangent of the shape of x
    (x * w).sum().backward()
    s.synchronize()
    # the inner-product test of the backward: <w, M db> = <M^T w, db> for a random db, M db by the forward call itself
    db = case["rhs"][3:6]
    lhs = float((case["fixed_new"][:3] * s.solve_rhs(db, np.zeros((3, B, n)))).sum())
    rhs_side = float((rhs.grad.cpu().numpy() * db).sum())
    scale = float(np.abs(case["fixed_new"][:3]).sum() * np.abs(db).max())
    print(f"torch backward: <w, M db> {lhs:.6e} against <M^T w, db> {rhs_side:.6e}")
    assert abs(lhs - rhs_side) <= SC.TOL * scale
    # jvp_rhs on the damped factor against the central difference of the oracle in b (step and bound from the CPU run of the same comparison)
    gap_cpu, fd = SC.jvp_gap("ik", 1)
    dx = jvp_rhs(s, torch.from_numpy(np.array(case["rhs"][:3])).cuda())
    s.synchronize()
    e = SC.rel_rows(dx.cpu().numpy(), fd)
    print(f"jvp_rhs against the central difference {e:.2e} (CPU {gap_cpu:.2e}, JVP_TOL {SC.JVP_TOL:.1e})")
    assert e <= SC.JVP_TOL
    s.close()


def test_torch_gradients_and_jvp_in_the_fixed_values(hip, oracle):
    """SolveNewRhs with a fixed tensor (forward, backward's grad_fixed) and jvp_rhs's dfixed, on the case with fixed variables, plain and damped:
    <w, N df> against <grad_fixed, df>, N df by jvp_rhs(0, df)"""
    from lexls_amd.torch_adjoint import jvp_rhs, solve_new_rhs
    for reg_type in (0, 8):
        case = SC.build("fixed", reg_type)
        B, n, nf = case["lod"].shape[0], case["n"], case["nf"]
        s = handle(hip, case, reg_type)
        s.set_adjoint_regularized_multi(True)
        s.factorize_solve(keep_factor=True)
        rhs = torch.from_numpy(np.array(case["rhs"][:3])).cuda().requires_grad_(True)
        fixed = torch.from_numpy(np.array(case["fixed_new"][:3])).cuda().requires_grad_(True)
        x = solve_new_rhs(s, rhs, fixed)
        s.synchronize()
        np.testing.assert_array_equal(bits(x.detach().cpu().numpy()), bits(s.solve_rhs(case["rhs"][:3], case["fixed_new"][:3])))
        assert SC.rel_rows(x.detach().cpu().numpy(), case["a"][:3]) <= SC.TOL
        w = case["rhs"][6:9, :, :n]  # any cotangent of the shape of x
        (x * torch.from_numpy(np.array(w)).cuda()).sum().backward()
        s.synchronize()
        grad_fixed = fixed.grad.cpu().numpy()
        for b in range(B):
            assert not grad_fixed[:, b, int(nf[b]):].any()  # slots behind nfixed: exactly zero
        db, df = case["rhs"][3:6], case["fixed_new"][3:6]
        live = np.arange(n)[None, None, :] < nf[None, :, None]
        N_df = jvp_rhs(s, torch.zeros((3, B, s.cap), dtype=torch.float64, device="cuda"), torch.from_numpy(np.array(df)).cuda())
        M_db = jvp_rhs(s, torch.from_numpy(np.array(db)).cuda())
        both = jvp_rhs(s, torch.from_numpy(np.array(db)).cuda(), torch.from_numpy(np.array(df)).cuda())
        s.synchronize()
        for lhs, rhs_side, what in ((float((w * N_df.cpu().numpy()).sum()), float((grad_fixed * np.where(live, df, 0.0)).sum()), "fixed"),
                                    (float((w * M_db.cpu().numpy()).sum()), float((rhs.grad.cpu().numpy() * db).sum()), "rhs")):
            scale = float(np.abs(w).sum() * max(np.abs(db).max(), np.abs(df).max()))
            print(f"type {reg_type} {what}: {lhs:.6e} against {rhs_side:.6e}")
            assert abs(lhs - rhs_side) <= SC.TOL * scale
        assert SC.rel_rows(both.cpu().numpy(), (M_db + N_df).cpu().numpy()) <= SC.TOL  # linear in (drhs, dfixed)
        np.testing.assert_array_equal(bits(both.cpu().numpy()), bits(s.solve_rhs(db, df)))  # the same call
        s.close()
