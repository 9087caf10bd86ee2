"""The forward-mode tangents of the LexLSE solve on the device (lexls_lse_solve_tangent*, tangent_rhs_kernel, apply_solve_map_multi_kernel) against
reference (A) of tests/tangent_cases.py — the differentiated dense KKT system on the original data — within TC.TOL (derived there from the two
references' own disagreement on the CPU, never from the device's figures).  Every producer of a kept factor the shape allows is named
(last_kernel), so a dispatch rule that moves makes the case fail instead of quietly testing something else.
K = 1 (M^T w by the single-cotangent kernel), 2 (the multi path), 64 (a full tile), 65 (a second tile)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import tangent_cases as TC
from lexls_amd import capi
from test_gpu_lse_adjoint_matrix import handle, observable_state

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
KS = (1, 2, 64, 65)
KMAX = max(KS)
_dp, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def worst_gap(got, ref):
    """largest error per problem and tangent, relative to max(1, largest magnitude of that reference row)"""
    return max(float(np.abs(got[c, b] - ref[c, b]).max()) / max(1.0, float(np.abs(ref[c, b]).max())) for c in range(ref.shape[0]) for b in range(ref.shape[1]))


def device_form(s, dlod, dfixed, with_flags=True):
    K = dlod.shape[0]
    d_dlod = torch.from_numpy(np.array(dlod, np.float64)).cuda()
    d_dfixed = None if dfixed is None else torch.from_numpy(np.array(dfixed, np.float64)).cuda()
    d_dx = torch.full((K, s.batch, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((s.batch,), 7, dtype=torch.uint8, device="cuda") if with_flags else None
    s.solve_tangent_device(d_dlod, d_dx, d_dfixed, d_f)
    s.synchronize()
    return d_dx.cpu().numpy(), d_f.cpu().numpy() if with_flags else None


def consumer(name):
    case = TC.base_case(name)
    return TC.placement(case["n"], case["lod"].shape[2])


def check_case(hip, name, producers, extra_state=False):
    t = TC.build(name, KMAX, 0, False)
    case, ref, dlod, dfixed = t["case"], t["A"], t["dlod"], t["dfixed"]
    flags = np.asarray(case["flags"], np.uint8)
    B, n = case["lod"].shape[0], case["n"]
    m = case["dims"].sum(axis=1)
    nfs = [TC.fixed_of(case, b)[0] for b in range(B)]
    for policy, producer in producers.items():
        ctx = f"{name} on {producer}: "
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        if producer is not None:
            assert s.last_kernel() == producer
        if extra_state:  # something to keep: the multipliers, the residuals and a removal search of this factor
            s.multipliers()
            s.get_v()
            assert capi.lib().lexls_lse_sensitivity(s._h, None, C.c_int32(0), C.c_double(1e-8), C.c_double(1e-12)) == 0
        before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.getCtrType(), s.getFixedType())
        state = observable_state(s)
        results = {}
        for K in KS:
            dx, diff = s.solve_tangent(dlod[:K], dfixed[:K])
            assert s.last_consumer_kernel() == consumer(name), ctx + s.last_consumer_kernel()
            np.testing.assert_array_equal(diff, flags, err_msg=ctx + f"K={K} flags")
            e = worst_gap(dx, ref[:K])
            print(f"{ctx}K={K} dx against (A) {e:.2e} (TOL {TC.TOL:.1e})")
            assert e <= TC.TOL, ctx + f"K={K}: {e:.3e}"
            for b in range(B):
                assert flags[b] or not dx[:, b].view(np.uint64).any(), ctx + f"K={K} problem {b}: flagged 0, dx not zero as bits"
            d_dx, d_f = device_form(s, dlod[:K], dfixed[:K])
            np.testing.assert_array_equal(d_dx.view(np.uint64), dx.view(np.uint64), err_msg=ctx + f"K={K} device form")
            np.testing.assert_array_equal(d_f, diff, err_msg=ctx + f"K={K} device form")
            results[K] = dx
        # a tangent's bits in the multi kernel do not depend on its company: lane 0 of K = 2, lane 63 of K = 64, lane 0 of the second tile
        order = list(range(1, 64)) + [0]
        moved = s.solve_tangent(dlod[order], dfixed[order])[0]
        np.testing.assert_array_equal(moved[63].view(np.uint64), results[2][0].view(np.uint64), err_msg=ctx + "lane 63 of 64 against lane 0 of 2")
        np.testing.assert_array_equal(results[64][0].view(np.uint64), results[2][0].view(np.uint64), err_msg=ctx + "lane 0 of 64 against lane 0 of 2")
        second = s.solve_tangent(dlod[[64, 0]], dfixed[[64, 0]])[0]
        np.testing.assert_array_equal(results[65][64].view(np.uint64), second[0].view(np.uint64), err_msg=ctx + "lane 0 of the second tile against lane 0 of 2")
        # NaN in the rows behind a problem's own and in the slots behind nfixed: never read
        nan_lod, nan_fixed = dlod[:2].copy(), dfixed[:2].copy()
        for b in range(B):
            nan_lod[:, b, :, int(m[b]):] = np.nan
            nan_fixed[:, b, nfs[b]:] = np.nan
        got = s.solve_tangent(nan_lod, nan_fixed)[0]
        np.testing.assert_array_equal(got.view(np.uint64), results[2].view(np.uint64), err_msg=ctx + "NaN in unread entries")
        if not any(nfs):  # dfixed = NULL is dfixed = 0, and without fixed variables it is never read
            np.testing.assert_array_equal(s.solve_tangent(dlod[:2])[0].view(np.uint64), results[2].view(np.uint64), err_msg=ctx + "dfixed = None")
        else:
            zero = s.solve_tangent(dlod[:2], np.zeros_like(dfixed[:2]))[0]
            np.testing.assert_array_equal(s.solve_tangent(dlod[:2])[0].view(np.uint64), zero.view(np.uint64), err_msg=ctx + "dfixed = None")
        # a single direction without the leading axis
        one, _ = s.solve_tangent(dlod[0], dfixed[0])
        np.testing.assert_array_equal(one.view(np.uint64), results[1][0].view(np.uint64), err_msg=ctx + "one direction")
        # the duality identity against the device's own reverse mode
        if "A" in case:
            G, gdiff = s.solve_adjoint_matrix(case["g"])
            np.testing.assert_array_equal(gdiff, flags)
            grad_fixed = s.solve_adjoint(case["g"])[1]
            dual = 0.0
            for b in range(B):
                if not flags[b]:
                    continue
                for c in range(4):
                    terms = np.concatenate([case["g"][b] * results[65][c, b], -(G[b][:, :m[b]] * dlod[c, b][:, :m[b]]).ravel(),
                                            -grad_fixed[b, :nfs[b]] * dfixed[c, b, :nfs[b]]])
                    dual = max(dual, abs(terms.sum()) / max(1.0, float(np.abs(terms).sum())))
            print(f"{ctx}duality against solve_adjoint_matrix {dual:.2e}")
            assert dual <= TC.TOL, ctx + f"duality {dual:.3e}"
        # x, the factor, the activation types and what the other getters answer are what they were
        after = (s.get_x(), s.get_lexqr(), s.get_hh_scalars(), s.getCtrType(), s.getFixedType())
        for a, b_, what in zip(after, before, ("x", "factor", "hh", "ctr_type", "fixed_type")):
            np.testing.assert_array_equal(a, b_, err_msg=ctx + what + " changed")
        assert observable_state(s) == state, ctx + "get_multipliers / get_v / get_lambda answer differently"
        s.close()


@pytest.mark.parametrize("name", TC.CASES)
def test_device_tangents_within_tol_of_the_kkt_reference(hip, oracle, name):
    """base / used_up / one_row: the small branches; ragged: empty levels and free variables; fixed: fixed variables with non-zero dfixed, the
    all-fixed problem; fixed_tall: more than 64 rows; ik: the project's shape; wide: n = 70; rank_def, fixed_rank_def: flag 0; mixed: a
    rank-unstable problem beside a stable one"""
    np.testing.assert_array_equal(TC.base_case(name)["flags"], np.asarray(TC.FLAGS[name], np.uint8))
    check_case(hip, name, TC.PRODUCERS[name], extra_state=name in ("ik", "fixed"))


@pytest.mark.parametrize("name", TC.FIT_NAMES)
def test_both_sides_of_each_placement_switch(hip, oracle, name):
    assert consumer(name) == TC.PLACEMENTS[name]
    check_case(hip, name, {None: None})


@pytest.mark.parametrize("name", ["ik", "fixed", "fixed_tall"])
def test_forced_placements_give_the_same_bits(hip, oracle, name, monkeypatch):
    """LEXLS_TANGENT_PLACEMENT moves a shape down the list: the same dfma chains, only the place of the per-lane vectors and of the factor differs"""
    t = TC.build(name, KMAX, 0, False)
    case = t["case"]
    s = handle(hip, case)
    s.factorize_solve(keep_factor=True)
    want = s.solve_tangent(t["dlod"], t["dfixed"])[0]
    assert s.last_consumer_kernel() == TC.STAGED
    for env, place in (("lds", TC.LDS), ("work", TC.WORK)):
        monkeypatch.setenv("LEXLS_TANGENT_PLACEMENT", env)
        got = s.solve_tangent(t["dlod"], t["dfixed"])[0]
        assert s.last_consumer_kernel() == place
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=f"{name}: {place}")
    s.close()


def rc_host(s, dlod, K):
    return capi.lib().lexls_lse_solve_tangent(s._h, None if dlod is None else dlod.ctypes.data_as(_dp), None, K)


def rc_device(s, dlod, K, with_dx=True):
    """(return code of the device form on sentinel-filled outputs, whether the outputs still hold the sentinels)"""
    d_in = None if dlod is None else torch.from_numpy(np.array(dlod, np.float64)).cuda()
    d_dx = torch.full((max(K, 1), s.batch, s.nVar), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((s.batch,), 7, dtype=torch.uint8, device="cuda")
    rc = capi.lib().lexls_lse_solve_tangent_device(s._h, None if d_in is None else C.c_void_p(d_in.data_ptr()), None, K,
                                                   C.c_void_p(d_dx.data_ptr()) if with_dx else None, C.c_void_p(d_f.data_ptr()))
    s.synchronize()
    return rc, bool((d_dx == 7.0).all() and (d_f == 7).all())


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    t = TC.build("ik", KMAX, 0, False)
    case, dlod = t["case"], np.ascontiguousarray(t["dlod"][:2])
    s = handle(hip, case)
    dx, f = np.full((2, s.batch, s.nVar), 7.0), np.full(s.batch, 7, np.uint8)

    def rc_get():
        return capi.lib().lexls_lse_get_tangent(s._h, dx.ctypes.data_as(_dp), f.ctypes.data_as(_u8p))

    def refused(code):
        assert rc_host(s, dlod, 2) == code
        assert rc_device(s, dlod, 2) == (code, True)
        assert rc_get() == INVALID
        assert (dx == 7.0).all() and (f == 7).all()

    refused(INVALID)                                   # no factorization yet
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    assert rc_host(s, None, 2) == INVALID and rc_device(s, None, 2) == (INVALID, True)      # null dlod
    assert rc_host(s, dlod, 0) == INVALID and rc_device(s, dlod, 0) == (INVALID, True)      # ntan == 0
    assert rc_device(s, dlod, 2, with_dx=False) == (INVALID, True)                          # null d_dx
    assert rc_get() == INVALID                         # nothing computed yet
    s.solveLeastNorm_1()                               # x is no longer the basic solution of the factor
    refused(INVALID)
    assert rc_host(s, dlod, 2) == INVALID and b"no x belongs" in capi.lib().lexls_last_error()
    s.solve()
    want = s.solve_tangent(dlod)
    assert rc_get() == 0
    np.testing.assert_array_equal(dx, want[0])
    np.testing.assert_array_equal(f, want[1])
    dx[:], f[:] = 7.0, 7
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert rc_get() == INVALID and (dx == 7.0).all()
    s.setRegularization(1, [1e-3] * len(case["caps"]))  # a regularized factorization
    s.factorize_solve(keep_factor=True)
    assert rc_host(s, dlod, 2) == UNSUPPORTED
    assert b"regularization_type" in capi.lib().lexls_last_error()
    assert rc_device(s, dlod, 2) == (UNSUPPORTED, True)
    assert rc_get() == INVALID and (dx == 7.0).all() and (f == 7).all()
    s.close()


def test_jvp_lod_is_the_c_abi_result(hip, oracle):
    from lexls_amd.torch_adjoint import jvp_lod
    t = TC.build("mixed", KMAX, 0, False)
    case = t["case"]
    B, n = case["lod"].shape[0], case["n"]
    s = hip.BatchedLexLSE(B, n, case["caps"])
    lod = torch.from_numpy(np.array(case["lod"])).cuda()
    d = torch.from_numpy(np.array(t["dlod"][:3])).cuda()
    x, dx = jvp_lod(s, lod, d)
    s.synchronize()
    assert float(np.abs(x.cpu().numpy() - case["ref"]["x"]).max()) <= 1e-10
    assert s.differentiable.cpu().numpy().tolist() == TC.FLAGS["mixed"]
    want, _ = s.solve_tangent(t["dlod"][:3])
    np.testing.assert_array_equal(dx.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert worst_gap(dx.cpu().numpy(), t["A"][:3]) <= TC.TOL
    x1, dx1 = jvp_lod(s, lod, d[0])  # one direction without the leading axis
    s.synchronize()
    assert tuple(dx1.shape) == (B, n)
    np.testing.assert_array_equal(dx1.cpu().numpy().view(np.uint64), s.solve_tangent(t["dlod"][0])[0].view(np.uint64))
    s.close()
