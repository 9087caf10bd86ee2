"""Bounds gradients of batched LexLSI solutions for MANY cotangents after a REGULARIZED resident run (lexls_lsi_batch_solve_adjoint_multi(_device)
once lexls_lsi_batch_set_adjoint_regularized_multi is on: the damped final factor of ensure_final_factor, lexls_lse_solve_adjoint_multi_device
on it — solve_adjoint_reg_multi_kernel — and lsi_adjoint_scatter_multi_kernel), on the runs of tests/test_gpu_lsi_adjoint_reg.py.

Reference, built the way that file builds its own: the oracle driver gives the final working set; lsi_adjoint_cases.final_problem forms the
equality problem; damped unit solves of the oracle's equality solver on it (adjoint_reg_multi_cases.solve_maps) give M_reg and N_reg; G M_reg and
G N_reg are scattered by constraint type in numpy.  Tolerance: adjoint_reg_multi_cases.TOL (1e-12, from the CPU references' own gap)."""
import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_reg_multi_cases as XC
import lsi_adjoint_cases as LC
from test_gpu_lsi_adjoint_reg import RUNS, factors_of, oracle_runs, rel

pytestmark = pytest.mark.gpu


def reference(case, reg_type, fac, G):
    """(grad_lb, grad_ub (batch, K, total), runs): tests/test_gpu_lsi_adjoint_reg.py's reference for K cotangents per instance"""
    n, probs = case["n"], case["probs"]
    runs = oracle_runs(case, reg_type, fac)
    B, K, total = len(probs), G.shape[1], sum(len(o["lb"]) for o in probs[0])
    off = 1 if "var" in probs[0][0] else 0
    formed = [LC.final_problem(n, probs[b], runs[b]["active"]) for b in range(B)]
    nf = np.asarray([len(f[3]) for f in formed], np.uint32)
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b, f in enumerate(formed):
        for j, (var, value, _, _) in enumerate(f[3]):
            idx[b, j], val[b, j] = var, value
    lse = dict(n=n, caps=formed[0][2], lod=np.stack([f[0] for f in formed]), dims=np.stack([f[1] for f in formed]),
               fixed=dict(nfixed=nf, fixed_idx=idx, fixed_val=val) if nf.any() else {},
               factors=np.stack([np.asarray(factors_of(fac, b), float)[off:] for b in range(B)]))
    grad_rhs, grad_fixed = XC.reference_a(lse, XC.solve_maps(lse, reg_type), G)
    glb, gub = np.zeros((B, K, total)), np.zeros((B, K, total))
    for b, f in enumerate(formed):
        if runs[b]["info"]["status"] != LC.SOLVED:
            continue
        for j, (_, _, u, t) in enumerate(f[3]):
            (glb if t == LC.LB else gub)[b, :, u] = grad_fixed[b, :, j]
        for r, (u, t) in enumerate(f[4]):
            (glb if t == LC.LB else gub)[b, :, u] = grad_rhs[b, :, r]
    return glb, gub, runs


def device_run(case, reg_type, fac, on_device, batch_obj=None, multi=True, single=False):
    from lexls_amd import lexlsi
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    b = batch_obj or lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.set_adjoint_regularized_multi(multi)
    b.set_adjoint_regularized(single)
    params = dict(regularization_type=reg_type)
    if fac is None:
        b.set_instance_regularization(None)
        params = {}
    elif fac.ndim == 2:
        b.set_instance_regularization(torch.from_numpy(fac.copy()).cuda() if on_device else fac)
    else:
        b.set_instance_regularization(None)
        params["regularization_factors"] = fac
    return b, b.run(pk, **params)


@pytest.mark.parametrize("name", list(RUNS))
def test_regularized_runs_against_the_damped_unit_solves(hip, oracle, name):
    case_name, reg_type, fac, on_device = RUNS[name]
    case = LC.build(case_name)
    B, n = len(case["probs"]), case["n"]
    sets = {"2": XC.P.normal(20330500, B * 2 * n).reshape(B, 2, n), "identity": np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))}
    b, r = device_run(case, reg_type, fac, on_device, single=True)  # both switches: the damped final factor is shared by the two calls
    assert "regularized" in b.last_kernel(), b.last_kernel()  # the run was resident on a regularized kernel
    before = b.final_factorizations()
    got = {}
    for st, G in sets.items():
        glb_ref, gub_ref, runs = reference(case, reg_type, fac, G)
        active = np.stack([np.concatenate(x["active"]) for x in runs])
        status = np.asarray([x["info"]["status"] for x in runs])
        np.testing.assert_array_equal(r["active"], active)
        assert max(np.abs(glb_ref).max(), np.abs(gub_ref).max()) > 1e-2
        glb, gub = b.solve_adjoint_multi(G)
        print(f"{name}, K = {st}: gap to the reference {max(rel(glb, glb_ref), rel(gub, gub_ref)):.2e} (TOL {XC.TOL:.0e})")
        assert rel(glb, glb_ref) <= XC.TOL and rel(gub, gub_ref) <= XC.TOL
        off_lb, off_ub = active != LC.LB, (active != LC.UB) & (active != LC.EQ)
        assert not glb[np.broadcast_to(off_lb[:, None, :], glb.shape)].any() and not gub[np.broadcast_to(off_ub[:, None, :], gub.shape)].any()  # exact zeros outside the working set
        assert not glb[status != LC.SOLVED].any() and not gub[status != LC.SOLVED].any()
        dlb, dub = b.solve_adjoint_multi_device(torch.from_numpy(G.copy()).cuda())  # the device form: the same bits
        np.testing.assert_array_equal(dlb.cpu().numpy(), glb), np.testing.assert_array_equal(dub.cpu().numpy(), gub)
        got[st] = (glb, gub)
    one = b.solve_adjoint(sets["2"][:, 0])  # the single call on the same factor: tolerance, and nothing is factorized again
    assert rel(got["2"][0][:, 0], one[0]) <= XC.TOL and rel(got["2"][1][:, 0], one[1]) <= XC.TOL
    assert b.final_factorizations() == before + 1  # once per run, however many single and multi calls follow
    jlb, jub = b.jacobian_bounds_device()
    np.testing.assert_array_equal(jlb.cpu().numpy(), got["identity"][0]), np.testing.assert_array_equal(jub.cpu().numpy(), got["identity"][1])
    for call in (b.lambdas, lambda: b.solve_adjoint_matrix(case["g"])):  # what stays refused after the same run
        with pytest.raises(Exception, match="regularized run"):
            call()
    # a later unregularized run on the same object: a fresh object's bits (nothing of the damped final factor is left on the handles)
    b, _ = device_run(case, 0, None, False, batch_obj=b, single=True)
    again = b.solve_adjoint_multi(sets["2"])
    assert b.final_factorizations() == before + 2
    fresh, _ = device_run(case, 0, None, False, multi=False)
    want = fresh.solve_adjoint_multi(sets["2"])
    np.testing.assert_array_equal(again[0], want[0]), np.testing.assert_array_equal(again[1], want[1])
    b.close(), fresh.close()


def test_without_the_switch_the_run_is_refused_and_the_switch_is_named(hip, oracle):
    from lexls_amd import capi
    case_name, reg_type, fac, on_device = RUNS["type1_shared"]
    case = LC.build(case_name)
    G = np.repeat(case["g"][:, None, :], 2, axis=1)
    b, _ = device_run(case, reg_type, fac, on_device, multi=False, single=True)
    with pytest.raises(Exception, match="regularized run"):
        b.solve_adjoint_multi(G)
    assert b"lexls_lsi_batch_set_adjoint_regularized_multi" in capi.lib().lexls_last_error()
    assert np.abs(b.solve_adjoint(case["g"])[1]).max() > 1e-3  # (the single call has its own switch, which was on)
    b.set_adjoint_regularized_multi(True)  # (the rule of the last run stands: the next run is the first one served)
    with pytest.raises(Exception, match="regularized run"):
        b.solve_adjoint_multi(G)
    b, _ = device_run(case, 2, fac, False, batch_obj=b)
    with pytest.raises(Exception, match="regularization_type 2"):
        b.solve_adjoint_multi(G)
    b, _ = device_run(case, reg_type, fac, False, batch_obj=b)  # the multi switch alone: the single call is refused, the multi call answers
    with pytest.raises(Exception, match="regularized run"):
        b.solve_adjoint(case["g"])
    assert np.abs(b.solve_adjoint_multi(G)[1]).max() > 1e-3
    one = b.solve_adjoint_multi(G[:, :1])  # (one cotangent stays on the multi entry while the single switch is off)
    np.testing.assert_array_equal(one[1], b.solve_adjoint_multi(G)[1][:, :1])
    b.close()
