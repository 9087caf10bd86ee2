"""Bounds gradients of batched LexLSI solutions after a REGULARIZED resident run (lexls_lsi_batch_solve_adjoint(_device) once
lexls_lsi_batch_set_adjoint_regularized is on; ensure_final_factor leaves the run's regularization on the groups' handles, the final problems are
factorized damped, and solve_adjoint_reg_kernel differentiates them), on the small batches of tests/lsi_adjoint_cases.py.

Reference, built the way that file builds its own: the oracle driver (oracle.lsi_run with the run's regularization, an instance at a time with its
own factors) gives the final working set; lsi_adjoint_cases.final_problem forms the equality problem; unit solves of the oracle's equality solver on
it WITH the run's type and the levels' factors (adjoint_reg_cases.reference_unit_solves) give M_reg^T g and N_reg^T g; numpy scatters them by
constraint type.  Tolerance: adjoint_reg_cases.TOL (1e-12, from the CPU references' own gap).
A central difference through the whole oracle driver on one active bound of one instance confirms the reference on the CPU side: step 1e-6, the map
is affine while the working set holds, so the difference is exact up to the rounding of x (1e-15 .. 1e-14) over 2e-6 — bound 1e-7.
MEASURED (CPU, oracle alone): central-difference gap on small_sb, instance 2: type 1 shared 2.6e-10, type 1 per instance 2.4e-10, type 3 2.3e-11 (D_CPU of
tests/adjoint_reg_cases.py: 5.8e-14)."""
import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_reg_cases as RC
import lsi_adjoint_cases as LC

pytestmark = pytest.mark.gpu

SHARED = np.array([0.0, 0.3, 0.2])  # per objective of small_sb (objective 0: simple bounds, no LexLSE level, its factor is never read)
# name -> case of lsi_adjoint_cases, regularization type, factors: (nObj,) shared or (batch, nObj) per instance, on the device or not
RUNS = {
    "type1_shared": ("small_sb", 1, SHARED, False),
    "type1_instance_device": ("small_sb", 1, np.array([[0.0, 0.1 + 0.05 * b, 0.4 - 0.07 * b] for b in range(4)]), True),
    "type3_shared": ("small_sb", 3, SHARED, False),
    "type1_general": ("general", 1, np.array([0.25, 0.0, 0.15]), False),  # no simple bounds; an undamped level between damped ones
}


def rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def factors_of(fac, b):
    return fac if fac.ndim == 1 else fac[b]


def oracle_runs(case, reg_type, fac, probs=None):
    from oracle import oracle_ctypes as oracle
    probs = case["probs"] if probs is None else probs
    return [oracle.lsi_run(case["n"], objs, regularization_factors=factors_of(fac, b), regularization_type=reg_type) for b, objs in enumerate(probs)]


def reference(case, reg_type, fac):
    """(grad_lb, grad_ub, runs): lsi_adjoint_cases.reference_a with the damped equality solver in the unit solves"""
    n, probs, g = case["n"], case["probs"], case["g"]
    runs = oracle_runs(case, reg_type, fac)
    B, total = len(probs), sum(len(o["lb"]) for o in probs[0])
    off = 1 if "var" in probs[0][0] else 0
    formed = [LC.final_problem(n, probs[b], runs[b]["active"]) for b in range(B)]
    nf = np.asarray([len(f[3]) for f in formed], np.uint32)
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b, f in enumerate(formed):
        for j, (var, value, _, _) in enumerate(f[3]):
            idx[b, j], val[b, j] = var, value
    lse = dict(n=n, caps=formed[0][2], lod=np.stack([f[0] for f in formed]), dims=np.stack([f[1] for f in formed]), g=np.asarray(g, float),
               fixed=dict(nfixed=nf, fixed_idx=idx, fixed_val=val) if nf.any() else {},
               factors=np.stack([np.asarray(factors_of(fac, b), float)[off:] for b in range(B)]))
    grad_rhs, grad_fixed = RC.reference_unit_solves(lse, reg_type)
    glb, gub = np.zeros((B, total)), np.zeros((B, total))
    for b, f in enumerate(formed):
        if runs[b]["info"]["status"] != LC.SOLVED:
            continue
        for j, (_, _, u, t) in enumerate(f[3]):
            (glb if t == LC.LB else gub)[b, u] = grad_fixed[b, j]
        for r, (u, t) in enumerate(f[4]):
            (glb if t == LC.LB else gub)[b, u] = grad_rhs[b, r]
    return glb, gub, runs


def device_run(case, reg_type, fac, on_device, batch_obj=None, switch=True):
    from lexls_amd import lexlsi
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    b = batch_obj or lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.set_adjoint_regularized(switch)
    params = dict(regularization_type=reg_type)
    if fac is None:
        b.set_instance_regularization(None)
        params = {}
    elif fac.ndim == 2:
        b.set_instance_regularization(torch.from_numpy(fac.copy()).cuda() if on_device else fac)
    else:
        b.set_instance_regularization(None)
        params["regularization_factors"] = fac
    r = b.run(pk, **params)
    return b, r


@pytest.mark.parametrize("name", list(RUNS))
def test_regularized_runs_against_the_damped_unit_solves(hip, oracle, name):
    case_name, reg_type, fac, on_device = RUNS[name]
    case = LC.build(case_name)
    glb_ref, gub_ref, runs = reference(case, reg_type, fac)
    assert max(np.abs(glb_ref).max(), np.abs(gub_ref).max()) > 1e-2
    plain = LC.build(case_name)["A"]
    assert max(np.abs(glb_ref - plain[0]).max(), np.abs(gub_ref - plain[1]).max()) > 1e-3  # the damping shows in the gradient
    b, r = device_run(case, reg_type, fac, on_device)
    assert "regularized" in b.last_kernel(), b.last_kernel()  # the run was resident on a regularized kernel
    active = np.stack([np.concatenate(x["active"]) for x in runs])
    status = np.asarray([x["info"]["status"] for x in runs])
    np.testing.assert_array_equal(r["active"], active)
    np.testing.assert_array_equal([r["info"][i]["status"] for i in range(len(runs))], status)
    before = b.final_factorizations()
    glb, gub = b.solve_adjoint(case["g"])
    print(f"{name}: gap to the reference {max(rel(glb, glb_ref), rel(gub, gub_ref)):.2e} (TOL {RC.TOL:.0e})")
    assert rel(glb, glb_ref) <= RC.TOL and rel(gub, gub_ref) <= RC.TOL
    assert not glb[active != LC.LB].any() and not gub[(active != LC.UB) & (active != LC.EQ)].any()  # exact zeros outside the working set
    assert not glb[status != LC.SOLVED].any() and not gub[status != LC.SOLVED].any()
    # once per run, not per call; the same bits from a second call and from the device form
    glb2, gub2 = b.solve_adjoint(case["g"])
    dlb, dub = b.solve_adjoint_device(torch.from_numpy(case["g"].copy()).cuda())
    assert b.final_factorizations() == before + 1
    np.testing.assert_array_equal(glb2, glb), np.testing.assert_array_equal(gub2, gub)
    np.testing.assert_array_equal(dlb.cpu().numpy(), glb), np.testing.assert_array_equal(dub.cpu().numpy(), gub)
    # what stays refused after the same run
    for call in (b.lambdas, lambda: b.solve_adjoint_multi(np.repeat(case["g"][:, None, :], 2, axis=1)), lambda: b.solve_adjoint_matrix(case["g"])):
        with pytest.raises(Exception, match="regularized run"):
            call()
    # a later unregularized run on the same object: today's bits (nothing of the damped final factor is left on the handles)
    b, _ = device_run(case, 0, None, False, batch_obj=b)
    got = b.solve_adjoint(case["g"])
    assert b.final_factorizations() == before + 2
    fresh, _ = device_run(case, 0, None, False, switch=False)
    want = fresh.solve_adjoint(case["g"])
    np.testing.assert_array_equal(got[0], want[0]), np.testing.assert_array_equal(got[1], want[1])
    assert rel(want[0], plain[0]) <= LC.TOL and rel(want[1], plain[1]) <= LC.TOL
    b.close(), fresh.close()


def test_the_status_rule_under_a_budget(hip, oracle):
    """instances the factorization budget stops do not end PROBLEM_SOLVED: exact zeros, as without regularization"""
    from lexls_amd import lexlsi
    from oracle import oracle_ctypes as orc
    case = LC.build_budget()
    runs = [orc.lsi_run(case["n"], objs, regularization_factors=SHARED, regularization_type=1, max_number_of_factorizations=1) for objs in case["probs"]]
    status = np.asarray([x["info"]["status"] for x in runs])
    assert (status == LC.SOLVED).any() and (status != LC.SOLVED).any()
    pk = lexlsi.pack_batch(case["n"], case["probs"])
    b = lexlsi.LsiBatch(case["n"], pk.dims, pk.types, pk.batch)
    b.set_adjoint_regularized(True)
    r = b.run(pk, regularization_factors=SHARED, regularization_type=1, max_number_of_factorizations=1)
    np.testing.assert_array_equal([r["info"][i]["status"] for i in range(len(runs))], status)
    glb, gub = b.solve_adjoint(case["g"])
    assert not glb[status != LC.SOLVED].any() and not gub[status != LC.SOLVED].any()
    assert np.abs(glb[status == LC.SOLVED]).max() + np.abs(gub[status == LC.SOLVED]).max() > 1e-3
    b.close()


def test_without_the_switch_and_for_the_other_types_the_run_is_refused(hip, oracle):
    case = LC.build("small_sb")
    from lexls_amd import capi
    b, _ = device_run(case, 1, SHARED, False, switch=False)
    with pytest.raises(Exception, match="regularized run"):
        b.solve_adjoint(case["g"])
    assert b"lexls_lsi_batch_set_adjoint_regularized" in capi.lib().lexls_last_error()
    b.set_adjoint_regularized(True)  # (the rule of the last run stands: the next run is the first one served)
    with pytest.raises(Exception, match="regularized run"):
        b.solve_adjoint(case["g"])
    b, _ = device_run(case, 2, SHARED, False, batch_obj=b)
    with pytest.raises(Exception, match="regularization_type 2"):
        b.solve_adjoint(case["g"])
    b, _ = device_run(case, 1, SHARED, False, batch_obj=b)
    assert np.abs(b.solve_adjoint(case["g"])[1]).max() > 1e-3
    assert capi.lib().lexls_lsi_batch_set_adjoint_regularized(None, 1) != 0
    b.close()


@pytest.mark.parametrize("name", ["type1_shared", "type1_instance_device", "type3_shared"])
def test_a_central_difference_through_the_oracle_driver_confirms_the_reference(oracle, name):
    case_name, reg_type, fac, _ = RUNS[name]
    case = LC.build(case_name)
    glb_ref, gub_ref, runs = reference(case, reg_type, fac)
    inst = 2
    active = np.concatenate(runs[inst]["active"])
    grad = np.where(active == LC.LB, glb_ref[inst], gub_ref[inst])
    row = int(np.argmax(np.abs(grad)))  # one active bound of one instance: the one the loss is most sensitive to
    assert active[row] != 0 and abs(grad[row]) > 1e-3
    h, xs = 1e-6, []
    for sign in (+1.0, -1.0):
        lb, ub = LC.bounds_of(case["probs"][inst])
        lb, ub = lb.copy(), ub.copy()
        equality = lb[row] == ub[row]  # moves as one
        if active[row] == LC.LB or equality:
            lb[row] += sign * h
        if active[row] != LC.LB or equality:
            ub[row] += sign * h
        probs = list(case["probs"])
        probs[inst] = LC.with_bounds(case["probs"][inst], lb, ub)
        r = oracle_runs(case, reg_type, fac, probs)[inst]
        assert r["info"]["status"] == LC.SOLVED and np.array_equal(np.concatenate(r["active"]), active)  # the working set holds
        xs.append(r["x"])
    fd = float(case["g"][inst] @ (xs[0] - xs[1])) / (2 * h)
    gap = abs(fd - grad[row]) / max(1.0, abs(grad[row]))
    print(f"{name}: instance {inst}, user row {row}: central difference {fd:.12e}, reference {grad[row]:.12e}, gap {gap:.1e}")
    assert gap <= 1e-7
