"""Every LexLSE factorization kernel family, the consumers of a kept factor and one LexLSI batch held to the oracle on data IN OTHER UNITS: the
cases of tests/scale_cases.py (what the generators are; tests/test_scale_cases.py: the conditions that make the comparison meaningful — the
oracle's own invariance under powers of two, kept / drawn, pivots that the scaling moved, the guard estimates, the consumer tolerances — from the
oracle alone).

Contracts as tests/test_gpu_lse_skip.py::assert_contract applies them: "B" bit for bit (ranks, first columns, total rank, permutation, x, with the
factor kept the Householder scalars and the factor over each problem's own rows), "T" pivots exact and x within test_gpu_qtol.TOL relative to
max(1, |x|_inf), "L" assert_tolerance_contract of tests/test_gpu_large_cases.py.  On `decades` a tolerance-contract problem is allowed
max(test_gpu_qtol.TOL, 100 x its one-ulp sensitivity) x max(1, |x_oracle|_inf), the multiple include/lexls_hip.h states for contract (T) and the
soaks use.  Beyond the contracts, two invariances the oracle has (tests/test_scale_cases.py) are demanded of the kernels themselves: a power
of two on [A | b] with the tolerance moved along changes no bit of x, ranks or permutation of ANY kernel, tolerance-contract ones included —
reciprocal and reciprocal-square-root seeds, Newton steps, fma chains and packed pivot keys are exact under a change of the exponent, so a
difference is a scale-dependent constant or an intermediate narrower than double —, and a power of two per level changes no bit of a bit-exact
kernel's x.  last_kernel() is asserted in every run: none passes on another kernel than the one it names.

MEASURED on MI355X (every test prints its figures; abs = largest |x - x_oracle|, rel = the same over max(1, |x_oracle|_inf) per problem, mult =
largest error / one-ulp sensitivity; every bit-exact family: 0 everywhere, factor and Householder scalars included):
    family                          pow2 (both k)      levels             decades
    lqr_qtol (five instantiations)  abs 4.8e-10        abs 5.6e-11        abs 1.1e-05  rel 1.8e-09  mult 15.9 (qtol_n24; qtol_guard in mode 1: 10.1)
    lqr_mfma (four instantiations)  abs 8.8e-11        abs 6.2e-10        abs 4.7e-05  rel 1.2e-10  mult 9.67 (mfma_two; mfma_four: rel 1.19e-10 at 3.4 x)
    lqr_large<step-per-pivot,mfma>  rel 1.8e-15        rel 3.1e-15        rel 1.2e-12  mult 3.73
Against max(1e-10, 100 x sensitivity): the largest multiple seen is 15.9.  Every tolerance-contract kernel kept the power-of-two invariance: at
k = -100 and k = +100 no entry of x, no rank and no transposition of any of the 23 cases without fixed variables differs from the kernel's own
run at k = 0, and no bit-exact kernel's x moved under the per-level powers of two.  The guard flags 19 of 19 decades problems (estimates 225 ..
3.04e4, the figures the oracle's factor gives).  Consumers on decades, against reference (A): solve_adjoint 2.8e-12, solve_adjoint_multi 2.7e-11
(tolerance 6.1e-11), solve_adjoint_matrix 1.55e-8 (1.55e-7), solve_tangent 1.72e-8 (1.73e-7) — both are the KKT references' own distance from
the restatement on the oracle's factor, the device sits on the latter —, solve_rhs 3.4e-16 (9.5e-11).  LexLSI: both resident paths equal the
oracle-backed driver on all six instances.  No kernel was found wrong, so none was changed.
"""
import numpy as np
import pytest

import adjoint_cases as AC
import scale_cases as SC
import skip_cases as S
import solve_rhs_cases as RH
import test_gpu_qtol as Q
from lexls_amd import lexlsi
from test_gpu_lse_skip import PIVOTS, assert_contract, handle, outputs, run

pytestmark = pytest.mark.gpu

RUNS = SC.runs()
IDS = [SC.run_id(*r) for r in RUNS]
NO_FIXED = [nm for nm in SC.NAMES if S.CASES[nm].get("nfixed") is None]
BIT_EXACT = [nm for nm in SC.NAMES if S.CASES[nm]["contract"] == "B"]
SENS_MULTIPLE = 100.0  # include/lexls_hip.h, contract (T); scripts/soak_qtol.py, scripts/soak_mfma.py


def solve(s, case, lod=None):
    s.setParameters(case["tol"])
    return run(s, case, case["lod"] if lod is None else lod)


def assert_decades_contract(o, case, ctx):
    """contract (T) on badly scaled data: pivots exact; per problem |x - x_oracle|_inf <= max(TOL, 100 x one-ulp sensitivity) x max(1, |x_oracle|_inf).
    Returns (largest relative error, largest error / sensitivity)"""
    ref, sens = case["ref"], case["sens"]
    for k in PIVOTS:
        np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{ctx}: {k}")
    assert np.isfinite(o["x"]).all(), ctx
    err = np.abs(o["x"] - ref["x"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1))
    multiple = float((err / np.maximum(sens, 1e-300)).max())
    print(f"{ctx}: largest |x - x_oracle| {np.abs(o['x'] - ref['x']).max():.3e}, relative {err.max():.3e}, largest error / one-ulp sensitivity {multiple:.3g}")
    bad = err > np.maximum(Q.TOL, SENS_MULTIPLE * sens)
    assert not bad.any(), f"{ctx}: problems {np.flatnonzero(bad).tolist()} err {err[bad].tolist()} sensitivity {sens[bad].tolist()}"
    return float(err.max()), multiple


@pytest.mark.parametrize("name,gen,k", RUNS, ids=IDS)
def test_family_against_the_oracle(hip, name, gen, k):
    case = SC.build(name, gen, k)
    s = handle(hip, case)
    o = solve(s, case)
    ctx = SC.run_id(name, gen, k)
    print(f"{ctx}: {s.last_kernel()}")
    if gen == "decades" and case["contract"] == "T":
        assert_decades_contract(o, case, ctx)
    else:
        assert_contract(o, case, case["ref"], np.arange(len(case["dims"])), ctx, case.get("sens"))
    s.close()


@pytest.mark.parametrize("name", NO_FIXED)
def test_power_of_two_scaling_changes_no_bit_of_x(hip, name):
    """one handle, k = 0, -100, +100: x, ranks, first columns, total rank and permutation of the scaled runs are the kernel's own at k = 0"""
    plain = SC.build(name, "pow2")
    s = handle(hip, plain)
    first = solve(s, plain)
    for k in SC.POW2_K:
        case = SC.build(name, "pow2", k)
        o = solve(s, case)
        for key in PIVOTS:
            np.testing.assert_array_equal(o[key], first[key], err_msg=f"{name}, k = {k}: {key}")
        diff = o["x"].view(np.uint64) != first["x"].view(np.uint64)
        print(f"{name}, k = {k}: {s.last_kernel()}, {int(diff.sum())} entries of x differ from k = 0")
        assert not diff.any(), f"{name}, k = {k}: x of problems {np.flatnonzero(diff.any(axis=1)).tolist()} differs by up to {np.abs(o['x'] - first['x']).max():.3e}"
    s.close()


@pytest.mark.parametrize("name", BIT_EXACT)
def test_level_scaling_changes_no_bit_of_x(hip, name):
    """one handle, the unscaled problems and the same problems with every level in its own power of two: the same x, ranks, first columns,
    total rank and permutation (the tolerance-contract kernels choose pivots per level as well, but their elimination order mixes levels: they
    get the contract in test_family_against_the_oracle)"""
    case = SC.build(name, "levels")
    s = handle(hip, case)
    first = solve(s, case, case["base"])
    o = solve(s, case)
    print(f"{name}: {s.last_kernel()}")
    for key in PIVOTS:
        np.testing.assert_array_equal(o[key], first[key], err_msg=f"{name}: {key}")
    np.testing.assert_array_equal(o["x"].view(np.uint64), first["x"].view(np.uint64), err_msg=f"{name}: x")
    s.close()


def test_guard_on_decades(hip):
    """guard mode 2 on qtol_guard / decades: every problem is badly scaled, so every one is flagged (include/lexls_hip.h: "it flags every badly
    scaled problem too"; tests/test_scale_cases.py: the estimate from the oracle's factor is beyond the threshold for each) and re-solved: bit for
    bit the oracle's; an unflagged problem would be held to test_gpu_qtol.TOL"""
    case = dict(SC.build("qtol_guard", "decades"), guard=2)
    s = handle(hip, case)
    o = solve(s, case)
    est, st, nf = s.get_accuracy()
    flagged = st == 3
    print(f"qtol_guard / decades: {s.last_kernel()}, {int(flagged.sum())} of {len(st)} flagged, estimates {est.min():.3g} .. {est.max():.3g}")
    assert np.isfinite(est).all() and (est >= 0).all()
    assert set(np.unique(st).tolist()) <= {1, 3} and nf == int(flagged.sum())
    ref = case["ref"]
    for k in PIVOTS:
        np.testing.assert_array_equal(o[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(o["x"][flagged], ref["x"][flagged], err_msg="x of a re-solved problem")
    assert np.isfinite(o["x"]).all()
    rest = ~flagged
    if rest.any():
        err = np.abs(o["x"][rest] - ref["x"][rest]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"][rest]).max(axis=1))
        assert (err <= Q.TOL).all(), err
    assert flagged.any()
    assert flagged.all(), f"not flagged: {np.flatnonzero(rest).tolist()}, estimates {est[rest].tolist()}"
    s.close()


@pytest.mark.parametrize("name", S.CONSUMER_CASES, ids=[f"{nm}-decades" for nm in S.CONSUMER_CASES])
def test_consumers_of_a_kept_factor(hip, name):
    """on the decades data of a factor-kept case: multipliers() and solveLeastNorm_1 equal the oracle; solve_adjoint, solve_adjoint_multi,
    solve_adjoint_matrix (differentiable as the rank-stability rule says, exact zeros elsewhere), solve_tangent and solve_rhs within
    scale_cases.CONSUMER_TOL — ten times what the family's two CPU references differ by on these data — of the family's reference (A)"""
    case, want = SC.build(name, "decades"), SC.consumers(name)
    B, K = len(case["dims"]), SC.K_COT
    s = handle(hip, case)
    o = solve(s, case)
    print(f"{name} / decades: {s.last_kernel()}")
    assert_contract(o, case, case["ref"], np.arange(B), f"{name} / decades")
    s.setCtrType(want["types"])
    np.testing.assert_array_equal(s.multipliers(), want["mult"], err_msg="multipliers()")
    tol, G, flags = SC.CONSUMER_TOL, want["G"], want["flags"]
    grad_rhs, grad_fixed = s.solve_adjoint(G[:, 0])
    assert np.isfinite(grad_rhs).all() and not grad_fixed.any()
    gap = max(AC._rel(grad_rhs[b] - want["grad_rhs_A"][b, 0], want["grad_rhs_A"][b, 0]) for b in range(B))
    multi, multi_fixed = s.solve_adjoint_multi(G)
    assert np.isfinite(multi).all() and not multi_fixed.any()
    gap_multi = max(AC._rel(multi[b, j] - want["grad_rhs_A"][b, j], want["grad_rhs_A"][b, j]) for b in range(B) for j in range(K))
    print(f"{name} / decades: solve_adjoint {gap:.2e}, solve_adjoint_multi {gap_multi:.2e} against the unit solves (tolerance {tol['adjoint']:.1e})")
    assert gap <= tol["adjoint"] and gap_multi <= tol["adjoint"]
    Gm, diff = s.solve_adjoint_matrix(G[:, 0])
    np.testing.assert_array_equal(diff, flags, err_msg="differentiable")
    assert np.isfinite(Gm).all() and not Gm[diff == 0].any()
    mgap = max(AC._rel(Gm[b] - want["GA"][b], want["GA"][b]) for b in np.flatnonzero(flags))
    print(f"{name} / decades: solve_adjoint_matrix {mgap:.2e} against the KKT reference on {int(flags.sum())} rank-stable problems of {B} "
          f"(tolerance {tol['adjoint_matrix']:.1e})")
    assert mgap <= tol["adjoint_matrix"]
    dx, tdiff = s.solve_tangent(want["dlod"])
    np.testing.assert_array_equal(tdiff, flags, err_msg="differentiable (tangent)")
    assert np.isfinite(dx).all() and not dx[:, flags == 0].any()
    tgap = max(AC._rel(dx[j, b] - want["TA"][j, b], want["TA"][j, b]) for b in np.flatnonzero(flags) for j in range(K))
    print(f"{name} / decades: solve_tangent {tgap:.2e} against the differentiated KKT system (tolerance {tol['tangent']:.1e})")
    assert tgap <= tol["tangent"]
    x = s.solve_rhs(want["rhs"])
    assert np.isfinite(x).all()
    rgap = RH.rel_rows(x, want["XA"])
    print(f"{name} / decades: solve_rhs {rgap:.2e} against the oracle from scratch (tolerance {tol['solve_rhs']:.1e})")
    assert rgap <= tol["solve_rhs"]
    s.solveLeastNorm_1()
    np.testing.assert_array_equal(s.get_x(), want["ln1"], err_msg="solveLeastNorm_1")
    s.solve()
    np.testing.assert_array_equal(s.get_x(), case["ref"]["x"], err_msg="solve() on the kept factor")
    s.close()


@pytest.mark.parametrize("path", ["persistent", "stages"])
def test_lsi_batch_in_other_units(hip, oracle, monkeypatch, path):
    """six LexLSI instances whose general levels, bounds included, are scaled by powers of two in [-10, 10]: info (iterations, activations,
    deactivations, factorizations, rank), x and the working set equal the oracle-backed driver's, through the persistent launch and through the
    stage path (LEXLS_LSI_NO_FUSED=1, as tests/test_gpu_lsi.py selects it)"""
    if path == "persistent":
        monkeypatch.delenv("LEXLS_LSI_NO_FUSED", raising=False)
    else:
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    probs = SC.lsi_problems()
    pk = lexlsi.pack_batch(SC.LSI_N, probs)
    srv = lexlsi.LsiBatch(SC.LSI_N, pk.dims, pk.types, len(probs))
    try:
        r = srv.run(pk)
        kernel = srv.last_kernel()
    finally:
        srv.close()
    print(f"LexLSI, {path}: {kernel}")
    assert kernel.startswith("lsi_fused<") == (path == "persistent") and kernel.startswith(("lsi_fused<", "lqr_"))
    for i, objs in enumerate(probs):
        o = oracle.lsi_run(SC.LSI_N, objs)
        assert o["info"]["status"] == 0
        assert r["info"][i] == o["info"], i
        np.testing.assert_array_equal(r["x"][i], o["x"], err_msg=str(i))
        np.testing.assert_array_equal(r["active"][i], np.concatenate(o["active"]), err_msg=str(i))
