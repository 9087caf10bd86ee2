"""getLambda of every instance of a lock-step LexLSI batch (lexls_lsi_batch_get_lambda, LsiBatch.lambdas) and every objective's
multipliers of an equality batch in one call (lexls_lse_multipliers, BatchedLexLSE.multipliers): bit for bit against the oracle-backed
driver's debug output (lexlsi.h:552-605), against the single-problem lexls_lsi_solve_debug, and against nObj ObjectiveSensitivity calls."""
import ctypes as C

import numpy as np
import pytest

from lexls_amd import problems as P

pytestmark = pytest.mark.gpu


def oracle_debug(oracle, n, problems, guesses=None, x0=None, v0=None, **params):
    out = []
    for i, objs in enumerate(problems):
        out.append(oracle.lsi_run_debug(n, objs, active_guess=None if guesses is None else guesses[i], x0=None if x0 is None else x0[i],
                                        v0=None if v0 is None else v0[i], **params))
    return out


def assert_lambdas_equal(got, ref):
    """got: LsiBatch.lambdas(); ref: oracle results"""
    assert len(got) == len(ref)
    for i, (g, o) in enumerate(zip(got, ref)):
        od = o["debug"]["lambda"]
        assert len(g) == len(od)
        for k, (a, b) in enumerate(zip(g, od)):
            np.testing.assert_array_equal(a, b, err_msg=f"instance {i}, objective {k}")


def run_and_compare(hip, oracle, n, problems, guesses=None, x0=None, v0=None, batch_obj=None, **params):
    from lexls_amd import lexlsi
    pk = lexlsi.pack_batch(n, problems)
    b = batch_obj or lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    v0a = None if v0 is None else np.stack([np.concatenate(v) for v in v0])
    r = b.run(pk, active_guess=guesses, x0=None if x0 is None else np.asarray(x0), v0=v0a, **params)
    ref = oracle_debug(oracle, n, problems, guesses, x0, v0, **params)
    for i, o in enumerate(ref):  # the run itself is the oracle's (tests/test_gpu_lsi.py checks it in depth)
        np.testing.assert_array_equal(r["x"][i], o["x"])
        assert r["info"][i]["status"] == o["info"]["status"]
    lam = b.lambdas()
    assert_lambdas_equal(lam, ref)
    return b, r, lam, ref


def stationarity(n, objs, lam_inst):
    """level-wise stationarity of the multipliers: for every LexLSE level k (objective off + k), sum_i lambda_i a_i = 0 over the
    constraints of objectives 0 .. off + k, a_i = row of A (general) or the unit row of the bounded variable (simple bounds)"""
    rows = []
    for o in objs:
        if "var" in o:
            e = np.zeros((len(o["var"]), n))
            e[np.arange(len(o["var"])), np.asarray(o["var"], int)] = 1.0
            rows.append(e)
        else:
            rows.append(np.asarray(o["A"], float))
    M = np.vstack(rows)
    L = np.vstack(lam_inst)  # total x nObj
    off = 1 if "var" in objs[0] else 0
    for j in range(off, len(objs)):
        g = M.T @ L[:, j]
        scale = max(1.0, float(np.max(np.abs(M).T @ np.abs(L[:, j]))))
        assert np.max(np.abs(g)) <= 1e-9 * scale, (j, np.max(np.abs(g)), scale)
    if off:
        assert not np.any(L[:, 0])


def ik_batch(count, seed0=20261000, n=40, dims=(12, 12, 12, 12, 12), perturb=0.0):
    return [P.lsi_problem(seed0 + i, n, dims, perturb=perturb) for i in range(count)]


def test_persistent_launch_ik_shape(hip, oracle):
    """(a) n = 40, 5 x 12 with simple bounds, 256 instances on the default (persistent) path, cold and warm-started as bench --workload lsi;
    a sample against the single-problem debug driver; level-wise stationarity on a few instances"""
    from lexls_amd import lexlsi
    n, count = 40, 256
    base = ik_batch(count)
    b, r, lam, ref = run_and_compare(hip, oracle, n, base)
    for i in (0, 1):
        stationarity(n, base[i], lam[i])
    guess = [[np.where(a == 3, 0, a).astype(np.uint8) for a in np.split(r["active"][i], np.cumsum(b.dims)[:-1])] for i in range(count)]
    pert = ik_batch(count, perturb=0.9)
    b, r2, lam2, ref2 = run_and_compare(hip, oracle, n, pert, guesses=guess, x0=list(r["x"]), batch_obj=b)
    for i in (0, 77, 255):
        d = lexlsi.lsi_solve_debug(n, pert[i], active_guess=guess[i], x0=r["x"][i])["debug"]["lambda"]
        for a, c in zip(lam2[i], d):
            np.testing.assert_array_equal(a, c)
    stationarity(n, pert[5], lam2[5])
    b.close()


@pytest.mark.parametrize("env", ["LEXLS_LSI_NO_FUSED", "LEXLS_LSI_RESIDENT"])
def test_other_run_paths(hip, oracle, monkeypatch, env):
    """(b) the three launches per resident stage, and the host-side active-set logic (lock-step stages)"""
    monkeypatch.setenv(env, "1" if env == "LEXLS_LSI_NO_FUSED" else "0")
    run_and_compare(hip, oracle, 40, ik_batch(256, seed0=20261500))[0].close()


def test_small_shape_cold_and_forced_removals(hip, oracle):
    """(c) n = 20, [6, 5, 5, 6]: cold, and from an all-upper-bound guess that forces removals; with initial residuals v0"""
    n, dims, count = 20, (6, 5, 5, 6), 48
    probs = [P.lsi_problem(700 + i, n, dims) for i in range(count)]
    b = run_and_compare(hip, oracle, n, probs)[0]
    guess = [[np.full(m, 2, np.uint8) for m in dims] for _ in range(count)]
    _, r, _, ref = run_and_compare(hip, oracle, n, probs, guesses=guess, batch_obj=b)
    assert sum(o["info"]["deactivations"] for o in ref) > 0
    v0 = [[0.01 * P.normal(900 + i, m, k) for k, m in enumerate(dims)] for i in range(count)]
    run_and_compare(hip, oracle, n, probs, v0=v0, batch_obj=b)
    b.close()


def test_general_objectives_only(hip, oracle):
    """(d) no simple bounds: every column is a LexLSE objective"""
    n = 20
    probs = [[o for o in P.lsi_problem(800 + i, n, (6, 5, 5, 6)) if "A" in o] for i in range(32)]
    b, _, lam, _ = run_and_compare(hip, oracle, n, probs)
    stationarity(n, probs[0], lam[0])
    b.close()


def test_factorization_limit(hip, oracle):
    """(e) instances stopped short of PROBLEM_SOLVED: the reference re-forms and refactorizes the final working set"""
    probs = ik_batch(64, seed0=20262000)
    _, r, _, ref = run_and_compare(hip, oracle, 40, probs, max_number_of_factorizations=4)
    assert any(o["info"]["status"] != 0 for o in ref)


@pytest.mark.parametrize("dims", [(6, 4, 4, 4, 4, 4, 4), (6, 3, 3, 3, 3, 3, 3, 3, 3, 3), (6, 18, 10)])
def test_deep_and_fallback_shapes(hip, oracle, dims):
    """(f) 7 levels (one sweep), 9 LexLSE objectives and a level of 18 rows (nObj launches of the per-objective kernel)"""
    n = 24
    probs = [P.lsi_problem(900 + i, n, dims) for i in range(24)]
    run_and_compare(hip, oracle, n, probs)[0].close()


@pytest.mark.parametrize("n", [42, 47])
def test_wide_columns(hip, oracle, n):
    """(g) 43-48 columns (the four-per-wavefront kernel serves the resident stages)"""
    run_and_compare(hip, oracle, n, [P.lsi_problem(1000 + i, n, (12, 12, 12, 12, 12)) for i in range(32)])[0].close()


def test_deactivate_first_wrong_sign(hip, oracle):
    """(h) the option that runs instances one by one through the single-problem driver"""
    n, dims = 20, (6, 5, 5, 6)
    probs = [P.lsi_problem(1100 + i, n, dims) for i in range(12)]
    guess = [[np.full(m, 2, np.uint8) for m in dims] for _ in range(12)]
    run_and_compare(hip, oracle, n, probs, guesses=guess, deactivate_first_wrong_sign=1)[0].close()


def test_cycling_and_regularized_runs_report_unsupported(hip):
    """(i) cycling handling relaxes bounds on the host, regularized runs factorize a different problem: documented error code"""
    from lexls_amd import capi, lexlsi
    n, dims = 20, (6, 5, 5, 6)
    pk = lexlsi.pack_batch(n, [P.lsi_problem(1200 + i, n, dims) for i in range(8)])
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    out = np.zeros((pk.batch, len(dims), pk.total))
    for params in (dict(cycling_handling_enabled=1), dict(regularization_type=1, max_number_of_factorizations=40)):
        kw = dict(regularization_factors=np.array([0, 0.1, 0.1, 0.1])) if "regularization_type" in params else {}
        b.run(pk, **kw, **params)
        assert capi.lib().lexls_lsi_batch_get_lambda(b._h, out.ctypes.data_as(C.POINTER(C.c_double))) == 3  # LEXLS_ERR_UNSUPPORTED
    b.run(pk)  # a plain run afterwards has them again
    assert b.lambda_array().shape == (pk.batch, len(dims), pk.total)
    b.close()


def test_second_run_replaces_first(hip, oracle):
    """(j) the multipliers refer to the last run"""
    first, second = ik_batch(16, seed0=20263000), ik_batch(16, seed0=20264000)
    b, _, lam1, _ = run_and_compare(hip, oracle, 40, first)
    _, _, lam2, _ = run_and_compare(hip, oracle, 40, second, batch_obj=b)
    for i in range(16):
        assert np.any(np.vstack(lam2[i])) and not np.array_equal(np.vstack(lam1[i]), np.vstack(lam2[i]))
    b.close()


def test_get_lambda_before_run_is_an_error(hip):
    """(k)"""
    from lexls_amd import capi, lexlsi
    b = lexlsi.LsiBatch(20, [6, 5, 5, 6], [1, 0, 0, 0], 4)
    out = np.zeros((4, 4, 22))
    assert capi.lib().lexls_lsi_batch_get_lambda(b._h, out.ctypes.data_as(C.POINTER(C.c_double))) == 1  # LEXLS_ERR_INVALID
    with pytest.raises(capi.LexlsError):
        b.lambdas()
    b.close()


def test_one_shot_with_lambda(hip, oracle):
    """lsi_batch_solve(..., with_lambda=True) and lexls_lsi_batch_solve_ex2"""
    from lexls_amd import capi, lexlsi
    n, dims = 20, (6, 5, 5, 6)
    probs = [P.lsi_problem(1500 + i, n, dims) for i in range(8)]
    r = lexlsi.lsi_batch_solve(n, probs, with_lambda=True)
    ref = oracle_debug(oracle, n, probs)
    assert_lambdas_equal(r["lambda"], ref)
    pk = lexlsi.pack_batch(n, probs)
    x, info, lam = np.zeros((8, n)), np.zeros((8, 6), np.int32), np.zeros((8, len(dims), pk.total))
    u32 = C.c_uint32

    def dp(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    capi.check(capi.lib().lexls_lsi_batch_solve_ex2(0, u32(8), u32(n), u32(len(dims)), dp(pk.dims, u32), dp(pk.types, C.c_int32), dp(pk.data, C.c_double),
                                                    dp(pk.var_index, u32), None, None, None, None, u32(0), dp(x, C.c_double), dp(info, C.c_int32),
                                                    None, None, None, dp(lam, C.c_double)))
    for i in range(8):
        np.testing.assert_array_equal(lam[i].T, np.vstack(ref[i]["debug"]["lambda"]))


@pytest.mark.parametrize("no_sweep", [False, True])
def test_lse_multipliers_equal_per_objective_sensitivity(hip, monkeypatch, no_sweep):
    """layer 1 on its own: ragged dims, fixed variables, factor kept — multipliers() == nObj ObjectiveSensitivity(k) + getWorkspace(),
    bit for bit; the handle's types are not touched.  Each side runs on the OTHER kernel family: the one-launch sweep against nObj launches of
    sensitivity_kernel, the per-objective fallback (sensitivity_kernel) against nObj launches of the removal sweep"""
    B, n, cap_dims = 96, 20, np.array([6, 5, 7, 6], np.uint32)
    lse = hip.BatchedLexLSE(B, n, cap_dims)
    lse.setProblem(P.lse_batch(4242, B, n, cap_dims))
    rng = np.random.default_rng(5)
    dims = np.stack([[rng.integers(0, c + 1) for c in cap_dims] for _ in range(B)]).astype(np.uint32)
    dims[:, 0] = np.maximum(dims[:, 0], 1)
    lse.setObjDim(dims)
    nfixed = rng.integers(0, 4, B).astype(np.uint32)
    idx = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.uint32)
    val = rng.standard_normal((B, n))
    ftype = rng.integers(1, 4, (B, n)).astype(np.uint8)
    lse.fixVariables(nfixed, idx, val, ftype)
    lse.setCtrType(rng.integers(0, 4, (B, lse.cap)).astype(np.uint8))
    lse.factorize()
    types0 = lse.getCtrType()
    if no_sweep:
        monkeypatch.setenv("LEXLS_SENS_NO_SWEEP", "1")  # (read at every call)
    L = lse.multipliers()
    np.testing.assert_array_equal(lse.getCtrType(), types0)
    assert L.shape == (B, len(cap_dims), n + lse.cap)
    assert np.any(L)
    if no_sweep:
        monkeypatch.delenv("LEXLS_SENS_NO_SWEEP")
    else:
        monkeypatch.setenv("LEXLS_SENS_NO_SWEEP", "1")
    for k in range(len(cap_dims)):
        lse.ObjectiveSensitivity(k)
        np.testing.assert_array_equal(L[:, k, :], lse.getWorkspace(), err_msg=f"objective {k}")
    # the matrices belong to that factor: after a new factorization they are refused until multipliers() runs again
    lse.factorize()
    from lexls_amd import capi
    with pytest.raises(capi.LexlsError):
        capi.check(capi.lib().lexls_lse_get_multipliers(lse._h, L.ctypes.data_as(C.POINTER(C.c_double))))
    np.testing.assert_array_equal(lse.multipliers(), L)
    lse.close()


def near_dependent(seed, n=20, dims=(6, 5, 5, 6), eps=1e-5):
    """lsi_problem whose equality level has a row that repeats another up to eps: its rank depends on tol_linear_dependence"""
    objs = P.lsi_problem(seed, n, dims)
    last = objs[-1]
    last["A"][1] = last["A"][0] + eps * P.normal(seed + 1, n, 77)
    last["lb"][1] = last["ub"][1] = last["lb"][0]
    return objs


def test_deactivate_first_wrong_sign_after_other_runs(hip, oracle):
    """(h) on a batch object that ran before: a regularized run (no multipliers), then one-by-one runs with the default and with a large
    tol_linear_dependence on near-dependent rows — get_lambda factorizes with each run's own parameters, not with what the handles held"""
    n, dims, count = 20, (6, 5, 5, 6), 12
    probs = [near_dependent(1600 + i) for i in range(count)]
    guess = [[np.full(m, 2, np.uint8) for m in dims] for _ in range(count)]
    from lexls_amd import capi, lexlsi
    pk = lexlsi.pack_batch(n, probs)
    b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
    b.run(pk, regularization_factors=np.array([0, 0.1, 0.1, 0.1]), regularization_type=1, max_number_of_factorizations=40)
    out = np.zeros((count, len(dims), pk.total))
    assert capi.lib().lexls_lsi_batch_get_lambda(b._h, out.ctypes.data_as(C.POINTER(C.c_double))) == 3  # LEXLS_ERR_UNSUPPORTED
    _, _, _, ref_default = run_and_compare(hip, oracle, n, probs, guesses=guess, batch_obj=b, deactivate_first_wrong_sign=1)
    _, _, _, ref_tol = run_and_compare(hip, oracle, n, probs, guesses=guess, batch_obj=b, deactivate_first_wrong_sign=1, tol_linear_dependence=1e-3)
    # the tolerance matters on these problems (else this test could not tell the two apart)
    assert any(any(not np.array_equal(a, c) for a, c in zip(o1["debug"]["lambda"], o2["debug"]["lambda"])) for o1, o2 in zip(ref_default, ref_tol))
    b.close()
