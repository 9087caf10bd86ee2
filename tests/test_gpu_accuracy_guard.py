"""The accuracy guard of tolerance-contract x-only solves (lexls_lse_set_accuracy_guard; include/lexls_hip.h, policy comment) against the CPU
oracle.  Mode 1 reports per problem an estimate and a status; mode 2 re-solves the flagged problems on the bit-exact kernel in the same
stream.  Sensitivity = the oracle's one-ulp sensitivity of scripts/calibrate_guard.py (a property of the problem, not of a kernel)."""
import ctypes as C

import numpy as np
import pytest

from lexls_amd import problems as P
from scripts import calibrate_guard as CG

pytestmark = pytest.mark.gpu

N, DIMS = 40, [12] * 5
TOL = 1e-10


def rel_err(x, ref_x):
    return np.abs(x - ref_x).max(axis=1) / np.maximum(1.0, np.abs(ref_x).max(axis=1))


def run(hip, lod, dims=DIMS, n=N, guard=None, threshold=0.0, policy=0):
    s = hip.BatchedLexLSE(lod.shape[0], n, dims)
    s.set_kernel_policy(policy)
    if guard is not None:
        s.set_accuracy_guard(guard, threshold)
    s.setProblem(lod)
    s.factorize_solve(keep_factor=False)
    return s


def outputs(s):
    r, fc, tr = s.getRanks()
    return dict(x=s.get_x(), rank=r, fcol=fc, totalrank=tr, perm=s.get_column_permutations())


@pytest.fixture(scope="module")
def ill_sets(oracle):
    """the ill-conditioned calibration sets with their oracle results and one-ulp sensitivities"""
    out = []
    for i, (name, lod) in enumerate(CG.guard_sets()):
        if name == "configs[2]":
            continue
        ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
        out.append((name, lod, ref, CG.sensitivity(lod, DIMS, N, ref, seed=i)))
    return out


def test_guard_off_changes_nothing(hip):
    lod = P.lse_batch_fast(20261110, 257, N, DIMS)
    a = run(hip, lod)
    b = run(hip, lod, guard=0)
    assert a.last_kernel() == b.last_kernel() == "lqr_qtol<3,12,shift 7>"
    oa, ob = outputs(a), outputs(b)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k
    # switched on and off again: the unguarded kernel, nothing reported
    c = run(hip, lod, guard=1)
    c.set_accuracy_guard(0)
    c.factorize_solve(keep_factor=False)
    assert c.last_kernel() == a.last_kernel()
    assert np.array_equal(c.get_x(), oa["x"])
    est, st, nf = c.get_accuracy()
    assert nf == 0 and not st.any() and not est.any()


def test_configs2_flags_nothing(hip, oracle):
    lod = P.lse_batch(20260100, 4096, N, DIMS)
    a = run(hip, lod)
    oa = outputs(a)
    for mode in (1, 2):
        g = run(hip, lod, guard=mode)
        assert g.last_kernel() == "lqr_qtol<3,12,shift 7,guard>"
        est, st, nf = g.get_accuracy()
        assert nf == 0 and (st == 1).all()
        assert np.isfinite(est).all() and (est > 0.5).all() and est.max() < 64.0
        og = outputs(g)
        for k in oa:  # mode 2 with nothing flagged: the re-solve leaves every problem alone
            assert np.array_equal(oa[k], og[k]), (mode, k)
    # the in-kernel estimate is the calibration script's, computed from the oracle's factor, up to the kernel's rounding
    ref = oracle.lse_run(lod[:512], DIMS, N, nthreads=8)
    np.testing.assert_allclose(est[:512], CG.estimate(lod[:512], DIMS, N, ref), rtol=1e-9)


def test_estimate_matches_the_calibration_on_ill_conditioned_data(hip, ill_sets):
    name, lod, ref, sens = ill_sets[1]  # near-dependent 1e-4: estimates up to ~3e4
    est = run(hip, lod, guard=1).get_accuracy()[0]
    np.testing.assert_allclose(est, CG.estimate(lod, DIMS, N, ref), rtol=1e-3, err_msg=name)


def test_mode1_no_false_negatives(hip, ill_sets):
    beyond = 0
    for name, lod, ref, sens in ill_sets:
        plain = run(hip, lod)
        beyond += int((rel_err(plain.get_x(), ref["x"]) > TOL).sum())
        g = run(hip, lod, guard=1)
        est, st, nf = g.get_accuracy()
        flagged = st == 2
        assert set(np.unique(st)) <= {1, 2}, name
        assert nf == int(flagged.sum())
        missed = (sens > 1e-11) & ~flagged
        assert not missed.any(), f"{name}: sensitive problems not flagged {np.flatnonzero(missed)[:8]} (estimates {est[missed][:8]})"
        err = rel_err(g.get_x(), ref["x"])
        assert (err[~flagged] <= TOL).all(), f"{name}: unflagged problem beyond {TOL}: {err[~flagged].max():.3e}"
        # the estimating instantiation computes the same (T) answer as the shipped one
        assert np.array_equal(g.get_x(), plain.get_x()), name
    print(f"unguarded lqr_qtol beyond {TOL} on {beyond} problems of the ill-conditioned sets")
    assert beyond > 0, "the sets do not exercise the guard"


def test_mode2_resolves_flagged_bit_exact(hip, ill_sets):
    for name, lod, ref, sens in ill_sets:
        m1 = outputs(run(hip, lod, guard=1))
        g = run(hip, lod, guard=2)
        est, st, nf = g.get_accuracy()
        assert set(np.unique(st)) <= {1, 3}, name
        f = st == 3
        assert nf == int(f.sum()) and not ((sens > 1e-11) & ~f).any(), name
        o = outputs(g)
        for k in ("x", "rank", "fcol", "perm", "totalrank"):
            assert np.array_equal(o[k][f], ref[k][f]), f"{name}: {k} of a re-solved problem differs from the oracle"
            assert np.array_equal(o[k][~f], m1[k][~f]), f"{name}: {k} of an unflagged problem differs from mode 1"
        assert (rel_err(o["x"], ref["x"]) <= TOL).all(), name


def test_mode2_threshold_splitting_a_set(hip, ill_sets):
    """a threshold at the median estimate: half the problems re-solved, in every ballot group and wavefront of the batch, the other half untouched"""
    for name, lod, ref, sens in ill_sets:
        m0 = outputs(run(hip, lod))
        est1 = run(hip, lod, guard=1).get_accuracy()[0]
        thr = float(np.median(est1))
        want = ~(est1 < thr)
        assert 0 < want.sum() < lod.shape[0]
        g = run(hip, lod, guard=2, threshold=thr)
        est, st, nf = g.get_accuracy()
        assert np.array_equal(est, est1) and np.array_equal(st == 3, want) and (st[~want] == 1).all() and nf == int(want.sum()), name
        o = outputs(g)
        for k in ("x", "rank", "fcol", "perm", "totalrank"):
            assert np.array_equal(o[k][want], ref[k][want]), f"{name}: {k} of a re-solved problem differs from the oracle"
            assert np.array_equal(o[k][~want], m0[k][~want]), f"{name}: {k} of a problem left alone differs from the unguarded solve"


def test_mode2_mixed_batch(hip, oracle):
    """well-conditioned problems with near-dependent ones spliced in at known places: the first and last problem, neighbours inside one
    wavefront, different 64-problem ballot groups, the partial last wavefront (1023 = 255 x 4 + 3)"""
    batch = 1023
    idx = np.array([0, 3, 64, 65, 130, 257, 511, 700, 1020, 1022])
    lod = P.lse_batch_fast(20261160, batch, N, DIMS)
    lod[idx] = P.near_dependent_batch(20261161, idx.size, N, DIMS, 1e-6)
    ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
    want = np.zeros(batch, bool)
    want[idx] = True
    assert np.array_equal(CG.estimate(lod, DIMS, N, ref) >= 64.0, want)  # (the construction does what it says)
    m0 = outputs(run(hip, lod))
    m1 = run(hip, lod, guard=1)
    est1, st1, nf1 = m1.get_accuracy()
    assert nf1 == idx.size and np.array_equal(st1 == 2, want) and (st1[~want] == 1).all()
    o1 = outputs(m1)
    g = run(hip, lod, guard=2)
    est, st, nf = g.get_accuracy()
    assert nf == idx.size and np.array_equal(st == 3, want) and (st[~want] == 1).all() and np.array_equal(est, est1)
    o = outputs(g)
    for k in ("x", "rank", "fcol", "perm", "totalrank"):
        assert np.array_equal(o[k][want], ref[k][want]), f"{k} of a re-solved problem differs from the oracle"
        assert np.array_equal(o[k][~want], m0[k][~want]), f"{k} of a problem left alone differs from the unguarded solve"
        assert np.array_equal(o1[k], m0[k]), f"{k}: mode 1 changes a result"
    assert (rel_err(o["x"], ref["x"]) <= TOL).all()


# (n, dims, guarded lqr_qtol instantiation): the re-solve takes the four-per-wavefront instantiation policy 4 takes
SHAPES = [(20, [12] * 3, "lqr_qtol<2,12,guard>"), (35, [12] * 4, "lqr_qtol<3,12,guard>"), (40, [8] * 5, "lqr_qtol<3,8,guard>"),
          (12, [8] * 3, "lqr_qtol<2,8,guard>"), (40, [12] * 5, "lqr_qtol<3,12,shift 7,guard>")]


@pytest.mark.parametrize("batch", [1, 5, 1023])
@pytest.mark.parametrize("n,dims,kernel", SHAPES)
def test_mode2_every_problem_flagged_equals_policy4(hip, oracle, n, dims, kernel, batch):
    lod = P.near_dependent_batch(20261120 + batch + n, batch, n, dims, 1e-3)
    p4 = outputs(run(hip, lod, dims, n, policy=4))
    g = run(hip, lod, dims, n, guard=2, threshold=1e-300)
    assert g.last_kernel() == kernel
    est, st, nf = g.get_accuracy()
    assert nf == batch and (st == 3).all() and (est > 0).all()
    o = outputs(g)
    for k in o:
        assert np.array_equal(o[k], p4[k]), k
    ref = oracle.lse_run(lod, dims, n, nthreads=8)
    assert np.array_equal(o["x"], ref["x"]) and np.array_equal(o["perm"], ref["perm"])
    # mode 1 with the same threshold: everything flagged, nothing re-solved
    m1 = run(hip, lod, dims, n, guard=1, threshold=1e-300)
    assert (m1.get_accuracy()[1] == 2).all()


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.6", "libamdhip64.so.7"):
        try:
            return C.CDLL(name)
        except OSError:
            pass
    pytest.fail("the HIP runtime library is not loadable")


def test_mode2_deferred_sync_on_user_stream(hip):
    lod = P.near_dependent_batch(20261130, 777, N, DIMS, 1e-5)
    sync = outputs(run(hip, lod, guard=2))
    rt = hip_runtime()
    stream = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(stream)) == 0
    s = hip.BatchedLexLSE(lod.shape[0], N, DIMS)
    s.set_stream(stream.value)
    s.set_accuracy_guard(2)
    from lexls_amd import capi
    capi.check(capi.lib().lexls_lse_set_deferred_sync(s._h, C.c_int(1)))
    s.setProblem(lod)
    s.factorize_solve(keep_factor=False)
    x = s.get_x()  # enqueued only
    s.synchronize()
    assert np.array_equal(x, sync["x"])
    est, st, nf = s.get_accuracy()
    assert nf > 0 and (st[st != 1] == 3).all()
    capi.check(capi.lib().lexls_lse_set_deferred_sync(s._h, C.c_int(0)))
    o = outputs(s)
    for k in o:
        assert np.array_equal(o[k], sync[k]), k
    s.close()
    assert rt.hipStreamDestroy(stream) == 0


def test_automatic_mfma_shape_takes_the_bit_exact_kernel(hip, oracle):
    """n = 41, [12] x 3: four lqr_qtol slices per wavefront do not fit one CU's LDS, two lqr_mfma ones do — automatic dispatch takes lqr_mfma;
    with the guard on, the bit-exact kernel of the shape"""
    n, dims = 41, [12] * 3
    lod = P.near_dependent_batch(20261141, 300, n, dims, 1e-5)
    assert run(hip, lod, dims, n).last_kernel() == "lqr_mfma<32,12>"
    ref = oracle.lse_run(lod, dims, n, nthreads=8)
    for mode in (1, 2):
        g = run(hip, lod, dims, n, guard=mode)
        assert g.last_kernel() == "lqr_quad<3,12>"
        est, st, nf = g.get_accuracy()
        assert nf == 0 and not st.any() and not est.any()
        o = outputs(g)
        for k in ("x", "rank", "fcol", "perm", "totalrank"):
            assert np.array_equal(o[k], ref[k]), k


@pytest.mark.parametrize("policy", [7, 8])
def test_mfma_solves_take_the_bit_exact_kernel(hip, oracle, policy):
    # the matrix-core tolerance-contract kernel (here by policy; automatic dispatch takes it where lqr_qtol's slices do not fit) gives way
    lod = P.near_dependent_batch(20261140, 300, N, DIMS, 1e-5)
    assert run(hip, lod, policy=policy).last_kernel().startswith("lqr_mfma")
    ref = oracle.lse_run(lod, DIMS, N, nthreads=8)
    for mode in (1, 2):
        g = run(hip, lod, guard=mode, policy=policy)
        assert g.last_kernel().startswith("lqr_quad"), g.last_kernel()
        est, st, nf = g.get_accuracy()
        assert nf == 0 and not st.any() and not est.any()
        o = outputs(g)
        for k in ("x", "rank", "fcol", "perm", "totalrank"):
            assert np.array_equal(o[k], ref[k]), k


def test_large_path_takes_the_multi_launch_kernel(hip, oracle):
    """beyond one CU's LDS: the step-per-pivot path (tolerance contract) gives way to the bit-exact multi-launch path, status 0"""
    n, dims = 150, [90, 90, 90]
    lod = P.lse_batch(77, 2, n, dims)
    assert run(hip, lod, dims, n).last_kernel().startswith("lqr_large<step-per-pivot")
    ref = oracle.lse_run(lod, dims, n)
    g = run(hip, lod, dims, n, guard=2)
    assert g.last_kernel() == "lqr_large<multi-launch>"
    est, st, nf = g.get_accuracy()
    assert nf == 0 and not st.any() and not est.any()
    o = outputs(g)
    for k in ("x", "rank", "fcol", "perm", "totalrank"):
        assert np.array_equal(o[k], ref[k]), k


def test_factor_keeping_solves_report_status_0(hip, oracle):
    lod = P.near_dependent_batch(20261150, 64, N, DIMS, 3e-6)
    s = hip.BatchedLexLSE(64, N, DIMS)
    s.set_accuracy_guard(2)
    s.setProblem(lod)
    s.factorize_solve(keep_factor=True)
    est, st, nf = s.get_accuracy()
    assert nf == 0 and not st.any()
    assert np.array_equal(s.get_x(), oracle.lse_run(lod, DIMS, N, nthreads=8)["x"])
