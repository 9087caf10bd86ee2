"""The ragged instantiations of the tolerance-contract kernel (lexls_amd/csrc/lqr_qtol_impl.h, RAG; lexls_lse_set_kernel_policy(h, 10)): levels of
at most 12 rows, per-problem dimensions, against the CPU oracle through the C ABI.  Acceptance = tests/test_gpu_qtol.py::check, contract (T) of
include/lexls_hip.h: column permutation, ranks, first columns and total rank EXACT, x finite and within 1e-10 relative to max(1, |x|_inf);
last_kernel() is asserted in every case."""
import numpy as np
import pytest

from lexls_amd import problems as P

pytestmark = pytest.mark.gpu

TOL = 1e-10


def ragged_name(n, max_level):
    """the ragged instantiation policy 10 takes: the eight-row pair where no level has more than 8 rows, else the twelve-row trio"""
    md = 8 if max_level <= 8 else 12
    if md == 12 and n == 40:
        return "lqr_qtol<3,12,shift 7,ragged>"
    return f"lqr_qtol<{2 if n + 1 <= 32 else 3},{md},ragged>"


def solve(hip, lod, dims, n, maxdim=None, policy=10, tol=None, guard=None, keep_factor=False, fixed=None):
    dims = np.asarray(dims, np.uint32)
    maxdim = np.asarray(dims.max(axis=0) if (maxdim is None and dims.ndim == 2) else (dims if maxdim is None else maxdim), np.uint32)
    s = hip.BatchedLexLSE(lod.shape[0], n, maxdim)
    s.set_kernel_policy(policy)
    if tol is not None:
        s.setParameters(tol)
    if guard is not None:
        s.set_accuracy_guard(guard)
    if dims.ndim == 2 or not np.array_equal(dims, maxdim):
        s.setObjDim(dims)
    if fixed is not None:
        s.fixVariables(*fixed)
    s.setProblem(lod)
    s.factorize_solve(keep_factor=keep_factor)
    return s


def check(hip, oracle, lod, dims, n, maxdim=None, expect=None, tol=None):
    dims = np.asarray(dims, np.uint32)
    if maxdim is None:
        maxdim = dims.max(axis=0) if dims.ndim == 2 else dims
    maxdim = np.asarray(maxdim, np.uint32)
    ref = oracle.lse_run(lod, dims, n, maxdim=maxdim, nthreads=8, **({} if tol is None else dict(tol=tol)))
    s = solve(hip, lod, dims, n, maxdim, tol=tol)
    assert s.last_kernel() == (expect if expect is not None else ragged_name(n, int(dims.max())))
    r, fc, tr = s.getRanks()
    np.testing.assert_array_equal(r, ref["rank"])
    np.testing.assert_array_equal(fc, ref["fcol"])
    np.testing.assert_array_equal(tr, ref["totalrank"])
    np.testing.assert_array_equal(s.get_column_permutations(), ref["perm"])
    x = s.get_x()
    assert np.isfinite(x).all()
    err = float(np.abs(x - ref["x"]).max())
    print(f"n={n} dims={dims.tolist() if dims.ndim == 1 else 'per problem'} batch={lod.shape[0]} {s.last_kernel()}: max|x - x_oracle| = {err:.3e}")
    assert err <= TOL * max(1.0, float(np.abs(ref["x"]).max()))
    return s, ref


def per_problem_batch(seed, batch, n, dims, cap, slack=0.0):
    """problem b: iid N(0,1) rows packed level after level (sum of its dims rows), `slack` in the rows behind them up to cap"""
    lod = np.full((batch, n + 1, cap), slack)
    for b in range(batch):
        m = int(dims[b].sum())
        lod[b, :, :m] = P.lse_problem(seed + b, n, dims[b])
    return lod


def random_dims(seed, batch, nobj, hi=12):
    return np.minimum((P.uniform(seed, batch * nobj) * (hi + 1)).astype(np.uint32), hi).reshape(batch, nobj)


# ---- 1. uniform short levels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dims", [(40, [6] * 5), (40, [4] * 8), (40, [10] * 4), (24, [6] * 3), (15, [5] * 4), (24, [10, 10, 10]), (36, [9] * 5)])
@pytest.mark.parametrize("batch", [1, 3, 5, 67])
def test_uniform_short_levels(hip, oracle, n, dims, batch):
    """eight-row and twelve-row forms, three and two slots, wavefront tails"""
    check(hip, oracle, P.lse_batch(11000 + 10 * n + batch + len(dims), batch, n, dims), dims, n)


def test_uniform_short_levels_kernel_names(hip, oracle):
    for n, dims, name in ((40, [6] * 5, "lqr_qtol<3,8,ragged>"), (40, [10] * 4, "lqr_qtol<3,12,shift 7,ragged>"), (24, [6] * 3, "lqr_qtol<2,8,ragged>"),
                          (15, [5] * 4, "lqr_qtol<2,8,ragged>"), (24, [10, 10, 10], "lqr_qtol<2,12,ragged>"), (36, [9] * 5, "lqr_qtol<3,12,ragged>")):
        check(hip, oracle, P.lse_batch(11500 + n, 9, n, dims), dims, n, expect=name)


# ---- 2. one hierarchy of mixed sizes for the whole batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[5, 12, 7, 12, 9], [1, 3, 12, 12, 12], [12, 0, 12, 12, 12], [3, 9, 11, 2, 12, 8]])
def test_mixed_hierarchy(hip, oracle, dims):
    """odd row offsets (and odd leading dimensions: 45 rows), an empty level, a one-row level"""
    for batch in (1, 6, 67):
        check(hip, oracle, P.lse_batch(12000 + sum(dims) + batch, batch, 40, dims), dims, 40, expect="lqr_qtol<3,12,shift 7,ragged>")


# ---- 3. per-problem dimensions --------------------------------------------------------------------------------------------------------
PARITY_DIMS = np.array([[8, 8, 8], [3, 0, 5], [1, 8, 2], [0, 0, 4], [8, 1, 0], [5, 5, 5], [2, 2, 2], [7, 3, 8]], np.uint32)


def test_per_problem_dims_of_the_parity_batch(hip, oracle):
    """the eight dims rows of tests/test_gpu_parity.py::test_ragged_batch (n = 20, capacities [8, 8, 8], zeros included)"""
    lod = per_problem_batch(900, 8, 20, PARITY_DIMS, 24)
    check(hip, oracle, lod, PARITY_DIMS, 20, maxdim=[8, 8, 8], expect="lqr_qtol<2,8,ragged>")


def test_per_problem_dims_differ_inside_wavefronts(hip, oracle):
    dims = random_dims(13000, 64, 5)
    assert len({tuple(d) for d in dims[:4]}) == 4
    check(hip, oracle, per_problem_batch(13100, 64, 40, dims, 60), dims, 40, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")


@pytest.mark.parametrize("n,caps", [(14, [2, 7, 3, 2, 7]), (40, [5, 12, 7, 12, 9]), (24, [1, 8, 3, 5])])
def test_odd_capacity_with_problems_that_fill_it(hip, oracle, n, caps):
    """an odd leading dimension, per-problem dimensions, and problems whose rows end exactly at the capacity (every fourth one): the last pair
    of a column starts at its last row — the clamped, straddling read of the ragged loads — with NaN behind the other problems' rows"""
    batch = 67
    dims = np.minimum(random_dims(19000 + n, batch, len(caps)), np.array(caps, np.uint32)[None, :])
    dims[::4] = caps
    assert sum(caps) % 2 == 1
    lod = per_problem_batch(19100 + n, batch, n, dims, sum(caps), np.nan)
    check(hip, oracle, lod, dims, n, maxdim=caps)


def test_the_ragged_batch_of_the_dispatch_rules(hip, oracle):
    """tests/test_gpu_qtol.py::test_dispatch_rules: 63 x [12] x 5 and one [12, 11, 12, 12, 12]"""
    lod = P.lse_batch(31, 64, 40, [12] * 5)
    dims = np.array([[12, 12, 12, 12, 12]] * 63 + [[12, 11, 12, 12, 12]], np.uint32)
    check(hip, oracle, lod, dims, 40, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")


# ---- 4. slack and neighbours are never used -------------------------------------------------------------------------------------------
def test_slack_rows_are_never_used(hip, oracle):
    dims = random_dims(14000, 64, 5)
    zero = per_problem_batch(14100, 64, 40, dims, 60)
    s0, _ = check(hip, oracle, zero, dims, 40, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")
    for slack in (np.nan, 1e300):
        s = solve(hip, per_problem_batch(14100, 64, 40, dims, 60, slack), dims, 40, [12] * 5)
        assert s.last_kernel() == "lqr_qtol<3,12,shift 7,ragged>"
        np.testing.assert_array_equal(s.get_x(), s0.get_x())
        np.testing.assert_array_equal(s.get_column_permutations(), s0.get_column_permutations())
        np.testing.assert_array_equal(s.getRanks()[0], s0.getRanks()[0])


# ---- 5. rank-deficient ragged levels, ties, mixed wavefronts --------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ranks", [([5, 12, 7, 12, 9], [3, 12, 4, 12, 9]), ([6] * 5, [4, 6, 2, 6, 6]), ([1, 3, 12, 12, 12], [1, 2, 7, 12, 3]),
                                        ([3, 9, 11, 2, 12, 8], [3, 5, 11, 1, 6, 8]), ([12, 0, 12, 12, 12], [9, 0, 12, 1, 12])])
def test_rank_deficient_ragged_levels(hip, oracle, dims, ranks):
    lod = np.stack([P.rank_deficient_problem(15000 + sum(ranks) + b, 40, dims, ranks) for b in range(21)])
    check(hip, oracle, lod, dims, 40)


@pytest.mark.parametrize("dims", [[5, 12, 7, 12, 9], [6] * 5])
def test_duplicated_columns_first_maximum_by_position(hip, oracle, dims):
    lod = P.lse_batch(15500 + len(dims), 16, 40, dims)
    lod[:, 7, :] = lod[:, 3, :]
    lod[:, 30, :] = lod[:, 3, :]
    lod[:, 20, :] = lod[:, 19, :]
    lod[:, 39, :] = lod[:, 0, :]
    check(hip, oracle, lod, dims, 40)


def test_mixed_ranks_inside_wavefronts(hip, oracle):
    dims = [5, 12, 7, 12, 9]
    lod = P.lse_batch(15700, 32, 40, dims)
    lod[1::3] = np.stack([P.rank_deficient_problem(15800 + b, 40, dims, [2, 12, 7, 12, 9]) for b in range(32)])[1::3]
    lod[2::5] = np.stack([P.rank_deficient_problem(15900 + b, 40, dims, [5, 12, 1, 12, 9]) for b in range(32)])[2::5]
    check(hip, oracle, lod, dims, 40)


# ---- 6. tolerance zero ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[5, 12, 7, 12, 9], [6] * 5, [4] * 8])
def test_zero_tolerance(hip, oracle, dims):
    """a level ends with its own rows, not with a zero norm that fails a rank test: x finite, ranks those of the oracle at tolerance 0"""
    check(hip, oracle, P.lse_batch(16000 + len(dims), 13, 40, dims), dims, 40, tol=0.0)


# ---- 7. dispatch ----------------------------------------------------------------------------------------------------------------------
def test_dispatch_policy_10(hip, oracle):
    for dims, name in (([12] * 5, "lqr_qtol<3,12,shift 7>"), ([8] * 5, "lqr_qtol<3,8>")):
        lod = P.lse_batch(17000, 8, 40, dims)
        check(hip, oracle, lod, dims, 40, expect=name)
    dims = [5, 12, 7, 12, 9]
    lod = P.lse_batch(17100, 8, 40, dims)
    ref = oracle.lse_run(lod, dims, 40)
    s = solve(hip, lod, dims, 40, keep_factor=True)
    assert not s.last_kernel().startswith("lqr_qtol")
    np.testing.assert_array_equal(s.get_x(), ref["x"])
    nf = np.full(8, 2, np.uint32)
    idx = np.zeros((8, 40), np.uint32)
    idx[:, 1] = 7
    val = np.zeros((8, 40))
    val[:, :2] = [0.25, -1.5]
    s = solve(hip, lod, dims, 40, fixed=(nf, idx, val))
    assert not s.last_kernel().startswith("lqr_qtol")
    np.testing.assert_array_equal(s.get_x(), oracle.lse_run(lod, dims, 40, nfixed=nf, fixed_idx=idx, fixed_val=val)["x"])
    for n2, dims2 in ((44, [5, 12, 7, 12, 9]), (40, [13, 6, 6, 6, 6])):
        lod2 = P.lse_batch(17200, 8, n2, dims2)
        s = solve(hip, lod2, dims2, n2)
        assert not s.last_kernel().startswith("lqr_qtol")
        np.testing.assert_array_equal(s.get_x(), oracle.lse_run(lod2, dims2, n2)["x"])
    # accuracy guard: no estimating ragged form — the bit-exact kernel of the shape, status 0 everywhere
    s = solve(hip, lod, dims, 40, guard=2)
    assert not s.last_kernel().startswith("lqr_qtol")
    est, status, flagged = s.get_accuracy()
    assert (status == 0).all() and flagged == 0
    np.testing.assert_array_equal(s.get_x(), ref["x"])
    # ... and a uniform batch runs the estimating instantiation, as under policy 6
    lod12 = P.lse_batch(17000, 8, 40, [12] * 5)
    s = solve(hip, lod12, [12] * 5, 40, guard=2)
    assert s.last_kernel() == "lqr_qtol<3,12,shift 7,guard>"


def test_other_policies_do_not_take_the_ragged_form(hip, oracle):
    dims = [5, 12, 7, 12, 9]
    lod = P.lse_batch(17300, 8, 40, dims)
    ref = oracle.lse_run(lod, dims, 40)
    for policy in (0, 4, 6):
        s = solve(hip, lod, dims, 40, policy=policy)
        assert not s.last_kernel().startswith("lqr_qtol")
        np.testing.assert_array_equal(s.get_x(), ref["x"])


# ---- 8. full size ---------------------------------------------------------------------------------------------------------------------
def test_full_size_batch_4096_per_problem_dims(hip, oracle):
    dims = random_dims(18000, 4096, 5)
    lod = per_problem_batch(20260100, 4096, 40, dims, 60)
    s, _ = check(hip, oracle, lod, dims, 40, maxdim=[12] * 5, expect="lqr_qtol<3,12,shift 7,ragged>")
    x0 = s.get_x().copy()
    for _ in range(5):
        s.factorize_solve(keep_factor=False)
        np.testing.assert_array_equal(s.get_x(), x0)
