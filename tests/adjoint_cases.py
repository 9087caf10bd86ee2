"""Cases that hold the adjoint of the LexLSE solve (lexls_lse_solve_adjoint, lexls_amd/csrc/lse_adjoint.hip: solve_adjoint_kernel) to two
references, both built from oracle.oracle_ctypes.lse_run alone (tests/test_adjoint_cases.py asserts on the CPU that they agree;
tests/test_gpu_lse_adjoint.py compares the device with them).

factorize() chooses pivots and tests ranks on the columns of A alone, so for fixed A the basic solution is exactly affine:
x = M b + N x_fixed.  With g = dloss/dx the adjoint is grad_rhs = M^T g, grad_fixed = N^T g.
    reference (A)  M and N by unit solves on the oracle — b = 0, x_fixed = 0, then every e_i, then every fixed unit value — and M^T g, N^T g
                   in numpy.  Independent of how the adjoint is computed.
    reference (B)  a numpy restatement of the kernel's steps on the oracle's factor (adjoint_from_factor).
    identities     the large cases (no unit solves: too many rows): <g, x(b1) - x(b0)> = <grad_rhs, b1 - b0> for three random pairs, the
                   forward solves by the oracle.

Cases — the smallest shapes at which each branch can go wrong:
    base        n = 3 (2, 2, 3), full rank
    used_up     n = 4 (3, 3, 3): the columns are used up before the last level
    one_row     n = 5 (1, 3, 2): a one-row level, R == 1, no reflector
    rank_def    n = 7 (3, 3, 3), P.rank_deficient_problem with ranks (2, 0, 2): a rank-0 level and levels of rank < dim
    ragged      n = 5, capacities (2, 3, 2), per-problem dimensions with empty levels: the absent rows of grad_rhs are 0
    fixed       n = 5 (2, 2, 3): nfixed = 2 with indices (1, 0) (factorize() re-maps fixed_var_index), (3, 1), every variable fixed, one variable
    ik          n = 40, 5 x 12, batch 8: the project's own workload
    wide        n = 70 (20, 40, 30): more than 64 columns, a second trip of the lanes over the variables — (B) + identities
    large       edges127, the smallest case of tests/large_cases.py (n = 127, [100, 1, 0, 40, 24], rank-deficient, a one-row and an empty
                level; reflectors over more than 64 rows and 65 rows below level 0: a second trip of the lanes over the rows), under kernel
                policy 5: the large path's kept factor — (B) + identities
Fixed variables at the other edges (reference (A), the unit solves, for all four):
    fixed_wide      n = 70 (20, 40, 30), batch 3, nfixed (6, 9, 0), indices a prefix of a fixed permutation: step (d)'s second and third groups
                    of four fixed columns on live data, its dot products over 90 > 64 rows, step (a) with pivot columns [nf, T) at n > 64, a
                    problem without fixed variables beside two with
    fixed_rank_def  n = 7 (3, 3, 3), ranks (2, 0, 2) behind nfixed (2, 1, 3): a rank-0 level and rank < dim behind fixed columns, another T
                    per problem
    fixed_ragged    n = 5, capacities (2, 3, 2), the dimensions of `ragged`, nfixed (2, 0, 4, 1): empty levels, one free variable, a level
                    that finds the columns used up (its first column >= T)
    fixed_tall      n = 12 (70, 30), batch 2, nfixed (5, 7): reflectors over 70 rows, a Gauss step and step (d) over 100 rows, the second
                    level at rank 0 because the columns are gone

D_CPU is the largest discrepancy the CPU test finds — (A) against (B), and both sides of the identities with (B)'s grad_rhs — each relative to
max(1, largest magnitude of the reference).  The GPU tolerance is TOL = max(10 * D_CPU, 1e-12): the factor 10 allows for fma contraction and
summation orders that differ from numpy's.  It has to stay at or below 1e-10, the project's tolerance contract; data that would need more are
too ill-conditioned and get replaced, the tolerance is not raised.
MEASURED (`python tests/adjoint_cases.py`, the oracle and numpy alone; gap = the case's largest discrepancy):
    base            n=3    [2,2,3]            batch 4  ranks [2,1,0] x 4                                   gap 2.2e-16
    used_up         n=4    [3,3,3]            batch 4  ranks [3,1,0] x 4                                   gap 2.2e-16
    one_row         n=5    [1,3,2]            batch 4  ranks [1,3,1] x 4                                   gap 2.2e-16
    rank_def        n=7    [3,3,3]            batch 3  ranks [2,0,2] x 3                                   gap 2.2e-16
    ragged          n=5    [2,3,2]            batch 4  ranks [2,3,0] [2,0,2] [1,3,0] [0,3,2]               gap 3.8e-16
    fixed           n=5    [2,2,3]            batch 4  ranks [2,1,0] [2,1,0] [0,0,0] [2,2,0]               gap 6.7e-16
    ik              n=40   [12,12,12,12,12]   batch 8  ranks [12,12,12,4,0] x 8                            gap 1.2e-15
    wide            n=70   [20,40,30]         batch 3  ranks [20,40,10] x 3                                gap 2.8e-16
    large           n=127  [100,1,0,40,24]    batch 2  ranks [17,1,0,5,10] [9,0,0,16,8]                    gap 1.6e-16
    fixed_wide      n=70   [20,40,30]         batch 3  ranks [20,40,4] [20,40,1] [20,40,10]                gap 2.6e-15
    fixed_rank_def  n=7    [3,3,3]            batch 3  ranks [2,0,2] x 3                                   gap 1.1e-15
    fixed_ragged    n=5    [2,3,2]            batch 4  ranks [2,1,0] [2,0,2] [1,0,0] [0,3,1]               gap 2.0e-16
    fixed_tall      n=12   [70,30]            batch 2  ranks [7,0] [5,0]                                   gap 2.2e-16
    D_CPU = 2.58e-15 (fixed_wide)  ->  TOL = max(10 D_CPU, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lexls_amd import problems as P  # noqa: E402
from oracle import oracle_ctypes as oracle  # noqa: E402

D_CPU = 2.58e-15  # measured: the table above (tests/test_adjoint_cases.py re-measures it and asserts that TOL still follows from it)
TOL = max(10.0 * D_CPU, 1e-12)

RAGGED_DIMS = np.array([[2, 3, 2], [2, 0, 2], [1, 3, 0], [0, 3, 2]], np.uint32)
WIDE_ORDER = [(37 * j + 11) % 70 for j in range(70)]  # a fixed permutation of the 70 variables of fixed_wide (37 and 70 are coprime)

# name -> n, dims (capacities), batch, seed; fixed: per problem the indices of its fixed variables, in fixVariables order (their number is nfixed);
# ranks: P.rank_deficient_problem; per_problem: ragged dimensions; large: reference (B) + identities instead of the unit solves
CASES = {
    "base": dict(n=3, dims=[2, 2, 3], batch=4, seed=20290101),
    "used_up": dict(n=4, dims=[3, 3, 3], batch=4, seed=20290102),
    "one_row": dict(n=5, dims=[1, 3, 2], batch=4, seed=20290103),
    "rank_def": dict(n=7, dims=[3, 3, 3], batch=3, seed=20290104, ranks=[2, 0, 2]),
    "ragged": dict(n=5, dims=[2, 3, 2], batch=4, seed=20290105, per_problem=RAGGED_DIMS),
    "fixed": dict(n=5, dims=[2, 2, 3], batch=4, seed=20290106, fixed=[[1, 0], [3, 1], [2, 0, 4, 1, 3], [4]]),
    "ik": dict(n=40, dims=[12] * 5, batch=8, seed=20290107),
    "wide": dict(n=70, dims=[20, 40, 30], batch=3, seed=20290108, large=True),
    "large": dict(n=127, dims=[100, 1, 0, 40, 24], batch=2, seed=20280106, large=True, large_case="edges127"),
    "fixed_wide": dict(n=70, dims=[20, 40, 30], batch=3, seed=20310101, fixed=[WIDE_ORDER[:6], WIDE_ORDER[:9], []]),
    "fixed_rank_def": dict(n=7, dims=[3, 3, 3], batch=3, seed=20310102, ranks=[2, 0, 2], fixed=[[4, 1], [6], [0, 5, 2]]),
    "fixed_ragged": dict(n=5, dims=[2, 3, 2], batch=4, seed=20310103, per_problem=RAGGED_DIMS, fixed=[[3, 0], [], [4, 2, 0, 1], [2]]),
    "fixed_tall": dict(n=12, dims=[70, 30], batch=2, seed=20310104, fixed=[[7, 2, 11, 0, 5], [1, 9, 4, 10, 6, 3, 8]]),
}

# case -> kernel policy -> the producer of the kept factor: every policy that gives the shape a distinct one (register-resident: lqr_wave;
# four-per-wavefront: lqr_quad; left-looking: lqr_lwave; bit-exact large: lqr_large<multi-launch>).  The names are the host-side dispatch plan's
# (lexls_amd/csrc/lexls_dispatch.h); tests/test_adjoint_multi_cases.py holds them to it on the CPU, tests/test_gpu_lse_adjoint.py on the device
QUAD1, GENERIC64, GENERIC256, LWAVE = "lqr_quad<1,12,factor>", "lqr_generic<64,lds>", "lqr_generic<256,lds>", "lqr_lwave<41,12>"
SMALL = {0: QUAD1, 1: GENERIC64, 3: LWAVE}
SMALL_FIXED = {0: "lqr_wave<41,12>", 1: GENERIC64, 4: "lqr_quad<3,12,factor,fixed>"}
PRODUCERS = {
    "base": SMALL, "used_up": SMALL, "one_row": SMALL, "rank_def": SMALL, "ragged": SMALL,
    "fixed": SMALL_FIXED,
    "ik": {0: "lqr_wave<41,12,exact>", 3: "lqr_lwave<41,12,exact>", 4: "lqr_quad<3,12,shift 7,factor>", 1: GENERIC64},
    "wide": {0: GENERIC256},
    "large": {5: "lqr_large<multi-launch>", 1: "lqr_generic<1024,hbm>"},
    "fixed_wide": {0: GENERIC256}, "fixed_rank_def": SMALL_FIXED, "fixed_ragged": SMALL_FIXED, "fixed_tall": {0: GENERIC256},
}


def _rel(err, ref):
    return float(np.abs(err).max()) / max(1.0, float(np.abs(ref).max())) if np.size(err) else 0.0


def draw(name):
    """inputs of a case: n, caps, lod (batch, n + 1, cap), dims (batch, nObj), fixed (keyword arguments of oracle.lse_run, {} without fixed
    variables), g (batch, n)"""
    c = CASES[name]
    n, caps, seed, B = c["n"], list(c["dims"]), c["seed"], c["batch"]
    dims = np.tile(np.asarray(caps, np.uint32), (B, 1))
    if c.get("large_case"):
        import large_cases as LC
        lod, dims = LC.draw(c["large_case"])
        lod, dims = lod.copy(), dims.copy()
    elif c.get("ranks"):
        lod = np.stack([P.rank_deficient_problem(seed + b, n, caps, c["ranks"]) for b in range(B)])
    elif c.get("per_problem") is not None:
        dims = c["per_problem"].copy()
        lod = np.stack([P.lse_problem(seed + b, n, dims[b], caps) for b in range(B)])
    else:
        lod = P.lse_batch(seed, B, n, caps)
    fixed = {}
    if c.get("fixed"):  # with any of the draws above: the fixed variables are columns of whatever matrix was drawn
        idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
        nfix = [len(c["fixed"][b]) for b in range(B)]
        for b in range(B):
            idx[b, :nfix[b]] = c["fixed"][b]
            val[b, :nfix[b]] = P.normal(seed + 500 + b, n)[:nfix[b]]
        fixed = dict(nfixed=np.asarray(nfix, np.uint32), fixed_idx=idx, fixed_val=val)
    g = P.normal(seed + 900, B * n).reshape(B, n)
    return dict(name=name, n=n, caps=caps, lod=lod, dims=dims, fixed=fixed, g=g, large=bool(c.get("large")))


def _solve(case, rhs, fixed_val=None):
    """the oracle's x for the case's matrices under other right-hand sides (batch, cap) and fixed values"""
    lod = case["lod"].copy()
    used = np.arange(lod.shape[2])[None, :] < case["dims"].sum(axis=1)[:, None]
    lod[:, case["n"], :] = np.where(used, rhs, lod[:, case["n"], :])
    fixed = dict(case["fixed"])
    if fixed:
        fixed["fixed_val"] = fixed_val if fixed_val is not None else np.zeros_like(fixed["fixed_val"])
    return oracle.lse_run(lod, case["dims"], case["n"], maxdim=np.asarray(case["caps"], np.uint32), nthreads=4, **fixed)


def reference_unit_solves(case):
    """reference (A): (grad_rhs (batch, cap), grad_fixed (batch, n)) from M and N by unit solves"""
    n, B, cap = case["n"], case["lod"].shape[0], sum(case["caps"])
    m = case["dims"].sum(axis=1)
    x0 = _solve(case, np.zeros((B, cap)))["x"]
    grad_rhs, grad_fixed = np.zeros((B, cap)), np.zeros((B, n))
    for i in range(cap):
        e = np.zeros((B, cap))
        e[:, i] = 1.0
        col = _solve(case, e)["x"] - x0                       # column i of M, every problem at once
        grad_rhs[:, i] = np.where(i < m, (col * case["g"]).sum(axis=1), 0.0)
    if case["fixed"]:
        nf = case["fixed"]["nfixed"]
        for j in range(int(nf.max())):
            val = np.zeros((B, n))
            val[:, j] = 1.0
            col = _solve(case, np.zeros((B, cap)), val)["x"] - x0  # column j of N
            grad_fixed[:, j] = np.where(j < nf, (col * case["g"]).sum(axis=1), 0.0)
    return grad_rhs, grad_fixed


def adjoint_from_factor(factor, hh, perm, rank, fcol, totalrank, dims, nf, g):
    """reference (B) for ONE problem: the steps of solve_adjoint_kernel in numpy on a kept factor — factor (n + 1, cap) as get_lexqr() gives
    it.  Returns (grad_rhs (cap,), grad_fixed (n,))"""
    W = factor.T  # W[row, column]
    cap, n, nobj = W.shape[0], len(g), len(dims)
    M, T = int(np.sum(dims)), int(totalrank)
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    gh = np.zeros(n)
    for i in range(n):  # (a) gh = P^T g
        p = i
        for k in range(T):
            pk = int(perm[k])
            p = pk if p == k else (k if p == pk else p)
        gh[p] = g[i]
    cb = np.zeros(cap)
    levels = [(k, int(first[k]), int(fcol[k]), int(dims[k]), int(rank[k])) for k in range(nobj) if nf < n and rank[k] > 0]
    for k, F, Fc, dim, r in levels:  # (b) the reverse of solve()
        y = np.zeros(r)
        for i in range(r):
            y[i] = (gh[Fc + i] - W[F:F + i, Fc + i] @ y[:i]) / W[F + i, Fc + i]
        cb[F:F + r] = y
        gh[Fc + r:T] -= W[F:F + r, Fc + r:T].T @ y
    for k, F, Fc, dim, r in reversed(levels):  # (c) the reverse of the right-hand-side updates of factorize()
        if k < nobj - 1:
            cb[F:F + r] -= W[F + dim:M, Fc:Fc + r].T @ cb[F + dim:M]
        for j in range(r - 1, -1, -1):
            tau = hh[F + j]
            if dim - j == 1 or tau == 0.0:
                continue
            v = np.concatenate([[1.0], W[F + j + 1:F + dim, Fc + j]])
            seg = cb[F + j:F + dim]
            seg -= tau * v * (v @ seg)
    grad_fixed = np.zeros(n)
    grad_fixed[:nf] = gh[:nf] - W[:M, :nf].T @ cb[:M]  # (d)
    return cb, grad_fixed


def reference_from_factor(case, ref):
    B = case["lod"].shape[0]
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    out = [adjoint_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b],
                               int(nf[b]), case["g"][b]) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def identity_gap(pair, g, grad_rhs):
    """<g, x(b1) - x(b0)> against <grad_rhs, b1 - b0>, per problem, relative to max(1, the larger sum of magnitudes of the two products)"""
    db, dx = pair
    lhs, rhs = (g * dx).sum(axis=1), (grad_rhs * db).sum(axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(g * dx).sum(axis=1), np.abs(grad_rhs * db).sum(axis=1)))
    return float((np.abs(lhs - rhs) / scale).max())


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: its inputs (draw), ref = the oracle's run on them, B = reference (B), A = reference (A) (None for the large cases),
    pairs = [(b1 - b0, x(b1) - x(b0))] x 3 for the large cases, gap = the case's share of D_CPU"""
    case = draw(name)
    B, cap, seed = case["lod"].shape[0], sum(case["caps"]), CASES[name]["seed"]
    fixed = case["fixed"]
    case["ref"] = oracle.lse_run(case["lod"], case["dims"], case["n"], maxdim=np.asarray(case["caps"], np.uint32), nthreads=4, **fixed)
    case["B"] = reference_from_factor(case, case["ref"])
    case["A"], case["pairs"], gap = None, [], 0.0
    used = np.arange(cap)[None, :] < case["dims"].sum(axis=1)[:, None]
    if case["large"]:
        for t in range(3):
            b0 = np.where(used, P.normal(seed + 7000 + 2 * t, B * cap).reshape(B, cap), 0.0)
            b1 = np.where(used, P.normal(seed + 7001 + 2 * t, B * cap).reshape(B, cap), 0.0)
            pair = (b1 - b0, _solve(case, b1, fixed.get("fixed_val"))["x"] - _solve(case, b0, fixed.get("fixed_val"))["x"])
            case["pairs"].append(pair)
            gap = max(gap, identity_gap(pair, case["g"], case["B"][0]))
    else:
        case["A"] = reference_unit_solves(case)
        for b in range(B):
            gap = max(gap, _rel(case["A"][0][b] - case["B"][0][b], case["A"][0][b]), _rel(case["A"][1][b] - case["B"][1][b], case["A"][1][b]))
    case["gap"] = gap
    for a in [case["lod"], case["dims"], case["g"], *case["B"], *(case["A"] or ()), *[x for p in case["pairs"] for x in p], *case["ref"].values(),
              *fixed.values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def expected(case):
    """what the device is compared with: reference (A), for the large cases (B)"""
    return case["A"] if case["A"] is not None else case["B"]


def summary(case):
    return (f"    {case['name']:<15} n={case['n']:<4} {str(case['caps']).replace(' ', ''):<18} batch {case['lod'].shape[0]}  ranks "
            f"{' '.join(str(r.tolist()).replace(' ', '') for r in case['ref']['rank']):<44} gap {case['gap']:.1e}  |grad_rhs| {np.abs(expected(case)[0]).max():.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in CASES:
        c = build(nm)
        worst = max(worst, c["gap"])
        print(summary(c))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
