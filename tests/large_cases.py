"""Problems that hold the LARGE path (lexls_amd/csrc/lqr_large.hip: lqr_large<multi-launch>, bit-exact, and lqr_large<step-per-pivot,mfma>,
tolerance contract, with the pivots of a single problem's level in one launch: fast_level_persist) to the oracle on both sides of the switches
of its kernels and launchers (tests/test_gpu_large_cases.py runs them on the GPU; tests/test_large_cases.py asserts on the CPU, from the oracle
and the constants alone, which side of which switch every case is on — its docstring holds the table).

Every case is a small BATCH whose problem 0 is also solved alone: the same data then go through a launch per pivot (a batch) and through the
one-launch form (one problem).  Unused rows of a ragged problem hold NaN (never read).  Cases (what each is for):
    rows1030   n = 60 [1030, 70], three problems.  Problem 0: level 0 has 1030 rows and rank 25 (P.rank_deficient_problem), so level 1 still has
               columns and the Gauss step behind a level of more than 1024 rows runs (large_trsm, the row-per-lane form: min(n, maxdim) <= 315 is
               all its LDS allows, hence the small n); rows left in the level R > 256 (tail loops of fast_step, one-by-one granules of
               fast_level_persist) and R > 1024 (second trip of large_pivot's loops), more than 1024 rows in all (second block of fast_level_end).
               Problem 1 has dims [300, 70]: the launchers take the > 1024 branch for a problem whose own level is short.  Problem 2 is iid, full
               rank in level 0: exhausted while the others are not.
    rows1024   n = 60 [1024, 70], two problems: the last level large_trsm_cols takes (a workgroup of 1024 threads), exactly one trip of large_pivot
    n1030      n = 1030 [40, 40], two problems.  Columns 1024 .. 1029 are scaled by 3: the first pivots are columns only the SECOND search loop of
               fast_step sees (candidates beyond 1024 / FNT per thread) and large_pivot's second trip over the columns.  In problem 0 column 1000
               repeats column 1027: an exact tie across the two loops, the first position must win.  G = (n + 4) / 4 = 258 > 256: no one-launch
               form fits, a single problem takes a launch per pivot
    rows257    n = 150 [257, 256, 60], ranks 50 / 60 / 20: one pivot above the 256-row window, next to an exact 256
    rows330    n = 150 [330, 120], iid: 74 pivots above the window, the columns run out (rank 150) inside a level of more than 256 rows
    edges127, edges128   n + 1 = 128 and 129 (tiles of 64 columns: none and one column over), [100, 1, 0, 40, 24]: 65 rows below level 0 (one over
               64 and over 8), level ranks 17 (one over TCH = 16), 1, 0, 5 (fewer than TCH), 10; a 1-row level and an empty level in the middle

Kept data only: the oracle's ranks, first columns and permutation are the same at 10 x and at 1 / 10 of the default tolerance (else another seed:
none was needed).  Per case the oracle's result and the ONE-ULP SENSITIVITY of x (as tests/rank_cases.py: the data perturbed by +-1.1e-16
relative, three draws, oracle only) — the yardstick of contract (T) in include/lexls_hip.h.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lexls_amd import problems as P  # noqa: E402
from oracle import oracle_ctypes as oracle  # noqa: E402

TOL = 1e-12    # the default tol_linear_dependence
FACTOR = 10.0  # stability window: same ranks and pivots at TOL / FACTOR and TOL * FACTOR

EDGE_DIMS = [100, 1, 0, 40, 24]
EDGE_RANKS = [17, 1, 0, 5, 10]

# name -> n, dims (capacities), seed, problems: per problem (dims, ranks); ranks None = iid full rank (P.lse_problem)
CASES = {
    "rows1030": dict(n=60, dims=[1030, 70], seed=20280101, problems=[([1030, 70], [25, 20]), ([300, 70], [30, 15]), ([1030, 70], None)]),
    "rows1024": dict(n=60, dims=[1024, 70], seed=20280102, problems=[([1024, 70], [25, 20]), ([300, 70], [30, 15])]),
    "n1030": dict(n=1030, dims=[40, 40], seed=20280103, problems=[([40, 40], None), ([40, 40], None)], scaled=(1024, 1030, 3.0), tie=(1000, 1027)),
    "rows257": dict(n=150, dims=[257, 256, 60], seed=20280104, problems=[([257, 256, 60], [50, 60, 20]), ([257, 100, 60], [40, 30, 60])]),
    "rows330": dict(n=150, dims=[330, 120], seed=20280105, problems=[([330, 120], None), ([330, 120], [100, 30])]),
    "edges127": dict(n=127, dims=EDGE_DIMS, seed=20280106, problems=[(EDGE_DIMS, EDGE_RANKS), ([99, 0, 0, 40, 24], [9, 0, 0, 16, 8])]),
    "edges128": dict(n=128, dims=EDGE_DIMS, seed=20280107, problems=[(EDGE_DIMS, EDGE_RANKS), ([99, 0, 0, 40, 24], [9, 0, 0, 16, 8])]),
}

# Work-space reuse (test_workspace_reuse of tests/test_gpu_large_cases.py): ONE handle of capacities [330, 100] solves reuse300, then reuse330
# (largest level 330: the work space grows), then reuse300 again (the larger work space is kept and laid out for the smaller shape).  Not among
# CASES: they sit on no new side of a switch; same shape of spec, built by build() like a case.
REUSE = {
    "reuse300": dict(n=60, dims=[330, 100], seed=20280108, problems=[([300, 100], [25, 20]), ([300, 100], [30, 15])]),
    "reuse330": dict(n=60, dims=[330, 100], seed=20280109, problems=[([330, 70], [25, 20]), ([330, 70], [30, 15])]),
}
SPECS = {**CASES, **REUSE}


def draw(name):
    """(lod (batch, n + 1, cap), dims (batch, nObj)) of a case"""
    c = SPECS[name]
    n, caps, seed = c["n"], list(c["dims"]), c["seed"]
    B, cap = len(c["problems"]), sum(caps)
    lod = np.full((B, n + 1, cap), np.nan)  # a problem's rows packed level after level; NaN behind them (never read)
    dims = np.zeros((B, len(caps)), np.uint32)
    for b, (d, ranks) in enumerate(c["problems"]):
        m = sum(d)
        dims[b] = d
        lod[b, :, :m] = P.lse_problem(seed + 1000 * b, n, d) if ranks is None else P.rank_deficient_problem(seed + 1000 * b, n, d, ranks)
        if c.get("scaled"):
            lo, hi, f = c["scaled"]
            lod[b, lo:hi, :m] *= f
    if c.get("tie"):
        first, second = c["tie"]
        lod[0, first, :] = lod[0, second, :]
    return lod, dims


def _run(name, lod, dims, tol=TOL):
    c = SPECS[name]
    return oracle.lse_run(lod, dims, c["n"], maxdim=np.asarray(c["dims"], np.uint32), tol=tol, nthreads=4)


def _rel(x, ref_x):
    return np.abs(x - ref_x).max(axis=1) / np.maximum(1.0, np.abs(ref_x).max(axis=1))


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: dict(name, n, caps, lod, dims, ref (the oracle's result for the batch), stable (per problem: ranks, first columns and
    permutation the same at TOL / 10 and 10 TOL), sens (per problem: one-ulp sensitivity of x), forced (the ranks the data were built for, None:
    iid))"""
    c = SPECS[name]
    lod, dims = draw(name)
    ref = _run(name, lod, dims)
    lo, hi = _run(name, lod, dims, TOL / FACTOR), _run(name, lod, dims, TOL * FACTOR)
    stable = np.ones(lod.shape[0], bool)
    for k in ("rank", "fcol", "perm"):
        stable &= (lo[k] == hi[k]).all(axis=1) & (lo[k] == ref[k]).all(axis=1)
    finite = np.where(np.isnan(lod), 0.0, lod)
    sens = np.zeros(lod.shape[0])
    for rep in range(3):
        sign = np.where(P.uniform(c["seed"] + 31 * rep, lod.size, 7).reshape(lod.shape) < 0.5, -1.0, 1.0)
        pert = np.where(np.isnan(lod), np.nan, finite * (1.0 + 1.1e-16 * sign))
        sens = np.maximum(sens, _rel(_run(name, pert, dims)["x"], ref["x"]))
    for a in [lod, dims, stable, sens, *ref.values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return dict(name=name, n=c["n"], caps=list(c["dims"]), lod=lod, dims=dims, ref=ref, stable=stable, sens=sens,
                forced=[r for _, r in c["problems"]], tie=c.get("tie"))


def levels_reached(case, b=0):
    """levels of problem b on which the launcher of the step-per-pivot path looks for pivots: non-empty, and columns left when the level starts"""
    rank, n = case["ref"]["rank"][b], case["n"]
    return sum(1 for k in range(len(rank)) if case["dims"][b, k] > 0 and int(rank[:k].sum()) < n)


def summary(case):
    r = case["ref"]["rank"]
    return (f"    {case['name']:<9} n={case['n']:<4} {str(case['caps']).replace(' ', ''):<16} batch {case['lod'].shape[0]}  ranks "
            f"{' '.join(str(x.tolist()).replace(' ', '') for x in r):<40} sens {' '.join(f'{s:.1e}' for s in case['sens'])}")


if __name__ == "__main__":
    for nm in CASES:
        print(summary(build(nm)))
