"""Batches that hold every LexLSE kernel to the rank threshold `tol_linear_dependence` on NEAR-singular data (tests/test_gpu_rank_tolerance.py
runs them on the GPU, tests/test_rank_cases.py asserts the conditions below on the CPU, from the oracle alone).

P.near_dependent_batch makes one column of a problem a combination of two others plus delta N(0,1): the pivot that finally takes that column
has a fresh squared norm of about delta^2 x (rows left) — small, not zero, far from rounding noise.  A case does not move the data towards the
threshold, it moves the THRESHOLD across the data: tol_keep < delta^2 x rows < tol_drop, so the column is a pivot at tol_keep (and at the
default 1e-12) and a rank break at tol_drop.  Every fourth problem (b % 4 == 1) is an iid full-rank one, which must NOT flip; a `mixed` case
also overwrites b % 8 == 3 with P.rank_deficient_problem (exact dependences, residual norms ~1e-30): neighbours in a wavefront then stop at
different pivots for different reasons.

A case keeps the STABLE problems only: those whose oracle ranks are the same at tol / 10 and 10 tol, for tol_keep, tol_drop and the default.
A tolerance-contract kernel's own rounding of a fresh norm then cannot legitimately flip a rank, and "ranks exact" is a fair demand of every
kernel.  Per kept problem and tolerance the case carries the oracle's result and the ONE-ULP SENSITIVITY of x (scripts/soak_qtol.py: the data
perturbed by +-1.1e-16 relative, three draws, oracle only) — the yardstick of contract (T) in include/lexls_hip.h.

Conditions (tests/test_rank_cases.py): a case keeps at least half of what it drew; at least a quarter of the kept problems flip; at least one
does not; flipping and non-flipping problems share a group of four consecutive kept problems (a wavefront of lqr_qtol / lqr_quad) at least
once (every case but the large one).  Every shape with a near-dependent column has at least as many rows as variables: a hierarchy with fewer
never flips (n = 30, [9, 12, 5]: 0 of 64).

Chosen on the CPU: delta = 1e-4 with (tol_keep, tol_drop) = (1e-13, 1e-4) for every case.  The small pivot's squared norm is not delta^2 x rows
but spreads over delta^2 x (1e-2 .. 1e3) = 1e-10 .. 1e-5 (the two coefficients, and often a single row left when the column is taken), while
the smallest pivot of an iid problem is 1e-2 .. 1 (its levels' last pivots): tol_drop = 1e-4 has a decade of room on both sides (with a
first try, delta = 1e-3 and tol_drop = 1e-3, 10 tol_drop = 1e-2 cuts into the iid pivots: the IK shape kept 28 of 64), tol_keep and
the default lie three and two decades below the data.  tol_drop^2 = 1e-8 lies INSIDE the data, so that every case has flipping problems whose
pivot a test on the norm instead of the squared norm would keep.  lqr_mfma holds n = 44 / 47 only with fewer rows than variables (two / one
level), where a near-dependent column is never a pivot: cases n44 and n47 make the last ROW of level 0 near-dependent instead.

MEASURED (oracle alone, `python tests/rank_cases.py`; mixed groups = groups of four consecutive kept problems with flipping and steady ones;
sens = largest one-ulp sensitivity of x over the kept problems, the default's = tol_keep's):
    case                 shape             drawn kept (near/full/exact) flip  mixed groups  pivot in (tol_drop^2, tol_drop)  sens keep / drop
    ik                   n=40  [12]x5         64   62  (38/16/8)         38       15                   38               5.1e-10 / 6.3e-14
    n36                  n=36  [12]x4         64   51  (35/16/0)         35       12                   10               1.3e-10 / 3.9e-14
    n24                  n=24  [12]x3         64   58  (42/16/0)         42       14                   16               3.1e-11 / 1.2e-14
    n40x8                n=40  [8]x6          64   60  (44/16/0)         45       14                   29               1.2e-10 / 3.9e-14
    n24x8                n=24  [8]x4          64   60  (45/15/0)         45       14                   17               1.2e-10 / 5.3e-14
    ragged               n=20  [6,3,12,2]     64   64  (48/16/0)         48       16                   27               5.1e-10 / 1.4e-14
    ragged_per_problem   n=40  [12]x5         64   64  (48/16/0)         48       16                   48               6.3e-11 / 2.3e-14
    n44                  n=44  [12]x2         64   64  (48/16/0)         48       16                   47               7.3e-12 / 2.0e-15
    n47                  n=47  [12]x1         64   64  (48/16/0)         48       16                   48               1.3e-11 / 1.4e-15
    n47x4                n=47  [12]x4         64   64  (48/16/0)         48       16                   42               5.0e-11 / 4.4e-13
    generic              n=30  [14,9,16]      64   64  (48/16/0)         48       16                   48               1.0e-10 / 5.3e-15
    large                n=100 [115]x2         3    3  (2/1/0)          2        0                    2               8.0e-12 / 2.4e-15
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

DELTA, TOL_KEEP, TOL_DROP, TOL_DEFAULT = 1e-4, 1e-13, 1e-4, 1e-12
TOLS = dict(keep=TOL_KEEP, drop=TOL_DROP, default=TOL_DEFAULT)
FACTOR = 10.0  # stability window: same ranks at tol / FACTOR and tol * FACTOR

IK_PER_PROBLEM = np.array([[12, 12, 12, 12, 12], [12, 0, 12, 12, 12], [5, 12, 7, 12, 9], [12, 12, 12, 0, 12], [9, 12, 12, 12, 3], [12, 11, 12, 12, 12]], np.uint32)

# name -> n, dims (capacities), batch, seed; mixed: exactly dependent problems join; per_problem: dims rows dealt round the batch
CASES = {
    "ik": dict(n=40, dims=[12] * 5, batch=64, seed=20261201, mixed=((5, 12, 12, 12, 12), (12, 12, 2, 12, 12))),
    "n36": dict(n=36, dims=[12] * 4, batch=64, seed=20261202),
    "n24": dict(n=24, dims=[12] * 3, batch=64, seed=20261203),
    "n40x8": dict(n=40, dims=[8] * 6, batch=64, seed=20261204),
    "n24x8": dict(n=24, dims=[8] * 4, batch=64, seed=20261205),
    "ragged": dict(n=20, dims=[6, 3, 12, 2], batch=64, seed=20261206),
    "ragged_per_problem": dict(n=40, dims=[12] * 5, batch=64, seed=20261207, per_problem=IK_PER_PROBLEM),
    # lqr_mfma holds n = 41 .. 47 only with fewer rows than variables (two workgroups' LDS per CU: n = 44 up to two levels, n = 47 one),
    # where a near-dependent COLUMN is never taken as a pivot: these two make the last ROW of level 0 near-dependent instead (near_row)
    "n44": dict(n=44, dims=[12] * 2, batch=64, seed=20261208, near_row=True),
    "n47": dict(n=47, dims=[12], batch=64, seed=20261209, near_row=True),
    "n47x4": dict(n=47, dims=[12] * 4, batch=64, seed=20261212),
    "generic": dict(n=30, dims=[14, 9, 16], batch=64, seed=20261210),
    "large": dict(n=100, dims=[115, 115], batch=3, seed=20261211),  # (n + 1) x 230 x 8 = 186 KB: beyond one CU's LDS
}


def draw(name):
    """(lod, dims, kind) of a case before anything is dropped; kind[b]: 0 near-dependent, 1 iid full rank, 2 exactly dependent"""
    c = CASES[name]
    n, caps, B, seed = c["n"], list(c["dims"]), c["batch"], c["seed"]
    kind = np.zeros(B, np.int32)
    if c.get("near_row"):  # row d0 - 1 of level 0 = a combination of its rows 0 and 1 + DELTA N(0,1) (right-hand side untouched): the level's
        lod = P.lse_batch_fast(seed, B, n, caps)  # last pivot has a fresh squared norm of about DELTA^2 x (n - d0 + 1)
        coef, noise = P.normal(seed, 2 * B, 2).reshape(B, 2), P.normal(seed, B * n, 3).reshape(B, n)
        lod[:, :n, caps[0] - 1] = coef[:, :1] * lod[:, :n, 0] + coef[:, 1:] * lod[:, :n, 1] + DELTA * noise
    else:
        lod = P.near_dependent_batch(seed, B, n, caps, DELTA)
    for b in range(1, B, 4):
        lod[b] = P.lse_problem(seed + 1000 + b, n, caps)
        kind[b] = 1
    for b in range(3, B, 8) if c.get("mixed") else ():
        lod[b] = P.rank_deficient_problem(seed + 2000 + b, n, caps, list(c["mixed"][(b // 8) % len(c["mixed"])]))
        kind[b] = 2
    dims = np.tile(np.asarray(caps, np.uint32), (B, 1))
    if c.get("per_problem") is not None:  # a problem's rows packed level after level; NaN behind them (never read)
        pp = c["per_problem"]
        dims = pp[np.arange(B) % len(pp)].copy()
        for b in range(B):
            m = int(dims[b].sum())
            assert m >= n
            lod[b, :, m:] = np.nan
    assert sum(caps) >= n or c.get("near_row")
    return lod, dims, kind


def _run(name, lod, dims, tol):
    c = CASES[name]
    return oracle.lse_run(lod, dims, c["n"], maxdim=np.asarray(c["dims"], np.uint32), tol=tol, nthreads=8)


def _rel(x, ref_x):
    return np.abs(x - ref_x).max(axis=1) / np.maximum(1.0, np.abs(ref_x).max(axis=1))


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: dict(n, caps, lod, dims (batch, nObj), uniform (all problems have the capacities' dims), kind, drawn, dropped,
    ref[t], sens[t] for t in keep / drop / default, flip (kept problem's ranks differ between keep and drop), mixed_groups)"""
    c = CASES[name]
    lod, dims, kind = draw(name)
    stable = np.ones(lod.shape[0], bool)
    for tol in TOLS.values():
        lo, hi = _run(name, lod, dims, tol / FACTOR), _run(name, lod, dims, tol * FACTOR)
        stable &= (lo["rank"] == hi["rank"]).all(axis=1) & (lo["fcol"] == hi["fcol"]).all(axis=1)
    keep = np.flatnonzero(stable)
    lod, dims, kind = np.ascontiguousarray(lod[keep]), np.ascontiguousarray(dims[keep]), kind[keep]
    ref, sens = {}, {}
    finite = np.where(np.isnan(lod), 0.0, lod)
    for t, tol in TOLS.items():
        ref[t] = _run(name, lod, dims, tol)
        s = np.zeros(len(keep))
        for rep in range(3):
            sign = np.where(P.uniform(c["seed"] + 31 * rep, lod.size, 7).reshape(lod.shape) < 0.5, -1.0, 1.0)
            pert = np.where(np.isnan(lod), np.nan, finite * (1.0 + 1.1e-16 * sign))
            s = np.maximum(s, _rel(_run(name, pert, dims, tol)["x"], ref[t]["x"]))
        sens[t] = s
    flip = (ref["keep"]["rank"] != ref["drop"]["rank"]).any(axis=1)
    # the smallest squared pivot the oracle accepts at tol_keep: between tol_drop^2 and tol_drop, a kernel that compared the NORM with the
    # tolerance (not the squared norm, lexlse.h:214) would keep that pivot at tol_drop as well
    smallest = np.full(len(keep), np.inf)
    for b in range(len(keep)):
        row = 0
        for k in range(dims.shape[1]):
            fc, r = int(ref["keep"]["fcol"][b, k]), int(ref["keep"]["rank"][b, k])
            for j in range(r):
                smallest[b] = min(smallest[b], ref["keep"]["factor"][b, fc + j, row + j] ** 2)
            row += int(dims[b, k])
    groups = [flip[i:i + 4] for i in range(0, len(flip) - 3, 4)]
    for a in [lod, dims, kind, flip, smallest, *sens.values()] + [v for r in ref.values() for v in r.values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return dict(name=name, n=c["n"], caps=list(c["dims"]), lod=lod, dims=dims, uniform=c.get("per_problem") is None, kind=kind,
                drawn=c["batch"], dropped=c["batch"] - len(keep), ref=ref, sens=sens, flip=flip, smallest_pivot_sq=smallest,
                norm_sensitive=int((flip & (smallest > TOL_DROP ** 2) & (smallest < TOL_DROP)).sum()),
                mixed_groups=sum(1 for g in groups if g.any() and not g.all()))


def summary(case):
    k = case["kind"]
    return (f"{case['name']:>18}: n={case['n']} dims={case['caps']} drawn {case['drawn']} kept {len(k)} (near {int((k == 0).sum())}, full {int((k == 1).sum())}, "
            f"exact {int((k == 2).sum())}) flipping {int(case['flip'].sum())} mixed groups of four {case['mixed_groups']} between tol_drop^2 and tol_drop {case['norm_sensitive']} "
            f"largest one-ulp sensitivity keep/drop/default {case['sens']['keep'].max():.1e}/{case['sens']['drop'].max():.1e}/{case['sens']['default'].max():.1e}")


if __name__ == "__main__":
    for nm in CASES:
        print(summary(build(nm)))
