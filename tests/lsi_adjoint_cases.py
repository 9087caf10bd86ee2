"""Cases that hold the gradients of batched LexLSI solutions with respect to the bounds (lexls_lsi_batch_solve_adjoint, lexls_amd/csrc/lsi_final.h:
lsi_adjoint_scatter_multi_kernel behind get_lambda's final-problem stage and solve_adjoint_kernel) to two references, both built from the oracle alone
(tests/test_lsi_adjoint_cases.py asserts on the CPU that they agree; tests/test_gpu_lsi_adjoint.py compares the device with them).

At an instance that ended PROBLEM_SOLVED x is the basic solution of the equality problem of its final working set W: right-hand sides = the active
bounds (lb for CTR_ACTIVE_LB, ub for CTR_ACTIVE_UB and CTR_ACTIVE_EQ), fixed values = the active simple bounds.  While W holds, x is affine in the
bounds; with g = dloss/dx the gradient of an active constraint is its entry of M^T g (general rows) or N^T g (simple bounds), in grad_lb or grad_ub
by its type, and everything outside W is 0.
    reference (A)  W from oracle.lsi_run; the final equality problem built here in numpy (rows in constraint order, level by level); M^T g and
                   N^T g by adjoint_cases.reference_unit_solves (unit solves on the oracle's equality solver); scattered in numpy.
    reference (B)  differences through the whole oracle LexLSI driver, independent of (A)'s formation:
                   <g, x(lb1, ub1) - x(lb0, ub0)> = <grad_lb, lb1 - lb0> + <grad_ub, ub1 - ub0> for three random perturbations of all bounds
                   (size PERTURB; an equality keeps lb = ub).  Every perturbed solve must end PROBLEM_SOLVED with the working set of the
                   unperturbed one, for every instance (asserted): then the map is affine between the two points and the identity is exact up
                   to rounding.

Cases — small on purpose:
    small_sb    n = 4, simple bounds on 4 variables, general (2), general (2, equalities), batch 4
    general     n = 5, general objectives only, dims (3, 2, 3), batch 4
    rank_def    n = 5, general (3, 2, 3): row 0 of level 1 repeats row 0 of level 0 (both equalities, so both are in W): a level of rank < rows
    empty_ws    n = 4, general (3, 3): instances 1 and 3 have bounds around 0 that nothing reaches — their final working set is empty (x = 0)
    ik          n = 40, simple bounds (12) + 4 x 12, batch 8: the shape of the persistent launch (tests/test_gpu_lsi_lambda.py)
    budget      (status rule, tests/test_gpu_lsi_adjoint.py) small_sb's shape, batch 6, run cold with max_number_of_factorizations = 1: instances
                0, 2, 4 have inequality bounds too wide to be reached and end PROBLEM_SOLVED on the equalities alone, the others are stopped by the
                budget (the oracle's statuses, asserted on the CPU)
    tile        (scatter tile, tests/test_gpu_lsi_adjoint_groups.py) n = 4, simple bounds (4), general (1030), general (2, equalities), batch 2:
                1036 user rows, more than the 1024 the scatter kernels take per tile.  Rows 5 and 1027 of the second objective are equalities, its
                other rows inequalities 100 away from anything |x_i| <= 1 reaches: the working set has rows on both sides of user row 1024.
                Reference (A) alone

D_CPU is the largest discrepancy the CPU test finds — the two sides of (B)'s identities with (A)'s gradients, per instance relative to
max(1, the larger sum of magnitudes of the two products) (adjoint_cases.identity_gap).  The GPU tolerance is TOL = max(10 * D_CPU, 1e-12), the rule
and the reasoning of tests/adjoint_cases.py: the factor 10 allows for fma contraction and summation orders that differ from numpy's; it never
comes from device figures and stays at or below the 1e-10 of the tolerance contract.
MEASURED (`python tests/lsi_adjoint_cases.py`, the oracle and numpy alone; gap = the case's largest discrepancy, |W| = active constraints per instance):
    small_sb  n=4   [4,2,2]            batch 4  |W| [3,3,5,5]                  held True  gap 6.8e-16  |grad| 2.1e+00
    general   n=5   [3,2,3]            batch 4  |W| [7,8,7,8]                  held True  gap 1.7e-15  |grad| 1.9e+01
    rank_def  n=5   [3,2,3]            batch 4  |W| [7,8,8,8]                  held True  gap 1.1e-15  |grad| 6.3e+00
    empty_ws  n=4   [3,3]              batch 4  |W| [4,0,5,0]                  held True  gap 8.4e-16  |grad| 1.7e+00
    ik        n=40  [12,12,12,12,12]   batch 8  |W| [42,42,47,42,42,41,45,43]  held True  gap 8.8e-15  |grad| 3.6e+00
    budget    statuses [0, 2, 0, 2, 0, 2]
    tile      n=4   [4,1030,2]  batch 2  statuses [0, 0]  active user rows [0,9,1031,1034,1035] [0,2,3,9,1031,1034,1035]  |grad| 4.1e+00
    D_CPU = 8.79e-15 (ik)  ->  TOL = max(10 D_CPU, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
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

import adjoint_cases as AC  # noqa: E402  (reference_unit_solves, identity_gap: imported, not copied)
from lexls_amd import problems as P  # noqa: E402
from oracle import oracle_ctypes as oracle  # noqa: E402

D_CPU = 8.79e-15  # measured: the table above (tests/test_lsi_adjoint_cases.py re-measures it and asserts that TOL still follows from it)
TOL = max(10.0 * D_CPU, 1e-12)
PERTURB = 1e-3  # size of (B)'s bound perturbations: the working sets of these cases hold under it (asserted for every instance)

LB, UB, EQ = 1, 2, 3  # ConstraintActivationType (include/lexls/typedefs.h)
SOLVED = 0

CASES = {
    "small_sb": dict(n=4, dims=(4, 2, 2), simple=True, batch=4, seed=20300101),
    "general": dict(n=5, dims=(3, 2, 3), simple=False, batch=4, seed=20300201),
    "rank_def": dict(n=5, dims=(3, 2, 3), simple=False, batch=4, seed=20300301, duplicate=True),
    "empty_ws": dict(n=4, dims=(3, 3), simple=False, batch=4, seed=20300401, empty=(1, 3)),
    "ik": dict(n=40, dims=(12, 12, 12, 12, 12), simple=True, batch=8, seed=20300514),
}
BUDGET = dict(n=4, dims=(4, 2, 2), simple=True, batch=6, seed=20300601, wide=(0, 2, 4))
# the scatter kernels tile the user rows by ADJ_TILE = 1024 (lexls_amd/csrc/lsi_final.h): 1036 rows, with active ones on both sides of row 1024
TILE = dict(n=4, dims=(4, 1030, 2), simple=True, batch=2, seed=20310301, equalities=(5, 1027), far=100.0)
ADJ_TILE = 1024


def problems_of(name):
    """the objective lists of a case's instances (lexls_amd.problems.lsi_problem, then the case's own changes)"""
    c = BUDGET if name == "budget" else TILE if name == "tile" else CASES[name]
    out = []
    for i in range(c["batch"]):
        objs = P.lsi_problem(c["seed"] + i, c["n"], c["dims"], simple_bounds=c["simple"])
        if c.get("duplicate"):  # equalities with the same row and different values on levels 0 and 1: both always in W, level 1 loses a rank
            objs[0]["ub"][0] = objs[0]["lb"][0]
            objs[1]["A"][0] = objs[0]["A"][0]
            objs[1]["lb"][0] = objs[1]["ub"][0] = objs[0]["lb"][0] + 0.5
        if i in c.get("empty", ()):  # nothing is an equality, 0 is strictly inside every bound: the cold start x = 0 is the answer
            for o in objs:
                w = 1.0 + P.uniform(c["seed"] + 50 + i, len(o["lb"]))
                o["lb"], o["ub"] = -w, w[::-1].copy()
        if c.get("equalities"):  # level 1: inequalities far away from anything x can reach (|x_i| <= 1), but for two equalities
            o = objs[1]
            keep = np.zeros(len(o["lb"]), bool)
            keep[list(c["equalities"])] = True
            mid = 0.5 * (o["lb"] + o["ub"])
            o["lb"], o["ub"] = np.where(keep, mid, o["lb"] - c["far"]), np.where(keep, mid, o["ub"] + c["far"])
        if i in c.get("wide", ()):  # the inequalities out of reach: the equalities of the last level alone decide
            for o in objs[:-1]:
                o["lb"], o["ub"] = o["lb"] - 100.0, o["ub"] + 100.0
        out.append(objs)
    return out


def with_bounds(objs, lb, ub):
    """the objectives with other bounds (total,), constraint order"""
    out, f = [], 0
    for o in objs:
        m = len(o["lb"])
        out.append(dict(o, lb=lb[f:f + m].copy(), ub=ub[f:f + m].copy()))
        f += m
    return out


def bounds_of(objs):
    return np.concatenate([o["lb"] for o in objs]), np.concatenate([o["ub"] for o in objs])


def final_problem(n, objs, active):
    """the equality problem of the working set `active` (per objective the activation types, constraint order) as the oracle's equality solver
    takes it: lod (n + 1, cap) with the active general rows level by level in constraint order, dims per level, the fixed variables (index, value),
    and per row of [fixed | LOD rows] its (user row, type)"""
    off = 1 if "var" in objs[0] else 0
    caps = [len(o["lb"]) for o in objs[off:]]
    lod, dims, rows, fixed, first, r = np.zeros((n + 1, sum(caps))), [], [], [], 0, 0
    for k, o in enumerate(objs):
        act = np.flatnonzero(np.asarray(active[k]) != 0)
        if k < off:
            for c in act:
                t = int(active[k][c])
                fixed.append((int(o["var"][c]), float(o["lb"][c] if t == LB else o["ub"][c]), first + int(c), t))
        else:
            for c in act:
                t = int(active[k][c])
                lod[:n, r] = o["A"][c]
                lod[n, r] = o["lb"][c] if t == LB else o["ub"][c]
                rows.append((first + int(c), t))
                r += 1
            dims.append(len(act))
        first += len(o["lb"])
    return lod, np.asarray(dims, np.uint32), caps, fixed, rows


def reference_a(n, probs, actives, statuses, g):
    """reference (A) for a batch: (grad_lb, grad_ub) (batch, total); zeros for the instances that did not end PROBLEM_SOLVED.  Also the ranks of
    the final problems' levels (what the rank-deficient case is named for)"""
    B, total = len(probs), sum(len(o["lb"]) for o in probs[0])
    formed = [final_problem(n, probs[b], actives[b]) for b in range(B)]
    caps = formed[0][2]
    nf = np.asarray([len(f[3]) for f in formed], np.uint32)
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b, f in enumerate(formed):
        for j, (var, value, _, _) in enumerate(f[3]):
            idx[b, j], val[b, j] = var, value
    case = dict(n=n, caps=caps, lod=np.stack([f[0] for f in formed]), dims=np.stack([f[1] for f in formed]), g=np.asarray(g, float),
                fixed=dict(nfixed=nf, fixed_idx=idx, fixed_val=val) if nf.any() else {})
    grad_rhs, grad_fixed = AC.reference_unit_solves(case)
    ranks = oracle.lse_run(case["lod"], case["dims"], n, maxdim=np.asarray(caps, np.uint32), **case["fixed"])["rank"]
    grad_lb, grad_ub = np.zeros((B, total)), np.zeros((B, total))
    for b, f in enumerate(formed):
        if statuses[b] != SOLVED:
            continue
        for j, (_, _, u, t) in enumerate(f[3]):
            (grad_lb if t == LB else grad_ub)[b, u] = grad_fixed[b, j]
        for r, (u, t) in enumerate(f[4]):
            (grad_lb if t == LB else grad_ub)[b, u] = grad_rhs[b, r]
    return grad_lb, grad_ub, ranks


def perturbation(seed, lb, ub):
    """bounds moved by PERTURB * N(0, 1) each (by a tenth of its width times N(0, 1) where a constraint is narrower than that: lb stays below
    ub); an equality (lb == ub) moves as one"""
    size = np.where(lb == ub, PERTURB, np.minimum(PERTURB, 0.1 * (ub - lb)))
    dl, du = size * P.normal(seed, lb.size, 1), size * P.normal(seed, ub.size, 2)
    du = np.where(lb == ub, dl, du)
    return lb + dl, ub + du


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: n, dims, types, probs (objective lists), runs (the oracle's lsi_run per instance), active (batch, total), status (batch,),
    g (batch, n), A = reference (A) (grad_lb, grad_ub), ranks, pairs = 3 x [(dlb, dub, dx)] (batch-wide arrays), held (every perturbed solve ended
    PROBLEM_SOLVED on the unperturbed working set), gap = the case's share of D_CPU"""
    c = CASES[name]
    n, B, seed = c["n"], c["batch"], c["seed"]
    probs = problems_of(name)
    runs = [oracle.lsi_run(n, objs) for objs in probs]
    status = np.asarray([r["info"]["status"] for r in runs])
    g = P.normal(seed + 900, B * n).reshape(B, n)
    glb, gub, ranks = reference_a(n, probs, [r["active"] for r in runs], status, g)
    total = glb.shape[1]
    pairs, held, gap = [], True, 0.0
    for t in range(3):
        dlb, dub, dx = np.zeros((B, total)), np.zeros((B, total)), np.zeros((B, n))
        for b, objs in enumerate(probs):
            lb0, ub0 = bounds_of(objs)
            lb1, ub1 = perturbation(seed + 7000 + 10 * t + b, lb0, ub0)
            r1 = oracle.lsi_run(n, with_bounds(objs, lb1, ub1))
            held = held and r1["info"]["status"] == SOLVED and all(np.array_equal(a, a0) for a, a0 in zip(r1["active"], runs[b]["active"]))
            dlb[b], dub[b], dx[b] = lb1 - lb0, ub1 - ub0, r1["x"] - runs[b]["x"]
        pairs.append((dlb, dub, dx))
        gap = max(gap, AC.identity_gap((np.hstack([dlb, dub]), dx), g, np.hstack([glb, gub])))
    case = dict(name=name, n=n, dims=np.asarray(c["dims"], np.uint32), probs=probs, runs=runs, status=status, g=g, A=(glb, gub), ranks=ranks,
                active=np.stack([np.concatenate(r["active"]) for r in runs]), pairs=pairs, held=held, gap=gap)
    for a in [g, glb, gub, ranks, case["active"], status, *[x for p in pairs for x in p]]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


@functools.lru_cache(maxsize=None)
def build_budget():
    """the status-rule case: cold, max_number_of_factorizations = 1.  status (batch,) from the oracle; A = reference (A) on the oracle's final
    working sets, zeros in the instances the budget stopped"""
    c = BUDGET
    n, B = c["n"], c["batch"]
    probs = problems_of("budget")
    runs = [oracle.lsi_run(n, objs, max_number_of_factorizations=1) for objs in probs]
    status = np.asarray([r["info"]["status"] for r in runs])
    g = P.normal(c["seed"] + 900, B * n).reshape(B, n)
    glb, gub, _ = reference_a(n, probs, [r["active"] for r in runs], status, g)
    return dict(name="budget", n=n, probs=probs, runs=runs, status=status, g=g, A=(glb, gub), active=np.stack([np.concatenate(r["active"]) for r in runs]))


@functools.lru_cache(maxsize=None)
def build_tile():
    """the scatter-tile case: 4 simple bounds, 1030 general rows of which rows 5 and 1027 are equalities and the rest out of reach, 2 equalities;
    user rows 0 .. 1035, so the scatter kernels run a second tile of ADJ_TILE rows.  A = reference (A) on the oracle's final working sets"""
    c = TILE
    n, B = c["n"], c["batch"]
    probs = problems_of("tile")
    runs = [oracle.lsi_run(n, objs) for objs in probs]
    status = np.asarray([r["info"]["status"] for r in runs])
    g = P.normal(c["seed"] + 900, B * n).reshape(B, n)
    glb, gub, ranks = reference_a(n, probs, [r["active"] for r in runs], status, g)
    return dict(name="tile", n=n, dims=np.asarray(c["dims"], np.uint32), probs=probs, runs=runs, status=status, g=g, A=(glb, gub), ranks=ranks,
                active=np.stack([np.concatenate(r["active"]) for r in runs]))


def summary(case):
    nact = (case["active"] != 0).sum(axis=1)
    return (f"    {case['name']:<9} n={case['n']:<3} {str(case['dims'].tolist()).replace(' ', ''):<18} batch {len(case['probs'])}  |W| {str(nact.tolist()).replace(' ', ''):<26} "
            f"held {case['held']}  gap {case['gap']:.1e}  |grad| {max(np.abs(case['A'][0]).max(), np.abs(case['A'][1]).max()):.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in CASES:
        cs = build(nm)
        worst = max(worst, cs["gap"])
        print(summary(cs))
    bd = build_budget()
    print(f"    budget    statuses {bd['status'].tolist()}")
    tl = build_tile()
    print(f"    tile      n=4   [4,1030,2]  batch 2  statuses {tl['status'].tolist()}  active user rows {[np.flatnonzero(a).tolist() for a in tl['active']]}  "
          f"|grad| {max(np.abs(tl['A'][0]).max(), np.abs(tl['A'][1]).max()):.1e}")
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
