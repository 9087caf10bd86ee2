"""Cases that hold the gradients of batched LexLSI solutions with respect to the whole constraint data (lexls_lsi_batch_solve_adjoint_matrix,
lexls_amd/csrc/lsi_final.h: lsi_adjoint_matrix_scatter_kernel behind the final-problem stage and the matrix chain of the equality solver) to two
references, both built from the oracle alone (tests/test_lsi_adjoint_matrix_cases.py asserts on the CPU that they agree;
tests/test_gpu_lsi_adjoint_matrix.py compares the device with reference (A)).

At an instance that ended PROBLEM_SOLVED x is the basic solution of the equality problem of its final working set W.  While W holds, x as a
function of the active rows' A and bounds is the LexLSE solve map of that final problem: an active general row gets its row of
- y x^T - lambda u^T in the A columns and its entry of y = M^T g in the lb (CTR_ACTIVE_LB) or ub (CTR_ACTIVE_UB, CTR_ACTIVE_EQ) column, an
active simple bound its slot of N^T g by the same rule, everything outside W is an exact 0.  An instance is differentiable (flag 1) when it
ended PROBLEM_SOLVED and its final problem is rank-stable (adjoint_matrix_cases.rank_stable); else the flag is 0 and its whole slice is zeros.
An empty working set is differentiable and all zeros.  grad_data has the layout of the data itself (lexls_amd.lexlsi.flatten).
    reference (A)  W from oracle.lsi_run; the final problem by lsi_adjoint_cases.final_problem; its ranks and transpositions from oracle.lse_run;
                   the dense KKT gradient on its original data by adjoint_matrix_cases.reference_kkt (A columns, y); N^T g = g_fixed - A_fixed^T y
                   from that y; scattered here in numpy with the zero, type and flag rules.
    reference (B)  central differences through the whole oracle LexLSI driver, independent of (A)'s formation: a random direction dD over ALL
                   data of an instance (A, lb, ub, inactive rows included; an equality keeps lb = ub), step FD_H of adjoint_matrix_cases:
                   (<g, x(D + h dD)> - <g, x(D - h dD)>) / 2h against <grad_data, dD>.  Both perturbed solves must end PROBLEM_SOLVED on the
                   unperturbed working set (asserted for every instance used: `held`); (B) covers every flag-1 instance of every case it runs on.
    D_CPU          the largest discrepancy between (A) and the numpy restatement of the kernels' steps on the oracle's factor of these final
                   problems (adjoint_matrix_cases.reference_from_factor for grad_lod, adjoint_cases.adjoint_from_factor for N^T g), relative to
                   max(1, largest magnitude of (A)) per instance.

Cases — small on purpose (problems_of of lsi_adjoint_cases; FLAGS as literals, the tests also compute them by the rule):
    small_sb    n = 4, simple bounds (4) + (2, 2), batch 4: one or two fixed variables (a last level that finds one column left)   1 1 1 1
    general     n = 5, (3, 2, 3), batch 4                                                                                  1 1 1 1
    empty_ws    n = 4, (3, 3): instances 1 and 3 have empty W                                                              1 1 1 1
    ik          n = 40, simple bounds (12) + 4 x 12, batch 8                                                               1 x 8
    rank_def    n = 5, (3, 2, 3): ranks (3, 1, 1)                                                                          0 0 0 0
    mixed       instances of general and rank_def interleaved: the flags differ between neighbours                         1 0 1 0
    budget      small_sb's shape, batch 6, cold with max_number_of_factorizations = 1: statuses (0, 2, 0, 2, 0, 2)         1 0 1 0 1 0
    tile        n = 4, (4, 1030, 2), batch 2: 1036 user rows, active rows on both sides of row 1024; reference (A) alone   1 1

GPU tolerance TOL = max(10 D_CPU, 1e-12): the rule and the reasoning of tests/adjoint_matrix_cases.py (the factor 10 allows for fma contraction
and other summation orders); never taken from device figures, never above the 1e-10 of the tolerance contract.
FD_BOUND, the bound on (B)'s gap (|fd - <grad_data, dD>| relative to max(1, sum of the magnitudes of the products)): ten times the largest gap
measured here on the CPU, not adjoint_matrix_cases' FD_BOUND; it may not exceed 1e-6.  The rounding term of a central difference is
eps |g| |x| cond / h with eps / h = 2e-10.
MEASURED (`python tests/lsi_adjoint_matrix_cases.py`, the oracle and numpy alone; scale = size of dD's entries, gapB = (A) vs (B), d = (A) vs factor):
    small_sb  n=4   [4,2,2]           batch 4  flags 1111      held True  scale 1.0  gapB 3.3e-11  d 1.1e-15  |grad| 2.8e+00  ranks [1,2] [1,2] [2,1] [2,1]
    general   n=5   [3,2,3]           batch 4  flags 1111      held True  scale 1.0  gapB 3.9e-11  d 1.0e-14  |grad| 1.1e+02  ranks [2,2,1] [3,2,0] [2,2,1] [3,2,0]
    empty_ws  n=4   [3,3]             batch 4  flags 1111      held True  scale 1.0  gapB 9.1e-11  d 4.0e-16  |grad| 2.2e+00  ranks [1,3] [0,0] [2,2] [0,0]
    ik        n=40  [12,12,12,12,12]  batch 8  flags 11111111  held True  scale 1.0  gapB 2.1e-11  d 1.1e-14  |grad| 5.6e+00  ranks [10,11,9,10] .. [12,10,11,5] ..
    rank_def  n=5   [3,2,3]           batch 4  flags 0000                                                       |grad| 0.0e+00  ranks [3,0,2] [3,1,1] [3,1,1] [3,1,1]
    mixed     n=5   [3,2,3]           batch 4  flags 1010      held True  scale 1.0  gapB 1.0e-11  d 1.0e-14  |grad| 1.7e+02  ranks [2,2,1] [3,0,2] [3,2,0] [3,1,1]
    budget    n=4   [4,2,2]           batch 6  flags 101010    held True  scale 1.0  gapB 1.8e-10  d 4.3e-16  |grad| 1.3e+00  statuses [0,2,0,2,0,2]
    tile      n=4   [4,1030,2]        batch 2  flags 11                                            d 4.9e-16  |grad| 5.4e+00  ranks [2,1] [1,0]
    D_CPU = 1.14e-14 (ik)  ->  TOL = max(10 D_CPU, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
    largest gapB 1.77e-10 (budget)  ->  FD_BOUND = 1.77e-09, far below the 1e-6 it may not exceed, and nine orders below a wrong sign or a
    missing term (|grad| ~ 1 .. 100).
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

import adjoint_cases as AC  # noqa: E402
import adjoint_matrix_cases as MC  # noqa: E402  (reference_kkt, reference_from_factor, rank_stable, FD_H: imported, not copied)
import lsi_adjoint_cases as LC  # noqa: E402  (final_problem, problems_of: imported, not copied)
from lexls_amd import lexlsi  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

oracle = LC.oracle

D_CPU = 1.14e-14  # measured (1.13e-14, rounded up): the table above (tests/test_lsi_adjoint_matrix_cases.py re-measures it and asserts that TOL still follows from it)
TOL = max(10.0 * D_CPU, 1e-12)
GAP_B = 1.77e-10  # measured (1.761e-10, rounded up): the largest gap of (B), the table above
FD_BOUND = min(10.0 * GAP_B, 1e-6)
FD_H = MC.FD_H
SOLVED, LB, UB, EQ = LC.SOLVED, LC.LB, LC.UB, LC.EQ

# case -> the expected differentiable flags, written out (a kernel cannot pass by flagging an instance away)
FLAGS = {
    "small_sb": [1, 1, 1, 1], "general": [1, 1, 1, 1], "empty_ws": [1, 1, 1, 1], "ik": [1] * 8, "rank_def": [0, 0, 0, 0], "mixed": [1, 0, 1, 0],
    "budget": [1, 0, 1, 0, 1, 0], "tile": [1, 1],
}
CASES = list(FLAGS)
WITH_B = [nm for nm in CASES if nm not in ("rank_def", "tile")]  # the cases (B) runs on: every flag-1 instance of each
RUN_PARAMS = {"budget": dict(max_number_of_factorizations=1)}  # what the case's runs take (oracle.lsi_run and LsiBatch.run alike)
MIXED_SEED = 20330101
# the size of dD's entries per case: 1, unless an instance's working set does not hold under h * dD — then the direction shrinks for that case
DIRECTION_SCALE = {nm: 1.0 for nm in WITH_B}


def spec_of(name):
    """n, seed of a case"""
    if name == "mixed":
        return LC.CASES["general"]["n"], MIXED_SEED
    c = LC.BUDGET if name == "budget" else LC.TILE if name == "tile" else LC.CASES[name]
    return c["n"], c["seed"] + 5000


def problems_of(name):
    if name != "mixed":
        return LC.problems_of(name)
    gen, rdf = LC.problems_of("general"), LC.problems_of("rank_def")
    return [gen[0], rdf[0], gen[1], rdf[1]]


def layout(n, objs):
    """per objective (offset of its block in the flat data, dim, w): a column-major dim x w block, w = n + 2 ([A | lb | ub]) or 2 ([lb | ub])"""
    out, off = [], 0
    for o in objs:
        d, w = len(o["lb"]), 2 if "var" in o else n + 2
        out.append((off, d, w))
        off += d * w
    return out, off


def reference_instance(n, objs, active, status, g):
    """reference (A) for ONE instance: (grad_data (per_data,), flag, ranks of the final problem's levels, d = its discrepancy to the numpy
    restatement of the kernels' steps on the oracle's factor)"""
    lay, per_data = layout(n, objs)
    out = np.zeros(per_data)
    if status != SOLVED:
        return out, 0, None, 0.0
    lod, dims, caps, fixed, rows = LC.final_problem(n, objs, active)
    nf = len(fixed)
    if nf + len(rows) == 0:
        return out, 1, np.zeros(len(dims), np.uint32), 0.0  # an empty working set: x = 0 whatever the data
    idx, val = np.zeros((1, n), np.uint32), np.zeros((1, n))
    for j, (var, value, _, _) in enumerate(fixed):
        idx[0, j], val[0, j] = var, value
    case = dict(n=n, caps=caps, lod=lod[None], dims=dims[None], g=np.asarray(g, float)[None],
                fixed=dict(nfixed=np.asarray([nf], np.uint32), fixed_idx=idx, fixed_val=val) if nf else {})
    ref = MC.run_oracle(case)
    rank, fcol, perm, T = ref["rank"][0], ref["fcol"][0], ref["perm"][0], ref["totalrank"][0]
    if not MC.rank_stable(n, dims, rank, fcol, nf):
        return out, 0, rank, 0.0
    G = MC.reference_kkt(n, lod, dims, rank, perm, T, nf, idx[0], val[0], g)
    y = G[n]
    grad_fixed = np.asarray([g[var] - lod[var] @ y for var, _, _, _ in fixed])
    # the kernels' steps on the oracle's factor, for D_CPU
    GB = MC.reference_from_factor(case, ref, 0)[0]
    fB = AC.adjoint_from_factor(ref["factor"][0], ref["hh"][0], perm, rank, fcol, T, dims, nf, g)[1][:nf]
    scale = max(1.0, float(np.abs(G).max()), float(np.abs(grad_fixed).max()) if nf else 0.0)
    d = max(float(np.abs(G - GB).max()), float(np.abs(grad_fixed - fB).max()) if nf else 0.0) / scale
    first = np.concatenate([[0], np.cumsum([len(o["lb"]) for o in objs])]).astype(int)
    k_of = lambda u: int(np.searchsorted(first, u, side="right") - 1)  # noqa: E731
    for j, (_, _, u, t) in enumerate(fixed):
        off, dm, w = lay[k_of(u)]
        out[off + (w - 2 if t == LB else w - 1) * dm + (u - first[k_of(u)])] = grad_fixed[j]
    for r, (u, t) in enumerate(rows):
        k = k_of(u)
        off, dm, w = lay[k]
        c = u - first[k]
        out[off + np.arange(n) * dm + c] = G[:n, r]
        out[off + (w - 2 if t == LB else w - 1) * dm + c] = y[r]
    return out, 1, rank, d


def direction(seed, n, objs, scale):
    """dD over all data of an instance: scale * N(0, 1) per entry; an equality (lb == ub) keeps lb = ub"""
    lay, per_data = layout(n, objs)
    dD = scale * P.normal(seed, per_data)
    for (off, dm, w), o in zip(lay, objs):
        eq = np.flatnonzero(np.asarray(o["lb"]) == np.asarray(o["ub"]))
        dD[off + (w - 1) * dm + eq] = dD[off + (w - 2) * dm + eq]
    return dD


def central_difference(n, objs, run, g, dD, params):
    """((<g, x(D + h dD)> - <g, x(D - h dD)>) / 2h, held: both perturbed solves ended PROBLEM_SOLVED on the working set of `run`)"""
    dims, types, D, var = lexlsi.flatten(n, objs)
    xs, held = [], True
    for s in (+1.0, -1.0):
        r = oracle.lsi_run(n, lexlsi.unflatten(n, dims, types, D + s * FD_H * dD, var), **params)
        held = held and r["info"]["status"] == SOLVED and all(np.array_equal(a, a0) for a, a0 in zip(r["active"], run["active"]))
        xs.append(r["x"])
    return float(g @ (xs[0] - xs[1])) / (2.0 * FD_H), held


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: n, dims, probs, params (of its runs), runs (the oracle's lsi_run per instance), status, active (batch, total), g (batch, n),
    A = reference (A) (batch, per_data), flags (by the rule, from the oracle), ranks, d = its share of D_CPU; for the cases of WITH_B also
    dD (batch, per_data), fd (batch,), held, gapB"""
    n, seed = spec_of(name)
    probs, params = problems_of(name), RUN_PARAMS.get(name, {})
    B = len(probs)
    runs = [oracle.lsi_run(n, objs, **params) for objs in probs]
    status = np.asarray([r["info"]["status"] for r in runs])
    g = P.normal(seed + 900, B * n).reshape(B, n)
    refs = [reference_instance(n, probs[b], runs[b]["active"], status[b], g[b]) for b in range(B)]
    case = dict(name=name, n=n, dims=np.asarray([len(o["lb"]) for o in probs[0]], np.uint32), probs=probs, params=params, runs=runs, status=status,
                active=np.stack([np.concatenate(r["active"]) for r in runs]), g=g, A=np.stack([r[0] for r in refs]),
                flags=np.asarray([r[1] for r in refs], np.uint8), ranks=[r[2] for r in refs], d=max(r[3] for r in refs))
    if name in WITH_B:
        dD, fd, held, gap = np.zeros_like(case["A"]), np.zeros(B), True, 0.0
        for b in np.flatnonzero(case["flags"]):
            dD[b] = direction(seed + 7000 + b, n, probs[b], DIRECTION_SCALE[name])
            fd[b], ok = central_difference(n, probs[b], runs[b], g[b], dD[b], params)
            held = held and ok
            gap = max(gap, abs(fd[b] - case["A"][b] @ dD[b]) / max(1.0, float(np.abs(case["A"][b] * dD[b]).sum())))
        case.update(dD=dD, fd=fd, held=held, gapB=gap)
    for a in [g, case["A"], case["flags"], case["active"], status, *([case["dD"], case["fd"]] if name in WITH_B else [])]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def split(case, row):
    """one instance's row of grad_data as per-objective dict(A=, lb=, ub=) (simple bounds: lb, ub) and, per user row, whether anything is non-zero"""
    n, objs = case["n"], case["probs"][0]
    dims, types, _, var = lexlsi.flatten(n, objs)
    parts = lexlsi.unflatten(n, dims, types, row, var)
    nonzero = np.concatenate([(np.abs(p["A"]).sum(axis=1) if "A" in p else 0.0) + np.abs(p["lb"]) + np.abs(p["ub"]) for p in parts]) != 0
    return parts, nonzero


def summary(case):
    s = (f"    {case['name']:<9} n={case['n']:<3} {str(case['dims'].tolist()).replace(' ', ''):<17} batch {len(case['probs'])}  flags "
         f"{''.join(str(int(f)) for f in case['flags']):<9}")
    if "gapB" in case:
        s += f" held {case['held']}  scale {DIRECTION_SCALE[case['name']]}  gapB {case['gapB']:.1e}"
    return s + f"  d {case['d']:.1e}  |grad| {np.abs(case['A']).max():.1e}  statuses {case['status'].tolist()}  ranks {[None if r is None else np.asarray(r).tolist() for r in case['ranks']]}"


if __name__ == "__main__":
    worst = worst_b = 0.0
    for nm in CASES:
        cs = build(nm)
        worst, worst_b = max(worst, cs["d"]), max(worst_b, cs.get("gapB", 0.0))
        print(summary(cs))
    print(f"    D_CPU (largest d) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
    print(f"    largest gapB {worst_b:.2e}  ->  FD_BOUND = {min(10 * worst_b, 1e-6):.2e}")
