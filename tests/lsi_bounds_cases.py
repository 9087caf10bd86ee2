"""Cases that hold the re-solve of batched LexLSI working sets on new bounds (lexls_lsi_batch_solve_bounds, lexls_amd/csrc/lsi_final.h:
lsi_bounds_gather_kernel, lexls_lse_solve_rhs_device, lsi_bounds_check_kernel) to references built from the oracle alone
(tests/test_lsi_bounds_cases.py asserts on the CPU that they agree; tests/test_gpu_lsi_solve_bounds.py compares the device with them).

At an instance that ended PROBLEM_SOLVED x is the basic solution of the equality problem of its final working set W: right-hand sides = the active
bounds (lb for CTR_ACTIVE_LB, ub for CTR_ACTIVE_UB and CTR_ACTIVE_EQ), fixed values = the active simple bounds.  For K_ALL other bound sets per
instance:
    reference (A)  W from oracle.lsi_run; the final equality problem RE-FORMED FROM SCRATCH with the new bounds (lsi_adjoint_cases.final_problem on
                   the objectives with the set's bounds) and solved by the oracle's equality solver.
    reference (B)  x_run + M (b_new - b_run) + N (f_new - f_run): the columns of M and N from unit solves on the run's own final problem
                   (adjoint_cases._solve), x_run the x the oracle's LexLSI driver returned.
    semantics      for the first N_SEM sets — perturbations of size SMALL, small enough that the working set holds — the
                   oracle's LexLSI driver run from scratch on the new bounds ends PROBLEM_SOLVED on the same working set (asserted for every solved
                   instance of every case, never skipped) and its x equals (A) within TOL.
The bound sets of an instance: set 0 = the run's own bounds (x must be the run's x), sets 1 .. K_ALL - 2 = small perturbations (all bounds moved,
an equality keeps lb = ub), set K_ALL - 1 = one deliberately large perturbation (LARGE * N(0, 1) on every bound), whose reference violation is > 0.

violation_of() is the definition of the header in numpy, on a given x: over all present rows max(lb - a.x, a.x - ub, lb - ub, 0), x[var] for a.x on
a simple bound.  violation_bound() is the rounding bound the device's own evaluation is held to on the device's own x: per row
gamma_n * sum_j |a_j x_j| for the fma chain of n terms (gamma_n = n u / (1 - n u), u = 2^-53; Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1) plus one ulp of the bound for the subtraction; a maximum of such values moves by at most the largest of them.

Cases — small on purpose:
    sb3       n = 4, simple bounds (3), general (3), general (2, equalities), batch 4
    gen7      n = 7, general objectives only, dims (3, 4, 3), batch 4
    rows      n = 4, simple bounds (4), general (70), general (2, equalities), batch 2: 76 user rows, more than one pass of 64 and more than four
              chunks of 16 rows; rows 5 and 66 of the second objective are equalities, the others out of reach
    ik        lsi_adjoint_cases' ik: n = 40, simple bounds (12) + 4 x 12, batch 8 — the shape of BASELINE configs[4]
    empty_ws  lsi_adjoint_cases' empty_ws: instances 1 and 3 end with an empty working set
    rank_def  lsi_adjoint_cases' rank_def: a level of the final problem has rank < rows
    budget    lsi_adjoint_cases' budget: run with max_number_of_factorizations = 1, instances 1, 3, 5 do not end PROBLEM_SOLVED
    lds46     n = 46, general (3, 4, 3), batch 2: the last nVar whose x tile lives in LDS (lexls_lds.h: bounds_check_placement)
    hbm47     n = 47, the same: the first nVar that reads x from global memory

D_CPU is the largest gap between (A) and (B), relative to max(1, |x|_inf), over all cases, solved instances and bound sets.  TOL = 10 * D_CPU: the
factor 10 allows for fma contraction and summation orders that differ from the oracle's; it never comes from device figures.
MEASURED (`python tests/lsi_bounds_cases.py`, the oracle and numpy alone):
    sb3       n=4   [3,3,2]            batch 4  status [0,0,0,0]          |W| [5,4,6,6]                  held True  (A)-(B) 4.4e-16  driver-(A) 3.3e-16  violation own 5.8e-01 large 1.6e+01
    gen7      n=7   [3,4,3]            batch 4  status [0,0,0,0]          |W| [8,9,7,8]                  held True  (A)-(B) 7.9e-16  driver-(A) 6.1e-16  violation own 1.3e+00 large 1.7e+01
    rows      n=4   [4,70,2]           batch 2  status [0,0]              |W| [7,5]                      held True  (A)-(B) 4.4e-16  driver-(A) 2.2e-16  violation own 2.9e+00 large 1.5e+01
    lds46     n=46  [3,4,3]            batch 2  status [0,0]              |W| [9,10]                     held True  (A)-(B) 1.2e-15  driver-(A) 8.0e-16  violation own 4.4e-16 large 1.1e+01
    hbm47     n=47  [3,4,3]            batch 2  status [0,0]              |W| [8,10]                     held True  (A)-(B) 3.9e-16  driver-(A) 2.8e-16  violation own 4.4e-16 large 1.9e+01
    ik        n=40  [12,12,12,12,12]   batch 8  status [0,0,0,0,0,0,0,0]  |W| [42,42,47,42,42,41,45,43]  held True  (A)-(B) 5.3e-15  driver-(A) 3.8e-15  violation own 2.5e+00 large 3.6e+01
    empty_ws  n=4   [3,3]              batch 4  status [0,0,0,0]          |W| [4,0,5,0]                  held True  (A)-(B) 7.2e-16  driver-(A) 3.6e-16  violation own 6.8e-02 large 1.4e+01
    rank_def  n=5   [3,2,3]            batch 4  status [0,0,0,0]          |W| [7,8,8,8]                  held True  (A)-(B) 1.1e-15  driver-(A) 6.0e-16  violation own 4.5e+00 large 1.1e+01
    budget    n=4   [4,2,2]            batch 6  status [0,2,0,2,0,2]      |W| [2,3,2,3,2,3]              held True  (A)-(B) 3.3e-16  driver-(A) 0.0e+00  violation own 8.9e-16 large 0.0e+00
    ("violation own": the largest violation of set 0 — rows of lower priority that the lexicographic optimum itself leaves unmet count;
     "large": the smallest violation of the large set, 0 only where an instance did not end PROBLEM_SOLVED)
    D_CPU = 6e-15 (ik: measured 5.27e-15, rounded up to one digit — (B)'s matrix products go through the BLAS numpy finds, whose summation order
    is not the same everywhere)  ->  TOL = 10 D_CPU = 6e-14.
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

import adjoint_cases as AC  # noqa: E402  (_solve: imported, not copied)
import lsi_adjoint_cases as LC  # noqa: E402  (final_problem, with_bounds, bounds_of, problems_of)
from lexls_amd import problems as P  # noqa: E402
from oracle import oracle_ctypes as oracle  # noqa: E402

D_CPU = 6e-15  # measured (5.27e-15, rounded up to one digit): the table above (tests/test_lsi_bounds_cases.py re-measures it and asserts that TOL still follows from it)
TOL = 10.0 * D_CPU
K_ALL = 66   # bound sets per instance: the run's own, 64 small perturbations, one large
N_SEM = 3    # of the small ones, those the oracle's driver is run from scratch on
SMALL = 1e-5  # size of the small perturbations: every solved instance of every case keeps its working set under it (build() records it, the CPU test asserts it)
LARGE = 10.0
SOLVED = LC.SOLVED

OWN = {
    "sb3": dict(n=4, dims=(3, 3, 2), simple=True, batch=4, seed=20340101),
    "gen7": dict(n=7, dims=(3, 4, 3), simple=False, batch=4, seed=20340201),
    "rows": dict(n=4, dims=(4, 70, 2), simple=True, batch=2, seed=20340301, equalities=(5, 66), far=100.0),
    "lds46": dict(n=46, dims=(3, 4, 3), simple=False, batch=2, seed=20340401),
    "hbm47": dict(n=47, dims=(3, 4, 3), simple=False, batch=2, seed=20340501),
}
BORROWED = ("ik", "empty_ws", "rank_def", "budget")
CASES = list(OWN) + list(BORROWED)
RUN_PARAMS = {"budget": dict(max_number_of_factorizations=1)}  # what the case's runs take (oracle.lsi_run and LsiBatch.run alike)


def spec_of(name):
    return OWN[name] if name in OWN else LC.BUDGET if name == "budget" else LC.CASES[name]


def problems_of(name):
    if name in BORROWED:
        return LC.problems_of(name)
    c, out = OWN[name], []
    for i in range(c["batch"]):
        objs = P.lsi_problem(c["seed"] + i, c["n"], c["dims"], simple_bounds=c["simple"])
        if c.get("equalities"):  # level 1: inequalities far away from anything x can reach (|x_i| <= 1), but for two equalities
            o = objs[1]
            keep = np.zeros(len(o["lb"]), bool)
            keep[list(c["equalities"])] = True
            mid = 0.5 * (o["lb"] + o["ub"])
            o["lb"], o["ub"] = np.where(keep, mid, o["lb"] - c["far"]), np.where(keep, mid, o["ub"] + c["far"])
        out.append(objs)
    return out


def bound_sets(seed, objs):
    """(lb, ub), each (K_ALL, total): the run's own bounds, the small perturbations, the large one"""
    lb0, ub0 = LC.bounds_of(objs)
    lbs, ubs = [lb0], [ub0]
    for c in range(1, K_ALL - 1):
        size = np.where(lb0 == ub0, SMALL, np.minimum(SMALL, 0.1 * (ub0 - lb0)))  # (lsi_adjoint_cases.perturbation's rule at another size)
        dl, du = size * P.normal(seed + 31 * c, lb0.size, 1), size * P.normal(seed + 31 * c, lb0.size, 2)
        lbs.append(lb0 + dl), ubs.append(ub0 + np.where(lb0 == ub0, dl, du))
    dl, du = LARGE * P.normal(seed + 9001, lb0.size, 1), LARGE * P.normal(seed + 9001, lb0.size, 2)
    du = np.where(lb0 == ub0, dl, du)
    lbs.append(lb0 + dl), ubs.append(ub0 + du)
    return np.stack(lbs), np.stack(ubs)


def formed_batch(n, forms):
    """final problems (lsi_adjoint_cases.final_problem) of one shape as the case dict adjoint_cases._solve and oracle.lse_run take"""
    B = len(forms)
    nf = np.asarray([len(f[3]) for f in forms], np.uint32)
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b, f in enumerate(forms):
        for j, (var, value, _, _) in enumerate(f[3]):
            idx[b, j], val[b, j] = var, value
    return dict(n=n, caps=forms[0][2], lod=np.stack([f[0] for f in forms]), dims=np.stack([f[1] for f in forms]),
                fixed=dict(nfixed=nf, fixed_idx=idx, fixed_val=val) if nf.any() else {})


def equality_solve(fb):
    return oracle.lse_run(fb["lod"], fb["dims"], fb["n"], maxdim=np.asarray(fb["caps"], np.uint32), nthreads=4, **fb["fixed"])["x"]


def violation_of(n, objs, x, counts=None):
    """the header's definition for ONE instance and ONE x: objs carry the bound set; counts: present rows per objective (None: all)"""
    worst = 0.0
    for k, o in enumerate(objs):
        m = len(o["lb"]) if counts is None else int(counts[k])
        ax = x[o["var"][:m].astype(int)] if "var" in o else _fma_rows(o["A"][:m], x)
        lb, ub = o["lb"][:m], o["ub"][:m]
        for val in (lb - ax, ax - ub, lb - ub):
            if m:
                worst = max(worst, float(np.max(val)))
    return worst


def _fma_rows(A, x):
    """a.x per row in extended precision: the reference's own rounding stays far below violation_bound()"""
    return np.asarray(A.astype(np.longdouble) @ x.astype(np.longdouble), np.float64)


def violation_bound(n, objs, x, counts=None):
    """how far an ordered fma evaluation of violation_of() may be from any other evaluation on the same x: the largest per-row bound"""
    u = 2.0 ** -53
    gamma = n * u / (1.0 - n * u)
    worst = 0.0
    for k, o in enumerate(objs):
        m = len(o["lb"]) if counts is None else int(counts[k])
        if not m:
            continue
        mag = np.zeros(m) if "var" in o else np.abs(o["A"][:m]) @ np.abs(x)
        ulp = np.maximum(np.spacing(np.abs(o["lb"][:m])), np.spacing(np.abs(o["ub"][:m])))
        worst = max(worst, float(np.max(gamma * mag + ulp)))
    return worst


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: n, probs, params, runs (the oracle's lsi_run per instance), active (batch, total), status (batch,), x_run (batch, n),
    lb / ub (K_ALL, batch, total), A and B (K_ALL, batch, n; zeros where the instance did not end PROBLEM_SOLVED), violation (K_ALL, batch) of (A),
    held / sem_gap (the semantic check), gap = the case's share of D_CPU"""
    c = spec_of(name)
    n, B, seed = c["n"], c["batch"], c["seed"]
    params = RUN_PARAMS.get(name, {})
    probs = problems_of(name)
    runs = [oracle.lsi_run(n, objs, **params) for objs in probs]
    status = np.asarray([r["info"]["status"] for r in runs])
    total = sum(len(o["lb"]) for o in probs[0])
    lb, ub = np.zeros((K_ALL, B, total)), np.zeros((K_ALL, B, total))
    A, Bref, viol = np.zeros((K_ALL, B, n)), np.zeros((K_ALL, B, n)), np.zeros((K_ALL, B))
    held, sem_gap, gap = True, 0.0, 0.0
    for i, objs in enumerate(probs):
        lb[:, i], ub[:, i] = bound_sets(seed + 5000 + 100 * i, objs)
        if status[i] != SOLVED:
            continue
        act = runs[i]["active"]
        empty = not any(np.asarray(a).any() for a in act)
        sets = [LC.with_bounds(objs, lb[c_, i], ub[c_, i]) for c_ in range(K_ALL)]
        if not empty:
            forms = [LC.final_problem(n, s_, act) for s_ in sets]
            A[:, i] = equality_solve(formed_batch(n, forms))
            # (B): unit solves on the run's own final problem
            one = formed_batch(n, forms[:1])
            cap, m, nf = sum(one["caps"]), int(one["dims"].sum()), len(forms[0][3])
            x0 = AC._solve(one, np.zeros((1, cap)))["x"][0]
            M, N = np.zeros((n, cap)), np.zeros((n, n))
            for r in range(m):
                e = np.zeros((1, cap))
                e[0, r] = 1.0
                M[:, r] = AC._solve(one, e)["x"][0] - x0
            for j in range(nf):
                val = np.zeros((1, n))
                val[0, j] = 1.0
                N[:, j] = AC._solve(one, np.zeros((1, cap)), val)["x"][0] - x0
            rhs = np.stack([f[0][n] for f in forms])
            fix = np.zeros((K_ALL, n))
            for c_, f in enumerate(forms):
                fix[c_, :nf] = [v for _, v, _, _ in f[3]]
            Bref[:, i] = runs[i]["x"] + (rhs - rhs[0]) @ M.T + (fix - fix[0]) @ N.T
            for c_ in range(K_ALL):
                gap = max(gap, float(np.abs(A[c_, i] - Bref[c_, i]).max()) / max(1.0, float(np.abs(A[c_, i]).max())))
        for c_ in range(K_ALL):
            viol[c_, i] = violation_of(n, sets[c_], A[c_, i])
        for c_ in range(1, 1 + N_SEM):
            r1 = oracle.lsi_run(n, sets[c_], **params)
            held = held and r1["info"]["status"] == SOLVED and all(np.array_equal(a, a0) for a, a0 in zip(r1["active"], act))
            sem_gap = max(sem_gap, float(np.abs(r1["x"] - A[c_, i]).max()) / max(1.0, float(np.abs(A[c_, i]).max())))
    case = dict(name=name, n=n, dims=np.asarray(c["dims"], np.uint32), probs=probs, params=params, runs=runs, status=status,
                active=np.stack([np.concatenate(r["active"]) for r in runs]), x_run=np.stack([r["x"] for r in runs]), lb=lb, ub=ub, A=A, B=Bref,
                violation=viol, held=held, sem_gap=sem_gap, gap=gap)
    for a in [case["active"], status, case["x_run"], lb, ub, A, Bref, viol]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def summary(case):
    nact = (case["active"] != 0).sum(axis=1)
    return (f"    {case['name']:<9} n={case['n']:<3} {str(case['dims'].tolist()).replace(' ', ''):<18} batch {len(case['probs'])}  status {str(case['status'].tolist()).replace(' ', ''):<14} "
            f"|W| {str(nact.tolist()).replace(' ', ''):<26} held {case['held']}  (A)-(B) {case['gap']:.1e}  driver-(A) {case['sem_gap']:.1e}  "
            f"violation own {case['violation'][0].max():.1e} large {case['violation'][-1].min():.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in CASES:
        cs = build(nm)
        worst = max(worst, cs["gap"])
        print(summary(cs))
    print(f"    D_CPU (largest (A)-(B) gap) {worst:.2e}  ->  TOL = 10 D_CPU = {10 * worst:.2e}")
