"""Cases that hold lexls_lse_solve_rhs (new right-hand sides and fixed values on a kept factor, plain and damped; lexls_amd/csrc/lse_adjoint.hip:
solve_rhs_front_kernel, apply_solve_map_kernel, apply_solve_map_multi_kernel, apply_solve_map_reg_multi_kernel) to two references, both from
oracle.lse_run and numpy alone (tests/test_solve_rhs_cases.py asserts on the CPU that they agree; tests/test_gpu_lse_solve_rhs.py compares the
device with (a)).

factorize() chooses pivots and ranks from A alone, so x = M b + N x_fixed exactly; the same holds after a damped factorization of type 1, 3, 4, 5,
8 or 9 with constant factors.  Per case and type (0 = plain), K = 65 right-hand sides and sets of fixed values per problem:
    reference (a)  the oracle factorizing and solving [A | b_new] with fixed_new from scratch, under the same regularization settings.
    reference (b)  solve_rhs_from_factor: the forward pass in numpy over the oracle's kept factor — the transpose, statement for statement, of the
                   reverse passes adjoint_cases.adjoint_from_factor and adjoint_reg_cases.adjoint_reg_from_factor.
    transposition  <g, x(b, f)> = <M^T g, b> + <N^T g, f> with M^T g, N^T g from those reverse passes.

Cases — the smallest shapes at which each branch can go wrong (data: adjoint_cases.draw / adjoint_reg_cases.draw, so the factors have an exact
zero at level 0 of problem 0 and 3e-16, below the gate, at level 1 of problem 1):
    six             n = 6 (2, 3, 2), full rank
    used_up         n = 4 (3, 3, 3): the last level finds the columns used up
    rank_def        n = 7 (3, 3, 3), ranks (2, 0, 2): a repeated-row level of rank < dim and a level of rank 0
    ragged          n = 5, capacities (2, 3, 2), per-problem dimensions with empty levels
    fixed           n = 5 (2, 2, 3): two, two, ALL and one variable fixed
    fixed_rank_def  rank-deficient levels behind fixed columns, nfixed (2, 1, 3)
    fixed_ragged    per-problem dimensions behind fixed columns, nfixed (2, 0, 4, 1)
    ik              n = 40, 5 x 12, batch 8: the project's shape
    mid             n = 60 (20, 40, 30), batch 2: the damped kernel's matrices leave LDS (solve_rhs_reg<64,hbm>)
    wide            n = 86 (20, 40, 30), batch 3: its per-lane state leaves LDS too (solve_rhs_reg<64,work>)
mid and wide run plain and for types 1 and 5 (as adjoint_reg_cases' wide), every other case for all of 0, 1, 3, 4, 5, 8, 9.

D_CPU is the largest discrepancy (a) against (b) over every case, type, problem and right-hand side, relative to max(1, largest magnitude of
the reference row); the GPU tolerance is TOL = 10 * D_CPU.  A central difference of the oracle in b with step JVP_STEP = 1 has no truncation
error on a linear map, only rounding: its largest gap to (b) over the damped ik cases is D_JVP, and JVP_TOL = 10 * D_JVP.
MEASURED (`python tests/solve_rhs_cases.py`; gap per type 0, 1, 3, 4, 5, 8, 9):
    case            n     capacities         batch    plain  damped  gaps
    six             n=6   [2,3,2]            batch 4  staged lds   1.4e-15 5.2e-15 7.9e-15 1.0e-14 9.3e-15 7.7e-15 1.0e-15
    used_up         n=4   [3,3,3]            batch 4  staged lds   1.0e-15 2.1e-15 2.6e-15 2.6e-15 1.9e-15 1.9e-15 4.0e-16
    rank_def        n=7   [3,3,3]            batch 3  staged lds   1.1e-15 2.3e-15 3.8e-15 7.4e-15 1.4e-15 2.4e-15 6.7e-16
    ragged          n=5   [2,3,2]            batch 4  staged lds   1.1e-15 3.7e-15 2.3e-15 2.3e-15 2.9e-15 3.1e-15 9.9e-16
    fixed           n=5   [2,2,3]            batch 4  staged lds   8.9e-16 9.3e-16 1.4e-15 1.4e-15 1.3e-15 1.3e-15 7.8e-16
    fixed_rank_def  n=7   [3,3,3]            batch 3  staged lds   1.4e-15 3.6e-15 4.4e-15 8.4e-15 4.7e-15 4.0e-15 7.2e-16
    fixed_ragged    n=5   [2,3,2]            batch 4  staged lds   5.4e-16 3.3e-15 1.4e-15 1.1e-15 3.3e-15 3.0e-15 4.1e-16
    ik              n=40  [12,12,12,12,12]   batch 8  staged lds   3.0e-15 4.0e-14 3.1e-14 5.6e-14 3.7e-14 3.6e-14 1.2e-15
    mid             n=60  [20,40,30]         batch 2  staged hbm   4.6e-15 1.2e-13    -       -    2.4e-13    -       -
    wide            n=86  [20,40,30]         batch 3  staged work  2.3e-15 3.2e-14    -       -    3.9e-14    -       -
    D_CPU = 2.4e-13 (2.39e-13 rounded up: mid, type 5)  ->  TOL = 10 D_CPU = 2.4e-12, a fortieth of the 1e-10 of the tolerance contract.
    Transposition identity, largest defect 1.6e-14.  D_JVP = 5.3e-14 (5.28e-14 rounded up)  ->  JVP_TOL = 5.3e-13.
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
import adjoint_reg_cases as RC  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

D_CPU = 2.4e-13  # measured (2.39e-13, rounded up): the table above (tests/test_solve_rhs_cases.py re-measures it)
TOL = 10.0 * D_CPU
JVP_STEP = 1.0
D_JVP = 5.3e-14  # measured (5.28e-14, rounded up)
JVP_TOL = 10.0 * D_JVP

K = 65
TYPES = (0,) + RC.TYPES
NAMES = ("six", "used_up", "rank_def", "ragged", "fixed", "fixed_rank_def", "fixed_ragged", "ik", "mid", "wide")
OWN = {"six": dict(n=6, dims=[2, 3, 2], batch=4, seed=20330101), "mid": dict(n=60, dims=[20, 40, 30], batch=2, seed=20330102)}
LDS_LIMIT = 160 * 1024


def types_of(name):
    return (0, 1, 5) if name in ("mid", "wide") else TYPES


# ---- the host's placement rules restated (lexls_lds.h); tests/test_solve_rhs_cases.py holds them to tests/solve_rhs_fit_check.cpp ----
def reg_lds_bytes(n, cap, form):
    b = 8 * n + (8 * 65 * (3 * n + cap) if form != "work" else 0) + (16 * n * n if form == "lds" else 0)
    return (b + 15) & ~15


def reg_variant(n, cap):
    for form in ("lds", "hbm"):
        if reg_lds_bytes(n, cap, form) <= LDS_LIMIT:
            return f"solve_rhs_reg<64,{form}>"
    return "solve_rhs_reg<64,work>"


def plain_lds_bytes(n, cap, staged):
    return (8 * 65 * (n + cap) + 8 * n + (8 * ((cap | 1) * n + cap) if staged else 0) + 15) & ~15


def plain_variant(n, cap, k=2):
    if k == 1:
        return "solve_rhs<64,single>"
    if plain_lds_bytes(n, cap, True) <= LDS_LIMIT:
        return "solve_rhs<64,staged>"
    return "solve_rhs<64,lds>" if plain_lds_bytes(n, cap, False) <= LDS_LIMIT else "solve_rhs<64,work>"


def variant(name_or_case, reg_type, k=2):
    c = draw(name_or_case) if isinstance(name_or_case, str) else name_or_case
    return reg_variant(c["n"], sum(c["caps"])) if reg_type else plain_variant(c["n"], sum(c["caps"]), k)


def draw(name):
    """inputs of a case: adjoint_reg_cases.draw's dictionary (n, caps, lod, dims, fixed, g, factors) + rhs (K, batch, cap), fixed_new (K, batch, n)"""
    if name in OWN:
        c = OWN[name]
        n, caps, B, seed = c["n"], list(c["dims"]), c["batch"], c["seed"]
        case = dict(name=name, n=n, caps=caps, lod=P.lse_batch(seed, B, n, caps), dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), fixed={},
                    g=P.normal(seed + 900, B * n).reshape(B, n), large=False)
        case["factors"] = RC.factors(B, len(caps))
    else:
        case = RC.draw(name)
    B, n, cap = case["lod"].shape[0], case["n"], sum(case["caps"])
    seed = 20330200 + 10 * NAMES.index(name)
    case["rhs"] = P.normal(seed, K * B * cap).reshape(K, B, cap)
    case["fixed_new"] = P.normal(seed + 1, K * B * n).reshape(K, B, n)
    case["nf"] = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    return case


def positions(perm, T, n):
    """pos[i] = the position variable i reaches by following the transpositions first to last"""
    pos = np.arange(n)
    for i in range(n):
        p = i
        for k in range(T):
            pk = int(perm[k])
            p = pk if p == k else (k if p == pk else p)
        pos[i] = p
    return pos


def solve_rhs_from_factor(factor, hh, perm, rank, fcol, totalrank, dims, nf, rhs, fixed, reg_type, fac):
    """reference (b) for ONE problem and ONE right-hand side: the forward pass of the (damped) solve in numpy on a kept factor.  Returns x (n,)"""
    W = factor.T  # W[row, column]
    cap, n, nobj = W.shape[0], W.shape[1] - 1, len(dims)
    M, T = int(np.sum(dims)), int(totalrank)
    accum, wide = reg_type in RC.ACCUMULATING, reg_type in RC.WIDE_W
    t = np.zeros(cap)
    t[:M] = rhs[:M] - W[:M, :nf] @ fixed[:nf]  # the fixed values enter the right-hand side in front of every level
    levels = RC.levels_of(rank, fcol, dims, nf, n)
    NS, r = np.zeros((n, n)), np.zeros(n)
    for k, F, Fc, dim, rk in levels:
        for j in range(rk):  # the level's reflectors, first to last
            tau = hh[F + j]
            if dim - j == 1 or tau == 0.0:
                continue
            v = np.concatenate([[1.0], W[F + j + 1:F + dim, Fc + j]])
            seg = t[F + j:F + dim]
            seg -= tau * v * (v @ seg)
        R = np.triu(W[F:F + rk, Fc:Fc + rk])
        m0 = Fc - nf
        y = t[F:F + rk].copy()
        if reg_type:
            U = NS[:m0, Fc:n].copy()  # the basis as it stands at the level's entry
            f = float(fac[k])
            if not abs(f - 0.0) < 1e-15:
                if reg_type == 9:
                    y = f * y
                else:
                    mu = f * f
                    Wm = np.hstack([R, W[F:F + rk, Fc + rk:n]]) if wide else R
                    N = Wm.shape[1]
                    D, d = Wm.T @ Wm + mu * np.eye(N), Wm.T @ y
                    if accum:
                        D += mu * U[:, :N].T @ U[:, :N]
                        d += mu * U[:, :N].T @ r[:m0]
                    y = Wm @ np.linalg.solve(D, d)
            if accum:  # r <- [r; 0] - [U_R; I] R^-1 y', then the level's step of the basis
                s = np.linalg.solve(R, y)
                r[:m0] -= U[:, :rk] @ s
                r[m0:m0 + rk] = -s
                NS[m0:m0 + rk, Fc:Fc + rk] = np.eye(rk)
                NS[:m0 + rk, Fc:Fc + rk] = np.linalg.solve(R.T, NS[:m0 + rk, Fc:Fc + rk].T).T
                NS[:m0 + rk, Fc + rk:n] -= NS[:m0 + rk, Fc:Fc + rk] @ W[F:F + rk, Fc + rk:n]
        t[F:F + rk] = y
        if k < nobj - 1:  # the Gauss step
            t[F + dim:M] -= W[F + dim:M, Fc:Fc + rk] @ y
    z = np.zeros(n)
    for k, F, Fc, dim, rk in reversed(levels):  # solve(): the block back-substitution
        R = np.triu(W[F:F + rk, Fc:Fc + rk])
        z[Fc:Fc + rk] = np.linalg.solve(R, t[F:F + rk] - W[F:F + rk, Fc + rk:T] @ z[Fc + rk:T])
    pos = positions(perm, T, n)
    return np.array([fixed[p] if p < nf else (z[p] if p < T else 0.0) for p in pos])


def rel_rows(got, ref):
    """largest error per row (last axis), relative to max(1, largest magnitude of that reference row)"""
    err = np.abs(got - ref).max(axis=-1)
    return float((err / np.maximum(1.0, np.abs(ref).max(axis=-1))).max())


def reference_a(case, reg_type, rhs, fixed_new):
    """x (K, batch, n) by the oracle from scratch, a problem at a time (the oracle takes one set of factors per call)"""
    B = case["lod"].shape[0]
    return np.stack([RC._run_one(case, b, reg_type, np.ascontiguousarray(rhs[:, b]), np.ascontiguousarray(fixed_new[:, b]))["x"] for b in range(B)], axis=1)


@functools.lru_cache(maxsize=None)
def build(name, reg_type):
    """the case under one type: inputs, ref = the oracle's own run, a, b (K, batch, n), gap, trans = the transposition identity's gap"""
    case = draw(name)
    B, n = case["lod"].shape[0], case["n"]
    runs = [RC._run_one(case, b, reg_type) for b in range(B)]
    ref = case["ref"] = {key: np.concatenate([r[key] for r in runs]) for key in ("x", "factor", "hh", "perm", "rank", "fcol", "totalrank")}
    nf = case["nf"]
    case["a"] = reference_a(case, reg_type, case["rhs"], case["fixed_new"])
    kept = lambda b: (ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b], int(nf[b]))  # noqa: E731
    case["b"] = np.stack([np.stack([solve_rhs_from_factor(*kept(b), case["rhs"][c, b], case["fixed_new"][c, b], reg_type, case["factors"][b])
                                    for b in range(B)]) for c in range(K)])
    case["gap"] = rel_rows(case["b"], case["a"])
    trans = 0.0
    for b in range(B):
        if reg_type:
            grad_rhs, grad_fixed = RC.adjoint_reg_from_factor(*kept(b), case["g"][b], reg_type, case["factors"][b])
        else:
            grad_rhs, grad_fixed = AC.adjoint_from_factor(*kept(b), case["g"][b])
        m = int(case["dims"][b].sum())
        for c in range(4):
            terms = np.concatenate([case["g"][b] * case["a"][c, b], -grad_rhs[:m] * case["rhs"][c, b, :m], -grad_fixed[:nf[b]] * case["fixed_new"][c, b, :nf[b]]])
            trans = max(trans, abs(terms.sum()) / max(1.0, float(np.abs(terms).sum())))
    case["trans"], case["reg_type"] = trans, reg_type
    for arr in [case["lod"], case["dims"], case["g"], case["factors"], case["rhs"], case["fixed_new"], case["a"], case["b"], *ref.values(), *case["fixed"].values()]:
        arr.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def own_rhs(case):
    """(batch, cap): the right-hand-side column of the case's own problem data"""
    return np.ascontiguousarray(case["lod"][:, case["n"], :])


def jvp_gap(name, reg_type, ndir=3):
    """central difference of the oracle in b (step JVP_STEP, the fixed values held) against reference (b) on (db, 0): the largest relative gap"""
    case = build(name, reg_type)
    B, n, ref, nf = case["lod"].shape[0], case["n"], case["ref"], case["nf"]
    db, b0 = case["rhs"][:ndir], own_rhs(case)[None]
    keep = np.repeat(case["fixed"]["fixed_val"][None], ndir, axis=0) if case["fixed"] else np.zeros((ndir, B, n))
    fd = (reference_a(case, reg_type, b0 + JVP_STEP * db, keep) - reference_a(case, reg_type, b0 - JVP_STEP * db, keep)) / (2 * JVP_STEP)
    lin = np.stack([np.stack([solve_rhs_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b],
                                                    case["dims"][b], int(nf[b]), db[c, b], np.zeros(n), reg_type, case["factors"][b]) for b in range(B)])
                    for c in range(ndir)])
    return rel_rows(lin, fd), fd


if __name__ == "__main__":
    worst = worst_t = 0.0
    for nm in NAMES:
        gaps = {t: build(nm, t) for t in types_of(nm)}
        c = gaps[0]
        worst = max(worst, *(v["gap"] for v in gaps.values()))
        worst_t = max(worst_t, *(v["trans"] for v in gaps.values()))
        print(f"    {nm:<15} n={c['n']:<3} {str(c['caps']).replace(' ', ''):<18} batch {c['lod'].shape[0]}  {variant(c, 0)[10:-1]:<7}{variant(c, 1)[14:-1]:<5} gaps "
              + " ".join(f"{gaps[t]['gap']:.1e}" if t in gaps else "   -   " for t in TYPES))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = 10 D_CPU = {10 * worst:.2e};  transposition identity, largest defect {worst_t:.2e}")
    dj = max(jvp_gap("ik", t)[0] for t in RC.TYPES)
    print(f"    D_JVP (ik, damped, step {JVP_STEP}) {dj:.2e}  ->  JVP_TOL = {10 * dj:.2e}")
