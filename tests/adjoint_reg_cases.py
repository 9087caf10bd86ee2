"""Cases that hold the adjoint of the REGULARIZED LexLSE solve (lexls_lse_solve_adjoint after a factorization with regularization type 1, 3, 4,
5, 8 or 9 and constant factors; lexls_amd/csrc/lse_adjoint.hip: solve_adjoint_reg_kernel) to two references, both from oracle.lse_run(...,
reg_type=, reg_factors=) and numpy alone (tests/test_adjoint_reg_cases.py asserts on the CPU that they agree; tests/test_gpu_lse_adjoint_reg.py
compares the device with (A)).

With A and the factors held fixed the damped solution is still exactly affine, x = M_reg b + N_reg x_fixed: the damping of a level is a linear map
of the level's right-hand side and of the right-hand-side column of the accumulated null-space basis, both linear in b.
    reference (A)  M_reg and N_reg by unit solves on the oracle with the regularization passed through, then M^T g, N^T g in numpy.
    reference (B)  adjoint_reg_from_factor: the reverse pass in numpy on the oracle's factor, the null-space basis rebuilt from the factor alone
                   (in the factor's final column order, no column swaps: see the kernel's comment).

The data are adjoint_cases.draw's (wide: the same generator at the n where the host's lds/hbm rule switches).  Every case is crossed with
TYPES; `wide` runs for types 1 and 5 only.  Factors per problem and level (factors()): 0.10 .. 0.46, different in every problem; problem 0 has an
exact zero at level 0 and problem 1 a factor of 3e-16 (below the 1e-15 gate of regularize_level) at level 1: for types 1, 3, 8 those levels
still accumulate the null space, and the damped levels behind them read it.
    wide    n = 86 (20, 40, 30), batch 3: adjoint_reg_in_lds (lexls_lds.h) is true up to n = 85 at nObj = 3, cap = 90 and false from 86 on —
            n = 70 is still on the LDS side, so the smallest n of the other side is used.  The order of D reaches 86 > 64: the Cholesky solve's
            second form.
Type 1 takes the dual form (reg_tikhonov_2) at a level when Fc + rank <= RC and the primal form otherwise; TIKHONOV_BRANCHES lists per case which
levels of which problems took which (from the oracle's ranks and first columns; the CPU test asserts it).  Both forms are the same map.

D_CPU is the largest discrepancy (A) against (B), relative to max(1, largest magnitude of the reference), over every case and type; the GPU
tolerance is TOL = max(10 * D_CPU, 1e-12), the rule of tests/adjoint_cases.py, and has to stay at or below 1e-10.
MEASURED (`python tests/adjoint_reg_cases.py`; gap per type 1, 3, 4, 5, 8, 9):
    base            n=3   [2,2,3]            batch 4  lds  gaps 3.3e-16 4.1e-16 4.1e-16 3.7e-16 3.7e-16 1.3e-16
    used_up         n=4   [3,3,3]            batch 4  lds  gaps 3.9e-16 3.9e-16 3.3e-16 5.0e-16 3.9e-16 1.3e-16
    one_row         n=5   [1,3,2]            batch 4  lds  gaps 3.4e-16 2.7e-16 3.1e-16 6.5e-16 5.4e-16 1.7e-16
    rank_def        n=7   [3,3,3]            batch 3  lds  gaps 9.3e-16 7.2e-16 2.3e-15 4.7e-16 9.3e-16 6.9e-17
    ragged          n=5   [2,3,2]            batch 4  lds  gaps 8.7e-16 8.2e-16 1.0e-15 8.0e-16 1.1e-15 2.2e-16
    fixed           n=5   [2,2,3]            batch 4  lds  gaps 5.6e-16 6.3e-16 8.0e-16 5.9e-16 7.3e-16 1.6e-16
    fixed_rank_def  n=7   [3,3,3]            batch 3  lds  gaps 2.5e-15 2.7e-15 3.4e-15 4.2e-15 3.5e-15 5.6e-16
    fixed_ragged    n=5   [2,3,2]            batch 4  lds  gaps 1.1e-15 4.0e-16 3.9e-16 6.4e-16 7.2e-16 2.1e-16
    ik              n=40  [12,12,12,12,12]   batch 8  lds  gaps 8.8e-15 2.9e-14 5.8e-14 3.9e-14 1.2e-14 8.1e-16
    wide            n=86  [20,40,30]         batch 3  hbm  gaps 1.5e-14    -       -    1.6e-14    -       -
    D_CPU = 5.8e-14 (5.75e-14 rounded up: ik, type 4)  ->  TOL = max(10 D_CPU, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
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
from lexls_amd import problems as P  # noqa: E402
from oracle import oracle_ctypes as oracle  # noqa: E402

D_CPU = 5.8e-14  # measured (5.75e-14, rounded up): the table above (tests/test_adjoint_reg_cases.py re-measures it)
TOL = max(10.0 * D_CPU, 1e-12)

TYPES = (1, 3, 4, 5, 8, 9)
ACCUMULATING = (1, 3, 8)  # the types that accumulate (and read) the null-space basis
WIDE_W = (1, 5, 8)        # W = [R | T]; else W = R
NAMES = ("base", "used_up", "one_row", "rank_def", "ragged", "fixed", "fixed_rank_def", "fixed_ragged", "ik", "wide")
WIDE = dict(n=86, dims=[20, 40, 30], batch=3, seed=20320108)
TINY = 3e-16              # a factor below the gate |f| < 1e-15

LDS_LIMIT = 160 * 1024


def types_of(name):
    return (1, 5) if name == "wide" else TYPES


def matrix_doubles(n, nobj):
    """lexls_lds.h: adjoint_reg_matrix_doubles"""
    return 2 * n * n + min(nobj, n) * ((n // 2) * ((n + 1) // 2))


def lds_bytes(n, cap, nobj, in_lds):
    """lexls_lds.h: adjoint_reg_lds_bytes"""
    return (8 * (3 * n + cap + (matrix_doubles(n, nobj) if in_lds else 0)) + 4 * n + 15) & ~15


def variant(n, cap, nobj):
    return "solve_adjoint_reg<64,lds>" if lds_bytes(n, cap, nobj, True) <= LDS_LIMIT else "solve_adjoint_reg<64,hbm>"


def factors(B, nobj):
    f = np.array([[0.1 + 0.04 * ((7 * b + 3 * k) % 10) for k in range(nobj)] for b in range(B)])
    f[0, 0] = 0.0
    if B > 1 and nobj > 1:
        f[1, 1] = TINY
    return f


def draw(name):
    if name != "wide":
        case = AC.draw(name)
    else:
        n, caps, B = WIDE["n"], WIDE["dims"], WIDE["batch"]
        case = dict(name=name, n=n, caps=list(caps), lod=P.lse_batch(WIDE["seed"], B, n, caps), dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), fixed={},
                    g=P.normal(WIDE["seed"] + 900, B * n).reshape(B, n), large=False)
    case["factors"] = factors(case["lod"].shape[0], len(case["caps"]))
    return case


def _run_one(case, b, reg_type, rhs=None, fixed_val=None, reg_factors=None):
    """the oracle on copies of problem b (one per row of rhs, (K, cap); None: the problem's own) under its own factors"""
    K = 1 if rhs is None else rhs.shape[0]
    lod = np.repeat(case["lod"][b:b + 1], K, axis=0).copy()
    if rhs is not None:
        m = int(case["dims"][b].sum())
        lod[:, case["n"], :m] = rhs[:, :m]
    fixed = {}
    if case["fixed"]:
        f = case["fixed"]
        val = np.repeat(f["fixed_val"][b:b + 1], K, axis=0) if fixed_val is None else fixed_val
        fixed = dict(nfixed=np.repeat(f["nfixed"][b:b + 1], K), fixed_idx=np.repeat(f["fixed_idx"][b:b + 1], K, axis=0), fixed_val=val)
    rf = case["factors"][b] if reg_factors is None else reg_factors
    return oracle.lse_run(lod, np.repeat(case["dims"][b:b + 1], K, axis=0), case["n"], maxdim=np.asarray(case["caps"], np.uint32), nthreads=4,
                          reg_type=reg_type, reg_factors=rf, **fixed)


def reference_unit_solves(case, reg_type):
    """reference (A): (grad_rhs (batch, cap), grad_fixed (batch, n)) from M_reg and N_reg by unit solves, a problem at a time (the oracle takes
    one set of factors per call)"""
    n, B, cap = case["n"], case["lod"].shape[0], sum(case["caps"])
    grad_rhs, grad_fixed = np.zeros((B, cap)), np.zeros((B, n))
    for b in range(B):
        m = int(case["dims"][b].sum())
        nf = int(case["fixed"]["nfixed"][b]) if case["fixed"] else 0
        rhs = np.zeros((1 + m + nf, cap))
        rhs[1 + np.arange(m), np.arange(m)] = 1.0
        val = np.zeros((1 + m + nf, n))
        val[1 + m + np.arange(nf), np.arange(nf)] = 1.0
        x = _run_one(case, b, reg_type, rhs, val)["x"]
        cols = x[1:] - x[0]
        grad_rhs[b, :m] = cols[:m] @ case["g"][b]
        grad_fixed[b, :nf] = cols[m:] @ case["g"][b]
    return grad_rhs, grad_fixed


def levels_of(rank, fcol, dims, nf, n):
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    return [(k, int(first[k]), int(fcol[k]), int(dims[k]), int(rank[k])) for k in range(len(dims)) if nf < n and rank[k] > 0]


def adjoint_reg_from_factor(factor, hh, perm, rank, fcol, totalrank, dims, nf, g, reg_type, fac):
    """reference (B) for ONE problem: the reverse pass of the regularized solve in numpy on a kept factor.  Returns (grad_rhs, grad_fixed)"""
    W = factor.T  # W[row, column]
    cap, n, nobj = W.shape[0], len(g), len(dims)
    M, T = int(np.sum(dims)), int(totalrank)
    accum, wide = reg_type in ACCUMULATING, reg_type in WIDE_W
    gh = np.zeros(n)
    for i in range(n):  # (a) gh = P^T g
        p = i
        for k in range(T):
            pk = int(perm[k])
            p = pk if p == k else (k if p == pk else p)
        gh[p] = g[i]
    cb = np.zeros(cap)
    levels = levels_of(rank, fcol, dims, nf, n)
    for k, F, Fc, dim, r in levels:  # (b) the reverse of solve(): the cotangent of the REGULARIZED right-hand sides
        y = np.zeros(r)
        for i in range(r):
            y[i] = (gh[Fc + i] - W[F:F + i, Fc + i] @ y[:i]) / W[F + i, Fc + i]
        cb[F:F + r] = y
        gh[Fc + r:T] -= W[F:F + r, Fc + r:T].T @ y
    NS, snap = np.zeros((n, n)), {}
    if accum:  # the basis as accumulate_nullspace_basis builds it, A side only, in the factor's final column order; U = its rows at entry
        for k, F, Fc, dim, r in levels:
            m0 = Fc - nf
            snap[k] = NS[:m0, Fc:n].copy()
            R = np.triu(W[F:F + r, Fc:Fc + r])
            NS[m0:m0 + r, Fc:Fc + r] = np.eye(r)
            NS[:m0 + r, Fc:Fc + r] = np.linalg.solve(R.T, NS[:m0 + r, Fc:Fc + r].T).T
            NS[:m0 + r, Fc + r:n] -= NS[:m0 + r, Fc:Fc + r] @ W[F:F + r, Fc + r:n]
    rbar = np.zeros(n)
    for k, F, Fc, dim, r in reversed(levels):  # (c)
        if k < nobj - 1:
            cb[F:F + r] -= W[F + dim:M, Fc:Fc + r].T @ cb[F + dim:M]
        m0 = Fc - nf
        R = np.triu(W[F:F + r, Fc:Fc + r])
        if accum:  # r_new = [r; 0] - L y', L = [U_R; I] R^-1
            U = snap[k]
            cb[F:F + r] -= np.linalg.solve(R.T, U[:, :r].T @ rbar[:m0] + rbar[m0:m0 + r])
        f = float(fac[k])
        if not abs(f - 0.0) < 1e-15:
            if reg_type == 9:
                cb[F:F + r] *= f
            else:
                mu = f * f
                Wm = np.hstack([R, W[F:F + r, Fc + r:n]]) if wide else R
                N = Wm.shape[1]
                D = Wm.T @ Wm + mu * np.eye(N)
                if accum:
                    D += mu * U[:, :N].T @ U[:, :N]
                t = np.linalg.solve(D, Wm.T @ cb[F:F + r])
                cb[F:F + r] = Wm @ t
                if accum:
                    rbar[:m0] += mu * U[:, :N] @ t
        for j in range(r - 1, -1, -1):
            tau = hh[F + j]
            if dim - j == 1 or tau == 0.0:
                continue
            v = np.concatenate([[1.0], W[F + j + 1:F + dim, Fc + j]])
            seg = cb[F + j:F + dim]
            seg -= tau * v * (v @ seg)
    grad_fixed = np.zeros(n)
    grad_fixed[:nf] = gh[:nf] - W[:M, :nf].T @ cb[:M]  # (d): the fixed values enter the right-hand side in front of every level
    return cb, grad_fixed


def tikhonov_branches(ref, nf, n):
    """per problem the form type 1 takes at each level of non-zero rank: 'dual' (Fc + rank <= RC) or 'primal'; '-' at rank 0"""
    out = []
    for b in range(len(nf)):
        row = []
        for k in range(ref["rank"].shape[1]):
            r, Fc = int(ref["rank"][b, k]), int(ref["fcol"][b, k])
            row.append("-" if r == 0 or nf[b] >= n else ("dual" if Fc + r <= n - Fc - r else "primal"))
        out.append(row)
    return out


# what tikhonov_branches gives per case (the forms of levels whose factor is below the gate are listed too: they are not taken there)
TIKHONOV_BRANCHES = {
    "base": [["primal", "primal", "-"]] * 4,
    "used_up": [["primal", "primal", "-"]] * 4,
    "one_row": [["dual", "primal", "primal"]] * 4,
    "rank_def": [["dual", "-", "primal"]] * 3,
    "ragged": [["dual", "primal", "-"], ["dual", "-", "primal"], ["dual", "primal", "-"], ["-", "primal", "primal"]],
    "fixed": [["primal", "primal", "-"], ["primal", "primal", "-"], ["-", "-", "-"], ["primal", "primal", "-"]],
    "fixed_rank_def": [["primal", "-", "primal"], ["dual", "-", "primal"], ["primal", "-", "primal"]],
    "fixed_ragged": [["primal", "primal", "-"], ["dual", "-", "primal"], ["primal", "-", "-"], ["-", "primal", "primal"]],
    "ik": [["dual", "primal", "primal", "primal", "-"]] * 8,
    "wide": [["dual", "primal", "primal"]] * 3,
}


@functools.lru_cache(maxsize=None)
def build(name, reg_type):
    """the case under one type: inputs, ref = the oracle's run (a problem at a time: its own factors), A, B, gap"""
    case = draw(name)
    B = case["lod"].shape[0]
    runs = [_run_one(case, b, reg_type) for b in range(B)]
    case["ref"] = {key: np.concatenate([r[key] for r in runs]) for key in ("x", "factor", "hh", "perm", "rank", "fcol", "totalrank")}
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    ref = case["ref"]
    out = [adjoint_reg_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b],
                                   int(nf[b]), case["g"][b], reg_type, case["factors"][b]) for b in range(B)]
    case["B"] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    case["A"] = reference_unit_solves(case, reg_type)
    case["gap"] = max(max(AC._rel(case["A"][i][b] - case["B"][i][b], case["A"][i][b]) for i in (0, 1)) for b in range(B))
    case["nf"], case["reg_type"] = nf, reg_type
    for a in [case["lod"], case["dims"], case["g"], case["factors"], *case["A"], *case["B"], *ref.values(), *case["fixed"].values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def affine_defect(name, reg_type, b=0):
    """|x(b0 + b1) - x(b0) - x(b1) + x(0)| of problem b on the oracle, relative to max(1, |x|): rounding level for an affine map"""
    case = draw(name)
    cap, seed = sum(case["caps"]), 77
    b0, b1 = P.normal(seed, cap), P.normal(seed + 1, cap)
    x = _run_one(case, b, reg_type, np.stack([b0 + b1, b0, b1, np.zeros(cap)]))["x"]
    return float(np.abs(x[0] - x[1] - x[2] + x[3]).max()) / max(1.0, float(np.abs(x).max()))


if __name__ == "__main__":
    worst = 0.0
    for nm in NAMES:
        gaps = {t: build(nm, t)["gap"] for t in types_of(nm)}
        c = build(nm, 1)
        worst = max(worst, *gaps.values())
        print(f"    {nm:<15} n={c['n']:<3} {str(c['caps']).replace(' ', ''):<18} batch {c['lod'].shape[0]}  {variant(c['n'], sum(c['caps']), len(c['caps']))[-4:-1]}  gaps "
              + " ".join(f"{gaps[t]:.1e}" if t in gaps else "   -   " for t in TYPES))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
    for nm in NAMES:
        c = build(nm, 1)
        print(f'    "{nm}": {tikhonov_branches(c["ref"], c["nf"], c["n"])},')
