"""Cases that hold the gradient of the LexLSE solve with respect to the matrix (lexls_lse_solve_adjoint_matrix, lexls_amd/csrc/lse_adjoint.hip:
apply_solve_map + adjoint_matrix_kernel) to two references (tests/test_adjoint_matrix_cases.py asserts on the CPU that they agree;
tests/test_gpu_lse_adjoint_matrix.py compares the device with reference (A)).

A problem is RANK-STABLE when rank_k == min(dim_k, n - Fc_k) for every level k (Fc_k the level's first column, fixed variables included; a level
that finds the columns used up has rank 0 and passes; a problem with every variable fixed passes).  There the levels above the last one of
non-zero rank, k*, are equalities C x = d, level k* is a least-squares objective min |E x - f|, the later levels do not touch x, and with
g = dloss/dx
    dloss/dA_k = - y_k x^T - lambda_k u^T,   dloss/db = y
y = M^T g (solve_adjoint's grad_rhs), lambda = [nu; r; 0] the multipliers of level k* (r = E x - f, E^T r + C^T nu = 0 on the pivot variables),
u = M y~ with y~ = y on the rows of level k* and 0 elsewhere.  G (batch, n + 1, cap) has the layout of the problem data: column j < n the
gradient of column j of A, column n the gradient of the right-hand side.  A problem that is not rank-stable has differentiable = 0 and G = 0.
    reference (A)  the KKT system of that equality-constrained least-squares problem on the ORIGINAL data, solved with numpy.linalg.solve:
                   x, nu from K [x; nu] = [E^T f; d], u and y from K [u; w] = [g; 0] (y_C = w, y_E = E u).  From the oracle's run it takes the
                   ranks (the level structure) and the transpositions (which variables stay free at total rank < n), nothing of the factor.
    reference (B)  a numpy restatement of the kernels' steps on the oracle's factor: adjoint_cases.adjoint_from_factor for y,
                   multipliers_from_factor for lambda, apply_solve_map for u, the assembly.
    duality        <g, apply_solve_map(r)> == <adjoint(g), r> for a random r: apply_solve_map is the transpose of the adjoint.
    sanity         central differences (h = 1e-6) of oracle.lse_run over every entry of `base` and `one_row` and 200 drawn entries of `ik`
                   against (A): a truncation-error check (FD_BOUND), never the device tolerance.

Cases (expected flags as literals, FLAGS; the tests also compute them from the oracle's ranks by the rule):
    base            n = 3 (2, 2, 3)                                              1
    used_up         n = 4 (3, 3, 3)                                              1
    one_row         n = 5 (1, 3, 2)                                              1
    ragged          n = 5, capacities (2, 3, 2), four dimension sets             1 1 1 1   total rank < n in two (free variables); absent rows zero
    fixed           n = 5 (2, 2, 3), four fixed sets                             1 1 1 1   the all-fixed problem among them
    fixed_tall      n = 12 (70, 30)                                              1 1       reflectors over 70 rows, a Gauss step over 100
    ik              n = 40, 5 x 12, batch 8                                      1 x 8     the project's own workload
    wide            n = 70 (20, 40, 30)                                          1 1 1     second trip over the columns
    rank_def        n = 7 (3, 3, 3), ranks (2, 0, 2)                             0 0 0     G entirely zero
    fixed_rank_def  the same behind fixed variables                              0 0 0     G entirely zero
    mixed           n = 7 (3, 3, 3): a full-rank problem beside a rank_def one   1 0       the flag and the zeros are per problem

D_CPU is the largest (A)-vs-(B) gap, relative to max(1, largest magnitude of the reference) per problem.  TOL = max(10 D_CPU, 1e-12) — the
factor 10 allows for fma contraction and other summation orders, the project's rule for the adjoint — and has to stay <= 1e-10; data that
would need more get another seed, the tolerance is not raised.
MEASURED (`python tests/adjoint_matrix_cases.py`; gap = (A) vs (B), dual = the duality gap, |G| = the largest magnitude of (A)):
    base            n=3    [2,2,3]            batch 4  flags 1111      gap 1.4e-15  dual 2.5e-16  |G| 1.8e+02
    used_up         n=4    [3,3,3]            batch 4  flags 1111      gap 4.4e-16  dual 3.4e-16  |G| 1.3e+01
    one_row         n=5    [1,3,2]            batch 4  flags 1111      gap 8.9e-16  dual 1.7e-16  |G| 7.3e+00
    ragged          n=5    [2,3,2]            batch 4  flags 1111      gap 5.0e-15  dual 3.3e-16  |G| 9.8e+00
    fixed           n=5    [2,2,3]            batch 4  flags 1111      gap 1.4e-15  dual 6.7e-16  |G| 1.0e+01
    fixed_tall      n=12   [70,30]            batch 2  flags 11        gap 8.3e-17  dual 5.6e-17  |G| 1.6e-01
    ik              n=40   [12,12,12,12,12]   batch 8  flags 11111111  gap 7.2e-14  dual 3.3e-15  |G| 1.1e+01
    wide            n=70   [20,40,30]         batch 3  flags 111       gap 1.7e-13  dual 1.5e-15  |G| 2.9e+00
    rank_def        n=7    [3,3,3]            batch 3  flags 000       gap 0.0e+00  dual 2.8e-16  |G| 0.0e+00
    fixed_rank_def  n=7    [3,3,3]            batch 3  flags 000       gap 0.0e+00  dual 1.1e-16  |G| 0.0e+00
    mixed           n=7    [3,3,3]            batch 2  flags 10        gap 1.7e-15  dual 1.6e-15  |G| 2.1e+01
    D_CPU = 1.70e-13 (wide)  ->  TOL = max(10 D_CPU, 1e-12) = 1.7e-12, well inside the 1e-10 of the tolerance contract.
    central differences, h = 1e-6, against (A): base 112 entries gap 2.1e-10, one_row 144 entries gap 4.9e-10, ik 200 entries gap 2.9e-09.
    FD_BOUND = 1e-7.  The rounding term of a central difference is eps |g| |x| cond / h: with eps / h = 2e-10 and the worst gap measured at 3e-9
    a bound of 1e-7 leaves a factor 30 for other data of the same shapes, and is still eight orders below a wrong sign or a missing term
    (|G| ~ 10).  The truncation term h^2 |x'''| / 6 ~ 1e-12 |x'''| does not count beside it.
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

D_CPU = 1.70e-13  # measured: the table above (tests/test_adjoint_matrix_cases.py re-measures it and asserts that TOL still follows from it)
TOL = max(10.0 * D_CPU, 1e-12)
FD_BOUND = 1e-7  # the central differences against (A): see the table above
FD_H = 1e-6

# case -> the expected differentiable flags, written out (a kernel cannot pass by flagging a problem away)
FLAGS = {
    "base": [1, 1, 1, 1], "used_up": [1, 1, 1, 1], "one_row": [1, 1, 1, 1], "ragged": [1, 1, 1, 1], "fixed": [1, 1, 1, 1], "fixed_tall": [1, 1],
    "ik": [1] * 8, "wide": [1, 1, 1], "rank_def": [0, 0, 0], "fixed_rank_def": [0, 0, 0], "mixed": [1, 0],
}
CASES = list(FLAGS)
MIXED_SEED = 20320101
# the producers of the kept factor per case (adjoint_cases.PRODUCERS; `mixed` has the shape of rank_def)
PRODUCERS = {nm: AC.PRODUCERS["rank_def" if nm == "mixed" else nm] for nm in CASES}


def draw(name):
    """adjoint_cases.draw, and the mixed batch: a full-rank and a rank-deficient problem of one shape side by side"""
    if name != "mixed":
        return AC.draw(name)
    n, caps = 7, [3, 3, 3]
    lod = np.stack([P.lse_problem(MIXED_SEED, n, caps), P.rank_deficient_problem(MIXED_SEED + 1, n, caps, [2, 0, 2])])
    return dict(name=name, n=n, caps=caps, lod=lod, dims=np.tile(np.asarray(caps, np.uint32), (2, 1)), fixed={},
                g=P.normal(MIXED_SEED + 900, 2 * n).reshape(2, n), large=False)


def run_oracle(case, lod=None):
    return oracle.lse_run(case["lod"] if lod is None else lod, case["dims"], case["n"], maxdim=np.asarray(case["caps"], np.uint32), nthreads=4,
                          **case["fixed"])


def rank_stable(n, dims, rank, fcol, nf):
    """the rule, as the kernel evaluates it: every variable fixed passes; else rank_k == min(dim_k, n - Fc_k) for every level (0 where Fc_k >= n)"""
    if nf >= n:
        return 1
    return int(all(int(rank[k]) == min(int(dims[k]), max(n - int(fcol[k]), 0)) for k in range(len(dims))))


def last_level(n, dims, rank, fcol, totalrank, nf):
    """k*: the last level of non-zero rank as the kernels trust it (adjoint_from_factor's levels), -1 without one"""
    ks = [k for k in range(len(dims)) if nf < n and rank[k] > 0]
    return ks[-1] if ks else -1


def position(perm, T, i):
    """the factor column of user variable i: the transpositions followed first to last (solve_adjoint_kernel's step (a))"""
    p = i
    for k in range(T):
        pk = int(perm[k])
        p = pk if p == k else (k if p == pk else p)
    return p


def reference_kkt(n, lod, dims, rank, perm, totalrank, nf, fixed_idx, fixed_val, g):
    """reference (A) for ONE rank-stable problem: G (n + 1, cap) from the dense KKT system on the original data"""
    cap = lod.shape[1]
    A, b = lod[:n].T, lod[n]  # A[row, variable]
    G = np.zeros((n + 1, cap))
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    ks = [k for k in range(len(dims)) if nf < n and rank[k] > 0]
    if not ks:
        return G
    kstar, T = ks[-1], int(totalrank)
    pos = [position(perm, T, i) for i in range(n)]
    S = [i for i in range(n) if nf <= pos[i] < T]  # the pivot variables: neither fixed nor free
    xfull = np.zeros(n)
    for j in range(nf):
        xfull[int(fixed_idx[j])] = fixed_val[j]
    rc = np.arange(first[0], first[kstar])          # rows of the equalities
    re = np.arange(first[kstar], first[kstar + 1])  # rows of the objective
    C, E = A[np.ix_(rc, S)], A[np.ix_(re, S)]
    d, f = b[rc] - A[rc] @ xfull, b[re] - A[re] @ xfull
    ns, nc = len(S), len(rc)
    K = np.zeros((ns + nc, ns + nc))
    K[:ns, :ns], K[:ns, ns:], K[ns:, :ns] = E.T @ E, C.T, C
    sol = np.linalg.solve(K, np.concatenate([E.T @ f, d]))
    adj = np.linalg.solve(K, np.concatenate([g[S], np.zeros(nc)]))
    xfull[S] = sol[:ns]
    u = np.zeros(n)
    u[S] = adj[:ns]
    y, lam = np.zeros(cap), np.zeros(cap)
    y[rc], y[re] = adj[ns:], E @ adj[:ns]
    lam[rc], lam[re] = sol[ns:], E @ sol[:ns] - f
    G[:n] = -np.outer(xfull, y) - np.outer(u, lam)
    G[n] = y
    return G


def apply_q(W, hh, F, Fc, dim, r, v):
    """v <- Q_k v in place (apply_q_block): the level's reflectors, last first"""
    for j in range(r - 1, -1, -1):
        tau = hh[F + j]
        if dim - j == 1:
            v[j] *= 1.0 - tau
        elif tau != 0.0:
            ess = W[F + j + 1:F + dim, Fc + j]
            t = ess @ v[j + 1:] + v[j]
            v[j] -= tau * t
            v[j + 1:] -= tau * ess * t
    return v


def multipliers_from_factor(W, hh, rank, fcol, dims, nf, kstar):
    """the multipliers of level kstar in LOD row order (sensitivity_kernel's steps; its output holds them behind the nf fixed variables)"""
    cap, n = W.shape[0], W.shape[1] - 1
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    lam, rhs = np.zeros(cap), np.zeros(n)
    F, Fc, dim, r = int(first[kstar]), int(fcol[kstar]), int(dims[kstar]), int(rank[kstar])
    lam[F + r:F + dim] = -W[F + r:F + dim, n]
    apply_q(W, hh, F, Fc, dim, r, lam[F:F + dim])
    rhs[:Fc] -= W[F:F + dim, :Fc].T @ lam[F:F + dim]
    for k in range(kstar - 1, -1, -1):
        F, Fc, dim, r = int(first[k]), int(fcol[k]), int(dims[k]), int(rank[k])
        lam[F:F + r] = rhs[Fc:Fc + r]
        apply_q(W, hh, F, Fc, dim, r, lam[F:F + dim])
        rhs[:Fc] -= W[F:F + dim, :Fc].T @ lam[F:F + dim]
    return lam


def apply_solve_map(W, hh, perm, rank, fcol, totalrank, dims, nf, rhs):
    """u = M rhs for ONE problem (fixed values zero), the steps of the apply_solve_map kernel: the transpose of adjoint_from_factor's (c), (b), (a)"""
    cap, n, nobj = W.shape[0], W.shape[1] - 1, len(dims)
    M, T = int(np.sum(dims)), int(totalrank)
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    levels = [(k, int(first[k]), int(fcol[k]), int(dims[k]), int(rank[k])) for k in range(nobj) if nf < n and rank[k] > 0]
    t = np.array(rhs[:cap], float)
    t[M:] = 0.0
    for k, F, Fc, dim, r in levels:  # the right-hand-side updates of factorize(): reflectors first to last, then the Gauss step
        for j in range(r):
            tau = hh[F + j]
            if dim - j == 1 or tau == 0.0:
                continue
            v = np.concatenate([[1.0], W[F + j + 1:F + dim, Fc + j]])
            seg = t[F + j:F + dim]
            seg -= tau * v * (v @ seg)
        t[F + dim:M] -= W[F + dim:M, Fc:Fc + r] @ t[F:F + r]
    z = np.zeros(n)
    for k, F, Fc, dim, r in reversed(levels):  # back-substitution, column by column
        for c in range(T - 1, Fc + r - 1, -1):
            t[F:F + r] -= W[F:F + r, c] * z[c]
        for j in range(r - 1, -1, -1):
            z[Fc + j] = t[F + j] / W[F + j, Fc + j]
            t[F:F + j] -= W[F:F + j, Fc + j] * z[Fc + j]
    z[:nf] = 0.0
    return np.array([z[p] if nf <= p < T else 0.0 for p in (position(perm, T, i) for i in range(n))])


def reference_from_factor(case, ref, b):
    """reference (B) for problem b of a case: (G (n + 1, cap), u, lambda, y) from the oracle's factor"""
    n, cap = case["n"], case["lod"].shape[2]
    nf = int(case["fixed"]["nfixed"][b]) if case["fixed"] else 0
    W, hh, perm, rank, fcol, T, dims = ref["factor"][b].T, ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b]
    y, _ = AC.adjoint_from_factor(ref["factor"][b], hh, perm, rank, fcol, T, dims, nf, case["g"][b])
    G = np.zeros((n + 1, cap))
    G[n] = y
    kstar = last_level(n, dims, rank, fcol, T, nf)
    u, lam = np.zeros(n), np.zeros(cap)
    G[:n] = -np.outer(ref["x"][b], y)
    if kstar >= 0:
        first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        yt = np.zeros(cap)
        yt[first[kstar]:first[kstar + 1]] = y[first[kstar]:first[kstar + 1]]
        u = apply_solve_map(W, hh, perm, rank, fcol, T, dims, nf, yt)
        lam = multipliers_from_factor(W, hh, rank, fcol, dims, nf, kstar)
        G[:n] -= np.outer(u, lam)
    return G, u, lam, y


def unit_solve_columns(case):
    """M (batch, n, cap) by unit solves on the oracle (fixed values zero): what lexls_internal_apply_solve_map has to reproduce on e_i"""
    B, cap = case["lod"].shape[0], case["lod"].shape[2]
    x0 = AC._solve(case, np.zeros((B, cap)))["x"]
    cols = np.zeros((B, case["n"], cap))
    m = case["dims"].sum(axis=1)
    for i in range(cap):
        e = np.zeros((B, cap))
        e[:, i] = 1.0
        cols[:, :, i] = np.where((i < m)[:, None], AC._solve(case, e)["x"] - x0, 0.0)
    return cols


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: its inputs (draw), ref = the oracle's run, flags (by the rule from the oracle's ranks), A / B = G of the two references
    (batch, n + 1, cap; zero where the flag is 0), gap = the case's share of D_CPU, dual = the duality gap of apply_solve_map"""
    case = draw(name)
    n, B, cap = case["n"], case["lod"].shape[0], case["lod"].shape[2]
    ref = case["ref"] = run_oracle(case)
    fx = case["fixed"]
    nfs = [int(fx["nfixed"][b]) if fx else 0 for b in range(B)]
    case["nf"] = np.asarray(nfs)
    case["flags"] = np.array([rank_stable(n, case["dims"][b], ref["rank"][b], ref["fcol"][b], nfs[b]) for b in range(B)], np.uint8)
    GA, GB = np.zeros((B, n + 1, cap)), np.zeros((B, n + 1, cap))
    gap = dual = 0.0
    for b in range(B):
        W = ref["factor"][b].T
        r = P.normal(CASE_SEED(name) + 40 + b, cap)
        lhs = case["g"][b] @ apply_solve_map(W, ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b], nfs[b], r)
        yb, _ = AC.adjoint_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b],
                                       nfs[b], case["g"][b])
        rhs = yb @ r
        dual = max(dual, abs(lhs - rhs) / max(1.0, abs(lhs), abs(rhs)))
        if not case["flags"][b]:
            continue
        GA[b] = reference_kkt(n, case["lod"][b], case["dims"][b], ref["rank"][b], ref["perm"][b], ref["totalrank"][b], nfs[b],
                              fx["fixed_idx"][b] if fx else None, fx["fixed_val"][b] if fx else None, case["g"][b])
        GB[b] = reference_from_factor(case, ref, b)[0]
        gap = max(gap, AC._rel(GA[b] - GB[b], GA[b]))
    case["A"], case["B"], case["gap"], case["dual"] = GA, GB, gap, dual
    for a in [case["lod"], case["dims"], case["g"], GA, GB, case["flags"], *ref.values(), *fx.values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def CASE_SEED(name):
    return MIXED_SEED if name == "mixed" else AC.CASES[name]["seed"]


def loss_gradient_fd(case, entries, h=FD_H):
    """central differences of <g, x> by the oracle: entries = [(b, j, i)], j <= n the column of the problem data, i the row; one run per sign serves
    every problem of the batch that has an entry with that (j, i)"""
    out = {}
    for (j, i) in sorted({(j, i) for _, j, i in entries}):
        xs = []
        for s in (+1.0, -1.0):
            lod = case["lod"].copy()
            lod[:, j, i] += s * h
            xs.append(run_oracle(case, lod)["x"])
        d = ((xs[0] - xs[1]) * case["g"]).sum(axis=1) / (2 * h)
        for b, jj, ii in entries:
            if (jj, ii) == (j, i):
                out[(b, j, i)] = d[b]
    return out


def fd_entries(name):
    case = build(name)
    n, B = case["n"], case["lod"].shape[0]
    m = case["dims"].sum(axis=1)
    if name == "ik":
        pick = (P.uniform(CASE_SEED(name) + 77, 600) * np.tile([B, n + 1, int(m.min())], 200)).astype(int).reshape(200, 3)
        return [tuple(int(v) for v in e) for e in pick]
    return [(b, j, i) for b in range(B) for j in range(n + 1) for i in range(int(m[b]))]


def fd_gap(name):
    """the largest gap between the central differences and reference (A) over the case's entries, relative to max(1, largest |G| of the problem)"""
    case = build(name)
    entries = fd_entries(name)
    fd = loss_gradient_fd(case, entries)
    return max(abs(fd[e] - case["A"][e[0], e[1], e[2]]) / max(1.0, float(np.abs(case["A"][e[0]]).max())) for e in entries)


def summary(case):
    return (f"    {case['name']:<15} n={case['n']:<4} {str(case['caps']).replace(' ', ''):<18} batch {case['lod'].shape[0]}  flags "
            f"{''.join(str(int(f)) for f in case['flags']):<9} gap {case['gap']:.1e}  dual {case['dual']:.1e}  |G| {np.abs(case['A']).max():.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in CASES:
        c = build(nm)
        worst = max(worst, c["gap"])
        print(summary(c))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
    for nm in ("base", "one_row", "ik"):
        print(f"    central differences, h = {FD_H:g}: {nm:<8} {len(fd_entries(nm)):>4} entries  gap {fd_gap(nm):.1e}")
