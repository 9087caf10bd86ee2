"""Cases that hold the forward-mode tangents of the LexLSE solve (lexls_lse_solve_tangent*, lexls_amd/csrc/lse_adjoint.hip: tangent_rhs_kernel +
apply_solve_map_multi_kernel) to three references (tests/test_tangent_cases.py asserts on the CPU that they agree; tests/test_gpu_lse_tangent.py
compares the device with reference (A)).  The cases, their data and their oracle runs are those of tests/adjoint_matrix_cases.py.

For a RANK-STABLE problem (adjoint_matrix_cases: the rule) and a direction d[A | b] (dlod, the layout of the problem data) and dx_fixed (dfixed,
one entry per fixed SLOT, the layout of solve_adjoint's grad_fixed):
    dx = M [ (db - dA x - A_fixed dx_fixed) - E_k* M^T (dA^T lambda) ]   on the pivot variables,   dx = dx_fixed on the fixed ones,   0 on the free
x the solution, lambda the multipliers of level k*, the last level of non-zero rank (its own rows hold A x - b), E_k* = keep the rows of level
k*, M the solve map, M^T the adjoint.  A problem that is not rank-stable has differentiable = 0 and dx = 0.
    reference (A)  the KKT system K [x; nu] = [E^T f; d] of the equality-constrained least-squares problem on the ORIGINAL data, differentiated:
                   [dx; dnu] = K^-1 (d rhs - dK [x; nu]), with numpy.linalg.solve.  The signs of the formula above were fixed against it.
    reference (B)  a numpy restatement of the kernels' steps on the oracle's factor: the two right-hand sides, adjoint_cases.adjoint_from_factor
                   for M^T, adjoint_matrix_cases.apply_solve_map for M, the fixed slots.
    reference (C)  central differences (h = 1e-6) of oracle.lse_run along the direction: a truncation-error check of (A) (FD_BOUND of
                   adjoint_matrix_cases, whose reasoning covers a directional derivative of unit-scale data as it covers one entry), never the
                   device tolerance.
    duality        <g, dx> == <grad_lod(g), dlod> + <N^T g, dfixed> with grad_lod reference (A) of adjoint_matrix_cases and N^T g reference (B) of
                   adjoint_cases: forward and reverse mode are transposes of one another.

NTAN = 3 directions per case, drawn standard normal over the whole of dlod and dfixed (rows behind a problem's own and slots behind nfixed
included: they must not be read).
D_CPU is the largest (A)-vs-(B) gap, relative to max(1, largest magnitude of the reference) per problem and tangent.  TOL = 10 D_CPU: the factor
10 of adjoint_matrix_cases (fma contraction, other summation orders), without that module's floor of 1e-12; it has to stay <= 1e-10.
MEASURED (`python tests/tangent_cases.py`; gap = (A) vs (B), dual = the duality gap, |dx| = the largest magnitude of (A)):
    base            n=3    [2,2,3]            batch 4  flags 1111      gap 2.4e-15  dual 1.9e-16  |dx| 2.6e+02
    used_up         n=4    [3,3,3]            batch 4  flags 1111      gap 5.3e-15  dual 2.2e-16  |dx| 7.7e+00
    one_row         n=5    [1,3,2]            batch 4  flags 1111      gap 1.5e-15  dual 1.5e-16  |dx| 1.3e+01
    ragged          n=5    [2,3,2]            batch 4  flags 1111      gap 4.8e-15  dual 2.7e-16  |dx| 3.5e+01
    fixed           n=5    [2,2,3]            batch 4  flags 1111      gap 2.8e-15  dual 1.7e-16  |dx| 9.6e+00
    fixed_tall      n=12   [70,30]            batch 2  flags 11        gap 6.1e-16  dual 3.2e-17  |dx| 2.0e+00
    ik              n=40   [12,12,12,12,12]   batch 8  flags 11111111  gap 9.1e-14  dual 3.7e-15  |dx| 7.4e+01
    wide            n=70   [20,40,30]         batch 3  flags 111       gap 7.0e-14  dual 2.3e-15  |dx| 1.6e+01
    rank_def        n=7    [3,3,3]            batch 3  flags 000       gap 0.0e+00  dual 0.0e+00  |dx| 0.0e+00
    fixed_rank_def  n=7    [3,3,3]            batch 3  flags 000       gap 0.0e+00  dual 0.0e+00  |dx| 0.0e+00
    mixed           n=7    [3,3,3]            batch 2  flags 10        gap 4.8e-15  dual 1.3e-16  |dx| 2.0e+01
    D_CPU = 9.1e-14 (ik)  ->  TOL = 10 D_CPU = 9.1e-13.
    central differences, h = 1e-6, against (A): base 3.2e-09, fixed 4.0e-10, ik 1.1e-09.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import adjoint_cases as AC  # noqa: E402
import adjoint_matrix_cases as AM  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

D_CPU = 9.1e-14  # measured: the table above (tests/test_tangent_cases.py re-measures it and asserts that TOL still follows from it)
TOL = 10.0 * D_CPU
FD_BOUND, FD_H = AM.FD_BOUND, AM.FD_H
NTAN = 3
CASES = list(AM.CASES)
FLAGS = AM.FLAGS
PRODUCERS = AM.PRODUCERS


# ---- the placement rule, restated from lexls_amd/csrc/lexls_lds.h (tangent_map_lds_bytes, tangent_map_placement); tests/test_tangent_cases.py
# holds the restatement to tests/tangent_fit_check.cpp's numbers ----
LDS_LIMIT = 160 * 1024  # kMaxLdsBytes: one workgroup's LDS
STAGED, LDS, WORK = "solve_tangent<64,staged>", "solve_tangent<64,lds>", "solve_tangent<64,work>"


def lds_bytes(n, cap, place):
    """the per-lane vectors z (n) and t (cap), [index][lane] with leading dimension 65, and 2 n words of transpositions and positions; staged:
    + the factor's n columns (odd leading dimension cap | 1) and hh (cap); work: the 2 n words alone (the vectors sit in a work buffer)"""
    if place == WORK:
        return (8 * n + 15) & ~15
    b = 8 * 65 * (n + cap) + 8 * n
    if place == STAGED:
        b += 8 * ((cap | 1) * n + cap)
    return (b + 15) & ~15


def placement(n, cap):
    return STAGED if lds_bytes(n, cap, STAGED) <= LDS_LIMIT else (LDS if lds_bytes(n, cap, LDS) <= LDS_LIMIT else WORK)


def last_cap(n, place):
    """the largest cap the rule still gives `place` at n variables (the rule is monotone in cap)"""
    cap = 1
    while placement(n, cap + 1) == place or placement(n, cap) != place:
        cap += 1
    return cap


# device runs on both sides of the rule's two switches at n = 40, batch 2, iid data in levels of 12 rows: the first four levels take the 40
# columns (ranks 12, 12, 12, 4: rank-stable), every later level finds them used up
FIT_N = 40
FIT_CAPS = {"fit_staged_last": last_cap(FIT_N, STAGED), "fit_lds_first": last_cap(FIT_N, STAGED) + 1, "fit_lds_last": last_cap(FIT_N, LDS),
            "fit_work_first": last_cap(FIT_N, LDS) + 1}
FIT_NAMES = list(FIT_CAPS)
FIT_SEED = 20330301
PLACEMENTS = {name: placement(FIT_N, cap) for name, cap in FIT_CAPS.items()}


@functools.lru_cache(maxsize=None)
def _fit_case(name):
    cap = FIT_CAPS[name]
    caps = [12] * (cap // 12) + ([cap % 12] if cap % 12 else [])
    n, B, seed = FIT_N, 2, FIT_SEED + FIT_NAMES.index(name)
    case = dict(name=name, n=n, caps=caps, lod=P.lse_batch(seed, B, n, caps), dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), fixed={},
                g=P.normal(seed + 900, B * n).reshape(B, n), large=False)
    ref = case["ref"] = AM.run_oracle(case)
    case["nf"] = np.zeros(B, int)
    case["flags"] = np.array([AM.rank_stable(n, case["dims"][b], ref["rank"][b], ref["fcol"][b], 0) for b in range(B)], np.uint8)
    for a in [case["lod"], case["dims"], case["g"], case["flags"], *ref.values()]:
        a.setflags(write=False)
    return case


def base_case(name):
    """the inputs, the oracle's run and the flags of a case: adjoint_matrix_cases.build(name), or one of the fit cases above"""
    return _fit_case(name) if name in FIT_CAPS else AM.build(name)


def case_seed(name):
    return FIT_SEED + 100 * (1 + FIT_NAMES.index(name)) if name in FIT_CAPS else AM.CASE_SEED(name)


def draw_tangents(name, K, salt=0):
    """K directions for case `name`: dlod (K, batch, n + 1, cap) and dfixed (K, batch, n), standard normal in every entry"""
    case = base_case(name)
    B, n, cap = case["lod"].shape[0], case["n"], case["lod"].shape[2]
    seed = case_seed(name) + 5000 + 17 * salt
    dlod = P.normal(seed, K * B * (n + 1) * cap).reshape(K, B, n + 1, cap)
    dfixed = P.normal(seed + 1, K * B * n).reshape(K, B, n)
    return dlod, dfixed


def fixed_of(case, b):
    """(nf, the variables of the fixed slots, their values) of problem b"""
    fx = case["fixed"]
    if not fx:
        return 0, np.zeros(0, int), np.zeros(0)
    nf = int(fx["nfixed"][b])
    return nf, np.asarray(fx["fixed_idx"][b][:nf], int), np.asarray(fx["fixed_val"][b][:nf], float)


def tangent_kkt(n, lod, dims, rank, perm, totalrank, nf, fidx, fval, dlod, dfixed):
    """reference (A) for ONE rank-stable problem and ONE direction: dx (n,) from the differentiated KKT system on the original data"""
    A, b = lod[:n].T, lod[n]
    dA, db = dlod[:n].T, dlod[n]
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    dx = np.zeros(n)
    xf, dxf = np.zeros(n), np.zeros(n)
    xf[fidx], dxf[fidx] = fval, dfixed[:nf]
    dx[fidx] = dfixed[:nf]
    ks = [k for k in range(len(dims)) if nf < n and rank[k] > 0]
    if not ks:
        return dx
    kstar, T = ks[-1], int(totalrank)
    pos = [AM.position(perm, T, i) for i in range(n)]
    S = [i for i in range(n) if nf <= pos[i] < T]
    rc, re = np.arange(first[0], first[kstar]), np.arange(first[kstar], first[kstar + 1])
    C, E, dC, dE = A[np.ix_(rc, S)], A[np.ix_(re, S)], dA[np.ix_(rc, S)], dA[np.ix_(re, S)]
    d, f = b[rc] - A[rc] @ xf, b[re] - A[re] @ xf
    dd, df = db[rc] - dA[rc] @ xf - A[rc] @ dxf, db[re] - dA[re] @ xf - A[re] @ dxf
    ns, nc = len(S), len(rc)
    K, dK = np.zeros((ns + nc, ns + nc)), np.zeros((ns + nc, ns + nc))
    K[:ns, :ns], K[:ns, ns:], K[ns:, :ns] = E.T @ E, C.T, C
    dK[:ns, :ns], dK[:ns, ns:], dK[ns:, :ns] = dE.T @ E + E.T @ dE, dC.T, dC
    sol = np.linalg.solve(K, np.concatenate([E.T @ f, d]))
    dsol = np.linalg.solve(K, np.concatenate([dE.T @ f + E.T @ df, dd]) - dK @ sol)
    dx[S] = dsol[:ns]
    return dx


def tangent_from_factor(case, ref, b, dlod, dfixed):
    """reference (B) for problem b and ONE direction: the kernels' steps on the oracle's factor.  Returns (dx, r, w): the two right-hand sides
    tangent_rhs_kernel forms, r (cap,) and w (n,)"""
    n, cap = case["n"], case["lod"].shape[2]
    nf = fixed_of(case, b)[0]
    W, hh, perm, rank, fcol, T, dims = ref["factor"][b].T, ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], case["dims"][b]
    M = int(np.sum(dims))
    first = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    dA, db = dlod[:n].T, dlod[n]
    kstar = AM.last_level(n, dims, rank, fcol, T, nf)
    lam = AM.multipliers_from_factor(W, hh, rank, fcol, dims, nf, kstar) if kstar >= 0 else np.zeros(cap)
    r = np.zeros(cap)
    r[:M] = db[:M] - dA[:M] @ ref["x"][b] - W[:M, :nf] @ dfixed[:nf]  # (the fixed slots' share: the transpose of solve_adjoint's step (d))
    w = dA[:M].T @ lam[:M]
    t = r.copy()
    if kstar >= 0:
        y, _ = AC.adjoint_from_factor(ref["factor"][b], hh, perm, rank, fcol, T, dims, nf, w)
        t[first[kstar]:first[kstar + 1]] -= y[first[kstar]:first[kstar + 1]]
    dx = AM.apply_solve_map(W, hh, perm, rank, fcol, T, dims, nf, t)
    for i in range(n):
        p = AM.position(perm, int(T), i)
        if p < nf:
            dx[i] = dfixed[p]
    return dx, r, w


def _run(case, lod, fixed_val):
    fx = dict(case["fixed"])
    if fx:
        fx["fixed_val"] = fixed_val
    return AM.oracle.lse_run(lod, case["dims"], case["n"], maxdim=np.asarray(case["caps"], np.uint32), nthreads=4, **fx)["x"]


def central_differences(name, dlod, dfixed, h=FD_H):
    """reference (C): (x(data + h d) - x(data - h d)) / 2h by the oracle, one direction (batch, ...) — rows behind a problem's own and slots
    behind nfixed do not reach the oracle's x"""
    case = base_case(name)
    fv = case["fixed"]["fixed_val"] if case["fixed"] else None
    xs = [_run(case, case["lod"] + s * h * dlod, None if fv is None else fv + s * h * dfixed) for s in (+1.0, -1.0)]
    return (xs[0] - xs[1]) / (2 * h)


@functools.lru_cache(maxsize=None)
def build(name, K=NTAN, salt=0, with_b=True):
    """the case `name` with K directions: case = adjoint_matrix_cases.build(name) (shared, read-only), dlod, dfixed, A / B = dx of the two
    references (K, batch, n; zero where the flag is 0; with_b = False: (A) alone, B and gap are None), gap = the case's share of D_CPU, dual = the duality gap"""
    case = base_case(name)
    ref = case["ref"]
    B, n = case["lod"].shape[0], case["n"]
    dlod, dfixed = draw_tangents(name, K, salt)
    XA, XB = np.zeros((K, B, n)), np.zeros((K, B, n))
    gap = dual = 0.0
    for b in range(B):
        if not case["flags"][b]:
            continue
        nf, fidx, fval = fixed_of(case, b)
        _, grad_fixed = AC.adjoint_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b],
                                               case["dims"][b], nf, case["g"][b])
        m = int(case["dims"][b].sum())
        for c in range(K):
            XA[c, b] = tangent_kkt(n, case["lod"][b], case["dims"][b], ref["rank"][b], ref["perm"][b], ref["totalrank"][b], nf, fidx, fval,
                                   dlod[c, b], dfixed[c, b])
            if with_b:
                XB[c, b] = tangent_from_factor(case, ref, b, dlod[c, b], dfixed[c, b])[0]
                gap = max(gap, AC._rel(XA[c, b] - XB[c, b], XA[c, b]))
            if "A" in case:  # (the fit cases have no reverse-mode reference)
                terms = np.concatenate([case["g"][b] * XA[c, b], -(case["A"][b][:, :m] * dlod[c, b][:, :m]).ravel(), -grad_fixed[:nf] * dfixed[c, b][:nf]])
                dual = max(dual, abs(terms.sum()) / max(1.0, float(np.abs(terms).sum())))
    out = dict(case=case, dlod=dlod, dfixed=dfixed, A=XA, B=XB if with_b else None, gap=gap if with_b else None, dual=dual)
    for a in (dlod, dfixed, XA, XB):
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return out


def fd_gap(name):
    """the largest gap between (C) and (A) over the case's directions, relative to max(1, largest |dx| of the problem and direction)"""
    t = build(name)
    worst = 0.0
    for c in range(NTAN):
        fd = central_differences(name, t["dlod"][c], t["dfixed"][c])
        for b in range(fd.shape[0]):
            if t["case"]["flags"][b]:
                worst = max(worst, AC._rel(fd[b] - t["A"][c, b], t["A"][c, b]))
    return worst


# ---- LexLSI batches (lexls_lsi_batch_solve_tangent): the instances of tests/lsi_adjoint_matrix_cases.py ----
# At an instance that ended PROBLEM_SOLVED on a rank-stable final problem, dx is the LexLSE tangent of that final problem along the direction the
# active rows carry: an active general row its dA row and dlb (CTR_ACTIVE_LB) or dub (CTR_ACTIVE_UB, CTR_ACTIVE_EQ), an active simple bound its
# dlb / dub entry as the tangent of the fixed value; every other instance has flag 0 and dx = 0; an empty working set has flag 1 and dx = 0.
#     (A) tangent_kkt on the final problem's original data, (B) tangent_from_factor on the oracle's factor of it, (C) central differences through
#     the whole oracle LexLSI driver along the direction (both perturbed solves must end PROBLEM_SOLVED on the unperturbed working set: held).
# MEASURED (`python tests/tangent_cases.py`; gap = (A) vs (B), (C) = central differences vs (A), both relative to max(1, largest |dx| of the row)):
#     small_sb  flags 1111      gap 1.4e-15  |dx| 6.0e+00  (C) 8.0e-11 held True
#     general   flags 1111      gap 1.1e-14  |dx| 7.7e+01  (C) 3.6e-10 held True
#     empty_ws  flags 1111      gap 1.9e-15  |dx| 2.4e+00  (C) 1.7e-10 held True
#     ik        flags 11111111  gap 2.0e-14  |dx| 1.4e+01  (C) 5.5e-10 held True
#     rank_def  flags 0000      gap 0.0e+00  |dx| 0.0e+00
#     mixed     flags 1010      gap 1.3e-14  |dx| 1.2e+02  (C) 1.0e-09 held True
#     budget    flags 101010    gap 4.6e-16  |dx| 3.6e+00  (C) 2.3e-10 held True
#     tile      flags 11        gap 1.3e-15  |dx| 7.2e+00
# LSI_D_CPU = 2.0e-14 (ik) -> LSI_TOL = 10 LSI_D_CPU = 2.0e-13.  Largest (C) gap 1.04e-9 (mixed) -> LSI_FD_BOUND = ten times it, the convention of
# lsi_adjoint_matrix_cases (never above 1e-6): 1.04e-8, seven orders below a wrong sign or a missing term.
LSI_NTAN = 3
LSI_D_CPU = 2.0e-14  # measured (1.996e-14, rounded up)
LSI_TOL = 10.0 * LSI_D_CPU
LSI_GAP_C = 1.04e-9  # measured (1.032e-9, rounded up)
LSI_FD_BOUND = min(10.0 * LSI_GAP_C, 1e-6)


def _lm():
    import lsi_adjoint_matrix_cases as LM
    return LM


def lsi_gather(n, objs, fixed, rows, dD, cap):
    """the direction of the final problem from the direction dD over an instance's data: (dlod (n + 1, cap), dfixed (n,)) — lsi_tangent_gather_kernel"""
    LM = _lm()
    lay, _ = LM.layout(n, objs)
    first = np.concatenate([[0], np.cumsum([len(o["lb"]) for o in objs])]).astype(int)
    k_of = lambda u: int(np.searchsorted(first, u, side="right") - 1)  # noqa: E731
    dlod, dfixed = np.zeros((n + 1, cap)), np.zeros(n)
    for j, (_, _, u, t) in enumerate(fixed):
        off, dm, w = lay[k_of(u)]
        dfixed[j] = dD[off + (w - 2 if t == LM.LB else w - 1) * dm + (u - first[k_of(u)])]
    for r, (u, t) in enumerate(rows):
        off, dm, w = lay[k_of(u)]
        c = u - first[k_of(u)]
        dlod[:n, r] = dD[off + np.arange(n) * dm + c]
        dlod[n, r] = dD[off + (w - 2 if t == LM.LB else w - 1) * dm + c]
    return dlod, dfixed


def lsi_reference_instance(n, objs, active, status, dDs, with_b=True):
    """(dx (A) (K, n), dx (B) (K, n), flag) for ONE instance and K directions dDs (K, per_data)"""
    LM = _lm()
    K = len(dDs)
    XA, XB = np.zeros((K, n)), np.zeros((K, n))
    if status != LM.SOLVED:
        return XA, XB, 0
    lod, dims, caps, fixed, rows = LM.LC.final_problem(n, objs, active)
    nf = len(fixed)
    if nf + len(rows) == 0:
        return XA, XB, 1
    idx, val = np.zeros((1, n), np.uint32), np.zeros((1, n))
    for j, (var, value, _, _) in enumerate(fixed):
        idx[0, j], val[0, j] = var, value
    case = dict(n=n, caps=caps, lod=lod[None], dims=dims[None], g=np.zeros((1, n)),
                fixed=dict(nfixed=np.asarray([nf], np.uint32), fixed_idx=idx, fixed_val=val) if nf else {})
    ref = AM.run_oracle(case)
    if not AM.rank_stable(n, dims, ref["rank"][0], ref["fcol"][0], nf):
        return XA, XB, 0
    for c in range(K):
        dlod, dfixed = lsi_gather(n, objs, fixed, rows, dDs[c], lod.shape[1])
        XA[c] = tangent_kkt(n, lod, dims, ref["rank"][0], ref["perm"][0], ref["totalrank"][0], nf, idx[0, :nf].astype(int), val[0, :nf], dlod, dfixed)
        if with_b:
            XB[c] = tangent_from_factor(case, ref, 0, dlod, dfixed)[0]
    return XA, XB, 1


def lsi_central_difference(n, objs, run, dD, params):
    """((x(D + h dD) - x(D - h dD)) / 2h, held) through the whole oracle LexLSI driver"""
    LM = _lm()
    dims, types, D, var = LM.lexlsi.flatten(n, objs)
    xs, held = [], True
    for sgn in (+1.0, -1.0):
        r = LM.oracle.lsi_run(n, LM.lexlsi.unflatten(n, dims, types, D + sgn * FD_H * dD, var), **params)
        held = held and r["info"]["status"] == LM.SOLVED and all(np.array_equal(a, a0) for a, a0 in zip(r["active"], run["active"]))
        xs.append(r["x"])
    return (xs[0] - xs[1]) / (2.0 * FD_H), held


@functools.lru_cache(maxsize=None)
def lsi_build(name, K=LSI_NTAN, with_b=True):
    """the LexLSI case `name` of lsi_adjoint_matrix_cases with K directions per instance: case (shared, read-only), ddata (K, batch, per_data;
    direction 0 is that module's dD where it has one), A / B (K, batch, n), flags, gap = its share of LSI_D_CPU"""
    LM = _lm()
    case = LM.build(name)
    n, probs = case["n"], case["probs"]
    B, per_data = len(probs), case["A"].shape[1]
    seed = LM.spec_of(name)[1]
    ddata = np.zeros((K, B, per_data))
    for b in range(B):
        for c in range(K):
            ddata[c, b] = LM.direction(seed + 9000 + 100 * c + b, n, probs[b], 1.0)
        if "dD" in case and case["flags"][b]:
            ddata[0, b] = case["dD"][b]
    XA, XB, flags, gap = np.zeros((K, B, n)), np.zeros((K, B, n)), np.zeros(B, np.uint8), 0.0
    for b in range(B):
        a, bb, flags[b] = lsi_reference_instance(n, probs[b], case["runs"][b]["active"], case["status"][b], ddata[:, b], with_b)
        XA[:, b], XB[:, b] = a, bb
        if with_b:
            gap = max([gap] + [AC._rel(a[c] - bb[c], a[c]) for c in range(K)])
    for a in (ddata, XA, XB, flags):
        a.setflags(write=False)
    return dict(case=case, ddata=ddata, A=XA, B=XB if with_b else None, flags=flags, gap=gap if with_b else None)


def lsi_fd_gap(name):
    """the largest gap between (C) and (A) over the flag-1 instances and the directions of a case, and whether every working set held"""
    LM = _lm()
    t = lsi_build(name)
    case = t["case"]
    worst, held = 0.0, True
    for b in np.flatnonzero(t["flags"]):
        for c in range(LSI_NTAN):
            fd, ok = lsi_central_difference(case["n"], case["probs"][b], case["runs"][b], t["ddata"][c, b], case["params"])
            held = held and ok
            worst = max(worst, AC._rel(fd - t["A"][c, b], t["A"][c, b]))
    return worst, held


def inactive_entries(case, b):
    """a mask (per_data,) over instance b's data: the entries of the user rows outside its final working set"""
    LM = _lm()
    n, objs = case["n"], case["probs"][b]
    lay, per_data = LM.layout(n, objs)
    out, first = np.zeros(per_data, bool), 0
    for (off, dm, w) in lay:
        idle = np.flatnonzero(np.asarray(case["active"][b][first:first + dm]) == 0)
        for j in range(w):
            out[off + j * dm + idle] = True
        first += dm
    return out


def summary(t):
    case = t["case"]
    return (f"    {case['name']:<15} n={case['n']:<4} {str(case['caps']).replace(' ', ''):<18} batch {case['lod'].shape[0]}  flags "
            f"{''.join(str(int(f)) for f in case['flags']):<9} gap {t['gap']:.1e}  dual {t['dual']:.1e}  |dx| {np.abs(t['A']).max():.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in CASES + FIT_NAMES:
        t = build(nm)
        worst = max(worst, t["gap"])
        print(summary(t))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = 10 D_CPU = {10 * worst:.2e}")
    for nm in ("base", "fixed", "ik"):
        print(f"    central differences, h = {FD_H:g}: {nm:<8} gap {fd_gap(nm):.1e}")
    LM = _lm()
    worst = worst_c = 0.0
    for nm in LM.CASES:
        t = lsi_build(nm)
        line = f"    LexLSI {nm:<9} flags {''.join(str(int(f)) for f in t['flags']):<9} gap {t['gap']:.1e}  |dx| {np.abs(t['A']).max():.1e}"
        worst = max(worst, t["gap"])
        if nm in LM.WITH_B:
            gc, held = lsi_fd_gap(nm)
            worst_c = max(worst_c, gc)
            line += f"  (C) {gc:.1e} held {held}"
        print(line)
    print(f"    LSI_D_CPU (largest gap) {worst:.2e}  ->  LSI_TOL = {10 * worst:.2e};  largest (C) gap {worst_c:.2e}  ->  LSI_FD_BOUND = {min(10 * worst_c, 1e-6):.2e}")
