"""Batches that hold the POST-FACTORIZATION kernels (lexls_amd/csrc/lse_postfactor.hip: solve_generic, residual, sensitivity<64,staged|hbm>, the
two sweeps, leastnorm 1 / 2 / 3) to the oracle beyond the small shapes (tests/test_gpu_postfactor.py runs them on the GPU, bit for bit;
tests/test_postfactor_cases.py asserts the conditions below on the CPU, from the oracle alone).

A shape alone is close to vacuous here: with fewer rows than variables above the last level every multiplier of every earlier objective is
exactly zero, and with enough rows the total rank is n and the three least-norm routines have nothing to do.  So every case is built to be
over-determined AND column-rank deficient: `dup` columns of a problem repeat other columns (exact ties in the pivot search, total rank at most
n - dup however many rows there are), all problems but every fourth (b % 4 == 3, which keeps full column rank); one row of a later level
repeats a row of an earlier one (right-hand side included); activation types are LB / UB / EQ mixed, and in every third problem every level
but the last is all equalities, so that a scan from level 0 has to go on to the end.  In tiny, where the first level could otherwise always be
met, every fourth problem's level 0 contradicts itself (same row, another right-hand side).  Data: P.lse_batch, seeds below (tiny's seed is
the first of a series at which solveLeastNorm_1 moves every one of its 769 free problems by more than 1e-3: condition (a)).

Cases (what each is for):
    n63 / n64 / n65   [16,16,16,16,8]: the nVar + 1 <= 64 switch of launch_solve_generic (n63 <64>, the others the blocked <256>) and the nVar <= 64
                      limit of both sweeps (n63, n64 swept; n65 not)
    row17, obj9       n = 40 with a 17-row level, n = 30 with 9 objectives: the sweeps refuse each by one unit
    blocks            n = 150 [64,65,1,30,45], three duplicated columns: level ranks 64, 65, 1, 17, 0.  The blocked back-substitution meets ranks on
                      both sides of its 64-row blocks (one full block; a full block under a partial one of ONE row; 64 + 65 > 128), and the columns
                      of the levels below are acc = 17, 18 and 83: the loops j + 64 <= acc, j + 16 <= acc and the scalar tail all run (the 16-wide
                      loop needs acc mod 64 >= 16, hence a fourth ranked level and n = 150 instead of 130).  Three trips of the least-norm
                      kernels' strided loops, 205 rows of capacity for residual_kernel
    large             n = 100 [115,115], one problem (rank_cases' large shape): lqr_large<multi-launch> under policy 5, the HBM-resident generic kernel
                      under policy 1; 231 x 101 x 8 B staged > 160 KB: sensitivity<64,hbm>
    staged            n = 88 [30,30,25,15]: 64 KB < 101 x 89 x 8 B <= 160 KB at batch 4: sensitivity<64,staged> behind set_lds
    tiny              n = 3 [2,2] at batch 4 CUs + 1 (the CPU test: 1025): sensitivity<64,hbm> chosen by batch size; the first 8 problems again at
                      batch 8 (the sweep)
    ragged            n = 40, capacity [12]x5, per-problem dimensions with empty levels, fixed variables with activation types: nfixed = dims[0] + 1
                      (problems 2 and 5), every variable fixed (problem 4: nVarRank = nVarFree = 0)
    ik, wide          n = 40 [12]x5 and n = 55 [14,9,16,5], batch 5: the producer matrix (every l-QR kernel's factor under every consumer)
    ln_panel, ln_switch   the least-norm group (LEAST_NORM_CASES, build_least_norm): n = 20 and n = 70, a handful of problems each whose nVarFree —
                      the order of the SPD system solveLeastNorm_2 and _3 solve (lexls_amd/csrc/lse_spd_solve.h) — is 1, 15, 16, 17 / 48, 64, 65:
                      the smallest order, both sides of a 16-column panel edge, a boundary behind three full panels, both sides of the switch
                      from the one-wavefront panel form to the column-by-column form; fixed variables in the last problem of each.  The cases
                      above leave nVarFree at about `dup` (at most 20)

Conditions (tests/test_postfactor_cases.py): (a) at least half of a case's problems have ranks of the levels + nfixed < n and solveLeastNorm_1 moves
some entry of theirs by more than 1e-3 (ragged: exempt, it is there for the other end; the least-norm group: EVERY problem has free variables and
solveLeastNorm_2 and _3 each move some entry by more than 1e-3, it is exempt from (b) — equalities only, no multipliers asked for — and of (c) the agreement of its two solutions is held); (b) at least two objectives have non-zero multipliers, found is 1 for some (problem, level) pairs and 0 for others, CORRECT_SIGN marks occur, a scan from level 0 stops at more than one
level (large, one problem: it stops somewhere); (c) the oracle against mathematics: stationarity of the multipliers and
lambda_k = residual of level k to 1e-12, get_v = A x - b and the agreement of the three least-norm solutions to 1e-10, x orthogonal to the null
space of the stacked matrix (no fixed variables) to 1e-10, each times max(1, largest magnitude of the quantity).

MEASURED (oracle alone, `python tests/postfactor_cases.py`; free = problems whose levels' ranks + nfixed < n; lam!=0 = objectives with a non-zero
multiplier block; found = (problem, level) pairs with / without a candidate; stops = levels a scan from 0 stops at; marks = CORRECT_SIGN marks
of the scan; the oracle's own figures for (c), relative as above: stat = stationarity, lam-v = lambda_k against the residual, v = get_v against
A x - b, ln = largest disagreement of the three least-norm solutions, orth = x against the null space; |ln1-x| = smallest over the free
problems of the largest entry solveLeastNorm_1 moves; the least-norm group: nVarFree per problem, and the same figure for _2 and _3):
    n63     n=63  [16,16,16,16,8]  batch 5    free 4    lam!=0 [3,4]         found 8/17 stops [3,4]     marks 69   stat 6.2e-15 lam-v 9.1e-15 v 1.6e-15 ln 1.2e-15 orth 4.0e-15 |ln1-x| 1.0e-01
    n64     n=64  [16,16,16,16,8]  batch 5    free 4    lam!=0 [3,4]         found 8/17 stops [3,4]     marks 57   stat 6.3e-15 lam-v 1.5e-14 v 1.9e-15 ln 7.0e-16 orth 8.4e-15 |ln1-x| 2.0e-01
    n65     n=65  [16,16,16,16,8]  batch 5    free 4    lam!=0 [3,4]         found 8/17 stops [3,4]     marks 75   stat 7.7e-15 lam-v 1.3e-14 v 1.8e-15 ln 9.3e-16 orth 9.9e-15 |ln1-x| 1.4e-01
    row17   n=40  [17,16,13]       batch 6    free 5    lam!=0 [1,2]         found 7/11 stops [1,2]     marks 64   stat 2.9e-15 lam-v 9.4e-15 v 1.2e-15 ln 8.2e-16 orth 2.0e-14 |ln1-x| 2.2e-01
    obj9    n=30  [4,4,4,4,4,4,4,4,4] batch 6    free 5    lam!=0 [6,7,8]       found 13/41 stops [6,8]     marks 40   stat 6.3e-15 lam-v 7.7e-15 v 1.4e-15 ln 8.8e-16 orth 3.7e-15 |ln1-x| 6.4e-02
    blocks  n=150 [64,65,1,30,45]  batch 3    free 3    lam!=0 [3,4]         found 5/10 stops [3,4]     marks 113  stat 1.4e-14 lam-v 1.6e-14 v 1.8e-15 ln 1.3e-15 orth 2.0e-15 |ln1-x| 8.2e-02
    large   n=100 [115,115]        batch 1    free 1    lam!=0 [0,1]         found 1/1 stops [1]       marks 32   stat 1.1e-14 lam-v 2.6e-15 v 6.8e-16 ln 3.3e-16 orth 1.2e-16 |ln1-x| 1.8e-02
    staged  n=88  [30,30,25,15]    batch 4    free 3    lam!=0 [2,3]         found 5/11 stops [2,3]     marks 60   stat 7.8e-15 lam-v 6.8e-14 v 1.3e-15 ln 9.3e-16 orth 1.8e-14 |ln1-x| 8.2e-01
    tiny    n=3   [2,2]            batch 1025 free 769  lam!=0 [0,1]         found 545/1505 stops [0,1]     marks 615  stat 1.3e-15 lam-v 4.1e-14 v 5.4e-15 ln 4.4e-16 orth 2.5e-14 |ln1-x| 3.7e-03
    ragged  n=40  [12,12,12,12,12] batch 6    free 4    lam!=0 [0,1,2,3,4]   found 14/16 stops [0,2,3,4] marks 42   stat 3.1e-15 lam-v 3.1e-14 v 1.0e-15 ln 9.4e-16 orth 5.8e-16 |ln1-x| 2.4e-01
    ik      n=40  [12,12,12,12,12] batch 5    free 4    lam!=0 [3,4]         found 8/17 stops [3,4]     marks 50   stat 3.7e-15 lam-v 1.1e-14 v 7.9e-16 ln 6.6e-16 orth 4.0e-15 |ln1-x| 7.5e-02
    wide    n=55  [14,9,16,5]      batch 5    free 5    lam!=0 [2,3]         found 6/14 stops [2,3]     marks 35   stat 4.5e-15 lam-v 7.8e-15 v 6.1e-15 ln 1.4e-15 orth 9.0e-15 |ln1-x| 5.7e-01
    ln_panel  n=20  nVarFree [1, 15, 16, 17, 16] |ln2-x| 8.3e-02 |ln3-x| 8.3e-02
    ln_switch n=70  nVarFree [48, 64, 65, 65] |ln2-x| 2.3e-01 |ln3-x| 2.3e-01
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

LB, UB, EQ, CORRECT = 1, 2, 3, 4
TOLW, TOLC = 1e-8, 1e-12
BOUND_DUAL, BOUND_X = 1e-12, 1e-10  # condition (c): the bounds of tests/test_oracle_golden.py, times max(1, largest magnitude of the quantity)

IK_PER_PROBLEM = np.array([[12, 12, 12, 12, 12], [12, 0, 12, 12, 12], [5, 12, 7, 12, 9], [12, 12, 12, 0, 12], [9, 12, 12, 12, 3], [12, 11, 12, 12, 12]], np.uint32)

# name -> n, dims (capacities), batch, seed, dup (duplicated columns per problem); policy: the kernel policy of the GPU test (None: automatic);
# per_problem: dims rows dealt round the batch; nfixed: fixed variables per problem; clash: every clash-th problem's level 0 contradicts itself
CASES = {
    "n63": dict(n=63, dims=[16, 16, 16, 16, 8], batch=5, seed=20270101, dup=3),
    "n64": dict(n=64, dims=[16, 16, 16, 16, 8], batch=5, seed=20270102, dup=3),
    "n65": dict(n=65, dims=[16, 16, 16, 16, 8], batch=5, seed=20270103, dup=3),
    "row17": dict(n=40, dims=[17, 16, 13], batch=6, seed=20270104, dup=8),
    "obj9": dict(n=30, dims=[4] * 9, batch=6, seed=20270105, dup=3),
    "blocks": dict(n=150, dims=[64, 65, 1, 30, 45], batch=3, seed=20270106, dup=3, policy=5),
    "large": dict(n=100, dims=[115, 115], batch=1, seed=20270107, dup=2, policy=5),
    "staged": dict(n=88, dims=[30, 30, 25, 15], batch=4, seed=20270108, dup=4),
    "tiny": dict(n=3, dims=[2, 2], batch=1025, seed=20420214, dup=1, clash=4),
    "ragged": dict(n=40, dims=[12] * 5, batch=6, seed=20270110, dup=2, per_problem=IK_PER_PROBLEM, nfixed=[0, 3, 6, 2, 40, 13]),
    "ik": dict(n=40, dims=[12] * 5, batch=5, seed=20270111, dup=1),
    "wide": dict(n=55, dims=[14, 9, 16, 5], batch=5, seed=20270112, dup=20),  # (44 rows against 55 variables: over-determined from 20 duplicated columns on)
}


def draw(name, batch=None):
    """the inputs of a case: dict(n, caps, lod, dims (batch, nObj), types, fixed (keyword arguments of oracle.lse_run, {} without fixed
    variables)).  Problem b is a function of (seed, b) alone: a smaller batch is a prefix of a larger one"""
    c = CASES[name]
    n, caps, seed = c["n"], list(c["dims"]), c["seed"]
    B, cap, nobj = int(batch or c["batch"]), sum(caps), len(caps)
    lod = P.lse_batch(seed, B, n, caps)
    dims = np.tile(np.asarray(caps, np.uint32), (B, 1))
    if c.get("per_problem") is not None:
        dims = c["per_problem"][np.arange(B) % len(c["per_problem"])].copy()
    types = np.zeros((B, cap), np.uint8)
    for b in range(B):
        m, first = int(dims[b].sum()), np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        lod[b, :, m:] = np.nan  # a problem's rows packed level after level; NaN behind them (never read)
        u = P.uniform(seed + 100000 + b, 2 * c["dup"] + 4)
        if b % 4 != 3:  # duplicated columns: column rank at most n - dup
            for d in range(c["dup"]):
                j = int(u[2 * d] * n)
                i = (j + 1 + int(u[2 * d + 1] * (n - 1))) % n
                lod[b, i, :] = lod[b, j, :]
        levels = [k for k in range(nobj) if dims[b, k] > 0]
        ka, kb = levels[0], levels[-1]  # one row of the last non-empty level repeats one of the first
        ra = first[ka] + int(u[-4] * dims[b, ka])
        rb = first[kb] + int(u[-3] * dims[b, kb])
        lod[b, :, rb] = lod[b, :, ra]
        types[b] = 1 + (P.uniform(seed + 200000 + b, cap) * 3).astype(np.uint8)  # LB / UB / EQ
        if b % 3 == 0:  # equalities on every level but the last: nothing to find there, a scan goes on to the end
            types[b, :first[nobj - 1]] = EQ
        if c.get("clash") and b % c["clash"] == 1:  # row 1 of level 0 repeats the matrix part of row 0 under another right-hand side: level 0 cannot be met
            lod[b, :n, 1] = lod[b, :n, 0]
    fixed = {}
    if c.get("nfixed") is not None:
        nfixed = np.asarray(c["nfixed"], np.uint32)[np.arange(B) % len(c["nfixed"])]
        idx, val, typ = np.zeros((B, n), np.uint32), np.zeros((B, n)), np.zeros((B, n), np.uint8)
        for b in range(B):
            nf = int(nfixed[b])
            idx[b, :nf] = np.argsort(P.uniform(seed + 300000 + b, n))[:nf]
            val[b, :nf] = P.normal(seed + 400000 + b, n)[:nf]
            typ[b, :nf] = 1 + (P.uniform(seed + 500000 + b, n)[:nf] * 3).astype(np.uint8)
        fixed = dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val, fixed_type=typ)
    return dict(name=name, n=n, caps=caps, lod=lod, dims=dims, types=types, fixed=fixed, policy=c.get("policy"))


# The least-norm group: the orders nVarFree of the SPD system D z = d that solveLeastNorm_2 and _3 solve (lse_spd_solve.h: the panel form takes
# 16 columns at a time up to order 64, the column-by-column form any order).  Dense data of full row rank and fewer rows than free columns, so
# nVarFree = n - nfixed - (the problem's rows), set per problem by its level dimensions: both sides of a panel edge, a boundary behind three
# full panels, both sides of the switch; fixed variables in the last problem of each.  name -> n, dims (capacities), seed, per_problem, nfixed
LEAST_NORM_CASES = {
    "ln_panel": dict(n=20, dims=[10, 9], seed=20270113, per_problem=[[10, 9], [3, 2], [2, 2], [2, 1], [1, 1]], nfixed=[0, 0, 0, 0, 2]),  # 1, 15, 16, 17, 16
    "ln_switch": dict(n=70, dims=[12, 10], seed=20270114, per_problem=[[12, 10], [3, 3], [3, 2], [2, 2]], nfixed=[0, 0, 0, 1]),          # 48, 64, 65, 65
}
LEAST_NORM_ORDERS = (1, 15, 16, 17, 48, 64, 65)  # smallest; a panel edge; three full panels; the switch to the workgroup form


@functools.lru_cache(maxsize=None)
def build_least_norm(name):
    """a case of the least-norm group: the inputs as draw() names them, the oracle's x, ranks, solveLeastNorm_2 (ln2) and solveLeastNorm_3 behind
    regularization type 1 with zero factors (ln3), and nvarfree per problem from the oracle's ranks"""
    c = LEAST_NORM_CASES[name]
    n, caps, seed = c["n"], list(c["dims"]), c["seed"]
    dims, nfixed = np.asarray(c["per_problem"], np.uint32), np.asarray(c["nfixed"], np.uint32)
    B = len(dims)
    lod = P.lse_batch(seed, B, n, caps)
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b in range(B):
        lod[b, :, int(dims[b].sum()):] = np.nan  # a problem's rows packed level after level; NaN behind them (never read)
        nf = int(nfixed[b])
        idx[b, :nf] = np.argsort(P.uniform(seed + 300000 + b, n))[:nf]
        val[b, :nf] = P.normal(seed + 400000 + b, n)[:nf]
    fixed = dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val, fixed_type=np.full((B, n), EQ, np.uint8))
    case = dict(name=name, n=n, caps=caps, lod=lod, dims=dims, types=np.full((B, sum(caps)), EQ, np.uint8), fixed=fixed, policy=None)
    run = functools.partial(oracle.lse_run, lod, dims, n, maxdim=np.asarray(caps, np.uint32), **fixed)
    basic = run()
    case["x"], case["rank"] = basic["x"], basic["rank"]
    case["ln2"] = run(solve_option=2)["x"]
    case["ln3"] = run(solve_option=3, reg_type=1, reg_factors=[0.0] * len(caps))["x"]
    case["nvarfree"] = n - nfixed.astype(int) - case["rank"].sum(axis=1).astype(int)
    for a in [v for v in case.values() if isinstance(v, np.ndarray)] + list(fixed.values()):
        a.setflags(write=False)
    return case


def _one(fixed, b):
    return {k: v[b:b + 1] for k, v in fixed.items()}


def _mark_fixed(typ, lam_fixed):
    """the marks the deciding overload leaves on the fixed variables' types (lexlse.h:935-987 called with LambdaFixed, nVarFixed): comparisons only"""
    out = typ.copy()
    for k in range(len(lam_fixed)):
        if out[k] in (EQ, CORRECT):
            continue
        a = -lam_fixed[k] if out[k] == LB else lam_fixed[k]
        if a > TOLC:
            out[k] = CORRECT
    return out


def reference_scan(n, caps, lod, dims, types, fixed, start):
    """setSensitivityScan(True) + ObjectiveSensitivity(start) as LexLSI's level loop does it (lexlsi.h:1121-1132), problem by problem on the oracle: stop at
    the first level that reports a candidate, marks of both type arrays carried along.  (sens, maxabs, lam, marks, stopped)"""
    B, nobj = lod.shape[0], len(caps)
    sens, maxabs, lam = np.zeros((B, 3), np.int32), np.zeros(B), np.zeros((B, n + sum(caps)))
    marks, stopped = types.copy(), np.zeros(B, int)
    for b in range(B):
        cur, kw = types[b:b + 1].copy(), _one(fixed, b)
        for level in range(start, nobj):
            ref = oracle.lse_run(lod[b:b + 1], dims[b:b + 1], n, maxdim=caps, ctr_type=cur, sens_obj=level, **kw)
            cur = ref["ctr_type_out"]
            if kw:
                nf = int(kw["nfixed"][0])
                kw["fixed_type"] = kw["fixed_type"].copy()
                kw["fixed_type"][0, :nf] = _mark_fixed(kw["fixed_type"][0, :nf], ref["lam"][0, :nf])
            if ref["sens"][0, 0] or level == nobj - 1:
                sens[b], maxabs[b], lam[b], marks[b], stopped[b] = ref["sens"][0], ref["maxabs"][0], ref["lam"][0], cur[0], level
                break
    return sens, maxabs, lam, marks, stopped


def reference_collect(n, caps, lod, dims, types, fixed, start, scan):
    """The collecting overload ObjectiveSensitivity(ObjIndex, tolW, tolC, ctr_wrong_sign) (lexlse.h:511-602 around the scan of :866-910) on the
    oracle's multipliers, problem by problem and statement for statement as in lexlse.h:891-908 and :575-601: the objective's own level, the levels
    above it downwards, then the fixed variables with the reference's quirk (min(dims[0], nVarFixed) entries, the CONSTRAINT multipliers Lambda[k]
    against fixed_var_type[k], pushed as ConstraintInfo(-1, k)).  With `scan` the loop of lexlsi.h:1072-1083 goes on to the next objective while the
    set is empty, marks carried along.  (mask (batch, n + cap): fixed variables then rows, constraint types, fixed types, lam, verdict)"""
    B, cap, nobj = lod.shape[0], sum(caps), len(caps)
    dims = np.broadcast_to(np.asarray(dims, np.uint32), (B, nobj))
    mask = np.zeros((B, n + cap), np.uint8)
    ctr = types.copy()
    fix = fixed["fixed_type"].copy() if fixed else np.zeros((B, n), np.uint8)
    lam, verdict = np.zeros((B, n + cap)), np.zeros((B, 3), np.int32)
    for b in range(B):
        nf = int(fixed["nfixed"][b]) if fixed else 0
        first = np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        for L in range(start, nobj):
            ref = oracle.lse_run(lod[b:b + 1], dims[b:b + 1], n, maxdim=caps, ctr_type=types[b:b + 1], sens_obj=L, **_one(fixed, b))
            lam[b] = ref["lam"][0]
            Lambda = lam[b, nf:]  # getWorkspace() = [lambda_fixed; lambda]

            def scan_group(tarr, toff, moff, count):
                for k in range(count):
                    t = tarr[b, toff + k]
                    if t == EQ or t == CORRECT:
                        continue
                    a = Lambda[toff + k]
                    if t == LB:
                        a = -a
                    if a > TOLC:
                        tarr[b, toff + k] = CORRECT
                    elif a < -TOLW:
                        mask[b, moff + k] = 1

            for k in range(L, -1, -1):
                scan_group(ctr, int(first[k]), n + int(first[k]), int(dims[b, k]))
            if nf > 0:
                scan_group(fix, 0, 0, min(int(dims[b, 0]), nf))
            verdict[b] = (int(mask[b].any()), int(mask[b].sum()), L)
            if mask[b].any() or not scan:
                break
    return mask, ctr, fix, lam, verdict


def _rel(err, *quantities):
    return float(err) / max([1.0] + [float(np.abs(q).max()) for q in quantities if np.size(q)])


def _authority(case):
    """the oracle against mathematics, condition (c): the largest relative figures over the case"""
    n, lod, dims, fixed = case["n"], case["lod"], case["dims"], case["fixed"]
    out = dict(stat=0.0, lam_v=0.0, v=0.0, ln=0.0, orth=0.0)
    for b in range(lod.shape[0]):
        m, nf = int(dims[b].sum()), int(fixed["nfixed"][b]) if fixed else 0
        A, rhs = lod[b, :n, :m].T, lod[b, n, :m]
        first = np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        E = np.zeros((nf, n))
        if nf:
            E[np.arange(nf), fixed["fixed_idx"][b, :nf]] = 1.0
        res = A @ case["x"][b] - rhs
        out["v"] = max(out["v"], _rel(np.abs(case["v"][b, :m] - res).max() if m else 0.0, res))
        for k in range(dims.shape[1]):
            lam = case["lam"][k][b]
            g = E.T @ lam[:nf] + A[:first[k + 1]].T @ lam[nf:nf + first[k + 1]]
            out["stat"] = max(out["stat"], _rel(np.abs(g).max(), lam))
            own = lam[nf + first[k]:nf + first[k + 1]]
            out["lam_v"] = max(out["lam_v"], _rel(np.abs(own - res[first[k]:first[k + 1]]).max() if own.size else 0.0, own))
            assert not lam[nf + first[k + 1]:].any()
        x1, x2, x3 = case["ln1"][b], case["ln2"][b], case["ln3"][b]
        out["ln"] = max(out["ln"], _rel(max(np.abs(x1 - x2).max(), np.abs(x1 - x3).max()), x1))
        if not nf and m:
            _, s, Vt = np.linalg.svd(A)
            r = int((s > 1e-9 * s[0]).sum())
            out["orth"] = max(out["orth"], _rel(np.abs(Vt[r:] @ x1).max() if r < n else 0.0, x1))
    return out


@functools.lru_cache(maxsize=None)
def build(name, batch=None):
    """the case `name` (at `batch` problems instead of its own number): its inputs (draw) and the oracle's results for everything the GPU test
    compares — basic (x, v, factor, hh, perm, rank, fcol, totalrank), sens[k] / maxabs[k] / lam[k] / marks[k] of ObjectiveSensitivity(k), scan (from
    level 0), collect (level collect_level, no scan), mult = the nObj lam vectors, ln1 / ln2 / ln3 — and the figures of the conditions"""
    case = draw(name, batch)
    n, caps, lod, dims, types, fixed = case["n"], case["caps"], case["lod"], case["dims"], case["types"], case["fixed"]
    nobj, B = len(caps), lod.shape[0]
    run = functools.partial(oracle.lse_run, lod, dims, n, maxdim=np.asarray(caps, np.uint32), nthreads=8, **fixed)
    basic = run(ctr_type=types)
    case.update({k: basic[k] for k in ("x", "v", "factor", "hh", "perm", "rank", "fcol", "totalrank")})
    case["basic"] = basic
    case["sens"], case["maxabs"], case["lam"], case["marks"] = [], [], [], []
    used = np.arange(sum(caps))[None, :] < dims.sum(axis=1)[:, None]  # behind a problem's own rows the oracle's type array is whatever it held before:
    for k in range(nobj):                                              # those entries keep the types they were given, as they do on the device
        r = run(ctr_type=types, sens_obj=k)
        case["sens"].append(r["sens"]), case["maxabs"].append(r["maxabs"]), case["lam"].append(r["lam"])
        case["marks"].append(np.where(used, r["ctr_type_out"], types))
    case["mult"] = np.stack(case["lam"], axis=1)
    scan = reference_scan(n, caps, lod, dims, types, fixed, 0)
    case["scan"] = scan[:3] + (np.where(used, scan[3], types), scan[4])
    case["collect_level"] = nobj - 1
    case["collect"] = reference_collect(n, caps, lod, dims, types, fixed, nobj - 1, False)
    case["ln1"], case["ln2"] = run(solve_option=1)["x"], run(solve_option=2)["x"]
    case["ln3"] = run(solve_option=3, reg_type=1, reg_factors=[0.0] * nobj)["x"]
    nfixed = fixed["nfixed"] if fixed else np.zeros(B, np.uint32)
    case["free"] = case["rank"].sum(axis=1) + nfixed < n  # nVarFree > 0 (the levels' ranks: getTotalRank() counts the fixed variables in)
    case["ln1_moves"] = np.abs(case["ln1"] - case["x"]).max(axis=1)
    case["nonzero_objectives"] = [k for k in range(nobj) if case["lam"][k].any()]
    case["found"] = np.stack([s[:, 0] for s in case["sens"]], axis=1)
    case["authority"] = _authority(case)
    for a in [v for v in case.values() if isinstance(v, np.ndarray)] + [x for key in ("sens", "maxabs", "lam", "marks", "scan", "collect") for x in case[key]]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def summary(case):
    a, f = case["authority"], case["found"]
    stops = sorted(set(case["scan"][4].tolist()))
    moves = case["ln1_moves"][case["free"]]
    return (f"    {case['name']:<7} n={case['n']:<3} {str(case['caps']).replace(' ', ''):<16} batch {case['lod'].shape[0]:<4} free {int(case['free'].sum()):<4} "
            f"lam!=0 {str(case['nonzero_objectives']).replace(' ', ''):<13} found {int(f.sum())}/{int((f == 0).sum())} stops {str(stops).replace(' ', ''):<9} "
            f"marks {int((case['scan'][3] == CORRECT).sum()):<4} stat {a['stat']:.1e} lam-v {a['lam_v']:.1e} v {a['v']:.1e} ln {a['ln']:.1e} orth {a['orth']:.1e} "
            f"|ln1-x| {moves.min() if moves.size else 0.0:.1e}")


def summary_least_norm(ln):
    moves = [np.abs(ln[k] - ln["x"]).max(axis=1).min() for k in ("ln2", "ln3")]
    return f"    {ln['name']:<9} n={ln['n']:<3} nVarFree {ln['nvarfree'].tolist()} |ln2-x| {moves[0]:.1e} |ln3-x| {moves[1]:.1e}"


if __name__ == "__main__":
    for nm in CASES:
        print(summary(build(nm)))
    for nm in LEAST_NORM_CASES:
        print(summary_least_norm(build_least_norm(nm)))
