"""Cases that hold the MANY-COTANGENT adjoint of the regularized LexLSE solve (lexls_lse_solve_adjoint_multi* once
lexls_lse_set_adjoint_regularized_multi is on; lexls_amd/csrc/lse_adjoint.hip: solve_adjoint_reg_multi_kernel, lane = cotangent) to the two
references of tests/adjoint_reg_cases.py, on its data, factors and oracle runs (draw, factors, _run_one, adjoint_reg_from_factor).

    reference (A)  M_reg (nVar x rows) and N_reg (nVar x nfixed) of every problem by unit solves on the oracle with the regularization passed
                   through; then G M_reg and G N_reg in numpy for every cotangent set.
    reference (B)  adjoint_reg_from_factor, one cotangent at a time.
Cotangent sets (sets_of): the identity (ncot = nVar: the Jacobian), 3 random cotangents, 65 random cotangents (two tiles) on the small cases and on
`edge` (the hbm form keeps one set of matrices per tile).

Cases: RC.NAMES, crossed with RC.types_of, and three more on both sides of the placement rule (lexls_lds.h: adjoint_reg_multi_form; restated here
as lds_bytes / variant, and tests/test_adjoint_reg_multi_cases.py holds the restatement to the header on a grid).  The per-lane state takes 8 * 65
* (3 nVar + cap) bytes, the problem's matrices adjoint_reg_matrix_doubles:
    edge_lds  n = 52 (24, 24), batch 3: the last nVar at nObj = 2, cap = 48 whose state and matrices fit 160 KiB (160576 bytes)     -> lds
    edge      n = 53 (24, 24), batch 3: the first that does not (164240 bytes)                                                       -> hbm
    deep      n = 70 (25, 25, 25), batch 3: hbm, and D reaches order 70 > 64 at level 0 (types 1, 5: W = [R | T]) — spd_factor's column form,
              and the per-lane substitutions against a factor that form wrote
    wide      (RC's, n = 86, cap 90): 8 * 65 * (3 * 86 + 90) = 180960 bytes of state alone — over the limit: the single-cotangent kernel once per
              cotangent ("solve_adjoint_reg<64,hbm> x K"); ik (n = 40, cap 60, nObj 5): 135520 bytes                                 -> lds
The factors are RC.factors: problem 0's exact zero at level 0 and problem 1's 3e-16 at level 1 are in every case (the gate with NS still
accumulating).

D_CPU is the largest gap (A) against (B), relative to max(1, largest magnitude of the reference), over every case, type and set; TOL =
max(10 * D_CPU, 1e-12), the rule of the other case modules, and has to stay at or below 1e-10.  It comes from the references' own disagreement,
never from the device's figures.
MEASURED (`python tests/adjoint_reg_multi_cases.py`; bytes with the matrices in LDS / of the state alone; gap per type 1, 3, 4, 5, 8, 9):
    base            n=3   [2,2,3]            batch 4     8544 /    8352 B  solve_adjoint_reg_multi<64,lds>    gaps 7.6e-16 5.3e-16 4.6e-16 7.6e-16 7.6e-16 2.4e-16
    used_up         n=4   [3,3,3]            batch 4    11312 /   10960 B  solve_adjoint_reg_multi<64,lds>    gaps 1.3e-15 1.0e-15 1.0e-15 1.5e-15 1.5e-15 6.3e-16
    one_row         n=5   [1,3,2]            batch 4    11504 /   10960 B  solve_adjoint_reg_multi<64,lds>    gaps 4.1e-16 4.6e-16 6.0e-16 6.6e-16 6.4e-16 2.8e-16
    rank_def        n=7   [3,3,3]            batch 3    16736 /   15664 B  solve_adjoint_reg_multi<64,lds>    gaps 1.7e-15 2.4e-15 4.7e-15 1.0e-15 1.4e-15 3.5e-16
    ragged          n=5   [2,3,2]            batch 4    12032 /   11488 B  solve_adjoint_reg_multi<64,lds>    gaps 1.1e-15 1.6e-15 1.6e-15 1.2e-15 1.2e-15 3.4e-16
    fixed           n=5   [2,2,3]            batch 4    12032 /   11488 B  solve_adjoint_reg_multi<64,lds>    gaps 7.8e-16 6.2e-16 1.0e-15 1.0e-15 8.9e-16 3.1e-16
    fixed_rank_def  n=7   [3,3,3]            batch 3    16736 /   15664 B  solve_adjoint_reg_multi<64,lds>    gaps 2.6e-15 5.0e-15 5.4e-15 4.6e-15 3.6e-15 6.5e-16
    fixed_ragged    n=5   [2,3,2]            batch 4    12032 /   11488 B  solve_adjoint_reg_multi<64,lds>    gaps 5.8e-15 1.4e-15 1.3e-15 8.0e-15 8.4e-15 3.3e-16
    ik              n=40  [12,12,12,12,12]   batch 8   135520 /   93920 B  solve_adjoint_reg_multi<64,lds>    gaps 6.8e-15 2.4e-14 5.5e-14 3.3e-14 9.1e-15 9.1e-16
    wide            n=86  [20,40,30]         batch 3   344368 /  181648 B  solve_adjoint_reg<64,hbm> x K      gaps 2.7e-14    -       -    1.7e-14    -       -   
    edge_lds        n=52  [24,24]            batch 3   160576 /  106496 B  solve_adjoint_reg_multi<64,lds>    gaps 1.2e-14 3.5e-14    -    1.0e-14    -       -   
    edge            n=53  [24,24]            batch 3   164240 /  108064 B  solve_adjoint_reg_multi<64,hbm>    gaps 3.0e-14 3.6e-14    -    9.7e-14    -       -   
    deep            n=70  [25,25,25]         batch 3   256560 /  148768 B  solve_adjoint_reg_multi<64,hbm>    gaps 1.8e-14    -       -    9.1e-15    -       -   
    D_CPU = 9.7e-14 (9.66e-14 rounded up: edge, type 5)  ->  TOL = max(10 D_CPU, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
"""
import functools
import os
import sys

import numpy as np

if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adjoint_reg_cases as RC  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

D_CPU = 9.7e-14  # measured (9.66e-14, rounded up: the table above; tests/test_adjoint_reg_multi_cases.py re-measures it)
TOL = max(10.0 * D_CPU, 1e-12)

NEW = {
    "edge_lds": dict(n=52, dims=[24, 24], batch=3, seed=20330211, types=(1, 3, 5)),
    "edge": dict(n=53, dims=[24, 24], batch=3, seed=20330212, types=(1, 3, 5)),
    "deep": dict(n=70, dims=[25, 25, 25], batch=3, seed=20330213, types=(1, 5)),
}
NAMES = RC.NAMES + tuple(NEW)
SMALL = ("base", "used_up", "one_row", "rank_def", "ragged", "fixed", "fixed_rank_def", "fixed_ragged")
SETS = ("identity", "3", "65")

LD = 65  # lexls_lds.h: kAdjointMultiLd
LDS_LIMIT = 160 * 1024
LDS, HBM = "solve_adjoint_reg_multi<64,lds>", "solve_adjoint_reg_multi<64,hbm>"


def types_of(name):
    return NEW[name]["types"] if name in NEW else RC.types_of(name)


def sets_of(name):
    return SETS if name in SMALL or name == "edge" else SETS[:2]


def lds_bytes(n, cap, nobj, in_lds):
    """lexls_lds.h: adjoint_reg_multi_lds_bytes"""
    return (8 * LD * (3 * n + cap) + 8 * n + (8 * RC.matrix_doubles(n, nobj) if in_lds else 0) + 15) & ~15


def variant(n, cap, nobj):
    """lexls_lds.h: adjoint_reg_multi_form and its name"""
    if lds_bytes(n, cap, nobj, True) <= LDS_LIMIT:
        return LDS
    if lds_bytes(n, cap, nobj, False) <= LDS_LIMIT:
        return HBM
    return RC.variant(n, cap, nobj) + " x K"


def draw(name):
    if name not in NEW:
        return RC.draw(name)
    c = NEW[name]
    n, caps, B = c["n"], c["dims"], c["batch"]
    case = dict(name=name, n=n, caps=list(caps), lod=P.lse_batch(c["seed"], B, n, caps), dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), fixed={},
                g=P.normal(c["seed"] + 900, B * n).reshape(B, n), large=False)
    case["factors"] = RC.factors(B, len(caps))
    return case


def cotangents(case, st):
    """(batch, K, nVar): the identity, or K random cotangents (the same for every type of a case)"""
    B, n = case["lod"].shape[0], case["n"]
    if st == "identity":
        return np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))
    K = int(st)
    return P.normal(20330300 + K, B * K * n).reshape(B, K, n)


def solve_maps(case, reg_type):
    """per problem (M_reg (nVar, rows), N_reg (nVar, nfixed)) by unit solves on the oracle under the problem's own factors"""
    n, B, cap = case["n"], case["lod"].shape[0], sum(case["caps"])
    maps = []
    for b in range(B):
        m = int(case["dims"][b].sum())
        nf = int(case["fixed"]["nfixed"][b]) if case["fixed"] else 0
        rhs = np.zeros((1 + m + nf, cap))
        rhs[1 + np.arange(m), np.arange(m)] = 1.0
        val = np.zeros((1 + m + nf, n))
        val[1 + m + np.arange(nf), np.arange(nf)] = 1.0
        x = RC._run_one(case, b, reg_type, rhs, val)["x"]
        cols = x[1:] - x[0]
        maps.append((cols[:m].T.copy(), cols[m:].T.copy()))
    return maps


def reference_a(case, maps, G):
    """(grad_rhs (batch, K, cap), grad_fixed (batch, K, nVar)) = (G M_reg, G N_reg), zero behind a problem's rows and its fixed slots"""
    B, K, n = G.shape
    cap = sum(case["caps"])
    rhs, fixed = np.zeros((B, K, cap)), np.zeros((B, K, n))
    for b, (M, N) in enumerate(maps):
        rhs[b, :, :M.shape[1]] = G[b] @ M
        fixed[b, :, :N.shape[1]] = G[b] @ N
    return rhs, fixed


def reference_b(case, G):
    """the same from adjoint_reg_from_factor, one cotangent at a time, on the oracle's factor of the case (case["ref"])"""
    B, K, n = G.shape
    ref, nf = case["ref"], case["nf"]
    rhs, fixed = np.zeros((B, K, sum(case["caps"]))), np.zeros((B, K, n))
    for b in range(B):
        for c in range(K):
            rhs[b, c], fixed[b, c] = RC.adjoint_reg_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b],
                                                                case["dims"][b], int(nf[b]), G[b, c], case["reg_type"], case["factors"][b])
    return rhs, fixed


def gap(got, ref):
    """largest |got - ref| of a problem relative to max(1, largest |ref| of that problem)"""
    return max(float(np.abs(got[b] - ref[b]).max()) / max(1.0, float(np.abs(ref[b]).max())) for b in range(len(ref)))


@functools.lru_cache(maxsize=None)
def build(name, reg_type):
    """the case under one type: inputs, ref = the oracle's run (a problem at a time: its own factors), maps, G[set], A[set]"""
    case = draw(name)
    B = case["lod"].shape[0]
    runs = [RC._run_one(case, b, reg_type) for b in range(B)]
    case["ref"] = {key: np.concatenate([r[key] for r in runs]) for key in ("x", "factor", "hh", "perm", "rank", "fcol", "totalrank")}
    case["nf"] = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    case["reg_type"] = reg_type
    case["maps"] = solve_maps(case, reg_type)
    case["G"] = {st: cotangents(case, st) for st in sets_of(name)}
    case["A"] = {st: reference_a(case, case["maps"], G) for st, G in case["G"].items()}
    case["variant"] = variant(case["n"], sum(case["caps"]), len(case["caps"]))
    arrays = [case["lod"], case["dims"], case["g"], case["factors"], *case["ref"].values(), *case["fixed"].values(), *case["G"].values()]
    for a in arrays + [x for pair in case["A"].values() for x in pair] + [x for pair in case["maps"] for x in pair]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def cpu_gap(name, reg_type):
    """the largest gap (A) against (B) over the case's sets (CPU only: (B) is a Python loop per cotangent)"""
    case = build(name, reg_type)
    worst = 0.0
    for st, G in case["G"].items():
        B_ = reference_b(case, G)
        worst = max(worst, gap(B_[0], case["A"][st][0]), gap(B_[1], case["A"][st][1]))
    return worst


if __name__ == "__main__":
    worst = 0.0
    for nm in NAMES:
        gaps = {t: cpu_gap(nm, t) for t in types_of(nm)}
        c = build(nm, types_of(nm)[0])
        worst = max(worst, *gaps.values())
        cap, nobj = sum(c["caps"]), len(c["caps"])
        print(f"    {nm:<15} n={c['n']:<3} {str(c['caps']).replace(' ', ''):<18} batch {c['lod'].shape[0]}  {lds_bytes(c['n'], cap, nobj, True):>7} / "
              f"{lds_bytes(c['n'], cap, nobj, False):>7} B  {c['variant']:<34} gaps " + " ".join(f"{gaps[t]:.1e}" if t in gaps else "   -   " for t in RC.TYPES))
    print(f"    D_CPU (largest gap) {worst:.2e}  ->  TOL = max(10 D_CPU, 1e-12) = {max(10 * worst, 1e-12):.2e}")
