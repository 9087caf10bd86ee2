"""Cases that hold the multi-cotangent adjoint of the LexLSE solve (lexls_lse_solve_adjoint_multi, lexls_amd/csrc/lse_adjoint.hip:
solve_adjoint_multi_kernel, lane = cotangent) to the references of tests/adjoint_cases.py, cotangent by cotangent
(tests/test_adjoint_multi_cases.py asserts on the CPU that the references agree; tests/test_gpu_lse_adjoint_multi.py compares the device
with them).

The cases are those of adjoint_cases.py (NAMES) plus:
    beyond      n = 200 (150, 50), batch 2, iid data, full rank: the per-lane state alone (65 x 400 doubles = 208 KB) exceeds one workgroup's
                160 KiB, so the launcher takes the single-cotangent kernel once per cotangent — (B) + identities, as the large cases
    fit_*       (FIT_NAMES, a test of their own) n = 40, batch 2, iid data in levels of 12 rows, on both sides of the fit rule's two switches
                as lds_bytes() below restates them: fit_staged_last cap = 167 ([12] x 13 + [11]: 162736 of 163840 bytes), fit_hbm_first cap =
                168 (staged it would need 163904), fit_hbm_last cap = 274 (163600), fit_single_first cap = 275 (the state alone 164128).  The
                kernel carves exactly adjoint_multi_lds_bytes out of LDS, so an off-by-one in the rule or in the carving shows here or
                nowhere.  The first four levels take the 40 columns; reference (A), the unit solves.

Cotangent sets per case, cut from ONE master set R of 65 cotangents per problem (R[:, 0] = the case's own g, the rest iid normal) so that the
reference is computed once:
    1           R[:, :1]    the case's own g
    3           R[:, :3]
    64          R[:, :64]   a full tile: the tile edge
    65          R           a second tile with one live lane
    identity    K = nVar, the unit vectors: the Jacobian, grad_rhs = M^T ... row i of it is row i of M
References, per cotangent:
    (B)  adjoint_cases.adjoint_from_factor on the oracle's factor
    (A)  small cases: M and N by unit solves on the oracle (unit_solve_matrices), then R M and R N in numpy; the identity cotangents give
         M and N themselves
    identities  large cases: <g_c, x(b1) - x(b0)> = <grad_rhs_c, b1 - b0> for the three pairs, every cotangent c of R

D_CPU_MULTI is the largest discrepancy of the CPU test — (A) against (B), identity cotangents included, and both sides of the identities with
(B)'s grad_rhs — each relative to max(1, largest magnitude of the problem's reference).  TOL_MULTI = max(10 * D_CPU_MULTI, 1e-12), the
rule of adjoint_cases.py; it has to stay at or below 1e-10: data that would need more are replaced, the tolerance is not raised.
MEASURED (`python tests/adjoint_multi_cases.py`, the oracle and numpy alone):
    base              n=3    [2,2,3]            batch 4  ranks [2,1,0] x 4                                   gap 2.9e-16
    used_up           n=4    [3,3,3]            batch 4  ranks [3,1,0] x 4                                   gap 4.8e-16
    one_row           n=5    [1,3,2]            batch 4  ranks [1,3,1] x 4                                   gap 5.6e-16
    rank_def          n=7    [3,3,3]            batch 3  ranks [2,0,2] x 3                                   gap 5.2e-16
    ragged            n=5    [2,3,2]            batch 4  ranks [2,3,0] [2,0,2] [1,3,0] [0,3,2]               gap 3.6e-16
    fixed             n=5    [2,2,3]            batch 4  ranks [2,1,0] [2,1,0] [0,0,0] [2,2,0]               gap 5.2e-16
    ik                n=40   [12,12,12,12,12]   batch 8  ranks [12,12,12,4,0] x 8                            gap 1.5e-15
    wide              n=70   [20,40,30]         batch 3  ranks [20,40,10] x 3                                gap 7.6e-16
    large             n=127  [100,1,0,40,24]    batch 2  ranks [17,1,0,5,10] [9,0,0,16,8]                    gap 7.5e-16
    fixed_wide        n=70   [20,40,30]         batch 3  ranks [20,40,4] [20,40,1] [20,40,10]                gap 1.8e-15
    fixed_rank_def    n=7    [3,3,3]            batch 3  ranks [2,0,2] x 3                                   gap 1.8e-15
    fixed_ragged      n=5    [2,3,2]            batch 4  ranks [2,1,0] [2,0,2] [1,0,0] [0,3,1]               gap 4.6e-16
    fixed_tall        n=12   [70,30]            batch 2  ranks [7,0] [5,0]                                   gap 2.6e-16
    beyond            n=200  [150,50]           batch 2  ranks [150,50] x 2                                  gap 1.1e-15
    fit_staged_last   n=40   [12]x13+[11]       batch 2  ranks [12,12,12,4,0,...] x 2                        gap 1.2e-15
    fit_hbm_first     n=40   [12]x14            batch 2  ranks [12,12,12,4,0,...] x 2                        gap 1.2e-15
    fit_hbm_last      n=40   [12]x22+[10]       batch 2  ranks [12,12,12,4,0,...] x 2                        gap 1.1e-15
    fit_single_first  n=40   [12]x22+[11]       batch 2  ranks [12,12,12,4,0,...] x 2                        gap 1.3e-15
    D_CPU_MULTI = 1.80e-15 (fixed_rank_def)  ->  TOL_MULTI = max(10 D_CPU_MULTI, 1e-12) = 1e-12, a hundredth of the 1e-10 of the tolerance contract.
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

D_CPU_MULTI = 1.80e-15  # measured: the table above (tests/test_adjoint_multi_cases.py re-measures it)
TOL_MULTI = max(10.0 * D_CPU_MULTI, 1e-12)

# cases of this file alone: name -> n, dims, batch, seed; large: reference (B) + identities, else the unit solves
EXTRA = {"beyond": dict(n=200, dims=[150, 50], batch=2, seed=20290301, large=True)}
NAMES = list(AC.CASES) + ["beyond"]
SETS = ("1", "3", "64", "65", "identity")
NR = 65  # cotangents of the master set

# ---- the fit rule, restated from lexls_amd/csrc/lexls_lds.h (adjoint_multi_lds_bytes, adjoint_multi_form); tests/test_adjoint_multi_cases.py holds
# the restatement to tests/adjoint_multi_fit_check.cpp's numbers ----
LDS_LIMIT = 160 * 1024  # kMaxLdsBytes: one workgroup's LDS
STAGED, HBM, SINGLE = "solve_adjoint_multi<64,staged>", "solve_adjoint_multi<64,hbm>", "solve_adjoint<64> x K"


def lds_bytes(n, cap, staged):
    """the per-lane state gh (n) and cb (cap), [index][lane] with leading dimension 65, and 2 n words of transpositions and positions; staged:
    + the factor's n columns (odd leading dimension cap | 1) and hh (cap)"""
    b = 8 * 65 * (n + cap) + 8 * n
    if staged:
        b += 8 * ((cap | 1) * n + cap)
    return (b + 15) & ~15


def form(n, cap):
    return STAGED if lds_bytes(n, cap, True) <= LDS_LIMIT else (HBM if lds_bytes(n, cap, False) <= LDS_LIMIT else SINGLE)


def last_cap(n, form_name):
    """the largest cap the rule still sends to `form_name` at n variables (the rule is monotone in cap)"""
    cap = 1
    while form(n, cap + 1) == form_name or form(n, cap) != form_name:
        cap += 1
    return cap


def levels_of(cap, dim=12):
    """cap rows in levels of `dim`, the rest in a last shorter one"""
    return [dim] * (cap // dim) + ([cap % dim] if cap % dim else [])


# device runs on both sides of the rule's two switches at n = 40: the last staged shape, the first hbm shape, the last hbm shape, the first
# per-cotangent shape.  iid data, batch 2; the first four levels take the 40 columns (ranks 12, 12, 12, 4)
FIT_N = 40
FIT_CAPS = {"fit_staged_last": last_cap(FIT_N, STAGED), "fit_hbm_first": last_cap(FIT_N, STAGED) + 1, "fit_hbm_last": last_cap(FIT_N, HBM),
            "fit_single_first": last_cap(FIT_N, HBM) + 1}
FIT_NAMES = list(FIT_CAPS)
for _i, (_name, _cap) in enumerate(FIT_CAPS.items()):
    EXTRA[_name] = dict(n=FIT_N, dims=levels_of(_cap), batch=2, seed=20310201 + _i, large=False)

# the form the host-side fit rule (lexls_lds.h: adjoint_multi_form) has to give each case
FORMS = {name: STAGED for name in AC.CASES}
FORMS.update(large=HBM, beyond=SINGLE)
FORMS.update({name: form(FIT_N, cap) for name, cap in FIT_CAPS.items()})
# case -> kernel policy -> the producer of the kept factor (adjoint_cases.PRODUCERS and this file's own cases)
PRODUCERS = dict(AC.PRODUCERS, beyond={5: "lqr_large<multi-launch>"}, **{name: {0: AC.GENERIC256} for name in FIT_NAMES})


def _base(name):
    """the case's inputs, the oracle's run on them and, for the large cases, the three pairs of the identities"""
    if name not in EXTRA:
        return AC.build(name)
    c = EXTRA[name]
    n, caps, B, seed = c["n"], list(c["dims"]), c["batch"], c["seed"]
    cap = sum(caps)
    case = dict(name=name, n=n, caps=caps, lod=P.lse_batch(seed, B, n, caps), dims=np.tile(np.asarray(caps, np.uint32), (B, 1)), fixed={},
                g=P.normal(seed + 900, B * n).reshape(B, n), large=c["large"], A=None, pairs=[])
    case["ref"] = oracle.lse_run(case["lod"], case["dims"], n, maxdim=np.asarray(caps, np.uint32), nthreads=4)
    for t in range(3 if c["large"] else 0):
        b0 = P.normal(seed + 7000 + 2 * t, B * cap).reshape(B, cap)
        b1 = P.normal(seed + 7001 + 2 * t, B * cap).reshape(B, cap)
        case["pairs"].append((b1 - b0, AC._solve(case, b1)["x"] - AC._solve(case, b0)["x"]))
    return case


def cotangents(case):
    """the master set R (batch, 65, n): R[:, 0] = the case's g"""
    B, n = case["g"].shape
    seed = (EXTRA.get(case["name"]) or AC.CASES[case["name"]])["seed"]
    R = P.normal(seed + 4000, B * NR * n).reshape(B, NR, n)
    R[:, 0, :] = case["g"]
    return R


def select(name_of_set, R):
    """the cotangent set `name_of_set` (batch, K, n) cut from the master set"""
    if name_of_set == "identity":
        B, _, n = R.shape
        return np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))
    return np.ascontiguousarray(R[:, :int(name_of_set), :])


def select_ref(name_of_set, case, which):
    """the reference for that set: which = 0 grad_rhs (batch, K, cap), 1 grad_fixed (batch, K, n)"""
    return case["ref_identity"][which] if name_of_set == "identity" else case["ref_R"][which][:, :int(name_of_set)]


def unit_solve_matrices(case):
    """reference (A): M (batch, n, cap) and N (batch, n, n) of x = M b + N x_fixed by unit solves on the oracle; the columns behind a
    problem's own rows, and from nfixed on, are zero (nothing reads those entries)"""
    n, B, cap = case["n"], case["lod"].shape[0], sum(case["caps"])
    m = case["dims"].sum(axis=1)
    x0 = AC._solve(case, np.zeros((B, cap)))["x"]
    M, N = np.zeros((B, n, cap)), np.zeros((B, n, n))
    for i in range(cap):
        e = np.zeros((B, cap))
        e[:, i] = 1.0
        M[:, :, i] = np.where((i < m)[:, None], AC._solve(case, e)["x"] - x0, 0.0)
    if case["fixed"]:
        nf = case["fixed"]["nfixed"]
        for j in range(int(nf.max())):
            val = np.zeros((B, n))
            val[:, j] = 1.0
            N[:, :, j] = np.where((j < nf)[:, None], AC._solve(case, np.zeros((B, cap)), val)["x"] - x0, 0.0)
    return M, N


def from_factor(case, G):
    """reference (B) for the cotangents G (batch, K, n): (grad_rhs (batch, K, cap), grad_fixed (batch, K, n))"""
    ref, B, K = case["ref"], G.shape[0], G.shape[1]
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    out = [[AC.adjoint_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b],
                                   case["dims"][b], int(nf[b]), G[b, c]) for c in range(K)] for b in range(B)]
    return np.array([[o[0] for o in row] for row in out]), np.array([[o[1] for o in row] for row in out])


def gap(got, ref):
    """largest error per problem over its cotangents, relative to max(1, largest magnitude of the problem's reference)"""
    return max(float(np.abs(got[b] - ref[b]).max()) / max(1.0, float(np.abs(ref[b]).max())) for b in range(len(ref)))


def identities(case, G, grad_rhs):
    """the largest gap of the three dot-product identities over the cotangents of G (large cases; 0.0 where there are no pairs)"""
    return max([AC.identity_gap(pair, G[:, c], grad_rhs[:, c]) for pair in case["pairs"] for c in range(G.shape[1])], default=0.0)


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name` with R (the master set), B_R / B_identity (reference (B)), A_R / A_identity (reference (A), None for the large cases),
    M / N (None for the large cases), ref_R / ref_identity (what the device is compared with: (A), for the large cases (B)), gap"""
    case = dict(_base(name))
    R = cotangents(case)
    I = select("identity", R)
    case["R"] = R
    case["B_R"], case["B_identity"] = from_factor(case, R), from_factor(case, I)
    if case["large"]:
        case["M"] = case["N"] = case["A_R"] = case["A_identity"] = None
        case["ref_R"], case["ref_identity"] = case["B_R"], case["B_identity"]
        case["gap"] = max(identities(case, R, case["B_R"][0]), identities(case, I, case["B_identity"][0]))
    else:
        M, N = unit_solve_matrices(case)
        case["M"], case["N"] = M, N
        case["A_R"] = (R @ M, R @ N)          # row c of problem b: M^T g_c, N^T g_c
        case["A_identity"] = (M.copy(), N.copy())  # the unit cotangents: row i = row i of M, of N
        case["ref_R"], case["ref_identity"] = case["A_R"], case["A_identity"]
        case["gap"] = max(gap(case["A_R"][w], case["B_R"][w]) for w in (0, 1))
        case["gap"] = max(case["gap"], *(gap(case["A_identity"][w], case["B_identity"][w]) for w in (0, 1)))
    for key in ("R", "M", "N"):
        if case[key] is not None:
            case[key].setflags(write=False)
    for key in ("B_R", "B_identity", "A_R", "A_identity"):
        for a in case[key] or ():
            a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def summary(case):
    return (f"    {case['name']:<15} n={case['n']:<4} {str(case['caps']).replace(' ', ''):<18} batch {case['lod'].shape[0]}  ranks "
            f"{' '.join(str(r.tolist()).replace(' ', '') for r in case['ref']['rank']):<44} gap {case['gap']:.1e}")


if __name__ == "__main__":
    worst = 0.0
    for nm in NAMES + FIT_NAMES:
        c = build(nm)
        worst = max(worst, c["gap"])
        print(summary(c))
    print(f"    D_CPU_MULTI (largest gap) {worst:.2e}  ->  TOL_MULTI = max(10 D_CPU_MULTI, 1e-12) = {max(10 * worst, 1e-12):.2e}")
