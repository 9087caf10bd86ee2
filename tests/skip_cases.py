"""Batches that hold the SKIP MASK of LexLSE (lexls_lse_set_skip, BatchedLexLSE.set_skip) to its contract on every factorization kernel family
(tests/test_gpu_lse_skip.py runs them on the GPU, tests/test_skip_cases.py asserts the conditions below on the CPU, from the oracle alone).

A case is three runs of ONE handle: lod1 without a mask, lod2 under the mask, lod3 with the mask cleared.  lod2 comes in two variants: `poison`
fills the slots of the skipped problems with NaN (a kernel that reads a skipped problem's input into anything it stores shows), `fresh` fills
them with valid iid data of another seed (a kernel that ignores the mask gives a valid, DIFFERENT result).  The live slots of lod2 hold new data,
two of them exactly rank deficient (P.rank_deficient_problem) where the levels are uniform, so neighbours of a skipped problem stop at different
pivots.  expected = the oracle on the composite batch: lod1[b] where skip[b], else lod2[b].  Dimensions and fixed variables never change.

Mask: batch 19, skipped {0, 5, 6, 7, 8, 9, 10, 11, 14, 18}.  Four problems per wavefront (lqr_qtol, lqr_quad, lqr_mfma<16>): a group with its first
member skipped (0..3), one with three skipped (4..7), a whole wavefront skipped (8..11), one skipped in the middle (12..15: 14), a tail group of three
with its last member skipped beside an idle quarter (16..18).  Two per wavefront (lqr_mfma<32>): pairs with the first (0,1), the second (4,5) and both
(6,7) members skipped.  Two degenerate masks per case: all zero (the bits of an unmasked run) and all one (every output keeps run 1's bits).

Tolerance-contract cases (lqr_qtol, lqr_mfma, the large path's step-per-pivot form) keep only STABLE problems in the sense of tests/rank_cases.py:
the same oracle ranks and first columns at tol / 10 and 10 tol.  The mask fixes the slots, so an unstable draw is not dropped but drawn again from
the next seed of the slot's series; drawn counts every draw of a live slot of lod2, kept the slots filled.  A case keeps at least three quarters of
what it drew and never redraws a skipped slot (of any of the three data sets).

MEASURED (oracle alone, `python tests/skip_cases.py`; min|dx| = smallest over the skipped problems of the largest entry by which the oracle's x on the
fresh lod2 differs from its x on lod1):
    case              n    caps                 policy keep kernel                                  drawn kept skipped live  min|dx| fresh
    qtol_ik           40   [12,12,12,12,12]     6      0    lqr_qtol<3,12,shift 7>                      9    9      10    9  1.2e+00
    qtol_8            40   [8,8,8,8,8]          6      0    lqr_qtol<3,8>                               9    9      10    9  2.6e+00
    qtol_n24          24   [12,12,12,12,12]     6      0    lqr_qtol<2,12>                              9    9      10    9  4.0e+00
    qtol_ragged       40   [12,12,12,12,12]     10     0    lqr_qtol<3,12,shift 7,ragged>               9    9      10    9  1.7e+00
    qtol_guard        40   [12,12,12,12,12]     6      0    lqr_qtol<3,12,shift 7,guard>                9    9      10    9  1.2e+00
    mfma_two          40   [12,12,12,12,12]     7      0    lqr_mfma<32,12,n40>                         9    9      10    9  1.3e+00
    mfma_one          40   [12,12,12,12,12]     8      0    lqr_mfma<64,12>                             9    9      10    9  9.1e-01
    mfma_four         40   [12,12,12,12,12]     9      0    lqr_mfma<16,12,n40>                         9    9      10    9  1.4e+00
    mfma_two_n44      44   [12,12]              7      0    lqr_mfma<32,12>                             9    9      10    9  1.0e+00
    mfma_one_n44      44   [12,12]              8      0    lqr_mfma<64,12>                             9    9      10    9  7.7e-01
    quad_ik_x         40   [12,12,12,12,12]     4      0    lqr_quad<3,12,shift 7>                      9    9      10    9  1.1e+00
    quad_ik_f         40   [12,12,12,12,12]     4      1    lqr_quad<3,12,shift 7,factor>               9    9      10    9  1.4e+00
    quad_wide_x       47   [14,9,16,8]          4      0    lqr_quad<4,16>                              9    9      10    9  3.2e+00
    quad_wide_f       47   [14,9,16,8]          4      1    lqr_quad<4,16,factor>                       9    9      10    9  2.2e+00
    quad_fixed_x      47   [14,9,16,8]          4      0    lqr_quad<4,16,fixed>                        9    9      10    9  3.1e+00
    quad_fixed_f      40   [12,12,12,12,12]     4      1    lqr_quad<3,12,shift 7,factor,fixed>         9    9      10    9  1.6e+00
    lwave_f           40   [12,12,12,12,12]     3      1    lqr_lwave<41,12,exact>                      9    9      10    9  1.3e+00
    lwave_x           31   [12,12,12]           3      0    lqr_lwave<41,12>                            9    9      10    9  1.6e+00
    wave_exact        40   [12,12,12,12,12]     2      1    lqr_wave<41,12,exact>                       9    9      10    9  1.7e+00
    wave_n31          31   [12,12,12]           2      1    lqr_wave<41,12>                             9    9      10    9  1.5e+00
    wave_64           47   [14,9,16,8]          2      1    lqr_wave<64,16>                             9    9      10    9  1.1e+00
    wave_reg          40   [12,12,12,12,12]     2      1    lqr_wave<41,12,regularized>                 9    9      10    9  1.2e+00
    generic_64        40   [12,12,12,12,12]     1      1    lqr_generic<64,lds>                         9    9      10    9  1.6e+00
    generic_256       40   [12,12,12,12,12,12]  1      1    lqr_generic<256,lds>                        9    9      10    9  1.3e+00
    generic_hbm       100  [115,115]            1      1    lqr_generic<1024,hbm>                       2    2       1    2  1.0e+00
    large_multi       100  [115,115]            5      1    lqr_large<multi-launch>                     2    2       1    2  1.0e+00
    large_fast        100  [115,115]            0      1    lqr_large<step-per-pivot,mfma>              2    2       1    2  1.0e+00
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

TOL_DEFAULT, FACTOR = 1e-12, 10.0  # the rank threshold every case runs under; the stability window of tests/rank_cases.py
RETENTION = 0.75                   # a tolerance-contract case keeps at least this share of the live problems it drew
BATCH = 19
SKIPPED = (0, 5, 6, 7, 8, 9, 10, 11, 14, 18)
# what the layout is for (tests/test_skip_cases.py finds each in the mask): (first problem of the group, mask bits of its members)
QUADS = {"first skipped": (0, (1, 0, 0, 0)), "three skipped": (4, (0, 1, 1, 1)), "whole wavefront": (8, (1, 1, 1, 1)), "middle skipped": (12, (0, 0, 1, 0)),
         "tail of three, last skipped": (16, (0, 0, 1))}
PAIRS = {"first skipped": (0, (1, 0)), "second skipped": (4, (0, 1)), "both skipped": (6, (1, 1))}
DEFICIENT = (1, 12)  # live slots of lod2 that hold exactly rank-deficient data (uniform levels, no fixed variables)

IK, WIDE = [12] * 5, [14, 9, 16, 8]
RAGGED_DIMS = np.array([[12, 12, 12, 12, 12], [12, 0, 12, 12, 12], [5, 12, 7, 12, 9], [12, 12, 12, 0, 12], [9, 12, 12, 12, 3], [12, 11, 12, 12, 12]], np.uint32)

# name -> n, caps, policy (set_kernel_policy), keep (factorize_solve(keep_factor)), kernel (last_kernel after runs 1 and 2), contract: "B" bit for
# bit, "T" pivots exact and x within test_gpu_qtol.TOL, "L" the large path's step-per-pivot contract; per_problem: dims rows dealt round the batch;
# nfixed: fixed variables per problem, dealt round the batch; reg: (type, factor of every level); guard: accuracy guard mode; batch / skipped: the
# three-problem batches of the large shape
CASES = {
    "qtol_ik": dict(n=40, caps=IK, policy=6, keep=0, kernel="lqr_qtol<3,12,shift 7>", contract="T", seed=20300100),
    "qtol_8": dict(n=40, caps=[8] * 5, policy=6, keep=0, kernel="lqr_qtol<3,8>", contract="T", seed=20300200),
    "qtol_n24": dict(n=24, caps=IK, policy=6, keep=0, kernel="lqr_qtol<2,12>", contract="T", seed=20300300),
    "qtol_ragged": dict(n=40, caps=IK, policy=10, keep=0, kernel="lqr_qtol<3,12,shift 7,ragged>", contract="T", seed=20300400, per_problem=RAGGED_DIMS),
    "qtol_guard": dict(n=40, caps=IK, policy=6, keep=0, kernel="lqr_qtol<3,12,shift 7,guard>", contract="T", seed=20300100, guard=1),
    "mfma_two": dict(n=40, caps=IK, policy=7, keep=0, kernel="lqr_mfma<32,12,n40>", contract="T", seed=20300500),
    "mfma_one": dict(n=40, caps=IK, policy=8, keep=0, kernel="lqr_mfma<64,12>", contract="T", seed=20300600),
    "mfma_four": dict(n=40, caps=IK, policy=9, keep=0, kernel="lqr_mfma<16,12,n40>", contract="T", seed=20300700),
    "mfma_two_n44": dict(n=44, caps=[12] * 2, policy=7, keep=0, kernel="lqr_mfma<32,12>", contract="T", seed=20300800),  # (the level count of tests/test_gpu_mfma.py at n = 44)
    "mfma_one_n44": dict(n=44, caps=[12] * 2, policy=8, keep=0, kernel="lqr_mfma<64,12>", contract="T", seed=20300900),
    "quad_ik_x": dict(n=40, caps=IK, policy=4, keep=0, kernel="lqr_quad<3,12,shift 7>", contract="B", seed=20301000),
    "quad_ik_f": dict(n=40, caps=IK, policy=4, keep=1, kernel="lqr_quad<3,12,shift 7,factor>", contract="B", seed=20301100),
    "quad_wide_x": dict(n=47, caps=WIDE, policy=4, keep=0, kernel="lqr_quad<4,16>", contract="B", seed=20301200),
    "quad_wide_f": dict(n=47, caps=WIDE, policy=4, keep=1, kernel="lqr_quad<4,16,factor>", contract="B", seed=20301300),
    "quad_fixed_x": dict(n=47, caps=WIDE, policy=4, keep=0, kernel="lqr_quad<4,16,fixed>", contract="B", seed=20301400, nfixed=[0, 3, 6, 2, 13]),
    "quad_fixed_f": dict(n=40, caps=IK, policy=4, keep=1, kernel="lqr_quad<3,12,shift 7,factor,fixed>", contract="B", seed=20301500, nfixed=[0, 3, 6, 2, 13]),
    "lwave_f": dict(n=40, caps=IK, policy=3, keep=1, kernel="lqr_lwave<41,12,exact>", contract="B", seed=20301600),
    "lwave_x": dict(n=31, caps=[12] * 3, policy=3, keep=0, kernel="lqr_lwave<41,12>", contract="B", seed=20301700),
    "wave_exact": dict(n=40, caps=IK, policy=2, keep=1, kernel="lqr_wave<41,12,exact>", contract="B", seed=20301800),
    "wave_n31": dict(n=31, caps=[12] * 3, policy=2, keep=1, kernel="lqr_wave<41,12>", contract="B", seed=20301900),
    "wave_64": dict(n=47, caps=WIDE, policy=2, keep=1, kernel="lqr_wave<64,16>", contract="B", seed=20302000),
    "wave_reg": dict(n=40, caps=IK, policy=2, keep=1, kernel="lqr_wave<41,12,regularized>", contract="B", seed=20302100, reg=(1, 1e-2)),
    "generic_64": dict(n=40, caps=IK, policy=1, keep=1, kernel="lqr_generic<64,lds>", contract="B", seed=20302200),
    "generic_256": dict(n=40, caps=[12] * 6, policy=1, keep=1, kernel="lqr_generic<256,lds>", contract="B", seed=20302300),  # 72 rows: beyond 64 threads
    # the `large` shape of tests/rank_cases.py: (n + 1) x 230 x 8 = 186 KB, beyond one CU's LDS; the middle problem skipped
    "generic_hbm": dict(n=100, caps=[115] * 2, policy=1, keep=1, kernel="lqr_generic<1024,hbm>", contract="B", seed=20302400, batch=3, skipped=(1,)),
    "large_multi": dict(n=100, caps=[115] * 2, policy=5, keep=1, kernel="lqr_large<multi-launch>", contract="B", seed=20302400, batch=3, skipped=(1,)),
    "large_fast": dict(n=100, caps=[115] * 2, policy=0, keep=1, kernel="lqr_large<step-per-pivot,mfma>", contract="L", seed=20302400, batch=3, skipped=(1,)),
}
CONSUMER_CASES = ("wave_exact", "quad_ik_f", "generic_64")  # factor kept: the post-factorization calls after the masked run
LB, UB, EQ = 1, 2, 3


def _dims(c, B):
    if c.get("per_problem") is not None:
        return c["per_problem"][np.arange(B) % len(c["per_problem"])].copy()
    return np.tile(np.asarray(c["caps"], np.uint32), (B, 1))


def _fixed(c, B):
    """keyword arguments of oracle.lse_run for the fixed variables ({} without): the same in all three runs"""
    if c.get("nfixed") is None:
        return {}
    n, seed = c["n"], c["seed"]
    nfixed = np.asarray(c["nfixed"], np.uint32)[np.arange(B) % len(c["nfixed"])]
    idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
    for b in range(B):
        nf = int(nfixed[b])
        idx[b, :nf] = np.argsort(P.uniform(seed + 300000 + b, n))[:nf]
        val[b, :nf] = P.normal(seed + 400000 + b, n)[:nf]
    return dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val)


def _oracle_kwargs(c):
    kw = dict(maxdim=np.asarray(c["caps"], np.uint32), nthreads=8)
    if c.get("reg"):
        kw.update(reg_type=c["reg"][0], reg_factors=[c["reg"][1]] * len(c["caps"]))
    return kw


def _run(c, lod, dims, fixed, tol=TOL_DEFAULT, **more):
    return oracle.lse_run(lod, dims, c["n"], tol=tol, **_oracle_kwargs(c), **fixed, **more)


def _stable(c, lod, dims, fixed):
    lo, hi = _run(c, lod, dims, fixed, TOL_DEFAULT / FACTOR), _run(c, lod, dims, fixed, TOL_DEFAULT * FACTOR)
    return (lo["rank"] == hi["rank"]).all(axis=1) & (lo["fcol"] == hi["fcol"]).all(axis=1)


def _deficient_ranks(n, caps):
    """level 0 three short of full, the levels behind it full while columns are left"""
    ranks, left = [], n
    for k, d in enumerate(caps):
        r = min(max(1, d - 3) if k == 0 else d, left)
        ranks.append(r)
        left -= r
    return ranks


def _problem(c, dims_b, seed, deficient):
    n, caps = c["n"], list(c["caps"])
    if deficient:
        return P.rank_deficient_problem(seed, n, caps, _deficient_ranks(n, caps))
    return P.lse_problem(seed, n, [int(d) for d in dims_b], caps)


def _data_set(c, dims, fixed, base, deficient_slots, filtered):
    """(lod, draws per slot): slot b holds the first draw of its series base + b, base + b + 100, ... that is stable (filtered cases; else the first)"""
    B = dims.shape[0]
    lod, draws = np.zeros((B, c["n"] + 1, sum(c["caps"]))), np.ones(B, int)
    for b in range(B):
        for attempt in range(8):
            lod[b] = _problem(c, dims[b], base + b + 100 * attempt, b in deficient_slots)
            one = {k: v[b:b + 1] for k, v in fixed.items()}
            if not filtered or _stable(c, lod[b:b + 1], dims[b:b + 1], one)[0]:
                break
            draws[b] += 1
        else:
            raise AssertionError(f"slot {b}: no stable draw")
    return lod, draws


def _sensitivity(c, lod, dims, fixed, ref, seed):
    """one-ulp sensitivity of x as tests/rank_cases.py measures it: the data perturbed by +-1.1e-16 relative, three draws, oracle only"""
    s = np.zeros(lod.shape[0])
    for rep in range(3):
        sign = np.where(P.uniform(seed + 31 * rep, lod.size, 7).reshape(lod.shape) < 0.5, -1.0, 1.0)
        x = _run(c, lod * (1.0 + 1.1e-16 * sign), dims, fixed)["x"]
        s = np.maximum(s, np.abs(x - ref["x"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1)))
    return s


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: dict(n, caps, policy, keep, kernel, contract, dims, fixed, skip (uint8 mask), lod1, lod2 = {poison, fresh}, lod3, ref1, ref3,
    expected (the oracle on the composite batch), ref2_fresh (the oracle on the fresh lod2), composite, sens = {1, expected, 3, fresh} for contract "L",
    drawn / kept (live slots of lod2), redrawn_skipped)"""
    c = CASES[name]
    B, seed = c.get("batch", BATCH), c["seed"]
    skipped = np.asarray(c.get("skipped", SKIPPED))
    skip = np.zeros(B, np.uint8)
    skip[skipped] = 1
    live = np.flatnonzero(skip == 0)
    dims, fixed = _dims(c, B), _fixed(c, B)
    filtered = c["contract"] in ("T", "L")
    uniform = c.get("per_problem") is None and not fixed and B == BATCH
    lod1, d1 = _data_set(c, dims, fixed, seed, (), filtered)
    new, d2 = _data_set(c, dims, fixed, seed + 1000, DEFICIENT if uniform else (), filtered)
    other, d2s = _data_set(c, dims, fixed, seed + 2000, (), filtered)
    lod3, d3 = _data_set(c, dims, fixed, seed + 3000, (), filtered)
    composite = np.where(skip[:, None, None] != 0, lod1, new)
    lod2 = dict(poison=np.where(skip[:, None, None] != 0, np.nan, new), fresh=np.where(skip[:, None, None] != 0, other, new))
    case = dict(name=name, n=c["n"], caps=list(c["caps"]), policy=c["policy"], keep=bool(c["keep"]), kernel=c["kernel"], contract=c["contract"],
                reg=c.get("reg"), guard=c.get("guard", 0), dims=dims, fixed=fixed, skip=skip, skipped=skipped, live=live, lod1=lod1, lod2=lod2, lod3=lod3,
                composite=composite, ref1=_run(c, lod1, dims, fixed), ref3=_run(c, lod3, dims, fixed), expected=_run(c, composite, dims, fixed),
                ref2_fresh=_run(c, lod2["fresh"], dims, fixed), deficient=[b for b in DEFICIENT if uniform],
                drawn=int(d2[live].sum()), kept=len(live), redrawn_skipped=int((d1[skipped] - 1).sum() + (d2s[skipped] - 1).sum() + (d3[skipped] - 1).sum()))
    if c["contract"] == "L":
        case["sens"] = {1: _sensitivity(c, lod1, dims, fixed, case["ref1"], seed), "expected": _sensitivity(c, composite, dims, fixed, case["expected"], seed + 1),
                        3: _sensitivity(c, lod3, dims, fixed, case["ref3"], seed + 2), "fresh": _sensitivity(c, lod2["fresh"], dims, fixed, case["ref2_fresh"], seed + 3)}
    for a in [dims, skip, lod1, lod3, composite, *lod2.values(), *fixed.values()] + [v for k in ("ref1", "ref3", "expected", "ref2_fresh") for v in case[k].values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


@functools.lru_cache(maxsize=None)
def consumers(name):
    """what the post-factorization calls must give on the composite batch of a factor-kept case (oracle only): types (LB / UB / EQ mixed), level (the
    last one), sens / maxabs / lam of ObjectiveSensitivity(level), mult (batch, nObj, n + cap), v; g and the adjoint from the oracle's factor
    (adjoint_cases.adjoint_from_factor, reference (B) of tests/adjoint_cases.py)"""
    import adjoint_cases as AC
    case, c = build(name), CASES[name]
    B, n, nobj, cap = len(case["skip"]), case["n"], len(case["caps"]), sum(case["caps"])
    types = (1 + (P.uniform(c["seed"] + 200000, B * cap) * 3).astype(np.uint8)).reshape(B, cap)
    per_level = [_run(c, case["composite"], case["dims"], case["fixed"], ctr_type=types, sens_obj=k) for k in range(nobj)]
    last = per_level[-1]
    g = P.normal(c["seed"] + 900, B * n).reshape(B, n)
    e = case["expected"]
    adj = [AC.adjoint_from_factor(e["factor"][b], e["hh"][b], e["perm"][b], e["rank"][b], e["fcol"][b], e["totalrank"][b], case["dims"][b], 0, g[b]) for b in range(B)]
    return dict(types=types, level=nobj - 1, sens=last["sens"], maxabs=last["maxabs"], lam=last["lam"], marks=last["ctr_type_out"],
                mult=np.stack([r["lam"] for r in per_level], axis=1), v=e["v"], g=g, grad_rhs=np.stack([a[0] for a in adj]))


# ---- the accuracy guard under the mask ------------------------------------------------------------------------------------------------------
GUARD_N, GUARD_THRESHOLD = 40, 64.0  # the IK shape; the guard's calibrated default (scripts/calibrate_guard.py, DESIGN.md "Accuracy guard")
GUARD_FLAGGED_RUN1 = 5       # skipped, ill-conditioned in lod1: flagged and re-solved in run 1, well-conditioned fresh data in lod2
GUARD_WOULD_FLAG = 6         # skipped, well-conditioned in lod1, ill-conditioned fresh data in lod2: a kernel that solved it would flag it
GUARD_LIVE_FLAGGED = (1, 12)  # live, ill-conditioned in lod2: re-solved under (B) in run 2


@functools.lru_cache(maxsize=None)
def guard_case():
    """19 problems of the calibration sets of scripts/calibrate_guard.py (what tests/test_gpu_accuracy_guard.py builds): configs[2] for the
    well-conditioned slots, `near-dependent 3e-6` for the ill-conditioned ones.  dict(skip, lod1, lod2 (fresh), composite, ref1, expected,
    est1 / est2 / est_expected: the calibration script's estimate from the oracle's factor)"""
    from scripts import calibrate_guard as CG
    sets = dict(CG.guard_sets())
    good, ill = sets["configs[2]"], sets["near-dependent 3e-6"]
    skip = np.zeros(BATCH, np.uint8)
    skip[list(SKIPPED)] = 1
    lod1, lod2 = good[:BATCH].copy(), good[BATCH:2 * BATCH].copy()
    lod1[GUARD_FLAGGED_RUN1] = ill[0]
    lod2[GUARD_WOULD_FLAG] = ill[1]
    for i, b in enumerate(GUARD_LIVE_FLAGGED):
        lod2[b] = ill[2 + i]
    composite = np.where(skip[:, None, None] != 0, lod1, lod2)
    run = lambda lod: oracle.lse_run(lod, IK, GUARD_N, nthreads=8)  # noqa: E731
    ref1, ref2, expected = run(lod1), run(lod2), run(composite)
    case = dict(skip=skip, lod1=lod1, lod2=lod2, composite=composite, ref1=ref1, expected=expected, est1=CG.estimate(lod1, IK, GUARD_N, ref1),
                est2=CG.estimate(lod2, IK, GUARD_N, ref2), est_expected=CG.estimate(composite, IK, GUARD_N, expected))
    for a in [skip, lod1, lod2, composite, *ref1.values(), *expected.values()]:
        a.setflags(write=False)
    return case


def fresh_gap(case):
    """smallest over the skipped problems of the largest entry by which x on the fresh lod2 differs from x on lod1"""
    s = case["skipped"]
    return float(np.abs(case["ref2_fresh"]["x"][s] - case["ref1"]["x"][s]).max(axis=1).min())


def summary(case):
    return (f"    {case['name']:<17} {case['n']:<4} {str(case['caps']).replace(' ', ''):<20} {case['policy']:<6} {int(case['keep']):<4} {case['kernel']:<40} "
            f"{case['drawn']:>4} {case['kept']:>4} {len(case['skipped']):>7} {len(case['live']):>4}  {fresh_gap(case):.1e}")


if __name__ == "__main__":
    print("    case              n    caps                 policy keep kernel                                  drawn kept skipped live  min|dx| fresh")
    for nm in CASES:
        print(summary(build(nm)))
