"""Batches that hold the REGULARIZATION family (lexls_amd/csrc/lexls_regularize.h, lexlse.h:277-411: in lqr_wave<..,regularized> and in lqr_generic)
to the oracle on both sides of its switches (tests/test_gpu_regularization.py runs them on the GPU, bit for bit; tests/test_reg_cases.py asserts
on the CPU, from the oracle and the planner alone, that each case stands where this text says).

Data: P.lse_batch with the seeds below, batch 3 - 5; per-problem factors |N(0,1)| * 0.3 + 0.05, one oracle call per problem.  So that a case is
not vacuous: every problem b with b % 3 == 1 repeats a row (a rank-deficient level: `short` below counts the problems whose level lost a rank
by it); every odd problem has one factor exactly 0.0 (regularize_level's nonzero == false: problem 1 at level 0, problem 3 at level 1); problem
0 has neither.  Fixed variables (m0 = Fc - nf) in p41_27 and window (wave kernels), g70r and t7 (generic kernel).

The switches, and the case on each side of each:
 1. Placement of the work matrix and of the null-space basis (wave_reg_lds_bytes -> reg_cfg -> RegView::with_order), four levels, 20 KB share.
    lqr_wave<41,12,regularized> (p41_<n>: four levels of (n + 4) / 4 + 1 rows): basis in LDS | not: types 1 and 8 p41_22 | p41_23, type 2
    p41_25 | p41_26, type 3 p41_26 | p41_27; window | none: type 8 p41_28 | p41_29, type 1 p41_29 | p41_30 (type 3's 12 x 12 window fits at every
    n).  lqr_wave<64,16,regularized> (p64_<n>: n <= 40 reaches it through a last level of 13 rows): basis: types 1, 8 and 3 p64_15 | p64_16,
    type 2 p64_17 | p64_18; window: types 1 and 8 p64_20 | p64_21, type 3 p64_24 | p64_25.  FLIPS lists them; PLAN holds kernel, window order and
    basis bit of every (case, type), equal to what tests/reg_plan_check.cpp prints and to what last_kernel() / last_reg_placement() answer.
    UNREACHABLE: a run in which with_order sends some levels to the window and others to the scratch.  Where a window is placed it holds every
    order its type can ask for: for TIKHONOV tikhonov_2 runs while Fc + rank <= n - Fc - rank, so its order Fc - nf + rank <= n / 2, and
    tikhonov_1 otherwise, so its order n - Fc <= ceil(n / 2) - 1 + rank < n / 2 + MD + 1, the window's (tests/test_reg_cases.py walks every
    n, Fc, rank, nf of both shapes).  `window` (n = 29, [12,12,12], window 27) takes both Tikhonov branches in one problem (0, 2 and 3; problem 1's level 0 has the factor 0.0) and reaches the
    largest order the shape can produce, 26 (problem 4: three fixed variables send level 0 to tikhonov_1); the scratch side of with_order is the side of the cases without a window.
 2. spd_solve_wave's panels of 16 (lse_spd_solve.h, behind reg_cholesky_solve): `panel`, n = 63 [16,1,15,1,15,1,14], type 8: problem 0 (full ranks, no zero factor) has the orders
    16, 17, 32, 33, 48, 49, 63; the same hierarchy under types 1 (orders 14 .. 46 by tikhonov_1, 16, 17, 31 by tikhonov_2) and 5; again under
    policy 1, where the same routine runs inside lqr_generic<64,lds>.
 3. spd_solve<NT> (behind reg_cholesky_solve<NT>), workgroup form: g64 (n = 64 [20,20], the first shape past the wave family), g100, g130 ([70,40,30]: a level over 64
    rows, last rank 20; orders 130 (type 1), 70 .. 130 (type 8), 70 (types 3, 5)), g70r (per-problem dimensions, an empty level, fixed
    variables) on lqr_generic<256,lds>; g150 on lqr_generic<1024,hbm>; `tall` (n = 20, 520 rows) on lqr_generic<1024,lds>, which a regularized
    shape does reach: more than 512 rows of a problem whose matrix still fits the LDS.  Orders within 64 on NT = 256 / 1024: g100 types 3 - 5.
 4. reg_cg's two exits: cg_w (wave reductions, lqr_wave<41,12,regularized>; levels of 12 rows: with 8 the CGLS of type 6 converges within 9
    steps) and cg_g (one-thread reductions, NT = 256) at caps 1, 10 and 400: x(9) != x(10) in every problem (cap 10 leaves by the cap),
    x(400) == x(401) bit for bit (400 leaves by sqrt(gamma) <= 1e-12).  UNREACHABLE: a cap of 0 — the oracle's binding reads 0 as "the
    default, 10" (oracle_lse_set_regularization), so it cannot say what zero iterations give.  g150 runs types 2 and 6 on NT = 1024.
 5. Types 4, 5, 6, 9 beyond the random sweep: p41_26, p64_20, g100, g150 run all eight non-experimental types: each of the four kernels per type.
 6. The conditioning-dependent factor: vf_w (n = 28, eps 8.2) and vf_g (n = 100, eps 20), types 1 and 3: ce < eps at half of the ranked levels,
    ce >= eps at the others, the nearest 4 % away from eps.
 7. Type 7 with by-products: t7, n = 70 [25,25,25], fixed variables in one problem (get_mu against the oracle's X_mu / residual_mu).

Conditions (tests/test_reg_cases.py): (a) PLAN is the planner's and the launcher's own arithmetic (reg_plan_check, also under the address and
undefined-behaviour sanitizers), the cases of FLIPS are neighbours in n on opposite sides; (b) the orders below come from the oracle's ranks and
first columns as regularize_level decides; (c) both CG exits; (d) every case's x differs from the unregularized x by more than 1e-6 in every
problem, permutations and ranks do not, and a level 0 with the factor 0.0 keeps the unregularized right-hand side; (e) ce recomputed in numpy.

MEASURED (oracle alone, `python tests/reg_cases.py`; ranks = the levels' ranks of problem 0; short = problems whose duplicated row cost a rank;
zero = (problem, level) pairs with the factor 0.0; nf = 1: fixed variables; per type the orders of the Cholesky factorizations of the ranked,
damped levels (T1 / T2: by tikhonov_1 / tikhonov_2) and dx = the smallest over the problems of the largest entry the regularization moves):
    p41_22  n=22  [7,7,7,7]              batch 3 ranks [7,7,7,1]              short 1 zero 1 nf 0 | 1:T1[1,2,8,9,15]T2[7] dx 6.0e-02; 8:[7,13,14,20,21,22] dx 6.0e-02; 3:[1,2,6,7] dx 2.0e-01; 2: dx 6.0e-02
    p41_23  n=23  [7,7,7,7]              batch 3 ranks [7,7,7,2]              short 1 zero 1 nf 0 | 1:T1[2,3,9,10,16]T2[7] dx 6.3e-02; 8:[7,13,14,20,21,23] dx 6.3e-02; 3:[2,3,6,7] dx 1.1e-01; 2: dx 6.3e-02
    p41_25  n=25  [8,8,8,8]              batch 3 ranks [8,8,8,1]              short 1 zero 1 nf 0 | 1:T1[1,2,9,10,17]T2[8] dx 9.3e-02; 8:[8,15,16,23,24,25] dx 9.3e-02; 3:[1,2,7,8] dx 1.2e-01; 2: dx 9.3e-02
    p41_26  n=26  [8,8,8,8]              batch 3 ranks [8,8,8,2]              short 1 zero 1 nf 0 | 1:T1[2,3,10,11,18]T2[8] dx 3.4e-02; 2: dx 3.4e-02; 3:[2,3,7,8] dx 4.2e-02; 4:[2,3,7,8] dx 4.3e-02; 5:[2,3,7,8] dx 1.2e-02; 6: dx 1.2e-02; 8:[8,15,16,23,24,26] dx 3.4e-02; 9: dx 1.1e+00
    p41_27  n=27  [8,8,8,8]              batch 3 ranks [8,8,8,3]              short 1 zero 1 nf 1 | 1:T1[2,3,10,11,17,18,19]T2[8] dx 1.3e-02; 8:[8,15,16,23,24,25,26,27] dx 1.3e-02; 3:[2,3,7,8] dx 2.4e-02; 2: dx 1.3e-02
    p41_28  n=28  [9,9,9,9]              batch 3 ranks [9,9,9,1]              short 1 zero 1 nf 0 | 1:T1[1,2,10,11,19]T2[9] dx 2.7e-02; 8:[9,17,18,26,27,28] dx 2.7e-02; 3:[1,2,8,9] dx 1.4e-01; 2: dx 2.7e-02
    p41_29  n=29  [9,9,9,9]              batch 3 ranks [9,9,9,2]              short 1 zero 1 nf 0 | 1:T1[2,3,11,12,20]T2[9] dx 3.9e-02; 8:[9,17,18,26,27,29] dx 3.9e-02; 3:[2,3,8,9] dx 5.1e-02; 2: dx 3.8e-02
    p41_30  n=30  [9,9,9,9]              batch 3 ranks [9,9,9,3]              short 1 zero 1 nf 0 | 1:T1[3,4,12,13,21]T2[9] dx 1.1e-01; 8:[9,17,18,26,27,30] dx 1.1e-01; 3:[3,4,8,9] dx 1.2e-01; 2: dx 1.2e-01
    p64_15  n=15  [4,4,4,13]             batch 3 ranks [4,4,4,3]              short 1 zero 1 nf 0 | 1:T1[3,4,7,8,11]T2[4,7] dx 6.0e-02; 8:[4,7,8,11,12,15] dx 6.0e-02; 3:[3,4] dx 6.6e-02; 2: dx 6.0e-02
    p64_16  n=16  [4,4,4,13]             batch 3 ranks [4,4,4,4]              short 1 zero 1 nf 0 | 1:T1[4,5,8,9]T2[4,7,8] dx 3.2e-02; 8:[4,7,8,11,12,16] dx 3.2e-02; 3:[3,4,5] dx 4.5e-02; 2: dx 3.2e-02
    p64_17  n=17  [4,4,4,13]             batch 3 ranks [4,4,4,5]              short 1 zero 1 nf 0 | 1:T1[5,6,9,10]T2[4,7,8] dx 7.8e-02; 8:[4,7,8,11,12,17] dx 7.8e-02; 3:[3,4,5,6] dx 1.5e-01; 2: dx 7.8e-02
    p64_18  n=18  [5,5,5,13]             batch 3 ranks [5,5,5,3]              short 1 zero 1 nf 0 | 1:T1[3,4,8,9,13]T2[5,9] dx 7.6e-02; 8:[5,9,10,14,15,18] dx 7.6e-02; 3:[3,4,5] dx 1.6e-01; 2: dx 7.6e-02
    p64_20  n=20  [5,5,5,13]             batch 3 ranks [5,5,5,5]              short 1 zero 1 nf 0 | 1:T1[5,6,10,11]T2[5,9,10] dx 4.6e-02; 2: dx 4.6e-02; 3:[4,5,6] dx 8.8e-02; 4:[4,5,6] dx 4.5e-02; 5:[4,5,6] dx 2.8e-02; 6: dx 2.8e-02; 8:[5,9,10,14,15,20] dx 4.6e-02; 9: dx 6.2e-01
    p64_21  n=21  [6,6,6,13]             batch 3 ranks [6,6,6,3]              short 1 zero 1 nf 0 | 1:T1[3,4,9,10,15]T2[6] dx 3.1e-02; 8:[6,11,12,17,18,21] dx 3.1e-02; 3:[3,4,5,6] dx 4.5e-02; 2: dx 3.1e-02
    p64_24  n=24  [7,7,7,13]             batch 3 ranks [7,7,7,3]              short 1 zero 1 nf 0 | 1:T1[3,4,10,11,17]T2[7] dx 7.0e-02; 8:[7,13,14,20,21,24] dx 7.0e-02; 3:[3,4,6,7] dx 3.9e-02; 2: dx 7.0e-02
    p64_25  n=25  [7,7,7,13]             batch 3 ranks [7,7,7,4]              short 1 zero 1 nf 0 | 1:T1[4,5,11,12,18]T2[7] dx 1.5e-02; 8:[7,13,14,20,21,25] dx 1.5e-02; 3:[4,5,6,7] dx 3.1e-02; 2: dx 1.5e-02
    window  n=29  [12,12,12]             batch 5 ranks [12,12,5]              short 2 zero 2 nf 1 | 1:T1[3,4,5,6,14,16,17,26]T2[12] dx 6.4e-03
    panel   n=63  [16,1,15,1,15,1,14]    batch 3 ranks [16,1,15,1,15,1,14]    short 1 zero 1 nf 0 | 8:[16,17,31,32,33,47,48,49,62,63] dx 1.8e-01; 1:T1[14,15,16,30,31,32,46]T2[16,17,31] dx 1.8e-01; 5:[1,14,15,16] dx 5.7e-02
    g64     n=64  [20,20]                batch 3 ranks [20,20]                short 1 zero 1 nf 0 | 1:T1[44]T2[20] dx 4.5e-03; 8:[20,39,40] dx 4.5e-03; 2: dx 2.4e-02
    g100    n=100 [30,30,30]             batch 3 ranks [30,30,30]             short 1 zero 1 nf 0 | 1:T1[40,41,70]T2[30] dx 9.0e-03; 2: dx 8.4e-01; 3:[29,30] dx 4.3e-02; 4:[29,30] dx 2.2e-02; 5:[29,30] dx 6.0e-03; 6: dx 7.3e-01; 8:[30,59,60,89,90] dx 9.0e-03; 9: dx 1.1e+00
    g130    n=130 [70,40,30]             batch 3 ranks [70,40,20]             short 1 zero 1 nf 0 | 1:T1[20,21,60,130]T2[] dx 1.3e-02; 8:[70,109,110,130] dx 1.3e-02; 3:[20,21,39,40,70] dx 4.9e-02; 5:[20,21,39,40,70] dx 7.1e-03; 6: dx 3.7e-01
    g150    n=150 [50,50,50]             batch 3 ranks [50,50,50]             short 1 zero 1 nf 0 | 1:T1[50,51,100]T2[50] dx 2.0e-01; 2: dx 1.2e+00; 3:[49,50] dx 3.4e-01; 4:[49,50] dx 1.3e-01; 5:[49,50] dx 6.8e-02; 6: dx 1.2e+00; 8:[50,99,100,149,150] dx 2.0e-01; 9: dx 1.4e+00
    g70r    n=70  [30,30,30]             batch 5 ranks [30,30,10]             short 2 zero 2 nf 1 | 1:T1[10,33,34,36,40,46,59,63]T2[7,22,30] dx 1.3e-02; 8:[7,22,30,34,37,56,59,60,64,70] dx 1.3e-02; 3:[7,10,12,19,22,29,30] dx 6.6e-02; 4:[7,10,12,19,22,29,30] dx 3.8e-02
    tall    n=20  [8,300,212]            batch 3 ranks [8,12,0]               short 0 zero 1 nf 0 | 8:[8,20] dx 3.4e-06; 2: dx 3.3e-06
    t7      n=70  [25,25,25]             batch 3 ranks [25,25,20]             short 1 zero 1 nf 1 | 7:T1[18,20,42,45,70]T2[] dx 3.3e-02
    cg_w    n=28  [12,12,12]             batch 3 ranks [12,12,4]              short 1 zero 1 nf 0 | 2: dx 9.2e-02; 6: dx 2.4e-02; 2: x(9)!=x(10) in 3, x(400)==x(401) in 3, x(10)!=x(400) True; 6: x(9)!=x(10) in 3, x(400)==x(401) in 3, x(10)!=x(400) True
    cg_g    n=100 [30,30,30]             batch 3 ranks [30,30,30]             short 1 zero 1 nf 0 | 2: dx 3.5e-01; 6: dx 3.5e-01; 2: x(9)!=x(10) in 3, x(400)==x(401) in 3, x(10)!=x(400) True; 6: x(9)!=x(10) in 3, x(400)==x(401) in 3, x(10)!=x(400) True
    vf_w    n=28  [8,8,8,8]              batch 4 ranks [8,8,8,4]              short 1 zero 2 nf 0 | 1:T1[12,13,20]T2[8] dx 1.5e-03; 3:[8] dx 1.1e-02; 1: ce<eps 8 (largest 7.861) ce>=eps 8 (smallest 8.596) eps 8.2; 3: ce<eps 8 (largest 7.861) ce>=eps 8 (smallest 8.596) eps 8.2
    vf_g    n=100 [30,30,30]             batch 4 ranks [30,30,30]             short 1 zero 2 nf 0 | 1:T1[40,70]T2[30] dx 2.4e-04; 3:[29,30] dx 3.0e-03; 1: ce<eps 6 (largest 18.148) ce>=eps 6 (smallest 23.671) eps 20.0; 3: ce<eps 6 (largest 18.148) ce>=eps 6 (smallest 23.394) eps 20.0
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

SHARE = 160 * 1024 // 8  # wave_reg_lds_share() without LEXLS_REG_LDS_WAVES: the LDS one wavefront's optional pieces may fill
W41, W64 = "lqr_wave<41,12,regularized>", "lqr_wave<64,16,regularized>"
G64, G256, G1024L, G1024H = "lqr_generic<64,lds>", "lqr_generic<256,lds>", "lqr_generic<1024,lds>", "lqr_generic<1024,hbm>"
ALL = (1, 2, 3, 4, 5, 6, 8, 9)  # the eight non-experimental types
LONG_CAP = 400  # a CG cap none of the cases reaches: the loop leaves by sqrt(gamma) <= 1e-12 (condition (c): cap and cap + 1 give the same bits)
PANEL_ORDERS = (16, 17, 32, 33, 48, 49, 63)


def _p41(n):  # four levels of at most 12 rows, n + 1 <= 41: lqr_wave<41,12,regularized>; more rows than variables
    return [(n + 4) // 4 + 1] * 4


def _p64(n):  # n <= 40 reaches lqr_wave<64,16,regularized> through a level of 13 rows, behind three levels that leave it columns
    return [(n - 3) // 3] * 3 + [13]


VF_W_EPS, VF_G_EPS = 8.2, 20.0  # condition (e): between the ce of the cases' levels (7.86 | 8.60 and 18.1 | 23.4: table below)

# name -> n, dims (capacities), batch, seed, types; policy: the kernel policy of the GPU run (None: automatic); per_problem: dims rows dealt round
# the batch; nfixed: fixed variables dealt round the batch; caps: CG iteration caps (default (10,)); var_reg: the variable factor's eps
CASES = {}
for _n in (22, 23, 25, 26, 27, 28, 29, 30):
    CASES[f"p41_{_n}"] = dict(n=_n, dims=_p41(_n), batch=3, seed=20280000 + _n, types=(1, 8, 3, 2))
for _n in (15, 16, 17, 18, 20, 21, 24, 25):
    CASES[f"p64_{_n}"] = dict(n=_n, dims=_p64(_n), batch=3, seed=20280100 + _n, types=(1, 8, 3, 2))
CASES["p41_26"].update(types=ALL)
CASES["p41_27"].update(nfixed=[0, 2, 1])
CASES["p64_20"].update(types=ALL)
CASES.update({
    "window": dict(n=29, dims=[12, 12, 12], batch=5, seed=20280201, types=(1,), nfixed=[0, 0, 1, 0, 3]),
    "panel": dict(n=63, dims=[16, 1, 15, 1, 15, 1, 14], batch=3, seed=20280202, types=(8, 1, 5)),
    "g64": dict(n=64, dims=[20, 20], batch=3, seed=20280203, types=(1, 8, 2)),
    "g100": dict(n=100, dims=[30, 30, 30], batch=3, seed=20280204, types=ALL),
    "g130": dict(n=130, dims=[70, 40, 30], batch=3, seed=20280205, types=(1, 8, 3, 5, 6)),
    "g150": dict(n=150, dims=[50, 50, 50], batch=3, seed=20280206, types=ALL),
    "g70r": dict(n=70, dims=[30, 30, 30], batch=5, seed=20280207, types=(1, 8, 3, 4), nfixed=[0, 4, 0, 11, 2],
                 per_problem=np.array([[30, 30, 30], [30, 0, 30], [7, 30, 19], [30, 30, 0], [22, 13, 30]], np.uint32)),
    "tall": dict(n=20, dims=[8, 300, 212], batch=3, seed=20280208, types=(8, 2)),
    "t7": dict(n=70, dims=[25, 25, 25], batch=3, seed=20280209, types=(7,), nfixed=[0, 3, 0]),
    "cg_w": dict(n=28, dims=[12, 12, 12], batch=3, seed=20280210, types=(2, 6), caps=(1, 10, LONG_CAP)),
    "cg_g": dict(n=100, dims=[30, 30, 30], batch=3, seed=20280211, types=(2, 6), caps=(1, 10, LONG_CAP)),
    "vf_w": dict(n=28, dims=[8, 8, 8, 8], batch=4, seed=20280212, types=(1, 3), var_reg=VF_W_EPS),
    "vf_g": dict(n=100, dims=[30, 30, 30], batch=4, seed=20280213, types=(1, 3), var_reg=VF_G_EPS),
})
CG_CPU_CAPS = (9, 10, LONG_CAP, LONG_CAP + 1)  # condition (c), oracle only

# (case, type) -> (kernel under automatic dispatch, order of the LDS window of the work matrix, null-space basis in LDS): the output of
# tests/reg_plan_check.cpp (tests/test_reg_cases.py holds the two equal); what last_kernel() and last_reg_placement() must answer on the GPU
PLAN = {
    "p41_22": {1: (W41, 22, 1), 8: (W41, 22, 1), 3: (W41, 12, 1), 2: (W41, 0, 1)},
    "p41_23": {1: (W41, 23, 0), 8: (W41, 23, 0), 3: (W41, 12, 1), 2: (W41, 0, 1)},
    "p41_25": {1: (W41, 25, 0), 8: (W41, 25, 0), 3: (W41, 12, 1), 2: (W41, 0, 1)},
    "p41_26": {1: (W41, 26, 0), 2: (W41, 0, 0), 3: (W41, 12, 1), 4: (W41, 12, 0), 5: (W41, 12, 0), 6: (W41, 0, 0), 8: (W41, 26, 0), 9: (W41, 0, 0)},
    "p41_27": {1: (W41, 26, 0), 8: (W41, 27, 0), 3: (W41, 12, 0), 2: (W41, 0, 0)},
    "p41_28": {1: (W41, 27, 0), 8: (W41, 28, 0), 3: (W41, 12, 0), 2: (W41, 0, 0)},
    "p41_29": {1: (W41, 27, 0), 8: (W41, 0, 0), 3: (W41, 12, 0), 2: (W41, 0, 0)},
    "p41_30": {1: (W41, 0, 0), 8: (W41, 0, 0), 3: (W41, 12, 0), 2: (W41, 0, 0)},
    "p64_15": {1: (W64, 15, 1), 8: (W64, 15, 1), 3: (W64, 16, 1), 2: (W64, 0, 1)},
    "p64_16": {1: (W64, 16, 0), 8: (W64, 16, 0), 3: (W64, 16, 0), 2: (W64, 0, 1)},
    "p64_17": {1: (W64, 17, 0), 8: (W64, 17, 0), 3: (W64, 16, 0), 2: (W64, 0, 1)},
    "p64_18": {1: (W64, 18, 0), 8: (W64, 18, 0), 3: (W64, 16, 0), 2: (W64, 0, 0)},
    "p64_20": {1: (W64, 20, 0), 2: (W64, 0, 0), 3: (W64, 16, 0), 4: (W64, 16, 0), 5: (W64, 16, 0), 6: (W64, 0, 0), 8: (W64, 20, 0), 9: (W64, 0, 0)},
    "p64_21": {1: (W64, 0, 0), 8: (W64, 0, 0), 3: (W64, 16, 0), 2: (W64, 0, 0)},
    "p64_24": {1: (W64, 0, 0), 8: (W64, 0, 0), 3: (W64, 16, 0), 2: (W64, 0, 0)},
    "p64_25": {1: (W64, 0, 0), 8: (W64, 0, 0), 3: (W64, 0, 0), 2: (W64, 0, 0)},
    "window": {1: (W41, 27, 0)},
    "panel": {8: (W64, 0, 0), 1: (W64, 0, 0), 5: (W64, 0, 0)},
    "g64": {1: (G256, 0, 0), 8: (G256, 0, 0), 2: (G256, 0, 0)},
    "g100": {1: (G256, 0, 0), 2: (G256, 0, 0), 3: (G256, 0, 0), 4: (G256, 0, 0), 5: (G256, 0, 0), 6: (G256, 0, 0), 8: (G256, 0, 0), 9: (G256, 0, 0)},
    "g130": {1: (G256, 0, 0), 8: (G256, 0, 0), 3: (G256, 0, 0), 5: (G256, 0, 0), 6: (G256, 0, 0)},
    "g150": {1: (G1024H, 0, 0), 2: (G1024H, 0, 0), 3: (G1024H, 0, 0), 4: (G1024H, 0, 0), 5: (G1024H, 0, 0), 6: (G1024H, 0, 0), 8: (G1024H, 0, 0), 9: (G1024H, 0, 0)},
    "g70r": {1: (G256, 0, 0), 8: (G256, 0, 0), 3: (G256, 0, 0), 4: (G256, 0, 0)},
    "tall": {8: (G1024L, 0, 0), 2: (G1024L, 0, 0)},
    "t7": {7: (G256, 0, 0)},
    "cg_w": {2: (W41, 0, 0), 6: (W41, 0, 0)},
    "cg_g": {2: (G256, 0, 0), 6: (G256, 0, 0)},
    "vf_w": {1: (W41, 27, 0), 3: (W41, 12, 0)},
    "vf_g": {1: (G256, 0, 0), 3: (G256, 0, 0)},
}
WAVE_CASES = tuple(nm for nm, p in PLAN.items() if next(iter(p.values()))[0] in (W41, W64))
POLICY_1 = G64  # what every wave case takes under kernel policy 1: the generic kernel of one wavefront, where spd_solve_wave runs again

# the flips of the placement (DOCSTRING, switch 1): (type, what flips, case on the LDS side, case on the other side)
FLIPS = (
    (1, "basis", "p41_22", "p41_23"), (8, "basis", "p41_22", "p41_23"), (3, "basis", "p41_26", "p41_27"), (2, "basis", "p41_25", "p41_26"),
    (8, "window", "p41_28", "p41_29"), (1, "window", "p41_29", "p41_30"),
    (1, "basis", "p64_15", "p64_16"), (8, "basis", "p64_15", "p64_16"), (3, "basis", "p64_15", "p64_16"), (2, "basis", "p64_17", "p64_18"),
    (1, "window", "p64_20", "p64_21"), (8, "window", "p64_20", "p64_21"), (3, "window", "p64_24", "p64_25"),
)


def plan_line(name, reg_type, policy=0):
    """the case as tests/reg_plan_check.cpp reads it: what the handle's query holds for it (lexls_capi.hip, query_of)"""
    c = CASES[name]
    dims = _dims(c)
    fixed = int(any(c.get("nfixed") or [0]))
    uniform = int(dims.max()) if dims.min() == dims.max() else 0
    vals = [c["batch"], c["n"], len(c["dims"]), sum(c["dims"]), uniform, int(dims.sum(axis=1).max()), int(dims.max()), fixed, reg_type, policy, SHARE]
    return f"{name}:{reg_type}:{policy} " + " ".join(str(int(v)) for v in vals)


def _dims(c):
    B = c["batch"]
    if c.get("per_problem") is not None:
        return c["per_problem"][np.arange(B) % len(c["per_problem"])].copy()
    return np.tile(np.asarray(c["dims"], np.uint32), (B, 1))


def draw(name):
    """the inputs of a case: dict(n, caps, lod, dims (batch, nObj), fac (batch, nObj), fixed (keyword arguments of oracle.lse_run, {} without
    fixed variables)).  Every problem b with b % 3 == 1 has a duplicated row (right-hand side included) in its first level of two rows or more
    behind level 0; every odd problem b has the factor of level (b - 1) / 2 exactly 0.0; problem 0 has neither."""
    c = CASES[name]
    n, caps, seed, B = c["n"], list(c["dims"]), c["seed"], c["batch"]
    nobj = len(caps)
    lod = P.lse_batch(seed, B, n, caps)
    dims = _dims(c)
    dup = {}  # problem -> the level with the duplicated row
    for b in range(B):
        m, first = int(dims[b].sum()), np.concatenate([[0], np.cumsum(dims[b])]).astype(int)
        lod[b, :, m:] = np.nan  # a problem's rows packed level after level; NaN behind them (never read)
        if b % 3 == 1:
            k = dup[b] = next(k for k in list(range(1, nobj)) + [0] if dims[b, k] >= 2)
            lod[b, :, first[k] + 1] = lod[b, :, first[k]]
    fac = np.abs(P.normal(seed + 1, B * nobj)).reshape(B, nobj) * 0.3 + 0.05
    for b in range(1, B, 2):
        fac[b, ((b - 1) // 2) % nobj] = 0.0
    fixed = {}
    if c.get("nfixed") is not None:
        nfixed = np.asarray(c["nfixed"], np.uint32)[np.arange(B) % len(c["nfixed"])]
        idx, val = np.zeros((B, n), np.uint32), np.zeros((B, n))
        for b in range(B):
            nf = int(nfixed[b])
            idx[b, :nf] = np.argsort(P.uniform(seed + 300000 + b, n))[:nf]
            val[b, :nf] = P.normal(seed + 400000 + b, n)[:nf]
        fixed = dict(nfixed=nfixed, fixed_idx=idx, fixed_val=val)
    return dict(name=name, n=n, caps=caps, lod=lod, dims=dims, fac=fac, fixed=fixed, dup=dup, types=tuple(c["types"]),
                cg_caps=tuple(c.get("caps", (10,))), var_reg=float(c.get("var_reg", 0.0)))


KEYS = ("x", "factor", "hh", "perm", "rank", "fcol", "totalrank")


def oracle_run(case, reg_type, cap=10, fac=None, problems=None):
    """the oracle on the case, problem by problem (its binding takes one factor vector per call), stacked"""
    n, lod, dims, fixed = case["n"], case["lod"], case["dims"], case["fixed"]
    fac = case["fac"] if fac is None else fac
    out = {}
    for b in (range(lod.shape[0]) if problems is None else problems):
        kw = {k: v[b:b + 1] for k, v in fixed.items()}
        r = oracle.lse_run(lod[b:b + 1], dims[b:b + 1], n, maxdim=np.asarray(case["caps"], np.uint32), reg_type=reg_type, reg_factors=fac[b],
                           var_reg=case["var_reg"] if reg_type else 0.0, cg_iters=cap, **kw)
        for k in KEYS + (("x_mu", "residual_mu") if reg_type == 7 else ()):
            out.setdefault(k, []).append(r[k][0])
    return {k: np.stack(v) for k, v in out.items()}


def level_orders(case, ref, reg_type):
    """per (problem, ranked level): (problem, level, order of the normal equations reg_cholesky_solve factorizes (0: none), Tikhonov branch
    (1 / 2, 0: not a Tikhonov type)) from the oracle's ranks and first columns, as regularize_level decides (lexls_regularize.h); levels whose
    factor is 0.0 are left out (nonzero == false: no routine runs)"""
    n, out = case["n"], []
    nfixed = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(len(case["lod"]), np.uint32)
    for b in range(len(case["lod"])):
        for k in range(len(case["caps"])):
            Fc, rank, nf = int(ref["fcol"][b, k]), int(ref["rank"][b, k]), int(nfixed[b])
            if rank == 0 or case["fac"][b, k] == 0.0:
                continue
            RC = n - Fc - rank
            if reg_type in (1, 7):
                branch = 2 if (reg_type == 1 and Fc + rank <= RC) else 1
                out.append((b, k, Fc - nf + rank if branch == 2 else RC + rank, branch))
            elif reg_type == 8:
                out.append((b, k, Fc - nf + rank, 2))
            elif reg_type in (3, 4, 5):
                out.append((b, k, rank, 0))
            else:
                out.append((b, k, 0, 0))
    return out


def conditioning(case, reg_type):
    """(e): ce = |y|^2 / |R^-1 y|^2 of every ranked level as regularize_level forms it, y = the level's transformed right-hand side BEFORE its own
    damping: read from the factor of a run whose factors are 0.0 from that level on (the levels above are damped as in the case's run, the
    level itself is not).  list of (problem, level, ce)"""
    n, out = case["n"], []
    full = case["ref"][(reg_type, 10)]
    for k in range(len(case["caps"])):
        fac = case["fac"].copy()
        fac[:, k:] = 0.0
        r = oracle_run(case, reg_type, fac=fac)
        for b in range(len(case["lod"])):
            rank, Fc = int(full["rank"][b, k]), int(full["fcol"][b, k])
            if rank == 0:
                continue
            F = int(case["dims"][b, :k].sum())
            R = np.triu(r["factor"][b, Fc:Fc + rank, F:F + rank].T)
            assert np.array_equal(R, np.triu(full["factor"][b, Fc:Fc + rank, F:F + rank].T))  # the damping touches right-hand sides only
            y = r["factor"][b, n, F:F + rank]
            z = np.linalg.solve(R, y)
            out.append((b, k, float(y @ y) / float(z @ z)))
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """the case `name`: its inputs (draw), plain = the oracle without regularization, ref[(type, cap)] = the oracle's results for everything the GPU
    test compares (x, factor, hh, perm, rank, fcol, totalrank; type 7: x_mu, residual_mu), orders[type] = level_orders"""
    case = draw(name)
    case["plain"] = oracle_run(case, 0)
    case["ref"] = {(t, cap): oracle_run(case, t, cap) for t in case["types"] for cap in (case["cg_caps"] if t in (2, 6) else (10,))}
    case["orders"] = {t: level_orders(case, case["ref"][(t, 10)], t) for t in case["types"]}
    if len(case["cg_caps"]) > 1:  # condition (c)
        case["cg_x"] = {(t, cap): oracle_run(case, t, cap)["x"] for t in case["types"] for cap in CG_CPU_CAPS}
    if case["var_reg"]:  # condition (e)
        case["ce"] = {t: conditioning(case, t) for t in case["types"]}
        for t in case["types"]:  # a level with ce >= eps gets the factor 0: no routine runs
            damped = {(b, k) for b, k, ce in case["ce"][t] if ce < case["var_reg"]}
            case["orders"][t] = [o for o in case["orders"][t] if (o[0], o[1]) in damped]
    r = case["plain"]
    case["short"] = sorted(b for b, k in case["dup"].items() if r["rank"][b, k] < min(int(case["dims"][b, k]), case["n"] - int(r["fcol"][b, k])))
    arrays = [case[k] for k in ("lod", "dims", "fac")] + list(case["fixed"].values()) + [a for r in [case["plain"]] + list(case["ref"].values()) for a in r.values()]
    for a in arrays:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


def summary(case):
    """one line per case: shape, types, then per type the orders of the ranked, damped levels (T1 / T2: by Tikhonov branch) and the largest
    entry the regularization moves x by (smallest over the problems)"""
    c, parts = CASES[case["name"]], []
    for t in case["types"]:
        ref = case["ref"][(t, 10)]
        moved = np.abs(ref["x"] - case["plain"]["x"]).max(axis=1).min()
        o = case["orders"][t]
        if t in (1, 7):
            txt = "T1" + str(sorted({N for _, _, N, br in o if br == 1})) + " T2" + str(sorted({N for _, _, N, br in o if br == 2}))
        elif t in (8, 3, 4, 5):
            txt = str(sorted({N for _, _, N, _ in o}))
        else:
            txt = ""
        parts.append(f"{t}:{txt.replace(' ', '')} dx {moved:.1e}")
    for t in case["types"] if "cg_x" in case else ():
        x = case["cg_x"]
        capped = sum(bool((x[(t, 9)][b] != x[(t, 10)][b]).any()) for b in range(len(case["lod"])))
        same = sum(bool((x[(t, LONG_CAP)][b] == x[(t, LONG_CAP + 1)][b]).all()) for b in range(len(case["lod"])))
        parts.append(f"{t}: x(9)!=x(10) in {capped}, x({LONG_CAP})==x({LONG_CAP + 1}) in {same}, x(10)!=x({LONG_CAP}) {bool((x[(t, 10)] != x[(t, LONG_CAP)]).any())}")
    for t in case["types"] if "ce" in case else ():
        ce, eps = sorted(v for _, _, v in case["ce"][t]), case["var_reg"]
        below = [v for v in ce if v < eps]
        parts.append(f"{t}: ce<eps {len(below)} (largest {below[-1]:.3f}) ce>=eps {len(ce) - len(below)} (smallest {ce[len(below)]:.3f}) eps {eps}")
    deficient = len(case["short"])
    zeros = int((case["fac"] == 0.0).sum())
    head = (f"    {case['name']:<7} n={case['n']:<3} {str(case['caps']).replace(' ', ''):<22} batch {len(case['lod'])} "
            f"ranks {str(case['plain']['rank'][0].tolist()).replace(' ', ''):<22} short {deficient} zero {zeros} nf {int(any(c.get('nfixed') or [0]))}")
    return head + " | " + "; ".join(parts)


if __name__ == "__main__":
    for nm in CASES:
        print(summary(build(nm)))
