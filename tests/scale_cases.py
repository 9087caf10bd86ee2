"""Batches that hold every LexLSE factorization kernel family to the oracle on data IN OTHER UNITS: entries that are not of order 1
(tests/test_gpu_scale.py runs them on the GPU, tests/test_scale_cases.py asserts the conditions below on the CPU, from the oracle and the planner
alone).  Every other batch of the suite is unit-variance Gaussian data or a transform that leaves the magnitudes near 1, so the hand-written
reciprocals, reciprocal square roots, packed pivot keys, the guard's ratio and anything a kernel might keep in `float` only ever see numbers
near 1.  An inverse-kinematics hierarchy mixes metres, millimetres, radians and torques between levels and between columns, and the rank
tolerance is an absolute number on a squared norm, so callers rescale whole problems to suit it.  Nothing here comes near overflow, underflow or
subnormal numbers: those are outside every stated contract.

Generators (pure functions of a seed; slot b of a case from seed + b, an unkept slot redrawn from seed + b + 100, ...; slots 1 and 12 hold
P.rank_deficient_problem where the levels are uniform and no variable is fixed, as skip_cases.DEFICIENT):
    pow2     the base problems [A | b] times 2^k, one k per run, k in POW2_K, under the rank tolerance ldexp(1e-12, 2 k): squared norms reach
             2^+-200 = 1e+-60, far inside double and far outside float.  The oracle's x, ranks, first columns and permutation do not change by a
             bit (no fixed variables; with fixed variables the values stay in the old units, so the expectation is the oracle on the same data).
             Tolerance-contract cases (T, L) draw base problems that are STABLE in the sense of tests/rank_cases.py.
    levels   level j of problem b, right-hand side included, times 2^e, e drawn per problem and level from the seed in [-10, 10] (units up to
             1e+-3), tolerance 1e-12.  A problem is kept when the oracle's ranks and first columns equal those of the unscaled problem and are
             the same at tol / 10 and 10 tol; then the oracle's x is bit-identical to the unscaled problem's.
    decades  the base problems with columns times 10^U(-3, 3) and rows times 10^U(-2, 2), each problem its own scales: the distribution of
             P.badly_scaled_batch per slot, on the case's own dimensions and fixed variables.  Tolerance-contract cases keep the stable
             problems only and carry the one-ulp sensitivity of x (+-1.1e-16 relative on the data, three draws, the oracle alone).

Cases: skip_cases.CASES (imported) without wave_reg (damping factors are absolute; tests/reg_cases.py owns that family) and mfma_one_n44
(mfma_one's instantiation); batch 19, the n = 100 shape 3.  Every case keeps at least skip_cases.RETENTION of what it drew.

Consumers of a kept factor (skip_cases.CONSUMER_CASES on decades): gap = the largest discrepancy between the two CPU references of each family
on these data, in that family's own norm (adjoint_cases._rel per problem and cotangent; per problem for the matrix gradient; per problem and
direction for the tangents; solve_rhs_cases.rel_rows).  tests/test_gpu_scale.py allows the device 10 x the largest gap of the family
(CONSUMER_TOL), the project's rule; the unit-scale TOLs of those modules are not reused.

MEASURED (`python tests/scale_cases.py`; oracle alone; sens = the largest one-ulp sensitivity of x relative to max(1, |x|_inf), tolerance-contract
cases; est = smallest .. largest accuracy-guard estimate computed from the oracle's factor, qtol_guard only):
    qtol_ik-pow2-100       n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7>               kept 19 / 19  max|x| 2.8e+01  sens 6.0e-14
    qtol_ik-pow2+100       n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7>               kept 19 / 19  max|x| 2.8e+01  sens 6.0e-14
    qtol_ik-levels         n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7>               kept 19 / 19  max|x| 2.7e+01  sens 6.3e-14
    qtol_ik-decades        n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7>               kept 19 / 19  max|x| 1.1e+04  sens 4.4e-11
    qtol_8-pow2-100        n=40  [8,8,8,8,8]         lqr_qtol<3,8>                        kept 19 / 19  max|x| 2.2e+02  sens 9.9e-13
    qtol_8-pow2+100        n=40  [8,8,8,8,8]         lqr_qtol<3,8>                        kept 19 / 19  max|x| 2.2e+02  sens 9.9e-13
    qtol_8-levels          n=40  [8,8,8,8,8]         lqr_qtol<3,8>                        kept 19 / 19  max|x| 7.2e+01  sens 1.2e-13
    qtol_8-decades         n=40  [8,8,8,8,8]         lqr_qtol<3,8>                        kept 19 / 20  max|x| 2.4e+04  sens 3.0e-11
    qtol_n24-pow2-100      n=24  [12,12,12,12,12]    lqr_qtol<2,12>                       kept 19 / 19  max|x| 2.7e+03  sens 1.4e-12
    qtol_n24-pow2+100      n=24  [12,12,12,12,12]    lqr_qtol<2,12>                       kept 19 / 19  max|x| 2.7e+03  sens 1.4e-12
    qtol_n24-levels        n=24  [12,12,12,12,12]    lqr_qtol<2,12>                       kept 19 / 19  max|x| 2.4e+02  sens 4.2e-13
    qtol_n24-decades       n=24  [12,12,12,12,12]    lqr_qtol<2,12>                       kept 19 / 19  max|x| 2.1e+04  sens 5.1e-12
    qtol_ragged-pow2-100   n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,ragged>        kept 19 / 19  max|x| 4.1e+00  sens 6.7e-15
    qtol_ragged-pow2+100   n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,ragged>        kept 19 / 19  max|x| 4.1e+00  sens 6.7e-15
    qtol_ragged-levels     n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,ragged>        kept 19 / 19  max|x| 2.2e+00  sens 5.1e-15
    qtol_ragged-decades    n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,ragged>        kept 19 / 19  max|x| 1.3e+04  sens 2.4e-11
    qtol_guard-pow2-100    n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,guard>         kept 19 / 19  max|x| 1.9e+01  sens 3.5e-14
    qtol_guard-pow2+100    n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,guard>         kept 19 / 19  max|x| 1.9e+01  sens 3.5e-14
    qtol_guard-levels      n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,guard>         kept 19 / 19  max|x| 1.0e+01  sens 3.3e-14
    qtol_guard-decades     n=40  [12,12,12,12,12]    lqr_qtol<3,12,shift 7,guard>         kept 19 / 19  max|x| 2.4e+04  sens 2.5e-09  est 225 .. 3.04e+04
    mfma_two-pow2-100      n=40  [12,12,12,12,12]    lqr_mfma<32,12,n40>                  kept 19 / 19  max|x| 1.9e+01  sens 2.5e-13
    mfma_two-pow2+100      n=40  [12,12,12,12,12]    lqr_mfma<32,12,n40>                  kept 19 / 19  max|x| 1.9e+01  sens 2.5e-13
    mfma_two-levels        n=40  [12,12,12,12,12]    lqr_mfma<32,12,n40>                  kept 19 / 19  max|x| 4.5e+02  sens 6.9e-13
    mfma_two-decades       n=40  [12,12,12,12,12]    lqr_mfma<32,12,n40>                  kept 19 / 19  max|x| 2.7e+04  sens 8.8e-12
    mfma_one-pow2-100      n=40  [12,12,12,12,12]    lqr_mfma<64,12>                      kept 19 / 19  max|x| 7.9e+01  sens 3.2e-13
    mfma_one-pow2+100      n=40  [12,12,12,12,12]    lqr_mfma<64,12>                      kept 19 / 19  max|x| 7.9e+01  sens 3.2e-13
    mfma_one-levels        n=40  [12,12,12,12,12]    lqr_mfma<64,12>                      kept 19 / 19  max|x| 1.2e+01  sens 2.1e-13
    mfma_one-decades       n=40  [12,12,12,12,12]    lqr_mfma<64,12>                      kept 19 / 19  max|x| 8.8e+05  sens 1.5e-09
    mfma_four-pow2-100     n=40  [12,12,12,12,12]    lqr_mfma<16,12,n40>                  kept 19 / 19  max|x| 6.6e+00  sens 1.9e-14
    mfma_four-pow2+100     n=40  [12,12,12,12,12]    lqr_mfma<16,12,n40>                  kept 19 / 19  max|x| 6.6e+00  sens 1.9e-14
    mfma_four-levels       n=40  [12,12,12,12,12]    lqr_mfma<16,12,n40>                  kept 19 / 19  max|x| 7.5e+01  sens 5.9e-13
    mfma_four-decades      n=40  [12,12,12,12,12]    lqr_mfma<16,12,n40>                  kept 19 / 19  max|x| 7.8e+03  sens 1.1e-10
    mfma_two_n44-pow2-100  n=44  [12,12]             lqr_mfma<32,12>                      kept 19 / 19  max|x| 2.2e+00  sens 1.0e-14
    mfma_two_n44-pow2+100  n=44  [12,12]             lqr_mfma<32,12>                      kept 19 / 19  max|x| 2.2e+00  sens 1.0e-14
    mfma_two_n44-levels    n=44  [12,12]             lqr_mfma<32,12>                      kept 19 / 19  max|x| 2.4e+00  sens 1.9e-15
    mfma_two_n44-decades   n=44  [12,12]             lqr_mfma<32,12>                      kept 19 / 19  max|x| 2.3e+01  sens 2.9e-12
    quad_ik_x-pow2-100     n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7>               kept 19 / 19  max|x| 4.8e+00
    quad_ik_x-pow2+100     n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7>               kept 19 / 19  max|x| 4.8e+00
    quad_ik_x-levels       n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7>               kept 19 / 19  max|x| 6.4e+01
    quad_ik_x-decades      n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7>               kept 19 / 19  max|x| 1.6e+05
    quad_ik_f-pow2-100     n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor>        kept 19 / 19  max|x| 5.4e+00
    quad_ik_f-pow2+100     n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor>        kept 19 / 19  max|x| 5.4e+00
    quad_ik_f-levels       n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor>        kept 19 / 19  max|x| 4.0e+00
    quad_ik_f-decades      n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor>        kept 19 / 19  max|x| 1.8e+04
    quad_wide_x-pow2-100   n=47  [14,9,16,8]         lqr_quad<4,16>                       kept 19 / 19  max|x| 2.5e+01
    quad_wide_x-pow2+100   n=47  [14,9,16,8]         lqr_quad<4,16>                       kept 19 / 19  max|x| 2.5e+01
    quad_wide_x-levels     n=47  [14,9,16,8]         lqr_quad<4,16>                       kept 19 / 19  max|x| 9.1e+01
    quad_wide_x-decades    n=47  [14,9,16,8]         lqr_quad<4,16>                       kept 19 / 19  max|x| 2.4e+04
    quad_wide_f-pow2-100   n=47  [14,9,16,8]         lqr_quad<4,16,factor>                kept 19 / 19  max|x| 4.5e+02
    quad_wide_f-pow2+100   n=47  [14,9,16,8]         lqr_quad<4,16,factor>                kept 19 / 19  max|x| 4.5e+02
    quad_wide_f-levels     n=47  [14,9,16,8]         lqr_quad<4,16,factor>                kept 19 / 19  max|x| 5.0e+01
    quad_wide_f-decades    n=47  [14,9,16,8]         lqr_quad<4,16,factor>                kept 19 / 19  max|x| 2.3e+04
    quad_fixed_x-pow2-100  n=47  [14,9,16,8]         lqr_quad<4,16,fixed>                 kept 19 / 19  max|x| 1.5e+01
    quad_fixed_x-pow2+100  n=47  [14,9,16,8]         lqr_quad<4,16,fixed>                 kept 19 / 19  max|x| 1.5e+01
    quad_fixed_x-levels    n=47  [14,9,16,8]         lqr_quad<4,16,fixed>                 kept 19 / 19  max|x| 1.1e+01
    quad_fixed_x-decades   n=47  [14,9,16,8]         lqr_quad<4,16,fixed>                 kept 19 / 19  max|x| 1.6e+06
    quad_fixed_f-pow2-100  n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor,fixed>  kept 19 / 19  max|x| 2.6e+01
    quad_fixed_f-pow2+100  n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor,fixed>  kept 19 / 19  max|x| 2.6e+01
    quad_fixed_f-levels    n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor,fixed>  kept 19 / 19  max|x| 1.0e+01
    quad_fixed_f-decades   n=40  [12,12,12,12,12]    lqr_quad<3,12,shift 7,factor,fixed>  kept 19 / 19  max|x| 7.9e+05
    lwave_f-pow2-100       n=40  [12,12,12,12,12]    lqr_lwave<41,12,exact>               kept 19 / 19  max|x| 6.5e+00
    lwave_f-pow2+100       n=40  [12,12,12,12,12]    lqr_lwave<41,12,exact>               kept 19 / 19  max|x| 6.5e+00
    lwave_f-levels         n=40  [12,12,12,12,12]    lqr_lwave<41,12,exact>               kept 19 / 19  max|x| 2.1e+01
    lwave_f-decades        n=40  [12,12,12,12,12]    lqr_lwave<41,12,exact>               kept 19 / 19  max|x| 6.2e+04
    lwave_x-pow2-100       n=31  [12,12,12]          lqr_lwave<41,12>                     kept 19 / 19  max|x| 8.8e+00
    lwave_x-pow2+100       n=31  [12,12,12]          lqr_lwave<41,12>                     kept 19 / 19  max|x| 8.8e+00
    lwave_x-levels         n=31  [12,12,12]          lqr_lwave<41,12>                     kept 19 / 19  max|x| 8.3e+00
    lwave_x-decades        n=31  [12,12,12]          lqr_lwave<41,12>                     kept 19 / 19  max|x| 7.3e+03
    wave_exact-pow2-100    n=40  [12,12,12,12,12]    lqr_wave<41,12,exact>                kept 19 / 19  max|x| 3.4e+02
    wave_exact-pow2+100    n=40  [12,12,12,12,12]    lqr_wave<41,12,exact>                kept 19 / 19  max|x| 3.4e+02
    wave_exact-levels      n=40  [12,12,12,12,12]    lqr_wave<41,12,exact>                kept 19 / 19  max|x| 4.1e+00
    wave_exact-decades     n=40  [12,12,12,12,12]    lqr_wave<41,12,exact>                kept 19 / 19  max|x| 3.8e+04
    wave_n31-pow2-100      n=31  [12,12,12]          lqr_wave<41,12>                      kept 19 / 19  max|x| 3.7e+00
    wave_n31-pow2+100      n=31  [12,12,12]          lqr_wave<41,12>                      kept 19 / 19  max|x| 3.7e+00
    wave_n31-levels        n=31  [12,12,12]          lqr_wave<41,12>                      kept 19 / 19  max|x| 2.4e+01
    wave_n31-decades       n=31  [12,12,12]          lqr_wave<41,12>                      kept 19 / 19  max|x| 2.6e+03
    wave_64-pow2-100       n=47  [14,9,16,8]         lqr_wave<64,16>                      kept 19 / 19  max|x| 6.1e+01
    wave_64-pow2+100       n=47  [14,9,16,8]         lqr_wave<64,16>                      kept 19 / 19  max|x| 6.1e+01
    wave_64-levels         n=47  [14,9,16,8]         lqr_wave<64,16>                      kept 19 / 19  max|x| 3.1e+01
    wave_64-decades        n=47  [14,9,16,8]         lqr_wave<64,16>                      kept 19 / 19  max|x| 1.0e+04
    generic_64-pow2-100    n=40  [12,12,12,12,12]    lqr_generic<64,lds>                  kept 19 / 19  max|x| 3.2e+01
    generic_64-pow2+100    n=40  [12,12,12,12,12]    lqr_generic<64,lds>                  kept 19 / 19  max|x| 3.2e+01
    generic_64-levels      n=40  [12,12,12,12,12]    lqr_generic<64,lds>                  kept 19 / 19  max|x| 6.0e+00
    generic_64-decades     n=40  [12,12,12,12,12]    lqr_generic<64,lds>                  kept 19 / 19  max|x| 1.5e+04
    generic_256-pow2-100   n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 kept 19 / 19  max|x| 3.4e+01
    generic_256-pow2+100   n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 kept 19 / 19  max|x| 3.4e+01
    generic_256-levels     n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 kept 19 / 19  max|x| 1.8e+01
    generic_256-decades    n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 kept 19 / 19  max|x| 3.1e+03
    generic_hbm-pow2-100   n=100 [115,115]           lqr_generic<1024,hbm>                kept  3 / 3   max|x| 1.1e+00
    generic_hbm-pow2+100   n=100 [115,115]           lqr_generic<1024,hbm>                kept  3 / 3   max|x| 1.1e+00
    generic_hbm-levels     n=100 [115,115]           lqr_generic<1024,hbm>                kept  3 / 3   max|x| 9.0e-01
    generic_hbm-decades    n=100 [115,115]           lqr_generic<1024,hbm>                kept  3 / 3   max|x| 4.8e+02
    large_multi-pow2-100   n=100 [115,115]           lqr_large<multi-launch>              kept  3 / 3   max|x| 6.2e-01
    large_multi-pow2+100   n=100 [115,115]           lqr_large<multi-launch>              kept  3 / 3   max|x| 6.2e-01
    large_multi-levels     n=100 [115,115]           lqr_large<multi-launch>              kept  3 / 3   max|x| 7.2e-01
    large_multi-decades    n=100 [115,115]           lqr_large<multi-launch>              kept  3 / 3   max|x| 6.6e+02
    large_fast-pow2-100    n=100 [115,115]           lqr_large<step-per-pivot,mfma>       kept  3 / 3   max|x| 1.0e+00  sens 2.7e-15
    large_fast-pow2+100    n=100 [115,115]           lqr_large<step-per-pivot,mfma>       kept  3 / 3   max|x| 1.0e+00  sens 2.7e-15
    large_fast-levels      n=100 [115,115]           lqr_large<step-per-pivot,mfma>       kept  3 / 3   max|x| 8.9e-01  sens 2.3e-15
    large_fast-decades     n=100 [115,115]           lqr_large<step-per-pivot,mfma>       kept  3 / 3   max|x| 2.8e+02  sens 5.1e-13
    wave_exact consumers   decades  rank-stable 17 / 19  gap adjoint 6.7e-13  adjoint_matrix 1.5e-08  tangent 1.7e-08  solve_rhs 5.1e-12
    quad_ik_f consumers    decades  rank-stable 17 / 19  gap adjoint 1.9e-12  adjoint_matrix 7.4e-10  tangent 3.2e-09  solve_rhs 9.5e-12
    generic_64 consumers   decades  rank-stable 17 / 19  gap adjoint 6.0e-12  adjoint_matrix 2.2e-09  tangent 1.5e-09  solve_rhs 8.9e-12
    consumer D_CPU (largest gap, rounded up): adjoint 6.1e-12, adjoint_matrix 1.55e-8, tangent 1.73e-8, solve_rhs 9.5e-12 -> device tolerance 10 x each.
    LexLSI: seed 20349000, iterations / activations / deactivations of the oracle driver 85/59/25, 116/73/42, 102/66/35, 68/48/19, 77/54/22, 68/49/18.
MEASURED on MI355X (tests/test_gpu_scale.py prints every figure; that module's text has the table per generator):
    largest |x - x_oracle| per family: lqr_qtol 1.1e-05 (qtol_guard / decades at |x|_inf 2.4e4: 1.8e-09 relative), lqr_mfma 4.7e-05 (mfma_one / decades
    at |x|_inf 8.8e5: 5.4e-11 relative), lqr_large<step-per-pivot,mfma> 1.2e-12 relative, every bit-exact family 0.
    largest multiple of the one-ulp sensitivity on decades: lqr_qtol 15.9 (qtol_n24), lqr_mfma 9.67 (mfma_two), lqr_large<step-per-pivot,mfma> 3.73;
    allowed 100.  Every tolerance-contract kernel kept the power-of-two invariance bit for bit at k = -100 and k = +100.
    consumers on decades against reference (A): adjoint 2.7e-11, adjoint_matrix 1.55e-8, tangent 1.72e-8, solve_rhs 3.4e-16.
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

import skip_cases as S  # noqa: E402
from lexls_amd import problems as P  # noqa: E402

GENERATORS = ("pow2", "levels", "decades")
POW2_K = (-100, 100)
NAMES = [nm for nm in S.CASES if nm not in ("wave_reg", "mfma_one_n44")]
BATCH, LARGE_BATCH = S.BATCH, 3
SEED = 20340000
TOL = S.TOL_DEFAULT
LEVEL_RANGE = 10      # exponents of `levels` in [-LEVEL_RANGE, LEVEL_RANGE]
LEVEL_RANGE_OF = {}   # name -> a narrower range, for a shape that cannot keep skip_cases.RETENTION under the full one (none needed)
ATTEMPTS = 12
K_COT = 3             # cotangents, tangent directions and right-hand sides per problem of the consumer cases


def runs(generators=GENERATORS):
    """(name, generator, k): pow2 at both k, the other generators once (k = 0)"""
    return [(nm, g, k) for nm in NAMES for g in generators for k in (POW2_K if g == "pow2" else (0,))]


def run_id(nm, g, k):
    return f"{nm}-{g}" + (f"{k:+d}" if g == "pow2" else "")


def batch_of(c):
    return LARGE_BATCH if c["n"] == 100 else BATCH


def uniform(c):
    return c.get("per_problem") is None and c.get("nfixed") is None


def tolerance(k):
    return float(np.ldexp(TOL, 2 * k))


def _one(fixed, b):
    return {key: v[b:b + 1] for key, v in fixed.items()}


def _stable(c, lod, dims, fixed, tol=TOL):
    lo, hi = S._run(c, lod, dims, fixed, tol / S.FACTOR), S._run(c, lod, dims, fixed, tol * S.FACTOR)
    return (lo["rank"] == hi["rank"]).all(axis=1) & (lo["fcol"] == hi["fcol"]).all(axis=1)


def _sensitivity(c, lod, dims, fixed, ref, seed, tol=TOL):
    """skip_cases._sensitivity under the rank tolerance `tol`"""
    s = np.zeros(lod.shape[0])
    for rep in range(3):
        sign = np.where(P.uniform(seed + 31 * rep, lod.size, 7).reshape(lod.shape) < 0.5, -1.0, 1.0)
        x = S._run(c, lod * (1.0 + 1.1e-16 * sign), dims, fixed, tol)["x"]
        s = np.maximum(s, np.abs(x - ref["x"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1)))
    return s


def level_exponents(seed, nobj, rng=LEVEL_RANGE):
    return (np.floor(P.uniform(seed, nobj, 970) * (2 * rng + 1)).astype(int) - rng).clip(-rng, rng)


def scale_levels(lod, dims_b, exps):
    out = lod.copy()
    first = np.concatenate([[0], np.cumsum(dims_b)]).astype(int)
    for k, e in enumerate(exps):
        out[:, first[k]:first[k + 1]] = np.ldexp(out[:, first[k]:first[k + 1]], int(e))
    return out


def decade_scales(seed, n, cap):
    """(column scales (n,), row scales (cap,)): the streams and ranges of P.badly_scaled_batch"""
    return 10.0 ** (6.0 * P.uniform(seed, n, 1) - 3.0), 10.0 ** (4.0 * P.uniform(seed, cap, 2) - 2.0)


def scale_decades(lod, col, row):
    out = lod.copy()
    out[:-1] *= col[:, None]
    out *= row[None, :]
    return out


def case_seed(name, gen):
    return SEED + 10000 * list(S.CASES).index(name) + 1000 * GENERATORS.index(gen)


@functools.lru_cache(maxsize=None)
def _draw(name, gen):
    """the slots of a case under a generator, before any power of two: dict(base (unscaled), lod, exps (levels), col / row (decades), draws)"""
    c = S.CASES[name]
    B, n, cap, nobj = batch_of(c), c["n"], sum(c["caps"]), len(c["caps"])
    seed = case_seed(name, gen)
    dims, fixed = S._dims(c, B), S._fixed(c, B)
    filtered = c["contract"] in ("T", "L")
    deficient = S.DEFICIENT if uniform(c) and B == BATCH else ()
    rng = LEVEL_RANGE_OF.get(name, LEVEL_RANGE)
    base, lod, draws = np.zeros((B, n + 1, cap)), np.zeros((B, n + 1, cap)), np.ones(B, int)
    exps, col, row = np.zeros((B, nobj), int), np.ones((B, n)), np.ones((B, cap))
    for b in range(B):
        d1, f1 = dims[b:b + 1], _one(fixed, b)
        for attempt in range(ATTEMPTS):
            s = seed + b + 100 * attempt
            base[b] = S._problem(c, dims[b], s, b in deficient)
            if gen == "pow2":
                lod[b] = base[b]
                ok = not filtered or _stable(c, lod[b:b + 1], d1, f1)[0]
            elif gen == "levels":
                exps[b] = level_exponents(s, nobj, rng)
                lod[b] = scale_levels(base[b], dims[b], exps[b])
                plain, scaled = S._run(c, base[b:b + 1], d1, f1), S._run(c, lod[b:b + 1], d1, f1)
                ok = bool((plain["rank"] == scaled["rank"]).all() and (plain["fcol"] == scaled["fcol"]).all() and _stable(c, lod[b:b + 1], d1, f1)[0])
            else:
                col[b], row[b] = decade_scales(s, n, cap)
                lod[b] = scale_decades(base[b], col[b], row[b])
                ok = not filtered or _stable(c, lod[b:b + 1], d1, f1)[0]
            if ok:
                break
            draws[b] += 1
        else:
            raise AssertionError(f"{name} / {gen}, slot {b}: no draw kept")
    return dict(base=base, lod=lod, exps=exps, col=col, row=row, draws=draws, dims=dims, fixed=fixed, seed=seed, deficient=list(deficient))


@functools.lru_cache(maxsize=None)
def build(name, gen, k=0):
    """the case `name` under the generator `gen` (pow2: times 2^k): the keys tests/test_gpu_lse_skip.py's handle / run / outputs / assert_contract
    read (n, caps, policy, keep, kernel, contract, reg, guard, dims, fixed, skip: all zero), lod, tol (the handle's rank tolerance), ref (the oracle
    on lod at tol), base / ref_base (the unscaled problems and the oracle on them at 1e-12), exps / col / row, drawn / kept, sens (T, L)"""
    assert k == 0 or gen == "pow2"
    c, d = S.CASES[name], _draw(name, gen)
    dims, fixed, B = d["dims"], d["fixed"], len(d["dims"])
    lod = np.ldexp(d["lod"], k) if k else d["lod"]
    tol = tolerance(k)
    case = dict(name=name, gen=gen, k=k, n=c["n"], caps=list(c["caps"]), policy=c["policy"], keep=bool(c["keep"]), kernel=c["kernel"], contract=c["contract"],
                reg=None, guard=c.get("guard", 0), dims=dims, fixed=fixed, skip=np.zeros(B, np.uint8), lod=lod, tol=tol, base=d["base"], exps=d["exps"],
                col=d["col"], row=d["row"], ref=S._run(c, lod, dims, fixed, tol), ref_base=S._run(c, d["base"], dims, fixed), drawn=int(d["draws"].sum()),
                kept=B, seed=d["seed"], deficient=d["deficient"])
    if c["contract"] in ("T", "L"):
        case["sens"] = _sensitivity(c, lod, dims, fixed, case["ref"], d["seed"], tol)
    for a in [lod, case["skip"], case["sens"] if "sens" in case else lod, *case["ref"].values(), *case["ref_base"].values()]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    for a in [dims, d["base"], d["lod"], d["exps"], d["col"], d["row"], *fixed.values()]:
        a.setflags(write=False)
    return case


def first_pivot(case, ref):
    """per problem: the variable the first pivot step takes (the transposition behind the fixed columns; -1 where every variable is fixed)"""
    B, n = len(case["dims"]), case["n"]
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(B, np.uint32)
    return np.array([int(ref["perm"][b, int(nf[b])]) if int(nf[b]) < n and int(ref["totalrank"][b]) > int(nf[b]) else -1 for b in range(B)])


def column_norm_ratio(case):
    """per problem: largest / smallest column norm of A over the problem's own rows"""
    out = []
    for b in range(len(case["dims"])):
        m = int(case["dims"][b].sum())
        nrm = np.sqrt((case["lod"][b, :case["n"], :m] ** 2).sum(axis=1))
        out.append(float(nrm.max() / nrm.min()))
    return np.array(out)


def guard_estimates(case):
    """the accuracy guard's estimate as scripts/calibrate_guard.py computes it from the oracle's factor (uniform IK shape)"""
    from scripts import calibrate_guard as CG
    return CG.estimate(case["lod"], case["caps"], case["n"], case["ref"])


# ---- the consumers of a kept factor on `decades` ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def consumers(name):
    """what the post-factorization calls must give on the decades data of a factor-kept case, and how far the two CPU references of each family
    are apart on them.  types, mult, ln1 as sparse_cases.consumers; G (batch, K, n) cotangents, grad_rhs_A / _B: references (A) and (B) of
    tests/adjoint_cases.py; flags, GA / GB: the rank-stability rule and references (A) / (B) of tests/adjoint_matrix_cases.py for cotangent 0;
    dlod (K, batch, n + 1, cap) directions in the data's own units, TA / TB: references (A) / (B) of tests/tangent_cases.py; rhs (K, batch, cap)
    in the rows' units, XA / XB: references (a) / (b) of tests/solve_rhs_cases.py; gaps = {family: largest (A)-(B) discrepancy}"""
    import adjoint_cases as AC
    import adjoint_matrix_cases as AM
    import solve_rhs_cases as SC
    import tangent_cases as TC
    case, c = build(name, "decades"), S.CASES[name]
    assert not case["fixed"] and case["keep"]
    B, n, nobj, cap, K = len(case["dims"]), case["n"], len(case["caps"]), sum(case["caps"]), K_COT
    ref, lod, dims, seed = case["ref"], case["lod"], case["dims"], case["seed"]
    types = (1 + (P.uniform(seed + 200000, B * cap) * 3).astype(np.uint8)).reshape(B, cap)
    per_level = [S._run(c, lod, dims, {}, ctr_type=types, sens_obj=k) for k in range(nobj)]
    G = P.normal(seed + 900, B * K * n).reshape(B, K, n)
    A, Bf = np.zeros((B, K, cap)), np.zeros((B, K, cap))
    for j in range(K):
        ac = dict(n=n, caps=case["caps"], lod=lod, dims=dims, fixed={}, g=G[:, j])
        A[:, j] = AC.reference_unit_solves(ac)[0]
        Bf[:, j] = AC.reference_from_factor(ac, ref)[0]
    am = dict(n=n, caps=case["caps"], lod=lod, dims=dims, fixed={}, g=G[:, 0])
    flags = np.array([AM.rank_stable(n, dims[b], ref["rank"][b], ref["fcol"][b], 0) for b in range(B)], np.uint8)
    GA, GB = np.zeros((B, n + 1, cap)), np.zeros((B, n + 1, cap))
    unit = np.concatenate([case["col"], np.ones((B, 1))], axis=1)[:, :, None] * case["row"][:, None, :]  # the magnitude of every entry of [A | b]
    dlod = P.normal(seed + 901, K * B * (n + 1) * cap).reshape(K, B, n + 1, cap) * unit[None]
    TA, TB = np.zeros((K, B, n)), np.zeros((K, B, n))
    for b in np.flatnonzero(flags):
        GA[b] = AM.reference_kkt(n, lod[b], dims[b], ref["rank"][b], ref["perm"][b], ref["totalrank"][b], 0, None, None, G[b, 0])
        GB[b] = AM.reference_from_factor(am, ref, b)[0]
        for j in range(K):
            TA[j, b] = TC.tangent_kkt(n, lod[b], dims[b], ref["rank"][b], ref["perm"][b], ref["totalrank"][b], 0, np.zeros(0, int), np.zeros(0),
                                      dlod[j, b], np.zeros(n))
            TB[j, b] = TC.tangent_from_factor(am, ref, b, dlod[j, b], np.zeros(n))[0]
    rhs = P.normal(seed + 902, K * B * cap).reshape(K, B, cap) * case["row"][None]
    XA, XB = np.zeros((K, B, n)), np.zeros((K, B, n))
    for j in range(K):
        other = lod.copy()
        other[:, n, :] = rhs[j]
        XA[j] = S._run(c, other, dims, {})["x"]
        for b in range(B):
            XB[j, b] = SC.solve_rhs_from_factor(ref["factor"][b], ref["hh"][b], ref["perm"][b], ref["rank"][b], ref["fcol"][b], ref["totalrank"][b], dims[b], 0,
                                                rhs[j, b], np.zeros(n), 0, None)
    gaps = dict(adjoint=max(AC._rel(A[b, j] - Bf[b, j], A[b, j]) for b in range(B) for j in range(K)),
                adjoint_matrix=max([AC._rel(GA[b] - GB[b], GA[b]) for b in np.flatnonzero(flags)] or [0.0]),
                tangent=max([AC._rel(TA[j, b] - TB[j, b], TA[j, b]) for b in np.flatnonzero(flags) for j in range(K)] or [0.0]),
                solve_rhs=SC.rel_rows(XB, XA))
    out = dict(types=types, mult=np.stack([r["lam"] for r in per_level], axis=1), ln1=S._run(c, lod, dims, {}, solve_option=1)["x"], G=G, grad_rhs_A=A, grad_rhs_B=Bf,
               flags=flags, GA=GA, GB=GB, dlod=dlod, TA=TA, TB=TB, rhs=rhs, XA=XA, XB=XB, gaps=gaps)
    for a in [v for v in out.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return out


# the largest (A)-(B) discrepancy of each family over skip_cases.CONSUMER_CASES on decades, rounded up (the table above; tests/test_scale_cases.py
# re-measures it) and what the device is allowed: 10 x, the project's rule
CONSUMER_D_CPU = dict(adjoint=6.1e-12, adjoint_matrix=1.55e-8, tangent=1.73e-8, solve_rhs=9.5e-12)  # (the KKT references square the condition number)
CONSUMER_TOL = {fam: 10.0 * d for fam, d in CONSUMER_D_CPU.items()}


# ---- one LexLSI case: the general levels of P.lsi_problem in other units ------------------------------------------------------------------------
LSI_N, LSI_DIMS, LSI_INSTANCES = 40, [12] * 5, 6
LSI_SEED = 20349000  # the first seed of the series 20349000, 20349100, ... at which the oracle driver ends PROBLEM_SOLVED for every instance


def lsi_exponents(seed=LSI_SEED):
    """(instances, levels): the power of two of every level; level 0 (simple bounds: a row is a variable, it has no unit of its own) keeps 0"""
    e = np.stack([level_exponents(seed + i, len(LSI_DIMS)) for i in range(LSI_INSTANCES)])
    e[:, 0] = 0
    return e


def lsi_problems(seed=LSI_SEED):
    """LSI_INSTANCES problems (instance i from seed + i): level 0 simple bounds, every general level — A, lower and upper bounds — times 2^e"""
    out, exps = [], lsi_exponents(seed)
    for i in range(LSI_INSTANCES):
        objs = P.lsi_problem(seed + i, LSI_N, LSI_DIMS, simple_bounds=True)
        for k in range(1, len(LSI_DIMS)):
            for key in ("A", "lb", "ub"):
                objs[k][key] = np.ldexp(objs[k][key], int(exps[i, k]))
        out.append(objs)
    return out


def summary(case):
    line = (f"    {run_id(case['name'], case['gen'], case['k']):<22} n={case['n']:<4}{str(case['caps']).replace(' ', ''):<20}{case['kernel']:<36} kept {case['kept']:>2} / "
            f"{case['drawn']:<2}  max|x| {np.abs(case['ref']['x']).max():.1e}")
    if "sens" in case:
        line += f"  sens {case['sens'].max():.1e}"
    if case["name"] == "qtol_guard" and case["gen"] == "decades":
        est = guard_estimates(case)
        line += f"  est {est.min():.3g} .. {est.max():.3g}"
    return line


def consumer_summary(name):
    g = consumers(name)["gaps"]
    return (f"    {name + ' consumers':<22} decades  rank-stable {int(consumers(name)['flags'].sum()):>2} / {len(consumers(name)['flags'])}  gap adjoint {g['adjoint']:.1e}  "
            f"adjoint_matrix {g['adjoint_matrix']:.1e}  tangent {g['tangent']:.1e}  solve_rhs {g['solve_rhs']:.1e}")


if __name__ == "__main__":
    for nm, g, k in runs():
        print(summary(build(nm, g, k)))
    for nm in S.CONSUMER_CASES:
        print(consumer_summary(nm))
