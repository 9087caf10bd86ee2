"""Batches that hold every LexLSE factorization kernel family to the oracle on BLOCK-SPARSE data: columns that are exactly zero in a level's
rows (tests/test_gpu_sparse.py runs them on the GPU, tests/test_sparse_cases.py asserts the conditions below on the CPU, from the oracle and
the planner alone).  Every other batch of the suite is dense Gaussian data or a transform of it: a dependent column reaches the rank test with
a squared norm near 1e-30, never with 0.0.  An inverse-kinematics Jacobian is block-sparse — a task on one limb has exact zeros in the columns
of every other limb, a joint no task touches is a zero column in all levels — and there a kernel searches its pivot among norms that all tie
at exactly zero, tests the rank on 0.0, builds reflectors with an exactly zero tail, and everything behind a kept factor reads levels of rank 0
and columns that were never pivoted.  No extreme scaling here: overflow and underflow are outside every stated contract.

Generators (pure functions of a seed, on P.lse_problem — what P.lse_batch stacks; one problem per slot, slot b of a case from seed + b):
    limbs       the n columns are cut into groups (WIDTHS, per shape); every level except the last keeps two groups, chosen per problem and level
                from the seed, every other entry of its rows is exactly 0.0; the last level stays dense.  Neighbours in a wavefront get different
                rank profiles.  The widths are chosen so that levels do lose rank: two groups of eight lose nothing under eight-row levels or
                under the two levels of n = 44, so those shapes get narrower groups.
    dead        limbs plus three variables that are zero in every level, one in each third of the column range (one in every column slot of the
                multi-slot kernels), another three per problem.
    zero_level  limbs plus, in the problems b % 3 == 1, one whole level of zero rows (A and b): the first, the middle or the last level, in turn.
    zero_rhs    limbs with b = 0 in all levels: x is exactly zero.
    neg_zero    limbs with a seeded half of the structural zeros stored as -0.0 (`lod_plus`: the same data with +0.0).

Cases: skip_cases.CASES (imported: n, caps, policy, keep, the expected last_kernel() name, the contract, fixed variables, ragged dimensions), one
per instantiation of every factorization kernel family; batch 19 (the large shape 3), so wavefront tails and mixed groups of four stay.  Every
case runs limbs and dead; zero_level, zero_rhs and neg_zero run on one case per family group (FULL).  Tolerance-contract cases (T, L) keep only
problems that are STABLE in the sense of tests/rank_cases.py — the same oracle ranks and first columns at tol / 10 and 10 tol — an unstable slot
is redrawn from the next seed of its series (seed + b + 100, ...), and a case keeps at least skip_cases.RETENTION of what it drew.
NOT covered: the regularized wave kernel (wave_reg: tests/reg_cases.py owns that family, and damping removes the exact zeros this module is
about) and lqr_generic<1024,lds>, which needs more than 512 rows and stays uncovered here as in the skip-mask tests.

What a level "cut at an exactly zero norm" is (cut_levels): rank below min(rows, columns left) with what is left of its rows in the unpivoted
columns exactly 0.0 in the oracle's factor.  Structural zeros survive the eliminations of the earlier levels only where every update term is
zero — a zero multiplier, or a pivot row that is itself zero in that column; tests/test_sparse_cases.py asserts that from the factor.

MEASURED (oracle alone, `python tests/sparse_cases.py`; zeros = share of exactly zero entries of A over the problems' own rows; kept / drawn as
above; rank 0 = (problem, level) pairs of rank 0; cut = pairs cut at an exactly zero norm, in `problems` of the batch; profiles = distinct rank
profiles in the batch):
    qtol_ik       limbs      n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7>               zeros 0.48  kept 19 / 19  rank 0 16  cut 27 in 18 problems  profiles 12  max|x| 1.5e+02
    qtol_ik       dead       n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7>               zeros 0.52  kept 19 / 19  rank 0 20  cut 64 in 19 problems  profiles 15  max|x| 2.1e+01
    qtol_ik       zero_level n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7>               zeros 0.52  kept 19 / 19  rank 0 21  cut 31 in 18 problems  profiles 11  max|x| 6.3e+02
    qtol_ik       zero_rhs   n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7>               zeros 0.48  kept 19 / 19  rank 0 19  cut 27 in 17 problems  profiles  8  max|x| 0.0e+00
    qtol_ik       neg_zero   n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7>               zeros 0.48  kept 19 / 19  rank 0 15  cut 33 in 17 problems  profiles  9  max|x| 4.4e+01
    qtol_8        limbs      n=40  [8,8,8,8,8]        lqr_qtol<3,8>                        zeros 0.64  kept 19 / 19  rank 0  7  cut 32 in 19 problems  profiles 11  max|x| 1.1e+02
    qtol_8        dead       n=40  [8,8,8,8,8]        lqr_qtol<3,8>                        zeros 0.67  kept 19 / 19  rank 0  7  cut 60 in 19 problems  profiles 18  max|x| 2.0e+03
    qtol_n24      limbs      n=24  [12,12,12,12,12]   lqr_qtol<2,12>                       zeros 0.48  kept 19 / 19  rank 0 29  cut 60 in 19 problems  profiles 13  max|x| 8.6e+00
    qtol_n24      dead       n=24  [12,12,12,12,12]   lqr_qtol<2,12>                       zeros 0.54  kept 19 / 19  rank 0 32  cut 95 in 19 problems  profiles 19  max|x| 3.6e+00
    qtol_ragged   limbs      n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7,ragged>        zeros 0.48  kept 19 / 19  rank 0 10  cut 24 in 16 problems  profiles 11  max|x| 1.3e+02
    qtol_ragged   dead       n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7,ragged>        zeros 0.52  kept 19 / 19  rank 0 14  cut 49 in 19 problems  profiles 17  max|x| 3.7e+01
    qtol_guard    limbs      n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7,guard>         zeros 0.48  kept 19 / 19  rank 0 18  cut 25 in 16 problems  profiles  8  max|x| 2.3e+02
    qtol_guard    dead       n=40  [12,12,12,12,12]   lqr_qtol<3,12,shift 7,guard>         zeros 0.52  kept 19 / 19  rank 0 19  cut 68 in 19 problems  profiles 15  max|x| 3.2e+01
    mfma_two      limbs      n=40  [12,12,12,12,12]   lqr_mfma<32,12,n40>                  zeros 0.48  kept 19 / 19  rank 0 14  cut 30 in 16 problems  profiles 10  max|x| 9.0e+01
    mfma_two      dead       n=40  [12,12,12,12,12]   lqr_mfma<32,12,n40>                  zeros 0.52  kept 19 / 19  rank 0 18  cut 62 in 19 problems  profiles 16  max|x| 8.6e+00
    mfma_two      zero_level n=40  [12,12,12,12,12]   lqr_mfma<32,12,n40>                  zeros 0.52  kept 19 / 19  rank 0 19  cut 34 in 18 problems  profiles 11  max|x| 9.3e+02
    mfma_two      zero_rhs   n=40  [12,12,12,12,12]   lqr_mfma<32,12,n40>                  zeros 0.48  kept 19 / 19  rank 0 20  cut 30 in 16 problems  profiles  7  max|x| 0.0e+00
    mfma_two      neg_zero   n=40  [12,12,12,12,12]   lqr_mfma<32,12,n40>                  zeros 0.48  kept 19 / 19  rank 0 20  cut 29 in 16 problems  profiles  8  max|x| 3.3e+01
    mfma_one      limbs      n=40  [12,12,12,12,12]   lqr_mfma<64,12>                      zeros 0.48  kept 19 / 19  rank 0 16  cut 29 in 17 problems  profiles  7  max|x| 7.0e+01
    mfma_one      dead       n=40  [12,12,12,12,12]   lqr_mfma<64,12>                      zeros 0.52  kept 19 / 19  rank 0 17  cut 67 in 19 problems  profiles 18  max|x| 1.3e+01
    mfma_four     limbs      n=40  [12,12,12,12,12]   lqr_mfma<16,12,n40>                  zeros 0.48  kept 19 / 19  rank 0 19  cut 35 in 18 problems  profiles  9  max|x| 6.1e+01
    mfma_four     dead       n=40  [12,12,12,12,12]   lqr_mfma<16,12,n40>                  zeros 0.52  kept 19 / 19  rank 0 16  cut 69 in 19 problems  profiles 14  max|x| 7.5e+01
    mfma_two_n44  limbs      n=44  [12,12]            lqr_mfma<32,12>                      zeros 0.39  kept 19 / 19  rank 0  0  cut 19 in 19 problems  profiles  2  max|x| 3.4e+00
    mfma_two_n44  dead       n=44  [12,12]            lqr_mfma<32,12>                      zeros 0.43  kept 19 / 19  rank 0  0  cut 19 in 19 problems  profiles  3  max|x| 3.6e+00
    quad_ik_x     limbs      n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7>               zeros 0.48  kept 19 / 19  rank 0 16  cut 31 in 17 problems  profiles 11  max|x| 2.3e+02
    quad_ik_x     dead       n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7>               zeros 0.52  kept 19 / 19  rank 0 23  cut 60 in 19 problems  profiles 14  max|x| 3.9e+01
    quad_ik_f     limbs      n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor>        zeros 0.48  kept 19 / 19  rank 0 17  cut 28 in 16 problems  profiles  9  max|x| 1.0e+02
    quad_ik_f     dead       n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor>        zeros 0.52  kept 19 / 19  rank 0 18  cut 68 in 19 problems  profiles 14  max|x| 2.2e+01
    quad_ik_f     zero_level n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor>        zeros 0.52  kept 19 / 19  rank 0 20  cut 26 in 15 problems  profiles  8  max|x| 4.6e+01
    quad_ik_f     zero_rhs   n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor>        zeros 0.48  kept 19 / 19  rank 0 19  cut 27 in 16 problems  profiles  8  max|x| 0.0e+00
    quad_ik_f     neg_zero   n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor>        zeros 0.48  kept 19 / 19  rank 0 16  cut 27 in 16 problems  profiles  8  max|x| 4.1e+01
    quad_wide_x   limbs      n=47  [14,9,16,8]        lqr_quad<4,16>                       zeros 0.50  kept 19 / 19  rank 0  1  cut 14 in 12 problems  profiles  8  max|x| 3.4e+02
    quad_wide_x   dead       n=47  [14,9,16,8]        lqr_quad<4,16>                       zeros 0.53  kept 19 / 19  rank 0  0  cut 18 in 16 problems  profiles 10  max|x| 9.8e+02
    quad_wide_f   limbs      n=47  [14,9,16,8]        lqr_quad<4,16,factor>                zeros 0.50  kept 19 / 19  rank 0  0  cut 13 in 13 problems  profiles  7  max|x| 2.6e+02
    quad_wide_f   dead       n=47  [14,9,16,8]        lqr_quad<4,16,factor>                zeros 0.53  kept 19 / 19  rank 0  0  cut 18 in 17 problems  profiles  9  max|x| 4.5e+02
    quad_fixed_x  limbs      n=47  [14,9,16,8]        lqr_quad<4,16,fixed>                 zeros 0.50  kept 19 / 19  rank 0  3  cut 15 in 12 problems  profiles 12  max|x| 1.0e+02
    quad_fixed_x  dead       n=47  [14,9,16,8]        lqr_quad<4,16,fixed>                 zeros 0.53  kept 19 / 19  rank 0  2  cut 30 in 19 problems  profiles 15  max|x| 4.8e+01
    quad_fixed_f  limbs      n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor,fixed>  zeros 0.48  kept 19 / 19  rank 0 21  cut 33 in 19 problems  profiles 16  max|x| 1.3e+02
    quad_fixed_f  dead       n=40  [12,12,12,12,12]   lqr_quad<3,12,shift 7,factor,fixed>  zeros 0.52  kept 19 / 19  rank 0 19  cut 69 in 19 problems  profiles 19  max|x| 2.2e+01
    lwave_f       limbs      n=40  [12,12,12,12,12]   lqr_lwave<41,12,exact>               zeros 0.48  kept 19 / 19  rank 0 18  cut 35 in 17 problems  profiles  9  max|x| 5.3e+03
    lwave_f       dead       n=40  [12,12,12,12,12]   lqr_lwave<41,12,exact>               zeros 0.52  kept 19 / 19  rank 0 17  cut 64 in 19 problems  profiles 16  max|x| 1.8e+01
    lwave_x       limbs      n=31  [12,12,12]         lqr_lwave<41,12>                     zeros 0.44  kept 19 / 19  rank 0  1  cut 38 in 19 problems  profiles  6  max|x| 1.2e+02
    lwave_x       dead       n=31  [12,12,12]         lqr_lwave<41,12>                     zeros 0.50  kept 19 / 19  rank 0  3  cut 46 in 19 problems  profiles 12  max|x| 2.1e+01
    wave_exact    limbs      n=40  [12,12,12,12,12]   lqr_wave<41,12,exact>                zeros 0.48  kept 19 / 19  rank 0 19  cut 27 in 17 problems  profiles 10  max|x| 2.0e+02
    wave_exact    dead       n=40  [12,12,12,12,12]   lqr_wave<41,12,exact>                zeros 0.52  kept 19 / 19  rank 0 19  cut 66 in 19 problems  profiles 15  max|x| 3.2e+01
    wave_exact    zero_level n=40  [12,12,12,12,12]   lqr_wave<41,12,exact>                zeros 0.52  kept 19 / 19  rank 0 19  cut 29 in 16 problems  profiles 10  max|x| 2.2e+02
    wave_exact    zero_rhs   n=40  [12,12,12,12,12]   lqr_wave<41,12,exact>                zeros 0.48  kept 19 / 19  rank 0 19  cut 31 in 17 problems  profiles  7  max|x| 0.0e+00
    wave_exact    neg_zero   n=40  [12,12,12,12,12]   lqr_wave<41,12,exact>                zeros 0.48  kept 19 / 19  rank 0 17  cut 29 in 17 problems  profiles  8  max|x| 4.3e+01
    wave_n31      limbs      n=31  [12,12,12]         lqr_wave<41,12>                      zeros 0.44  kept 19 / 19  rank 0  1  cut 38 in 19 problems  profiles  7  max|x| 3.2e+01
    wave_n31      dead       n=31  [12,12,12]         lqr_wave<41,12>                      zeros 0.50  kept 19 / 19  rank 0  2  cut 47 in 19 problems  profiles 13  max|x| 9.2e+00
    wave_64       limbs      n=47  [14,9,16,8]        lqr_wave<64,16>                      zeros 0.50  kept 19 / 19  rank 0  0  cut 13 in 12 problems  profiles  9  max|x| 7.5e+01
    wave_64       dead       n=47  [14,9,16,8]        lqr_wave<64,16>                      zeros 0.53  kept 19 / 19  rank 0  1  cut 20 in 17 problems  profiles  8  max|x| 1.1e+02
    generic_64    limbs      n=40  [12,12,12,12,12]   lqr_generic<64,lds>                  zeros 0.48  kept 19 / 19  rank 0 18  cut 27 in 15 problems  profiles  8  max|x| 6.6e+02
    generic_64    dead       n=40  [12,12,12,12,12]   lqr_generic<64,lds>                  zeros 0.52  kept 19 / 19  rank 0 16  cut 62 in 19 problems  profiles 17  max|x| 8.6e+00
    generic_64    zero_level n=40  [12,12,12,12,12]   lqr_generic<64,lds>                  zeros 0.52  kept 19 / 19  rank 0 20  cut 25 in 16 problems  profiles  9  max|x| 1.2e+03
    generic_64    zero_rhs   n=40  [12,12,12,12,12]   lqr_generic<64,lds>                  zeros 0.48  kept 19 / 19  rank 0 19  cut 29 in 15 problems  profiles  6  max|x| 0.0e+00
    generic_64    neg_zero   n=40  [12,12,12,12,12]   lqr_generic<64,lds>                  zeros 0.48  kept 19 / 19  rank 0 20  cut 30 in 16 problems  profiles  7  max|x| 5.8e+01
    generic_256   limbs      n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 zeros 0.50  kept 19 / 19  rank 0 34  cut 46 in 17 problems  profiles  9  max|x| 1.4e+02
    generic_256   dead       n=40  [12,12,12,12,12,12] lqr_generic<256,lds>                 zeros 0.53  kept 19 / 19  rank 0 35  cut 86 in 19 problems  profiles 15  max|x| 5.3e+01
    generic_hbm   limbs      n=100 [115,115]          lqr_generic<1024,hbm>                zeros 0.30  kept  3 / 3   rank 0  0  cut  3 in  3 problems  profiles  1  max|x| 5.0e-01
    generic_hbm   dead       n=100 [115,115]          lqr_generic<1024,hbm>                zeros 0.32  kept  3 / 3   rank 0  0  cut  6 in  3 problems  profiles  2  max|x| 4.9e-01
    large_multi   limbs      n=100 [115,115]          lqr_large<multi-launch>              zeros 0.30  kept  3 / 3   rank 0  0  cut  3 in  3 problems  profiles  1  max|x| 4.8e-01
    large_multi   dead       n=100 [115,115]          lqr_large<multi-launch>              zeros 0.32  kept  3 / 3   rank 0  0  cut  6 in  3 problems  profiles  2  max|x| 4.1e-01
    large_multi   zero_level n=100 [115,115]          lqr_large<multi-launch>              zeros 0.37  kept  3 / 3   rank 0  1  cut  3 in  3 problems  profiles  2  max|x| 4.8e-01
    large_multi   zero_rhs   n=100 [115,115]          lqr_large<multi-launch>              zeros 0.30  kept  3 / 3   rank 0  0  cut  3 in  3 problems  profiles  1  max|x| 0.0e+00
    large_multi   neg_zero   n=100 [115,115]          lqr_large<multi-launch>              zeros 0.30  kept  3 / 3   rank 0  0  cut  3 in  3 problems  profiles  1  max|x| 5.7e-01
    large_fast    limbs      n=100 [115,115]          lqr_large<step-per-pivot,mfma>       zeros 0.30  kept  3 / 3   rank 0  0  cut  3 in  3 problems  profiles  1  max|x| 5.4e-01
    large_fast    dead       n=100 [115,115]          lqr_large<step-per-pivot,mfma>       zeros 0.32  kept  3 / 3   rank 0  0  cut  6 in  3 problems  profiles  3  max|x| 4.2e-01
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

GENERATORS = ("limbs", "dead", "zero_level", "zero_rhs", "neg_zero")
NAMES = [nm for nm in S.CASES if nm not in ("wave_reg", "mfma_one_n44")]  # (mfma_one_n44: lqr_mfma<64,12> is mfma_one's instantiation)
FULL = ("qtol_ik", "mfma_two", "quad_ik_f", "wave_exact", "generic_64", "large_multi")  # one case per family group: all five generators
CONSUMER_GENERATORS = ("dead", "zero_level")
BATCH, LARGE_BATCH = 19, 3
KEPT_GROUPS = 2
SEED = 20330000
# (n, number of levels) -> widths of the column groups
WIDTHS = {
    (40, 5): [8] * 5,                 # 12-row levels: level 0 keeps its rank, the levels behind it lose theirs where groups repeat
    (40, 6): [8] * 5,
    (24, 5): [5, 5, 5, 5, 4],         # two groups hold 9 or 10 columns: level 0 is always cut
    (47, 4): [9, 9, 9, 10, 10],
    (44, 2): [5] * 8 + [4],           # level 0 is the only sparse one: 9 or 10 columns under 12 rows
    (31, 3): [5, 5, 5, 5, 5, 6],
    (100, 2): [20] * 5,               # 40 columns under 115 rows
}
WIDTHS_8 = [4] * 10                   # eight-row levels at n = 40: two groups hold eight columns
# the zero_level data of the consumer cases: the first seed of the series seed, seed + 20, ... at which at least two problems are rank-stable
# (tests/adjoint_matrix_cases.py: they have a gradient with respect to A) and references (A) and (B) of that module agree within TOL / 10 on them
# — its rule: data that would need more get another seed, the tolerance is not raised (generic_64: 1.2e-12, 1.1e-12, 2.3e-13 ... before 2.7e-14)
SEED_SHIFT = {("wave_exact", "zero_level"): 20, ("quad_ik_f", "zero_level"): 20, ("generic_64", "zero_level"): 280}


def cases(generators=GENERATORS):
    """(name, generator) pairs: limbs and dead everywhere, the other three on FULL"""
    return [(nm, g) for nm in NAMES for g in generators if g in ("limbs", "dead") or nm in FULL]


def widths_of(c):
    if c["n"] == 40 and max(c["caps"]) == 8:
        return WIDTHS_8
    return WIDTHS[(c["n"], len(c["caps"]))]


def batch_of(c):
    return LARGE_BATCH if c["n"] == 100 else BATCH


def _problem(c, gen, dims_b, seed, b):
    """one problem: (lod (n + 1, cap), structural (n, cap) bool: the entries of A set to zero by construction)"""
    n, caps, nobj = c["n"], list(c["caps"]), len(c["caps"])
    dims_b = [int(d) for d in dims_b]
    lod = P.lse_problem(seed, n, dims_b, caps)
    first = np.concatenate([[0], np.cumsum(dims_b)]).astype(int)
    group = np.repeat(np.arange(len(widths_of(c))), widths_of(c))
    assert len(group) == n
    structural = np.zeros((n, lod.shape[1]), bool)
    for k in range(nobj - 1):
        kept = np.argsort(P.uniform(seed, len(widths_of(c)), 900 + k))[:KEPT_GROUPS]
        structural[np.ix_(~np.isin(group, kept), np.arange(first[k], first[k + 1]))] = True
    if gen == "dead":
        for t, u in enumerate(P.uniform(seed, 3, 950)):
            lo, hi = t * n // 3, (t + 1) * n // 3
            structural[lo + int(u * (hi - lo)), :first[nobj]] = True
    lod[:n][structural] = 0.0
    if gen == "zero_level" and b % 3 == 1:
        k = (0, nobj // 2, nobj - 1)[(b // 3) % 3]
        lod[:, first[k]:first[k + 1]] = 0.0
        structural[:, first[k]:first[k + 1]] = True
    if gen == "zero_rhs":
        lod[n, :] = 0.0
    if gen == "neg_zero":
        minus = structural & (P.uniform(seed, structural.size, 960).reshape(structural.shape) < 0.5)
        lod[:n][minus] = -0.0
    return lod, structural


def cut_levels(case):
    """[(problem, level)] whose rank is below min(rows, columns left): candidates for a cut at an exactly zero norm"""
    ref, dims, n = case["ref"], case["dims"], case["n"]
    return [(b, k) for b in range(dims.shape[0]) for k in range(dims.shape[1])
            if int(ref["rank"][b, k]) < min(int(dims[b, k]), max(n - int(ref["fcol"][b, k]), 0))]


def leftover(case, b, k):
    """what the oracle's factor holds of level k's rows behind its pivots, in the unpivoted columns: (columns left, rows left)"""
    ref, dims, n = case["ref"], case["dims"], case["n"]
    F = int(dims[b, :k].sum())
    Fc, r = int(ref["fcol"][b, k]), int(ref["rank"][b, k])
    return ref["factor"][b, Fc + r:n, F + r:F + int(dims[b, k])]


@functools.lru_cache(maxsize=None)
def build(name, gen):
    """the case `name` under the generator `gen`: dict(n, caps, policy, keep, kernel, contract, guard, reg, dims, fixed, lod, structural, ref (the
    oracle), drawn / kept, sens (contract L: the one-ulp sensitivity of x, skip_cases._sensitivity), lod_plus (neg_zero: the data with +0.0))"""
    c = S.CASES[name]
    B, n = batch_of(c), c["n"]
    seed = SEED + 10000 * list(S.CASES).index(name) + 1000 * GENERATORS.index(gen) + SEED_SHIFT.get((name, gen), 0)
    dims, fixed = S._dims(c, B), S._fixed(c, B)
    filtered = c["contract"] in ("T", "L")
    lod, structural, draws = np.zeros((B, n + 1, sum(c["caps"]))), np.zeros((B, n, sum(c["caps"])), bool), np.ones(B, int)
    for b in range(B):
        for attempt in range(8):
            lod[b], structural[b] = _problem(c, gen, dims[b], seed + b + 100 * attempt, b)
            one = {k: v[b:b + 1] for k, v in fixed.items()}
            if not filtered or S._stable(c, lod[b:b + 1], dims[b:b + 1], one)[0]:
                break
            draws[b] += 1
        else:
            raise AssertionError(f"{name} / {gen}, slot {b}: no stable draw")
    case = dict(name=name, gen=gen, n=n, caps=list(c["caps"]), policy=c["policy"], keep=bool(c["keep"]), kernel=c["kernel"], contract=c["contract"],
                reg=None, guard=c.get("guard", 0), dims=dims, fixed=fixed, lod=lod, structural=structural, ref=S._run(c, lod, dims, fixed),
                drawn=int(draws.sum()), kept=B, seed=seed)
    if c["contract"] == "L":
        case["sens"] = S._sensitivity(c, lod, dims, fixed, case["ref"], seed)
    if gen == "neg_zero":
        case["lod_plus"] = np.where(lod == 0.0, 0.0, lod)
    for a in [dims, lod, structural, *fixed.values(), *case["ref"].values()] + [case[k] for k in ("sens", "lod_plus") if k in case]:
        a.setflags(write=False)  # shared among the tests: nobody changes it
    return case


@functools.lru_cache(maxsize=None)
def consumers(name, gen):
    """what the post-factorization calls must give on a factor-kept case (oracle only): types (LB / UB / EQ mixed), v, sens / maxabs / lam / marks
    of ObjectiveSensitivity(k) for every level k, mult = the nObj lam vectors, ln1 (solveLeastNorm_1); G (batch, K, n) cotangents with
    grad_rhs_A (batch, K, cap): reference (A) of tests/adjoint_cases.py, the unit solves of the oracle, and grad_rhs_B: its reference (B);
    flags / GA / GB: the rank-stability rule and references (A) (KKT) and (B) of tests/adjoint_matrix_cases.py for cotangent 0"""
    import adjoint_cases as AC
    import adjoint_matrix_cases as AM
    case, c = build(name, gen), S.CASES[name]
    assert not case["fixed"]
    B, n, nobj, cap, K = case["lod"].shape[0], case["n"], len(case["caps"]), sum(case["caps"]), 3
    types = (1 + (P.uniform(case["seed"] + 200000, B * cap) * 3).astype(np.uint8)).reshape(B, cap)
    per_level = [S._run(c, case["lod"], case["dims"], {}, ctr_type=types, sens_obj=k) for k in range(nobj)]
    G = P.normal(case["seed"] + 900, B * K * n).reshape(B, K, n)
    ref = case["ref"]
    A, Bf = np.zeros((B, K, cap)), np.zeros((B, K, cap))
    for j in range(K):
        ac = dict(n=n, caps=case["caps"], lod=case["lod"], dims=case["dims"], fixed={}, g=G[:, j])
        A[:, j] = AC.reference_unit_solves(ac)[0]
        Bf[:, j] = AC.reference_from_factor(ac, ref)[0]
    am = dict(n=n, caps=case["caps"], lod=case["lod"], dims=case["dims"], fixed={}, g=G[:, 0])
    flags = np.array([AM.rank_stable(n, case["dims"][b], ref["rank"][b], ref["fcol"][b], 0) for b in range(B)], np.uint8)
    GA, GB = np.zeros((B, n + 1, cap)), np.zeros((B, n + 1, cap))
    for b in np.flatnonzero(flags):
        GA[b] = AM.reference_kkt(n, case["lod"][b], case["dims"][b], ref["rank"][b], ref["perm"][b], ref["totalrank"][b], 0, None, None, G[b, 0])
        GB[b] = AM.reference_from_factor(am, ref, b)[0]
    out = dict(types=types, v=ref["v"], sens=[r["sens"] for r in per_level], maxabs=[r["maxabs"] for r in per_level], lam=[r["lam"] for r in per_level],
               marks=[r["ctr_type_out"] for r in per_level], mult=np.stack([r["lam"] for r in per_level], axis=1),
               ln1=S._run(c, case["lod"], case["dims"], {}, solve_option=1)["x"], G=G, grad_rhs_A=A, grad_rhs_B=Bf, flags=flags, GA=GA, GB=GB)
    for a in [v for v in out.values() if isinstance(v, np.ndarray)] + [x for k in ("sens", "maxabs", "lam", "marks") for x in out[k]]:
        a.setflags(write=False)
    return out


# ---- one LexLSI case: the general levels of P.lsi_problem made block-sparse by the `limbs` rule ----------------------------------------------
LSI_N, LSI_DIMS, LSI_INSTANCES = 40, [12] * 5, 6
LSI_SEED = 20339000  # the first seed of the series 20339000, 20339100, ... at which the oracle driver ends PROBLEM_SOLVED for every instance


def lsi_problems(seed=LSI_SEED):
    """LSI_INSTANCES problems (instance i from seed + i): level 0 simple bounds, the general levels but the last keep two column groups of eight"""
    group = np.repeat(np.arange(5), 8)
    out = []
    for i in range(LSI_INSTANCES):
        objs = P.lsi_problem(seed + i, LSI_N, LSI_DIMS, simple_bounds=True)
        for k in range(1, len(LSI_DIMS) - 1):
            kept = np.argsort(P.uniform(seed + i, 5, 900 + k))[:KEPT_GROUPS]
            objs[k]["A"][:, ~np.isin(group, kept)] = 0.0
        out.append(objs)
    return out


def profiles(case):
    return {tuple(r) for r in case["ref"]["rank"].tolist()}


def summary(case):
    m = case["dims"].sum(axis=1)
    own = np.arange(case["lod"].shape[2])[None, None, :] < m[:, None, None]
    A = case["lod"][:, :case["n"], :]
    zeros = float(((A == 0.0) & own).sum()) / float(np.broadcast_to(own, A.shape).sum())
    cut = [(b, k) for b, k in cut_levels(case) if not leftover(case, b, k).any()]
    rank0 = int(((case["ref"]["rank"] == 0) & (case["dims"] > 0)).sum())
    return (f"    {case['name']:<13} {case['gen']:<10} n={case['n']:<4}{str(case['caps']).replace(' ', ''):<18} {case['kernel']:<36} zeros {zeros:4.2f}  kept {case['kept']:>2} / "
            f"{case['drawn']:<2}  rank 0 {rank0:>2}  cut {len(cut):>2} in {len({b for b, _ in cut}):>2} problems  profiles {len(profiles(case)):>2}  "
            f"max|x| {np.abs(case['ref']['x']).max():.1e}")


if __name__ == "__main__":
    for nm, g in cases():
        print(summary(build(nm, g)))
