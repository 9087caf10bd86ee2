"""A certificate of lexicographic optimality for LexLSI results, from the problem data and x alone.

A lexicographic least-squares problem with inequalities is a sequence of convex QPs: level k minimises |v_k|^2 over the points that keep the
violations v_j of every level j < k at their optimal values.  Given x, those points are the polyhedron {y : lb_j <= A_j y - v_j(x) <= ub_j, j < k}
(a point of it can only have smaller violations row by row, and x is optimal for the levels above, so it has the same ones), and x is optimal for
level k over a polyhedron iff its KKT conditions hold: multipliers mu on the rows of the earlier levels exist with

    g_k + sum_{j<k} A_j' mu_j = 0,   g_k = A_k' v_k,

mu >= 0 on a row that sits on its shifted upper bound, mu <= 0 on its shifted lower bound, free on both (an equality), 0 strictly inside.
certificate() looks for such multipliers with one LP per level and returns how far from zero the best ones leave the stationarity condition.
No active-set method runs, and nothing of this project is called: numpy and scipy.optimize.linprog(method="highs") only, A x, the violations and
the gradients in np.longdouble.  The LP finds ANY admissible multiplier, so degenerate working sets and rank-deficient levels raise no false alarm.

Beside the certificate: consistent() checks what a run reports (v, the working set) against x, lambda_check() checks returned multipliers
(LsiBatch.lambdas(), with_lambda=True) column by column without an LP, read_dat() reads the reference's ".dat" hierarchy files.

Out of scope (the certificate is not meant for them):
  * regularized runs: they solve a damped problem, not the stated one;
  * degenerate inputs whose bounds the cycling handler really relaxes: the relaxed bounds are not returned to the caller;
  * runs that stop on the factorization limit (status != 0).

The constants ACCEPT and ACCEPT_LAMBDA are measured, see below; tests/test_lexopt_certificate.py measures them again on every run."""
import numpy as np
from scipy.optimize import linprog

LD = np.longdouble

EPS_ON_BOUND = 1e-9  # "on a bound": within EPS_ON_BOUND * max(1, |bound|)
TOL_WRONG_SIGN_LAMBDA = 1e-8  # copy of ParametersLexLSI::tol_wrong_sign_lambda's default, include/lexls/typedefs.h:226 (lexls_amd/lexlsi.py:16)
TOL_CORRECT_SIGN_LAMBDA = 1e-12  # copy of tol_correct_sign_lambda's default, include/lexls/typedefs.h:227

# Acceptance bounds on the scaled stationarity residuals.  Measured on the CPU by tests/test_lexopt_certificate.py over every accepted case (the
# oracle-backed driver on all fixture families and run modes, and the reference's stored #Solution of tests/golden/test_01.dat), times 1000 as
# headroom for the LP solver and other seeds; the test asserts that each stays at least 100 x below the smallest value among the rejected cases.
#   certificate:  largest accepted 3.97e-11 (the 15-digit #Solution of test_01.dat; the oracle-backed driver's own solutions: 2.74e-13),
#                 smallest rejected 4.67e-4 (a run stopped one factorization early) -> ACCEPT = 4e-8, 1.2e4 x below it
#   lambda_check: largest accepted 5.74e-14, smallest rejected 8.83e-8 (1e-6 N(0,1) on the multipliers) -> ACCEPT_LAMBDA = 6e-11, 1.5e3 x below it
MEASURED_MAX_T = 4e-11
MEASURED_MIN_REJECTED_T = 4.67e-4
MEASURED_MAX_LAMBDA = 6e-14
MEASURED_MIN_REJECTED_LAMBDA = 8.83e-8
ACCEPT = 1000 * MEASURED_MAX_T
ACCEPT_LAMBDA = 1000 * MEASURED_MAX_LAMBDA


def rows_of(n, objectives):
    """per objective (A, lb, ub) in np.longdouble; simple bounds (var / lb / ub) become unit rows"""
    out = []
    for o in objectives:
        lb, ub = np.asarray(o["lb"], LD).ravel(), np.asarray(o["ub"], LD).ravel()
        if "var" in o:
            var = np.asarray(o["var"]).astype(np.int64).ravel()
            A = np.zeros((var.size, n), LD)
            A[np.arange(var.size), var] = 1
        else:
            A = np.asarray(o["A"], LD).reshape(lb.size, n)
        out.append((A, lb, ub))
    return out


def violations(rows, x):
    """-> ([A_k x], [v_k]): v = a x - ub above ub, a x - lb below lb, 0 inside"""
    x = np.asarray(x, LD)
    Ax = [A @ x for A, _, _ in rows]
    v = [np.where(ax > ub, ax - ub, np.where(ax < lb, ax - lb, LD(0))) for ax, (_, lb, ub) in zip(Ax, rows)]
    return Ax, v


def _scale(b):
    return np.maximum(LD(1), np.abs(b))


def multipliers_lp(B, g, lower, upper):
    """min t  s.t.  |g + B' mu|_inf <= t,  lower <= mu <= upper (+-inf allowed), as float64 in HiGHS; -> (t, mu) with t evaluated again in
    np.longdouble at the returned mu clipped to its bounds, so that no tolerance of the LP solver enters the result"""
    p, n = B.shape
    g64, B64 = np.asarray(g, np.float64), np.asarray(B, np.float64)
    c = np.zeros(p + 1)
    c[p] = 1.0
    A_ub = np.block([[B64.T, -np.ones((n, 1))], [-B64.T, -np.ones((n, 1))]])
    b_ub = np.concatenate([-g64, g64])
    bounds = [(None if np.isinf(lo) else float(lo), None if np.isinf(hi) else float(hi)) for lo, hi in zip(lower, upper)] + [(0.0, None)]
    res = linprog(c, A_ub=A_ub, b_ub=b_ub, bounds=bounds, method="highs",
                  options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10))
    mu = np.zeros(p) if res.x is None else res.x[:p]  # (mu = 0 is admissible: the relaxed sign bounds contain it)
    mu = np.clip(mu, lower, upper)
    return np.max(np.abs(g + B.T @ mu.astype(LD))), mu


def certificate(n, objectives, x, details=False):
    """-> array of t_k / max(1, |g_k|_inf), one per level: 0 (up to rounding) iff x is lexicographically optimal.  details=True: also the
    list of per-level dicts (g, rows, mu)"""
    rows = rows_of(n, objectives)
    Ax, v = violations(rows, x)
    out, info = [], []
    B, lower, upper = np.zeros((0, n), LD), np.zeros(0), np.zeros(0)
    for k, (A, lb, ub) in enumerate(rows):
        g = A.T @ v[k]
        gmax = np.max(np.abs(g)) if g.size else LD(0)
        if B.shape[0]:
            t, mu = multipliers_lp(B, g, lower, upper)
        else:
            t, mu = gmax, np.zeros(0)
        out.append(float(t / max(LD(1), gmax)))
        info.append(dict(g=g, t=t, mu=mu, rows=B.shape[0]))
        # the rows of this level as constraints of the levels below: bounds shifted by the violation at x
        on_ub = np.abs(Ax[k] - (ub + v[k])) <= EPS_ON_BOUND * _scale(ub)
        on_lb = np.abs(Ax[k] - (lb + v[k])) <= EPS_ON_BOUND * _scale(lb)
        keep = on_ub | on_lb
        lo = np.where(on_lb, -np.inf, -TOL_WRONG_SIGN_LAMBDA)  # on the lower bound: mu <= 0, relaxed; on both: free
        hi = np.where(on_ub, np.inf, TOL_WRONG_SIGN_LAMBDA)
        B = np.vstack([B, A[keep]])
        lower, upper = np.concatenate([lower, lo[keep]]), np.concatenate([upper, hi[keep]])
    return (np.array(out), info) if details else np.array(out)


def consistent(n, objectives, x, active, v):
    """What a run reports against its own x.  `active`, `v`: per objective, or flat over the stacked objectives.  -> dict of figures, every one
    of which a correct run keeps within EPS_ON_BOUND (assert_consistent):
      v_error            max |v - violation derived from x| / max(1, |lb|, |ub|)
      active_off_bound   max over active rows |a x - v - bound| / max(1, |bound|), bound = lb (type 1), ub (type 2, 3); type 3 needs lb == ub
      inactive_v         max |v| over inactive rows (must be exactly 0)
      inactive_margin    min over inactive rows of min(a x - lb, ub - a x) / max(1, |lb|, |ub|) (must be > 0: strictly inside)
      bad_types          rows whose type is not one of 0..3, or 3 with lb != ub"""
    rows = rows_of(n, objectives)
    Ax, viol = violations(rows, x)
    dims = [r[1].size for r in rows]
    cuts = np.cumsum(dims)[:-1]
    if not isinstance(active, (list, tuple)):
        active = np.split(np.asarray(active).ravel(), cuts)
    if not isinstance(v, (list, tuple)):
        v = np.split(np.asarray(v).ravel(), cuts)
    fig = dict(v_error=0.0, active_off_bound=0.0, inactive_v=0.0, inactive_margin=np.inf, bad_types=0)
    for (A, lb, ub), ax, w, act, vr in zip(rows, Ax, viol, active, v):
        act, vr = np.asarray(act).astype(np.int64), np.asarray(vr, LD)
        s = np.maximum(_scale(lb), _scale(ub))
        fig["v_error"] = max(fig["v_error"], float(np.max(np.abs(vr - w) / s, initial=0)))
        fig["bad_types"] += int(np.sum((act < 0) | (act > 3) | ((act == 3) & (lb != ub))))
        on_lb, on_ub, off = act == 1, (act == 2) | (act == 3), act == 0
        fig["active_off_bound"] = max(fig["active_off_bound"], float(np.max(np.abs(ax - vr - lb)[on_lb] / _scale(lb)[on_lb], initial=0)),
                                      float(np.max(np.abs(ax - vr - ub)[on_ub] / _scale(ub)[on_ub], initial=0)))
        fig["inactive_v"] = max(fig["inactive_v"], float(np.max(np.abs(vr[off]), initial=0)))
        fig["inactive_margin"] = min(fig["inactive_margin"], float(np.min((np.minimum(ax - lb, ub - ax) / s)[off], initial=np.inf)))
    return fig


def assert_consistent(fig, what=""):
    assert fig["bad_types"] == 0, (what, fig)
    assert fig["v_error"] <= EPS_ON_BOUND, (what, fig)
    assert fig["active_off_bound"] <= EPS_ON_BOUND, (what, fig)
    assert fig["inactive_v"] == 0.0, (what, fig)
    assert fig["inactive_margin"] > 0.0, (what, fig)


def lambda_check(n, objectives, x, active, lam):
    """Returned multipliers against x, without an LP.  `lam`: per objective the (dim_k x nObj) matrix of LexLSI::getLambda (LsiBatch.lambdas(),
    frontend debug output), or the stacked (total x nObj) matrix; row = constraint in the caller's order, column k = the multipliers of level
    k's problem (layout and signs as in test_multipliers_are_the_dual_of_the_lexicographic_problem, tests/test_oracle_golden.py: block k of
    column k is the level's own residual, sum_{j<=k} A_j' Lambda_j[:, k] = 0, the blocks below are zero).  With simple bounds in objective 0 the
    driver leaves column 0 zero (its level holds no least-squares problem of the equality solver); then g_0 = 0 is checked instead.
    -> dict:
      stationarity   max over columns k of |g_k + sum_{j<k} A_j' Lambda_j[:, k]|_inf / max(1, |g_k|_inf), g_k from x, not from Lambda
      own_block      max over k of |Lambda_k[:, k] - v_k(x)| on active rows / max(1, |lb|, |ub|)
      wrong_sign     the largest wrong-sign multiplier on an inequality row of an earlier level (type 2: -Lambda, type 1: +Lambda), over the rows
                     the lexicographic rule still constrains in column k: a row whose multiplier had the correct sign by more than
                     tol_correct_sign_lambda in an earlier column (its own level's included) is an implicit equality for the levels below and its
                     multiplier there is free — the rule LexLSE::ObjectiveSensitivity applies (CORRECT_SIGN_OF_LAMBDA).  This is the same rule
                     the driver uses: a mistake in that rule itself would pass here and is left to certificate(), whose LP knows no such mark
      stray          max |Lambda| where it must be zero: inactive rows, and the blocks of levels below k in column k"""
    rows = rows_of(n, objectives)
    Ax, viol = violations(rows, x)
    dims = [r[1].size for r in rows]
    cuts = np.cumsum(dims)[:-1]
    L = np.vstack([np.asarray(m) for m in lam]) if isinstance(lam, (list, tuple)) else np.asarray(lam)
    L = L.astype(LD)
    nobj = len(rows)
    assert L.shape == (sum(dims), nobj), L.shape
    act = np.concatenate([np.asarray(a).astype(np.int64).ravel() for a in active]) if isinstance(active, (list, tuple)) else np.asarray(active).astype(np.int64).ravel()
    M = np.vstack([r[0] for r in rows])
    level = np.concatenate([np.full(d, k) for k, d in enumerate(dims)])
    vflat = np.concatenate(viol)
    s = np.concatenate([np.maximum(_scale(lb), _scale(ub)) for _, lb, ub in rows])
    first = 1 if "var" in objectives[0] else 0
    fig = dict(stationarity=0.0, own_block=0.0, wrong_sign=0.0, stray=0.0)
    settled = np.zeros(L.shape[0], bool)  # rows with a multiplier of the correct sign beyond tol_correct_sign_lambda in an earlier column
    for k, (A, lb, ub) in enumerate(rows):
        g = A.T @ viol[k]
        gs = max(LD(1), np.max(np.abs(g), initial=0))
        col = L[:, k]
        if k < first:
            fig["stationarity"] = max(fig["stationarity"], float(np.max(np.abs(g), initial=0) / gs))
            fig["stray"] = max(fig["stray"], float(np.max(np.abs(col), initial=0)))
            continue
        above, own, below = level < k, level == k, level > k
        r = g + M[above].T @ col[above]
        fig["stationarity"] = max(fig["stationarity"], float(np.max(np.abs(r), initial=0) / gs))
        own_active = own & (act != 0)
        fig["own_block"] = max(fig["own_block"], float(np.max((np.abs(col - vflat) / s)[own_active], initial=0)))
        fig["stray"] = max(fig["stray"], float(np.max(np.abs(col[below | (act == 0)]), initial=0)))
        signed = np.where(act == 2, col, np.where(act == 1, -col, LD(0)))  # > 0: correct sign
        checked = (above | own) & ((act == 1) | (act == 2)) & ~settled
        fig["wrong_sign"] = max(fig["wrong_sign"], float(np.max(-signed[checked], initial=0)))
        settled |= (above | own) & (signed > TOL_CORRECT_SIGN_LAMBDA)
    return fig


def assert_lambda(fig, what=""):
    assert fig["stationarity"] <= ACCEPT_LAMBDA, (what, fig)
    assert fig["own_block"] <= EPS_ON_BOUND, (what, fig)
    assert fig["wrong_sign"] <= TOL_WRONG_SIGN_LAMBDA, (what, fig)
    assert fig["stray"] == 0.0, (what, fig)


def read_dat(path, one_based=True):
    """The reference's ASCII hierarchy format (include/lexls/tools.h:22-31): header fields #nVar, #nObj, #nCtr (list), #HierType (200
    inequalities, 210 inequalities with a trailing activation flag per row), #ObjType (100 simple bounds, 200 general), then "#OBJECTIVE k"
    blocks of rows [a_1..a_n lb ub] or [var lb ub], then optional #SolGuess / #Solution.  `one_based`: how the file stores the variable
    indices of simple bounds.  -> dict(n, objectives (the dict form of P.lsi_problem), guess or None, solution or None)"""
    with open(path) as f:
        lines = [ln.strip() for ln in f]
    head, i = {}, 0
    while len(head) < 5 and i < len(lines):
        key = lines[i].replace(" ", "")
        if key in ("#nVar", "#nObj", "#nCtr", "#HierType", "#ObjType"):
            i += 1
            while not lines[i]:
                i += 1
            head[key] = [int(t) for t in lines[i].split()]
        i += 1
    n, nobj, htype = head["#nVar"][0], head["#nObj"][0], head["#HierType"][0]
    if htype not in (200, 210) or len(head["#nCtr"]) != nobj or len(head["#ObjType"]) != nobj:
        raise ValueError("unsupported or inconsistent header")
    objectives = []
    for k in range(nobj):
        while not lines[i].replace(" ", "").startswith("#OBJECTIVE"):
            i += 1
        i += 1
        m, simple = head["#nCtr"][k], head["#ObjType"][k] == 100
        ncols = 3 if simple else n + 2
        block = np.array([[float(t) for t in lines[i + r].split()[:ncols]] for r in range(m)]).reshape(m, ncols)
        i += m
        if simple:
            objectives.append(dict(var=(np.rint(block[:, 0]).astype(np.int64) - (1 if one_based else 0)).astype(np.uint32), lb=block[:, 1].copy(), ub=block[:, 2].copy()))
        else:
            objectives.append(dict(A=block[:, :n].copy(), lb=block[:, n].copy(), ub=block[:, n + 1].copy()))
    out = dict(n=n, objectives=objectives, guess=None, solution=None)
    tail = " ".join(lines[i:]).split("#")
    for part in tail:
        name, _, body = part.partition(" ")
        if name in ("SolGuess", "Solution"):
            out["guess" if name == "SolGuess" else "solution"] = np.array([float(t) for t in body.split()[:n]])
    return out
