"""Batches that hold the hand-written DECISIONS of the resident LexLSI iterations to the oracle-backed driver where P.lsi_problem never takes them
(tests/test_gpu_lsi_decisions.py runs them on the GPU, tests/test_lsi_decision_cases.py asserts the conditions below on the CPU, from the oracle
alone).  Every other LexLSI batch of the suite is P.lsi_problem as it stands — dense N(0,1) rows, intervals of width U(0,1), entries of order 1,
default tolerances — or a repeated row whose interval was moved, which conflicts by construction.  So the ratio test has never had to break a tie
between equal POSITIVE ratios, the four tolerances have reached the device at their defaults only, num / den has only seen numbers near 1 and a
middle level has only held two-sided intervals on dense rows.

Shapes (8 instances each, seeds start .. start + 7, nothing dropped):
    general  n = 12, (4, 5, 4, 6)         level 0 general rows
    ik       n = 40, 5 x 12               level 0 simple bounds; lsi_fused<lqr_wave<41,12...>>
    wide     n = 57, (12, 16, 16, 16, 16) level 0 simple bounds; the 64 x 16 instantiation, 76 rows in all
    cols46   n = 45, 5 x 12               level 0 simple bounds; 46 columns: the stage path
    tall     n = 8, (4, 72, 4)            level 0 general rows; rows c and c + 64 of level 1 are rows 4 + c and 68 + c of the instance, visited by
                                          the same lane of lsi_step_wave in successive trips: the one place where that lane's own `ratio == best`
                                          branch decides between two rows that can both be blocking
last_kernel() as measured on MI355X, default / no_fused (host: "host"; the other paths as default): general lsi_fused<lqr_wave<41,12>> /
lqr_wave<41,12>, ik lsi_fused<lqr_wave<41,12,exact>> / lqr_wave<41,12,exact>, wide lsi_fused<lqr_wave<64,16>> / lqr_wave<64,16>, cols46
lqr_quad<3,12,factor,fixed> on both, and `tall` lqr_generic<256,lds> on both: a level of 72 rows is not served by the persistent launch, so its
resident iterations run lsi_step_wave behind the lock-step stages.  (The route that serves `tall` was not read from the code and is not asserted.)

Families.  G0, G1 are the first and second general objective that is not the last one (general, tall: levels 0, 1; the others: levels 1, 2); the
last level (equalities) is left alone except under the scalings, which are changes of units of whole columns and rows.
  twins      rows that repeat another inequality row exactly, A, lb and ub (PAIRS).  Identical data and an identical history give bit-identical
             v, A x, A dx, hence a bit-identical ratio: when one of a pair becomes blocking, so does the other, at the same value.
                 same      G0 row 1 := G0 row 0                            same level: the inactive list's order decides
                 cross     G1 row 0 := G0 row 2                            the objective decides
                 reversed  G1 row 3 := G1 row LAST                         the copy sits at the LOWER index.  An ADD moves the LAST entry of the
                                                                           inactive list into the gap (workingset.h: swap with last), so once a row
                                                                           in front of row 3 has joined, the last row stands before row 3 in the list
                                                                           and behind it by index: this kind shows which order is followed
                 mirror    G1 row 2 := -(G1 row 1) with [-ub, -lb]         equal ratios if every rounding is sign-symmetric; LB <-> UB
                 unit      G0 row 5 := e_j, j = var[0], both with           shapes with simple bounds: ties with the bound on x_j across the two
                           [-UNIT_BOUND, UNIT_BOUND]                        branches of the step (x_j read directly / an A dx chain that is exact).
                                                                           P.lsi_problem's [-1, 1] binds in one instance in eight of `wide` and the
                                                                           bound on var[0] in fewer: the bound of this one variable is narrowed
                 lane_a    G1 row 69 := G1 row 5                           tall only: the same lane, the copy behind
                 lane_b    G1 row 6 := G1 row 70                           tall only: the same lane, the copy in front
             Evidence of a tie is the oracle's working-set log alone (replay): a VIRGIN tie is an ADD of one of a pair while its partner is
             inactive and neither has been active before in this run.  Later ADDs with an inactive partner that has a past are counted apart
             ("later") and asserted on nowhere: their v may differ.
  tol_*      unchanged P.lsi_problem data under ONE non-default parameter at a time (TOLERANCES).
  decades    column j of every general objective times s_j = 10^U(-2, 2), the simple bounds on x_j divided by s_j (x_j is measured in another
             unit), then every general row with its bounds times 10^U(-2, 2), the last level included.
  pow2_up / pow2_down   every general row with its bounds times 2^+20 / 2^-20, the last level included.  The driver's tolerances are absolute, so
             the oracle takes other and much longer trajectories; max_number_of_factorizations stays 200.
  kinds      in every general level but the last: row 0 an equality (ub := lb), row 1 one-sided below (ub = +1e10), row 2 one-sided above
             (lb = -1e10), row 3 all zeros with lb < 0 < ub, and on levels of at least 5 rows row 4 all zeros with 0 < lb < ub: a violation
             nothing can remove.

Seeds: every (family, shape) takes the first start of its series BASE + 1000 * (index of the shape) + 100 * j, j = 0, 1, ..., at which the
conditions of tests/test_lsi_decision_cases.py hold (`python tests/lsi_decision_cases.py --search` prints the search); STARTS holds the results
that are not j = 0.

MEASURED on the oracle (`python tests/lsi_decision_cases.py`):
    twins   general seeds 41000+8  status 0: 8 / 8  log entries 11-15  zero-step ADDs 4-7
            virgin ties, instances (low / high first; later ADDs): same 6 (6 / 0; 1)  cross 7 (7 / 0; 5)  reversed 8 (2 / 6; 1)  mirror 8 (8 / 0; 1)
            first_wrong_sign: status 0 8 / 8, virgin ties same 6  cross 7  reversed 8  mirror 8
            warm: status 0 8 / 8, virgin ties same 1  cross 0  reversed 2  mirror 2
    twins   ik      seeds 42000+8  status 0: 8 / 8  log entries 34-59  zero-step ADDs 17-26
            virgin ties, instances (low / high first; later ADDs): same 8 (8 / 0; 3)  cross 8 (8 / 0; 1)  reversed 8 (4 / 4; 0)  mirror 7 (7 / 0; 1)  unit 8 (8 / 0; 3)
            first_wrong_sign: status 0 6 / 8, virgin ties same 8  cross 8  reversed 8  mirror 8  unit 7
            warm: status 0 8 / 8, virgin ties same 1  cross 1  reversed 1  mirror 1  unit 1
    twins   wide    seeds 43000+8  status 0: 8 / 8  log entries 43-75  zero-step ADDs 24-34
            virgin ties, instances (low / high first; later ADDs): same 8 (8 / 0; 0)  cross 8 (8 / 0; 1)  reversed 8 (3 / 5; 1)  mirror 8 (8 / 0; 1)  unit 8 (8 / 0; 3)
            first_wrong_sign: status 0 8 / 8, virgin ties same 8  cross 8  reversed 8  mirror 8  unit 8
            warm: status 0 8 / 8, virgin ties same 0  cross 1  reversed 1  mirror 4  unit 0
    twins   cols46  seeds 44000+8  status 0: 8 / 8  log entries 30-49  zero-step ADDs 18-27
            virgin ties, instances (low / high first; later ADDs): same 8 (8 / 0; 0)  cross 8 (8 / 0; 0)  reversed 8 (1 / 7; 0)  mirror 8 (8 / 0; 0)  unit 7 (7 / 0; 0)
            first_wrong_sign: status 0 8 / 8, virgin ties same 8  cross 8  reversed 8  mirror 8  unit 7
            warm: status 0 8 / 8, virgin ties same 2  cross 3  reversed 1  mirror 0  unit 0
    twins   tall    seeds 45000+8  status 0: 8 / 8  log entries 69-90  zero-step ADDs 31-53
            virgin ties, instances (low / high first; later ADDs): same 8 (8 / 0; 0)  cross 7 (7 / 0; 0)  reversed 8 (7 / 1; 0)  mirror 8 (8 / 0; 0)  lane_a 8 (4 / 4; 0)  lane_b 8 (5 / 3; 0)
            first_wrong_sign: status 0 8 / 8, virgin ties same 8  cross 7  reversed 8  mirror 8  lane_a 8  lane_b 8
            warm: status 0 8 / 8, virgin ties same 0  cross 4  reversed 0  mirror 0  lane_a 0  lane_b 0
    tol_wrong_sign_1e-1         changed instances of 8: general 5  ik 6  wide 8  cols46 8  tall 5   at the limit: general 0  ik 0  wide 0  cols46 0  tall 0
    tol_correct_sign_1e-1       changed instances of 8: general 1  ik 0  wide 0  cols46 0  tall 8   at the limit: general 1  ik 0  wide 0  cols46 0  tall 8
    tol_linear_dependence_1e-1  changed instances of 8: general 5  ik 3  wide 5  cols46 5  tall 3   at the limit: general 3  ik 1  wide 1  cols46 2  tall 0
    tol_feasibility_1e-1        changed instances of 8: general 3  ik 8  wide 8  cols46 8  tall 8   at the limit: general 0  ik 0  wide 0  cols46 0  tall 0
    tol_wrong_sign_0 (dropped)  changed instances of 8: general 0  ik 0  wide 0  cols46 0  tall 0   at the limit: general 0  ik 0  wide 0  cols46 0  tall 0
    decades   general seeds 41000+8  status 0: 8  at the limit: 0  other: 0  log entries 17-46
    decades   ik      seeds 42000+8  status 0: 7  at the limit: 1  other: 0  log entries 117-200
    decades   wide    seeds 43000+8  status 0: 4  at the limit: 4  other: 0  log entries 117-200
    decades   cols46  seeds 44000+8  status 0: 7  at the limit: 1  other: 0  log entries 57-200
    decades   tall    seeds 45000+8  status 0: 8  at the limit: 0  other: 0  log entries 81-104
    pow2_up   general seeds 41000+8  status 0: 8  at the limit: 0  other: 0  log entries 19-27
    pow2_up   ik      seeds 42000+8  status 0: 8  at the limit: 0  other: 0  log entries 54-76
    pow2_up   wide    seeds 43000+8  status 0: 8  at the limit: 0  other: 0  log entries 49-106
    pow2_up   cols46  seeds 44000+8  status 0: 8  at the limit: 0  other: 0  log entries 41-72
    pow2_up   tall    seeds 45000+8  status 0: 8  at the limit: 0  other: 0  log entries 63-98
    pow2_down general seeds 41000+8  status 0: 4  at the limit: 4  other: 0  log entries 13-200
    pow2_down ik      seeds 42000+8  status 0: 2  at the limit: 6  other: 0  log entries 53-200
    pow2_down wide    seeds 43100+8  status 0: 4  at the limit: 4  other: 0  log entries 74-200
    pow2_down cols46  seeds 44000+8  status 0: 5  at the limit: 3  other: 0  log entries 39-200
    pow2_down tall    seeds 45300+8  status 0: 5  at the limit: 3  other: 0  log entries 67-200
    kinds     general seeds 41000+8  status 0: 8  at the limit: 0  other: 0  log entries 1-6
    kinds     ik      seeds 42000+8  status 0: 8  at the limit: 0  other: 0  log entries 24-49
    kinds     wide    seeds 43000+8  status 0: 8  at the limit: 0  other: 0  log entries 38-47
    kinds     cols46  seeds 44000+8  status 0: 8  at the limit: 0  other: 0  log entries 23-30
    kinds     tall    seeds 45000+8  status 0: 8  at the limit: 0  other: 0  log entries 62-105
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

SHAPES = {
    "general": dict(n=12, dims=[4, 5, 4, 6], simple_bounds=False),
    "ik": dict(n=40, dims=[12] * 5, simple_bounds=True),
    "wide": dict(n=57, dims=[12, 16, 16, 16, 16], simple_bounds=True),
    "cols46": dict(n=45, dims=[12] * 5, simple_bounds=True),
    "tall": dict(n=8, dims=[4, 72, 4], simple_bounds=False),
}
BATCH = 8
BASE = 41000
STARTS = {("pow2_down", "wide"): 1, ("pow2_down", "tall"): 3}  # (family, shape) -> j of the series above, where it is not 0
MAX_FACTORIZATIONS = 200  # the default; the long runs of pow2_down end on it
AT_THE_LIMIT = 2          # TerminationStatus MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED
PERTURB = 0.05            # the warm-start neighbour, as tests/test_lexopt_certificate.py
LOG_CAPACITY = 256        # entries per instance the GPU file asks for: above every log here (MAX_FACTORIZATIONS entries at the most)

# one parameter off its default at a time.  tol_feasibility: 1e-3 changes nothing on any shape, 1e-2 changes 0-2 instances of four shapes and 5 of
# tall, 1e-1 changes every shape (the table)
TOLERANCES = {
    "tol_wrong_sign_1e-1": dict(tol_wrong_sign_lambda=1e-1),
    "tol_correct_sign_1e-1": dict(tol_correct_sign_lambda=1e-1),
    "tol_linear_dependence_1e-1": dict(tol_linear_dependence=1e-1),
    "tol_feasibility_1e-1": dict(tol_feasibility=1e-1),
}
# a set that changes neither log nor final working set of any instance of any shape proves nothing and is not run (tests/test_lsi_decision_cases.py
# asserts that it still changes nothing).  0 has no decade to move to; 1e-12 and 1e-6 change nothing either, 1e-4 one instance of wide, 1e-2 1-5
# per shape, and 1e-1 is a set of its own
DROPPED_SETS = {"tol_wrong_sign_0": dict(tol_wrong_sign_lambda=0.0)}
SCALED = ("decades", "pow2_up", "pow2_down")
FAMILIES = ["twins", *TOLERANCES, *SCALED, "kinds"]

# twins: kind -> ((objective, row) that is copied, (objective, row) that becomes the copy); objectives as indices into general_levels()
PAIRS = {
    "same": ((0, 0), (0, 1)),
    "cross": ((0, 2), (1, 0)),
    "reversed": ((1, "last"), (1, 3)),
    "mirror": ((1, 1), (1, 2)),
    "unit": (("bound", 0), (0, 5)),
    "lane_a": ((1, 5), (1, 69)),
    "lane_b": ((1, 70), (1, 6)),
}
SAME_LANE = ("lane_a", "lane_b")
UNIT_BOUND = 0.1
DROPPED_KINDS = {}  # kind -> why (none: the oracle shows virgin ties of every kind, mirror included)


def general_levels(shape):
    """the general objectives that are not the last one"""
    s = SHAPES[shape]
    return list(range(1 if s["simple_bounds"] else 0, len(s["dims"]) - 1))


def kinds_of(shape):
    """the pair kinds a shape holds"""
    s = SHAPES[shape]
    out = ["same", "cross", "reversed", "mirror"]
    if s["simple_bounds"]:
        out.append("unit")
    if shape == "tall":
        out += list(SAME_LANE)
    return [k for k in out if k not in DROPPED_KINDS]


def pairs_of(shape):
    """kind -> ((objective, row), (objective, row)) in the problem's own objective numbers, source first"""
    G = general_levels(shape)
    dims = SHAPES[shape]["dims"]
    at = lambda ref: (0, ref[1]) if ref[0] == "bound" else (G[ref[0]], dims[G[ref[0]]] - 1 if ref[1] == "last" else ref[1])
    return {kind: (at(PAIRS[kind][0]), at(PAIRS[kind][1])) for kind in kinds_of(shape)}


def start_of(family, shape):
    return BASE + 1000 * list(SHAPES).index(shape) + 100 * STARTS.get((family, shape), 0)


def base_problem(shape, seed, perturb=0.0):
    s = SHAPES[shape]
    return P.lsi_problem(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"], perturb=perturb)


# ---- the generators: each changes the objectives of one P.lsi_problem in place and returns them ---------------------------------------------------
def twins(shape, objs):
    n = SHAPES[shape]["n"]
    for kind, ((ko, ro), (kc, rc)) in pairs_of(shape).items():
        src, dst = objs[ko], objs[kc]
        if kind == "unit":
            src["lb"][ro], src["ub"][ro] = -UNIT_BOUND, UNIT_BOUND
            dst["A"][rc] = 0.0
            dst["A"][rc, int(src["var"][ro])] = 1.0
            dst["lb"][rc], dst["ub"][rc] = src["lb"][ro], src["ub"][ro]
        elif kind == "mirror":
            dst["A"][rc] = -src["A"][ro]
            dst["lb"][rc], dst["ub"][rc] = -src["ub"][ro], -src["lb"][ro]
        else:
            dst["A"][rc] = src["A"][ro]
            dst["lb"][rc], dst["ub"][rc] = src["lb"][ro], src["ub"][ro]
        assert dst["A"].shape[1] == n
    return objs


def decade_scales(seed, n, rows):
    """column scales (n,), row scales (rows,): 10^U(-2, 2) each, streams of their own"""
    return 10.0 ** (4.0 * P.uniform(seed, n, 4100) - 2.0), 10.0 ** (4.0 * P.uniform(seed, rows, 4101) - 2.0)


def decades(shape, objs, seed):
    n = SHAPES[shape]["n"]
    col, row = decade_scales(seed, n, sum(len(o["lb"]) for o in objs))
    first = 0
    for o in objs:
        m = len(o["lb"])
        if "var" in o:
            o["lb"], o["ub"] = o["lb"] / col[o["var"]], o["ub"] / col[o["var"]]
        else:
            r = row[first:first + m]
            o["A"] = o["A"] * col[None, :] * r[:, None]
            o["lb"], o["ub"] = o["lb"] * r, o["ub"] * r
        first += m
    return objs


def pow2(objs, k):
    for o in objs:
        if "A" in o:
            for key in ("A", "lb", "ub"):
                o[key] = np.ldexp(o[key], k)
    return objs


def kinds(shape, objs):
    for k in general_levels(shape):
        o = objs[k]
        w = 0.5 * (o["ub"] - o["lb"])  # the half widths U(0, 1) of P.lsi_problem
        o["ub"][0] = o["lb"][0]
        o["ub"][1] = 1e10
        o["lb"][2] = -1e10
        o["A"][3] = 0.0
        o["lb"][3], o["ub"][3] = -(0.25 + w[3]), 0.25 + w[3]
        if len(o["lb"]) >= 5:
            o["A"][4] = 0.0
            o["lb"][4], o["ub"][4] = 0.25 + w[4], 0.5 + 2.0 * w[4]
    return objs


def unsatisfiable_rows(shape):
    """(objective, row) of the all-zero rows of `kinds` whose interval does not hold 0"""
    return [(k, 4) for k in general_levels(shape) if SHAPES[shape]["dims"][k] >= 5]


def generate(family, shape, seed, perturb=0.0):
    objs = base_problem(shape, seed, perturb)
    if family == "twins":
        return twins(shape, objs)
    if family == "decades":
        return decades(shape, objs, seed)
    if family in ("pow2_up", "pow2_down"):
        return pow2(objs, 20 if family == "pow2_up" else -20)
    if family == "kinds":
        return kinds(shape, objs)
    assert family in TOLERANCES or family in DROPPED_SETS, family
    return objs


def params_of(family):
    return dict(TOLERANCES.get(family, DROPPED_SETS.get(family, {})))


@functools.lru_cache(maxsize=None)
def problems(family, shape, start=None, perturb=0.0):
    """the batch of a family on a shape (perturb = 0) or its warm-start neighbours; made once, shared, never modified"""
    start = start_of(family, shape) if start is None else start
    out = [generate(family, shape, start + i, perturb) for i in range(BATCH)]
    for objs in out:
        for o in objs:
            for a in o.values():
                a.setflags(write=False)
    return out


def split(shape, a):
    return np.split(np.asarray(a), np.cumsum(SHAPES[shape]["dims"])[:-1])


@functools.lru_cache(maxsize=None)
def warm_start(family, shape, start=None):
    """-> (guess, x0), each (batch, ...): working set and x of every instance's neighbour (right-hand sides perturbed by PERTURB) from the
    oracle-backed driver, as test_lexopt_certificate.warm_start_of: equality flags are not part of a guess"""
    n = SHAPES[shape]["n"]
    rs = [oracle.lsi_run(n, p) for p in problems(family, shape, start, PERTURB)]
    active = np.stack([np.concatenate(r["active"]) for r in rs])
    guess, x0 = np.where(active == 3, 0, active).astype(np.uint8), np.stack([r["x"] for r in rs])
    guess.setflags(write=False)
    x0.setflags(write=False)
    return guess, x0


MODES = {"cold": {}, "first_wrong_sign": dict(deactivate_first_wrong_sign=1), "warm": {}}


@functools.lru_cache(maxsize=None)
def refs(family, shape, mode="cold", start=None, default_parameters=False):
    """per instance the oracle-backed driver's debug run (x, info, active, v, debug) with ["log"] = its working-set log; computed once per key,
    shared, never modified.  default_parameters: the family's data under the default parameters (what a tol_* run is compared with)"""
    n, out = SHAPES[shape]["n"], []
    par = dict(MODES[mode], **({} if default_parameters else params_of(family)))
    for i, p in enumerate(problems(family, shape, start)):
        kw = {}
        if mode == "warm":
            guess, x0 = warm_start(family, shape, start)
            kw = dict(active_guess=split(shape, guess[i]), x0=x0[i])
        o = oracle.lsi_run_debug(n, p, **kw, **par)
        o["log"] = o["debug"]["working_set_log"]
        out.append(o)
    return out


# ---- what the oracle's logs show ---------------------------------------------------------------------------------------------------------------
def replay(log, pairs):
    """kind -> dict(virgin, later, first): ADDs of one of the pair while the partner is inactive, with neither active before in this run (virgin) or
    not (later); first = which of the pair the virgin ADD took, "low" / "high" by (objective, row)"""
    out = {kind: dict(virgin=0, later=0, first=None) for kind in pairs}
    active, ever = set(), set()
    for e in log:
        row = (e["obj_index"], e["ctr_index"])
        if e["ctr_type"] == 0:  # REMOVE
            active.discard(row)
            continue
        for kind, pair in pairs.items():
            if row in pair:
                partner = pair[1] if row == pair[0] else pair[0]
                if partner not in active:
                    if row not in ever and partner not in ever:
                        out[kind]["virgin"] += 1
                        out[kind]["first"] = "low" if row < partner else "high"
                    else:
                        out[kind]["later"] += 1
        active.add(row)
        ever.add(row)
    return out


def zero_step_adds(log):
    return sum(1 for e in log if e["ctr_type"] != 0 and e["alpha_or_lambda"] == 0.0)


def tie_counts(shape, mode="cold", start=None):
    """kind -> dict(instances with a virgin tie, low / high: which of the pair it took, later: ADDs counted apart)"""
    pairs = pairs_of(shape)
    per = [replay(o["log"], pairs) for o in refs("twins", shape, mode, start)]
    return {kind: dict(instances=sum(r[kind]["virgin"] > 0 for r in per), low=sum(r[kind]["first"] == "low" for r in per),
                       high=sum(r[kind]["first"] == "high" for r in per), later=sum(r[kind]["later"] for r in per)) for kind in pairs}


def changed(family, shape, start=None):
    """the instances whose log or final working set differs between the family's parameters and the defaults, on the same data"""
    a, b = refs(family, shape, "cold", start), refs(family, shape, "cold", start, True)
    return [i for i, (u, v) in enumerate(zip(a, b)) if u["log"] != v["log"] or not np.array_equal(np.concatenate(u["active"]), np.concatenate(v["active"]))]


def statuses(family, shape, mode="cold", start=None):
    return [o["info"]["status"] for o in refs(family, shape, mode, start)]


def kinds_hold(shape, start=None):
    """kinds: at least half of the batch ends with status 0, and in each of those every unsatisfiable zero row is active with non-zero v"""
    rs = refs("kinds", shape, "cold", start)
    solved = [o for o in rs if o["info"]["status"] == 0]
    return 2 * len(solved) >= BATCH and all(o["active"][k][r] != 0 and o["v"][k][r] != 0.0 for o in solved for k, r in unsatisfiable_rows(shape))


def holds(family, shape, start=None):
    """the condition of tests/test_lsi_decision_cases.py that picks the seeds of a (family, shape); the tolerance sets are judged over all shapes"""
    st = statuses(family, shape, "cold", start)
    if family == "twins":
        t = tie_counts(shape, "cold", start)
        return (not any(st) and all(2 * c["instances"] >= BATCH for c in t.values()) and t["reversed"]["low"] > 0 and t["reversed"]["high"] > 0)
    if family in ("decades", "pow2_up"):
        return 2 * st.count(0) >= BATCH
    if family == "pow2_down":
        return 4 * st.count(AT_THE_LIMIT) >= BATCH
    if family == "kinds":
        return kinds_hold(shape, start)
    return True


def search(limit=40):
    for family in FAMILIES:
        for shape in SHAPES:
            base = BASE + 1000 * list(SHAPES).index(shape)
            j = next((j for j in range(limit) if holds(family, shape, base + 100 * j)), None)
            print(f"    {family:<28}{shape:<9}j = {j}" + ("" if j == STARTS.get((family, shape), 0) else "   <-- STARTS differs"))


def _span(values):
    return f"{min(values)}-{max(values)}"


def table():
    lines = []
    for shape in SHAPES:
        rs, t = refs("twins", shape), tie_counts(shape)
        lines.append(f"    twins   {shape:<8}seeds {start_of('twins', shape)}+8  status 0: {statuses('twins', shape).count(0)} / 8  log entries {_span([len(o['log']) for o in rs])}"
                     f"  zero-step ADDs {_span([zero_step_adds(o['log']) for o in rs])}")
        lines.append("            virgin ties, instances (low / high first; later ADDs): " +
                     "  ".join(f"{k} {c['instances']} ({c['low']} / {c['high']}; {c['later']})" for k, c in t.items()))
        for mode in ("first_wrong_sign", "warm"):
            tm = tie_counts(shape, mode)
            lines.append(f"            {mode}: status 0 {statuses('twins', shape, mode).count(0)} / 8, virgin ties " + "  ".join(f"{k} {c['instances']}" for k, c in tm.items()))
    for family in [*TOLERANCES, *DROPPED_SETS]:
        lines.append(f"    {family + (' (dropped)' if family in DROPPED_SETS else ''):<28}changed instances of 8: " + "  ".join(f"{shape} {len(changed(family, shape))}" for shape in SHAPES) +
                     "   at the limit: " + "  ".join(f"{shape} {statuses(family, shape).count(AT_THE_LIMIT)}" for shape in SHAPES))
    for family in SCALED + ("kinds",):
        for shape in SHAPES:
            st, rs = statuses(family, shape), refs(family, shape)
            lines.append(f"    {family:<10}{shape:<8}seeds {start_of(family, shape)}+8  status 0: {st.count(0)}  at the limit: {st.count(AT_THE_LIMIT)}  other: "
                         f"{len(st) - st.count(0) - st.count(AT_THE_LIMIT)}  log entries {_span([len(o['log']) for o in rs])}")
    return "\n".join(lines)


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        print(table())
