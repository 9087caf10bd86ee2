"""What the cases of tests/large_cases.py claim, from the CPU oracle, the host planner and the constants alone: the GPU tests of
tests/test_gpu_large_cases.py compare the large path's kernels with these cases, so a case that sat on the tested side of a switch after
all — or whose ranks a kernel's rounding may legitimately move — would let them pass on anything.

The constants below are READ from lexls_amd/csrc/lqr_large_plan.h (tests/large_plan.py runs tests/large_plan_check.cpp, which prints them: the
header the kernels and launchers take them from is the only place that states a value); side() computes from them, per case, which side of each switch of
the kernels and launchers the case is on, and the union of the cases must hold both sides of every row:
    step R>256     fast_step: rows left in the level beyond the 64 x FRC a lane keeps in registers (the tail loops of the dot product and of
                   the update) — every problem of a batch, and problem 0 alone under LEXLS_LARGE_PERSIST = 0 / 2
    persist R>256  fast_level_persist: beyond the one granule per thread of the batch (64 x NW), fetched one by one — problem 0 alone, default
    n>1024         fast_step's second search loop (candidates beyond NCAND per thread), large_pivot's second trip over the columns
    G>256          persist_within_limits (kPersistMaxG): no one-launch form, a single problem takes a launch per pivot
    level>1024     launchers: large_trsm (a row per lane, multipliers in LDS) instead of large_trsm_cols behind a level
    pivot R>1024   large_pivot's second trip over the rows of a level
    rows>1024      fast_level_end's second block of rows
    tiles          n + 1 = 0 and 1 (mod GBN = 64); rows below level 0 = 1 (mod GBM = 64, and mod TRB = 8); a level rank = 1 (mod TCH = 16) and
                   a rank below TCH; a 1-row level; an empty level in the middle
    states         a level on which one problem of the batch is exhausted and another is not; a level the launchers take the > 1024 branch
                   for while a problem's own level is at most 1024 rows

MEASURED (`python tests/large_cases.py` and side(); Y = the case is on the far side of the switch for some pivot / level, - = on the near side only, both = both;
ranks per problem; sens = largest one-ulp sensitivity of x over the case's problems — every one far below 1e-12, so contract (T)'s plain
1e-10 is the bound of every case):
    case       shape                   step R>256  persist R>256  n>1024  G>256  level>1024  pivot R>1024  rows>1024  ranks                          sens
    rows1030   n=60   [1030,70]  x3    both        both           -       -      Y           both          Y          [25,20] [30,15] [60,0]         7.3e-16
    rows1024   n=60   [1024,70]  x2    both        both           -       -      -           -             Y          [25,20] [30,15]                7.9e-16
    n1030      n=1030 [40,40]    x2    -           (no form)      Y       Y      -           -             -          [40,40] [40,40]                1.2e-15
    rows257    n=150  [257,256,60] x2  both        both           -       -      -           -             -          [50,60,20] [40,30,60]          1.5e-13
    rows330    n=150  [330,120]  x2    both        both           -       -      -           -             -          [150,0] [100,30]               7.9e-16
    edges127   n=127  [100,1,0,40,24] x2  -        -              -       -      -           -             -          [17,1,0,5,10] [9,0,0,16,8]     5.0e-16
    edges128   n=128  [100,1,0,40,24] x2  -        -              -       -      -           -             -          [17,1,0,5,10] [9,0,0,16,8]     4.2e-16
tiles: n + 1 = 128 (edges127), 129 (edges128), neither (the others); 65 rows below level 0, ranks 17 and 5, a 1-row and an empty level (edges*).
states: rows1030 (problem 2 exhausted after level 0; problem 1's level 0 has 300 rows under the batch's 1030), rows330 (problem 0 exhausted).
n1030 on the oracle: the first seven pivots are the six scaled columns and column 1000, the copy of 1027, which is taken while 1027 is not.
No case needed another seed or a larger shape: every one is planned lqr_large<multi-launch> / lqr_large<step-per-pivot,mfma> as drawn.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import large_cases as L
import large_plan as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the constants of lexls_amd/csrc/lqr_large_plan.h, as tests/large_plan_check.cpp prints them ----
K = LP.constants()
FRC, FNT = K["FRC"], K["FNT"]            # fast_step: rows per lane in registers, threads
NW = K["PTC_MIN"]                        # fast_level_persist<PTC_MIN,1>, the default form: wavefronts = columns per workgroup; one granule per thread in the batch
NTP = K["NTP"]                           # large_pivot's threads
ONE_TRIP = max(K["kStepCandWindow"], NTP)  # columns beyond BOTH fast_step's candidates in registers and one trip of large_pivot's search
G_MAX = K["kPersistMaxG"]                # persist_within_limits
TRSM_COLS_MAX = K["kTrsmColsMax"]        # plan_level: large_trsm_cols up to this level dimension
LEVEL_END_ROWS = K["kLevelEndRows"]      # fast_level_end: rows per block
GBM, GBN = K["GBM"], K["GBN"]            # large_gemm_mfma's tile
TRB, TCH = K["TRB"], K["TCH"]            # large_trsm_cols: rows per workgroup, multipliers per chunk


def pivots(case, b):
    """(level, rows left) of every pivot the oracle takes in problem b"""
    return [(k, int(case["dims"][b, k]) - c) for k in range(case["dims"].shape[1]) for c in range(int(case["ref"]["rank"][b, k]))]


def side(case):
    """row of the table -> set of sides (False near, True far) the case reaches"""
    n, dims, rank = case["n"], case["dims"].astype(int), case["ref"]["rank"].astype(int)
    B, nobj = dims.shape
    G = (n + NW) // NW
    s = {}
    s["step R>256"] = {R > 64 * FRC for b in range(B) for _, R in pivots(case, b)}
    s["persist R>256"] = {R > 64 * NW for _, R in pivots(case, 0)} if G <= G_MAX else set()
    s["n>1024"] = {n > ONE_TRIP and max(case["ref"]["perm"][b, :int(rank[b].sum())].max() for b in range(B)) >= ONE_TRIP}
    s["G>256"] = {G > G_MAX}
    level_max = dims.max(axis=0)
    s["level>1024"] = {int(level_max[k]) > TRSM_COLS_MAX for k in range(nobj - 1) if level_max[k] > 0}
    s["pivot R>1024"] = {R > NTP for b in range(B) for _, R in pivots(case, b)}
    s["rows>1024"] = {int(dims.sum(axis=1).max()) > LEVEL_END_ROWS}
    below0 = [int(dims[b, 1:].sum()) for b in range(B)]
    s["n+1=0 mod 64"] = {(n + 1) % GBN == 0}
    s["n+1=1 mod 64"] = {(n + 1) % GBN == 1}
    s["below=1 mod 64"] = {r % GBM == 1 and r % TRB == 1 for r in below0}
    s["rank=1 mod 16"] = {r > TCH and r % TCH == 1 for r in rank.ravel()}
    s["rank<16"] = {0 < r < TCH for r in rank.ravel()}
    s["1-row level"] = {bool((dims == 1).any())}
    s["empty level inside"] = {bool((dims[:, 1:-1] == 0).any())}
    start_exhausted = np.array([[int(rank[b, :k].sum()) >= n for k in range(nobj)] for b in range(B)])
    s["exhausted beside live"] = {bool(start_exhausted[:, k].any() and not start_exhausted[:, k].all()) for k in range(nobj) if level_max[k] > 0}
    s["short under >1024"] = {bool(level_max[k] > TRSM_COLS_MAX and (dims[:, k] <= TRSM_COLS_MAX).any()) for k in range(nobj - 1) if level_max[k] > 0}
    return s


@pytest.fixture(scope="module", params=list(L.CASES))
def case(request):
    return L.build(request.param)


def test_union_of_the_cases_holds_both_sides_of_every_switch():
    union = {}
    for name in L.CASES:
        for row, sides in side(L.build(name)).items():
            union.setdefault(row, set()).update(sides)
    assert all(v == {False, True} for v in union.values()), {k: v for k, v in union.items() if v != {False, True}}


def test_each_case_is_where_it_was_built_to_be():
    s = {name: side(L.build(name)) for name in L.CASES}
    for name in ("rows1030", "rows1024", "rows257", "rows330"):
        assert s[name]["step R>256"] == {False, True} and s[name]["persist R>256"] == {False, True}, name
    assert s["rows1030"]["level>1024"] == {True} and s["rows1030"]["pivot R>1024"] == {False, True} and s["rows1030"]["rows>1024"] == {True}
    assert s["rows1030"]["exhausted beside live"] == {False, True} and s["rows1030"]["short under >1024"] == {True}
    assert s["rows1024"]["level>1024"] == {False} and s["rows1024"]["pivot R>1024"] == {False} and s["rows1024"]["rows>1024"] == {True}
    assert int(L.build("rows1024")["dims"].max()) == TRSM_COLS_MAX  # the boundary itself
    assert s["n1030"]["n>1024"] == {True} and s["n1030"]["G>256"] == {True} and s["n1030"]["persist R>256"] == set()
    assert max(R for _, R in pivots(L.build("rows257"), 0)) == 64 * FRC + 1  # just above the window ...
    assert 64 * FRC in [R for k, R in pivots(L.build("rows257"), 0) if k == 1]  # ... next to an exact 256
    assert s["rows330"]["exhausted beside live"] == {False, True}
    assert s["edges127"]["n+1=0 mod 64"] == {True} and s["edges128"]["n+1=1 mod 64"] == {True}
    for name in ("edges127", "edges128"):
        for row in ("below=1 mod 64", "rank=1 mod 16", "rank<16"):
            assert True in s[name][row], (name, row)
        assert s[name]["1-row level"] == {True} and s[name]["empty level inside"] == {True}


def test_ranks_are_the_ones_the_data_were_built_for(case):
    print(L.summary(case))
    n, rank = case["n"], case["ref"]["rank"]
    for b, forced in enumerate(case["forced"]):
        if forced is not None:
            assert rank[b].tolist() == forced, (case["name"], b)
        else:  # iid: every level takes what it can
            left = n
            for k, d in enumerate(case["dims"][b]):
                assert rank[b, k] == min(int(d), left)
                left -= int(rank[b, k])
    if case["name"] == "rows330":
        assert rank[0].tolist() == [150, 0]  # the columns run out inside a level of more than 256 rows
    assert np.isfinite(case["ref"]["x"]).all()


def test_ranks_and_pivots_are_stable_a_decade_either_side_of_the_tolerance(case):
    """ranks, first columns and permutation the same at 10 x and 1 / 10 of the default tolerance: 'pivots and ranks exact' is a fair demand of
    the tolerance-contract path — and rows1030's level-0 rank deficiency, which sits on 1030-row sums, is settled here, not on the GPU"""
    assert case["stable"].all(), case["name"]
    for f in (1.0 / L.FACTOR, L.FACTOR):
        o = L._run(case["name"], case["lod"], case["dims"], L.TOL * f)
        for k in ("rank", "fcol", "perm"):
            np.testing.assert_array_equal(o[k], case["ref"][k], err_msg=f"{case['name']} x {f}: {k}")


def test_one_ulp_sensitivity(case):
    """every case is well conditioned: the plain 1e-10 of contract (T) is its bound (max(1e-10, 100 x sensitivity))"""
    assert (case["sens"] > 0).all() and (100.0 * case["sens"] < 1e-10).all(), case["sens"]


def test_n1030_first_pivots_lie_beyond_1024_and_the_tie_goes_to_the_first_position():
    case = L.build("n1030")
    n, perm, lod = case["n"], case["ref"]["perm"], case["lod"]
    for b in range(lod.shape[0]):
        assert (perm[b, :6] >= ONE_TRIP).sum() >= 4, perm[b, :8]
    first, second = case["tie"]
    assert first < ONE_TRIP <= second and np.array_equal(lod[0, first], lod[0, second])
    at = list(range(n))  # physical column at every position, through the swaps of lexlse.h:222-232
    taken = []
    for c in range(int(case["ref"]["totalrank"][0])):
        p = int(perm[0, c])
        if at[p] == first:  # the copy is taken: the original is still where it was, behind it, with the same norm
            assert at.index(second) == second > p == first
        at[c], at[p] = at[p], at[c]
        taken.append(at[c])
    assert first in taken[:7] and second not in taken, taken[:8]


# ---- the planner (lexls_amd/csrc/lexls_dispatch.h) on the host, as tests/test_dispatch_plan.py runs it ----
def query(i, n, caps, dims, policy):
    d = np.asarray(dims)
    uniform = int(d.max()) if d.min() == d.max() else 0
    vals = ["lse", i, d.shape[0], n, len(caps), sum(caps), uniform, max(int(d.sum(axis=1).max()), 1), int(d.max()), 0, 0, 16, 1, 1, policy, 0, 0, 2048, 0]
    return " ".join(str(v) for v in vals)


def test_the_reuse_cases_are_planned_on_the_step_per_pivot_path_and_well_conditioned(tmp_path):
    """what test_workspace_reuse of tests/test_gpu_large_cases.py relies on: reuse300 / reuse330, as a batch of two and problem 0 alone, are planned
    lqr_large<step-per-pivot,mfma> under policy 0, and the plain 1e-10 of contract (T) is their bound; pivots stable around the tolerance"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "plan")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "lexls_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    lines = []
    for name in L.REUSE:
        c = L.build(name)
        print(L.summary(c))
        assert (c["sens"] > 0).all() and (100.0 * c["sens"] < 1e-10).all(), (name, c["sens"])
        assert c["stable"].all(), name
        assert [r.tolist() for r in c["ref"]["rank"]] == c["forced"], name
        assert L.levels_reached(c) == 2  # both levels look for pivots: the Gauss step below level 0 runs
        for dims in (c["dims"], c["dims"][:1]):
            lines.append(query(len(lines), c["n"], c["caps"], dims, 0))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    assert [ln.split("|")[1] for ln in run.stdout.splitlines()] == ["lqr_large<step-per-pivot,mfma>"] * len(lines), run.stdout


def test_planned_on_the_large_path(tmp_path):
    """policy 5: lqr_large<multi-launch>; policy 0: lqr_large<step-per-pivot,mfma> — the batch, and every problem of it alone"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "plan")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "lexls_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    lines, want = [], []
    for name in L.CASES:
        c = L.build(name)
        for dims in [c["dims"]] + [c["dims"][b:b + 1] for b in range(c["dims"].shape[0])]:
            for policy, kernel in ((5, "lqr_large<multi-launch>"), (0, "lqr_large<step-per-pivot,mfma>")):
                lines.append(query(len(lines), c["n"], c["caps"], dims, policy))
                want.append((name, dims.shape[0], policy, kernel))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    got = [ln.split("|")[1] for ln in run.stdout.splitlines()]
    assert got == [w[3] for w in want], [(w, g) for w, g in zip(want, got) if w[3] != g]
