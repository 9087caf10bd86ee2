"""The conditions on the cases of tests/reg_cases.py, from the CPU oracle and the planner alone: tests/test_gpu_regularization.py compares the
regularization family with what these cases carry, so a case that stands on the same side of a switch as its neighbour, whose Cholesky orders
miss the panel edges, whose CG always leaves by the same exit or whose damping moves nothing would let the kernels pass on anything.
Conditions (a) - (e) of the docstring of tests/reg_cases.py; the measured figures are in that docstring.  No GPU needed."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import reg_cases as C

ROOT = C.ROOT
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "reg_plan_check.cpp")


@functools.lru_cache(maxsize=None)
def program(sanitized=False):
    cxx = shutil.which("g++")
    assert cxx is not None, "tests of the regularization cases' plan need g++"
    d = tempfile.mkdtemp(prefix="reg_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "reg_plan_check")
    build = subprocess.run([cxx, *FLAGS, *(["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []), SOURCE, "-o", exe],
                           capture_output=True, text=True)
    if sanitized and build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        return None  # the toolchain has no sanitizer runtime
    assert build.returncode == 0, build.stderr
    return exe


def run_plan(lines, sanitized=False):
    """id -> (kernel, window order, basis in LDS, dynamic LDS of the launch)"""
    exe = program(sanitized)
    if exe is None:
        return None
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        ident, kernel, window, basis, lds = ln.split("|")
        out[ident] = (kernel, int(window), int(basis), int(lds))
    assert len(out) == len(lines)
    return out


def all_lines():
    return [C.plan_line(nm, t, p) for nm, c in C.CASES.items() for t in c["types"] for p in (0, 1)]


@pytest.fixture(scope="module")
def plans():
    return run_plan(all_lines())


@pytest.fixture(scope="module", params=list(C.CASES))
def case(request):
    return C.build(request.param)


def test_docstring_table_is_what_the_module_measures(case):
    print(C.summary(case))
    assert C.summary(case) in C.__doc__


def test_a_committed_plan_is_the_planner_s(plans):
    """(a) PLAN, the table the GPU test asserts last_kernel() and last_reg_placement() against, is what reg_plan_check prints"""
    assert set(C.PLAN) == set(C.CASES)
    for nm, c in C.CASES.items():
        assert set(C.PLAN[nm]) == set(c["types"]), nm
        for t in c["types"]:
            assert plans[f"{nm}:{t}:0"][:3] == C.PLAN[nm][t], (nm, t)
            want = C.POLICY_1 if nm in C.WAVE_CASES else C.PLAN[nm][t][0]
            assert plans[f"{nm}:{t}:1"][:3] == (want, 0, 0), (nm, t)
            if nm in C.WAVE_CASES:
                assert plans[f"{nm}:{t}:0"][3] <= 160 * 1024


def test_a_plan_check_is_clean_under_the_sanitizers(plans):
    got = run_plan(all_lines(), sanitized=True)
    if got is None:
        pytest.skip("g++ has no sanitizer runtime here")
    assert got == plans


def test_a_cases_stand_on_opposite_sides_of_every_flip():
    """(a) switch 1: for each kernel shape and type, the largest n on one side and the smallest on the other of every flip of the placement"""
    seen = set()
    for t, what, lds_side, other in C.FLIPS:
        a, b = C.PLAN[lds_side][t], C.PLAN[other][t]
        assert a[0] == b[0] and a[0] in (C.W41, C.W64), (t, what)
        assert C.CASES[other]["n"] == C.CASES[lds_side]["n"] + 1 and len(C.CASES[other]["dims"]) == len(C.CASES[lds_side]["dims"])  # neighbours: THE flip
        col = 2 if what == "basis" else 1
        assert a[col] > 0 and b[col] == 0, (t, what, a, b)
        seen.add((a[0], t, what))
    types_with = {"basis": (1, 8, 3, 2), "window": (1, 8, 3)}  # (type 2 has no work matrix; the windows of 4 and 5 are type 3's)
    for kernel in (C.W41, C.W64):
        for what, types in types_with.items():
            for t in types:
                if (kernel, t, what) == (C.W41, 3, "window"):  # 8 x 12 x 12 B behind the vectors fits for every n + 1 <= 41 of four levels: no flip
                    assert all(C.PLAN[nm][3][1] == 12 for nm in C.PLAN if nm.startswith("p41_"))
                    continue
                assert (kernel, t, what) in seen, (kernel, t, what)
    # every placement the body can be given occurs: window + basis, window only, basis only, nothing
    combos = {(k, w > 0, b > 0) for p in C.PLAN.values() for k, w, b in p.values() if k in (C.W41, C.W64)}
    assert combos == {(k, w, b) for k in (C.W41, C.W64) for w in (True, False) for b in (True, False)}


def test_a_every_type_on_every_kernel():
    for t in C.ALL:
        kernels = {p[t][0] for p in C.PLAN.values() if t in p}
        assert {C.W41, C.W64, C.G256, C.G1024H} <= kernels, (t, kernels)
    assert C.PLAN["tall"][8][0] == C.G1024L  # a regularized shape does reach lqr_generic<1024,lds>: more than 512 rows
    assert C.PLAN["t7"][7][0] == C.G256 and C.CASES["t7"]["n"] == 70


def test_b_the_window_holds_every_order_when_there_is_one():
    """(b) switch 1, RegView::with_order: whenever the launcher places a window, every order the type can ask for fits it — for TIKHONOV
    tikhonov_2 runs while Fc + rank <= n - Fc - rank (order Fc - nf + rank <= n / 2) and tikhonov_1 otherwise (order n - Fc < n / 2 + rank):
    exhaustively over every shape of the wave family.  The HBM side of with_order is reached only without a window (the placement cases)"""
    for md in (12, 16):
        for n in range(1, 64):
            window = min(n // 2 + md + 1, n)
            for Fc in range(n):
                for rank in range(1, min(md, n - Fc) + 1):
                    RC = n - Fc - rank
                    for nf in range(Fc + 1):
                        order = Fc - nf + rank if Fc + rank <= RC else RC + rank
                        assert order <= window, (md, n, Fc, rank, nf)
    case = C.build("window")
    window = C.PLAN["window"][1][1]
    orders = case["orders"][1]
    assert window == 29 // 2 + 12 + 1 < 29
    assert max(N for _, _, N, _ in orders) == window - 1  # the largest order the shape can produce: 14 + 12
    for b in range(len(case["lod"])):  # both Tikhonov branches in the same problem (1: level 0 has the factor 0.0; 4: three fixed variables, tikhonov_1 at once)
        assert {br for pb, _, _, br in orders if pb == b} == ({1} if b in (1, 4) else {1, 2}), b
    assert case["fixed"]["nfixed"].any()


def test_b_orders_meet_the_panel_edges_and_pass_64():
    case = C.build("panel")
    assert case["plain"]["rank"][0].tolist() == case["caps"] and not case["fixed"] and (case["fac"][0] != 0.0).all()
    in_problem_0 = sorted(N for b, _, N, _ in case["orders"][8] if b == 0)
    assert in_problem_0 == list(C.PANEL_ORDERS)  # spd_solve_wave (lse_spd_solve.h): 16 | 17, 32 | 33, 48 | 49 and 63
    assert set(C.CASES["panel"]["types"]) == {8, 1, 5}
    assert {N for _, _, N, _ in case["orders"][1]} & {16, 17, 32}  # ... and under type 1
    big = {(nm, t): max([N for _, _, N, _ in C.build(nm)["orders"][t]] or [0]) for nm in ("g100", "g130", "g150", "g70r") for t in C.CASES[nm]["types"]}
    assert big[("g130", 1)] == 130 and big[("g130", 3)] == 70 and big[("g150", 8)] == 150 and big[("g100", 8)] > 64  # the workgroup Cholesky beyond 64
    assert any(0 < v <= 64 for v in big.values())  # ... and within 64 on NT = 256 / 1024
    assert C.build("g130")["plain"]["rank"][0].tolist() == [70, 40, 20]
    g = C.build("g70r")
    assert (g["dims"] == 0).any() and g["fixed"]["nfixed"].any() and (g["dims"] != g["dims"][0]).any()


def test_c_both_exits_of_the_cg_loop():
    for nm in ("cg_w", "cg_g"):
        case = C.build(nm)
        assert set(case["cg_caps"]) == {1, 10, C.LONG_CAP} and case["types"] == (2, 6)
        for t in case["types"]:
            x = case["cg_x"]
            for b in range(len(case["lod"])):
                assert (x[(t, 9)][b] != x[(t, 10)][b]).any(), (nm, t, b)  # cap 10 ends the loop by the cap
                np.testing.assert_array_equal(x[(t, C.LONG_CAP)][b], x[(t, C.LONG_CAP + 1)][b])  # ... the long cap by convergence
            assert (x[(t, 10)] != x[(t, C.LONG_CAP)]).any() and (case["ref"][(t, 1)]["x"] != x[(t, 10)]).any()
            np.testing.assert_array_equal(case["ref"][(t, 10)]["x"], x[(t, 10)])


def test_d_the_regularization_moves_x_and_zero_factors_do_not(case):
    zero_at_0 = 0
    for t in case["types"]:
        ref = case["ref"][(t, 10)]
        for k in ("perm", "rank", "fcol", "totalrank"):  # the damping touches right-hand sides only
            np.testing.assert_array_equal(ref[k], case["plain"][k])
        assert (np.abs(ref["x"] - case["plain"]["x"]).max(axis=1) > 1e-6).all(), t
        assert np.isfinite(ref["x"]).all()
        for b in np.flatnonzero(case["fac"][:, 0] == 0.0):  # level 0 with the factor 0.0: its transformed right-hand side is the unregularized one
            r = int(ref["rank"][b, 0])
            np.testing.assert_array_equal(ref["factor"][b, case["n"], :r], case["plain"]["factor"][b, case["n"], :r])
            zero_at_0 += 1
    assert zero_at_0 > 0 and (case["fac"][0] != 0.0).all() and (case["fac"] == 0.0).any()
    if case["fixed"]:
        np.testing.assert_array_equal(case["plain"]["fcol"][:, 0], case["fixed"]["nfixed"])  # m0 = Fc - nf starts at 0


def test_d_rank_deficient_levels_and_fixed_variables():
    short = {nm: C.build(nm)["short"] for nm in C.CASES}
    assert sum(1 for v in short.values() if v) >= len(C.CASES) - 1, short  # (tall: 300 rows on 12 columns keep their rank)
    fixed = {nm for nm, c in C.CASES.items() if c.get("nfixed")}
    assert fixed & set(C.WAVE_CASES) and fixed - set(C.WAVE_CASES)


def test_e_variable_factor_takes_both_sides():
    for nm in ("vf_w", "vf_g"):
        case = C.build(nm)
        eps = case["var_reg"]
        assert eps > 0 and case["types"] == (1, 3)
        for t in case["types"]:
            ce = np.array([v for _, _, v in case["ce"][t]])
            assert (ce < eps).any() and (ce >= eps).any()
            assert (np.abs(ce - eps) > 1e-6 * eps).all()  # rounding cannot move a level across
            ranked = int((case["plain"]["rank"] > 0).sum())
            assert len(ce) == ranked
    assert C.PLAN["vf_w"][1][0] == C.W41 and C.PLAN["vf_g"][1][0] == C.G256
