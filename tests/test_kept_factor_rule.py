"""The rule by which the kernels that walk a kept factor trust a level's stored rank (lexls_amd/csrc/lse_kept_factor.h: trusted_rank, its only
statement) against the rule restated here, on a table that meets every clamp and each boundary one step to either side.  The C++ rule runs
on the host through tests/kept_factor_check.cpp.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule(n, nf, T, dim, rk, Fc):
    """the `level` rule as the adjoint kernels spelled it out before it had one home: rank 0 when every variable is fixed or the level starts
    behind the pivot columns [nf, T), else the stored rank held inside the level's rows and inside the pivot columns"""
    rank = rk if (nf < n and Fc < T) else 0
    if rank > dim:
        rank = dim
    room = T - (Fc if Fc < T else T)
    if rank > room:
        rank = room
    return rank


# (n, nf, T, dim, rk, Fc) -> what the rule must answer, and why the row is here
TABLE = [
    ((7, 0, 7, 3, 2, 2), 2, "no clamp bites"),
    ((7, 6, 7, 3, 1, 6), 1, "one variable left free: the ranks count"),
    ((7, 7, 7, 3, 2, 0), 0, "every variable fixed (nf == n)"),
    ((7, 8, 7, 3, 2, 0), 0, "nf beyond n (the view holds it to n; the rule answers the same)"),
    ((7, 0, 5, 3, 1, 4), 1, "Fc == T - 1: the last pivot column"),
    ((7, 0, 5, 3, 2, 5), 0, "Fc == T: the level starts behind the pivot columns"),
    ((7, 0, 5, 3, 2, 6), 0, "Fc > T"),
    ((9, 0, 9, 3, 2, 1), 2, "rk == dim - 1"),
    ((9, 0, 9, 3, 3, 1), 3, "rk == dim"),
    ((9, 0, 9, 3, 4, 1), 3, "rk > dim: held to the level's rows"),
    ((9, 0, 6, 8, 2, 3), 2, "rk == T - Fc - 1"),
    ((9, 0, 6, 8, 3, 3), 3, "rk == T - Fc"),
    ((9, 0, 6, 8, 4, 3), 3, "rk > T - Fc: held to the pivot columns"),
    ((9, 0, 6, 2, 7, 3), 2, "both clamps bite, the rows first"),
    ((7, 0, 0, 3, 2, 0), 0, "T == 0: no pivot at all"),
    ((7, 0, 1, 3, 2, 0), 1, "T == 1: one pivot column"),
    ((7, 0, 7, 0, 2, 0), 0, "a level without rows"),
    ((7, 0, 7, 3, 0, 2), 0, "stored rank 0"),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path_factory.mktemp("kept_factor") / "kept_factor_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "kept_factor_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe] + [str(v) for row, _, _ in TABLE for v in row], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = [int(line) for line in run.stdout.split()]
    assert len(out) == len(TABLE)
    return out


def test_the_rule_answers_what_the_restatement_answers(answers):
    for (row, expected, why), got in zip(TABLE, answers):
        print(f"{row} -> {got}  ({why})")
        assert rule(*row) == expected, (row, why)  # the table's own column against the restatement
        assert got == expected, (row, why)


def test_the_table_meets_every_clamp_and_both_sides_of_each_boundary():
    rows = [r for r, _, _ in TABLE]
    assert {nf - n for n, nf, T, dim, rk, Fc in rows} >= {-1, 0, 1}                            # nf against n
    assert {Fc - T for n, nf, T, dim, rk, Fc in rows if nf < n and T > 1} >= {-1, 0, 1}        # Fc against T
    live = [(n, nf, T, dim, rk, Fc) for n, nf, T, dim, rk, Fc in rows if nf < n and Fc < T]
    assert {rk - dim for n, nf, T, dim, rk, Fc in live if dim <= T - Fc} >= {-1, 0, 1}         # rk against dim where the rows bind
    assert {rk - (T - Fc) for n, nf, T, dim, rk, Fc in live if T - Fc < dim} >= {-1, 0, 1}     # rk against T - Fc where the columns bind
    assert any(rule(*r) == r[4] and r[4] > 0 for r in rows) and any(r[2] == 0 for r in rows)   # no clamp bites; T == 0
