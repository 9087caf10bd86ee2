"""lexls_lsi_batch_solve_bounds(_device) without a GPU: the symbols and their prototypes, the refusals that need no device (with the outputs left
alone), the Python entries, and the placement rule of lsi_bounds_check_kernel on both sides of its switch (tests/lsi_bounds_fit_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT

INVALID = 1
SENTINEL, FLAG_SENTINEL = 7.25, 9
DP, BP = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
NAMES = ("lexls_lsi_batch_solve_bounds", "lexls_lsi_batch_solve_bounds_device", "lexls_lsi_batch_last_consumer_kernel")


def test_symbols_and_prototypes():
    from lexls_amd import capi
    from test_capi_symbols import header_functions
    lib = capi.lib()
    declared = header_functions()
    for name in NAMES:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    host, dev, last = (getattr(lib, name) for name in NAMES)
    assert host.restype is C.c_int and dev.restype is C.c_int and last.restype is C.c_char_p
    assert host.argtypes == [C.c_void_p, DP, DP, C.c_uint32, DP, DP, BP]
    assert dev.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert last.argtypes == [C.c_void_p]
    header = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    text = header[header.index("NEW BOUNDS on the final working set"):header.index("int lexls_lsi_batch_solve_bounds(")]
    assert "NECESSARY" in text and "NOT\n * SUFFICIENT" in text and "signs of the multipliers under the new bounds are not re-examined" in text


def test_refusals_without_a_device_leave_the_outputs_alone():
    """a null handle is refused before anything else is looked at, in both forms; the variant getter answers "" for it"""
    from lexls_amd import capi
    lib = capi.lib()
    K, batch, total, n = 2, 3, 5, 4
    lb, ub = np.zeros((K, batch, total)), np.ones((K, batch, total))
    x, viol, valid = np.full((K, batch, n), SENTINEL), np.full((K, batch), SENTINEL), np.full(batch, FLAG_SENTINEL, np.uint8)
    args = (lb.ctypes.data_as(DP), ub.ctypes.data_as(DP), K, x.ctypes.data_as(DP), viol.ctypes.data_as(DP), valid.ctypes.data_as(BP))
    assert lib.lexls_lsi_batch_solve_bounds(None, *args) == INVALID
    assert b"lexls_lsi_batch_solve_bounds: null handle" in lib.lexls_last_error()
    void = tuple(a if isinstance(a, int) else C.cast(a, C.c_void_p) for a in args)
    assert lib.lexls_lsi_batch_solve_bounds_device(None, *void) == INVALID
    assert b"lexls_lsi_batch_solve_bounds_device: null handle" in lib.lexls_last_error()
    for k in (0, 65536):
        assert lib.lexls_lsi_batch_solve_bounds(None, args[0], args[1], k, *args[3:]) == INVALID
    assert (x == SENTINEL).all() and (viol == SENTINEL).all() and (valid == FLAG_SENTINEL).all()
    assert lib.lexls_lsi_batch_last_consumer_kernel(None) == b""


def test_python_entries_exist():
    from lexls_amd import lexlsi, torch_adjoint
    for name in ("solve_bounds", "solve_bounds_device", "last_consumer_kernel"):
        assert callable(getattr(lexlsi.LsiBatch, name)), name
    assert callable(torch_adjoint.solve_new_bounds)
    assert torch_adjoint.SolveNewBounds.__name__ == "SolveNewBounds"


def fit_check(tmp_path, nvars):
    """tests/lsi_bounds_fit_check.cpp on a list of nVar -> [(variant, bytes lds, bytes hbm, budget)]"""
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed for the stand-alone placement check (tests/lsi_bounds_fit_check.cpp)"
    exe = str(tmp_path / "lsi_bounds_fit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc"),
                            os.path.join(ROOT, "tests", "lsi_bounds_fit_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], input="".join(f"{n}\n" for n in nvars), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(nvars)
    return [(f[0], *(int(v) for v in f[1:])) for f in (ln.split("|") for ln in lines)]


def test_the_placement_rule_on_both_sides_of_its_switch(tmp_path):
    """restated here: two tiles of 16 rows x 65 doubles for lb / ub under either placement, nVar x 65 doubles more for the x tile; lds while the sum
    stays within the budget.  The switch the GPU cases are named for (lds46 / hbm47) is the rule's"""
    nvars = [1, 4, 7, 40, 46, 47, 64, 300]
    got = fit_check(tmp_path, nvars)
    switch = None
    for n, (variant, lds, hbm, budget) in zip(nvars, got):
        assert hbm == 8 * 65 * 2 * 16 and lds == hbm + 8 * 65 * n, n
        assert budget == 40 * 1024 and hbm <= budget
        assert variant == ("lsi_bounds_check<lds>" if lds <= budget else "lsi_bounds_check<hbm>"), n
        if variant.endswith("<hbm>") and switch is None:
            switch = n
    assert switch == 47 and got[nvars.index(46)][0] == "lsi_bounds_check<lds>"
    import lsi_bounds_cases as BC
    assert BC.OWN["lds46"]["n"] == 46 and BC.OWN["hbm47"]["n"] == 47
