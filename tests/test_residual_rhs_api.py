"""Residuals of new right-hand sides on a kept LexLSE factor and per-objective costs of new LexLSI bounds in the C ABI: declared in
include/lexls_hip.h, exported by the library, listed in capi.SYMBOLS and bound with the documented argument types, documented where callers read,
refusing null arguments before anything else; the Python surface; lex_argmin on literal arrays.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

LEXLS_ERR_INVALID = 1
_dp, _u8p, _vp = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_void_p
ARGTYPES = {
    "lexls_lse_residual_rhs": [_vp, _dp, _dp, C.c_uint32],
    "lexls_lse_get_residual_rhs": [_vp, _dp, _dp],
    "lexls_lse_residual_rhs_device": [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp],
    "lexls_lsi_batch_solve_bounds_cost": [_vp, _dp, _dp, C.c_uint32, _dp, _dp, _dp, _u8p],
    "lexls_lsi_batch_solve_bounds_cost_device": [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp],
}
DECLARATIONS = (
    r"int\s+lexls_lse_residual_rhs\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*h_rhs\s*,\s*const\s+double\s*\*\s*h_fixed\s*,\s*uint32_t\s+nrhs\s*\)",
    r"int\s+lexls_lse_get_residual_rhs\s*\(\s*lexls_lse_t\s+h\s*,\s*double\s*\*\s*h_v\s*,\s*double\s*\*\s*h_cost\s*\)",
    r"int\s+lexls_lse_residual_rhs_device\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*d_rhs\s*,\s*const\s+double\s*\*\s*d_fixed\s*,\s*uint32_t\s+nrhs\s*,"
    r"\s*double\s*\*\s*d_x\s*,\s*double\s*\*\s*d_v\s*,\s*double\s*\*\s*d_cost\s*\)",
    r"int\s+lexls_lsi_batch_solve_bounds_cost\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*h_lb\s*,\s*const\s+double\s*\*\s*h_ub\s*,\s*uint32_t\s+nrhs\s*,"
    r"\s*double\s*\*\s*h_x\s*,\s*double\s*\*\s*h_violation\s*,\s*double\s*\*\s*h_cost\s*,\s*uint8_t\s*\*\s*h_valid\s*\)",
    r"int\s+lexls_lsi_batch_solve_bounds_cost_device\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*d_lb\s*,\s*const\s+double\s*\*\s*d_ub\s*,\s*uint32_t\s+nrhs\s*,"
    r"\s*double\s*\*\s*d_x\s*,\s*double\s*\*\s*d_violation\s*,\s*double\s*\*\s*d_cost\s*,\s*uint8_t\s*\*\s*d_valid\s*\)",
)


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_symbols_are_declared_exported_listed_and_bound():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name, argtypes in ARGTYPES.items():
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
        assert getattr(lib, name).restype is C.c_int and list(getattr(lib, name).argtypes) == argtypes, f"{name} is not bound with the documented types"
    for pattern in DECLARATIONS:
        assert re.search(r"\b" + pattern, code), pattern


def test_null_arguments_are_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    a = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out, out2, flag = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_uint8 * 2)(9, 9)
    void = lambda p: C.cast(p, C.c_void_p)  # noqa: E731
    assert lib.lexls_lse_residual_rhs(None, a, None, 1) == LEXLS_ERR_INVALID and b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lse_get_residual_rhs(None, out, out2) == LEXLS_ERR_INVALID
    assert lib.lexls_lse_residual_rhs_device(None, void(a), None, 1, void(out), void(out2), None) == LEXLS_ERR_INVALID and b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_bounds_cost(None, a, a, 1, out, None, out2, flag) == LEXLS_ERR_INVALID and b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_bounds_cost_device(None, void(a), void(a), 1, void(out), None, void(out2), void(flag)) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert list(out) == [7.0] * 4 and list(out2) == [7.0] * 4 and list(flag) == [9, 9]


def test_the_header_states_the_layouts_and_the_rules():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lse_residual_rhs\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lse_residual_rhs"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("nrhs x batch x cap", "nrhs x batch x nObj", "LOD row order", "lexls_lse_get_v", "written as 0", "one ordered fma chain", "rank == dim",
                   "0.0 exactly", "bit for bit", "LEXLS_ERR_UNSUPPORTED", "regularization_type != 0", "every output null", "nrhs > 65535", "no kept factor",
                   "before any device work and with every output left alone", "lexls_lse_set_deferred_sync", "no atomics", "residual_rhs<64,staged>",
                   "not changed by these calls", "only while they belong to the current factor"):
        assert phrase in doc, f"the header comment does not state: {phrase}"
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lsi_batch_solve_bounds_cost\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lsi_batch_solve_bounds_cost"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("cost must be non-NULL", "x may be NULL", "nrhs x batch x nObj", "max(lb - a.x, a.x - ub, 0)", "user's row order", "the very fma chain violation uses",
                   "in or out of the working set", "lexls_lsi_batch_set_instance_obj_dims", "exact zeros", "keeps its bits", "lsi_bounds_cost<lds>",
                   "launches exactly what it launched before"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    code = ("import sys, inspect; import lexls_amd.lexlse as e, lexls_amd.lexlsi as l; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert callable(e.BatchedLexLSE.residual_rhs) and callable(e.BatchedLexLSE.residual_rhs_device) and callable(l.lex_argmin); "
            "assert inspect.signature(l.LsiBatch.solve_bounds).parameters['with_cost'].default is False; "
            "assert inspect.signature(l.LsiBatch.solve_bounds_device).parameters['cost'].default is None; "
            "assert l.lex_argmin([[[0.0]]]).tolist() == [0]; assert 'torch' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_lex_argmin_on_literal_arrays():
    from lexls_amd.lexlsi import lex_argmin
    # (K = 3, batch = 2, nObj = 2): level order comes before magnitude — candidate 1 is worse at level 0 by little and better at level 1 by much
    cost = np.array([[[1.0, 9.0], [0.0, 5.0]],
                     [[1.1, 0.0], [0.0, 4.0]],
                     [[1.0, 9.5], [2.0, 0.0]]])
    assert lex_argmin(cost).tolist() == [0, 1]
    assert lex_argmin(cost, 0.0).dtype == np.int64
    # the tie window is absolute and per level: with 0.2 candidate 1 stays in the running at level 0 of instance 0 and wins level 1
    assert lex_argmin(cost, 0.2).tolist() == [1, 1]
    # ties through every level: the first candidate; a window does not chain (1.0, 1.15, 1.3 with 0.2: 1.3 is out)
    assert lex_argmin(np.array([[[1.0, 2.0]], [[1.0, 2.0]]])).tolist() == [0]
    assert lex_argmin(np.array([[[1.3, 0.0]], [[1.15, 5.0]], [[1.0, 5.0]]]), 0.2).tolist() == [1]
    # a single candidate, a single level, and a refusal of other shapes
    assert lex_argmin(np.zeros((1, 4, 3))).tolist() == [0, 0, 0, 0]
    assert lex_argmin(np.array([[[3.0]], [[2.0]]])).tolist() == [1]
    for bad in (np.zeros((2, 3)), np.zeros((0, 2, 3))):
        try:
            lex_argmin(bad)
        except ValueError:
            continue
        raise AssertionError(f"lex_argmin accepted shape {bad.shape}")
