"""The gradient of the LexLSE solve with respect to the matrix in the C ABI: declared in include/lexls_hip.h, exported by the library, listed in
capi.SYMBOLS, documented where callers read, and refusing a null handle before anything else.  No GPU."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lexls_lse_solve_adjoint_matrix", "lexls_lse_get_adjoint_matrix", "lexls_lse_solve_adjoint_matrix_device")
LEXLS_ERR_INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_three_symbols_are_declared_exported_and_listed():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*lexls_lse_t\s+h\b", code), f"{name} is not declared in include/lexls_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
    assert re.search(r"lexls_lse_solve_adjoint_matrix\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*h_g\s*\)", code)
    assert re.search(r"lexls_lse_get_adjoint_matrix\s*\(\s*lexls_lse_t\s+h\s*,\s*double\s*\*\s*h_grad_lod\s*,\s*uint8_t\s*\*\s*h_differentiable\s*\)", code)
    assert re.search(r"lexls_lse_solve_adjoint_matrix_device\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*d_g\s*,\s*double\s*\*\s*d_grad_lod\s*,"
                     r"\s*uint8_t\s*\*\s*d_differentiable\s*\)", code)
    # the solve map stays internal: exported for the tests, absent from the public header
    assert hasattr(lib, "lexls_internal_apply_solve_map") and "apply_solve_map" not in header()
    internal = open(os.path.join(ROOT, "lexls_amd", "csrc", "lexls_internal.h")).read()
    assert re.search(r"int\s+lexls_internal_apply_solve_map\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*d_rhs\s*,\s*double\s*\*\s*d_out\s*\)", internal)


def test_a_null_handle_is_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out_G, out_f = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_uint8 * 4)(7, 7, 7, 7)
    assert lib.lexls_lse_solve_adjoint_matrix(None, g) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lse_get_adjoint_matrix(None, out_G, out_f) == LEXLS_ERR_INVALID
    assert lib.lexls_lse_solve_adjoint_matrix_device(None, C.cast(g, C.c_void_p), C.cast(out_G, C.c_void_p), C.cast(out_f, C.c_void_p)) == LEXLS_ERR_INVALID
    assert lib.lexls_internal_apply_solve_map(None, C.cast(g, C.c_void_p), C.cast(out_G, C.c_void_p)) == LEXLS_ERR_INVALID
    assert list(out_G) == [7.0] * 4 and list(out_f) == [7] * 4


def test_the_header_states_the_formula_the_rule_the_layouts_and_the_error_rules():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lse_solve_adjoint_matrix\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lse_solve_adjoint_matrix"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("dloss/dA_k = - y_k x^T - lambda_k u^T", "dloss/db = y", "y = M^T g", "u = M y~", "multipliers of level k", "its residual r = A_k",
                   "rank_k == min(dim_k, nVar - Fc_k) for every level k", "a problem with every variable fixed is rank-stable",
                   "a level that finds the columns used up has rank 0 and passes", "where Fc_k >= nVar",
                   "g is batch x nVar", "grad_lod is batch x (nVar + 1) x cap", "j cap + i", "column nVar is y",
                   "rows behind the problem's own are zero", "one byte per problem", "exact zeros",
                   "either output may be NULL", "(NULL: not wanted; d_grad_lod may not be NULL)", "no host-synchronising call",
                   "Tolerance contract", "the same bits from run to run",
                   "LEXLS_ERR_INVALID for a null handle, a null g or a null d_grad_lod", "LEXLS_ERR_INVALID when there is no kept factor",
                   "LEXLS_ERR_INVALID when no x belongs to the current factor",
                   "LEXLS_ERR_UNSUPPORTED when the factorization ran with regularization_type != 0", "before any device work",
                   "belong to the current factor", "solve_adjoint_matrix<64>"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    import subprocess
    import sys
    code = ("import sys; import lexls_amd.torch_adjoint as t, lexls_amd.lexlse as l; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert hasattr(l.BatchedLexLSE, 'solve_adjoint_matrix') and hasattr(l.BatchedLexLSE, 'solve_adjoint_matrix_device') and callable(t.solve_lod)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
