"""The adjoint of the LexLSE solve in the C ABI: declared in include/lexls_hip.h, exported by the library, listed in capi.SYMBOLS, documented
where callers read, and refusing a null handle before anything else.  No GPU."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lexls_lse_solve_adjoint", "lexls_lse_get_adjoint", "lexls_lse_solve_adjoint_device")
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
    assert re.search(r"lexls_lse_solve_adjoint\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*h_g\s*\)", code)
    assert re.search(r"lexls_lse_get_adjoint\s*\(\s*lexls_lse_t\s+h\s*,\s*double\s*\*\s*h_grad_rhs\s*,\s*double\s*\*\s*h_grad_fixed\s*\)", code)
    assert re.search(r"lexls_lse_solve_adjoint_device\s*\(\s*lexls_lse_t\s+h\s*,\s*const\s+double\s*\*\s*d_g\s*,\s*double\s*\*\s*d_grad_rhs\s*,"
                     r"\s*double\s*\*\s*d_grad_fixed\s*\)", code)


def test_a_null_handle_is_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out_rhs, out_fixed = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    assert lib.lexls_lse_solve_adjoint(None, g) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lse_get_adjoint(None, out_rhs, out_fixed) == LEXLS_ERR_INVALID
    assert lib.lexls_lse_solve_adjoint_device(None, C.cast(g, C.c_void_p), C.cast(out_rhs, C.c_void_p), C.cast(out_fixed, C.c_void_p)) == LEXLS_ERR_INVALID
    assert list(out_rhs) == [7.0] * 4 and list(out_fixed) == [7.0] * 4


def test_the_header_states_the_layouts_and_the_error_rules():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lse_solve_adjoint\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lse_solve_adjoint"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("x = M b + N x_fixed", "A HELD FIXED", "NO derivatives with respect to A", "not continuous in A",
                   "g is batch x nVar", "grad_rhs is batch x cap", "LOD row order", "grad_fixed is batch x nVar", "fixVariable order",
                   "either output may be NULL", "(NULL: not wanted)", "no host-synchronising call",
                   "LEXLS_ERR_INVALID for a null handle or a null g", "LEXLS_ERR_INVALID when there is no kept factor",
                   "LEXLS_ERR_UNSUPPORTED when the factorization ran with regularization_type != 0", "before any device work",
                   "belong to the current factor"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    import subprocess
    import sys
    code = ("import sys; import lexls_amd.torch_adjoint as t, lexls_amd.lexlse as l; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert hasattr(l.BatchedLexLSE, 'solve_adjoint') and hasattr(l.BatchedLexLSE, 'solve_adjoint_device') and callable(t.solve_rhs)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
