"""Gradients of batched LexLSI solutions with respect to the bounds in the C ABI: declared in include/lexls_hip.h, exported by the library,
listed in capi.SYMBOLS, documented where callers read, and refusing a null handle before anything else.  No GPU."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lexls_lsi_batch_solve_adjoint", "lexls_lsi_batch_solve_adjoint_device")
LEXLS_ERR_INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_two_symbols_are_declared_exported_and_listed():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
    assert re.search(r"\bint\s+lexls_lsi_batch_solve_adjoint\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*h_g\s*,\s*double\s*\*\s*h_grad_lb\s*,"
                     r"\s*double\s*\*\s*h_grad_ub\s*\)", code)
    assert re.search(r"\bint\s+lexls_lsi_batch_solve_adjoint_device\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*d_g\s*,\s*double\s*\*\s*d_grad_lb\s*,"
                     r"\s*double\s*\*\s*d_grad_ub\s*\)", code)


def test_a_null_handle_is_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out_lb, out_ub = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    assert lib.lexls_lsi_batch_solve_adjoint(None, g, out_lb, out_ub) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_device(None, C.cast(g, C.c_void_p), C.cast(out_lb, C.c_void_p), C.cast(out_ub, C.c_void_p)) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert list(out_lb) == [7.0] * 4 and list(out_ub) == [7.0] * 4


def test_the_header_states_the_layouts_and_the_rules():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lsi_batch_solve_adjoint\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lsi_batch_solve_adjoint"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("A HELD FIXED", "NO derivatives with respect to A",
                   "g is batch x nVar", "user's variable order", "grad_lb and grad_ub are batch x sum(dims) each", "constraint order of h_active / h_v",
                   "Either output may be NULL", "host-synchronous", "passes through host memory",
                   "CTR_ACTIVE_LB — the value goes to grad_lb", "CTR_ACTIVE_UB — the value goes to grad_ub", "CTR_ACTIVE_EQ — the value goes to grad_ub",
                   "grad_fixed of their slot", "not in the working set is exactly 0", "lexls_lsi_batch_set_instance_obj_dims",
                   "Status rule", "ANY OTHER status", "gets zeros in all its rows", "never read from an array of the caller",
                   "Mask rule", "keeps the bits of its rows in both outputs",
                   "piecewise-affine", "one-sided", "Tolerance contract", "same bits from run to run and from the host and the device form",
                   "before any device work and with every output left alone", "LEXLS_ERR_INVALID for a null handle, a null g, or both outputs null",
                   "no completed run", "waiting for lexls_lsi_batch_finish",
                   "LEXLS_ERR_UNSUPPORTED after exactly the runs for which lexls_lsi_batch_get_lambda answers LEXLS_ERR_UNSUPPORTED"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    import subprocess
    import sys
    code = ("import sys; import lexls_amd.torch_adjoint as t, lexls_amd.lexlsi as l; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert callable(l.LsiBatch.solve_adjoint) and callable(l.LsiBatch.solve_adjoint_device); "
            "assert callable(t.solve_bounds) and callable(t.solve_rhs)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
