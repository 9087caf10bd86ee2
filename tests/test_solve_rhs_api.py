"""The entries for new right-hand sides on a kept factor (lexls_lse_solve_rhs, lexls_lse_get_solve_rhs, lexls_lse_solve_rhs_device) are declared,
exported and bound with the right argument types, refuse what they have to refuse without a device, and the Python and torch layers have their
methods.  No compute calls here."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

INVALID = 1
NAMES = ["lexls_lse_solve_rhs", "lexls_lse_get_solve_rhs", "lexls_lse_solve_rhs_device"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lexls_hip.h")).read(), flags=re.S)


def test_the_symbols_are_in_the_header_in_the_library_and_in_the_binding():
    from lexls_amd import capi
    lib = capi.lib()
    declared = set(re.findall(r"\b(lexls_[a-z0-9_]+)\s*\(", header_text()))
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int
    dp = C.POINTER(C.c_double)
    assert lib.lexls_lse_solve_rhs.argtypes == [C.c_void_p, dp, dp, C.c_uint32]
    assert lib.lexls_lse_get_solve_rhs.argtypes == [C.c_void_p, dp]
    assert lib.lexls_lse_solve_rhs_device.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    text = header_text()
    assert re.search(r"int\s+lexls_lse_solve_rhs\(lexls_lse_t h, const double \*h_rhs, const double \*h_fixed, uint32_t nrhs\);", text)
    assert re.search(r"int\s+lexls_lse_get_solve_rhs\(lexls_lse_t h, double \*h_x\);", text)
    assert re.search(r"int\s+lexls_lse_solve_rhs_device\(lexls_lse_t h, const double \*d_rhs, const double \*d_fixed, uint32_t nrhs, double \*d_x\);", text)


def test_null_handle_null_arguments_and_bad_counts_are_invalid():
    from lexls_amd import capi
    lib = capi.lib()
    d = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    assert lib.lexls_lse_solve_rhs(None, d, None, 1) == INVALID
    assert lib.lexls_lse_solve_rhs(None, None, None, 1) == INVALID
    assert lib.lexls_lse_solve_rhs(None, d, None, 0) == INVALID
    assert lib.lexls_lse_solve_rhs(None, d, None, 65536) == INVALID
    assert lib.lexls_lse_get_solve_rhs(None, d) == INVALID
    assert lib.lexls_lse_solve_rhs_device(None, C.c_void_p(8), None, 1, C.c_void_p(8)) == INVALID
    assert lib.lexls_lse_solve_rhs_device(None, C.c_void_p(8), None, 1, None) == INVALID
    assert list(d) == [7.0] * 4


def test_the_python_and_torch_layers_have_the_methods():
    from lexls_amd import torch_adjoint
    from lexls_amd.lexlse import BatchedLexLSE
    assert list(inspect.signature(BatchedLexLSE.solve_rhs).parameters) == ["self", "rhs", "fixed"]
    assert list(inspect.signature(BatchedLexLSE.solve_rhs_device).parameters) == ["self", "rhs", "x", "fixed"]
    assert list(inspect.signature(torch_adjoint.solve_new_rhs).parameters) == ["solver", "rhs", "fixed"]
    assert list(inspect.signature(torch_adjoint.jvp_rhs).parameters) == ["solver", "drhs", "dfixed"]
    assert "zeros" in torch_adjoint.jvp_rhs.__doc__ and "constant part" in torch_adjoint.jvp_rhs.__doc__
    assert list(inspect.signature(torch_adjoint.solve_rhs).parameters) == ["rhs", "lse", "lod"]  # the factorizing operation keeps its signature
