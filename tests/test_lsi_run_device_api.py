"""lexls_lsi_batch_run_device (a lock-step LexLSI batch solved from device memory, phase 1 on the device) is part of the C ABI and of the Python
binding.  No GPU needed: the symbol, its argument types, the method and the header's documentation only."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "lexls_lsi_batch_run_device"


def test_library_exports_the_entry_point():
    from lexls_amd import capi
    lib = capi.lib()
    assert hasattr(lib, NAME), f"{NAME} is not exported by liblexls_hip.so"
    assert NAME in capi.SYMBOLS, f"{NAME} is missing from lexls_amd.capi.SYMBOLS"
    dev = C.c_void_p  # a device address
    assert getattr(lib, NAME).argtypes == [C.c_void_p, dev, dev, dev, dev, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, dev, dev, dev, dev]
    assert getattr(lib, NAME).restype == C.c_int


def test_python_binding_has_the_method():
    from lexls_amd import lexlsi
    assert callable(getattr(lexlsi.LsiBatch, "run_device"))


def test_header_documents_the_entry_point_and_the_switch():
    text = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    decl = (r"int\s+" + NAME + r"\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*d_data\s*,\s*const\s+uint32_t\s*\*\s*d_var_index\s*,"
            r"\s*const\s+uint8_t\s*\*\s*d_active_guess\s*,\s*const\s+double\s*\*\s*d_x0\s*,\s*const\s+double\s*\*\s*h_reg_factors\s*,"
            r"\s*const\s+double\s*\*\s*h_params\s*,\s*uint32_t\s+nparams\s*,\s*double\s*\*\s*d_x\s*,\s*int32_t\s*\*\s*d_info6\s*,"
            r"\s*uint8_t\s*\*\s*d_active\s*,\s*double\s*\*\s*d_v\s*\)\s*;")
    assert re.search(decl, text)
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    for member in ("h_data", "h_var_index", "h_active_guess", "h_x0", "h_x", "h_info6", "h_active", "h_v"):  # the members it replaces
        assert member in comment, member
    assert "LEXLS_ERR_UNSUPPORTED" in comment and "LEXLS_ERR_INVALID" in comment
    assert "LEXLS_LSI_DEVICE_PHASE1" in text
    how = text[text.index("How a run executes"):text.index("int lexls_lsi_batch_stats")]
    assert "LEXLS_LSI_DEVICE_PHASE1" in how and NAME in how


def test_null_handle_is_an_error_not_a_crash():
    from lexls_amd import capi
    assert getattr(capi.lib(), NAME)(None, None, None, None, None, None, None, 9, None, None, None, None) != 0
