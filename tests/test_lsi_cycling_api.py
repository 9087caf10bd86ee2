"""LexLSI::getCyclingCounter() of a batch (lexls_lsi_batch_get_cycling_counters) is part of the C ABI and of the Python binding.  No GPU needed:
the symbol, its argument types, the method and the header's documentation only."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "lexls_lsi_batch_get_cycling_counters"


def test_library_exports_the_entry_point():
    from lexls_amd import capi
    lib = capi.lib()
    assert hasattr(lib, NAME), f"{NAME} is not exported by liblexls_hip.so"
    assert NAME in capi.SYMBOLS, f"{NAME} is missing from lexls_amd.capi.SYMBOLS"
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.POINTER(C.c_uint32)]


def test_python_binding_has_the_method():
    from lexls_amd import lexlsi
    assert callable(getattr(lexlsi.LsiBatch, "cycling_counters"))


def test_header_documents_the_entry_point():
    text = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    assert re.search(r"int\s+" + NAME + r"\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*uint32_t\s*\*\s*h_counts\s*\)\s*;", text)
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "getCyclingCounter" in comment  # the reference member it replaces
    assert "LEXLS_ERR_INVALID" in comment


def test_null_handle_is_an_error_not_a_crash():
    from lexls_amd import capi
    assert getattr(capi.lib(), NAME)(None, None) != 0
