"""lexls_lsi_batch_run_device_ex (lexls_lsi_batch_run_device plus initial residuals, multipliers and cycling counters in device memory) is part of
the C ABI and of the Python binding.  No GPU needed: the symbol, its argument types, the keywords of LsiBatch.run_device and what the header
promises about it."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

NAME = "lexls_lsi_batch_run_device_ex"
OLD = "lexls_lsi_batch_run_device"


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def comment_of(text):
    """the comment block in front of the declaration, the line starts' asterisks dropped and white space folded"""
    return " ".join(re.sub(r"\n\s*\*", "\n", text[:text.index("int " + NAME)].rsplit("/*", 1)[1]).split())


def test_library_exports_the_entry_point():
    from lexls_amd import capi
    lib = capi.lib()
    assert hasattr(lib, NAME), f"{NAME} is not exported by liblexls_hip.so"
    assert NAME in capi.SYMBOLS, f"{NAME} is missing from lexls_amd.capi.SYMBOLS"
    dev = C.c_void_p  # a device address
    argtypes = getattr(lib, NAME).argtypes
    assert len(argtypes) == 15
    assert argtypes == [C.c_void_p, dev, dev, dev, dev, dev, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, dev, dev, dev, dev, dev, dev]
    assert getattr(lib, NAME).restype == C.c_int
    assert len(getattr(lib, OLD).argtypes) == 12  # the old entry point keeps its signature


def test_header_declares_it():
    decl = (r"int\s+" + NAME + r"\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*d_data\s*,\s*const\s+uint32_t\s*\*\s*d_var_index\s*,"
            r"\s*const\s+uint8_t\s*\*\s*d_active_guess\s*,\s*const\s+double\s*\*\s*d_x0\s*,\s*const\s+double\s*\*\s*d_v0\s*,"
            r"\s*const\s+double\s*\*\s*h_reg_factors\s*,\s*const\s+double\s*\*\s*h_params\s*,\s*uint32_t\s+nparams\s*,\s*double\s*\*\s*d_x\s*,"
            r"\s*int32_t\s*\*\s*d_info6\s*,\s*uint8_t\s*\*\s*d_active\s*,\s*double\s*\*\s*d_v\s*,\s*double\s*\*\s*d_lambda\s*,"
            r"\s*uint32_t\s*\*\s*d_cycling_counts\s*\)\s*;")
    m = re.search(decl, header())
    assert m
    assert m.group(0).count(",") == 14  # 15 arguments


def test_header_states_the_rules():
    c = comment_of(header())
    assert "d_v0 without d_x0 is disregarded" in c and "lexlsi.h:695-701" in c  # the v0-without-x0 rule
    assert "initialize_v0" in c and "formInitialWorkingSet" in c and "A x0 is still formed" in c
    assert re.search(r"returns LEXLS_ERR_UNSUPPORTED when d_lambda is non-NULL, before any device work", c)  # the rule for d_lambda
    for case in ("cycling handling enabled", "regularization_type != 0", "more than 65535"):
        assert case in c, case
    assert OLD + " itself is unchanged" in c  # the old entry point
    assert "d_v0, d_lambda and d_cycling_counts all NULL" in c
    assert "lexls_lsi_batch_get_cycling_counters" in c and "zeros after a run without cycling handling" in c
    assert "LEXLS_LSI_DEVICE_PHASE1=1 still changes nothing when h_v0 is given" in c


def test_python_binding_has_the_keywords():
    from lexls_amd import lexlsi
    par = inspect.signature(lexlsi.LsiBatch.run_device).parameters
    assert par["v0"].default is None and par["with_lambda"].default is False and par["with_cycling_counters"].default is False
    doc = lexlsi.LsiBatch.run_device.__doc__
    assert NAME in doc and "cycling_counters" in doc


def test_null_handle_is_an_error_not_a_crash():
    from lexls_amd import capi
    assert getattr(capi.lib(), NAME)(None, None, None, None, None, None, None, None, 9, None, None, None, None, None, None) != 0
