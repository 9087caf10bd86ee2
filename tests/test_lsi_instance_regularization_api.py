"""lexls_lsi_batch_set_instance_regularization (regularization factors of its own for every instance of a LexLSI batch) is part of the C ABI
and of the Python binding.  No GPU needed: the symbol, its argument types, LsiBatch.set_instance_regularization and what the header promises
about the call — its three error cases among it."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

NAME = "lexls_lsi_batch_set_instance_regularization"
LEXLS_ERR_INVALID = 1


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
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.c_void_p, C.c_int]  # handle, host or device address of the factors, in_device_memory
    assert getattr(lib, NAME).restype == C.c_int


def test_header_declares_it():
    decl = r"int\s+" + NAME + r"\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*factors\s*,\s*int\s+in_device_memory\s*\)\s*;"
    assert re.search(decl, header())


def test_no_existing_signature_changed():
    from lexls_amd import capi
    lib = capi.lib()
    assert len(lib.lexls_lsi_batch_run_device.argtypes) == 12 and len(lib.lexls_lsi_batch_run_device_ex.argtypes) == 15
    h = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    run = re.search(r"int\s+lexls_lsi_batch_run\s*\((.*?)\)\s*;", h, flags=re.S).group(1)
    assert run.count(",") == 13 and "h_reg_factors" in run


def test_header_states_the_rules():
    c = comment_of(header())
    assert "batch x nObj" in c and "instance-major" in c and "factors[b * nObj + k]" in c  # the layout
    assert "simple-bounds objective 0 is ignored" in c
    assert "factors == NULL clears the setting" in c
    assert "in_device_memory == 0: the array is copied at the call" in c
    assert "in_device_memory == 1: the POINTER is kept" in c and "start of every run" in c
    for run in ("lexls_lsi_batch_run", "lexls_lsi_batch_run_device", "lexls_lsi_batch_run_device_ex"):
        assert run in c, run
    assert "regularization_type 0 ignores the setting" in c
    assert "lexls_lsi_batch_solve*" in c and "shared factors only" in c
    # the call's error cases: null handle; device factors on a batch that can never be resident
    assert "LEXLS_ERR_INVALID for a null handle" in c
    assert re.search(r"LEXLS_ERR_UNSUPPORTED for in_device_memory == 1 on a batch whose regularized runs cannot be resident at all", c)
    # the runs' error cases while the setting holds
    assert "LEXLS_ERR_INVALID when h_reg_factors is not NULL" in c
    assert re.search(r"LEXLS_ERR_UNSUPPORTED when device factors are set and the regularized run would not be resident", c)
    assert re.search(r"LEXLS_ERR_UNSUPPORTED when device factors are set and lexls_lsi_batch_run is given h_v0", c)
    assert "before any work" in c and "every output left alone" in c
    # what it does on each path
    assert "lsi_instance_factors_kernel" in c and "never copied to the host" in c
    assert "as if LEXLS_LSI_DEVICE_PHASE1=1 were set for that run" in c
    assert "one-by-one path" in c and "host factors only" in c
    assert "lexls_lsi_batch_get_lambda after a regularized run stays LEXLS_ERR_UNSUPPORTED" in c
    assert header().index("int " + NAME) < header().index("/* How a run executes")  # next to that section


def test_python_binding_has_the_method():
    from lexls_amd import lexlsi
    assert hasattr(lexlsi.LsiBatch, "set_instance_regularization")
    par = inspect.signature(lexlsi.LsiBatch.set_instance_regularization).parameters
    assert list(par) == ["self", "factors"]
    doc = lexlsi.LsiBatch.set_instance_regularization.__doc__
    assert NAME in doc and "None clears" in doc


def test_null_handle_is_an_error_not_a_crash():
    from lexls_amd import capi
    assert getattr(capi.lib(), NAME)(None, None, 0) == LEXLS_ERR_INVALID
