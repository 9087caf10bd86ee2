"""lexls_lsi_batch_enqueue_device / lexls_lsi_batch_finish without a device: both symbols are in the header with the documented prototypes, in the
library and in the ctypes mirror; a null handle is LEXLS_ERR_INVALID; LsiBatch has the two methods with the documented keywords."""
import ctypes as C
import inspect
import os
import re

from lexls_amd import capi, lexlsi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEXLS_ERR_INVALID = 1


def prototype(name):
    text = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name + " is not declared in include/lexls_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_prototypes_in_the_header():
    assert prototype("lexls_lsi_batch_enqueue_device") == [
        "lexls_lsi_batch_t b", "void *hip_stream", "const double *d_data", "const uint32_t *d_var_index", "const uint8_t *d_active_guess", "const double *d_x0",
        "const double *d_v0", "const double *h_reg_factors", "const double *h_params", "uint32_t nparams", "double *d_x", "int32_t *d_info6", "uint8_t *d_active",
        "double *d_v", "double *d_lambda", "uint32_t *d_cycling_counts", "uint32_t *d_status"]
    assert prototype("lexls_lsi_batch_finish") == ["lexls_lsi_batch_t b", "void *hip_stream"]
    # the arguments between the stream and d_status are those of lexls_lsi_batch_run_device_ex
    assert prototype("lexls_lsi_batch_enqueue_device")[2:-1] == prototype("lexls_lsi_batch_run_device_ex")[1:]


def test_symbols_in_the_library_and_the_ctypes_mirror():
    lib = capi.lib()
    for name in ("lexls_lsi_batch_enqueue_device", "lexls_lsi_batch_finish"):
        assert name in capi.SYMBOLS
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.lexls_lsi_batch_enqueue_device.argtypes) == 17
    assert len(lib.lexls_lsi_batch_finish.argtypes) == 2


def test_null_handle_is_invalid():
    lib = capi.lib()
    none = [None] * 6
    assert lib.lexls_lsi_batch_enqueue_device(None, None, *none, None, 0, *none, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_finish(None, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()


def test_python_methods():
    enqueue = inspect.signature(lexlsi.LsiBatch.enqueue_device).parameters
    run = inspect.signature(lexlsi.LsiBatch.run_device).parameters
    assert [k for k in run if k in enqueue] == list(run), "enqueue_device mirrors run_device's keyword set"
    assert enqueue["stream"].default is None and enqueue["status"].default is None
    assert list(inspect.signature(lexlsi.LsiBatch.finish).parameters) == ["self", "stream"]
