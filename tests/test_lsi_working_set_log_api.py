"""The C ABI and the Python layer of the batched working-set log, as far as they can be checked without a device: the three entry points are
exported with the prototypes include/lexls_hip.h states, lexls_amd.capi declares them, the errors that are decidable before any device work
(a null handle) are reported, and the header's row layout is the one the Python decoder uses.  The log itself is compared with the oracle on
the GPU (test_gpu_lsi_working_set_log.py)."""
import ctypes as C
import os
import re

from conftest import ROOT

from lexls_amd import capi, lexlsi

LEXLS_ERR_INVALID = 1
PROTOTYPES = {
    "lexls_lsi_batch_set_working_set_log": "int lexls_lsi_batch_set_working_set_log(lexls_lsi_batch_t b, uint32_t max_entries);",
    "lexls_lsi_batch_get_working_set_log": "int lexls_lsi_batch_get_working_set_log(lexls_lsi_batch_t b, int32_t *h_log, double *h_alpha, uint32_t *h_counts);",
    "lexls_lsi_batch_working_set_log_device": "int lexls_lsi_batch_working_set_log_device(lexls_lsi_batch_t b, void **d_log, void **d_alpha, void **d_counts);",
}
ARGTYPES = {
    "lexls_lsi_batch_set_working_set_log": [C.c_void_p, C.c_uint32],
    "lexls_lsi_batch_get_working_set_log": [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)],
    "lexls_lsi_batch_working_set_log_device": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
}


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_library_exports_the_three_entry_points():
    lib = capi.lib()
    for name in PROTOTYPES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"


def test_the_header_states_the_prototypes():
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header(), flags=re.S))
    for name, proto in PROTOTYPES.items():
        assert proto in text, name


def test_capi_declares_them():
    lib = capi.lib()
    for name, argtypes in ARGTYPES.items():
        assert name in capi.SYMBOLS
        f = getattr(lib, name)
        assert f.restype is C.c_int and list(f.argtypes) == argtypes, name


def test_null_handle_is_invalid():
    lib = capi.lib()
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    assert lib.lexls_lsi_batch_set_working_set_log(None, 16) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_set_working_set_log(None, 0) == LEXLS_ERR_INVALID
    assert lib.lexls_lsi_batch_get_working_set_log(None, None, None, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_working_set_log_device(None, *(C.byref(p) for p in out)) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert all(p.value is None for p in out)


def test_header_layout_matches_the_python_decoder():
    text = header()
    assert int(re.search(r"#define\s+LEXLS_LSI_LOG_FIELDS\s+(\d+)", text).group(1)) == len(capi.WORKING_SET_LOG_FIELDS) == 5
    index = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"LEXLS_LSI_LOG_([A-Z_]+?)\s*=\s*(\d+)", text)}
    assert index == {name: i for i, name in enumerate(capi.WORKING_SET_LOG_FIELDS)}
    # the single-problem decoder reads the same row (lexls_lsi_debug::log) at the same positions
    buf = lexlsi.debug_buffers(3, [2, 2], max_log=1)
    buf["log"][0] = [10, 11, 12, 13, 14]
    buf["log_alpha"][0] = 0.5
    buf["counts"][:] = [2, 2, 0, 1]
    entry = lexlsi.debug_structure(3, [2, 2], buf, False)["working_set_log"][0]
    assert [entry[k] for k in capi.WORKING_SET_LOG_FIELDS] == [10, 11, 12, 13, 14] and entry["alpha_or_lambda"] == 0.5
    for b in (lexlsi.LsiBatch.set_working_set_log, lexlsi.LsiBatch.working_set_log, lexlsi.LsiBatch.working_set_log_device):
        assert callable(b)
