"""The collecting removal search (lexls_lse_sensitivity_collect, the device form of ObjectiveSensitivity(ObjIndex, tolW, tolC, ctr_wrong_sign),
lexlse.h:511-602) is part of the C ABI and of the Python binding.  No GPU needed: symbols, argument types and the array id only."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ["lexls_lse_sensitivity_collect", "lexls_lse_sensitivity_collect_resident", "lexls_lse_get_wrong_sign"]


def test_library_exports_the_collect_entry_points():
    from lexls_amd import capi
    lib = capi.lib()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by liblexls_hip.so"
        assert name in capi.SYMBOLS, f"{name} is missing from lexls_amd.capi.SYMBOLS"
    assert lib.lexls_lse_sensitivity_collect.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_double]
    assert lib.lexls_lse_sensitivity_collect_resident.argtypes == [C.c_void_p, C.c_double, C.c_double]
    assert lib.lexls_lse_get_wrong_sign.argtypes == [C.c_void_p, C.POINTER(C.c_uint8)]


def test_wrong_sign_array_continues_the_numbering():
    """LEXLS_ARRAY_WRONG_SIGN is the id behind the last one of enum lexls_array (whose ids keep their values) and capi.ARRAY knows it"""
    from lexls_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lexls_hip.h")).read(), flags=re.S)
    body = re.search(r"enum\s+lexls_array\s*\{(.*?)\}", text, flags=re.S).group(1)
    names = re.findall(r"\b(LEXLS_ARRAY_[A-Z_]+)\b", body)
    assert names[-1] == "LEXLS_ARRAY_MULTIPLIERS", names
    assert re.search(r"LEXLS_ARRAY_WRONG_SIGN\s*=\s*LEXLS_ARRAY_MULTIPLIERS\s*\+\s*1\b", text)
    assert capi.ARRAY["wrong_sign"] == len(names) == capi.ARRAY["multipliers"] + 1


def test_python_binding_has_the_methods():
    import lexls_amd
    assert callable(getattr(lexls_amd.BatchedLexLSE, "sensitivity_collect")) and callable(getattr(lexls_amd.BatchedLexLSE, "wrong_sign"))


def test_null_handle_is_an_error_not_a_crash():
    from lexls_amd import capi
    lib = capi.lib()
    assert lib.lexls_lse_sensitivity_collect(None, None, 0, 1e-8, 1e-12) != 0
    assert lib.lexls_lse_sensitivity_collect_resident(None, 1e-8, 1e-12) != 0
    assert lib.lexls_lse_get_wrong_sign(None, None) != 0
