"""The forward-mode entries of the C ABI (lexls_lse_solve_tangent, lexls_lse_get_tangent, lexls_lse_solve_tangent_device) are declared, exported
and bound, refuse what they have to refuse without a device, and the solve map itself stays internal.  No compute calls here."""
import ctypes as C
import os
import re

from conftest import ROOT

INVALID = 1
NAMES = ["lexls_lse_solve_tangent", "lexls_lse_get_tangent", "lexls_lse_solve_tangent_device"]


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


def test_null_handle_null_outputs_and_no_tangents_are_invalid():
    from lexls_amd import capi
    lib = capi.lib()
    d = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    f = (C.c_uint8 * 4)(7, 7, 7, 7)
    assert lib.lexls_lse_solve_tangent(None, d, None, 1) == INVALID
    assert lib.lexls_lse_solve_tangent(None, d, None, 0) == INVALID
    assert lib.lexls_lse_get_tangent(None, d, f) == INVALID
    assert lib.lexls_lse_solve_tangent_device(None, C.c_void_p(8), None, 1, C.c_void_p(8), None) == INVALID
    assert lib.lexls_lse_solve_tangent_device(None, C.c_void_p(8), None, 1, None, None) == INVALID  # null d_dx
    assert lib.lexls_lse_solve_tangent_device(None, C.c_void_p(8), None, 0, C.c_void_p(8), None) == INVALID  # ntan == 0
    assert list(d) == [7.0] * 4 and list(f) == [7] * 4


def test_the_solve_map_stays_internal():
    """no forward multi-right-hand-side solve in the public header: the tangent entries are derivatives of the solve, apply_solve_map is not public"""
    text = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    assert "apply_solve_map" not in header_text()
    assert not re.search(r"\blexls_[a-z0-9_]*apply_solve_map[a-z0-9_]*\s*\(", text)
    from lexls_amd import capi
    assert not [s for s in capi.SYMBOLS if "apply_solve_map" in s]
