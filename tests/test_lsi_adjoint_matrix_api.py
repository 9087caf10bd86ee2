"""Gradients of batched LexLSI solutions with respect to the constraint matrices in the C ABI: declared in include/lexls_hip.h, exported by the
library, listed in capi.SYMBOLS and bound, documented where callers read, refusing null arguments before anything else; the Python surface.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from conftest import ROOT

NAMES = ("lexls_lsi_batch_solve_adjoint_matrix", "lexls_lsi_batch_solve_adjoint_matrix_device")
LEXLS_ERR_INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_two_symbols_are_declared_exported_listed_and_bound():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == 4, f"{name} is not bound"
    assert re.search(r"\bint\s+lexls_lsi_batch_solve_adjoint_matrix\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*h_g\s*,\s*double\s*\*\s*h_grad_data\s*,"
                     r"\s*uint8_t\s*\*\s*h_differentiable\s*\)", code)
    assert re.search(r"\bint\s+lexls_lsi_batch_solve_adjoint_matrix_device\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*const\s+double\s*\*\s*d_g\s*,\s*double\s*\*\s*d_grad_data\s*,"
                     r"\s*uint8_t\s*\*\s*d_differentiable\s*\)", code)


def test_null_arguments_are_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    g = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out, flag = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_uint8 * 2)(9, 9)
    assert lib.lexls_lsi_batch_solve_adjoint_matrix(None, g, out, flag) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_matrix_device(None, C.cast(g, C.c_void_p), C.cast(out, C.c_void_p), C.cast(flag, C.c_void_p)) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert list(out) == [7.0] * 4 and list(flag) == [9, 9]


def test_the_header_states_the_layouts_and_the_rules():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lsi_batch_solve_adjoint_matrix\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lsi_batch_solve_adjoint_matrix"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("g is batch x nVar", "exactly the layout lexls_lsi_batch_run_device reads", "w = nVar + 2", "w = 2 for simple bounds", "grad_data may not be NULL",
                   "- y x^T - lambda u^T", "CTR_ACTIVE_EQ", "N^T g", "lexls_lsi_batch_set_instance_obj_dims", "exact zeros",
                   "Flag rule", "PROBLEM_SOLVED", "rank-stable", "empty working set is differentiable", "WHOLE slice", "bound columns included",
                   "still gives", "Mask rule", "keeps the bits of its slice and of its flag", "host-synchronous", "passes through host memory",
                   "no atomics", "same bits from run to run and from the host and the device form", "nothing is factorized twice",
                   "before any device work and with every output left alone", "null grad_data", "cycling handling", "a regularized run",
                   "more than 65535 constraints", "constraint data not resident"):
        assert phrase in doc, f"the header comment does not state: {phrase}"
    assert "lexls_lsi_batch_solve_adjoint_matrix" in re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lsi_batch_solve_adjoint\(", text, flags=re.S).group(1)


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    code = ("import sys; import lexls_amd.torch_adjoint as t, lexls_amd.lexlsi as l; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert callable(l.LsiBatch.solve_adjoint_matrix) and callable(l.LsiBatch.solve_adjoint_matrix_device) and callable(l.LsiBatch.split_grad_data); "
            "assert callable(t.solve_data); assert 'torch' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_split_grad_data_is_the_inverse_of_flatten():
    from lexls_amd import lexlsi
    from lexls_amd import problems as P
    n, objs = 4, P.lsi_problem(20330201, 4, (4, 2, 3))
    dims, types, data, _ = lexlsi.flatten(n, objs)
    b = lexlsi.LsiBatch.__new__(lexlsi.LsiBatch)  # (the helper reads the structure alone: no handle, no device)
    b.nvar, b.dims, b.types, b._h = n, dims, types, None
    assert b.per_data == data.size
    parts = b.split_grad_data(data)
    assert len(parts) == 3 and set(parts[0]) == {"lb", "ub"} and set(parts[1]) == {"A", "lb", "ub"}
    for p, o in zip(parts, objs):
        for k in p:
            np.testing.assert_array_equal(p[k], np.asarray(o[k], float).reshape(p[k].shape))
