"""lexls_lsi_batch_last_kernel (the kernel that served the resident iterations of a lock-step LexLSI run): declared, exported, listed, bound
and reachable from Python.  No GPU needed."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_symbol_declared_exported_and_listed():
    from lexls_amd import capi
    lib = capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lexls_hip.h")).read(), flags=re.S)
    assert re.search(r"const\s+char\s*\*\s*lexls_lsi_batch_last_kernel\s*\(\s*lexls_lsi_batch_t\s+\w+\s*\)\s*;", text)
    assert hasattr(lib, "lexls_lsi_batch_last_kernel")
    assert "lexls_lsi_batch_last_kernel" in capi.SYMBOLS
    assert capi.SYMBOLS[-1] == "lexls_lsi_batch_last_kernel"  # appended


def test_bound_as_a_string_function():
    from lexls_amd import capi
    f = capi.lib().lexls_lsi_batch_last_kernel
    assert f.restype is C.c_char_p
    assert f(None) == b""  # no batch: the empty name, not a crash


def test_python_method_exists():
    from lexls_amd import lexlsi
    assert callable(getattr(lexlsi.LsiBatch, "last_kernel", None))
