"""The accuracy guard's interface without a GPU: the C ABI exports it, the ctypes prototypes and the Python methods exist, the device-array
ids follow the header, and the problem generators of its test sets are deterministic and of the documented kind."""
import os
import re

import numpy as np

from conftest import ROOT


def test_guard_symbols_exported_and_declared():
    from lexls_amd import capi
    lib = capi.lib()
    for name in ("lexls_lse_set_accuracy_guard", "lexls_lse_get_accuracy"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    assert lib.lexls_lse_set_accuracy_guard.argtypes is not None and lib.lexls_lse_get_accuracy.argtypes is not None


def test_guard_array_ids_follow_the_header():
    from lexls_amd import capi
    text = open(os.path.join(ROOT, "include", "lexls_hip.h")).read()
    body = re.search(r"enum lexls_array\s*\{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\b(LEXLS_ARRAY_[A-Z_]+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names.index("LEXLS_ARRAY_GUARD_ESTIMATE") == capi.ARRAY["guard_estimate"] == 10
    assert names.index("LEXLS_ARRAY_GUARD_STATUS") == capi.ARRAY["guard_status"] == 11


def test_python_methods():
    from lexls_amd import BatchedLexLSE
    assert callable(BatchedLexLSE.set_accuracy_guard) and callable(BatchedLexLSE.get_accuracy)


def test_generators():
    from lexls_amd import problems as P
    a = P.near_dependent_batch(7, 6, 10, [12, 12], 1e-6)
    assert a.shape == (6, 11, 24) and np.array_equal(a, P.near_dependent_batch(7, 6, 10, [12, 12], 1e-6))
    base = P.lse_batch_fast(7, 6, 10, [12, 12])
    for b in range(6):
        changed = [c for c in range(10) if not np.array_equal(a[b, c], base[b, c])]
        assert len(changed) == 1  # one column replaced by a combination of two others plus 1e-6 noise
        k = changed[0]
        others = np.delete(a[b, :10], k, axis=0)
        coef, *_ = np.linalg.lstsq(others.T, a[b, k], rcond=None)
        assert np.linalg.norm(others.T @ coef - a[b, k]) < 1e-5 and np.count_nonzero(np.abs(coef) > 1e-3) == 2
    s = P.badly_scaled_batch(8, 4, 10, [4, 4])
    ratio = s / P.lse_batch_fast(8, 4, 10, [4, 4])
    assert np.allclose(ratio, ratio[:, :, :1] * ratio[:, :1, :] / ratio[:, :1, :1])  # rank-one scaling: columns x rows
    assert 1e-5 <= np.abs(ratio).min() and np.abs(ratio).max() <= 1e5
