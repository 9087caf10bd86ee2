"""The multiplier outputs of batched solves (lexls_lse_multipliers / lexls_lse_get_multipliers, lexls_lsi_batch_get_lambda,
lexls_lsi_batch_solve_ex2): exported, declared, reachable from Python, and the device-array enum extended at its end only.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

NEW_SYMBOLS = ["lexls_lse_multipliers", "lexls_lse_get_multipliers", "lexls_lsi_batch_get_lambda", "lexls_lsi_batch_solve_ex2"]
OLD_ARRAY_IDS = ["LEXLS_ARRAY_X", "LEXLS_ARRAY_FACTOR", "LEXLS_ARRAY_HH", "LEXLS_ARRAY_PERM", "LEXLS_ARRAY_RANK", "LEXLS_ARRAY_FIRST_COL",
                 "LEXLS_ARRAY_TOTAL_RANK", "LEXLS_ARRAY_V", "LEXLS_ARRAY_LAMBDA", "LEXLS_ARRAY_INPUT", "LEXLS_ARRAY_GUARD_ESTIMATE",
                 "LEXLS_ARRAY_GUARD_STATUS"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lexls_hip.h")).read(), flags=re.S)


def test_new_symbols_exported_declared_and_listed():
    from lexls_amd import capi
    lib = capi.lib()
    text = header_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS, name


def test_array_id_appended_last():
    text = header_text()
    body = re.search(r"enum\s+lexls_array\s*\{(.*?)\}", text, flags=re.S).group(1)
    names = [e.split("=")[0].strip() for e in body.split(",") if e.strip()]
    assert names[:len(OLD_ARRAY_IDS)] == OLD_ARRAY_IDS  # the old ids keep their values (0, 1, ..., 11)
    assert names[-1] == "LEXLS_ARRAY_MULTIPLIERS" and len(names) == len(OLD_ARRAY_IDS) + 1
    assert "LEXLS_ARRAY_X = 0" in re.sub(r"\s+", " ", body)
    from lexls_amd import capi
    assert capi.ARRAY["multipliers"] == len(OLD_ARRAY_IDS)
    assert [capi.ARRAY[k] for k in ("x", "lam", "guard_status")] == [0, 8, 11]


def test_python_methods_exist():
    from lexls_amd import lexlse, lexlsi
    assert callable(getattr(lexlsi.LsiBatch, "lambdas", None))
    assert callable(getattr(lexlsi.LsiBatch, "lambda_array", None))
    assert callable(getattr(lexlse.BatchedLexLSE, "multipliers", None))
    sig = inspect.signature(lexlsi.lsi_batch_solve)
    assert "with_lambda" in sig.parameters and sig.parameters["with_lambda"].default is False


def test_null_handles_are_refused():
    from lexls_amd import capi
    lib = capi.lib()
    buf = (C.c_double * 4)()
    assert lib.lexls_lsi_batch_get_lambda(None, buf) == 1  # LEXLS_ERR_INVALID
    assert lib.lexls_lse_multipliers(None) == 1
    assert lib.lexls_lse_get_multipliers(None, buf) == 1
