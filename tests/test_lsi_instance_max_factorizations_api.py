"""lexls_lsi_batch_set_instance_max_factorizations without a device: the symbol is in the header with the documented prototype, in the library and
in the ctypes mirror; a null handle is LEXLS_ERR_INVALID; LsiBatch has set_instance_max_factorizations and the entries it serves gained no
argument; the header's comment states the contract — the pointer is kept, the limits are read per run, NULL clears the setting,
lexls_lsi_batch_run answers LEXLS_ERR_UNSUPPORTED while it is set."""
import ctypes as C
import inspect
import os
import re

from lexls_amd import capi, lexlsi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEXLS_ERR_INVALID = 1
NAME = "lexls_lsi_batch_set_instance_max_factorizations"


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_prototype_in_the_header():
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, NAME + " is not declared in include/lexls_hip.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ["lexls_lsi_batch_t b", "const int32_t *d_limits"]


def test_symbol_in_the_library_and_the_ctypes_mirror():
    lib = capi.lib()
    assert NAME in capi.SYMBOLS
    assert getattr(lib, NAME).restype is C.c_int
    assert len(getattr(lib, NAME).argtypes) == 2


def test_null_handle_is_invalid():
    lib = capi.lib()
    assert getattr(lib, NAME)(None, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()


def test_python_method():
    assert list(inspect.signature(lexlsi.LsiBatch.set_instance_max_factorizations).parameters) == ["self", "limits"]
    # the entries the limits serve keep their signatures: no new argument anywhere
    want = dict(run_device=["self", "data", "var_index", "active_guess", "x0", "regularization_factors", "v0", "with_lambda", "with_cycling_counters", "params"],
                enqueue_device=["self", "data", "var_index", "active_guess", "x0", "regularization_factors", "v0", "with_lambda", "with_cycling_counters", "stream",
                                "status", "out", "params"],
                finish=["self", "stream"])
    for name, parameters in want.items():
        assert list(inspect.signature(getattr(lexlsi.LsiBatch, name)).parameters) == parameters, name


def test_the_header_states_the_contract():
    """the comment in front of the declaration, with its line breaks and comment stars taken out"""
    text = header()
    end = text.index("int " + NAME + "(")
    start = text.rindex("/*", 0, end)
    comment = re.sub(r"\s+", " ", text[start:end].replace("\n *", " "))
    for phrase in ("The pointer is kept", "The limits are read per run", "d_limits == NULL clears the setting", "LEXLS_ERR_UNSUPPORTED"):
        assert phrase in comment, phrase
