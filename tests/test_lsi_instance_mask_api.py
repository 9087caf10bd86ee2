"""lexls_lsi_batch_set_instance_mask without a device: the symbol is in the header with the documented prototype, in the library and in the ctypes
mirror; a null handle is LEXLS_ERR_INVALID; LsiBatch has set_instance_mask; the header's comment states the contract — the pointer is kept, the
mask is read per run, caller-owned rows are untouched, lexls_lsi_batch_run is refused while the mask is set."""
import ctypes as C
import inspect
import os
import re

from lexls_amd import capi, lexlsi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEXLS_ERR_INVALID = 1
NAME = "lexls_lsi_batch_set_instance_mask"


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_prototype_in_the_header():
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, NAME + " is not declared in include/lexls_hip.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ["lexls_lsi_batch_t b", "const uint8_t *d_mask"]


def test_symbol_in_the_library_and_the_ctypes_mirror():
    lib = capi.lib()
    assert NAME in capi.SYMBOLS
    assert getattr(lib, NAME).restype is C.c_int
    assert len(getattr(lib, NAME).argtypes) == 2


def test_null_handle_is_invalid():
    lib = capi.lib()
    assert lib.lexls_lsi_batch_set_instance_mask(None, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()


def test_python_method():
    assert list(inspect.signature(lexlsi.LsiBatch.set_instance_mask).parameters) == ["self", "mask"]
    # the entries a mask serves keep their signatures: no mask argument anywhere
    for name in ("run_device", "enqueue_device", "finish"):
        assert "mask" not in inspect.signature(getattr(lexlsi.LsiBatch, name)).parameters


def test_the_header_states_the_contract():
    """the comment in front of the declaration, with its line breaks and comment stars taken out"""
    text = header()
    end = text.index("int " + NAME + "(")
    start = text.rindex("/*", 0, end)
    comment = re.sub(r"\s+", " ", text[start:end].replace("\n *", " "))
    for phrase in ("The pointer is kept", "The mask is read per run", "caller-owned rows are untouched", "lexls_lsi_batch_run is refused while the mask is set",
                   "d_mask == NULL clears the setting", "LEXLS_ERR_UNSUPPORTED"):
        assert phrase in comment, phrase
