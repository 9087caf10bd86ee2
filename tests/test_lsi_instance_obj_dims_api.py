"""lexls_lsi_batch_set_instance_obj_dims without a device: the symbol is in the header with the documented prototype, in the library and in the
ctypes mirror; a null handle is LEXLS_ERR_INVALID; LsiBatch.set_instance_obj_dims exists and turns away a host array and a wrong shape before the
library is asked; the header's comment states the contract — the pointer is kept, the counts are read per run, NULL clears the setting, the dims
are capacities and every layout the capacity layout, absent rows are written as 0, fault code 5, lexls_lsi_batch_run is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lexls_amd import capi, lexlsi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEXLS_ERR_INVALID = 1
NAME = "lexls_lsi_batch_set_instance_obj_dims"


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_prototype_in_the_header():
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, NAME + " is not declared in include/lexls_hip.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == ["lexls_lsi_batch_t b", "const uint32_t *d_dims"]


def test_symbol_in_the_library_and_the_ctypes_mirror():
    lib = capi.lib()
    assert NAME in capi.SYMBOLS
    assert getattr(lib, NAME).restype is C.c_int
    assert len(getattr(lib, NAME).argtypes) == 2


def test_null_handle_is_invalid():
    lib = capi.lib()
    assert getattr(lib, NAME)(None, None) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()


def test_python_method_signature():
    assert list(inspect.signature(lexlsi.LsiBatch.set_instance_obj_dims).parameters) == ["self", "dims"]
    # the entries the counts serve keep their signatures: no new argument anywhere
    for name in ("run_device", "enqueue_device", "finish"):
        assert not any("dims" in p for p in inspect.signature(getattr(lexlsi.LsiBatch, name)).parameters), name


def test_python_method_rejects_a_host_array_and_a_wrong_shape():
    """on an object that has no handle: every case is turned away in Python, before the library is asked"""
    torch = pytest.importorskip("torch")
    b = object.__new__(lexlsi.LsiBatch)
    b.batch, b.dims, b.device, b._h, b._instance_obj_dims = 4, np.array([4, 3, 4], np.uint32), 0, C.c_void_p(), None
    with pytest.raises(TypeError):
        b.set_instance_obj_dims(np.ones((4, 3), np.uint32))  # a numpy array
    with pytest.raises(TypeError):
        b.set_instance_obj_dims(torch.ones((4, 3), dtype=torch.int64))  # not uint32 / int32
    for shape in ((4, 4), (3, 3), (12,), (4, 3, 1)):
        with pytest.raises(ValueError, match="shape"):
            b.set_instance_obj_dims(torch.ones(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="device"):
        b.set_instance_obj_dims(torch.ones((4, 3), dtype=torch.int32))  # the right shape in host memory
    assert b._instance_obj_dims is None


def test_the_header_states_the_contract():
    """the comment in front of the declaration, with its line breaks and comment stars taken out"""
    text = header()
    end = text.index("int " + NAME + "(")
    start = text.rindex("/*", 0, end)
    comment = re.sub(r"\s+", " ", text[start:end].replace("\n *", " "))
    for phrase in ("The pointer is kept", "The counts are read per run", "d_dims == NULL clears the setting", "become capacities", "Every layout stays the capacity layout",
                   "the leading dimension of a block is still dims[k]", "are written as 0", "code 5", "instance * 8 + 5", "A count of 0 is an empty objective and is served",
                   "an instance mask skips are not read", "lexls_lsi_batch_run returns LEXLS_ERR_UNSUPPORTED", "With the setting off no kernel loads anything new"):
        assert phrase in comment, phrase
