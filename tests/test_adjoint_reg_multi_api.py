"""The switches of the many-cotangent adjoint of regularized solves in the C ABI: declared in include/lexls_hip.h, exported by the library, listed in
capi.SYMBOLS, reachable from Python, and refusing a null handle.  No GPU."""
import os
import re

from conftest import ROOT

NAMES = {"lexls_lse_set_adjoint_regularized_multi": "lexls_lse_t h", "lexls_lsi_batch_set_adjoint_regularized_multi": "lexls_lsi_batch_t b"}
LEXLS_ERR_INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_both_symbols_are_declared_exported_and_listed():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name, handle in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + handle.replace(" ", r"\s+") + r"\s*,\s*int\s+on\s*\)", code), f"{name} is not declared in include/lexls_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"


def test_a_null_handle_is_invalid():
    from lexls_amd import capi
    lib = capi.lib()
    assert lib.lexls_lse_set_adjoint_regularized_multi(None, 1) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_set_adjoint_regularized_multi(None, 1) == LEXLS_ERR_INVALID
    assert b"lexls_lsi_batch_set_adjoint_regularized_multi" in lib.lexls_last_error()


def test_the_header_states_the_contract_of_the_switch():
    text = header()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int lexls_lse_set_adjoint_regularized_multi\(", text, flags=re.S)
    assert m, "no comment in front of lexls_lse_set_adjoint_regularized_multi"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("type 1, 3, 4, 5, 8 or 9", "variable_regularization_factor == 0", "Independent of lexls_lse_set_adjoint_regularized", "Takes effect at the next call",
                   "LEXLS_ERR_INVALID for a null handle", "before any device work", "AT THE TIME OF THE ADJOINT CALL", "EVERY TILE REPEATS",
                   "solve_adjoint_reg_multi<64,lds>", "solve_adjoint_reg_multi<64,hbm>", "solve_adjoint_reg<64,lds> x K", "solve_adjoint_reg<64,hbm> x K",
                   "NOT promised bit-equal to lexls_lse_solve_adjoint"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_methods_exist():
    from lexls_amd import lexlse, lexlsi
    assert callable(lexlse.BatchedLexLSE.set_adjoint_regularized_multi) and callable(lexlsi.LsiBatch.set_adjoint_regularized_multi)
