"""The multi-cotangent adjoint in the C ABI: the five functions are declared in include/lexls_hip.h, exported by the library and listed in
capi.SYMBOLS; a null handle is refused before anything else; the header states the independence contract and the error rules.  No GPU."""
import ctypes as C
import os
import re

from conftest import ROOT

LSE = ("lexls_lse_solve_adjoint_multi", "lexls_lse_get_adjoint_multi", "lexls_lse_solve_adjoint_multi_device")
LSI = ("lexls_lsi_batch_solve_adjoint_multi", "lexls_lsi_batch_solve_adjoint_multi_device")
LEXLS_ERR_INVALID = 1


def header():
    return open(os.path.join(ROOT, "include", "lexls_hip.h")).read()


def test_the_five_symbols_are_declared_exported_and_listed():
    from lexls_amd import capi
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = capi.lib()
    for name in LSE + LSI:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in include/lexls_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
    d, cd, u = r"double\s*\*\s*", r"const\s+double\s*\*\s*", r"uint32_t\s+ncot\s*"
    assert re.search(r"lexls_lse_solve_adjoint_multi\s*\(\s*lexls_lse_t\s+h\s*,\s*" + cd + r"h_G\s*,\s*" + u + r"\)", code)
    assert re.search(r"lexls_lse_get_adjoint_multi\s*\(\s*lexls_lse_t\s+h\s*,\s*" + d + r"h_grad_rhs\s*,\s*" + d + r"h_grad_fixed\s*\)", code)
    assert re.search(r"lexls_lse_solve_adjoint_multi_device\s*\(\s*lexls_lse_t\s+h\s*,\s*" + cd + r"d_G\s*,\s*" + u + r",\s*" + d + r"d_grad_rhs\s*,\s*" + d + r"d_grad_fixed\s*\)", code)
    assert re.search(r"lexls_lsi_batch_solve_adjoint_multi\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*" + cd + r"h_G\s*,\s*" + u + r",\s*" + d + r"h_grad_lb\s*,\s*" + d + r"h_grad_ub\s*\)", code)
    assert re.search(r"lexls_lsi_batch_solve_adjoint_multi_device\s*\(\s*lexls_lsi_batch_t\s+b\s*,\s*" + cd + r"d_G\s*,\s*" + u + r",\s*" + d + r"d_grad_lb\s*,\s*" + d + r"d_grad_ub\s*\)", code)


def test_a_null_handle_is_invalid_and_outputs_are_left_alone():
    from lexls_amd import capi
    lib = capi.lib()
    G = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    out_a, out_b = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0), (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    void = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    assert lib.lexls_lse_solve_adjoint_multi(None, G, 2) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lse_get_adjoint_multi(None, out_a, out_b) == LEXLS_ERR_INVALID
    assert lib.lexls_lse_solve_adjoint_multi_device(None, void(G), 2, void(out_a), void(out_b)) == LEXLS_ERR_INVALID
    assert lib.lexls_lsi_batch_solve_adjoint_multi(None, G, 2, out_a, out_b) == LEXLS_ERR_INVALID
    assert b"null handle" in lib.lexls_last_error()
    assert lib.lexls_lsi_batch_solve_adjoint_multi_device(None, void(G), 2, void(out_a), void(out_b)) == LEXLS_ERR_INVALID
    assert list(out_a) == [7.0] * 4 and list(out_b) == [7.0] * 4


def doc_in_front_of(name):
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + name + r"\(", header(), flags=re.S)
    assert m, f"no comment in front of {name}"
    return " ".join(m.group(1).replace("*", " ").split())


def test_the_header_states_the_independence_contract_and_the_error_rules():
    doc = doc_in_front_of("lexls_lse_solve_adjoint_multi")
    for phrase in ("G is batch x ncot x nVar", "grad_rhs is batch x ncot x cap", "LOD row order", "grad_fixed is batch x ncot x nVar",
                   "zero from nfixed on", "(NULL: not wanted)", "lane = cotangent", "no host-synchronising call",
                   "Independence contract", "does not depend on ncot, on its position in G, or on the other cotangents", "bit for bit the same",
                   "from run to run and from the host and the device form", "NOT promised to be bit-equal to lexls_lse_solve_adjoint",
                   "the contract is the tolerance one", "before any device work", "with every output left alone",
                   "LEXLS_ERR_INVALID for a null handle, a null G or a null d_grad_rhs", "LEXLS_ERR_INVALID for ncot == 0",
                   "LEXLS_ERR_INVALID when there is no kept factor", "LEXLS_ERR_UNSUPPORTED when the factorization ran with regularization_type != 0",
                   "belong to the current factor", "solve_adjoint_multi<64,staged>", "solve_adjoint_multi<64,hbm>", "solve_adjoint<64> x K"):
        assert phrase in doc, f"the header comment does not state: {phrase}"
    doc = doc_in_front_of("lexls_lsi_batch_solve_adjoint_multi")
    for phrase in ("G is batch x ncot x nVar", "batch x ncot x sum(dims)", "nothing is factorized twice", "lsi_adjoint_scatter_multi_kernel",
                   "exact zeros unless PROBLEM_SOLVED", "keeps the bits of all its ncot rows", "LEXLS_ERR_INVALID for ncot == 0",
                   "before any device work"):
        assert phrase in doc, f"the header comment does not state: {phrase}"


def test_the_python_surface_exists_without_importing_torch_at_import_time():
    import subprocess
    import sys
    code = ("import sys; import lexls_amd.torch_adjoint as t, lexls_amd.lexlse as l, lexls_amd.lexlsi as i; "
            "assert 'torch' not in sys.modules, 'torch imported with the package'; "
            "assert all(hasattr(l.BatchedLexLSE, m) for m in ('solve_adjoint_multi', 'solve_adjoint_multi_device', 'jacobian_device')); "
            "assert all(hasattr(i.LsiBatch, m) for m in ('solve_adjoint_multi', 'solve_adjoint_multi_device', 'jacobian_bounds_device')); "
            "assert callable(t.jacobian_rhs) and callable(t.jacobian_bounds)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
