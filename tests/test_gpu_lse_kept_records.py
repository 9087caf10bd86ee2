"""The life cycle of what the kept-factor calls of the C ABI keep in a LexLSE handle (lexls_amd/csrc/lse_kept_capi.h): the host-result record
of each of the five families — lexls_lse_solve_adjoint, _adjoint_multi, _adjoint_matrix, _tangent, _rhs — and the grow-only work buffers.  One tiny
problem set: batch 2, nVar 3, levels [2, 1], one fixed variable in problem 0.  Nothing here is compared with a reference solution (the families'
own test files do that): a handle that has grown, shrunk and been re-factorized has to give the BYTES of a fresh one, and every refusal its code
and its text, written out here as the library has always worded them."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

from lexls_amd import capi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
B, N, CAPS, CAP = 2, 3, (2, 1), 3
KMAX = 65
_dp, _bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
_rng = np.random.default_rng(20260321)
LOD = _rng.standard_normal((B, N + 1, CAP))
FIXED = dict(nfixed=np.array([1, 0], np.uint32), idx=np.array([[1, 0, 0], [0, 0, 0]], np.uint32), val=np.array([[0.7, 0, 0], [0, 0, 0]], np.float64))
INPUT = {  # per family: the host call's input arrays for KMAX items (the families of one item: for one)
    "adjoint": (_rng.standard_normal((B, N)),),
    "adjoint_multi": (_rng.standard_normal((B, KMAX, N)),),
    "adjoint_matrix": (_rng.standard_normal((B, N)),),
    "tangent": (_rng.standard_normal((KMAX, B, N + 1, CAP)), _rng.standard_normal((KMAX, B, N))),
    "solve_rhs": (_rng.standard_normal((KMAX, B, CAP)), _rng.standard_normal((KMAX, B, N))),
}
FAMILIES = tuple(INPUT)
COUNTED = ("adjoint_multi", "tangent", "solve_rhs")
GETTER = {"adjoint": "lexls_lse_get_adjoint", "adjoint_multi": "lexls_lse_get_adjoint_multi", "adjoint_matrix": "lexls_lse_get_adjoint_matrix",
          "tangent": "lexls_lse_get_tangent", "solve_rhs": "lexls_lse_get_solve_rhs"}
HOST = {"adjoint": "lexls_lse_solve_adjoint", "adjoint_multi": "lexls_lse_solve_adjoint_multi", "adjoint_matrix": "lexls_lse_solve_adjoint_matrix",
        "tangent": "lexls_lse_solve_tangent", "solve_rhs": "lexls_lse_solve_rhs"}


def handle(hip, reg_type=0, variable=0.0, switches=True, factorized=True):
    s = hip.BatchedLexLSE(B, N, CAPS)
    s.set_kernel_policy(1)  # (lqr_generic: keeps its factor whatever the regularization)
    s.fixVariables(FIXED["nfixed"], FIXED["idx"], FIXED["val"])
    s.setProblem(LOD)
    if reg_type:
        s.setRegularization(reg_type, np.full(len(CAPS), 0.2), variable)
    s.set_adjoint_regularized(switches)
    s.set_adjoint_regularized_multi(switches)
    if factorized:
        s.factorize_solve(keep_factor=True)
    return s


def inputs(family, K):
    """the first K items of the family's input, C-contiguous"""
    a = INPUT[family]
    if family == "adjoint_multi":
        return (np.ascontiguousarray(a[0][:, :K]),)
    return tuple(np.ascontiguousarray(v[:K]) for v in a) if family in COUNTED else a


def results(family, K, fill=7.0):
    """the getter's (or the device form's) output arrays for K items, pre-filled"""
    flags = np.full(B, 7, np.uint8)
    return {"adjoint": (np.full((B, CAP), fill), np.full((B, N), fill)), "adjoint_multi": (np.full((B, K, CAP), fill), np.full((B, K, N), fill)),
            "adjoint_matrix": (np.full((B, N + 1, CAP), fill), flags), "tangent": (np.full((K, B, N), fill), flags), "solve_rhs": (np.full((K, B, N), fill),)}[family]


def _p(a):
    return None if a is None else a.ctypes.data_as(_bp if a.dtype == np.uint8 else _dp)


def host_call(s, family, K, arrays):
    """the host form on these input arrays (None: a null pointer); the families with a count get K"""
    fn = getattr(capi.lib(), HOST[family])
    return fn(s._h, *[_p(a) for a in arrays], K) if family in COUNTED else fn(s._h, *[_p(a) for a in arrays])


def get(s, family, K):
    out = results(family, K)
    return getattr(capi.lib(), GETTER[family])(s._h, *[_p(a) for a in out]), out


def device_call(s, family, K, arrays, null_output=False):
    """the device form on copies of these arrays (None: a null pointer) and sentinel-filled outputs; returns (rc, the outputs on the host)"""
    d_in = [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]
    d_out = [torch.from_numpy(a).cuda() for a in results(family, min(K, KMAX) if K else 1)]
    pin = [None if t is None else C.c_void_p(t.data_ptr()) for t in d_in]
    pout = [C.c_void_p(t.data_ptr()) for t in d_out]
    if null_output:
        pout[0] = None
    lib = capi.lib()
    if family == "adjoint":
        rc = lib.lexls_lse_solve_adjoint_device(s._h, pin[0], *pout)
    elif family == "adjoint_multi":
        rc = lib.lexls_lse_solve_adjoint_multi_device(s._h, pin[0], K, *pout)
    elif family == "adjoint_matrix":
        rc = lib.lexls_lse_solve_adjoint_matrix_device(s._h, pin[0], *pout)
    elif family == "tangent":
        rc = lib.lexls_lse_solve_tangent_device(s._h, pin[0], pin[1], K, *pout)
    else:
        rc = lib.lexls_lse_solve_rhs_device(s._h, pin[0], pin[1], K, *pout)
    err = lib.lexls_last_error().decode() if rc else ""
    s.synchronize()
    return rc, err, [t.cpu().numpy() for t in d_out]


def same_bytes(a, b):
    return all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def untouched(arrays):
    return all((a == 7).all() for a in arrays)


@pytest.fixture(scope="module")
def fresh(hip):
    """(family, K) -> the getter's arrays after ONE host call on a handle of its own"""
    cache = {}

    def of(family, K):
        if (family, K) not in cache:
            s = handle(hip)
            assert host_call(s, family, K, inputs(family, K)) == 0, capi.lib().lexls_last_error()
            rc, out = get(s, family, K)
            assert rc == 0 and not untouched(out[:1])
            s.close()
            cache[family, K] = out
        return cache[family, K]
    return of


@pytest.mark.parametrize("family", COUNTED)
def test_a_record_that_grew_and_shrank_gives_a_fresh_handle_s_bytes(hip, fresh, family):
    """K = 2, 1, 3, 2 on one handle: room made (2), kept (1), made anew (3: three frees, three allocations, the work buffer regrown), kept (2)"""
    s = handle(hip)
    for K in (2, 1, 3, 2):
        assert host_call(s, family, K, inputs(family, K)) == 0, capi.lib().lexls_last_error()
        rc, out = get(s, family, K)
        assert rc == 0 and same_bytes(out, fresh(family, K)), f"{family} K={K}"
    s.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_getter_answers_only_for_the_factor_its_call_ran_on(hip, fresh, family):
    lib, getter, call = capi.lib(), GETTER[family], HOST[family]
    s = handle(hip)
    rc, out = get(s, family, 2)
    assert rc == INVALID and lib.lexls_last_error().decode() == f"{getter}: call {call} first" and untouched(out)
    assert host_call(s, family, 2, inputs(family, 2)) == 0, lib.lexls_last_error()
    rc, out = get(s, family, 2)
    assert rc == 0 and same_bytes(out, fresh(family, 2))
    s.factorize()
    rc, out = get(s, family, 2)
    assert rc == INVALID and untouched(out)
    assert lib.lexls_last_error().decode() == f"{getter}: the problem or its factorization changed since {call} (call it again)"
    s.solve()  # (the matrix gradient and the tangents want the x of the factor)
    assert host_call(s, family, 2, inputs(family, 2)) == 0, lib.lexls_last_error()
    rc, out = get(s, family, 2)
    assert rc == 0 and same_bytes(out, fresh(family, 2))
    s.close()


# ---- the refusals: (code, text behind "<function>: "), None where the family has no such refusal and answers ----
NULL_INPUT = {"adjoint": "null g", "adjoint_multi": "null G", "adjoint_matrix": "null g", "tangent": "null dlod", "solve_rhs": "null rhs"}
NULL_OUTPUT = {"adjoint": "null d_grad_rhs", "adjoint_multi": "null d_grad_rhs", "adjoint_matrix": "null d_grad_lod", "tangent": "null d_dx", "solve_rhs": "null d_x"}
ZERO = {"adjoint_multi": "ncot == 0", "tangent": "ntan == 0", "solve_rhs": "nrhs == 0"}
TOO_MANY = {"adjoint_multi": None,  # (64 cotangents a tile, up to 65535 tiles: 65536 cotangents are served — not run here)
            "tangent": "ntan > 65535 (split the directions over several calls)", "solve_rhs": "nrhs > 65535 (split the right-hand sides over several calls)"}
NO_FACTOR = "needs a factorization whose factor was kept"
SERVES_NONE = ("the factorization ran with regularization_type != 0 (lexls_lse_solve_adjoint, the single-cotangent call, serves "
               "regularization types 1, 3, 4, 5, 8 and 9; this call serves none)")
NOT_AFFINE = "regularization_type 2 is not an affine map of the right-hand side (the CG types 2 and 6 iterate from x = 0, type 7 is experimental); served: 1, 3, 4, 5, 8, 9"
VARIABLE = "variable_regularization_factor != 0 under regularization_type 1 (the factor depends on the right-hand side: x is not an affine map of it)"
SINGLE_OFF = ("the factorization ran with regularization_type != 0 and the adjoint of damped solves is not switched on "
              "for this handle (lexls_lse_set_adjoint_regularized; it serves regularization types 1, 3, 4, 5, 8 and 9)")
MULTI_OFF = ("the factorization ran with regularization_type != 0 and the many-cotangent adjoint of damped solves is not "
             "switched on for this handle (lexls_lse_set_adjoint_regularized_multi; it serves regularization types 1, 3, 4, 5, 8 "
             "and 9, as lexls_lse_solve_adjoint, the single-cotangent call, does under lexls_lse_set_adjoint_regularized)")
DAMPED = {  # what (reg_type, variable factor, switches) -> the text per family
    (2, 0.0, True): {"adjoint": NOT_AFFINE, "adjoint_multi": NOT_AFFINE, "adjoint_matrix": SERVES_NONE, "tangent": SERVES_NONE, "solve_rhs": NOT_AFFINE},
    (1, 0.5, True): {"adjoint": VARIABLE, "adjoint_multi": VARIABLE, "adjoint_matrix": SERVES_NONE, "tangent": SERVES_NONE, "solve_rhs": VARIABLE},
    (1, 0.0, False): {"adjoint": SINGLE_OFF, "adjoint_multi": MULTI_OFF, "adjoint_matrix": SERVES_NONE, "tangent": SERVES_NONE, "solve_rhs": None},  # (no switch)
}


def refused(s, family, K, arrays, code, text, null_output=False, host=True):
    """both forms refuse with the code and '<their own name>: text', the device outputs and what the getter writes to stay as they were"""
    lib = capi.lib()
    if host and not null_output:  # (the host forms have no output argument)
        assert host_call(s, family, K, arrays) == code, (family, text)
        assert lib.lexls_last_error().decode() == f"{HOST[family]}: {text}"
        rc, out = get(s, family, 1)
        assert rc == INVALID and untouched(out), (family, text)
    rc, err, out = device_call(s, family, K, arrays, null_output)
    assert rc == code and err == f"{HOST[family]}_device: {text}" and untouched(out), (family, text, err)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_argument_refusals_of_both_forms(hip, family):
    s = handle(hip)
    a = inputs(family, 2)
    refused(s, family, 2, (None,) + a[1:], INVALID, NULL_INPUT[family])
    refused(s, family, 2, a, INVALID, NULL_OUTPUT[family], null_output=True)
    if family in COUNTED:
        refused(s, family, 0, a, INVALID, ZERO[family])
        if TOO_MANY[family]:
            refused(s, family, 65536, a, INVALID, TOO_MANY[family])  # (refused before anything is read: the arrays of 2 items do)
    # the order of the tests: the null argument before the count, the count before the factor
    if family in COUNTED:
        refused(s, family, 0, (None,) + a[1:], INVALID, NULL_INPUT[family])
    s.close()
    s = handle(hip, factorized=False)
    refused(s, family, 2, a, INVALID, NO_FACTOR)
    if family in COUNTED:
        refused(s, family, 0, a, INVALID, ZERO[family])
    s.close()
    lib = capi.lib()
    assert getattr(lib, HOST[family])(None, *([None] * len(a)), *([2] if family in COUNTED else [])) == INVALID and lib.lexls_last_error() == b"null handle"
    assert getattr(lib, GETTER[family])(None, *([None] * len(results(family, 1)))) == INVALID and lib.lexls_last_error() == b"null handle"


@pytest.mark.parametrize("damping", sorted(DAMPED), ids=lambda d: f"type{d[0]}-variable{d[1]}-switches{'on' if d[2] else 'off'}")
def test_the_regularization_refusals_of_both_forms(hip, damping):
    reg_type, variable, switches = damping
    s = handle(hip, reg_type, variable, switches)
    for family in FAMILIES:
        text, a = DAMPED[damping][family], inputs(family, 2)
        if text is not None:
            refused(s, family, 2, a, UNSUPPORTED, text)
        else:
            assert host_call(s, family, 2, a) == 0, capi.lib().lexls_last_error()
            rc, err, out = device_call(s, family, 2, a)
            assert rc == 0 and same_bytes(out, get(s, family, 2)[1])
    s.close()


def test_the_tile_keyed_work_buffer_regrows_and_gives_a_fresh_handle_s_bytes(hip, monkeypatch):
    """A type 1 damped factor with LEXLS_ADJOINT_REG_MULTI_FORM = hbm (at this shape the matrices fit in LDS: the switch moves the shape down the
    list): the matrices live in a work buffer of the handle with one set per tile of 64 cotangents.  ncot = 3 (one tile), 65 (two: the buffer is
    freed and made anew), 3 (kept): each the bytes of a handle that saw that call alone."""
    monkeypatch.setenv("LEXLS_ADJOINT_REG_MULTI_FORM", "hbm")
    family = "adjoint_multi"

    def run(s, K):
        assert host_call(s, family, K, inputs(family, K)) == 0, capi.lib().lexls_last_error()
        assert s.last_consumer_kernel() == "solve_adjoint_reg_multi<64,hbm>"
        rc, out = get(s, family, K)
        assert rc == 0
        return out
    s = handle(hip, 1)
    for K in (3, 65, 3):
        alone = handle(hip, 1)
        assert same_bytes(run(s, K), run(alone, K)), f"ncot = {K}"
        alone.close()
    s.close()
