"""The multi-cotangent adjoint of the LexLSE solve on the device (lexls_lse_solve_adjoint_multi*, solve_adjoint_multi_kernel: lane =
cotangent) against the references of tests/adjoint_multi_cases.py, within MC.TOL_MULTI (derived there from the references' own disagreement
on the CPU, never from the device's figures): every case x every cotangent set behind every producer of a kept factor that
tests/test_gpu_lse_adjoint.py uses; the form the fit rule takes is named (last_consumer_kernel); the independence contract is held bit for
bit; NaN sentinels around G and the outputs stay intact; the error rules leave the outputs alone.  Every case also runs with the form moved
down the launcher's list by LEXLS_ADJOINT_MULTI_FORM (read at every call): `hbm` bit-equal to the staged run, `single` bit-equal to K calls of
the single-cotangent entry; and four shapes sit on both sides of the fit rule's two switches (MC.FIT_NAMES)."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import adjoint_multi_cases as MC
from lexls_amd import capi
from test_gpu_lse_adjoint import handle

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 3
PAD = 96  # sentinel doubles in front of and behind every device array
PRODUCERS = MC.PRODUCERS


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def host_form(s, G):
    """lexls_lse_solve_adjoint_multi + lexls_lse_get_adjoint_multi through the C ABI (K = 1 included: the Python method would route it away)"""
    G = np.ascontiguousarray(G, np.float64)
    K = G.shape[1]
    capi.check(capi.lib().lexls_lse_solve_adjoint_multi(s._h, ptr(G), K))
    rhs, fixed = np.full((s.batch, K, s.cap), 7.0), np.full((s.batch, K, s.nVar), 7.0)
    capi.check(capi.lib().lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)))
    return rhs, fixed


def padded(shape, fill=None):
    """a device array of `shape` inside a buffer with PAD NaNs on either side -> (buffer, view)"""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[PAD:PAD + size].view(*shape)
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill, np.float64)))
    return buf, view


def pads_intact(buf):
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all())


def device_form(s, G, with_fixed=True):
    """lexls_lse_solve_adjoint_multi_device through the C ABI on sentinel-framed arrays; asserts that the frames are intact"""
    K = G.shape[1]
    bG, dG = padded(G.shape, G)
    bR, dR = padded((s.batch, K, s.cap))
    bF, dF = padded((s.batch, K, s.nVar))
    capi.check(capi.lib().lexls_lse_solve_adjoint_multi_device(s._h, C.c_void_p(dG.data_ptr()), K, C.c_void_p(dR.data_ptr()),
                                                                C.c_void_p(dF.data_ptr()) if with_fixed else None))
    s.synchronize()
    assert pads_intact(bG) and pads_intact(bR) and pads_intact(bF), "a sentinel around G or the outputs was overwritten"
    np.testing.assert_array_equal(dG.cpu().numpy(), G)  # G itself is read only
    if not with_fixed:
        assert bool(torch.isnan(dF).all()), "grad_fixed was not wanted and was written"
    return dR.cpu().numpy(), dF.cpu().numpy() if with_fixed else None


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_set_within_tol_of_the_reference_behind_every_producer(hip, oracle, name):
    case = MC.build(name)
    m = case["dims"].sum(axis=1)
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(len(m), np.uint32)
    first = {}
    for policy, producer in PRODUCERS[name].items():
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
        for st in MC.SETS:
            ctx = f"{name} on {producer}, K = {st}: "
            G = MC.select(st, case["R"])
            rhs, fixed = host_form(s, G)
            assert s.last_consumer_kernel() == MC.FORMS[name], ctx + s.last_consumer_kernel()
            e_rhs, e_fixed = MC.gap(rhs, MC.select_ref(st, case, 0)), MC.gap(fixed, MC.select_ref(st, case, 1))
            ident = MC.identities(case, G, rhs)
            print(f"{ctx}grad_rhs {e_rhs:.2e} grad_fixed {e_fixed:.2e} identities {ident:.2e} (TOL_MULTI {MC.TOL_MULTI:.1e})")
            assert e_rhs <= MC.TOL_MULTI and e_fixed <= MC.TOL_MULTI, ctx + f"{e_rhs:.3e} {e_fixed:.3e}"
            assert ident <= MC.TOL_MULTI, ctx + f"identities {ident:.3e}"
            for b in range(len(m)):  # rows behind a ragged problem's own, entries from nfixed on: exactly 0
                assert not rhs[b, :, m[b]:].any() and not fixed[b, :, nf[b]:].any(), ctx + f"problem {b}"
            d_rhs, d_fixed = device_form(s, G)  # the device form, sentinels around everything: the same bits
            assert s.last_consumer_kernel() == MC.FORMS[name]
            np.testing.assert_array_equal(d_rhs, rhs, err_msg=ctx + "device form")
            np.testing.assert_array_equal(d_fixed, fixed, err_msg=ctx + "device form")
            if st in first:  # whoever wrote the (bit-identical) factor
                np.testing.assert_array_equal(rhs, first[st][0], err_msg=ctx + "against the first producer")
                np.testing.assert_array_equal(fixed, first[st][1], err_msg=ctx + "against the first producer")
            first.setdefault(st, (rhs, fixed))
        np.testing.assert_array_equal(device_form(s, MC.select("3", case["R"]), with_fixed=False)[0], first["3"][0])
        for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
            np.testing.assert_array_equal(a, b_, err_msg=f"{name} on {producer}: {what} changed")
        s.close()


@pytest.mark.parametrize("name", MC.NAMES)
def test_within_tol_of_k_calls_of_the_single_cotangent_entry(hip, oracle, name):
    """tolerance, not bits: the summation order differs"""
    case = MC.build(name)
    policy = next(iter(PRODUCERS[name]))
    s = handle(hip, case, policy)
    s.factorize_solve(keep_factor=True)
    R = case["R"]
    rhs, fixed = host_form(s, R)
    d_rhs = torch.empty((s.batch, s.cap), dtype=torch.float64, device="cuda")
    d_fixed = torch.empty((s.batch, s.nVar), dtype=torch.float64, device="cuda")
    worst = 0.0
    for c in range(R.shape[1]):
        s.solve_adjoint_device(torch.from_numpy(np.ascontiguousarray(R[:, c])).cuda(), d_rhs, d_fixed)
        s.synchronize()
        assert s.last_consumer_kernel() == "solve_adjoint<64>"
        worst = max(worst, MC.gap(rhs[:, c][:, None], d_rhs.cpu().numpy()[:, None]), MC.gap(fixed[:, c][:, None], d_fixed.cpu().numpy()[:, None]))
    print(f"{name}: multi against {R.shape[1]} single-cotangent calls {worst:.2e} (TOL_MULTI {MC.TOL_MULTI:.1e})")
    assert worst <= MC.TOL_MULTI
    s.close()


@pytest.mark.parametrize("name", MC.NAMES)
def test_a_cotangent_is_independent_of_its_company_bit_for_bit(hip, oracle, name):
    case = MC.build(name)
    s = handle(hip, case, next(iter(PRODUCERS[name])))
    s.factorize_solve(keep_factor=True)
    R = case["R"]
    base = host_form(s, R)

    def same(got, cols, what):
        for w in (0, 1):
            np.testing.assert_array_equal(got[w], base[w][:, cols], err_msg=f"{name}: {what} ({('grad_rhs', 'grad_fixed')[w]})")

    same(host_form(s, R), slice(None), "a second run")
    same(device_form(s, R), slice(None), "the device form")
    for c in (0, 5, 63, 64):                      # alone: K = 1, ncot changes, lane 0 of tile 0
        same(host_form(s, R[:, c:c + 1]), [c], f"cotangent {c} alone")
    c = 7                                         # at positions 0, 63 and 64 of a K = 65 set: first lane, last lane, a second tile
    for position in (0, 63, 64):
        order = np.arange(65)
        order[[position, c]] = order[[c, position]]
        got = host_form(s, R[:, order])
        same(got, order, f"cotangent {c} at position {position}")
        np.testing.assert_array_equal(got[0][:, position], base[0][:, c])
    order = np.random.default_rng(20290401).permutation(65)  # a permuted set
    same(host_form(s, R[:, order]), order, "a permuted set")
    same(host_form(s, R[:, :3]), [0, 1, 2], "the first three")
    s.close()


FORM_SWITCH = "LEXLS_ADJOINT_MULTI_FORM"


def assert_within_tol(case, st, G, rhs, fixed, ctx):
    """within TOL_MULTI of the reference, the identities of the large cases, exact zeros in the absent rows and slots"""
    m = case["dims"].sum(axis=1)
    nf = case["fixed"]["nfixed"] if case["fixed"] else np.zeros(len(m), np.uint32)
    e_rhs, e_fixed = MC.gap(rhs, MC.select_ref(st, case, 0)), MC.gap(fixed, MC.select_ref(st, case, 1))
    ident = MC.identities(case, G, rhs)
    print(f"{ctx}grad_rhs {e_rhs:.2e} grad_fixed {e_fixed:.2e} identities {ident:.2e} (TOL_MULTI {MC.TOL_MULTI:.1e})")
    assert e_rhs <= MC.TOL_MULTI and e_fixed <= MC.TOL_MULTI, ctx + f"{e_rhs:.3e} {e_fixed:.3e}"
    assert ident <= MC.TOL_MULTI, ctx + f"identities {ident:.3e}"
    for b in range(len(m)):
        assert not rhs[b, :, m[b]:].any() and not fixed[b, :, nf[b]:].any(), ctx + f"problem {b}"


@pytest.mark.parametrize("name", MC.NAMES)
def test_forced_hbm_is_the_staged_run_bit_for_bit(hip, oracle, monkeypatch, name):
    """the two instantiations run the same dfma chains on the same values; only where a factor entry is read from differs — so bits, not a tolerance"""
    case = MC.build(name)
    natural = MC.FORMS[name]
    forced = MC.HBM if natural == MC.STAGED else natural  # (the switch only moves a shape down the list)
    s = handle(hip, case, next(iter(PRODUCERS[name])))
    s.factorize_solve(keep_factor=True)
    before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
    sets = {st: MC.select(st, case["R"]) for st in ("3", "65", "identity")}
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    base = {}
    for st, G in sets.items():
        base[st] = host_form(s, G)
        assert s.last_consumer_kernel() == natural
    monkeypatch.setenv(FORM_SWITCH, "hbm")
    for st, G in sets.items():
        ctx = f"{name}, hbm forced, K = {st}: "
        rhs, fixed = host_form(s, G)
        assert s.last_consumer_kernel() == forced, ctx + s.last_consumer_kernel()
        np.testing.assert_array_equal(rhs, base[st][0], err_msg=ctx + "grad_rhs against the natural form")
        np.testing.assert_array_equal(fixed, base[st][1], err_msg=ctx + "grad_fixed against the natural form")
        assert_within_tol(case, st, G, rhs, fixed, ctx)
        d_rhs, d_fixed = device_form(s, G)  # NaN frames around G and both outputs
        assert s.last_consumer_kernel() == forced
        np.testing.assert_array_equal(d_rhs, rhs, err_msg=ctx + "device form")
        np.testing.assert_array_equal(d_fixed, fixed, err_msg=ctx + "device form")
    np.testing.assert_array_equal(device_form(s, sets["3"], with_fixed=False)[0], base["3"][0])
    if case["fixed"]:
        assert all(base["65"][1][b].any() for b in np.flatnonzero(case["fixed"]["nfixed"])), "grad_fixed is 0: the fixed columns were not read"
    monkeypatch.delenv(FORM_SWITCH)
    np.testing.assert_array_equal(host_form(s, sets["65"])[0], base["65"][0])
    assert s.last_consumer_kernel() == natural
    for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
        np.testing.assert_array_equal(a, b_, err_msg=f"{name}: {what} changed")
    s.close()


@pytest.mark.parametrize("name", MC.NAMES)
def test_forced_single_is_k_calls_of_the_single_cotangent_entry_bit_for_bit(hip, oracle, monkeypatch, name):
    """the per-cotangent form runs solve_adjoint<64> itself: only its three strided copies can differ from a call on that cotangent alone"""
    case = MC.build(name)
    s = handle(hip, case, next(iter(PRODUCERS[name])))
    s.factorize_solve(keep_factor=True)
    before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
    R = np.ascontiguousarray(case["R"])
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    natural = host_form(s, R[:, :3])  # the natural form first: where it is not per-cotangent the handle has no work buffer yet
    assert s.last_consumer_kernel() == MC.FORMS[name]
    monkeypatch.setenv(FORM_SWITCH, "single")
    ctx = f"{name}, single forced, K = 65: "
    rhs, fixed = host_form(s, R)
    assert s.last_consumer_kernel() == MC.SINGLE, ctx + s.last_consumer_kernel()
    assert_within_tol(case, "65", R, rhs, fixed, ctx)
    assert_within_tol(case, "3", R[:, :3], natural[0], natural[1], f"{name}, natural form, K = 3: ")
    d_rhs, d_fixed = device_form(s, R)  # NaN frames around G and both outputs
    assert s.last_consumer_kernel() == MC.SINGLE
    np.testing.assert_array_equal(d_rhs, rhs, err_msg=ctx + "device form")
    np.testing.assert_array_equal(d_fixed, fixed, err_msg=ctx + "device form")
    np.testing.assert_array_equal(device_form(s, R, with_fixed=False)[0], rhs, err_msg=ctx + "device form without grad_fixed")  # (grad_fixed stays NaN)
    one_rhs = torch.empty((s.batch, s.cap), dtype=torch.float64, device="cuda")
    one_fixed = torch.empty((s.batch, s.nVar), dtype=torch.float64, device="cuda")
    for c in range(R.shape[1]):
        s.solve_adjoint_device(torch.from_numpy(np.ascontiguousarray(R[:, c])).cuda(), one_rhs, one_fixed)
        s.synchronize()
        assert s.last_consumer_kernel() == "solve_adjoint<64>"
        np.testing.assert_array_equal(rhs[:, c], one_rhs.cpu().numpy(), err_msg=ctx + f"grad_rhs of cotangent {c}")
        np.testing.assert_array_equal(fixed[:, c], one_fixed.cpu().numpy(), err_msg=ctx + f"grad_fixed of cotangent {c}")
    if case["fixed"]:
        for b in np.flatnonzero(case["fixed"]["nfixed"]):
            assert fixed[b].any(axis=1).all(), ctx + f"grad_fixed of problem {b} is 0 for some cotangent"
    ident = MC.select("identity", R)  # another K behind it: the pitches follow ncot
    i_rhs, i_fixed = host_form(s, ident)
    assert s.last_consumer_kernel() == MC.SINGLE
    assert_within_tol(case, "identity", ident, i_rhs, i_fixed, f"{name}, single forced, K = identity: ")
    for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
        np.testing.assert_array_equal(a, b_, err_msg=f"{name}: {what} changed")
    s.close()


@pytest.mark.parametrize("name", MC.FIT_NAMES)
def test_both_sides_of_the_fit_rule(hip, oracle, monkeypatch, name):
    """n = 40 at the last staged, first hbm, last hbm and first per-cotangent capacity: the kernel carves gh | cb | perm | pos | L | hh out of
    exactly adjoint_multi_lds_bytes, so an off-by-one in the rule or in the carving is an LDS overrun at these shapes"""
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    case = MC.build(name)
    for policy, producer in PRODUCERS[name].items():
        s = handle(hip, case, policy)
        s.factorize_solve(keep_factor=True)
        assert s.last_kernel() == producer
        assert float(np.abs(s.get_x() - case["ref"]["x"]).max()) <= 1e-10
        before = (s.get_x(), s.get_lexqr(), s.get_hh_scalars())
        for st in ("3", "65"):
            ctx = f"{name} (cap {s.cap}) on {producer}, K = {st}: "
            G = MC.select(st, case["R"])
            rhs, fixed = host_form(s, G)
            assert s.last_consumer_kernel() == MC.FORMS[name], ctx + s.last_consumer_kernel()
            assert_within_tol(case, st, G, rhs, fixed, ctx)
            d_rhs, d_fixed = device_form(s, G)
            np.testing.assert_array_equal(d_rhs, rhs, err_msg=ctx + "device form")
            np.testing.assert_array_equal(d_fixed, fixed, err_msg=ctx + "device form")
        for a, b_, what in zip((s.get_x(), s.get_lexqr(), s.get_hh_scalars()), before, ("x", "factor", "hh")):
            np.testing.assert_array_equal(a, b_, err_msg=f"{name} on {producer}: {what} changed")
        s.close()


@pytest.mark.parametrize("name", [n for n in MC.NAMES if n not in ("wide", "large", "beyond")])  # the cases with unit solves
def test_jacobian_device_is_m_and_n_of_the_unit_solves(hip, oracle, name):
    from lexls_amd.torch_adjoint import jacobian_rhs
    case = MC.build(name)
    s = handle(hip, case, next(iter(PRODUCERS[name])))
    s.factorize_solve(keep_factor=True)
    dx_db, dx_dfixed = s.jacobian_device()
    s.synchronize()
    assert tuple(dx_db.shape) == (s.batch, s.nVar, s.cap) and tuple(dx_dfixed.shape) == (s.batch, s.nVar, s.nVar)
    e_m, e_n = MC.gap(dx_db.cpu().numpy(), case["M"]), MC.gap(dx_dfixed.cpu().numpy(), case["N"])
    print(f"{name}: dx/db against M {e_m:.2e}, dx/dx_fixed against N {e_n:.2e} (TOL_MULTI {MC.TOL_MULTI:.1e})")
    assert e_m <= MC.TOL_MULTI and e_n <= MC.TOL_MULTI
    again = jacobian_rhs(s)
    s.synchronize()
    assert torch.equal(again[0], dx_db) and torch.equal(again[1], dx_dfixed)
    host = s.solve_adjoint_multi(MC.select("identity", case["R"]))  # the Python host form
    np.testing.assert_array_equal(host[0], dx_db.cpu().numpy())
    np.testing.assert_array_equal(host[1], dx_dfixed.cpu().numpy())
    one = s.solve_adjoint_multi(case["R"][:, :1])  # one cotangent: the single-cotangent entry
    assert s.last_consumer_kernel() == "solve_adjoint<64>" and one[0].shape == (s.batch, 1, s.cap)
    s.close()


def test_error_rules_leave_the_outputs_alone(hip, oracle):
    case = MC.build("ik")
    lib = capi.lib()
    G = np.ascontiguousarray(case["R"][:, :3])
    s = handle(hip, case)

    def fresh():
        return np.full((s.batch, 3, s.cap), 7.0), np.full((s.batch, 3, s.nVar), 7.0)

    def device_rc(G_, ncot, null_rhs=False):
        """(return code of the device form on sentinel-filled outputs, whether they still hold the sentinels)"""
        dG = None if G_ is None else torch.from_numpy(np.array(G_, np.float64)).cuda()
        dR = torch.full((s.batch, 3, s.cap), 7.0, dtype=torch.float64, device="cuda")
        dF = torch.full((s.batch, 3, s.nVar), 7.0, dtype=torch.float64, device="cuda")
        rc = lib.lexls_lse_solve_adjoint_multi_device(s._h, None if dG is None else C.c_void_p(dG.data_ptr()), ncot,
                                                      None if null_rhs else C.c_void_p(dR.data_ptr()), C.c_void_p(dF.data_ptr()))
        s.synchronize()
        return rc, bool((dR == 7.0).all() and (dF == 7.0).all())

    def refused(code):
        rhs, fixed = fresh()
        assert lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), 3) == code
        assert device_rc(G, 3) == (code, True)
        assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)) == INVALID  # (never UNSUPPORTED: there is nothing to return)
        assert (rhs == 7.0).all() and (fixed == 7.0).all()

    refused(INVALID)                                   # no factorization yet
    assert lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), 3) == INVALID and b"kept" in lib.lexls_last_error()
    s.factorize_solve(keep_factor=False)               # an x-only solve: no kept factor
    refused(INVALID)
    s.factorize_solve(keep_factor=True)
    assert lib.lexls_lse_solve_adjoint_multi(s._h, None, 3) == INVALID and device_rc(None, 3) == (INVALID, True)   # null G
    assert lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), 0) == INVALID and device_rc(G, 0) == (INVALID, True)    # ncot == 0
    assert b"ncot" in lib.lexls_last_error()
    assert device_rc(G, 3, null_rhs=True) == (INVALID, True)                                                       # null d_grad_rhs
    rhs, fixed = fresh()
    assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)) == INVALID                                  # nothing computed yet
    assert (rhs == 7.0).all() and (fixed == 7.0).all()

    want = host_form(s, G)
    assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), None) == 0 and lib.lexls_lse_get_adjoint_multi(s._h, None, ptr(fixed)) == 0  # either may be NULL
    np.testing.assert_array_equal(rhs, want[0])
    np.testing.assert_array_equal(fixed, want[1])
    rhs, fixed = fresh()
    s.factorize_solve(keep_factor=True)                # a later factorization: the results no longer belong to the current factor
    assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)) == INVALID
    assert (rhs == 7.0).all() and (fixed == 7.0).all()
    np.testing.assert_array_equal(host_form(s, G)[0], want[0])
    s.setParameters(1e-9)                              # a tolerance change invalidates the factor
    refused(INVALID)
    s.setParameters(1e-12)
    s.setProblem(case["lod"])
    refused(INVALID)

    s.setRegularization(1, [1e-3] * len(case["caps"]))  # a regularized factorization: the damping rewrites the right-hand side
    s.factorize_solve(keep_factor=True)
    rhs, fixed = fresh()
    assert lib.lexls_lse_solve_adjoint_multi(s._h, ptr(G), 3) == UNSUPPORTED
    assert b"regularization_type" in lib.lexls_last_error()
    assert device_rc(G, 3) == (UNSUPPORTED, True)
    assert lib.lexls_lse_get_adjoint_multi(s._h, ptr(rhs), ptr(fixed)) == INVALID
    assert (rhs == 7.0).all() and (fixed == 7.0).all()
    s.close()
