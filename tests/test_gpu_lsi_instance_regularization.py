"""Regularization factors of its own for every instance of a LexLSI batch (lexls_lsi_batch_set_instance_regularization,
LsiBatch.set_instance_regularization), on every run path.  A batch of N instances with N factor sets is N solves of the reference, so the
yardstick is the oracle-backed single-problem driver (oracle.lsi_run) run per instance with that instance's own row, and the tolerance is
zero: counters, x, the final working set and v compare with assert_array_equal, as for every LexLSI path.

Shapes (those of tests/test_gpu_lsi_regularized_resident.py): `small` = n 20, dims [6, 5, 5, 6], 12 instances, simple bounds in front (LexLSE
level k = objective k + 1); `general` = the same general objectives without the bounds objective (level k = objective k); `ik` = n 40,
5 x 12, 64 instances (the 41 x 12 regularized instantiation).  Instance b's factors are the shape's shared vector times 2^((b mod 7) - 3); the
entry of a simple-bounds objective 0 is 1e30, which every path must ignore.  Before any device result is looked at, every batch is held to
the precondition that the rows matter: in at least half its instances the oracle's x under the instance's row differs in at least one bit
from the oracle's x under the shared vector."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime — the device-factor cases hand torch tensors to the library)

from lexls_amd import capi, lexlsi, problems as P

pytestmark = pytest.mark.gpu

LEXLS_ERR_INVALID, LEXLS_ERR_UNSUPPORTED = 1, 3
SENTINEL = 1e30
SHAPES = {
    "ik": dict(n=40, dims=[12] * 5, factors=[0, 0.02, 0.05, 0.03, 0.04], count=64, seed=20261000),
    "small": dict(n=20, dims=[6, 5, 5, 6], factors=[0, 0.3, 0.2, 0.4], count=12, seed=700),
}
_cache = {}


def make(shape, count=None):
    """-> n, the shared factors, the problems (`general`: small without its bounds objective; `ik_perturbed`: the warm-start neighbours of ik)"""
    key = ("probs", shape, count)
    if key not in _cache:
        s = SHAPES["small" if shape == "general" else shape.replace("_perturbed", "")]
        probs = [P.lsi_problem(s["seed"] + i, s["n"], s["dims"], perturb=0.9 if shape.endswith("_perturbed") else 0.0) for i in range(count or s["count"])]
        if shape == "general":
            _cache[key] = (s["n"], s["factors"][1:], [p[1:] for p in probs])
        else:
            _cache[key] = (s["n"], s["factors"], probs)
    return _cache[key]


def instance_factors(shape, count, shift=0, distinct=False):
    """(count, nObj): the shared vector times 2^(((b + shift) mod 7) - 3) — times 1 + b / 1024 on top when every instance is to have a value
    of its own; a simple-bounds objective 0 gets the sentinel"""
    _, shared, probs = make(shape, count)
    b = np.arange(count)
    mult = 2.0 ** (((b + shift) % 7) - 3) * ((1.0 + b / 1024.0) if distinct else 1.0)
    rows = mult[:, None] * np.asarray(shared, np.float64)[None, :]
    if "var" in probs[0][0]:
        rows[:, 0] = SENTINEL
    return np.ascontiguousarray(rows)


def oracle_refs(oracle, shape, rows, count=None, only=None, guesses=None, x0=None, **params):
    """the oracle-backed driver per instance, instance b under rows[b] (rows: (count, nObj), or one shared vector); cached"""
    rows = np.asarray(rows, np.float64)
    key = ("oracle", shape, count, rows.tobytes(), None if only is None else tuple(only), None if guesses is None else guesses.tobytes(),
           None if x0 is None else np.asarray(x0).tobytes(), tuple(sorted(params.items())))
    if key not in _cache:
        n, _, probs = make(shape, count)
        refs = {}
        for i in (range(len(probs)) if only is None else only):
            p = probs[i]
            refs[i] = oracle.lsi_run(n, p, active_guess=None if guesses is None else np.split(guesses[i], np.cumsum([len(o["lb"]) for o in p])[:-1]),
                                     x0=None if x0 is None else x0[i], regularization_factors=rows[i] if rows.ndim == 2 else rows, **params)
        _cache[key] = refs
    return _cache[key]


def assert_rows_matter(oracle, shape, rows, count=None, only=None, **params):
    """the precondition, from the oracle alone: a build that ignored the rows could not pass"""
    _, shared, _ = make(shape, count)
    own, common = oracle_refs(oracle, shape, rows, count, only, **params), oracle_refs(oracle, shape, shared, count, only, **params)
    differ = sum(not np.array_equal(own[i]["x"].view(np.uint64), common[i]["x"].view(np.uint64)) for i in own)
    assert 2 * differ >= len(own), f"{shape}: only {differ} of {len(own)} instances notice their own factors"


def assert_equals_oracle(r, refs):
    for b, o in refs.items():
        assert dict(zip(lexlsi.INFO_KEYS, np.asarray(info_array(r)[b]).tolist())) == o["info"], b
        np.testing.assert_array_equal(r["x"][b], o["x"], err_msg=str(b))
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]), err_msg=str(b))
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]), err_msg=str(b))


def info_array(r):
    return r["info"].array if hasattr(r["info"], "array") else r["info"]


def assert_same_run(a, b):
    np.testing.assert_array_equal(info_array(a), info_array(b))
    np.testing.assert_array_equal(a["active"], b["active"])
    for k in ("x", "v"):
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64))


def new_batch(shape, count=None):
    n, _, probs = make(shape, count)
    key = ("packed", shape, count)
    if key not in _cache:
        _cache[key] = lexlsi.pack_batch(n, probs)
    pk = _cache[key]
    return lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs)), pk


def fused_run(shape, reg_type):
    """case 1's run: host factors on the persistent launch (cached: the later cases compare with it)"""
    key = ("fused", shape, reg_type)
    if key not in _cache:
        n, _, probs = make(shape)
        b, pk = new_batch(shape)
        b.set_instance_regularization(instance_factors(shape, len(probs)))
        r = b.run(pk, regularization_type=reg_type)
        _cache[key] = (r, b.last_kernel())
        b.close()
    return _cache[key]


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def device_inputs(pk):
    return to_device(pk.data), None if pk.var_index is None else to_device(pk.var_index.view(np.int32))


def to_host(r):
    return {k: r[k].cpu().numpy() for k in ("x", "info", "active", "v")}


@pytest.mark.parametrize("shape,reg_type", [("small", 1), ("small", 2), ("small", 8), ("general", 1), ("ik", 1)])
def test_persistent_launch(hip, oracle, shape, reg_type):
    n, _, probs = make(shape)
    rows = instance_factors(shape, len(probs))
    assert_rows_matter(oracle, shape, rows, regularization_type=reg_type)
    r, name = fused_run(shape, reg_type)
    assert name.startswith("lsi_fused<") and name.endswith("regularized>>"), name
    assert_equals_oracle(r, oracle_refs(oracle, shape, rows, regularization_type=reg_type))


@pytest.mark.parametrize("shape", ["small", "general"])
def test_stages_and_host_path(hip, monkeypatch, shape):
    n, _, probs = make(shape)
    rows = instance_factors(shape, len(probs))
    fused, _ = fused_run(shape, 1)
    b, pk = new_batch(shape)
    b.set_instance_regularization(rows)
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    staged = b.run(pk, regularization_type=1)
    name = b.last_kernel()
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")
    b.close()
    assert name.startswith("lqr_wave<") and name.endswith("regularized>"), name
    assert_same_run(staged, fused)
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    h, _ = new_batch(shape)
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    h.set_instance_regularization(rows)
    host = h.run(pk, regularization_type=1)
    name = h.last_kernel()
    h.close()
    assert name == "host"
    assert_same_run(host, fused)


@pytest.mark.parametrize("shape", ["small", "general"])
def test_device_factors_are_read_per_run(hip, oracle, shape):
    n, _, probs = make(shape)
    rows, second = instance_factors(shape, len(probs)), instance_factors(shape, len(probs), shift=2)
    assert_rows_matter(oracle, shape, second, regularization_type=1)
    assert not np.array_equal(rows, second)
    fused, fused_name = fused_run(shape, 1)
    b, pk = new_batch(shape)
    d_data, d_var = device_inputs(pk)
    d_rows = to_device(rows)
    b.set_instance_regularization(d_rows)
    first = to_host(b.run_device(d_data, d_var, regularization_type=1))
    assert b.last_kernel() == fused_name
    d_rows.copy_(to_device(second))  # in place: the setter is not called again
    again = to_host(b.run_device(d_data, d_var, regularization_type=1))
    assert b.last_kernel() == fused_name
    assert np.array_equal(d_rows.cpu().numpy(), second)  # the caller's array is never written
    b.close()
    assert_same_run(first, fused)
    assert_equals_oracle(again, oracle_refs(oracle, shape, second, regularization_type=1))


@pytest.mark.parametrize("shape", ["small", "ik"])
def test_device_factors_through_run(hip, shape):
    n, _, probs = make(shape)
    fused, fused_name = fused_run(shape, 1)
    b, pk = new_batch(shape)
    b.set_instance_regularization(to_device(instance_factors(shape, len(probs))))
    r = b.run(pk, regularization_type=1)
    name = b.last_kernel()
    b.close()
    assert name == fused_name
    assert_same_run(r, fused)


def test_two_groups(hip, oracle, monkeypatch):
    """600 instances in two groups of 300, every instance with a value of its own and its own oracle run: a wrong first-instance offset of a
    group shows in every instance of that group.  (A resident batch uses one group whatever its size; LEXLS_LSI_GROUPS, read when the batch
    object is made, asks for two.)  Host and device factors."""
    count = 600
    n, _, probs = make("small", count)
    rows = instance_factors("small", count, distinct=True)
    assert len({row.tobytes() for row in rows}) == count
    only = None
    assert_rows_matter(oracle, "small", rows, count, only, regularization_type=1)
    monkeypatch.setenv("LEXLS_LSI_GROUPS", "2")
    b, pk = new_batch("small", count)
    monkeypatch.delenv("LEXLS_LSI_GROUPS")
    b.set_instance_regularization(rows)
    r = b.run(pk, regularization_type=1)
    assert b.stats()["groups"] == 2
    assert b.last_kernel().startswith("lsi_fused<") and b.last_kernel().endswith("regularized>>")
    b.set_instance_regularization(to_device(rows))
    d = b.run(pk, regularization_type=1)
    assert b.stats()["groups"] == 2
    b.close()
    assert_equals_oracle(r, oracle_refs(oracle, "small", rows, count, only, regularization_type=1))
    assert_same_run(d, r)


@pytest.mark.parametrize("shape", ["small", "general"])
def test_equal_rows_are_the_shared_run(hip, shape):
    n, shared, probs = make(shape)
    b, pk = new_batch(shape)
    b.set_instance_regularization(np.tile(np.asarray(shared, np.float64), (len(probs), 1)))
    r = b.run(pk, regularization_type=1)
    name = b.last_kernel()
    b.close()
    f, _ = new_batch(shape)
    ref = f.run(pk, regularization_factors=shared, regularization_type=1)
    ref_name = f.last_kernel()
    f.close()
    assert name == ref_name
    assert_same_run(r, ref)


def test_clearing(hip):
    n, shared, probs = make("small")
    f, pk = new_batch("small")
    fresh_shared = f.run(pk, regularization_factors=shared, regularization_type=1)
    f.close()
    f, _ = new_batch("small")
    fresh_plain = f.run(pk)
    f.close()
    b, _ = new_batch("small")
    b.set_instance_regularization(instance_factors("small", len(probs)))
    mine = b.run(pk, regularization_type=1)
    plain = b.run(pk)  # regularization_type 0: the setting is ignored
    plain_name = b.last_kernel()
    b.set_instance_regularization(None)
    shared_again = b.run(pk, regularization_factors=shared, regularization_type=1)
    b.close()
    assert "regularized" not in plain_name, plain_name
    assert_same_run(plain, fresh_plain)
    assert_same_run(shared_again, fresh_shared)
    assert np.abs(mine["x"] - fresh_shared["x"]).max() > 0.0
    assert_same_run(mine, fused_run("small", 1)[0])


def _raw_run(b, pk, par, factors=None, v0=None):
    """lexls_lsi_batch_run with outputs pre-filled with 7 -> (return code, the outputs untouched)"""
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    x, info = np.full((pk.batch, pk.nvar), 7.0), np.full((pk.batch, 6), 7, np.int32)
    active, v, rounds = np.full((pk.batch, pk.total), 7, np.uint8), np.full((pk.batch, pk.total), 7.0), np.full(2, 7, np.int32)
    rc = capi.lib().lexls_lsi_batch_run(b._h, p(pk.data, C.c_double), p(pk.var_index, C.c_uint32), None, None, p(v0, C.c_double), p(factors, C.c_double),
                                        p(par, C.c_double), C.c_uint32(len(par)), p(x, C.c_double), p(info, C.c_int32), p(active, C.c_uint8), p(v, C.c_double),
                                        p(rounds, C.c_int32))
    return rc, all(bool((a == 7).all()) for a in (x, info, active, v, rounds))


def _raw_run_device(b, pk, par, d_data, d_var, factors=None):
    dev = torch.device("cuda", 0)
    out = [torch.full((pk.batch, pk.nvar), 7.0, dtype=torch.float64, device=dev), torch.full((pk.batch, 6), 7, dtype=torch.int32, device=dev),
           torch.full((pk.batch, pk.total), 7, dtype=torch.uint8, device=dev), torch.full((pk.batch, pk.total), 7.0, dtype=torch.float64, device=dev)]
    torch.cuda.synchronize()
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = capi.lib().lexls_lsi_batch_run_device(b._h, ptr(d_data), ptr(d_var), None, None, None if factors is None else factors.ctypes.data_as(C.POINTER(C.c_double)),
                                               par.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(par)), *[ptr(a) for a in out])
    torch.cuda.synchronize()
    return rc, all(bool((a == 7).all()) for a in out)


def test_errors_leave_the_outputs_alone(hip, monkeypatch):
    n, shared, probs = make("small")
    rows = instance_factors("small", len(probs))
    shared = np.asarray(shared, np.float64)
    b, pk = new_batch("small")
    d_data, d_var = device_inputs(pk)
    tik, type7 = lexlsi.pack_params_ex(regularization_type=1), lexlsi.pack_params_ex(regularization_type=7)
    v0 = np.zeros((pk.batch, pk.total))
    try:
        # both factor sources given: host setting, device setting; run and run_device; the Python binding raises the library's error
        b.set_instance_regularization(rows)
        assert _raw_run(b, pk, tik, factors=shared) == (LEXLS_ERR_INVALID, True)
        assert _raw_run_device(b, pk, tik, d_data, d_var, factors=shared) == (LEXLS_ERR_INVALID, True)
        with pytest.raises(capi.LexlsError, match="h_reg_factors must be NULL"):
            b.run(pk, regularization_factors=shared, regularization_type=1)
        with pytest.raises(capi.LexlsError, match="h_reg_factors must be NULL"):
            b.run_device(d_data, d_var, regularization_factors=shared, regularization_type=1)
        # host factors: the type-7 run proceeds on the host path, v0 is taken
        assert _raw_run(b, pk, type7)[0] == 0 and b.last_kernel() == "host"
        assert _raw_run(b, pk, tik, v0=v0)[0] == 0
        d_rows = to_device(rows)
        b.set_instance_regularization(d_rows)
        assert _raw_run(b, pk, tik, factors=shared) == (LEXLS_ERR_INVALID, True)
        # device factors: no v0 on run, no run that is not resident
        assert _raw_run(b, pk, tik, v0=v0) == (LEXLS_ERR_UNSUPPORTED, True)
        assert _raw_run(b, pk, type7) == (LEXLS_ERR_UNSUPPORTED, True)
        assert _raw_run_device(b, pk, type7, d_data, d_var) == (LEXLS_ERR_UNSUPPORTED, True)
        assert _raw_run(b, pk, lexlsi.pack_params_ex(regularization_type=1, cycling_handling_enabled=1)) == (LEXLS_ERR_UNSUPPORTED, True)
        # ... and the object serves the next correct run
        assert_same_run(b.run(pk, regularization_type=1), fused_run("small", 1)[0])
    finally:
        b.close()
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    h, _ = new_batch("small")
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    try:
        h.set_instance_regularization(d_rows)
        assert _raw_run(h, pk, tik) == (LEXLS_ERR_UNSUPPORTED, True)
    finally:
        h.close()
    # a shape without a register-resident kernel (levels of 20 rows): device factors are refused by the setter itself
    wide = [P.lsi_problem(5, 30, [20, 20])]
    wpk = lexlsi.pack_batch(30, wide)
    w = lexlsi.LsiBatch(30, wpk.dims, wpk.types, 1)
    try:
        rc = capi.lib().lexls_lsi_batch_set_instance_regularization(w._h, C.c_void_p(d_rows.data_ptr()), 1)
        assert rc == LEXLS_ERR_UNSUPPORTED
        assert capi.lib().lexls_lsi_batch_set_instance_regularization(w._h, rows.ctypes.data_as(C.c_void_p), 0) == 0
    finally:
        w.close()


def test_one_by_one_path(hip, oracle, monkeypatch):
    n, _, probs = make("small")
    rows = instance_factors("small", len(probs))
    par = dict(regularization_type=1, deactivate_first_wrong_sign=1)
    assert_rows_matter(oracle, "small", rows, **par)
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")
    b, pk = new_batch("small")
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    b.set_instance_regularization(rows)
    r = b.run(pk, **par)
    name = b.last_kernel()
    b.close()
    assert name == "host"
    assert_equals_oracle(r, oracle_refs(oracle, "small", rows, **par))


def test_three_paths_warm_start(hip, oracle, monkeypatch):
    """the configs[4] recipe (test_three_paths_warm_start of tests/test_gpu_lsi_regularized_resident.py) with per-instance factors"""
    n, shared, base = make("ik")
    count = len(base)
    rows = instance_factors("ik_perturbed", count)
    cold = lexlsi.lsi_batch_solve(n, base, regularization_factors=shared, regularization_type=1)
    guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
    start = dict(guesses=guess, x0=cold["x"])
    assert_rows_matter(oracle, "ik_perturbed", rows, regularization_type=1, **start)
    run_args = dict(active_guess=guess, x0=cold["x"], regularization_type=1)
    b, pk = new_batch("ik_perturbed")
    b.set_instance_regularization(rows)
    fused = b.run(pk, **run_args)
    assert b.last_kernel().startswith("lsi_fused<") and b.last_kernel().endswith("regularized>>")
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    staged = b.run(pk, **run_args)
    assert b.last_kernel().startswith("lqr_wave<") and b.last_kernel().endswith("regularized>")
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")
    b.close()
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")
    h, _ = new_batch("ik_perturbed")
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    h.set_instance_regularization(rows)
    host = h.run(pk, **run_args)
    assert h.last_kernel() == "host"
    h.close()
    assert_same_run(staged, fused)
    assert_same_run(host, fused)
    assert_equals_oracle(fused, oracle_refs(oracle, "ik_perturbed", rows, regularization_type=1, **start))
