"""lexls_lsi_batch_set_instance_mask (LsiBatch.set_instance_mask): a byte per instance in device memory, read by the kernels of every device run;
0 skips the instance.  The tolerance is zero, as for every LexLSI path.  The reference of a solved instance's rows is the same call on the same
data with no mask set, on a batch object of its own; the reference of a skipped instance's rows is the sentinel (or the earlier answer) the test
put there before the run.  Every caller-owned output is requested — x, info, active, v, the cycling counts and, where the run has them, the
multipliers — and every comparison is assert_array_equal on the bits.

Entries: lexls_lsi_batch_run_device_ex ("sync") and lexls_lsi_batch_enqueue_device + lexls_lsi_batch_finish ("enqueue").

Shapes: bounds, n = 14, (4, 5, 5, 4) with simple bounds, 40 instances (ten workgroups of the four-instance kernels); ik, n = 40, 5 x 12, 12 instances
(the 41 x 12 instantiation at its full width); wide, n = 50 (51 columns, the 64 x 16 instantiation), 8 instances.  LEXLS_LSI_NO_FUSED=1 and
LEXLS_LSI_GROUPS=2 are read when a run starts / a batch is created, so those cases and the capture run this file's child_* functions in a process
of their own, under a time limit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

from lexls_amd import capi, lexlsi, problems as P
from test_gpu_lsi_cycling_resident import CAP3, degenerate
from test_gpu_lsi_device_entry_ex import SHAPES as CHAIN_SHAPES, chain
from test_gpu_lsi_working_set_log import make_wide

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LEXLS_ERR_INVALID, LEXLS_ERR_UNSUPPORTED = 1, 3
SENTINEL = 7  # every element of every output, as sentinel_outputs of tests/test_gpu_lsi_device_entry_ex.py
CAPACITY = 128  # working-set log entries per instance (tests/test_gpu_lsi_working_set_log.py: above the longest log of these batches)
KEYS = ("x", "info", "active", "v", "lambda", "cycling_counters")
ENTRIES = ("sync", "enqueue")
_cache = {}


def device():
    return torch.device("cuda", 0)


def packed(shape, maker=P.lsi_problem):
    key = ("packed", shape, maker.__name__)
    if key not in _cache:
        if shape == "wide":
            s, probs = make_wide(8)
        else:
            s = CHAIN_SHAPES[shape]
            probs = [maker(seed, s["n"], s["dims"], simple_bounds=s["simple_bounds"]) for seed in s["seeds"]]
        _cache[key] = lexlsi.pack_batch(s["n"], probs)
    return _cache[key]


def upload(pk, guess=None, x0=None, v0=None):
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(device())
    return dict(data=up(pk.data.reshape(pk.batch, -1), np.float64), var_index=None if pk.var_index is None else up(pk.var_index.reshape(pk.batch, -1).view(np.int32), np.int32),
                active_guess=up(guess, np.uint8), x0=up(x0, np.float64), v0=up(v0, np.float64))


def new_batch(pk, log=False):
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    if log:
        b.set_working_set_log(CAPACITY)
    return b


def sentinel_outputs(pk):
    shapes = dict(x=((pk.batch, pk.nvar), torch.float64), info=((pk.batch, 6), torch.int32), active=((pk.batch, pk.total), torch.uint8), v=((pk.batch, pk.total), torch.float64),
                  cycling_counters=((pk.batch,), torch.int32), **{"lambda": ((pk.batch, len(pk.dims), pk.total), torch.float64)})
    out = {k: torch.full(s, SENTINEL, dtype=d, device=device()) for k, (s, d) in shapes.items()}
    torch.cuda.synchronize()
    return out


def params_of(kw):
    return lexlsi.pack_params_ex(**kw) if any(k in lexlsi.REG_PARAM_KEYS for k in kw) else lexlsi.pack_params(**kw)


def solve(entry, b, t, out, lam=True, status=None, regularization_factors=None, **kw):
    """one run through `entry` into the tensors of `out` -> the return code (of finish, for an enqueued run that was accepted)"""
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    torch.cuda.synchronize()
    if entry == "sync":
        par = lexlsi.pack_params_ex(**kw) if regularization_factors is not None else params_of(kw)
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        rc = capi.lib().lexls_lsi_batch_run_device_ex(
            b._h, ptr(t["data"]), ptr(t["var_index"]), ptr(t.get("active_guess")), ptr(t.get("x0")), ptr(t.get("v0")), None if rfa is None else rfa.ctypes.data_as(C.POINTER(C.c_double)),
            par.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint32(len(par)), ptr(out["x"]), ptr(out["info"]), ptr(out["active"]), ptr(out["v"]), ptr(out["lambda"]) if lam else None,
            ptr(out["cycling_counters"]))
        torch.cuda.synchronize()
        return rc
    try:
        b.enqueue_device(t["data"], t["var_index"], t.get("active_guess"), t.get("x0"), regularization_factors=regularization_factors, v0=t.get("v0"), with_lambda=lam,
                         with_cycling_counters=True, status=status, out=out, **kw)
        b.finish()
    except capi.LexlsError as e:
        return int(str(e).split("error ")[1].split(":")[0])
    return 0


def host(out):
    torch.cuda.synchronize()
    return {k: a.detach().cpu().numpy().copy() for k, a in out.items()}


def rows(a):
    """the bytes of an array, one row per instance"""
    a = np.ascontiguousarray(a)
    return a.reshape(a.shape[0], -1).view(np.uint8)


def host_view(b, lam):
    """what the library keeps of the last run: the cycling counters, the working-set log when it is on and the multipliers when the run has them"""
    view = dict(counters=b.cycling_counters())
    if b._log_entries:
        view["log"], view["alpha"], view["counts"] = b.working_set_log_arrays()
    if lam:
        view["lambda"] = b.lambda_array()
    return view


def reference(entry, pk, t, key, lam=True, log=False, prepare=None, **kw):
    """the unmasked run: (outputs on the host, host view, kernel name); computed once per key on a batch object of its own, shared, never modified"""
    key = ("reference", entry, key)
    if key not in _cache:
        b = new_batch(pk, log)
        try:
            if prepare:
                prepare(b)
            out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
            assert solve(entry, b, t, out, lam=lam, status=status, **kw) == 0, capi.lib().lexls_last_error()
            got = host(out)
            if not lam:
                del got["lambda"]
            assert not any((a == SENTINEL).all() for a in got.values()), "the unmasked run left an output alone"
            _cache[key] = (got, host_view(b, lam), b.last_kernel())
        finally:
            b.close()
    return _cache[key]


def assert_rows(got, ref, mask, untouched, what):
    """solved instances: the rows of the unmasked run; skipped instances: the rows of `untouched` (None: the sentinel)"""
    solved = np.asarray(mask) != 0
    for k, r in ref.items():
        np.testing.assert_array_equal(rows(got[k])[solved], rows(r)[solved], err_msg=f"{what}: {k} of the solved instances")
        if untouched is None:
            assert (got[k][~solved] == SENTINEL).all(), f"{what}: {k} of a skipped instance was written"
        else:
            np.testing.assert_array_equal(rows(got[k])[~solved], rows(untouched[k])[~solved], err_msg=f"{what}: {k} of the skipped instances")
    if "lambda" not in ref:  # not requested: nobody wrote it
        assert (got["lambda"] == SENTINEL).all(), what


def assert_host_view(view, ref, mask, what):
    """library-owned results describe the run: a skipped instance is an empty entry, a solved one has what the unmasked run has"""
    solved = np.asarray(mask) != 0
    assert set(view) == set(ref), what
    for k, r in ref.items():
        np.testing.assert_array_equal(rows(view[k])[solved], rows(r)[solved], err_msg=f"{what}: {k} of the solved instances")
        assert not rows(view[k])[~solved].any(), f"{what}: {k} of a skipped instance is not empty"


def patterns(batch):
    alt = np.arange(batch) % 2
    only = lambda i: (np.arange(batch) == i % batch).astype(np.uint8)
    other = np.where(np.arange(batch) % 3 == 1, 0, 2 + 23 * np.arange(batch) % 254)  # every third byte 0, the others 2 .. 255
    other[0] = 255
    return {"ones": np.ones(batch), "alternating": alt, "only instance 0": only(0), "only the last": only(-1), "all but one": 1 - only(batch // 2),
            "zeros": np.zeros(batch), "bytes other than 1": other}


def masked_run(entry, b, mask_t, mask, pk, t, ref, what, lam=True, untouched=None, out=None, **kw):
    """set the bytes of the batch's mask tensor, run into sentinels (or `out`), check every row and the status -> host copy of the outputs"""
    mask_t.copy_(torch.from_numpy(np.asarray(mask, np.uint8)))
    out = sentinel_outputs(pk) if out is None else out
    status = torch.zeros(1, dtype=torch.int32, device=device())
    assert solve(entry, b, t, out, lam=lam, status=status, **kw) == 0, (what, capi.lib().lexls_last_error())
    if entry == "enqueue":
        assert int(status.item()) == -1, what  # 0xffffffff
    got = host(out)
    assert_rows(got, ref[0], mask, untouched, what)
    assert_host_view(host_view(b, lam), ref[1], mask, what)
    return got


# ---- 1: mask patterns ----
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["bounds", "ik", "wide"])
def test_mask_patterns(hip, shape, entry):
    pk = packed(shape)
    t = upload(pk)
    ref = reference(entry, pk, t, shape)
    assert ref[2].startswith("lsi_fused<lqr_wave<64,16" if shape == "wide" else "lsi_fused<lqr_wave<41,12"), ref[2]
    b = new_batch(pk)
    try:
        mask_t = torch.ones(pk.batch, dtype=torch.uint8, device=device())
        b.set_instance_mask(mask_t)
        for name, mask in patterns(pk.batch).items():
            masked_run(entry, b, mask_t, mask, pk, t, ref, f"{shape}, {entry}, {name}")
            if name not in ("ones", "zeros"):
                assert b.last_kernel().startswith("lsi_fused<"), (name, b.last_kernel())
            if name == "ones":
                assert b.last_kernel() == ref[2]
        bool_mask = torch.from_numpy(patterns(pk.batch)["alternating"].astype(bool)).to(device())  # a bool tensor is a byte per instance as well
        b.set_instance_mask(bool_mask)
        masked_run(entry, b, bool_mask.view(torch.uint8), patterns(pk.batch)["alternating"], pk, t, ref, f"{shape}, {entry}, bool tensor")
    finally:
        b.close()


# ---- 2: poisoned skipped instances ----
def poison(pk, guess, x0, v0, instance, kind):
    """one fault of `kind` in `instance` of the bounds shape's arrays (simple bounds first: [lb (4) | ub (4)]) -> the code of the setup kernel's fault word"""
    data, var = pk.data.reshape(pk.batch, -1), pk.var_index.reshape(pk.batch, -1)
    if kind == "NaN data":
        data[instance] = np.nan
    elif kind == "lb > ub":
        data[instance, 2], data[instance, 4 + 2] = 1.0, 0.0
        return 1
    elif kind == "index >= nVar":
        var[instance, 1] = pk.nvar
        return 2
    elif kind == "repeated index":
        var[instance, 3] = var[instance, 0]
        return 3
    elif kind == "guess flag 9":
        guess[instance, 5] = 9
        return 4
    else:
        x0[instance], v0[instance] = np.nan, np.nan
    return None


def writable_chain():
    pk, _, guess, x0, v0 = chain("bounds")
    pk = lexlsi.PackedBatch(pk.nvar, pk.dims, pk.types, pk.data.copy(), pk.var_index.copy())
    return pk, guess.copy(), x0.copy(), v0.copy()


POISON = {3: "NaN data", 7: "lb > ub", 11: "index >= nVar", 17: "repeated index", 22: "guess flag 9", 39: "NaN x0 / v0"}


@pytest.mark.parametrize("entry", ENTRIES)
def test_poisoned_skipped_instances(hip, entry):
    clean, _, guess, x0, v0 = chain("bounds")
    ref = reference(entry, clean, upload(clean, guess, x0, v0), "bounds warm")
    pk, g, x, v = writable_chain()
    for instance, kind in POISON.items():
        poison(pk, g, x, v, instance, kind)
    mask = np.ones(pk.batch, np.uint8)
    mask[list(POISON)] = 0
    b = new_batch(pk)
    try:
        mask_t = torch.ones(pk.batch, dtype=torch.uint8, device=device())
        b.set_instance_mask(mask_t)
        masked_run(entry, b, mask_t, mask, pk, upload(pk, g, x, v), ref, f"{entry}: poisoned skipped instances")
        # the same faults in a solved instance are reported as without a mask, and name it
        for kind in ("lb > ub", "index >= nVar", "repeated index", "guess flag 9"):
            pk, g, x, v = writable_chain()
            code = poison(pk, g, x, v, 5, kind)
            out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
            assert solve(entry, b, upload(pk, g, x, v), out, status=status) == LEXLS_ERR_INVALID, kind
            assert "instance 5:" in capi.lib().lexls_last_error().decode(), kind
            if entry == "enqueue":
                assert int(status.item()) == 5 * 8 + code, kind
            assert all((a == SENTINEL).all() for a in host(out).values()), kind + ": an output was written"
        masked_run(entry, b, mask_t, mask, clean, upload(clean, guess, x0, v0), ref, f"{entry}: a good run after the faulty ones")
    finally:
        b.close()


# ---- 3: the mask rewritten in place ----
@pytest.mark.parametrize("entry", ENTRIES)
def test_mask_rewritten_in_place(hip, entry):
    pk = packed("bounds")
    t = upload(pk)
    ref = reference(entry, pk, t, "bounds")
    b = new_batch(pk)
    try:
        mask_t = (torch.arange(pk.batch, device=device()) % 2).to(torch.uint8)
        b.set_instance_mask(mask_t)
        for run in range(3):
            out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
            assert solve(entry, b, t, out, status=status) == 0
            assert_rows(host(out), ref[0], mask_t.cpu().numpy(), None, f"{entry}: run {run}")
            assert_host_view(host_view(b, True), ref[1], mask_t.cpu().numpy(), f"{entry}: run {run}")
            if run == 0:
                mask_t.logical_not_()  # a torch op on the tensor the library holds: the other half
            else:
                mask_t[: pk.batch // 4] = 1
                mask_t[pk.batch // 4:] = 0
    finally:
        b.close()


# ---- 4: capture ----
def child_capture():
    """an uncaptured masked enqueue + finish, a captured one, three replays with the mask and the data rewritten on the device in between: each
    replay against an uncaptured masked run on the same inputs.  A replay that reports a fault ends the test: nothing else is started"""
    pks = [lexlsi.pack_batch(CHAIN_SHAPES["bounds"]["n"], [P.lsi_problem(seed, 14, [4, 5, 5, 4], simple_bounds=True, perturb=1.0 if step else 0.0, perturb_seed=step)
                                                            for seed in CHAIN_SHAPES["bounds"]["seeds"]]) for step in range(4)]
    ts = [upload(pk) for pk in pks]  # (torch opens the device first)
    pk, pat = pks[0], patterns(pks[0].batch)
    ba, bs = new_batch(pk, log=True), new_batch(pk, log=True)
    stream = torch.cuda.Stream(device())
    data, mask_a, mask_s = ts[0]["data"].clone(), torch.ones(pk.batch, dtype=torch.uint8, device=device()), torch.ones(pk.batch, dtype=torch.uint8, device=device())
    ba.set_instance_mask(mask_a)
    bs.set_instance_mask(mask_s)
    out, status = sentinel_outputs(pk), torch.zeros(1, dtype=torch.int32, device=device())
    kw = dict(with_cycling_counters=True, with_lambda=True, status=status, out=out)
    mask_a.copy_(torch.from_numpy(pat["alternating"].astype(np.uint8)))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        ba.enqueue_device(data, ts[0]["var_index"], **kw)
    ba.finish()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        ba.enqueue_device(data, ts[0]["var_index"], **kw)
    for step, name in ((1, "all but one"), (2, "alternating"), (3, "bytes other than 1")):
        mask = torch.from_numpy(pat[name].astype(np.uint8)).to(device())
        with torch.cuda.stream(stream):
            for a in out.values():
                a.fill_(SENTINEL)
            mask_a.copy_(mask)
            data.copy_(ts[step]["data"])
            graph.replay()
        ba.finish(stream)  # (raises on a fault: the test ends here)
        assert int(status.item()) == -1, (step, int(status.item()))
        got, view = host(out), host_view(ba, True)
        mask_s.copy_(mask)
        ref_out = sentinel_outputs(pk)
        assert solve("enqueue", bs, ts[step], ref_out, status=torch.zeros(1, dtype=torch.int32, device=device())) == 0
        ref, ref_view = host(ref_out), host_view(bs, True)
        for k in KEYS:
            np.testing.assert_array_equal(rows(got[k]), rows(ref[k]), err_msg=f"replay {step}: {k}")
        for k in ref_view:
            np.testing.assert_array_equal(rows(view[k]), rows(ref_view[k]), err_msg=f"replay {step}: {k}")
        assert (got["x"][pat[name] == 0] == SENTINEL).all() and not (got["x"][pat[name] != 0] == SENTINEL).all(axis=1).any(), step
    ba.close()
    bs.close()


def in_child(name, limit=120, **env):
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_instance_mask as m; m.{name}()"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]


def test_capture(hip):
    in_child("child_capture")


# ---- 5: the closed loop ----
@pytest.mark.parametrize("entry", ENTRIES)
def test_closed_loop(hip, entry):
    """step 1 solves everybody; step 2 moves the data on the device, skips every second instance and starts from active / x / v of step 1 with v0
    given: the solved rows are step 2 of the unmasked loop, the skipped rows still hold the answers of step 1"""
    pk0 = packed("bounds")
    pk1 = chain("bounds")[0]
    mask = patterns(pk0.batch)["alternating"]
    delta = torch.from_numpy(pk1.data.reshape(pk1.batch, -1) - pk0.data.reshape(pk0.batch, -1)).to(device())

    def loop(masked):
        b = new_batch(pk0)
        try:
            t = upload(pk0)
            out = sentinel_outputs(pk0)
            assert solve(entry, b, t, out) == 0
            first = host(out)
            t["data"] += delta  # the data moves on the device
            t.update(active_guess=out["active"].clone(), x0=out["x"].clone(), v0=out["v"].clone())
            if masked:
                b.set_instance_mask(torch.from_numpy(mask.astype(np.uint8)).to(device()))
            assert solve(entry, b, t, out) == 0  # into the tensors that hold step 1
            return first, host(out), host_view(b, True)
        finally:
            b.close()

    first, second, view = loop(False)
    masked_first, masked_second, masked_view = loop(True)
    for k in KEYS:
        np.testing.assert_array_equal(rows(masked_first[k]), rows(first[k]), err_msg=k)
    assert not np.array_equal(rows(first["x"])[mask != 0], rows(second["x"])[mask != 0]), "step 2 changes no x: the loop shows nothing"
    assert_rows(masked_second, second, mask, first, f"{entry}: step 2")
    assert_host_view(masked_view, view, mask, f"{entry}: step 2")


# ---- 6: options ----
def removes_in(view, solved):
    """solved instances with a REMOVE entry (ctr_type 0) in the unmasked run's working-set log"""
    log, counts = view["log"], view["counts"]
    return [b for b in np.flatnonzero(solved) if any(log[b, i, 2] == 0 for i in range(min(int(counts[b]), CAPACITY)))]


def option_run(entry, name, pk, prepare=None, lam=False, **kw):
    t = upload(pk)
    ref = reference(entry, pk, t, name, lam=lam, log=True, prepare=prepare, **kw)
    mask = patterns(pk.batch)["alternating"]
    assert removes_in(ref[1], mask != 0), f"{name}: no solved instance logs a REMOVE"
    b = new_batch(pk, log=True)
    try:
        if prepare:
            prepare(b)
        mask_t = torch.ones(pk.batch, dtype=torch.uint8, device=device())
        b.set_instance_mask(mask_t)
        masked_run(entry, b, mask_t, mask, pk, t, ref, f"{entry}: {name}", lam=lam, **kw)
        assert b.last_kernel() == ref[2] and ref[2].startswith("lsi_fused<"), (b.last_kernel(), ref[2])
    finally:
        b.close()
    return ref, mask


FACTORS = [0.0, 0.02, 0.05, 0.03]  # bounds shape: one per objective


@pytest.mark.parametrize("entry", ENTRIES)
def test_tikhonov_with_shared_factors(hip, entry):
    ref, _ = option_run(entry, "TIKHONOV, shared factors", packed("bounds"), regularization_factors=FACTORS, regularization_type=1)
    assert "regularized" in ref[2], ref[2]


@pytest.mark.parametrize("entry", ENTRIES)
def test_device_per_instance_factors(hip, entry):
    pk = packed("bounds")
    factors = torch.from_numpy(np.ascontiguousarray(np.outer(1.0 + 0.25 * np.arange(pk.batch), FACTORS))).to(device())
    ref, _ = option_run(entry, "TIKHONOV, per-instance factors on the device", pk, prepare=lambda b: b.set_instance_regularization(factors), regularization_type=1)
    assert "regularized" in ref[2], ref[2]


@pytest.mark.parametrize("entry", ENTRIES)
def test_deactivate_first_wrong_sign(hip, entry):
    option_run(entry, "deactivate_first_wrong_sign", packed("bounds"), lam=True, deactivate_first_wrong_sign=1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_cycling_handling(hip, entry):
    ref, mask = option_run(entry, "cycling handling", packed("bounds", degenerate), **CAP3)
    relaxing = ref[1]["counters"] > 0
    assert relaxing.sum() >= 38, "fewer than 38 of the 40 degenerate instances relax a bound"
    assert (relaxing & (mask != 0)).sum() >= 10, "fewer than 10 relaxing instances are solved"
    np.testing.assert_array_equal(ref[0]["cycling_counters"].view(np.uint32), ref[1]["counters"])


# ---- 7: the stage path ----
def child_stage_path():
    pk = packed("bounds")
    t = upload(pk)
    ref = reference("sync", pk, t, "bounds, stages", log=True)
    assert not ref[2].startswith("lsi_fused<") and ref[2] not in ("host", ""), ref[2]
    b = new_batch(pk, log=True)
    mask_t = torch.ones(pk.batch, dtype=torch.uint8, device=device())
    b.set_instance_mask(mask_t)
    for name in ("alternating", "all but one", "zeros"):
        masked_run("sync", b, mask_t, patterns(pk.batch)[name], pk, t, ref, "LEXLS_LSI_NO_FUSED=1, " + name)
        assert name == "zeros" or b.last_kernel() == ref[2], (name, b.last_kernel(), ref[2])
    b.close()


def test_stage_path(hip):
    in_child("child_stage_path", LEXLS_LSI_NO_FUSED="1")


# ---- 8: two groups ----
def child_two_groups():
    """group g reads the mask from byte lo[g]: the two halves of the mask differ"""
    pk = packed("bounds")
    t = upload(pk)
    ref = reference("sync", pk, t, "bounds, two groups", log=True)
    half = pk.batch // 2
    mask = np.concatenate([np.arange(half) % 2, 1 - np.arange(pk.batch - half) % 2, ])
    mask[half + 4:half + 9] = 0
    assert not np.array_equal(mask[:half], mask[half:])
    b = new_batch(pk, log=True)
    mask_t = torch.ones(pk.batch, dtype=torch.uint8, device=device())
    b.set_instance_mask(mask_t)
    masked_run("sync", b, mask_t, mask, pk, t, ref, "LEXLS_LSI_GROUPS=2")
    assert b.stats()["groups"] == 2
    masked_run("sync", b, mask_t, np.concatenate([np.zeros(half), np.ones(pk.batch - half)]), pk, t, ref, "LEXLS_LSI_GROUPS=2, the first group skipped")
    b.close()


def test_two_groups(hip):
    in_child("child_two_groups", LEXLS_LSI_GROUPS="2")


# ---- 9: refusals and clearing ----
def test_run_is_refused_and_none_clears(hip):
    pk = packed("bounds")
    t = upload(pk)
    b, fresh = new_batch(pk), new_batch(pk)
    try:
        b.set_instance_mask(torch.ones(pk.batch, dtype=torch.uint8, device=device()))
        with pytest.raises(capi.LexlsError) as e:
            b.run(pk)
        assert str(e.value).startswith(f"liblexls_hip error {LEXLS_ERR_UNSUPPORTED}:") and "mask" in str(e.value), str(e.value)
        x, info = np.full((pk.batch, pk.nvar), 7.0), np.full((pk.batch, 6), 7, np.int32)
        active, v, rounds = np.full((pk.batch, pk.total), 7, np.uint8), np.full((pk.batch, pk.total), 7.0), np.full(2, 7, np.int32)
        par = lexlsi.pack_params()
        p = lambda a, c: a.ctypes.data_as(C.POINTER(c))
        rc = capi.lib().lexls_lsi_batch_run(b._h, p(pk.data, C.c_double), p(pk.var_index, C.c_uint32), None, None, None, None, p(par, C.c_double), C.c_uint32(len(par)),
                                            p(x, C.c_double), p(info, C.c_int32), p(active, C.c_uint8), p(v, C.c_double), p(rounds, C.c_int32))
        assert rc == LEXLS_ERR_UNSUPPORTED and "mask" in capi.lib().lexls_last_error().decode()
        assert all((a == 7).all() for a in (x, info, active, v, rounds)), "a refused run wrote an output"
        b.set_instance_mask(None)
        got, want = b.run(pk), fresh.run(pk)
        np.testing.assert_array_equal(got["info"].array, want["info"].array)
        for k in ("x", "active", "v"):
            np.testing.assert_array_equal(rows(got[k]), rows(want[k]), err_msg=k)
        out, fresh_out = sentinel_outputs(pk), sentinel_outputs(pk)
        assert solve("sync", b, t, out) == 0 and solve("sync", fresh, t, fresh_out) == 0
        got, want = host(out), host(fresh_out)
        for k in KEYS:
            np.testing.assert_array_equal(rows(got[k]), rows(want[k]), err_msg=k)
        assert b.last_kernel() == fresh.last_kernel() and b.stats() == fresh.stats()
        assert not (got["x"] == SENTINEL).all(axis=1).any(), "an instance was skipped after the mask was cleared"
    finally:
        b.close()
        fresh.close()
