"""lexls_lsi_batch_enqueue_device / lexls_lsi_batch_finish (LsiBatch.enqueue_device, LsiBatch.finish): the device entry of a LexLSI batch as work in a
stream.  The tolerance is zero: x, info, the final working set, v, the cycling counts, the multipliers (those the call writes into device memory and those of get_lambda after finish) and the working-set log of an enqueued run are
compared bit for bit with LsiBatch.run_device on a second batch object that went through the same calls.

Shapes: n = 8, objectives (6 simple bounds, 5, 4) and (5, 4, 3) general only, 7 instances (two workgroups of the four-instance kernels, the second
one partly filled).  LEXLS_LSI_GROUPS=2 (6 instances: refused, several groups are not served) and LEXLS_LSI_NO_FUSED=1 are read when a batch is
created / a run starts, so those cases run this file's child_* functions in a process of their own, under a time limit, as does the capture.  The inputs that relax bounds are those of
tests/test_gpu_lsi_cycling_resident.py (degenerate)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lexls_amd import capi, lexlsi, problems as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 8
SHAPES = {"bounds": dict(dims=[6, 5, 4], simple_bounds=True), "general": dict(dims=[5, 4, 3], simple_bounds=False)}
CAP3 = dict(tol_wrong_sign_lambda=0.0, cycling_handling_enabled=1, cycling_max_counter=3, cycling_relax_step=1e-6)
LOG_ENTRIES = 24
LEXLS_ERR_INVALID, LEXLS_ERR_UNSUPPORTED = 1, 3
SENTINEL = {"x": -7.5, "info": -77, "active": 9, "v": -3.25, "cycling_counters": -5, "lambda": -1.5}


def degenerate(seed, dims, simple_bounds, **kw):
    from test_gpu_lsi_cycling_resident import degenerate as make
    return make(seed, N, dims, simple_bounds)


def problems(shape, batch=7, maker=None, perturb=0.0):
    s = SHAPES[shape]
    if maker is not None:
        return [maker(100 + i, s["dims"], s["simple_bounds"]) for i in range(batch)]
    return [P.lsi_problem(100 + i, N, s["dims"], simple_bounds=s["simple_bounds"], perturb=perturb, perturb_seed=1 if perturb else 0) for i in range(batch)]


def relaxing_problems(shape, batch):
    """`batch` degenerate problems that relax a bound.  Few of the degenerate problems of these small shapes do, so they are picked from 70
    candidates by the synchronous entry (LsiBatch.run_device, the reference of every comparison here): the first `batch` whose counter is not zero"""
    s = SHAPES[shape]
    candidates = [degenerate(100 + i, s["dims"], s["simple_bounds"]) for i in range(70)]
    pk = lexlsi.pack_batch(N, candidates)
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    try:
        t = upload(pk)
        counts = b.run_device(t["data"], t["var_index"], with_cycling_counters=True, **CAP3)["cycling_counters"].cpu().numpy()
    finally:
        b.close()
    picked = [p for p, c in zip(candidates, counts) if c][:batch]
    assert len(picked) == batch, f"{shape}: only {len(picked)} of the 70 degenerate candidates relax a bound"
    return picked


def device():
    import torch
    return torch.device("cuda", 0)


def upload(pk):
    import torch
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(device())
    return dict(data=up(pk.data, np.float64), var_index=None if pk.var_index is None else up(pk.var_index.view(np.int32), np.int32))


def new_batch(pk, log=True):
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    if log:
        b.set_working_set_log(LOG_ENTRIES)
    return b


def bits(t):
    return t.detach().cpu().numpy().view(np.uint8)


def assert_same_results(got, ref, what):
    assert set(got) == set(ref), what
    for k in ref:
        np.testing.assert_array_equal(bits(got[k]), bits(ref[k]), err_msg=f"{what}: {k}")


def assert_same_host_view(ba, bs, what, lam, fused=True):
    """what the getters answer after finish() against what they answer after run_device(); fused = False: the run may have ended in iteration 0
    on every instance (a warm start next to its answer), after which both entries name 'host'"""
    assert ba.last_kernel() == bs.last_kernel() and (not fused or ba.last_kernel().startswith("lsi_fused<")), (what, ba.last_kernel(), bs.last_kernel())
    assert ba.stats() == bs.stats(), what
    np.testing.assert_array_equal(ba.cycling_counters(), bs.cycling_counters(), err_msg=what + ": cycling counters")
    for a, s in zip(ba.working_set_log_arrays(), bs.working_set_log_arrays()):
        np.testing.assert_array_equal(a.view(np.uint8), s.view(np.uint8), err_msg=what + ": working-set log")
    for a, s in zip(ba.working_set_log_device().values(), bs.working_set_log_device().values()):
        np.testing.assert_array_equal(bits(a), bits(s), err_msg=what + ": working-set log on the device")
    if lam:
        np.testing.assert_array_equal(ba.lambda_array().view(np.uint64), bs.lambda_array().view(np.uint64), err_msg=what + ": lambda")


def solve_both(ba, bs, t, what, lam=True, stream=None, **kw):
    """one run through enqueue_device + finish on ba and through run_device on bs: the same bits everywhere.  -> the reference result"""
    import torch
    status = torch.zeros(1, dtype=torch.int32, device=device())
    got = ba.enqueue_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=lam, stream=stream, status=status, **kw)
    ba.finish()
    ref = bs.run_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=lam, **kw)
    assert int(status.item()) == -1, what
    assert_same_results(got, ref, what)
    assert_same_host_view(ba, bs, what, lam)
    return ref


def equality_configurations(shape, batch):
    """every configuration of the equality test on one pair of batch objects (each also a run after another kind of run on the same objects)"""
    import torch
    pk0, pk1 = (lexlsi.pack_batch(N, problems(shape, batch, perturb=p)) for p in (0.0, 1.0))
    nobj = len(pk0.dims)
    ba, bs = new_batch(pk0), new_batch(pk0)
    try:
        t0, t1 = upload(pk0), upload(pk1)
        first = solve_both(ba, bs, t0, "cold")
        solve_both(ba, bs, t1, "x0 + guess", active_guess=first["active"], x0=first["x"])
        solve_both(ba, bs, t1, "x0 + v0", active_guess=first["active"], x0=first["x"], v0=first["v"])
        factors = [0.0] + [0.02 + 0.01 * k for k in range(1, nobj)]
        solve_both(ba, bs, t0, "TIKHONOV, shared factors", lam=False, regularization_factors=factors, regularization_type=1)
        rows = torch.from_numpy(np.ascontiguousarray(np.outer(1.0 + 0.25 * np.arange(batch), factors))).to(device())
        for b in (ba, bs):
            b.set_instance_regularization(rows)
        solve_both(ba, bs, t0, "TIKHONOV, per-instance factors on the device", lam=False, regularization_type=1)
        for b in (ba, bs):
            b.set_instance_regularization(None)
        solve_both(ba, bs, t0, "deactivate_first_wrong_sign", deactivate_first_wrong_sign=1)
        td = upload(lexlsi.pack_batch(N, relaxing_problems(shape, batch)))
        ref = bs.run_device(td["data"], td["var_index"], with_cycling_counters=True, **CAP3)
        assert int(ref["cycling_counters"].cpu().numpy().view(np.uint32).sum()) > 0, "the degenerate inputs relax no bound: the cycling handler is not exercised"
        solve_both(ba, bs, td, "cycling handling", lam=False, **CAP3)
    finally:
        ba.close()
        bs.close()


def capture_and_replay(shape, batch):
    """warm up, capture one enqueue, rewrite the data in place, replay once, finish: the results of run_device on the new data"""
    import torch
    pk0, pk1 = (lexlsi.pack_batch(N, problems(shape, batch, perturb=p)) for p in (0.0, 1.0))
    ba, bs = new_batch(pk0), new_batch(pk0)
    try:
        t, t1 = upload(pk0), upload(pk1)
        stream = torch.cuda.Stream(device())
        out = {k: torch.zeros_like(a) for k, a in bs.run_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=True).items()}
        status = torch.zeros(1, dtype=torch.int32, device=device())
        with torch.cuda.stream(stream):
            ba.enqueue_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=True, status=status, out=out)  # the uncaptured run that may allocate
        ba.finish()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            ba.enqueue_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=True, status=status, out=out)
        for a in out.values():
            a.fill_(SENTINEL["info"] if a.dtype == torch.int32 else 3)
        with torch.cuda.stream(stream):
            t["data"].copy_(t1["data"])
            graph.replay()
        ba.finish(stream)
        ref = bs.run_device(t1["data"], t1["var_index"], with_cycling_counters=True, with_lambda=True)
        assert int(status.item()) == -1
        assert_same_results(out, ref, "replay")
        assert_same_host_view(ba, bs, "replay", True)
    finally:
        ba.close()
        bs.close()


def capture_closed_loop():
    """the closed loop as a graph: ONE captured step — the data moves, the run starts from active / x / v of the previous answer, which are its own
    output tensors — replayed five times back to back, finish, and all of it once more behind that finish: every time the five-step run_device chain.
    (The fault word is set anew by every replay: a replay that found it stale would stop every instance.)"""
    import torch
    pk0 = lexlsi.pack_batch(N, problems("bounds"))
    t = upload(pk0)  # (torch opens the device first)
    ba, bs = new_batch(pk0), new_batch(pk0)
    try:
        step = 0.05 * torch.randn(t["data"].shape, dtype=torch.float64, device=device(), generator=torch.Generator(device()).manual_seed(1))
        step[:, :12] = 0.0  # (the simple bounds stay ordered; the general rows' intervals move as one with their matrices: only A changes)
        o = 12
        for d in (5, 4):
            step[:, o + d * N: o + d * (N + 2)] = 0.0
            o += d * (N + 2)
        stream, data = torch.cuda.Stream(device()), t["data"].clone()
        status = torch.zeros(1, dtype=torch.int32, device=device())
        kw = dict(with_cycling_counters=True, with_lambda=True, status=status)
        with torch.cuda.stream(stream):
            state = ba.enqueue_device(data, t["var_index"], **kw)
            ba.enqueue_device(data, t["var_index"], active_guess=state["active"], x0=state["x"], v0=state["v"], out=state, **kw)  # the options of the captured call
        ba.finish()
        with torch.cuda.stream(stream):
            ba.enqueue_device(data, t["var_index"], out=state, **kw)
        ba.finish()
        cold = {k: a.clone() for k, a in state.items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            data += step
            ba.enqueue_device(data, t["var_index"], active_guess=state["active"], x0=state["x"], v0=state["v"], out=state, **kw)
        for turn in range(2):
            with torch.cuda.stream(stream):
                data.copy_(t["data"])
                for k, a in cold.items():
                    state[k].copy_(a)
                for _ in range(5):
                    graph.replay()
            ba.finish(stream)
            d, ref = t["data"].clone(), cold
            for _ in range(5):
                d += step
                ref = bs.run_device(d, t["var_index"], active_guess=ref["active"], x0=ref["x"], v0=ref["v"], with_cycling_counters=True, with_lambda=True)
            assert int(status.item()) == -1, turn
            assert_same_results(state, ref, f"five replays, turn {turn}")
            assert_same_host_view(ba, bs, f"five replays, turn {turn}", True, fused=False)
    finally:
        ba.close()
        bs.close()


def capture_replay_after_input_error():
    """one captured enqueue replayed on faulty data (status and finish report it, the outputs keep their sentinel), then on good data: the fault word of
    the first replay does not reach the second one"""
    import torch
    bad, instance, code = faulty("lb > ub")
    good = lexlsi.pack_batch(N, problems("bounds", perturb=1.0))
    tb, tg = upload(bad), upload(good)
    ba, bs = new_batch(good), new_batch(good)
    try:
        stream, data = torch.cuda.Stream(device()), tg["data"].clone()
        out, status = sentinel_outputs(ba), torch.zeros(1, dtype=torch.int32, device=device())
        kw = dict(with_cycling_counters=True, with_lambda=True, status=status, out=out)
        with torch.cuda.stream(stream):
            ba.enqueue_device(data, tg["var_index"], **kw)
        ba.finish()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ba.enqueue_device(data, tg["var_index"], **kw)
        with torch.cuda.stream(stream):
            for k, a in out.items():
                a.fill_(SENTINEL[k])
            data.copy_(tb["data"])
            graph.replay()
        with pytest.raises(capi.LexlsError) as e:
            ba.finish(stream)
        assert f"instance {instance}:" in str(e.value)
        assert int(status.item()) == instance * 8 + code
        assert_sentinels(out, "replay on faulty data")
        with torch.cuda.stream(stream):
            data.copy_(tg["data"])
            graph.replay()
        ba.finish(stream)
        ref = bs.run_device(tg["data"], tg["var_index"], with_cycling_counters=True, with_lambda=True)
        assert int(status.item()) == -1
        assert_same_results(out, ref, "replay on good data after a faulty one")
        assert_same_host_view(ba, bs, "replay on good data after a faulty one", True)
    finally:
        ba.close()
        bs.close()


def child_two_groups():
    """a batch split into groups (LEXLS_LSI_GROUPS=2) is not served: refused before any device work; the synchronous entry goes on serving it"""
    pk = lexlsi.pack_batch(N, problems("bounds", 6))
    t = upload(pk)  # (torch opens the device first)
    b = new_batch(pk, log=False)
    try:
        out = sentinel_outputs(b)
        assert raw_enqueue(b, t, out) == LEXLS_ERR_UNSUPPORTED
        assert_sentinels(out, "LEXLS_LSI_GROUPS=2")
        b.run_device(t["data"], t["var_index"])
        assert b.stats()["groups"] == 2
    finally:
        b.close()


def child_no_fused():
    import torch
    pk = lexlsi.pack_batch(N, problems("bounds"))
    b, t = new_batch(pk, log=False), upload(pk)
    try:
        out = sentinel_outputs(b)
        rc = raw_enqueue(b, t, out)
        assert rc == LEXLS_ERR_UNSUPPORTED, rc
        assert_sentinels(out, "LEXLS_LSI_NO_FUSED=1")
    finally:
        b.close()


def in_child(name, limit=150, **env):
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_enqueue_device as m; m.{name}()"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]


def sentinel_outputs(b):
    import torch
    shapes = dict(x=((b.batch, b.nvar), torch.float64), info=((b.batch, 6), torch.int32), active=((b.batch, b.total), torch.uint8),
                  v=((b.batch, b.total), torch.float64), cycling_counters=((b.batch,), torch.int32), **{"lambda": ((b.batch, len(b.dims), b.total), torch.float64)})
    return {k: torch.full(s, SENTINEL[k], dtype=d, device=device()) for k, (s, d) in shapes.items()}


def assert_sentinels(out, what):
    for k, a in out.items():
        assert bool((a == SENTINEL[k]).all()), f"{what}: {k} was written"


def raw_enqueue(b, t, out, status=None, with_lambda=True, **kw):
    """enqueue_device's return code instead of its exception"""
    import torch
    torch.cuda.synchronize()
    try:
        b.enqueue_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=with_lambda, status=status, out=out, **kw)
    except capi.LexlsError as e:
        return int(str(e).split("error ")[1].split(":")[0])
    return 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_enqueue_and_finish_equal_run_device(shape):
    equality_configurations(shape, 7)


def test_two_groups_are_refused():
    in_child("child_two_groups", limit=120, LEXLS_LSI_GROUPS="2")


def test_alternating_with_run_device():
    """enqueue_device and run_device take turns on ONE batch object, through plain, regularized and warm-started runs: every answer is that of a
    batch object that only ever ran run_device (what one entry leaves in the batch does not reach the other's next run)"""
    pk0, pk1 = (lexlsi.pack_batch(N, problems("bounds", perturb=p)) for p in (0.0, 1.0))
    ba, bs = new_batch(pk0), new_batch(pk0)
    try:
        t0, t1 = upload(pk0), upload(pk1)
        reg = dict(regularization_factors=[0.0, 0.03, 0.04], regularization_type=1)
        first = solve_both(ba, bs, t0, "enqueue, plain")
        for what, t, lam, kw in (("run_device, regularized", t0, False, reg), ("enqueue, warm", t1, True, dict(active_guess=first["active"], x0=first["x"], v0=first["v"])),
                                 ("run_device, plain", t1, True, {}), ("enqueue, regularized", t0, False, reg), ("run_device, first wrong sign", t0, True, dict(deactivate_first_wrong_sign=1)),
                                 ("enqueue, plain again", t0, True, {})):
            if what.startswith("enqueue"):
                solve_both(ba, bs, t, what, lam=lam, **kw)
            else:
                got = ba.run_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=lam, **kw)
                ref = bs.run_device(t["data"], t["var_index"], with_cycling_counters=True, with_lambda=lam, **kw)
                assert_same_results(got, ref, what)
                assert_same_host_view(ba, bs, what, lam)
    finally:
        ba.close()
        bs.close()


def test_stream_order():
    """enqueue on a side stream, a torch op on x behind it, a second enqueue warm-started from the first one's outputs, one finish: the two-step
    run_device chain, and the op saw the complete x"""
    import torch
    pk0, pk1 = (lexlsi.pack_batch(N, problems("bounds", perturb=p)) for p in (0.0, 1.0))
    ba, bs = new_batch(pk0), new_batch(pk0)
    try:
        t0, t1 = upload(pk0), upload(pk1)
        stream = torch.cuda.Stream(device())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            first = ba.enqueue_device(t0["data"], t0["var_index"], with_cycling_counters=True, with_lambda=True)
            doubled = first["x"] * 2.0
            second = ba.enqueue_device(t1["data"], t1["var_index"], active_guess=first["active"], x0=first["x"], v0=first["v"], with_cycling_counters=True, with_lambda=True)
        ba.finish()
        ref0 = bs.run_device(t0["data"], t0["var_index"], with_cycling_counters=True, with_lambda=True)
        ref1 = bs.run_device(t1["data"], t1["var_index"], active_guess=ref0["active"], x0=ref0["x"], v0=ref0["v"], with_cycling_counters=True, with_lambda=True)
        assert_same_results(first, ref0, "first step")
        np.testing.assert_array_equal(bits(doubled), bits(ref0["x"] * 2.0), err_msg="the consumer of x in the same stream")
        assert_same_results(second, ref1, "second step")
        assert_same_host_view(ba, bs, "second step", True)
    finally:
        ba.close()
        bs.close()


def test_capture_and_replay():
    in_child("capture_and_replay_bounds_7", limit=120)


def test_captured_closed_loop():
    in_child("capture_closed_loop", limit=120)


def test_captured_replay_after_input_error():
    in_child("capture_replay_after_input_error", limit=120)


def capture_and_replay_bounds_7():
    capture_and_replay("bounds", 7)


def faulty(kind):
    """-> (packed batch, instance, code): instance 4 of the bounds shape with one input error"""
    probs = problems("bounds")
    pk = lexlsi.pack_batch(N, probs)
    data, var = pk.data.reshape(pk.batch, -1).copy(), pk.var_index.reshape(pk.batch, -1).copy()
    if kind == "lb > ub":
        data[4, 2], data[4, 6 + 2], code = 1.0, 0.0, 1  # simple bounds: [lb (6) | ub (6)]
    elif kind == "repeated index":
        var[4, 3], code = var[4, 0], 3
    else:
        var[4, 5], code = N, 2
    pk.data, pk.var_index = data.reshape(pk.data.shape), var.reshape(pk.var_index.shape)
    return pk, 4, code


@pytest.mark.parametrize("kind", ["lb > ub", "repeated index", "index out of range"])
def test_input_errors_are_handled_on_the_device(kind):
    import torch
    bad, instance, code = faulty(kind)
    good = lexlsi.pack_batch(N, problems("bounds"))
    ba, bs = new_batch(good), new_batch(good)
    try:
        tb, tg = upload(bad), upload(good)
        with pytest.raises(capi.LexlsError) as sync_error:
            bs.run_device(tb["data"], tb["var_index"])
        assert f"instance {instance}:" in str(sync_error.value)
        out, status = sentinel_outputs(ba), torch.zeros(1, dtype=torch.int32, device=device())
        assert raw_enqueue(ba, tb, out, status) == 0
        with pytest.raises(capi.LexlsError) as e:
            ba.finish()
        assert str(e.value).startswith(f"liblexls_hip error {LEXLS_ERR_INVALID}:")
        assert str(e.value).split(": ", 1)[1] == str(sync_error.value).split(": ", 1)[1]  # the same instance and reason
        assert int(status.item()) == instance * 8 + code
        assert_sentinels(out, kind)
        solve_both(ba, bs, tg, "good data after " + kind)
    finally:
        ba.close()
        bs.close()


def test_refusals():
    import torch
    in_child("child_no_fused", limit=120, LEXLS_LSI_NO_FUSED="1")
    pk = lexlsi.pack_batch(N, problems("bounds"))
    b, t = new_batch(pk), upload(pk)
    try:
        out = sentinel_outputs(b)
        torch.cuda.synchronize()
        assert raw_enqueue(b, t, out, **CAP3) == LEXLS_ERR_UNSUPPORTED
        assert_sentinels(out, "d_lambda with cycling handling")
        bs = new_batch(pk)
        try:
            solve_both(b, bs, t, "the same run without d_lambda is served", lam=False, **CAP3)
        finally:
            bs.close()
        b.enqueue_device(t["data"], t["var_index"])
        for call in (b.stats, b.cycling_counters, b.lambda_array, b.working_set_log_arrays, lambda: b.run_device(t["data"], t["var_index"])):
            with pytest.raises(capi.LexlsError) as e:
                call()
            assert str(e.value).startswith(f"liblexls_hip error {LEXLS_ERR_INVALID}:"), str(e.value)
        b.finish()
        assert b.stats()["groups"] == 1 and b.lambda_array().shape == (7, 3, 15)
    finally:
        b.close()
