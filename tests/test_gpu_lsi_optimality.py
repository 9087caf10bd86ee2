"""Every batched LexLSI path certified as lexicographically optimal, by tests/lexopt.py: from the problem data and the returned x alone, without
this project's driver.  The other LSI tests compare the GPU paths bit for bit with oracle.lsi_run, the oracle-backed instantiation of the same
driver template; a mistake that the host restatement and its device form share passes all of them, and fails here.

Each fixture family of tests/test_lexopt_certificate.py (6-8 instances; that module validates the certificate and the acceptance bounds on the
CPU, and checks that every instance ends with status 0) runs through each path:

  default            the persistent launch (lsi_fused<...>; 46 columns: the stage path behind the gather launch), with the multipliers of lambdas()
  no_fused           LEXLS_LSI_NO_FUSED=1: three launches per stage
  host               LEXLS_LSI_RESIDENT=0: the active-set logic on the host
  first_wrong_sign   deactivate_first_wrong_sign, with the multipliers of lambdas()
  cycling            cycling_handling_enabled on these random inputs; every cycling counter must be zero, so the bounds are the caller's
  warm, warm_v0      from a neighbouring problem's working set / x (right-hand sides perturbed by 0.05), without and with its v as v0
  run_device         LsiBatch.run_device: problem and results in device memory
  run_device_v0_lambda   run_device(..., v0=, with_lambda=True): the returned multipliers are checked directly
  device_phase1      LEXLS_LSI_DEVICE_PHASE1=1

and asserts status 0 for every instance (none is skipped or filtered), the kernel that served the run where its name is known, the
certificate (lexopt.ACCEPT), the consistency of v and the working set with x, and the returned multipliers where there are any.

Shapes: n = 40, 5 x 12 with simple bounds (lqr_wave<41,12> at full width); n = 20, (6, 5, 5, 6) with simple bounds; n = 12, (4, 5, 4, 6) general
only, also with a row duplicated across two levels (rank deficiency) and with a level 0 that cannot be met; n = 57 with levels of 16 rows (the
64 x 16 instantiation); n = 45, 5 x 12 (46 columns).

Out of scope: regularized runs (they solve a damped problem), degenerate inputs whose bounds the cycling handler really relaxes (the relaxed
bounds are not returned), runs that stop on the factorization limit.

What the cases on n = 20, (6, 5, 5, 6) can and cannot show: that shape has 16 general rows for 20 variables, every level is met
exactly, every gradient and multiplier is zero and ANY feasible point is optimal.  Its ten cases therefore check feasibility, status, kernel and
the consistency of v and the working set with x, and little more; the other six families have a last level that cannot be met, so x is pinned.

What the path names do not show: nothing reports whether phase 1 ran on the device.  run_device has no other way; LEXLS_LSI_DEVICE_PHASE1=1 is
honoured for resident runs without v0 (lsi_batch.h), which "device_phase1" is, but no name or counter says so — as in tests/test_gpu_lsi_device_entry.py,
the evidence is that the results are right.

Known defect: deactivate_first_wrong_sign with simple bounds leaves four instances (test_lexopt_certificate.FIRST_WRONG_SIGN_NOT_OPTIMAL) at a point
that is not optimal, with status 0.  Those four are asserted to be REJECTED by the certificate, with the figure the oracle-backed driver gives; status,
kernel and consistency are asserted for them as for all others, and every other instance of their batches must certify."""
import numpy as np
import pytest

import lexopt
import test_lexopt_certificate as F
from lexls_amd import lexlsi

pytestmark = pytest.mark.gpu

PATHS = ["default", "no_fused", "host", "first_wrong_sign", "cycling", "warm", "warm_v0", "run_device", "run_device_v0_lambda", "device_phase1"]
_packed = {}


def packed(name):
    if name not in _packed:
        _packed[name] = lexlsi.pack_batch(F.FAMILIES[name]["n"], F.problems_of(name))
    return _packed[name]


def to_device(pk, guess=None, x0=None, v0=None):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)
    return dict(data=up(pk.data, np.float64), var_index=None if pk.var_index is None else up(pk.var_index.view(np.int32), np.int32),
                active_guess=up(guess, np.uint8), x0=up(x0, np.float64), v0=up(v0, np.float64))


def expected_kernel(name, path, kernel):
    if path == "host":
        assert kernel == "host", kernel
    elif path == "no_fused" or name == "cols46":  # (42..48 columns never take the persistent launch)
        assert not kernel.startswith("lsi_fused<") and kernel not in ("host", ""), kernel
    elif name == "wide":
        assert kernel == "lsi_fused<lqr_wave<64,16>>", kernel
    elif name == "ik":
        assert kernel.startswith("lsi_fused<lqr_wave<41,12"), kernel
    else:
        assert kernel.startswith("lsi_fused<"), kernel


def certify(name, r, lam=None, what="", not_optimal=()):
    """r: x / info / active / v of a batch run as host arrays; not_optimal: instances the run is known to leave at a non-optimal point"""
    f, probs = F.FAMILIES[name], F.problems_of(name)
    info = r["info"].array if hasattr(r["info"], "array") else np.asarray(r["info"])
    assert info.shape[0] == len(probs)
    assert not info[:, 0].any(), (what, "status", info[:, 0])
    worst = 0.0
    for b, p in enumerate(probs):
        lexopt.assert_consistent(lexopt.consistent(f["n"], p, r["x"][b], r["active"][b], r["v"][b]), (what, b))
        if b in not_optimal:
            F.assert_not_optimal(name, b, p, r["x"][b], r["active"][b], None if lam is None else lam[b], what)
            continue
        t = lexopt.certificate(f["n"], p, r["x"][b])
        worst = max(worst, float(t.max()))
        assert t.max() <= lexopt.ACCEPT, (what, b, t)
        if lam is not None:
            lexopt.assert_lambda(lexopt.lambda_check(f["n"], p, r["x"][b], r["active"][b], lam[b]), (what, b))
    print(what, ": largest certificate", worst)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_path_returns_the_lexicographic_optimum(hip, oracle, monkeypatch, name, path):
    pk, what = packed(name), f"{name} / {path}"
    for env in ("LEXLS_LSI_NO_FUSED", "LEXLS_LSI_RESIDENT", "LEXLS_LSI_DEVICE_PHASE1"):
        monkeypatch.delenv(env, raising=False)
    if path == "no_fused":
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    elif path == "host":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    elif path == "device_phase1":
        monkeypatch.setenv("LEXLS_LSI_DEVICE_PHASE1", "1")  # (read per run)
    params = dict(F.RUN_MODES.get(path, {}))
    guess = x0 = v0 = None
    if path in ("warm", "warm_v0", "run_device_v0_lambda"):
        guess, x0, v0 = F.warm_start_of(oracle, name)
        if path == "warm":
            v0 = None
    lam = None
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    try:
        if path.startswith("run_device"):
            t = to_device(pk, guess, x0, v0)
            out = b.run_device(t["data"], t["var_index"], t["active_guess"], t["x0"], v0=t["v0"], with_lambda=path == "run_device_v0_lambda")
            r = {k: a.cpu().numpy() for k, a in out.items()}
            if "lambda" in r:
                lam = [np.ascontiguousarray(m.T) for m in r["lambda"]]  # (nObj, total) per instance -> (total, nObj)
        else:
            r = b.run(pk, active_guess=guess, x0=x0, v0=v0, **params)
            if path in ("default", "first_wrong_sign"):
                lam = b.lambdas()
        kernel = b.last_kernel()
        if path == "cycling":
            assert not b.cycling_counters().any(), (what, b.cycling_counters())  # nothing was relaxed: the bounds are the caller's
    finally:
        b.close()
    expected_kernel(name, path, kernel)
    certify(name, r, lam, what, F.not_optimal(name, path))
