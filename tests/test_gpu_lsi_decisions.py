"""The decisions of the resident LexLSI iterations — the tie-break of the ratio test, the four tolerances, num / den on data in other units, row
kinds a middle level never held — against the oracle-backed driver, on the batches of tests/lsi_decision_cases.py (that module has the
generators, the seeds and the measured table; tests/test_lsi_decision_cases.py asserts on the CPU that the batches hold what is relied on here:
the twins tie, every parameter set changes decisions, the scaled runs end solved or at the factorization limit as stated).

Every instance is compared, whatever its status; none is filtered out.  With the working-set log on (256 entries per instance) the log is compared
first, entry for entry, so that a failure names the first decision that went another way; then info (status, iterations, activations,
deactivations, factorizations, rank), x, the working set and v with assert_array_equal.  The tolerance is zero, as on every LexLSI path.

One test is one (family, shape, path), a batch of 8:
  default       the persistent launch (46 columns: the stage path behind the gather launch)
  no_fused      LEXLS_LSI_NO_FUSED=1: three launches per stage
  host          LEXLS_LSI_RESIDENT=0: the active-set logic on the host
  run_device    LsiBatch.run_device: phase 1 on the device
and for twins also
  first_wrong_sign   deactivate_first_wrong_sign
  warm          working set and x of the neighbour (right-hand sides perturbed by 0.05): the inactive lists start in another order
  lambdas       lambdas() after the default run, bit for bit the single-problem debug output — also where the final problem holds both twins

last_kernel() is asserted wherever test_gpu_lsi_optimality.expected_kernel knows the name (general, ik, wide, cols46; host and no_fused on every
shape); what `tall` reports on the other paths is printed and stated in tests/lsi_decision_cases.py."""
import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime — run_device hands torch tensors to the library)

import lsi_decision_cases as D
from lexls_amd import capi, lexlsi
from test_gpu_lsi_optimality import expected_kernel, to_device

pytestmark = pytest.mark.gpu

PATHS = ["default", "no_fused", "host", "run_device"]
TWIN_PATHS = ["first_wrong_sign", "warm", "lambdas"]
CASES = [(family, shape, path) for family in D.FAMILIES for shape in D.SHAPES for path in PATHS + (TWIN_PATHS if family == "twins" else [])]
FIELDS = capi.WORKING_SET_LOG_FIELDS
_packed = {}


def packed(family, shape):
    if (family, shape) not in _packed:
        _packed[family, shape] = lexlsi.pack_batch(D.SHAPES[shape]["n"], D.problems(family, shape))
    return _packed[family, shape]


def assert_logs(arrays, refs, what):
    log, alpha, counts = arrays
    assert log.shape == (len(refs), D.LOG_CAPACITY, len(FIELDS))
    for b, o in enumerate(refs):
        got = [dict(alpha_or_lambda=float(a), **{k: int(f) for k, f in zip(FIELDS, e)}) for e, a in zip(log[b, :int(counts[b])], alpha[b, :int(counts[b])])]
        for i, (g, w) in enumerate(zip(got, o["log"])):
            assert g == w, f"{what}, instance {b}: decision {i} of {len(o['log'])} went another way: device {g}, oracle {w}"
        assert int(counts[b]) == len(o["log"]), (what, b, int(counts[b]), len(o["log"]))
        assert not log[b, len(got):].any() and not alpha[b, len(got):].any(), (what, b)


def assert_results(r, refs, what):
    info = np.asarray(r["info"].array if hasattr(r["info"], "array") else r["info"])
    for b, o in enumerate(refs):
        np.testing.assert_array_equal(info[b], [o["info"][k] for k in lexlsi.INFO_KEYS], err_msg=f"{what}, instance {b}: info")
        np.testing.assert_array_equal(r["x"][b], o["x"], err_msg=f"{what}, instance {b}: x")
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]), err_msg=f"{what}, instance {b}: working set")
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]), err_msg=f"{what}, instance {b}: v")


@pytest.mark.parametrize("family,shape,path", CASES, ids=["-".join(c) for c in CASES])
def test_decisions_are_the_oracles(hip, oracle, monkeypatch, family, shape, path):
    what = f"{family} / {shape} / {path}"
    for env in ("LEXLS_LSI_NO_FUSED", "LEXLS_LSI_RESIDENT", "LEXLS_LSI_DEVICE_PHASE1"):
        monkeypatch.delenv(env, raising=False)
    if path == "no_fused":
        monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    elif path == "host":
        monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    mode = path if path in ("first_wrong_sign", "warm") else "cold"
    refs = D.refs(family, shape, mode)
    params = dict(D.MODES[mode], **D.params_of(family))
    guess, x0 = D.warm_start(family, shape) if path == "warm" else (None, None)
    pk, lam = packed(family, shape), None
    b = lexlsi.LsiBatch(pk.nvar, pk.dims, pk.types, pk.batch)
    try:
        b.set_working_set_log(D.LOG_CAPACITY)
        if path == "run_device":
            t = to_device(pk)
            r = {k: a.cpu().numpy() for k, a in b.run_device(t["data"], t["var_index"], **params).items()}
        else:
            r = b.run(pk, active_guess=guess, x0=x0, **params)
        kernel, arrays = b.last_kernel(), b.working_set_log_arrays()
        if path == "lambdas":
            lam = b.lambdas()
    finally:
        b.close()
    print(what, ": kernel", kernel, " statuses", [o["info"]["status"] for o in refs], " log entries", [len(o["log"]) for o in refs])
    if shape != "tall" or path in ("host", "no_fused"):
        expected_kernel(shape, path, kernel)
    assert_logs(arrays, refs, what)
    assert_results(r, refs, what)
    if lam is not None:
        both = 0
        for i, (g, o) in enumerate(zip(lam, refs)):
            for k, (got, want) in enumerate(zip(g, o["debug"]["lambda"])):
                np.testing.assert_array_equal(got, want, err_msg=f"{what}, instance {i}, objective {k}")
            both += sum(o["active"][ka][ra] != 0 and o["active"][kb][rb] != 0 for (ka, ra), (kb, rb) in D.pairs_of(shape).values())
        print(what, ": pairs with both rows in the final working set", both)
