"""Regularized LexLSI batches with their active-set iterations resident on the device: the persistent launch whose l-QR is the regularized
body (lsi_fused<lqr_wave<...,regularized>>), the lock-step stages on lqr_wave<...,regularized> (LEXLS_LSI_NO_FUSED=1) and the host path
(LEXLS_LSI_RESIDENT=0, type 7, cycling handling).  The yardstick is the oracle-backed single-problem driver (oracle.lsi_run) and the
tolerance is zero everywhere: counters, x, the final working set and v compare with assert_array_equal — bit for bit is the contract of
every LexLSI path, so there is no number to choose."""
import numpy as np
import pytest

from lexls_amd import lexlsi, problems as P

pytestmark = pytest.mark.gpu

REG_TYPES = [1, 2, 3, 4, 5, 6, 8, 9]  # everything the REG instantiation of the register-resident kernel serves (7: host path, below)
SHAPES = {
    # the IK shape (BASELINE configs[2..4]): objective 0 = simple bounds, four general objectives of 12 rows
    "ik": dict(n=40, dims=[12] * 5, factors=[0, 0.02, 0.05, 0.03, 0.04], count=64, seed=20261000),
    # the batch of tests/test_gpu_lsi.py::test_lock_step_batch_with_regularization
    "small": dict(n=20, dims=[6, 5, 5, 6], factors=[0, 0.3, 0.2, 0.4], count=12, seed=700),
    # levels of up to 16 rows, 51 columns: the 64 x 16 instantiation
    "wide": dict(n=50, dims=[10, 16, 16, 14], factors=[0, 0.1, 0.2, 0.3], count=16, seed=20261500),
    # 57 columns: the shape of test_lds_fallback_to_the_stage_path
    "wide56": dict(n=56, dims=[10, 16, 16, 14], factors=[0, 0.1, 0.2, 0.3], count=16, seed=20261600),
    # 48 columns with levels of up to 12 rows: a plain batch of this shape runs the four-per-wavefront kernel behind a gather launch; there is
    # no regularized four-per-wavefront kernel, so the regularized batch takes the 64 x 16 instantiation
    "slot48": dict(n=47, dims=[8, 12, 12, 12], factors=[0, 0.1, 0.2, 0.3], count=16, seed=20261700),
}


def make(shape):
    s = SHAPES[shape]
    return s, [P.lsi_problem(s["seed"] + i, s["n"], s["dims"]) for i in range(s["count"])]


def oracle_refs(oracle, n, probs, factors, guesses=None, x0=None, v0=None, **params):
    return [oracle.lsi_run(n, p, active_guess=None if guesses is None else np.split(guesses[i], np.cumsum([len(o["lb"]) for o in p])[:-1]),
                           x0=None if x0 is None else x0[i], v0=None if v0 is None else v0[i], regularization_factors=factors, **params)
            for i, p in enumerate(probs)]


def assert_equals_oracle(r, refs):
    for b, o in enumerate(refs):
        assert r["info"][b] == o["info"], b  # status, iterations, activations, deactivations, factorizations, rank
        np.testing.assert_array_equal(r["x"][b], o["x"])
        np.testing.assert_array_equal(r["active"][b], np.concatenate(o["active"]))
        np.testing.assert_array_equal(r["v"][b], np.concatenate(o["v"]))


def assert_same_run(a, b):
    np.testing.assert_array_equal(a["info"].array, b["info"].array)
    for k in ("x", "active", "v"):
        np.testing.assert_array_equal(a[k], b[k])


def new_batch(probs, n):
    pk = lexlsi.pack_batch(n, probs)
    return lexlsi.LsiBatch(n, pk.dims, pk.types, len(probs)), pk


@pytest.mark.parametrize("shape", ["ik", "small"])
@pytest.mark.parametrize("reg_type", REG_TYPES)
def test_parity_on_the_persistent_launch(hip, oracle, shape, reg_type):
    s, probs = make(shape)
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, regularization_factors=s["factors"], regularization_type=reg_type)
    name = b.last_kernel()
    b.close()
    assert name.startswith("lsi_fused<") and "regularized" in name, name
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], regularization_type=reg_type))


@pytest.mark.parametrize("shape", ["wide", "slot48"])
def test_parity_64x16(hip, oracle, shape):
    """both shapes run the persistent launch: by the launchers' LDS rule (wave_reg_lds_bytes) the l-QR image of the 64 x 16 instantiation plus the
    regularization routines' vectors is 28,704 B for n = 50 with three LexLSE levels (48,768 B for the largest shape the kernel takes: n = 63,
    16 levels, a CG type), and the optional work matrix and null-space basis only enter below a 20 KB share — far from the launch's 64 KB"""
    s, probs = make(shape)
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, regularization_factors=s["factors"], regularization_type=1)
    name = b.last_kernel()
    b.close()
    assert name == "lsi_fused<lqr_wave<64,16,regularized>>"
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], regularization_type=1))


LDS_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_lsi_regularized_resident as T
s, probs = T.make("wide56")
b, pk = T.new_batch(probs, s["n"])
r = b.run(pk, regularization_factors=s["factors"], regularization_type=1)
name = b.last_kernel()
b.close()
np.savez({out!r}, x=r["x"], v=r["v"], active=r["active"], info=r["info"].array, name=np.array(name))
"""


def test_lds_fallback_to_the_stage_path(hip, oracle, tmp_path):
    """The fallback order of a regularized shape whose LDS need exceeds the persistent launch's 64 KB: the lock-step stages on
    lqr_wave<64,16,regularized>.  Unreachable with the default share of a CU's LDS (see test_parity_64x16); with LEXLS_REG_LDS_WAVES=1 (read
    once per process: a child process) the share is the whole 160 KB, so for n = 56, three levels, type 1, the work matrix (order
    n/2 + 16 + 1 = 45: 8 * 45^2 = 16,200 B) and the null-space basis (8 * 57 * 57 = 25,992 B) join the 31,920 B of image and vectors:
    74,112 B > 65,536 B.  (The last fallback, the host path beyond a workgroup's 160 KB, cannot be reached at all: the optional pieces
    never exceed the share and the rest is at most 48,768 B.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "run.npz")
    env = dict(os.environ, LEXLS_REG_LDS_WAVES="1")
    subprocess.run([sys.executable, "-c", LDS_CHILD.format(root=root, tests=os.path.join(root, "tests"), out=out)], env=env, cwd=root, check=True, timeout=300)
    z = np.load(out)
    assert str(z["name"]) == "lqr_wave<64,16,regularized>"
    s, probs = make("wide56")
    keys = ["status", "iterations", "activations", "deactivations", "factorizations", "total_rank"]
    r = dict(x=z["x"], v=z["v"], active=z["active"], info=[dict(zip(keys, row)) for row in z["info"].tolist()])
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], regularization_type=1))


def test_fused_decision_is_taken_per_run(hip, monkeypatch):
    """LEXLS_LSI_NO_FUSED is read per run (include/lexls_hip.h): a plain run under it takes the stages, the next one on the same object the
    persistent launch again; same results"""
    s, probs = make("ik")
    b, pk = new_batch(probs, s["n"])
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    staged = b.run(pk)
    assert not b.last_kernel().startswith("lsi_fused<") and b.last_kernel() != "host", b.last_kernel()
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")
    fused = b.run(pk)
    name = b.last_kernel()
    b.close()
    assert name.startswith("lsi_fused<") and "regularized" not in name, name
    assert_same_run(staged, fused)


def test_the_path_is_the_new_one(hip, oracle, monkeypatch):
    s, probs = make("ik")
    par = dict(regularization_factors=s["factors"], regularization_type=1)
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, **par)
    name, stats = b.last_kernel(), b.stats()
    assert name.startswith("lsi_fused<") and "regularized" in name, name
    longest = max(i["factorizations"] for i in r["info"])
    print(f"kernel {name}, longest instance {longest} factorizations, stats {stats}")
    assert stats["device_step"] >= longest - 1
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], regularization_type=1))

    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")  # (read per run)
    staged = b.run(pk, **par)
    assert b.last_kernel() == "lqr_wave<41,12,regularized>"
    assert_same_run(staged, r)
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")

    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")  # (read when the batch object is made)
    h, _ = new_batch(probs, s["n"])
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    host = h.run(pk, **par)
    assert h.last_kernel() == "host"
    h.close()
    assert_same_run(host, r)

    b.run(pk)
    plain = b.last_kernel()
    b.close()
    assert plain.startswith("lsi_fused<") and "41,12" in plain and "regularized" not in plain, plain


def three_paths(monkeypatch, probs, n, **run_args):
    b, pk = new_batch(probs, n)
    fused = b.run(pk, **run_args)
    assert b.last_kernel().startswith("lsi_fused<") and "regularized" in b.last_kernel()
    monkeypatch.setenv("LEXLS_LSI_NO_FUSED", "1")
    staged = b.run(pk, **run_args)
    assert b.last_kernel().startswith("lqr_wave<") and "regularized" in b.last_kernel()
    monkeypatch.delenv("LEXLS_LSI_NO_FUSED")
    b.close()
    monkeypatch.setenv("LEXLS_LSI_RESIDENT", "0")
    h, _ = new_batch(probs, n)
    monkeypatch.delenv("LEXLS_LSI_RESIDENT")
    host = h.run(pk, **run_args)
    assert h.last_kernel() == "host"
    h.close()
    assert_same_run(staged, fused)
    assert_same_run(host, fused)
    return fused


def test_three_paths_warm_start(hip, oracle, monkeypatch):
    """the configs[4] recipe (bench.py, side_config4_lsi): the perturbed neighbour from the cold solve's working set (equalities left to the
    driver) and x"""
    s = SHAPES["ik"]
    n, dims, count = s["n"], s["dims"], s["count"]
    base = [P.lsi_problem(s["seed"] + i, n, dims) for i in range(count)]
    pert = [P.lsi_problem(s["seed"] + i, n, dims, perturb=0.9) for i in range(count)]
    par = dict(regularization_factors=s["factors"], regularization_type=1)
    cold = lexlsi.lsi_batch_solve(n, base, **par)
    guess = np.where(cold["active"] == 3, 0, cold["active"]).astype(np.uint8)
    r = three_paths(monkeypatch, pert, n, active_guess=guess, x0=cold["x"], **par)
    assert_equals_oracle(r, oracle_refs(oracle, n, pert, s["factors"], guesses=guess, x0=cold["x"], regularization_type=1))


def test_three_paths_v0(hip, oracle, monkeypatch):
    s, probs = make("ik")
    v0 = [[0.01 * P.normal(900 + i, m, k) for k, m in enumerate(s["dims"])] for i in range(s["count"])]
    v0a = np.stack([np.concatenate(v) for v in v0])
    x0 = np.stack([0.1 * P.normal(950 + i, s["n"], 0) for i in range(s["count"])])  # (the driver takes v0 only next to an x0, lexlsi.h set_v0)
    r = three_paths(monkeypatch, probs, s["n"], x0=x0, v0=v0a, regularization_factors=s["factors"], regularization_type=3)
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], x0=x0, v0=v0, regularization_type=3))


def test_three_paths_factorization_limit(hip, oracle, monkeypatch):
    s, probs = make("ik")
    par = dict(regularization_type=1, max_number_of_factorizations=64)  # (a cold start of this batch takes 54 .. 83 and more)
    r = three_paths(monkeypatch, probs, s["n"], regularization_factors=s["factors"], **par)
    stopped = sum(i["status"] != 0 for i in r["info"])
    assert 0 < stopped < s["count"], "the limit must cut some instances short and let others finish"
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], **par))


def test_no_leakage_on_a_reused_batch_object(hip):
    s, probs = make("ik")
    n = s["n"]
    other = [0, 0.3, 0.01, 0.2, 0.05]
    b, pk = new_batch(probs, n)
    runs = [dict(), dict(regularization_factors=s["factors"], regularization_type=1), dict(regularization_factors=other, regularization_type=3), dict()]
    got, names = [], []
    for par in runs:
        got.append(b.run(pk, **par))
        names.append(b.last_kernel())
    b.close()
    assert [("regularized" in k) for k in names] == [False, True, True, False], names
    assert all(k.startswith("lsi_fused<") for k in names), names
    for par, r in zip(runs, got):
        assert_same_run(r, lexlsi.lsi_batch_solve(n, probs, **par))
    assert_same_run(got[3], got[0])
    assert np.abs(got[1]["x"] - got[0]["x"]).max() > 1e-6 and np.abs(got[2]["x"] - got[1]["x"]).max() > 1e-6  # (the factors do something)


def test_level_mapping(hip, oracle):
    """the same general objectives with and without a simple-bounds objective in front, all factors different: LexLSE level k takes the
    factor of objective k + 1 in the first batch and of objective k in the second"""
    s = SHAPES["ik"]
    n, count = s["n"], 16
    with_bounds = [P.lsi_problem(s["seed"] + 100 + i, n, s["dims"]) for i in range(count)]
    without = [p[1:] for p in with_bounds]
    f4 = [0.5, 0.002, 0.08, 0.03]
    for probs, factors in ((with_bounds, [0.0] + f4), (without, f4)):
        b, pk = new_batch(probs, n)
        r = b.run(pk, regularization_factors=factors, regularization_type=1)
        name = b.last_kernel()
        b.close()
        assert name.startswith("lsi_fused<") and "regularized" in name, name
        assert_equals_oracle(r, oracle_refs(oracle, n, probs, factors, regularization_type=1))


@pytest.mark.parametrize("par", [dict(regularization_type=7), dict(regularization_type=1, cycling_handling_enabled=1)], ids=["type7", "cycling"])
def test_what_stays_on_the_host(hip, oracle, par):
    s, probs = make("small")
    b, pk = new_batch(probs, s["n"])
    r = b.run(pk, regularization_factors=s["factors"], **par)
    name = b.last_kernel()
    b.close()
    assert name == "host"
    assert_equals_oracle(r, oracle_refs(oracle, s["n"], probs, s["factors"], **par))


@pytest.mark.parametrize("n", [22, 29])
@pytest.mark.parametrize("reg_type", [1, 3])
def test_three_paths_across_the_placement_of_the_routines_pieces(hip, oracle, monkeypatch, n, reg_type):
    """The persistent launch runs the regularized body with the placement lsi_fused_lds_bytes finds (wave_reg_lds_bytes behind its own carve-up):
    two LexLSE levels under a simple-bounds objective on the 41 x 12 shape, at n = 22, where the launcher of lqr_wave<41,12,regularized> keeps
    work matrix and null-space basis in LDS, and at n = 29, where type 1 keeps the window alone and type 3 loses its basis
    (tests/reg_cases.py, switch 1): persistent launch, stages and host path give the same bits, and the oracle-backed driver's"""
    dims, factors, count = [8, 8, 8] if n == 22 else [8, 12, 12], [0, 0.2, 0.3], 8  # (more rows than that at n = 22 and half of the instances cycle to the limit)
    probs = [P.lsi_problem(20281000 + 100 * n + i, n, dims) for i in range(count)]
    par = dict(regularization_factors=factors, regularization_type=reg_type)
    b, pk = new_batch(probs, n)
    b.run(pk, **par)
    assert b.last_kernel() == "lsi_fused<lqr_wave<41,12,regularized>>", b.last_kernel()
    b.close()
    r = three_paths(monkeypatch, probs, n, **par)
    refs = oracle_refs(oracle, n, probs, factors, regularization_type=reg_type)
    assert_equals_oracle(r, refs)
    plain = oracle_refs(oracle, n, probs, None)
    assert max(np.abs(o["x"] - p["x"]).max() for o, p in zip(refs, plain)) > 1e-6  # (the factors do something)
