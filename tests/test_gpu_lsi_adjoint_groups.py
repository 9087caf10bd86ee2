"""The LexLSI adjoints (lexls_lsi_batch_solve_adjoint(_multi)(_device), LsiBatch.jacobian_bounds_device) where the batch object's own
arithmetic decides what a cotangent meets, on the cases of tests/lsi_adjoint_cases.py:

    groups   LEXLS_LSI_GROUPS = 2 and 3 split the `ik` batch (8 instances: 4 + 4, 3 + 3 + 2) and the `budget` batch (6: 3 + 3, 2 + 2 + 2); group g
             works on rows lo[g] * nVar of g, lo[g] * ncot * nVar of G and lo[g] * total, lo[g] * ncot * total of the outputs.  An instance's
             gradients do not depend on its company, so every entry is bit-equal to the one-group run: plain, under two instance masks (each
             skips the whole of one group and part of another for one of the splits) and with instances stopped by the factorization budget
             in the groups' last positions.  The switch is read when a batch is created: the split runs are a child process each, under a time
             limit of its own, that writes its arrays for the parent to compare.
    forms    LEXLS_ADJOINT_MULTI_FORM (read by the launcher at every call) = hbm: the bits of the default run; = single: the bits of K calls of
             solve_adjoint_device.
    tile     lsi_adjoint_scatter_multi_kernel (the single call: ncot = 1) tiles the user rows by 1024: the `tile` case has 1036 and a working set on both sides of row 1024.
             Reference (A) of tests/lsi_adjoint_cases.py within its TOL, exact zeros everywhere else in both tiles."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch  # (before the HIP library loads: one process, one HIP runtime)

import lsi_adjoint_cases as LC
from lexls_amd import capi
from lexls_amd import problems as P
from test_gpu_lsi_adjoint import SENTINEL, rel, solve, upload
from test_gpu_lsi_adjoint_multi import assert_close_with_the_same_zeros, cotangents, device_form, host_form, single_calls

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DP = C.POINTER(C.c_double)
GROUPS_SWITCH, FORM_SWITCH = "LEXLS_LSI_GROUPS", "LEXLS_ADJOINT_MULTI_FORM"
# instance masks of the ik batch.  "a": 2 groups (0-3 | 4-7) — the whole of group 1 and part of group 0; 3 groups (0-2 | 3-5 | 6-7) — groups 1 and 2
# whole, part of group 0.  "b": 3 groups — the whole of group 1 and part of group 0, group 2 runs; 2 groups — part of either
MASKS = {"a": [1, 0, 1, 1, 0, 0, 0, 0], "b": [1, 1, 0, 0, 0, 0, 1, 1]}
KS = (3, 65)


def sizes(batch, groups):
    """the instances per group, as the batch object splits them"""
    return [batch // groups + (1 if g < batch % groups else 0) for g in range(groups)]


def adjoints(b, g, total):
    """every adjoint entry on the batch's last run, each into outputs that hold SENTINEL (the Jacobian: zeros) -> {name: array}"""
    out = {}
    g = np.ascontiguousarray(g)
    B = g.shape[0]
    lb, ub = np.full((B, total), SENTINEL), np.full((B, total), SENTINEL)
    capi.check(capi.lib().lexls_lsi_batch_solve_adjoint(b._h, g.ctypes.data_as(DP), lb.ctypes.data_as(DP), ub.ctypes.data_as(DP)))
    out["host_lb"], out["host_ub"] = lb, ub
    dev = b.solve_adjoint_device(torch.from_numpy(g).cuda(), *(torch.full((B, total), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)))
    out["device_lb"], out["device_ub"] = (t.cpu().numpy() for t in dev)
    for K in KS:
        G = cotangents(dict(g=g), K)
        out[f"multi{K}_host_lb"], out[f"multi{K}_host_ub"] = host_form(b, G, total)
        out[f"multi{K}_device_lb"], out[f"multi{K}_device_ub"] = device_form(b, G, total)
    out["jacobian_lb"], out["jacobian_ub"] = (t.cpu().numpy() for t in b.jacobian_bounds_device())
    return out


def collect():
    """the ik batch plain and under the two masks, the budget batch cold with max_number_of_factorizations = 1 -> {name: array}, in whatever
    number of groups this process's environment asks for"""
    from lexls_amd import lexlsi
    out = {}
    for name, c, params in (("ik", LC.CASES["ik"], {}), ("budget", LC.BUDGET, dict(max_number_of_factorizations=1))):
        n, probs = c["n"], LC.problems_of(name)
        g = P.normal(c["seed"] + 900, len(probs) * n).reshape(len(probs), n)
        pk = lexlsi.pack_batch(n, probs)
        data, var = upload(pk)
        b = lexlsi.LsiBatch(n, pk.dims, pk.types, pk.batch)
        runs = {name: None}
        if name == "ik":
            runs.update({f"ik_mask_{key}": mask for key, mask in MASKS.items()})
        for run, mask in runs.items():
            b.set_instance_mask(None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).cuda())
            r = b.run_device(data, var_index=var, **params)
            torch.cuda.synchronize()
            out[f"{run}.groups"] = np.asarray(b.stats()["groups"])
            for k in ("x", "active", "info"):
                out[f"{run}.{k}"] = r[k].cpu().numpy()
            for k, a in adjoints(b, g, pk.total).items():
                out[f"{run}.{k}"] = a
        b.set_instance_mask(None)
        b.close()
    return out


def child_collect(path):
    np.savez(path, **collect())


def in_child(call, limit=120, **env):
    """a function of this file in a fresh process (nothing replaces its program) with `env` on top of this one's, under a time limit"""
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_lsi_adjoint_groups as m; m.{call}"
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]


_one_group = {}


def one_group(monkeypatch):
    """collect() in this process with the switch unset: one group.  Computed once, shared, never modified"""
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    if not _one_group:
        _one_group.update(collect())
        for a in _one_group.values():
            a.setflags(write=False)
    return _one_group


def test_the_one_group_run_is_the_reference(hip, monkeypatch):
    """what the split runs are compared with is itself held to reference (A), and the masks and the budget do what the comparison relies on"""
    ref = one_group(monkeypatch)
    case, bd = LC.build("ik"), LC.build_budget()
    for run, c in (("ik", case), ("budget", bd)):
        assert int(ref[f"{run}.groups"]) == 1
        np.testing.assert_array_equal(ref[f"{run}.active"], c["active"])
        np.testing.assert_array_equal(ref[f"{run}.info"][:, 0], c["status"])
        for w, side in enumerate(("lb", "ub")):
            assert rel(ref[f"{run}.host_{side}"], c["A"][w]) <= LC.TOL
            np.testing.assert_array_equal(ref[f"{run}.device_{side}"], ref[f"{run}.host_{side}"])
            for K in KS:
                assert rel(ref[f"{run}.multi{K}_host_{side}"][:, 0], c["A"][w]) <= LC.TOL  # cotangent 0 is the case's g
                np.testing.assert_array_equal(ref[f"{run}.multi{K}_device_{side}"], ref[f"{run}.multi{K}_host_{side}"])
            assert not (ref[f"{run}.multi65_host_{side}"] == SENTINEL).any()
    for key, mask in MASKS.items():
        skipped = np.asarray(mask) == 0
        for k in (k for k in ref if k.startswith(f"ik_mask_{key}.") and k.split(".")[1][:4] in ("host", "devi", "mult", "jaco")):
            plain = ref["ik." + k.split(".")[1]]
            np.testing.assert_array_equal(ref[k][~skipped], plain[~skipped], err_msg=k)
            assert (ref[k][skipped] == (0.0 if "jacobian" in k else SENTINEL)).all(), k  # a skipped instance's rows keep the caller's bits
    stopped = bd["status"] != LC.SOLVED
    for groups in (2, 3):  # the budget stops the instance in the last position of a group (of every group, with three)
        last = np.cumsum(sizes(len(stopped), groups)) - 1
        assert stopped[last].any() and (groups == 2 or stopped[last].all())
    assert not ref["budget.multi65_host_ub"][stopped].any() and np.abs(ref["budget.multi65_host_ub"][~stopped]).max() > 1e-3
    # each mask skips the whole of one group and part of another for one of the splits
    for key, groups in (("a", 2), ("b", 3)):
        m, lo = np.asarray(MASKS[key]), np.concatenate([[0], np.cumsum(sizes(8, groups))])
        per_group = [m[lo[i]:lo[i + 1]] for i in range(groups)]
        assert any(not p.any() for p in per_group) and any(p.any() and not p.all() for p in per_group), key


@pytest.mark.parametrize("groups", [2, 3])
def test_split_into_groups_every_adjoint_is_the_one_group_run_bit_for_bit(hip, monkeypatch, tmp_path, groups):
    ref = one_group(monkeypatch)
    path = str(tmp_path / "groups.npz")
    in_child(f"child_collect({path!r})", **{GROUPS_SWITCH: str(groups)})
    with np.load(path) as z:
        got = {k: z[k] for k in z.files}
    assert set(got) == set(ref)
    for k in ref:
        if k.endswith(".groups"):
            assert int(got[k]) == groups, (k, int(got[k]))  # stats()["groups"] of every run
        else:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{groups} groups: {k}")


@pytest.mark.parametrize("name", ["ik", "small_sb"])
def test_the_forms_of_the_multi_cotangent_launcher(hip, monkeypatch, name):
    """hbm: the same dfma chains as the default (staged) form, so its bits; single: solve_adjoint<64> itself once per cotangent, so the bits of K
    calls of solve_adjoint_device"""
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    case = LC.build(name)
    b, _, active, _, status = solve("run_device", case["probs"], case["n"])
    np.testing.assert_array_equal(active, case["active"])
    total = active.shape[1]
    sets = {K: cotangents(case, K) for K in KS}
    base = {K: host_form(b, G, total) for K, G in sets.items()}
    singles = {K: single_calls(b, G) for K, G in sets.items()}
    for K in KS:
        assert rel(base[K][0][:, 0], case["A"][0]) <= LC.TOL and rel(base[K][1][:, 0], case["A"][1]) <= LC.TOL
        assert_close_with_the_same_zeros(base[K], singles[K], f"{name}, default form, K = {K}")
    if name == "ik":  # the default form sums in another order than the single-cotangent kernel: equal bits below show that the switch was followed
        assert any(not np.array_equal(base[K][w], singles[K][w]) for K in KS for w in (0, 1))
    for form, want in (("hbm", base), ("single", singles)):
        monkeypatch.setenv(FORM_SWITCH, form)
        for K, G in sets.items():
            for how, got in (("host", host_form(b, G, total)), ("device", device_form(b, G, total))):
                for w in (0, 1):
                    np.testing.assert_array_equal(got[w], want[K][w], err_msg=f"{name}, {form} forced, K = {K}, {how} form, {('grad_lb', 'grad_ub')[w]}")
    monkeypatch.delenv(FORM_SWITCH)
    again = host_form(b, sets[65], total)
    np.testing.assert_array_equal(again[0], base[65][0]), np.testing.assert_array_equal(again[1], base[65][1])
    b.close()


def test_the_second_tile_of_the_scatter_kernels(hip, monkeypatch):
    """1036 user rows: the scatter kernels go round their tile loop twice, with rows of the working set in both tiles"""
    monkeypatch.delenv(FORM_SWITCH, raising=False)
    monkeypatch.delenv(GROUPS_SWITCH, raising=False)
    tl = LC.build_tile()
    t0 = time.perf_counter()
    b, _, active, _, status = solve("run", tl["probs"], tl["n"])
    print(f"tile: run() took {time.perf_counter() - t0:.2f} s on {b.last_kernel()}")
    np.testing.assert_array_equal(active, tl["active"])
    np.testing.assert_array_equal(status, tl["status"])
    total = active.shape[1]
    assert total == 1036 > LC.ADJ_TILE
    ra, rb = tl["A"]
    inactive_lb, inactive_ub = active != LC.LB, (active != LC.UB) & (active != LC.EQ)
    glb, gub = b.solve_adjoint(tl["g"])
    print(f"tile: solve_adjoint against (A) {max(rel(glb, ra), rel(gub, rb)):.2e} (TOL {LC.TOL:.0e})")
    assert rel(glb, ra) <= LC.TOL and rel(gub, rb) <= LC.TOL
    assert not glb[inactive_lb].any() and not gub[inactive_ub].any()  # exact zeros everywhere else, in both tiles
    for u in (4 + r for r in LC.TILE["equalities"]):  # the two equalities, on either side of user row 1024
        assert (np.abs(gub[:, u]) > 1e-3).all(), u
    dlb, dub = b.solve_adjoint_device(torch.from_numpy(tl["g"].copy()).cuda())
    np.testing.assert_array_equal(dlb.cpu().numpy(), glb), np.testing.assert_array_equal(dub.cpu().numpy(), gub)
    G = cotangents(tl, 3)
    got = host_form(b, G, total)
    print(f"tile: solve_adjoint_multi, cotangent 0 against (A) {max(rel(got[0][:, 0], ra), rel(got[1][:, 0], rb)):.2e}")
    assert rel(got[0][:, 0], ra) <= LC.TOL and rel(got[1][:, 0], rb) <= LC.TOL
    assert_close_with_the_same_zeros(got, single_calls(b, G), "tile, K = 3")
    for c in range(3):
        assert not got[0][:, c][inactive_lb].any() and not got[1][:, c][inactive_ub].any()
        for u in (4 + r for r in LC.TILE["equalities"]):
            assert (np.abs(got[1][:, c, u]) > 1e-6).all(), (c, u)
    dev = device_form(b, G, total)
    np.testing.assert_array_equal(dev[0], got[0]), np.testing.assert_array_equal(dev[1], got[1])
    b.close()
