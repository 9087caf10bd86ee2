"""The cases of tests/device_input_cases.py on the CPU, from the oracle and the planner alone: each has the ranks its docstring states, and
the dispatch plan (lexls_amd/csrc/lexls_dispatch.h, through the stand-alone program tests/dispatch_plan_check.cpp and the query lines of
scripts/record_dispatch_table.py) reaches the kernel the case names for an input aligned to 16 bytes AND for one aligned to 8 bytes only.
tests/test_gpu_device_input.py asserts the same names on the device; a dispatch rule that moves fails here first.  No GPU needed."""
import atexit
import functools
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import device_input_cases as D
from scripts import record_dispatch_table as R

ROOT = D.ROOT
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "dispatch_plan_check.cpp")


@functools.lru_cache(maxsize=None)
def program():
    cxx = shutil.which("g++")
    assert cxx is not None, "the plan of the device-input cases needs g++"
    d = tempfile.mkdtemp(prefix="device_input_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "dispatch_plan_check")
    build = subprocess.run([cxx, *FLAGS, SOURCE, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def entry(name, align, ident):
    """the case as an entry of record_dispatch_table (its own capacities and dimensions): what the handle's query holds when the GPU test runs it"""
    c, case = D.CASES[name], D.draw(name)
    return dict(kind="lse", id=ident, caps=case["caps"], dims=case["dims"], n=c["n"], batch=c["batch"], policy=c["policy"], keep=c["keep"], mode="fs",
                fixed=int(bool(c.get("fixed"))), guard=0, reg=int(c.get("reg", 0)), qtol0=0, align8=int(align == 8))


@functools.lru_cache(maxsize=None)
def plans():
    """(case, align) -> the kernel name plan_lqr prints"""
    with open(R.TABLE) as f:
        cus = json.load(f)["cu_count"]  # the device the recorded table stands for: wave capacity = CUs x 8
    keys = [(nm, a) for nm in D.CASES for a in (16, 8)]
    lines = [R.query_line(entry(nm, a, i), cus) for i, (nm, a) in enumerate(keys)]
    run = subprocess.run([program()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = run.stdout.splitlines()
    assert len(out) == len(keys)
    got = {}
    for i, (key, line) in enumerate(zip(keys, out)):
        ident, kernel, *_ = line.split("|")
        assert int(ident) == i
        got[key] = kernel
    return got


@pytest.mark.parametrize("align", [16, 8])
@pytest.mark.parametrize("name", list(D.CASES))
def test_planner_reaches_the_named_kernel(name, align):
    print(f"{name} align {align}: {plans()[(name, align)]}")
    assert plans()[(name, align)] == D.kernel_at(name, align)


def test_only_the_tolerance_kernels_give_way_at_8_bytes():
    """the uniform lqr_qtol and lqr_mfma need 16 bytes and leave the shape to the bit-exact four-per-wavefront kernel; nothing else moves, the
    ragged lqr_qtol included"""
    moved = {nm for nm in D.CASES if plans()[(nm, 16)] != plans()[(nm, 8)]}
    assert moved == {"t_auto", "t_qtol", "t_mfma"}
    for nm in moved:
        assert plans()[(nm, 8)] == D.QS7 and D.contract_at(nm, 16) == "T" and D.contract_at(nm, 8) == "B"
    assert plans()[("ragged", 8)] == "lqr_qtol<3,12,shift 7,ragged>"


def test_every_family_that_reads_the_input_has_a_case():
    names = set(plans().values())
    want = {"lqr_quad<1,12>", "lqr_quad<2,12>", "lqr_quad<3,12>", "lqr_quad<3,12,shift 7>", "lqr_quad<4,16>", "lqr_quad<1,12,factor>", "lqr_quad<2,12,factor>",
            "lqr_quad<3,12,factor>", "lqr_quad<3,12,shift 7,factor>", "lqr_quad<4,16,factor>", "lqr_quad<3,12,shift 7,fixed>", "lqr_lwave<41,12>",
            "lqr_lwave<41,12,exact>", "lqr_wave<41,12,exact>", "lqr_wave<41,12>", "lqr_wave<64,16>", "lqr_wave<41,12,regularized>", "lqr_generic<64,lds>",
            "lqr_generic<256,lds>", "lqr_large<multi-launch>", "lqr_large<step-per-pivot,mfma>", "lqr_qtol<3,12,shift 7,ragged>", "lqr_qtol<3,12,shift 7>",
            "lqr_mfma<32,12,n40>"}
    assert want <= names, want - names
    assert all(5 <= c["batch"] <= 13 or nm.startswith("large") for nm, c in D.CASES.items())
    assert any(c["batch"] % 4 for c in D.CASES.values())  # a four-per-wavefront tail
    assert set(D.CONSUMER_CASES) <= {nm for nm, c in D.CASES.items() if c["keep"] and not c.get("fixed")}
    assert {D.CASES[nm]["kernel"].split("<")[0] for nm in D.CONSUMER_CASES} == {"lqr_wave", "lqr_quad", "lqr_generic"}


@pytest.mark.parametrize("name", list(D.CASES))
def test_ranks_are_what_the_docstring_says(name):
    case = D.build(name)
    print(D.summary(case))
    assert D.summary(case) in D.__doc__
    c, ref, B = D.CASES[name], case["ref"], len(case["lod"])
    short = D.deficient_problems(case)
    if c.get("deficient"):  # the last two problems lose ranks to exact dependences, the others do not
        assert short == [B - 2, B - 1]
        want = np.minimum(np.asarray(c["deficient"]), np.maximum(0, c["n"] - np.concatenate([[0], np.cumsum(c["deficient"])[:-1]])))
        for b in short:
            assert ref["rank"][b].tolist() == want.tolist()
    elif not c.get("ragged"):
        assert short == []
    if c.get("ragged"):
        assert set(np.unique(case["dims"]).tolist()) == set(range(13)) and (case["dims"].sum(axis=1) <= sum(c["caps"])).all()
        assert (case["dims"] != case["dims"][0]).any()
    if c.get("fixed"):
        np.testing.assert_array_equal(ref["fcol"][:, 0], case["fixed"]["nfixed"])
        assert case["fixed"]["nfixed"].min() == 0 and case["fixed"]["nfixed"].max() >= 3
    assert np.isfinite(ref["x"]).all()


@pytest.mark.parametrize("name", D.CONSUMER_CASES)
def test_consumer_references_are_not_zeros(name):
    """what the consumers are compared with: candidates found at some (problem, level) pairs and not at others, non-zero multipliers of at least
    two objectives, CORRECT_SIGN marks, a least-norm solution whose bits are not the basic one's"""
    case = D.build(name)
    c = case["consumers"]
    found = np.stack([s[:, 0] for s in c["sens"]])
    assert found.any() and not found.all()
    assert sum(1 for k in range(len(case["caps"])) if (c["mult"][:, k] != 0.0).any()) >= 2
    assert any((m != case["types"]).any() for m in c["marks"])
    assert (c["ln1"] != case["ref"]["x"]).any()  # (total rank n: the same solution by another routine, other bits)
    assert (np.abs(case["ref"]["v"]) > 1e-6).any()


def test_odd_leading_dimension_alternates_the_alignment():
    """cap x (n + 1) odd: problem b starts 8 b mod 16 bytes past the base"""
    for nm in ("oddld_w", "oddld_q"):
        c = D.CASES[nm]
        assert (sum(c["caps"]) * (c["n"] + 1)) % 2 == 1
    assert sum(1 for c in D.CASES.values() if sum(c["caps"]) % 2) >= 3  # odd capacities: columns of one problem alternate as well


def test_rebound_data_differs():
    """what the rebinding and stream tests put into the buffer next has another solution: a stale result cannot pass for the new one"""
    for nm in ("w41F", "q3s7_x", "g64", "q2_x", "oddld_q"):
        a, b = D.build(nm)["ref"]["x"], D.other_data(nm)["ref"]["x"]
        assert (np.abs(a - b).max(axis=1) > 1e-3).all(), nm
