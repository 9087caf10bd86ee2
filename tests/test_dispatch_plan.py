"""The dispatch plan (lexls_amd/csrc/lexls_dispatch.h) on its own, on the host: every entry of the recorded grid (tests/dispatch_table.json,
recorded through the public API on the commit before the plan existed) goes through plan_lqr and its sibling planners in a stand-alone
program, tests/dispatch_plan_check.cpp, and the names and properties it prints must account for the recorded observations entry for
entry.  No GPU needed."""
import json
import os
import shutil
import subprocess

import pytest

from scripts import record_dispatch_table as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc")]


def table():
    with open(R.TABLE) as f:
        return json.load(f)


def test_the_table_is_the_grid():
    """the recorded entries are grid()'s, in order: a changed grid needs a table recorded on the commit before the change"""
    assert [t["entry"] for t in table()["entries"]] == R.grid()


def observed(e, fields):
    """what the public API shows for entry e when the plan printed `fields`"""
    if e["kind"] == "lsi":
        fused, _, stage = fields
        return dict(kernel=stage if (not fused or "LEXLS_LSI_NO_FUSED" in e["env"]) else fused)
    name, props, _ = fields
    p = {x[0]: x[1] == "1" for x in props.split()}
    assert p["E"] == name.endswith(",guard>"), (e, name)  # the estimating bit drives the guard's compaction: exactly lqr_qtol's guard instantiations
    keep = e["keep"] if e["mode"] == "fs" else 1
    solve = "solve_generic<64>" if e["n"] + 1 <= 64 else ("solve_generic<256,reciprocal>" if p["C"] else "solve_generic<256>")
    consumer = solve if p["S"] else ""
    return dict(kernel=name, consumer=consumer, reuse_ready=int(p["R"] and bool(keep) and e["reg"] == 0),
                solve="error" if not p["H"] else (consumer if p["X"] else solve))


def check(tmp_path, name, extra):
    cxx = shutil.which("g++")
    exe = str(tmp_path / name)
    build = subprocess.run([cxx, *FLAGS, *extra, os.path.join(HERE, "dispatch_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    t = table()
    cus = t["cu_count"]
    entries = [R.resolve(x["entry"], cus) for x in t["entries"]]
    run = subprocess.run([exe], input="\n".join(R.query_line(e, cus) for e in entries) + "\n", capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(entries)
    wrong = []
    for e, x, line in zip(entries, t["entries"], lines):
        eid, *fields = line.split("|")
        assert int(eid) == e["id"]
        if x["expect"]["kernel"] == "host":  # (regularization type 7: the driver keeps the run on the host before any kernel is planned)
            assert e["kind"] == "lsi" and e["reg"] == 7
            continue
        got = observed(e, fields)
        if got != x["expect"]:
            wrong.append((e, x["expect"], got))
        if e["kind"] == "lse" and e["guard"] == 2 and "guard" in fields[0]:
            assert fields[2].startswith("lqr_quad<") and fields[2].endswith(",indirect>"), line  # the re-solve has a kernel
    assert not wrong, f"{len(wrong)} entries differ, first: {wrong[0]}"


def test_plan_reproduces_the_recorded_table(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    check(tmp_path, "dispatch_plan_check", [])


def test_plan_under_address_and_undefined_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined (stand-alone, host only)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"  # a program that cannot fail to compile: only missing sanitizer runtimes stop it
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("this g++ cannot build with -fsanitize=address,undefined: " + (can.stderr.strip().splitlines() or ["?"])[-1])
    check(tmp_path, "dispatch_plan_check_san", san)
