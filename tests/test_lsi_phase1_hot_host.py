"""The hot-start options of phase 1 as the device's setup kernel runs them (lexls_amd/csrc/lsi_phase1_setup.h: p1_hot_working_set, p1_rebuild_stamps,
p1_initial_v) on their own, on the host, against host LexLSI objects after begin() — and the activation order LexLSI rebuilds behind
formInitialWorkingSet.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "lexls_amd", "csrc")]


def build_and_run(tmp_path, name, extra):
    cxx = shutil.which("g++")
    exe = str(tmp_path / name)
    build = subprocess.run([cxx, *FLAGS, *extra, os.path.join(HERE, "lsi_phase1_hot_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    print(run.stdout[-4000:], run.stderr[-4000:])
    return run


def test_hot_start_functions_against_the_host_driver(tmp_path):
    """lsi_phase1_hot_check.cpp: all 16 combinations of the four options x with / without x0 x with / without v0 x with / without a guess, on a
    simple-bounds-first and a general-only hierarchy, capacity rows and ragged rows (absent rows hold NaN): every list, type, stamp, x, v, A x and
    the first equality problem against LexLSI after begin(); every branch of phase 1 taken; a hot-activated constraint removed under
    deactivate_first_wrong_sign through the rebuilt activation order"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    run = build_and_run(tmp_path, "lsi_phase1_hot_check", [])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "phase 1 hot start ok" in run.stdout


def test_hot_start_functions_under_address_and_undefined_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined (stand-alone, host only): the walk over the activation order and the erase stay
    inside the list"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"  # a program that cannot fail to compile: only missing sanitizer runtimes stop it
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("this g++ cannot build with -fsanitize=address,undefined: " + (can.stderr.strip().splitlines() or ["?"])[-1])
    run = build_and_run(tmp_path, "lsi_phase1_hot_check_san", san)
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "phase 1 hot start ok" in run.stdout
