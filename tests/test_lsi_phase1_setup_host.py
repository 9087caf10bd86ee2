"""The serial, order-defining part of phase 1 on the device (lexls_amd/csrc/lsi_phase1_setup.h: input checks, working-set lists, activation
stamps, the first equality problem's row references) on its own, on the host, against the host LexLSI driver.  No GPU needed."""
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
    build = subprocess.run([cxx, *FLAGS, *extra, os.path.join(HERE, "lsi_phase1_setup_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    print(run.stdout[-4000:], run.stderr[-4000:])
    return run


def test_setup_header_against_the_host_driver(tmp_path):
    """lsi_phase1_setup_check.cpp: general only, simple bounds first, rows with lb == ub (one with a zero normal, one within isEqual's tolerance),
    a simple bound with lb == ub, guesses that name active rows and carry EQ flags, with and without x0 — every list, type, stamp, count and
    row reference against LexLSI after runner::setup + begin(); each of the four input checks on the instance that has the fault"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    run = build_and_run(tmp_path, "lsi_phase1_setup_check", [])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "phase 1 setup ok" in run.stdout


def test_setup_header_under_address_and_undefined_sanitizers(tmp_path):
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
    run = build_and_run(tmp_path, "lsi_phase1_setup_check_san", san)
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "phase 1 setup ok" in run.stdout
