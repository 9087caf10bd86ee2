"""The worker pool of the lock-step LexLSI driver (lexls_amd/csrc/lsi_worker_pool.h) on its own, on the host, under ThreadSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")


def test_worker_pool_under_thread_sanitizer(tmp_path):
    """worker_pool_check.cpp: every index once (inline and pooled, 0 / 1 / 5 workers), thousands of back-to-back runs, runs after the
    workers went to sleep with and without prewake(), a light run that stays inline, exceptions, destruction while spinning / asleep."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "worker_pool_check")
    flags = ["-std=c++17", "-pthread", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "lexls_amd", "csrc")]
    probe = tmp_path / "probe.cpp"  # a program that cannot fail to compile: only a missing ThreadSanitizer runtime stops it
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([cxx, "-pthread", "-fsanitize=thread", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if can.returncode != 0:
        pytest.skip("this g++ cannot build with -fsanitize=thread: " + (can.stderr.strip().splitlines() or ["?"])[-1])
    build = subprocess.run([cxx, *flags, os.path.join(HERE, "worker_pool_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    print(run.stdout, run.stderr)
    assert "ThreadSanitizer" not in run.stderr, run.stderr
    assert run.returncode == 0, run.stderr
    assert "worker pool ok" in run.stdout
