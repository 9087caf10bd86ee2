"""The large path's host-side plan (lexls_amd/csrc/lqr_large_plan.h) as the tests read it: tests/large_plan_check.cpp is built with g++ (as
tests/test_dispatch_plan.py builds dispatch_plan_check.cpp), run once per set of shapes, and its output parsed.  constants() is the ONLY
source of the kernels' shape constants for the Python tests: nothing here or in the tests repeats a value of the header."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lexls_amd", "csrc")]
SOURCE = os.path.join(ROOT, "tests", "large_plan_check.cpp")


def compile_check(exe, extra=()):
    cxx = shutil.which("g++")
    assert cxx is not None, "tests of the large path's plan need g++"
    build = subprocess.run([cxx, *FLAGS, *extra, SOURCE, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@functools.lru_cache(maxsize=None)
def program():
    d = tempfile.mkdtemp(prefix="large_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return compile_check(os.path.join(d, "large_plan_check"))


def shape_line(i, batch, n, cap, rows_max, level_max):
    return " ".join(str(int(v)) for v in [i, batch, n, cap, rows_max, len(level_max), *level_max])


def _pairs(tokens):
    return {tokens[i]: int(tokens[i + 1]) for i in range(0, len(tokens), 2)}


def run(lines, exe=None):
    """(constants, shapes): constants name -> value; per shape line dict(maxdim, layout: piece -> offset, clear: (begin, end), Gmax, colld,
    total, lds, fields_fit, forms: (nw, cpw) -> dict, levels: list of dict)"""
    r = subprocess.run([exe or program()], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    cut = out.index("--")
    consts = {name: int(v) for name, v in (ln.rsplit(" ", 1) for ln in out[:cut])}
    shapes = []
    for ln in out[cut + 1:]:
        t = ln.split()
        if t[0] == "shape":
            shapes.append(dict(id=int(t[1]), maxdim=int(t[3]), forms={}, levels=[]))
        elif t[0] == "layout":
            shapes[-1]["layout"] = _pairs(t[1:])
        elif t[0] == "clear":
            shapes[-1].update(clear=(int(t[1]), int(t[2])), **_pairs(t[3:]))
        elif t[0] == "lds":
            shapes[-1]["lds"] = _pairs(t[1:])
        elif t[0] == "form":
            shapes[-1]["forms"][(int(t[1]), int(t[2]))] = _pairs(t[3:])
        elif t[0] == "level":
            d = _pairs(t[:10])
            d.update(gemm_grid=(int(t[11]), int(t[12])), level_end_grid=int(t[14]))
            shapes[-1]["levels"].append(d)
        else:
            raise AssertionError(ln)
    assert len(shapes) == len(lines)
    return consts, shapes


@functools.lru_cache(maxsize=None)
def constants():
    return run([])[0]
