"""The libraries next to libfedagg.so share one error header (csrc/lib_error.h), one loader
(substrafl_amd/_loader.py) and one build table (__graft_entry__.LIBRARIES).  Without a GPU: each
library's error text is its own, whatever flags the libraries are loaded with, and each thread's
is its own; the build table and the bindings name the same libraries.  Every call below is refused
before the library's first HIP call."""

import ctypes
import importlib
import os
import subprocess
import sys
import threading
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SATELLITES = ("dense", "promote", "mx", "mxef")
F32 = 1  # FEDAGG_F32
A, B, C = 0x100000, 0x200000, 0x300000  # never dereferenced


def open_all(mode: int) -> dict:
    """name -> a handle of the library opened with ``mode``, its binding's signatures bound."""
    libs = {}
    for name in SATELLITES:
        binding = importlib.import_module(f"substrafl_amd._native_{name}")
        lib = ctypes.CDLL(str(binding.LIB_PATH), mode=mode)
        for fn, (res, args) in binding.SIGNATURES.items():
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = res, args
        libs[name] = lib
    return libs


def last_errors(libs: dict) -> dict:
    return {name: getattr(lib, f"fedagg_{name}_last_error")() for name, lib in libs.items()}


# one refused call per library (two for libfedagg_mx.so) and a piece of the text it leaves
REFUSALS = [
    ("mx", lambda lib: lib.fedagg_mx_quantize(None, F32, 64, B, C, None), b"mx quantize: d_x is NULL"),
    ("mxef", lambda lib: lib.fedagg_mxef_quantize(None, F32, 64, A, B, C, None), b"mxef quantize: d_x is NULL"),
    ("mx", lambda lib: lib.fedagg_mx_fedavg_e4m3(None, None, None, 0, 64, None, 0, None, None),
     b"mx fedavg: K must be positive (K=0)"),
    ("dense", lambda lib: lib.fedagg_dense_potrf_f64(None, 4, 4, A, None), b"d_A is NULL"),
    ("promote", lambda lib: lib.fedagg_promote_tune(b"no_such_key", 0), b"promote tune: unknown key"),
]


def isolation_check(mode: int) -> None:
    """In a process that has not used the libraries yet: all four opened before any call, then after
    each refusal that library holds its text and the other three hold what they held, which is the
    empty string until their own first refusal."""
    libs = open_all(mode)
    held = last_errors(libs)
    assert held == dict.fromkeys(SATELLITES, b""), held
    for name, refuse, text in REFUSALS:
        assert refuse(libs[name]) == -1, text
        now = last_errors(libs)
        assert text in now[name], (name, now)
        held[name] = now[name]
        assert now == held, (name, now, held)
    assert len(set(held.values())) == len(SATELLITES)


@pytest.mark.parametrize("mode", ["RTLD_LOCAL", "RTLD_GLOBAL"])
def test_each_library_keeps_its_own_error_text(mode):
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import ctypes, test_satellite_libraries as t\n"
            "t.isolation_check(ctypes.%s)\n" % (str(ROOT), str(ROOT / "tests"), mode))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


# the same refusal with another value on each of two threads, through the shared fail(): name, call(lib, v), text(v)
PER_THREAD = [
    ("mx", lambda lib, v: lib.fedagg_mx_fedavg_e4m3(None, None, None, -v, 64, None, 0, None, None),
     lambda v: b"mx fedavg: K must be positive (K=-%d)" % v),
    ("mxef", lambda lib, v: lib.fedagg_mxef_quantize(A, 100 + v, 64, A, B, C, None),
     lambda v: b"mxef quantize: kind %d is not FEDAGG_F32 / FEDAGG_BF16" % (100 + v)),
    ("promote", lambda lib, v: lib.fedagg_promote_tune(b"vec", 1 + v),
     lambda v: b"promote tune: vec takes 0 or 1 (got %d)" % (1 + v)),
    ("dense", lambda lib, v: lib.fedagg_dense_potrf_f64(A, 8, v, B, None),
     lambda v: b"lda = %d is smaller than n" % v),
]


@pytest.mark.parametrize("name,call,text", PER_THREAD, ids=[p[0] for p in PER_THREAD])
def test_the_error_text_is_per_thread(name, call, text):
    lib = open_all(ctypes.RTLD_LOCAL)[name]
    both_refused = threading.Barrier(2)
    seen = {}

    def run(v):
        rc = call(lib, v)
        both_refused.wait(timeout=60)  # neither thread reads before both have written
        seen[v] = (rc, getattr(lib, f"fedagg_{name}_last_error")())

    threads = [threading.Thread(target=run, args=(v,)) for v in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert seen == {1: (-1, text(1)), 2: (-1, text(2))}


def test_the_build_table_and_the_bindings_name_the_same_libraries():
    """Every entry of ``__graft_entry__.LIBRARIES`` is the default ``LIB_PATH`` of exactly one binding
    module and every binding module has an entry (defaults: read without the FEDAGG_*_LIB variables)."""
    import __graft_entry__ as g

    bindings = sorted(p.stem for p in (ROOT / "substrafl_amd").glob("_native*.py"))
    assert "_native" in bindings and {f"_native_{s}" for s in SATELLITES} <= set(bindings)
    code = ("import sys, importlib; sys.path.insert(0, %r)\n"
            "for b in %r:\n"
            "    p = importlib.import_module('substrafl_amd.' + b).LIB_PATH\n"
            "    print(b, p.name, p.parent)\n" % (str(ROOT), bindings))
    env = {k: v for k, v in os.environ.items() if not (k.startswith("FEDAGG_") and k.endswith("LIB"))}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert all(parent == str(ROOT / "substrafl_amd") for _, _, parent in rows), rows
    assert sorted(name for _, name, _ in rows) == sorted(lib.name for lib in g.LIBRARIES)  # one to one
    assert len({lib.name for lib in g.LIBRARIES}) == len(g.LIBRARIES) == len(bindings)
    for lib in g.LIBRARIES:
        assert lib.srcs and all((ROOT / "substrafl_amd" / "csrc" / s).exists() for s in lib.srcs), lib
