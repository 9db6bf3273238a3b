"""The fp16 / bf16 kinds of the host value check (substrafl_amd/csrc/host_pool.h ``check_rows``:
what ``fedagg_session_stage_check`` runs on the pack workers for 16-bit copies of Scaffold's
server control variate, scaffold.py:193-196), as a stand-alone g++ program with planted differences
(tests/c/host_check16_test.cpp): plain, and under AddressSanitizer + UBSan, where a read past a
segment's end or a misaligned load is an error.  CPU only."""

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "c" / "host_check16_test.cpp"


@pytest.mark.parametrize("flags,env", [
    ([], {}),
    (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], {"ASAN_OPTIONS": "detect_leaks=1"}),
], ids=["plain", "asan_ubsan"])
def test_host_check16(tmp_path, flags, env):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "host_check16_test"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-pthread",
                    f"-I{ROOT / 'substrafl_amd' / 'csrc'}", str(SRC), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    run_env = dict(os.environ)
    run_env.update(env)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=run_env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "host_check16_test: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_host_pool_test_still_builds_with_its_esz_argument(tmp_path):
    """tests/c/host_pool_test.cpp calls ``check_rows(..., 4)``: the kind of 2-byte elements is an
    extra defaulted argument, so that call compiles unchanged."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    subprocess.run([gxx, "-std=c++17", "-O1", "-fsyntax-only", "-pthread", f"-I{ROOT / 'substrafl_amd' / 'csrc'}",
                    str(ROOT / "tests" / "c" / "host_pool_test.cpp")], check=True, capture_output=True, text=True)
