"""The installable package (VERDICT r04 "Next 2"): ``pip wheel`` runs the build hook (setup.py ->
``__graft_entry__.compile_entry`` over ``LIBRARIES``), so the wheel carries ``libfedagg.so`` and
every other library of that table for gfx950; without
hipcc the build fails loudly; the reference's own ``Dependency`` machinery accepts the repo and
ships that wheel (tests/reference_dependency.py, container only).  No GPU: nothing is launched,
the installed library is only loaded and its ABI version read."""

import json
import os
import shutil
import subprocess
import sys
import zipfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HERE = Path(__file__).resolve().parent

needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()),
                                 reason="needs hipcc (the build hook compiles for gfx950)")


def _pip_wheel(dest, env=None):
    return subprocess.run([sys.executable, "-m", "pip", "wheel", "--no-deps", "--no-build-isolation", "--no-index",
                           "--wheel-dir", str(dest), str(ROOT)], capture_output=True, text=True, timeout=900,
                          env=env)


@pytest.fixture(autouse=True, scope="module")
def _no_build_leftovers():
    """setuptools builds a local directory in place (``build/``, ``*.egg-info``): whatever these
    tests create there is removed afterwards, so no second copy of the package stays in the tree."""
    made = [d for d in (ROOT / "build", ROOT / "substrafl_amd.egg-info") if not d.exists()]
    yield
    for d in made:
        shutil.rmtree(d, ignore_errors=True)


@needs_hipcc
def test_wheel_carries_the_library_and_installs(tmp_path):
    r = _pip_wheel(tmp_path / "w")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    (whl,) = (tmp_path / "w").glob("substrafl_amd-*.whl")
    assert not whl.name.endswith("none-any.whl")  # a platform wheel: it holds a gfx950 binary
    names = zipfile.ZipFile(whl).namelist()
    assert any(n.endswith("substrafl_amd/libfedagg.so") for n in names)
    import __graft_entry__

    for lib in __graft_entry__.LIBRARIES:  # every library of the build table, or a binding finds nothing to load
        assert any(n.endswith("substrafl_amd/" + lib.name) for n in names), lib.name
    assert len(__graft_entry__.LIBRARIES) >= 5
    assert any(n.endswith("substrafl_amd/algorithms/accelerate.py") for n in names)
    assert not any("tuning" in n or n.endswith(".o") for n in names)
    r = subprocess.run([sys.executable, "-m", "pip", "install", "--no-deps", "--no-index", "--target",
                        str(tmp_path / "site"), str(whl)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # the installed copy, from a directory where the repo is not importable
    code = ("import substrafl_amd, substrafl_amd._native as n; "
            "print(substrafl_amd.__file__, n.LIB_PATH, n.load().fedagg_abi_version())")
    env = {k: v for k, v in os.environ.items() if k not in ("FEDAGG_LIB", "PYTHONPATH")}
    env["PYTHONPATH"] = str(tmp_path / "site")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=tmp_path, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    pkg, lib, abi = r.stdout.split()
    assert pkg.startswith(str(tmp_path / "site")) and lib == str(tmp_path / "site" / "substrafl_amd" / "libfedagg.so")
    from substrafl_amd import _native

    assert int(abi) == _native.ABI_VERSION


def test_wheel_build_without_hipcc_fails_loudly(tmp_path):
    env = dict(os.environ, HIPCC=str(tmp_path / "no-hipcc"))
    r = _pip_wheel(tmp_path / "w", env=env)
    assert r.returncode != 0
    assert "hipcc not found" in r.stdout + r.stderr
    assert not list((tmp_path / "w").glob("*.whl"))


@pytest.mark.skipif(not Path("/root/reference/substrafl").exists(),
                    reason="needs the reference source (build container only)")
@needs_hipcc
def test_reference_dependency_ships_the_wheel(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, str(HERE / "reference_dependency.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert len(res["wheels"]) == 1 and res["wheels"][0].startswith("substrafl_amd-0.5.0-")
    assert res["wheel_has_library"] and res["wheel_has_package"] and not res["wheel_has_tests"]
    assert res["requirements_name_the_wheel"]
    assert res["non_package_dir"] == "InvalidPathError"
