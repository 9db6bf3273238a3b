#!/usr/bin/env python3
"""Demangled names of every GPU kernel in a built libfedagg.so, one per line, sorted.  Symbol
names only: the library's .hip_fatbin section is split into its offload bundles, each bundle's
gfx950 code object is unbundled (clang-offload-bundler) and its symbol table listed
(llvm-readelf --symbols); a kernel is a symbol with a `<name>.kd` descriptor next to it.  The
instructions are never read.  Names are normalised as tools/kernel_resources.py prints them (no
anonymous namespace, template arguments kept, parameter list dropped).
Usage: tools/product_kernels.py [substrafl_amd/libfedagg.so] > profiles/product_kernels.txt"""

import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "substrafl_amd" / "libfedagg.so"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name: str) -> str:
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (shutil.which(name), f"{rocm}/llvm/bin/{name}", f"{rocm}/lib/llvm/bin/{name}"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError(f"{name} not found (PATH, {rocm}/llvm/bin)")


def normalise(demangled: str) -> str:
    """The short form of tools/kernel_resources.py."""
    dem = demangled.strip().replace("(anonymous namespace)::", "")
    if dem.startswith("void "):
        dem = dem[len("void "):]
    return dem.split("(")[0] if "<" not in dem else dem[: dem.index(">(") + 1]


def kernel_names(lib: Path = LIB) -> list:
    """Sorted, normalised kernel names of ``lib`` (raises when a tool is missing or fails)."""
    mangled = set()
    with tempfile.TemporaryDirectory() as d:
        fat = Path(d) / "fatbin"
        subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(lib), str(Path(d) / "rest")],
                       check=True, capture_output=True)
        blob = fat.read_bytes()
        starts = []
        at = blob.find(MAGIC)
        while at >= 0:
            starts.append(at)
            at = blob.find(MAGIC, at + 1)
        if not starts:
            raise RuntimeError(f"{lib}: no offload bundle in .hip_fatbin")
        for i, s in enumerate(starts):  # one bundle per linked object that holds device code
            bundle, co = Path(d) / f"bundle{i}", Path(d) / f"code{i}.co"
            bundle.write_bytes(blob[s: starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                            f"--input={bundle}", f"--output={co}"], check=True, capture_output=True)
            if not co.exists() or co.stat().st_size == 0:
                continue
            syms = subprocess.run([_tool("llvm-readelf"), "--symbols", "--wide", str(co)], check=True,
                                  capture_output=True, text=True).stdout
            for line in syms.splitlines():
                f = line.split()
                if len(f) == 8 and f[7].endswith(".kd") and f[3] == "OBJECT":
                    mangled.add(f[7][:-3])
    mangled = sorted(mangled)
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout
    names = sorted(normalise(n) for n in dem.splitlines() if n.strip())
    if len(set(names)) != len(names):
        raise RuntimeError("two kernels share a normalised name")
    return names


def main():
    lib = Path(sys.argv[1]) if len(sys.argv) > 1 else LIB
    print("\n".join(kernel_names(lib)))


if __name__ == "__main__":
    main()
