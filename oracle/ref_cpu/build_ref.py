"""Build the reference's own rasterizer and simple-knn for the host: oracle/_ref/libgs4d_ref.so.

TEST INFRASTRUCTURE ONLY.  The reference checkout (GS4D_REFERENCE, default /root/reference) holds the CUDA
sources of submodules/depth-diff-gaussian-rasterization/cuda_rasterizer and submodules/simple-knn.  They use
nothing of CUDA that cuda_on_cpu.h does not restate for a host compiler, so this recipe

  1. copies cuda_rasterizer/*.{cu,h} and simple_knn.{cu,h} into oracle/_ref/src/ (the .cu files as .cpp) and
     rewrites ONLY the `kernel << <grid, block >> > (` launch sites into CUDA_ON_CPU_LAUNCH(kernel, grid, block,
     -- nothing else of their text changes;
  2. compiles them with g++ -std=c++17 -O1 -ffp-contract=off (no -ffast-math), this directory first on the
     include path so that <cuda.h>, <cub/cub.cuh>, <cooperative_groups.h>, <thrust/...> resolve to the shim, and
     the reference's third_party/glm as an include path only;
  3. links them with the block runtime (cuda_on_cpu.cpp) and the extern "C" wrappers (ref_wrap.cpp, knn_wrap.cpp).

Floating point: nvcc would contract a * b + c into FMAs; this build does not (-ffp-contract=off, and x86-64 has
no FMA without -march).  oracle/Makefile builds the C oracle with the same convention, so the two CPU references
are compared under one set of rounding rules, and what separates them is the order of operations alone.

Everything derived from the reference stays inside oracle/_ref/, which git ignores; nothing of it is committed.
When the checkout is absent (any machine but the build container) `build()` returns None and builds nothing.
"""
import glob
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(os.path.dirname(HERE), "_ref")
LIB = os.path.join(OUT_DIR, "libgs4d_ref.so")
REFERENCE = os.environ.get("GS4D_REFERENCE", "/root/reference")
RASTER = os.path.join("submodules", "depth-diff-gaussian-rasterization")
KNN = os.path.join("submodules", "simple-knn")
N_LAUNCH_SITES = {"forward.cu": 2, "backward.cu": 3, "rasterizer_impl.cu": 3, "simple_knn.cu": 3}
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-w", "-D__CUDACC__="]

_LAUNCH = re.compile(r"(\w+(?:<\s*\w+\s*>)?)\s*<<\s*<\s*(.+?)\s*>>\s*>\s*\(")


def reference_present(ref=None):
    ref = REFERENCE if ref is None else ref
    return os.path.isfile(os.path.join(ref, RASTER, "cuda_rasterizer", "rasterizer_impl.cu")) and \
        os.path.isfile(os.path.join(ref, KNN, "simple_knn.cu"))


def _split_config(cfg):
    """'grid, block' at the last comma outside parentheses"""
    depth = 0
    for i in range(len(cfg) - 1, -1, -1):
        c = cfg[i]
        depth += (c == ")") - (c == "(")
        if c == "," and depth == 0:
            return cfg[:i].strip(), cfg[i + 1:].strip()
    raise ValueError(f"launch configuration without a block size: {cfg!r}")


def rewrite_launches(text):
    """(text with every launch site rewritten, number of sites)"""
    def sub(m):
        grid, block = _split_config(m.group(2))
        return f"CUDA_ON_CPU_LAUNCH({m.group(1)}, ({grid}), ({block}), "
    return _LAUNCH.subn(sub, text)


def _sources(ref):
    r = os.path.join(ref, RASTER, "cuda_rasterizer")
    files = sorted(glob.glob(os.path.join(r, "*.cu")) + glob.glob(os.path.join(r, "*.h")))
    return files + [os.path.join(ref, KNN, "simple_knn.cu"), os.path.join(ref, KNN, "simple_knn.h")]


def _own_files():
    return [os.path.join(HERE, f) for f in ("cuda_on_cpu.h", "cuda_on_cpu.cpp", "ref_wrap.cpp", "knn_wrap.cpp",
                                            "build_ref.py")]


def build(verbose=False, ref=None):
    """Build oracle/_ref/libgs4d_ref.so if the reference checkout is present; returns its path, or None without
    a checkout.  Up to date when newer than every input."""
    ref = REFERENCE if ref is None else ref
    if not reference_present(ref):
        return None
    inputs = _sources(ref) + _own_files()
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(f) for f in inputs):
        return LIB
    src = os.path.join(OUT_DIR, "src")
    obj = os.path.join(OUT_DIR, "obj")
    for d in (src, obj):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    units = []
    for f in _sources(ref):
        name = os.path.basename(f)
        with open(f, encoding="utf-8", errors="surrogateescape") as fh:
            text = fh.read()
        if name.endswith(".cu"):
            text, n = rewrite_launches(text)
            if n != N_LAUNCH_SITES.get(name, 0):
                raise RuntimeError(f"{name}: {n} launch sites rewritten, {N_LAUNCH_SITES.get(name, 0)} expected")
            name = name[:-3] + ".cpp"
            units.append(os.path.join(src, name))
        with open(os.path.join(src, name), "w", encoding="utf-8", errors="surrogateescape") as fh:
            fh.write(text)
    units += [os.path.join(HERE, f) for f in ("cuda_on_cpu.cpp", "ref_wrap.cpp", "knn_wrap.cpp")]
    cxx = os.environ.get("CXX", "g++")
    includes = ["-I", HERE, "-I", src, "-I", os.path.join(ref, RASTER, "third_party", "glm")]
    procs = []
    for u in units:
        o = os.path.join(obj, os.path.splitext(os.path.basename(u))[0] + ".o")
        cmd = [cxx] + CXXFLAGS + includes + ["-c", u, "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((subprocess.Popen(cmd), cmd, o))
    objs = []
    for p, cmd, o in procs:
        if p.wait() != 0:
            raise RuntimeError("reference host build failed: " + " ".join(cmd))
        objs.append(o)
    tmp = LIB + ".tmp"
    subprocess.check_call([cxx, "-shared", "-o", tmp] + objs)
    os.replace(tmp, LIB)
    if verbose:
        print("built", LIB, flush=True)
    return LIB


if __name__ == "__main__":
    if build(verbose=True) is None:
        print("no reference checkout at", REFERENCE, file=sys.stderr)
        sys.exit(1)
