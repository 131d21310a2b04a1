"""Recipe for oracle/_ref/: the REFERENCE's own rasterizer sources, compiled for the host CPU.

TEST INFRASTRUCTURE ONLY.  Called from __graft_entry__.build().  When the reference tree is present, the three CUDA sources
of each rasterizer submodule (forward.cu, backward.cu, rasterizer_impl.cu) are copied into oracle/_ref/src/<variant>/ with
one textual change -- every `kernel<<<grid, block>>>(` becomes `ref_shim::launch(kernel, grid, block, ` -- and compiled with
oracle/ref_glue.cpp against the reference's own headers and its bundled glm; oracle/ref_shim/ stands in for the CUDA
headers.  One library per config.h variant (the submodules differ only in NUM_CHANNELS):

    oracle/_ref/libref_raster_17.so  (h36m)    libref_raster_19.so  (panoptic)    libref_raster_15.so  (op)

When the reference tree is absent, whatever is in oracle/_ref/ is left alone and nothing is built.  Nothing under
oracle/_ref/ is ever committed (.gitignore), and nothing here holds reference program text.
"""
import os
import re
import subprocess
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, "_ref")
SHIM = os.path.join(_HERE, "ref_shim")
GLUE = os.path.join(_HERE, "ref_glue.cpp")
REF = "/root/reference"

VARIANTS = {17: "diff-gaussian-rasterization-h36m", 19: "diff-gaussian-rasterization-panoptic",
            15: "diff-gaussian-rasterization-op"}
SOURCES = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
N_LAUNCH_SITES = 8

# `name<T> << <grid, block >> > (`  (the sources spell the chevrons with blanks inside)
_LAUNCH = re.compile(r"(\b\w+(?:\s*<\s*\w+\s*>)?)\s*<\s*<\s*<(.*?)>\s*>\s*>\s*\(", re.S)
# same numeric contract as oracle/Makefile; -O1 keeps the three builds short, the arithmetic does not depend on it
CXXFLAGS = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]


def lib_path(channels):
    return os.path.join(OUT, "libref_raster_%d.so" % channels)


def submodule(channels):
    return os.path.join(REF, "submodules", VARIANTS[channels])


def reference_present():
    return all(os.path.isfile(os.path.join(submodule(c), "cuda_rasterizer", s)) for c in VARIANTS for s in SOURCES)


def rewrite_launches(text):
    """-> (text with every triple-chevron launch turned into an ordinary call, number of launches rewritten)"""
    return _LAUNCH.subn(lambda m: "ref_shim::launch(%s, %s, " % (m.group(1), m.group(2).strip()), text)


def _stale(so, deps):
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)


def _own_files():
    own = [GLUE, os.path.abspath(__file__)]
    for d, _, files in os.walk(SHIM):
        own += [os.path.join(d, f) for f in files]
    return own


def build(force=False, verbose=False, cxx=None):
    """-> {channels: path of the library} for what exists afterwards; builds only with the reference tree present."""
    if not reference_present():
        if verbose:
            print("ref_build: no reference tree at %s -- oracle/_ref left as it is" % REF)
        return {c: lib_path(c) for c in VARIANTS if os.path.exists(lib_path(c))}
    cxx = cxx or os.environ.get("CXX", "g++")
    for c, name in VARIANTS.items():
        root = submodule(c)
        cu_dir = os.path.join(root, "cuda_rasterizer")
        headers = [os.path.join(cu_dir, f) for f in os.listdir(cu_dir) if f.endswith(".h")]
        srcs = [os.path.join(cu_dir, s) for s in SOURCES]
        so = lib_path(c)
        if not (force or _stale(so, srcs + headers + _own_files())):
            continue
        t0 = time.time()
        dst = os.path.join(OUT, "src", name)
        os.makedirs(dst, exist_ok=True)
        n_sites, copied = 0, []
        for s in srcs:
            with open(s) as f:
                text, n = rewrite_launches(f.read())
            n_sites += n
            copied.append(os.path.join(dst, os.path.basename(s)))
            with open(copied[-1], "w") as f:
                f.write(text)
        assert n_sites == N_LAUNCH_SITES, "%s: rewrote %d kernel launches, the rasterizer has %d" % (name, n_sites, N_LAUNCH_SITES)
        assert not any(re.search(r"<\s*<\s*<", open(p).read()) for p in copied), "%s: a launch was left behind" % name
        tmp = so + ".tmp"
        cmd = [cxx] + CXXFLAGS + ["-shared", "-o", tmp, "-I", SHIM, "-I", cu_dir, "-I", os.path.join(root, "third_party", "glm"),
                                  "-x", "c++"] + copied + [GLUE]
        subprocess.check_call(cmd)
        os.replace(tmp, so)
        if verbose:
            print("ref_build: %s (NUM_CHANNELS %d) in %.1f s" % (os.path.relpath(so, os.path.dirname(_HERE)), c, time.time() - t0))
    return {c: lib_path(c) for c in VARIANTS if os.path.exists(lib_path(c))}


if __name__ == "__main__":
    import sys
    print(build(force="--force" in sys.argv, verbose=True))
