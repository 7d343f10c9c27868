"""Build libmms_hip.so (HIP kernels + C ABI) and libmms_caffe.so (the Caffe-API mirror) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU.  Flags that matter for parity:
  -ffp-contract=off   the reference CPU build has no FMA contraction; mul and
                      add must round separately for bit-exact Euclidean paths.
  -fhip-fp32-correctly-rounded-divide-sqrt   IEEE sqrt / divide (hipcc default,
                      stated explicitly because the parity tests rely on it).
  -mllvm -amdgpu-kernarg-preload-count=16   leading kernel arguments are placed in
                      SGPRs at wave launch (gfx940+), so a latency-bound kernel does not
                      begin with a scalar fetch of its argument block.
"""
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmms_hip.so")
LAYER_LIB = os.path.join(HERE, "libmms_caffe.so")

HIP_SOURCES = ["mms_abi.hip", "net_glue.hip", "simcross_rows.hip", "simcross_rows_cosine.hip", "simcross_rows_f16.hip", "simcross_cross.hip", "simcross_cross_f16.hip", "gemm32.hip", "bilinear.hip", "bilinear_f16.hip", "simmatrix.hip", "pairrank.hip", "triplet_steps.hip", "ranking.hip", "rank_onewg.hip", "embed.hip", "f64_paths.hip", "fm.hip", "bn.hip", "bn_pool.hip", "conv.hip", "conv_stage.hip", "conv_stage_train.hip", "head.hip", "score_tail.hip", "train_tail.hip", "train_tail_backward.hip", "solver.hip", "dropout.hip", "pool.hip", "fc.hip"]
# libmms_caffe.so: the Caffe-API mirror, host code compiled as HIP sources (caffe_api.hpp includes the HIP runtime header)
LAYER_SOURCES = ["caffe_runtime.cpp", "prototxt_reader.cpp", "layers_scoring.cpp", "layers_embed.cpp", "layers_metrics.cpp",
                 "layers_hdf5data.cpp", "path_net.cpp", "layer_handles.cpp", "caffemodel_io.cpp", "hdf5_io.cpp"]


def _hip_headers():
    """Every header under csrc/ and under include/ is a dependency of every object (panel_gemm.h is included by
    simmatrix.hip, gemm32.h by four sources, mms_conv.h, mms_head.h and mms_dropout.h by one each, ...): found by glob so that a new
    header cannot be forgotten."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hpp")) +
                  glob.glob(os.path.join(ROOT, "include", "*.h")))


HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-fno-fast-math", "-Wall", "-Wno-unused-function",
    "-mllvm", "-amdgpu-kernarg-preload-count=16",
]
# triplet_steps.hip: the arrival atomics of the fused steps are issued by ONE lane and their return values are consumed
# after the gradient stores; the atomic optimizer's wave scan + readfirstlane would pull the wait to the issue.
EXTRA_FLAGS = {"triplet_steps.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]}
LAYER_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-x", "hip", "--offload-arch=gfx950", "-Wall"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP library cannot be built (no fallback exists)")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_one(args):
    cmd, verbose = args
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _compile_objects(sources, flags_for, force, verbose):
    """One object under build/ per source of csrc/ (compiled in parallel, rebuilt only when the source, a header or this
    file is newer).  flags_for(name) gives the compile flags of one source.  Returns (objects, whether any was compiled)."""
    from concurrent.futures import ThreadPoolExecutor
    hdrs = _hip_headers() + [os.path.abspath(__file__)]
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs, objs = [], []
    for f in sources:
        src = os.path.join(CSRC, f)
        obj = os.path.join(objdir, os.path.splitext(f)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append(([_hipcc()] + flags_for(f) + ["-c", "-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", obj],
                         verbose))
    if jobs:
        # os.cpu_count() is the whole host's, whatever share of it this process may use: MAX_JOBS, else 16, caps the pool
        cap = int(os.environ.get("MAX_JOBS") or 16)
        with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), cap, (os.cpu_count() or 2) // 2))) as ex:
            list(ex.map(_compile_one, jobs))
    return objs, bool(jobs)


def _link(lib, objs, libs, verbose):
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib] + libs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build_hip(force=False, verbose=False):
    """libmms_hip.so: one object per .hip source, then one link."""
    cflags = [f for f in HIPCC_FLAGS if f != "-shared"]
    objs, compiled = _compile_objects(HIP_SOURCES, lambda f: cflags + EXTRA_FLAGS.get(f, []), force, verbose)
    if compiled or force or _stale(LIB, objs):
        _link(LIB, objs, [], verbose)
    return LIB


def build_layers(force=False, verbose=False):
    """libmms_caffe.so, the C++ mirror of the Caffe Layer/Blob API on top of the C ABI: one object per layer source,
    then one link against libmms_hip.so."""
    objs, compiled = _compile_objects(LAYER_SOURCES, lambda f: LAYER_FLAGS, force, verbose)
    if compiled or force or _stale(LAYER_LIB, objs + [LIB]):
        _link(LAYER_LIB, objs, ["-L", HERE, "-lmms_hip", "-lz", "-Wl,-rpath,$ORIGIN"], verbose)
    return LAYER_LIB


def build_all(force=False, verbose=False):
    return [build_hip(force, verbose), build_layers(force, verbose)]


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv, verbose=True))
