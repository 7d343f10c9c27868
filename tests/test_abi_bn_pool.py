"""CPU suite: the six BN -> AvePool -> TanH entry points are declared in include/mms.h with the documented parameter
lists, exported by the built library and bound by capi.py; every host-side argument rule holds without a GPU (nothing is
enqueued on any of these paths); the workspace query is 0 on the one-workgroup route and grows with N; adding them did
not change the ABI version."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from pooled_stage_suite import (BAD_SHAPES, DIMS, EMPTY, INVALID, LARGE, OK, SMALL, WORKSPACE, WS, P,
                                bn_pool_forward_params)

def _backward(t):
    c = "const %s* " % t
    m = "%s* " % t
    return (DIMS + [c + "x", c + "top", c + "top_diff", c + "save_pool", c + "scale", c + "save_mean", c + "save_std",
                    m + "bottom_diff", m + "scale_diff", m + "shift_diff"] + WS)


SIGNATURES = {
    "mms_bn_pool_tanh_workspace_bytes": ("size_t", DIMS),
    "mms_bn_pool_tanh_workspace_bytes_f64": ("size_t", DIMS),
    "mms_bn_pool_tanh_forward_f32": ("int", bn_pool_forward_params("float")),
    "mms_bn_pool_tanh_forward_f64": ("int", bn_pool_forward_params("double")),
    "mms_bn_pool_tanh_backward_f32": ("int", _backward("float")),
    "mms_bn_pool_tanh_backward_f64": ("int", _backward("double")),
}
NAMES = sorted(SIGNATURES)
WRAPPERS = {n: n[len("mms_"):].replace("_f32", "") for n in NAMES}
FORWARDS = ["mms_bn_pool_tanh_forward_f32", "mms_bn_pool_tanh_forward_f64"]
BACKWARDS = ["mms_bn_pool_tanh_backward_f32", "mms_bn_pool_tanh_backward_f64"]
N_FWD, N_BWD = 9, 10                      # arrays of a forward / a backward call


def _query(hiplib, name):
    return getattr(hiplib, "mms_bn_pool_tanh_workspace_bytes" + ("" if name.endswith("f32") else "_f64"))


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_call_is_declared_with_the_documented_signature(name):
    ret, want = SIGNATURES[name]
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, "include/mms.h does not declare %s %s" % (ret, name)
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == want, params


@pytest.mark.parametrize("name", NAMES)
def test_call_is_exported(hiplib, name):
    assert hasattr(hiplib, name), "libmms_hip.so lacks %s" % name
    so = os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so")
    assert name.encode() in open(so, "rb").read()


@pytest.mark.parametrize("name", NAMES)
def test_capi_carries_the_signature(hiplib, name):
    from mms_answer_selection_amd import capi
    assert name in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), name)
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
    assert fn.restype is ctype[SIGNATURES[name][0]]
    want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in SIGNATURES[name][1]]
    assert list(fn.argtypes) == want
    assert callable(getattr(capi, WRAPPERS[name]))


def _distinct(n):
    return [P + 64 * i for i in range(n)]


def _fwd(fn, phase, shape, arrays=None, mem=0.9, ws=P, ws_bytes=1 << 40):
    arrays = _distinct(N_FWD) if arrays is None else arrays
    return fn(phase, *shape, mem, *arrays, ws, ws_bytes, None)


def _bwd(fn, shape, arrays=None, ws=P, ws_bytes=1 << 40):
    arrays = _distinct(N_BWD) if arrays is None else arrays
    return fn(*shape, *arrays, ws, ws_bytes, None)





@pytest.mark.parametrize("name", FORWARDS)
def test_forward_host_side_rules(hiplib, name):
    fn = getattr(hiplib, name)
    for shape in BAD_SHAPES:
        for phase in (0, 1):
            assert _fwd(fn, phase, shape) == INVALID, shape
    assert _fwd(fn, 0, (4095, 1024, 32, 16, 4, 4), [None] * N_FWD) == INVALID      # a good shape: the NULLs are what is wrong
    for phase in (-1, 2, 7):
        assert _fwd(fn, phase, SMALL) == INVALID                 # a phase other than TRAIN / TEST
        assert _fwd(fn, phase, EMPTY) == INVALID                 # ... also on the empty batch
    for phase in (0, 1):
        assert _fwd(fn, phase, EMPTY) == OK                      # N == 0: a no-op, whatever the pointers
        assert _fwd(fn, phase, EMPTY, [None] * N_FWD, ws=None, ws_bytes=0) == OK
        for k in range(N_FWD):                                   # every array is required
            arrays = _distinct(N_FWD)
            arrays[k] = None
            assert _fwd(fn, phase, SMALL, arrays) == INVALID, k
            assert _fwd(fn, phase, LARGE, arrays) == INVALID, k
        # x, scale, shift, running_mean, running_var, top, save_pool, ...: top and save_pool alias no input ...
        for out in (5, 6):
            for inp in range(5):
                arrays = _distinct(N_FWD)
                arrays[out] = arrays[inp]
                assert _fwd(fn, phase, SMALL, arrays) == INVALID, (out, inp)
                assert _fwd(fn, phase, LARGE, arrays) == INVALID, (out, inp)
        arrays = _distinct(N_FWD)                                # ... nor each other
        arrays[6] = arrays[5]
        assert _fwd(fn, phase, SMALL, arrays) == INVALID
        assert _fwd(fn, phase, LARGE, arrays) == INVALID


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_workspace_rule(hiplib, name):
    """TRAIN on the two-launch route needs the workspace the query names; the arrays are distinct and non-NULL, so the
    workspace is the only thing wrong (checked last, still before any launch)."""
    fn = getattr(hiplib, name)
    need = _query(hiplib, name)(*LARGE)
    assert need > 0
    arrays = _distinct(N_FWD)
    assert _fwd(fn, 0, LARGE, arrays, ws=None, ws_bytes=need) == WORKSPACE
    assert _fwd(fn, 0, LARGE, arrays, ws=P, ws_bytes=need - 1) == WORKSPACE
    assert _fwd(fn, 0, LARGE, arrays, ws=P, ws_bytes=0) == WORKSPACE
    arrays[3] = None
    assert _fwd(fn, 0, LARGE, arrays, ws=None, ws_bytes=0) == INVALID      # arguments are judged before the workspace
    arrays = _distinct(N_FWD)
    arrays[5] = arrays[0]
    assert _fwd(fn, 0, LARGE, arrays, ws=None, ws_bytes=0) == INVALID
    assert _fwd(fn, 0, (8, 2, 36, 36, 5, 4), ws=None, ws_bytes=0) == INVALID


@pytest.mark.parametrize("name", BACKWARDS)
def test_backward_host_side_rules(hiplib, name):
    fn = getattr(hiplib, name)
    for shape in BAD_SHAPES:
        assert _bwd(fn, shape) == INVALID, shape
    assert _bwd(fn, EMPTY) == OK
    assert _bwd(fn, EMPTY, [None] * N_BWD, ws=None, ws_bytes=0) == OK
    for k in range(7):                            # x, top, top_diff, save_pool, scale, save_mean, save_std
        arrays = _distinct(N_BWD)
        arrays[k] = None
        assert _bwd(fn, SMALL, arrays) == INVALID, k
        assert _bwd(fn, LARGE, arrays) == INVALID, k
        arrays = _distinct(N_BWD)                 # bottom_diff aliases no input
        arrays[7] = arrays[k]
        assert _bwd(fn, SMALL, arrays) == INVALID, k
        assert _bwd(fn, LARGE, arrays, ws=None, ws_bytes=0) == INVALID, k
    arrays = _distinct(7) + [None] * 3
    assert _bwd(fn, SMALL, arrays) == INVALID     # none of the three outputs asked for
    assert _bwd(fn, LARGE, arrays) == INVALID
    need = _query(hiplib, name)(*LARGE)
    for given in range(7, 10):                    # any one output is enough: the workspace is then the only thing wrong
        arrays = _distinct(7) + [None] * 3
        arrays[given] = P + 64 * given
        assert _bwd(fn, LARGE, arrays, ws=None, ws_bytes=need) == WORKSPACE
        assert _bwd(fn, LARGE, arrays, ws=P, ws_bytes=need - 1) == WORKSPACE
        assert _bwd(fn, LARGE, arrays, ws=P, ws_bytes=0) == WORKSPACE


@pytest.mark.parametrize("name", ["mms_bn_pool_tanh_workspace_bytes", "mms_bn_pool_tanh_workspace_bytes_f64"])
def test_workspace_query(hiplib, name):
    q = getattr(hiplib, name)
    item = 4 if name == "mms_bn_pool_tanh_workspace_bytes" else 8
    assert q(50, 64, 5, 5, 5, 5) == 0             # the training batch's second BN: one workgroup per channel
    assert q(1, 1, 1, 1, 1, 1) == 0 and q(0, 32, 36, 36, 4, 4) == 0
    for bad in BAD_SHAPES:
        assert q(*bad) == 0, bad                  # bad shapes ask for nothing
    assert q(50, 32, 36, 36, 4, 4) > 0 and q(1517, 32, 36, 36, 4, 4) > 0 and q(1517, 64, 5, 5, 5, 5) > 0
    for C_, H, W, kh, kw in ((32, 36, 36, 4, 4), (64, 5, 5, 5, 5), (1, 1, 1, 1, 1), (3, 25, 41, 5, 1), (5, 9, 37, 3, 37)):
        sizes = [q(N, C_, H, W, kh, kw) for N in range(1, 400)]
        sizes += [q(N, C_, H, W, kh, kw) for N in (700, 1517, 4099, 20000, 100000, 1000000, 2 ** 31 - 1)
                  if N * C_ * H * W <= 2 ** 31 - 1]
        assert sizes == sorted(sizes), (C_, H, W, kh, kw)
        assert sizes[-1] > 0
        for b in sizes:
            assert b % (C_ * 4 * item) == 0       # C channels x K chunks x 4 words
            assert b // (C_ * 4 * item) <= 64     # at most 64 chunks per channel, however long
    assert q(1517, 64, 5, 5, 5, 5) == 2 * q(1517, 32, 5, 5, 5, 5)
    assert q(1517, 32, 36, 36, 4, 4) == q(1517, 32, 36, 36, 36, 36)      # 64 chunks either way


def test_version_is_unchanged(hiplib):
    from mms_answer_selection_amd import capi
    assert hiplib.mms_version() == 212
    assert capi.MMS_VERSION == 212
    assert re.search(r"#define\s+MMS_VERSION\s+212\b", _header())
