"""CPU suite: the six BN -> MaxPool -> TanH entry points are declared in include/mms_bn_maxpool.h (valid C) with the
documented parameter lists, exported by the built library and bound by mms_answer_selection_amd/bn_maxpool.py; the
refusal table of tests/test_abi_bn_pool.py holds for the new names -- the same codes, the same winner where two rules
fail, nothing enqueued -- with `shift` one more required input of the backward; the workspace query is
mms_bn_pool_tanh_workspace_bytes' figure; include/mms.h, capi.py and the ABI version are as they were."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import pooled_stage_suite as A
from conftest import ROOT

OK, INVALID, WORKSPACE = A.OK, A.INVALID, A.WORKSPACE
P, LARGE, SMALL, EMPTY, BAD_SHAPES = A.P, A.LARGE, A.SMALL, A.EMPTY, A.BAD_SHAPES
N_FWD, N_BWD = 9, 11                      # arrays of a forward / a backward call: the backward has shift too
N_BWD_INPUTS = 8                          # x, top, top_diff, save_pool, scale, shift, save_mean, save_std


def _backward(t):
    c = "const %s* " % t
    m = "%s* " % t
    return (A.DIMS + [c + "x", c + "top", c + "top_diff", c + "save_pool", c + "scale", c + "shift", c + "save_mean",
                      c + "save_std", m + "bottom_diff", m + "scale_diff", m + "shift_diff"] + A.WS)


SIGNATURES = {
    "mms_bn_maxpool_tanh_workspace_bytes": ("size_t", A.DIMS),
    "mms_bn_maxpool_tanh_workspace_bytes_f64": ("size_t", A.DIMS),
    "mms_bn_maxpool_tanh_forward_f32": ("int", A.bn_pool_forward_params("float")),
    "mms_bn_maxpool_tanh_forward_f64": ("int", A.bn_pool_forward_params("double")),
    "mms_bn_maxpool_tanh_backward_f32": ("int", _backward("float")),
    "mms_bn_maxpool_tanh_backward_f64": ("int", _backward("double")),
}
NAMES = sorted(SIGNATURES)
FORWARDS = ["mms_bn_maxpool_tanh_forward_f32", "mms_bn_maxpool_tanh_forward_f64"]
BACKWARDS = ["mms_bn_maxpool_tanh_backward_f32", "mms_bn_maxpool_tanh_backward_f64"]
QUERIES = ["mms_bn_maxpool_tanh_workspace_bytes", "mms_bn_maxpool_tanh_workspace_bytes_f64"]


@pytest.fixture(scope="module")
def lib(hiplib):
    from mms_answer_selection_amd import bn_maxpool
    return bn_maxpool.lib()


def _query(lib, name):
    return getattr(lib, "mms_bn_maxpool_tanh_workspace_bytes" + ("" if name.endswith("f32") else "_f64"))


def _header():
    txt = open(os.path.join(ROOT, "include", "mms_bn_maxpool.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_the_header_declares_these_six_and_nothing_else():
    assert sorted(set(re.findall(r"\b(mms_\w+)\s*\(", _header()))) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_call_is_declared_exported_and_bound(lib, name):
    from mms_answer_selection_amd import bn_maxpool
    ret, want = SIGNATURES[name]
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), _header())
    assert m, "include/mms_bn_maxpool.h does not declare %s %s" % (ret, name)
    assert [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")] == want
    so = os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so")
    assert hasattr(lib, name) and name.encode() in open(so, "rb").read()
    assert name in bn_maxpool.EXPORTED_SYMBOLS and len(bn_maxpool.EXPORTED_SYMBOLS) == 6
    fn = getattr(lib, name)
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
    assert fn.restype is ctype[ret]
    assert list(fn.argtypes) == [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in want]
    assert callable(getattr(bn_maxpool, name[len("mms_"):].replace("_f32", "")))


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "bn_maxpool_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(lib):
    from mms_answer_selection_amd import capi
    for f in (os.path.join("include", "mms.h"), os.path.join("mms_answer_selection_amd", "capi.py"),
              os.path.join("mms_answer_selection_amd", "__init__.py")):
        assert "maxpool" not in open(os.path.join(ROOT, f)).read(), f
    assert not [n for n in dir(capi) if "maxpool" in n]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "maxpool" in n]
    assert lib.mms_version() == 212 and capi.MMS_VERSION == 212


def _distinct(n):
    return [P + 64 * i for i in range(n)]


def _fwd(fn, phase, shape, arrays=None, mem=0.9, ws=P, ws_bytes=1 << 40):
    arrays = _distinct(N_FWD) if arrays is None else arrays
    return fn(phase, *shape, mem, *arrays, ws, ws_bytes, None)


def _bwd(fn, shape, arrays=None, ws=P, ws_bytes=1 << 40):
    arrays = _distinct(N_BWD) if arrays is None else arrays
    return fn(*shape, *arrays, ws, ws_bytes, None)


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_host_side_rules(lib, name):
    fn = getattr(lib, name)
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
        for out in (5, 6):                                       # top and save_pool alias no input ...
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
def test_forward_workspace_rule(lib, name):
    """TRAIN on the two-launch route needs the workspace the query names; it is judged last, still before any launch."""
    fn = getattr(lib, name)
    need = _query(lib, name)(*LARGE)
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
def test_backward_host_side_rules(lib, name):
    fn = getattr(lib, name)
    for shape in BAD_SHAPES:
        assert _bwd(fn, shape) == INVALID, shape
    assert _bwd(fn, EMPTY) == OK
    assert _bwd(fn, EMPTY, [None] * N_BWD, ws=None, ws_bytes=0) == OK
    for k in range(N_BWD_INPUTS):                 # every input is required, shift among them
        arrays = _distinct(N_BWD)
        arrays[k] = None
        assert _bwd(fn, SMALL, arrays) == INVALID, k
        assert _bwd(fn, LARGE, arrays) == INVALID, k
        arrays = _distinct(N_BWD)                 # bottom_diff aliases no input
        arrays[N_BWD_INPUTS] = arrays[k]
        assert _bwd(fn, SMALL, arrays) == INVALID, k
        assert _bwd(fn, LARGE, arrays, ws=None, ws_bytes=0) == INVALID, k
    arrays = _distinct(N_BWD_INPUTS) + [None] * 3
    assert _bwd(fn, SMALL, arrays) == INVALID     # none of the three outputs asked for
    assert _bwd(fn, LARGE, arrays) == INVALID
    need = _query(lib, name)(*LARGE)
    for given in range(N_BWD_INPUTS, N_BWD):      # any one output is enough: the workspace is then the only thing wrong
        arrays = _distinct(N_BWD_INPUTS) + [None] * 3
        arrays[given] = P + 64 * given
        assert _bwd(fn, LARGE, arrays, ws=None, ws_bytes=need) == WORKSPACE
        assert _bwd(fn, LARGE, arrays, ws=P, ws_bytes=need - 1) == WORKSPACE
        assert _bwd(fn, LARGE, arrays, ws=P, ws_bytes=0) == WORKSPACE


@pytest.mark.parametrize("name", QUERIES)
def test_workspace_query_is_the_ave_calls(lib, hiplib, name):
    q, ave = getattr(lib, name), getattr(hiplib, name.replace("maxpool", "pool"))
    assert q(50, 64, 5, 5, 5, 5) == 0 and q(1, 1, 1, 1, 1, 1) == 0 and q(0, 32, 36, 36, 4, 4) == 0
    for bad in BAD_SHAPES:
        assert q(*bad) == 0, bad
    assert q(50, 32, 36, 36, 4, 4) > 0 and q(1517, 32, 36, 36, 4, 4) > 0 and q(1517, 64, 5, 5, 5, 5) > 0
    for C_, H, W, kh, kw in ((32, 36, 36, 4, 4), (64, 5, 5, 5, 5), (1, 1, 1, 1, 1), (3, 25, 41, 5, 1), (5, 9, 37, 3, 37),
                             (32, 38, 38, 2, 2), (64, 6, 6, 6, 6)):
        for N in list(range(1, 400)) + [700, 1517, 4099, 20000, 100000]:
            assert q(N, C_, H, W, kh, kw) == ave(N, C_, H, W, kh, kw), (N, C_, H, W, kh, kw)


def test_the_binding_binds_before_its_first_call():
    """In a fresh process the first call of each wrapper -- refused here for its host tensors -- leaves the signatures
    on the handle: no call reaches the library with an unbound function (pointers would go in as 32-bit ints)."""
    code = ("import torch\n"
            "from mms_answer_selection_amd import capi, bn_maxpool as M\n"
            "x, p, k = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2, 2), torch.zeros(3)\n"
            "try:\n"
            "    %s\n"
            "    raise SystemExit(3)\n"
            "except capi.MMSError:\n"
            "    pass\n"
            "assert all(getattr(capi.lib(), n).argtypes is not None for n in M.EXPORTED_SYMBOLS)\n")
    for call in ("M.bn_maxpool_tanh_forward(x, 2, k, k, k, k, p, p, k, k)",
                 "M.bn_maxpool_tanh_backward(x, 2, p, p, p, k, k, k, k, x)"):
        subprocess.check_call([sys.executable, "-c", code % call], cwd=ROOT)
