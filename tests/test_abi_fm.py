"""CPU suite: the five FM entry points are declared in include/mms.h with the documented parameter lists, exported by
the built library and bound by capi.py; their host-side argument rules hold without a GPU (nothing is enqueued on any
of these paths); adding them did not change the ABI version."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

F, D = "const float*", "const double*"
SIGNATURES = {
    "mms_fm_forward_f32": ["int N", "int C", "int dim", F + " x", F + " bias", "float* top", "void* stream"],
    "mms_fm_backward_f32": ["int N", "int C", "int dim", F + " x", F + " top_diff", "float* bottom_diff",
                            "float* bias_diff", "void* stream"],
    "mms_fm_forward_backward_f32": ["int N", "int C", "int dim", F + " x", F + " bias", F + " top_diff", "float* top",
                                    "float* bottom_diff", "float* bias_diff", "void* stream"],
    "mms_fm_forward_f64": ["int N", "int C", "int dim", D + " x", D + " bias", "double* top", "void* stream"],
    "mms_fm_backward_f64": ["int N", "int C", "int dim", D + " x", D + " top_diff", "double* bottom_diff",
                            "double* bias_diff", "void* stream"],
}
NAMES = sorted(SIGNATURES)
WRAPPERS = {"mms_fm_forward_f32": "fm_forward", "mms_fm_backward_f32": "fm_backward",
            "mms_fm_forward_backward_f32": "fm_forward_backward", "mms_fm_forward_f64": "fm_forward_f64",
            "mms_fm_backward_f64": "fm_backward_f64"}


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_fm_call_is_declared_with_the_documented_signature(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/mms.h does not declare %s" % name
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == SIGNATURES[name], params


@pytest.mark.parametrize("name", NAMES)
def test_fm_call_is_exported(hiplib, name):
    assert hasattr(hiplib, name), "libmms_hip.so lacks %s" % name
    so = os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so")
    assert name.encode() in open(so, "rb").read()


@pytest.mark.parametrize("name", NAMES)
def test_capi_carries_the_signature(hiplib, name):
    from mms_answer_selection_amd import capi
    assert name in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_int] * 3 + [C.c_void_p] * (len(SIGNATURES[name]) - 3)
    assert callable(getattr(capi, WRAPPERS[name]))


@pytest.mark.parametrize("name", NAMES)
def test_host_side_checks_need_no_gpu(hiplib, name):
    """Argument errors and the empty batch are decided before anything is enqueued.  `p` stands for arrays that are
    never touched: the calls below return before a launch."""
    fn = getattr(hiplib, name)
    narr = len(SIGNATURES[name]) - 4
    z, p = [None] * narr, [4096] * narr
    assert fn(-1, 2, 301, *p, None) == 1           # MMS_ERR_INVALID_ARG: negative N
    assert fn(8, 0, 301, *p, None) == 1            # C == 0
    assert fn(8, -2, 301, *p, None) == 1
    assert fn(8, 2, 0, *p, None) == 1              # dim == 0
    assert fn(8, 2, 301, *z, None) == 1            # NULL arrays with N > 0
    assert fn(0, 2, 301, *z, None) == 0            # N == 0: a no-op, whatever the pointers
    assert fn(0, 2, 301, *p, None) == 0
    assert fn(4096, 1024, 512, *p, None) == 1      # N*C*dim = 2^31 > INT_MAX: the reference indexes with int
    assert fn(2 ** 16, 2 ** 16, 1, *p, None) == 1  # ... already in N*C
    assert fn(2 ** 30, 2 ** 30, 2 ** 30, *p, None) == 1   # ... and past 64 bits


def test_each_required_array_is_checked(hiplib):
    """x and the outputs a call cannot do without; the optional ones (bias, bias_diff, and bottom_diff of the separate
    backward) are not among them -- that they may be NULL is exercised on the GPU."""
    p = 4096
    assert hiplib.mms_fm_forward_f32(8, 2, 3, None, p, p, None) == 1
    assert hiplib.mms_fm_forward_f32(8, 2, 3, p, p, None, None) == 1
    assert hiplib.mms_fm_forward_f64(8, 2, 3, None, p, p, None) == 1
    assert hiplib.mms_fm_forward_f64(8, 2, 3, p, p, None, None) == 1
    for fn in (hiplib.mms_fm_backward_f32, hiplib.mms_fm_backward_f64):
        assert fn(8, 2, 3, None, p, p, p, None) == 1
        assert fn(8, 2, 3, p, None, p, p, None) == 1
    fb = hiplib.mms_fm_forward_backward_f32
    assert fb(8, 2, 3, None, p, p, p, p, p, None) == 1     # x
    assert fb(8, 2, 3, p, p, None, p, p, p, None) == 1     # top_diff
    assert fb(8, 2, 3, p, p, p, None, p, p, None) == 1     # top
    assert fb(8, 2, 3, p, p, p, p, None, p, None) == 1     # bottom_diff is required in the fused call


def test_version_is_unchanged(hiplib):
    from mms_answer_selection_amd import capi
    assert hiplib.mms_version() == 212
    assert capi.MMS_VERSION == 212
    assert re.search(r"#define\s+MMS_VERSION\s+212\b", _header())
