"""CPU suite: the fused cosine triplet step is declared in include/mms.h, exported by the built library and bound
by capi.py -- and adding it did not change the ABI version (no compute calls without a GPU)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "mms_triplet_cosine_step_f32"


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_triplet_cosine_step_is_declared_with_the_documented_signature():
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, _header())
    assert m, "include/mms.h does not declare %s" % NAME
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == [
        "int N", "int D", "float margin", "float loss_weight", "const float* q", "const float* a_pos",
        "const float* a_neg", "const float* y", "float* s_pos", "float* s_neg", "float* norm_q", "float* norm_pos",
        "float* norm_neg", "float* loss", "float* dq", "float* da_pos", "float* da_neg", "void* workspace",
        "size_t workspace_bytes", "void* stream"], params


def test_triplet_cosine_step_is_exported(hiplib):
    assert hasattr(hiplib, NAME), "libmms_hip.so lacks %s" % NAME
    so = os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so")
    assert NAME.encode() in open(so, "rb").read()


def test_capi_carries_the_signature(hiplib):
    from mms_answer_selection_amd import capi
    assert NAME in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_int, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 14 + [C.c_size_t, C.c_void_p]
    assert callable(capi.triplet_cosine_step)


def test_host_side_checks_need_no_gpu(hiplib):
    """Argument errors and the empty batch are decided before anything is enqueued."""
    z = [None] * 14
    assert getattr(hiplib, NAME)(-1, 300, 1.0, 1.0, *z, 0, None) == 1          # MMS_ERR_INVALID_ARG
    assert getattr(hiplib, NAME)(8, 0, 1.0, 1.0, *z, 0, None) == 1
    assert getattr(hiplib, NAME)(8, 300, 1.0, 1.0, *z, 0, None) == 1           # NULL arrays
    assert getattr(hiplib, NAME)(0, 300, 1.0, 1.0, *z, 0, None) == 0           # N == 0: a no-op


def test_version_is_unchanged(hiplib):
    from mms_answer_selection_amd import capi
    assert hiplib.mms_version() == 212
    assert capi.MMS_VERSION == 212
    assert re.search(r"#define\s+MMS_VERSION\s+212\b", _header())
