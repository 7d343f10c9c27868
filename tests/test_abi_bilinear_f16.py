"""The fp16-storage bilinear word-grid calls in the C ABI: declared in include/mms.h with their parameter lists, exported by the built
library, bound in capi, and MMS_VERSION still 212 (the change is additive)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID = r"int N, int W1, int W2, int D, int M, const void\* q_f16, const void\* a_f16, const float\* W, "
DECLS = {
    "mms_simcross_bilinear_workspace_bytes_f16": r"size_t %s\(int N, int W1, int W2, int D, int M\);",
    "mms_simcross_bilinear_forward_f16":
        r"int %s\(" + GRID + r"const float\* bias, float\* top, void\* workspace, size_t workspace_bytes, void\* stream\);",
    "mms_simcross_bilinear_backward_f16":
        r"int %s\(" + GRID + r"int bias_term, const float\* top_diff, void\* dq_f16, void\* da_f16, float\* dW, float\* dbias, "
        r"void\* workspace, size_t workspace_bytes, void\* stream\);",
    "mms_simcross_bilinear_forward_backward_f16":
        r"int %s\(" + GRID + r"const float\* bias, const float\* top_diff, float\* top, void\* dq_f16, void\* da_f16, float\* dW, "
        r"float\* dbias, void\* workspace, size_t workspace_bytes, void\* stream\);",
    "mms_embed_simcross_bilinear_forward_f16":
        r"int %s\(int N, int W1, int W2, int D, int M, int K, const float\* index_q, const float\* index_a, const void\* table_f16, "
        r"const float\* embed_bias, const float\* W, const float\* bias, float\* top, void\* stream\);",
}
WRAPPERS = ("simcross_bilinear_forward_f16", "simcross_bilinear_backward_f16", "simcross_bilinear_forward_backward_f16",
            "embed_simcross_bilinear_forward_f16", "simcross_bilinear_workspace_bytes_f16")


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"\s+", " ", txt)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_declared_exported_and_bound(name, hiplib):
    from mms_answer_selection_amd import capi
    assert re.search(DECLS[name] % name, _header()), "%s is not declared in include/mms.h with the agreed parameter list" % name
    assert hasattr(hiplib, name), "%s is not exported by libmms_hip.so" % name
    assert name in capi._SIGNATURES and name in capi.EXPORTED_SYMBOLS
    res, args = capi._SIGNATURES[name]
    decl = re.search(r"%s\((.*?)\);" % name, _header()).group(1)
    assert len(args) == len(decl.split(",")), "capi binds %d arguments, the header declares %d" % (len(args), len(decl.split(",")))
    assert res is (ctypes.c_size_t if "workspace_bytes" in name else ctypes.c_int)


def test_wrappers_exist():
    from mms_answer_selection_amd import capi
    for w in WRAPPERS:
        assert callable(getattr(capi, w)), w


def test_version_is_still_212(hiplib):
    from mms_answer_selection_amd import capi
    header = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert re.search(r"#define MMS_VERSION 212\b", header)
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_host_side_checks_need_no_gpu(hiplib):
    """The workspace query and the refusals that come before any launch."""
    ws = hiplib.mms_simcross_bilinear_workspace_bytes_f16
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    base = hiplib.mms_simcross_workspace_bytes
    base.restype, base.argtypes = ctypes.c_size_t, [ctypes.c_int] * 6
    assert ws(50, 40, 40, 50, 4) == base(2, 50, 40, 40, 50, 4) > 0, "both directions fused: the fp32 layer's workspace"
    for s in ((1517, 40, 40, 50, 4), (300, 5, 7, 50, 2), (3, 5, 7, 65, 2)):
        N, W1, W2, D, M = s
        assert ws(*s) >= base(2, *s) + 2 * 4 * N * (W1 + W2) * D, "the generic route holds q, a, dq, da in fp32: %s" % (s,)
    assert ws(4, 1, 1, 50, 1) == 0 and ws(-1, 5, 7, 50, 2) == 0 and ws(4, 5, 7, 50, 0) == 0
    f = hiplib.mms_simcross_bilinear_forward_f16
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    assert f(4, 5, 7, 50, 0, 1, 1, 1, None, 1, 1, 1 << 30, None) == 1          # MMS_ERR_INVALID_ARG: M == 0
    assert f(4, 1, 1, 50, 1, 1, 1, 1, None, 1, 1, 1 << 30, None) == 2          # MMS_ERR_UNSUPPORTED: the rows family
    assert f(4, 5, 7, 50, 2, None, 1, 1, None, 1, 1, 1 << 30, None) == 1       # q NULL
    assert f(4, 5, 7, 50, 2, 1, 1, 1, None, 1, None, 0, None) == 3             # MMS_ERR_WORKSPACE, nothing enqueued
    assert f(4, 5, 7, 50, 2, 1, 1, 1, None, 1, 1, ws(4, 5, 7, 50, 2) - 1, None) == 3
    assert f(0, 5, 7, 50, 2, None, None, None, None, None, None, 0, None) == 0  # N == 0
