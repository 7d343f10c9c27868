"""The fp16-storage Embed calls in the C ABI (mms_embed_forward_f16, _forward_pair_f16, _backward_f16, _backward_pair_f16,
_backward_pair_indexed_f16): declared in include/mms.h with their parameter lists, exported by the built library, bound in capi
with wrappers, MMS_VERSION still 212 (the change is additive), no workspace query of their own, and their host-side checks --
which need no GPU -- those of the _f32 twins, argument tuple for argument tuple."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3          # include/mms.h
I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

PAIR_BWD = (r"int %s\(int M0, int M1, int N, int K, const float\* index0, const void\* top_diff0_f16, const float\* index1, "
            r"const void\* top_diff1_f16, float\* weight_diff, float\* bias_diff, void\* (index_)?workspace, "
            r"size_t (index_)?workspace_bytes, void\* stream\);")
# name -> (declaration, argument types, wrapper, _f32 twin)
CALLS = {
    "mms_embed_forward_f16": (
        r"int %s\(int M, int N, int K, const float\* index, const void\* table_f16, const float\* bias, void\* top_f16, "
        r"void\* stream\);", [I] * 3 + [VP] * 5, "embed_forward_f16", "mms_embed_forward_f32"),
    "mms_embed_forward_pair_f16": (
        r"int %s\(int M0, int M1, int N, int K, const float\* index0, const float\* index1, const void\* table_f16, "
        r"const float\* bias, void\* top0_f16, void\* top1_f16, void\* index_workspace, size_t index_workspace_bytes, "
        r"void\* stream\);", [I] * 4 + [VP] * 7 + [SZ, VP], "embed_forward_pair_f16", "mms_embed_forward_pair_f32"),
    "mms_embed_backward_f16": (
        r"int %s\(int M, int N, int K, const float\* index, const void\* top_diff_f16, float\* weight_diff, "
        r"float\* bias_diff, void\* workspace, size_t workspace_bytes, void\* stream\);",
        [I] * 3 + [VP] * 5 + [SZ, VP], "embed_backward_f16", "mms_embed_backward_f32"),
    "mms_embed_backward_pair_f16": (PAIR_BWD, [I] * 4 + [VP] * 7 + [SZ, VP], "embed_backward_pair_f16",
                                    "mms_embed_backward_pair_f32"),
    "mms_embed_backward_pair_indexed_f16": (PAIR_BWD, [I] * 4 + [VP] * 7 + [SZ, VP], "embed_backward_pair_indexed_f16",
                                            "mms_embed_backward_pair_indexed_f32"),
}


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"\s+", " ", txt)


@pytest.mark.parametrize("name", list(CALLS))
def test_declared_exported_and_bound(hiplib, name):
    from mms_answer_selection_amd import capi
    decl, argtypes, wrapper, twin = CALLS[name]
    assert re.search(decl % name, _header()), "%s is not declared in include/mms.h with the agreed parameter list" % name
    assert hasattr(hiplib, name), "%s is not exported by libmms_hip.so" % name
    assert name in capi._SIGNATURES and name in capi.EXPORTED_SYMBOLS
    res, args = capi._SIGNATURES[name]
    declared = re.search(r"%s\((.*?)\);" % name, _header()).group(1).split(",")
    assert len(args) == len(declared) == len(argtypes), "capi binds %d arguments, the header declares %d" % (
        len(args), len(declared))
    assert len(args) == len(capi._SIGNATURES[twin][1])             # the twin's shape
    assert res is ctypes.c_int
    assert callable(getattr(capi, wrapper))


def test_the_f32_workspace_query_serves_the_f16_calls():
    """No mms_embed_workspace_bytes_f16: the layout holds nothing of the storage type, and the header says so."""
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert "mms_embed_workspace_bytes_f16" not in txt
    comment = txt[:txt.index("int mms_embed_forward_f16(")].rsplit("/*", 1)[1]
    assert "mms_embed_workspace_bytes(M, N)" in comment and "unchanged" in comment
    assert "MMS_ERR_UNSUPPORTED" in comment and "MMS_ERR_WORKSPACE" in comment


def test_version_is_still_212(hiplib):
    from mms_answer_selection_amd import capi
    header = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert re.search(r"#define MMS_VERSION 212\b", header)
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def _entry(hiplib, name, argtypes):
    f = getattr(hiplib, name)
    f.restype, f.argtypes = ctypes.c_int, argtypes
    return f


# 1 stands for a pointer that is never followed -- every tuple is answered before any launch
P = 1
BIG = (1 << 31) // 50 + 1             # BIG * 50 > 2^31 - 1
# (M, N, K, index, table, bias, top, stream)
FORWARD = [
    ((-1, 50, 97, P, P, None, P, None), INVALID_ARG, "M < 0"),
    ((7, 0, 97, P, P, None, P, None), INVALID_ARG, "N == 0"),
    ((7, -50, 97, P, P, None, P, None), INVALID_ARG, "N < 0"),
    ((7, 50, 0, P, P, None, P, None), INVALID_ARG, "K == 0"),
    ((7, 50, -1, P, P, None, P, None), INVALID_ARG, "K < 0"),
    ((BIG, 50, 97, P, P, None, P, None), INVALID_ARG, "M * N > 2^31 - 1"),
    ((7, 50, 97, None, P, None, P, None), INVALID_ARG, "index NULL"),
    ((7, 50, 97, P, None, None, P, None), INVALID_ARG, "table NULL"),
    ((7, 50, 97, P, P, None, None, None), INVALID_ARG, "top NULL"),
    ((0, 50, 97, None, None, None, None, None), OK, "M == 0 with NULL pointers"),
    ((0, 0, 97, None, None, None, None, None), INVALID_ARG, "M == 0 but N == 0"),
]
# (M, N, K, index, top_diff, weight_diff, bias_diff, workspace, workspace_bytes, stream)
BACKWARD = [
    ((-1, 50, 97, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M < 0"),
    ((7, 0, 97, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "N == 0"),
    ((7, 50, 0, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "K == 0"),
    ((7, 50, -2, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "K < 0"),
    ((BIG, 50, 97, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M * N > 2^31 - 1"),
    ((7, 50, 97, None, P, P, P, P, 1 << 30, None), INVALID_ARG, "index NULL"),
    ((7, 50, 97, P, None, P, P, P, 1 << 30, None), INVALID_ARG, "top_diff NULL"),
    ((7, 50, 97, P, P, None, None, None, 0, None), OK, "both diffs NULL"),
    ((7, 50, 97, None, None, None, None, None, 0, None), OK, "both diffs NULL, before the pointers are looked at"),
    ((0, 50, 97, None, None, P, P, None, 0, None), OK, "M == 0"),
    ((7, 50, 97, P, P, P, P, None, 0, None), WORKSPACE, "no workspace"),
    ((7, 50, 97, P, P, P, P, P, 16, None), WORKSPACE, "short workspace"),
    ((7, 50, 97, P, P, None, P, None, 0, None), WORKSPACE, "no workspace, bias_diff only"),
]
# (M0, M1, N, K, index0, index1, table, bias, top0, top1, index_workspace, index_workspace_bytes, stream)
FORWARD_PAIR = [
    ((0, 5, 50, 97, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "M0 == 0"),
    ((5, 0, 50, 97, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "M1 == 0"),
    ((-5, 5, 50, 97, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "M0 < 0"),
    ((5, 5, 0, 97, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "N == 0"),
    ((5, 5, 50, 0, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "K == 0"),
    ((BIG, 5, 50, 97, P, P, P, None, P, P, None, 0, None), INVALID_ARG, "(M0 + M1) * N > 2^31 - 1"),
    ((5, 5, 50, 97, None, P, P, None, P, P, None, 0, None), INVALID_ARG, "index0 NULL"),
    ((5, 5, 50, 97, P, None, P, None, P, P, None, 0, None), INVALID_ARG, "index1 NULL"),
    ((5, 5, 50, 97, P, P, None, None, P, P, None, 0, None), INVALID_ARG, "table NULL"),
    ((5, 5, 50, 97, P, P, P, None, None, P, None, 0, None), INVALID_ARG, "top0 NULL"),
    ((5, 5, 50, 97, P, P, P, None, P, None, None, 0, None), INVALID_ARG, "top1 NULL"),
    ((5, 5, 50, 97, P, P, P, None, P, P, P, 16, None), WORKSPACE, "short index workspace"),
]
# (M0, M1, N, K, index0, top_diff0, index1, top_diff1, weight_diff, bias_diff, workspace, workspace_bytes, stream)
BACKWARD_PAIR = [
    ((0, 5, 50, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M0 == 0"),
    ((5, 0, 50, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M1 == 0"),
    ((5, -1, 50, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M1 < 0"),
    ((0, 5, 50, 97, P, P, P, P, None, None, None, 0, None), INVALID_ARG, "M0 == 0 with both diffs NULL"),
    ((5, 5, 0, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "N == 0"),
    ((5, 5, 50, 0, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "K == 0"),
    ((BIG, 5, 50, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "(M0 + M1) * N > 2^31 - 1"),
    (((1 << 31) - 1, 5, 1, 97, P, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "M0 + M1 > 2^31 - 1"),
    ((5, 5, 50, 97, None, P, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "index0 NULL"),
    ((5, 5, 50, 97, P, None, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "top_diff0 NULL"),
    ((5, 5, 50, 97, P, P, None, P, P, P, P, 1 << 30, None), INVALID_ARG, "index1 NULL"),
    ((5, 5, 50, 97, P, P, P, None, P, P, P, 1 << 30, None), INVALID_ARG, "top_diff1 NULL"),
    ((5, 5, 50, 97, P, P, P, P, None, None, None, 0, None), OK, "both diffs NULL"),
    ((5, 5, 50, 97, P, P, P, P, P, P, None, 0, None), WORKSPACE, "no workspace"),
    ((5, 5, 50, 97, P, P, P, P, P, P, P, 16, None), WORKSPACE, "short workspace"),
]
# the indexed call: the same tuples, and sizes no index is built for
BACKWARD_PAIR_INDEXED = BACKWARD_PAIR + [
    ((4000, 97, 50, 97, P, P, P, P, P, P, P, 1 << 30, None), UNSUPPORTED, "4097 ids"),
    ((4000, 97, 50, 97, P, P, P, P, None, None, P, 1 << 30, None), UNSUPPORTED, "4097 ids, both diffs NULL"),
    ((4000, 97, 50, 97, P, None, P, P, P, P, P, 1 << 30, None), INVALID_ARG, "4097 ids, top_diff0 NULL"),
]
TABLES = {"mms_embed_forward_f16": FORWARD, "mms_embed_backward_f16": BACKWARD, "mms_embed_forward_pair_f16": FORWARD_PAIR,
          "mms_embed_backward_pair_f16": BACKWARD_PAIR, "mms_embed_backward_pair_indexed_f16": BACKWARD_PAIR_INDEXED}
TUPLES = [(name, args, code, what) for name, table in TABLES.items() for args, code, what in table]


@pytest.mark.parametrize("name,args,code,what", TUPLES, ids=["%s: %s" % (t[0][4:], t[3]) for t in TUPLES])
def test_host_side_checks_need_no_gpu(name, args, code, what, hiplib):
    _, argtypes, _, twin = CALLS[name]
    f16, f32 = _entry(hiplib, name, argtypes), _entry(hiplib, twin, argtypes)
    assert f16(*args) == code, what
    assert f32(*args) == code, "%s: %s answers differently" % (what, twin)
