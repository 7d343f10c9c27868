"""mms_embed_simcross_forward_f16 in the C ABI: declared in include/mms.h with its parameter list, exported by the built library, bound in
capi with a wrapper, MMS_VERSION still 212 (the change is additive), and its host-side checks -- which need no GPU -- those of
mms_embed_simcross_forward_f32, argument tuple for argument tuple."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mms_embed_simcross_forward_f16"
DECL = (r"int %s\(int dist_mode, int N, int W1, int W2, int D, int K, const float\* index_q, const float\* index_a, const void\* table_f16, "
        r"const float\* embed_bias, float\* top, float\* norm0, float\* norm1, void\* stream\);")
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2          # include/mms.h


def _header():
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"\s+", " ", txt)


def test_declared_exported_and_bound(hiplib):
    from mms_answer_selection_amd import capi
    assert re.search(DECL % NAME, _header()), "%s is not declared in include/mms.h with the agreed parameter list" % NAME
    assert hasattr(hiplib, NAME), "%s is not exported by libmms_hip.so" % NAME
    assert NAME in capi._SIGNATURES and NAME in capi.EXPORTED_SYMBOLS
    res, args = capi._SIGNATURES[NAME]
    decl = re.search(r"%s\((.*?)\);" % NAME, _header()).group(1)
    assert len(args) == len(decl.split(",")) == 14, "capi binds %d arguments, the header declares %d" % (len(args), len(decl.split(",")))
    assert res is ctypes.c_int


def test_header_comment_names_the_bilinear_call():
    """dist_mode 2 is MMS_ERR_UNSUPPORTED here: the comment in front of the declaration says where it is served."""
    txt = open(os.path.join(ROOT, "include", "mms.h")).read()
    comment = txt[:txt.index("int %s(" % NAME)].rsplit("/*", 1)[1]
    assert "MMS_ERR_UNSUPPORTED" in comment and "mms_embed_simcross_bilinear_forward_f16" in comment


def test_wrapper_exists():
    from mms_answer_selection_amd import capi
    assert callable(capi.embed_simcross_forward_f16)
    assert issubclass(capi.MMSArgumentError, ValueError) and issubclass(capi.MMSArgumentError, capi.MMSError)


def test_version_is_still_212(hiplib):
    from mms_answer_selection_amd import capi
    header = open(os.path.join(ROOT, "include", "mms.h")).read()
    assert re.search(r"#define MMS_VERSION 212\b", header)
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def _entry(hiplib, name):
    f = getattr(hiplib, name)
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.c_void_p] * 8
    return f


# (dist_mode, N, W1, W2, D, K, index_q, index_a, table, embed_bias, top, norm0, norm1, stream): 1 stands for a pointer that is never
# followed -- every tuple is answered before any launch
P = 1
BAD = [
    ((2, 4, 5, 7, 50, 97, P, P, P, None, P, P, P, None), UNSUPPORTED, "dist_mode 2"),
    ((2, 0, 5, 7, 50, 97, None, None, None, None, None, None, None, None), UNSUPPORTED, "dist_mode 2, N == 0"),
    ((1, 4, 5, 7, 50, 0, P, P, P, None, P, None, None, None), INVALID_ARG, "K == 0"),
    ((1, 4, 5, 7, 50, -3, P, P, P, None, P, None, None, None), INVALID_ARG, "K < 0"),
    ((1, 4, 5, 7, 0, 97, P, P, P, None, P, None, None, None), INVALID_ARG, "D == 0"),
    ((0, 4, 0, 7, 50, 97, P, P, P, None, P, P, P, None), INVALID_ARG, "W1 == 0"),
    ((0, 4, 5, -7, 50, 97, P, P, P, None, P, P, P, None), INVALID_ARG, "W2 < 0"),
    ((1, -1, 5, 7, 50, 97, P, P, P, None, P, None, None, None), INVALID_ARG, "N < 0"),
    ((1, 4, 5, 7, 50, (1 << 31) // 50 + 1, P, P, P, None, P, None, None, None), INVALID_ARG, "K * D > 2^31 - 1"),
    ((1, 1 << 20, 64, 7, 50, 97, P, P, P, None, P, None, None, None), INVALID_ARG, "N * W1 * D > 2^31 - 1"),
    ((1, 4, 5, 7, 50, 97, P, P, None, None, P, None, None, None), INVALID_ARG, "table NULL"),
    ((1, 4, 5, 7, 50, 97, None, P, P, None, P, None, None, None), INVALID_ARG, "index_q NULL"),
    ((1, 4, 5, 7, 50, 97, P, None, P, None, P, None, None, None), INVALID_ARG, "index_a NULL"),
    ((0, 4, 5, 7, 50, 97, P, P, P, None, None, P, P, None), INVALID_ARG, "top NULL"),
    ((0, 4, 5, 7, 50, 97, P, P, P, None, P, None, P, None), INVALID_ARG, "cosine: norm0 NULL"),
    ((0, 4, 5, 7, 50, 97, P, P, P, None, P, P, None, None), INVALID_ARG, "cosine: norm1 NULL"),
    ((1, 0, 5, 7, 50, 97, None, None, None, None, None, None, None, None), OK, "N == 0 with NULL pointers"),
    ((0, 0, 1, 1, 1, 1, None, None, None, None, None, None, None, None), OK, "N == 0, cosine"),
]


@pytest.mark.parametrize("args,code,what", BAD, ids=[b[2] for b in BAD])
def test_host_side_checks_need_no_gpu(args, code, what, hiplib):
    f16, f32 = _entry(hiplib, NAME), _entry(hiplib, "mms_embed_simcross_forward_f32")
    assert f16(*args) == code, what
    assert f32(*args) == code, "%s: mms_embed_simcross_forward_f32 answers differently" % what
