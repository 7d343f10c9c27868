"""CPU suite: the Convolution calls are declared in include/mms_conv.h (valid C), exported by the built library and
bound by mms_answer_selection_amd/conv.py; include/mms.h, capi.py and the ABI version are as they were; every
host-side rule of the header holds without a GPU -- nothing is enqueued on any of these paths, the arrays are NULL or
addresses that are never touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import conv_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
P = 4096                                  # stands for arrays that are never touched: every call here returns first
FORWARDS = ["mms_conv_forward_f32", "mms_conv_forward_f64", "mms_conv_forward_generic_f32"]
BACKWARDS = ["mms_conv_backward_f32", "mms_conv_backward_f64", "mms_conv_backward_generic_f32"]
V4 = [(4, 40, 40, 32), (32, 9, 9, 64)]    # (C, H, W, K) of network_v4's two layers, 5 x 5


@pytest.fixture(scope="module")
def conv(hiplib):
    from mms_answer_selection_amd import conv
    conv.lib()
    return conv


def _declared():
    txt = open(os.path.join(ROOT, "include", "mms_conv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


def _distinct(n):
    return [P + 64 * i for i in range(n)]


def test_every_declared_name_is_exported_and_bound(conv, hiplib):
    names = _declared()
    assert len(names) == 10 and all(n.startswith("mms_conv_") for n in names), names
    assert sorted(conv.EXPORTED_SYMBOLS) == names
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(conv.lib(), n).argtypes is not None, n
    for f in ("conv_output_dims", "conv_workspace_bytes", "conv_route", "conv_forward", "conv_backward"):
        assert callable(getattr(conv, f)) and callable(getattr(conv, f + "_f64")), f


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "conv_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(conv, hiplib):
    from mms_answer_selection_amd import capi
    assert "mms_conv_" not in open(os.path.join(ROOT, "include", "mms.h")).read()
    assert not [n for n in dir(capi) if n.startswith("conv_") or n.startswith("_conv_")]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "conv" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


@pytest.mark.parametrize("s", R.GPU_SHAPES + [R.S(1, 1, 11, 11, 1, 4, 3, stride=(3, 2))], ids=str)
def test_output_dims_match_the_reference_formula(conv, s):
    shape = conv.conv_shape(s.N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group)
    assert conv.conv_output_dims(shape) == R.output_dims(s)


def test_output_dims_with_rows_left_over(conv):
    # (10 + 2 - 3) / 2 = 4.5: the last row and column of the padded image are never the top-left of a window
    assert conv.conv_output_dims(conv.conv_shape(2, 3, 10, 10, 4, 3, stride=2, pad=1)) == (5, 5)
    assert conv.conv_output_dims(conv.conv_shape(2, 3, 11, 11, 4, 4, stride=3)) == (3, 3)      # 7 / 3 = 2.33


def _shape(conv, **kw):
    d = dict(N=2, C_=4, H=12, W=12, K=6, kernel=3, stride=1, pad=0, group=1, dilation=1)
    d.update(kw)
    return conv.conv_shape(**d)


def _bad_shapes(conv):
    big = 2 ** 16
    return [(_shape(conv, N=-1), INVALID), (_shape(conv, C_=0), INVALID), (_shape(conv, C_=-4), INVALID),
            (_shape(conv, H=0), INVALID), (_shape(conv, W=-1), INVALID), (_shape(conv, K=0), INVALID),
            (_shape(conv, kernel=(0, 3)), INVALID), (_shape(conv, kernel=(3, -1)), INVALID),
            (_shape(conv, stride=(0, 1)), INVALID), (_shape(conv, stride=(1, -2)), INVALID),
            (_shape(conv, group=0), INVALID), (_shape(conv, group=-1), INVALID),
            (_shape(conv, dilation=(0, 1)), INVALID), (_shape(conv, dilation=(1, -1)), INVALID),
            (_shape(conv, pad=(-1, 0)), INVALID), (_shape(conv, pad=(0, -1)), INVALID),
            (_shape(conv, group=3), INVALID),                         # 4 % 3
            (_shape(conv, C_=6, K=4, group=3), INVALID),              # 4 % 3 on the output side
            (_shape(conv, kernel=13), INVALID), (_shape(conv, kernel=(3, 13)), INVALID),      # an empty output
            (_shape(conv, N=big, C_=big, H=1, W=1, kernel=1), INVALID),                       # N*C > INT_MAX
            (_shape(conv, N=8, C_=big, H=big, W=1, kernel=1), INVALID),                       # bottom over INT_MAX
            (_shape(conv, N=big, C_=1, H=182, W=182, K=1, kernel=1), INVALID),                # 2^16 * 182^2 > 2^31
            (_shape(conv, N=1, C_=1, H=4, W=4, K=2 ** 30, kernel=3, pad=1), INVALID),         # top over INT_MAX
            (_shape(conv, N=1, C_=big, H=3, W=3, K=big, kernel=3), INVALID),                  # weight over INT_MAX
            (_shape(conv, dilation=2), UNSUPPORTED), (_shape(conv, dilation=(1, 2)), UNSUPPORTED),
            (_shape(conv, N=0, dilation=2), UNSUPPORTED)]


def test_shape_refusals_in_every_call(conv, hiplib):
    oh, ow = C.c_int(-7), C.c_int(-7)
    for shape, code in _bad_shapes(conv):
        sp = C.byref(shape)
        what = tuple(getattr(shape, f) for f, _ in shape._fields_)
        assert hiplib.mms_conv_output_dims(sp, C.byref(oh), C.byref(ow)) == code, what
        assert (oh.value, ow.value) == (-7, -7)
        assert hiplib.mms_conv_route(sp, 0) == conv.ROUTE_NONE, what
        assert hiplib.mms_conv_workspace_bytes(sp) == 0 and hiplib.mms_conv_workspace_bytes_f64(sp) == 0, what
        for name in FORWARDS:
            assert getattr(hiplib, name)(sp, None, None, None, None, None, 0, None) == code, (name, what)
            assert getattr(hiplib, name)(sp, *_distinct(4), P, 1 << 40, None) == code, (name, what)
        for name in BACKWARDS:
            assert getattr(hiplib, name)(sp, None, None, None, None, None, None, None, 0, None) == code, (name, what)
            assert getattr(hiplib, name)(sp, *_distinct(6), P, 1 << 40, None) == code, (name, what)
    for name in FORWARDS:
        assert getattr(hiplib, name)(None, *_distinct(4), P, 1 << 40, None) == INVALID
    for name in BACKWARDS:
        assert getattr(hiplib, name)(None, *_distinct(6), P, 1 << 40, None) == INVALID
    assert hiplib.mms_conv_output_dims(None, C.byref(oh), C.byref(ow)) == INVALID
    assert hiplib.mms_conv_route(None, 0) == conv.ROUTE_NONE and hiplib.mms_conv_workspace_bytes(None) == 0
    good = _shape(conv)
    assert hiplib.mms_conv_route(C.byref(good), 3) == conv.ROUTE_NONE
    assert hiplib.mms_conv_route(C.byref(good), -1) == conv.ROUTE_NONE


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_pointer_rules(conv, hiplib, name):
    fn = getattr(hiplib, name)
    for shape in (_shape(conv), _shape(conv, stride=2, pad=1)):
        sp = C.byref(shape)
        for k in (0, 1, 3):                           # x, weight, top; the bias may be NULL
            a = _distinct(4)
            a[k] = None
            assert fn(sp, *a, None, 0, None) == INVALID, k
        a = _distinct(4)
        a[3] = a[0]
        assert fn(sp, *a, None, 0, None) == INVALID   # top == x
    empty = _shape(conv, N=0)
    assert fn(C.byref(empty), None, None, None, None, None, 0, None) == OK
    assert fn(C.byref(empty), *_distinct(4), None, 0, None) == OK


@pytest.mark.parametrize("name", BACKWARDS)
def test_backward_pointer_and_workspace_rules(conv, hiplib, name):
    fn = getattr(hiplib, name)
    query = hiplib.mms_conv_workspace_bytes_f64 if name.endswith("f64") else hiplib.mms_conv_workspace_bytes
    for shape in (_shape(conv), _shape(conv, stride=2, pad=1), _shape(conv, C_=32, H=9, W=9, K=64, kernel=5)):
        sp = C.byref(shape)
        need = query(sp)
        assert need > 0
        for k in range(3):                            # x, weight, top_diff
            a = _distinct(6)
            a[k] = None
            assert fn(sp, *a, P, need, None) == INVALID, k
        assert fn(sp, *(_distinct(3) + [None] * 3), P, need, None) == INVALID        # no output asked for
        for other in (0, 2):                          # bottom_diff aliasing x, top_diff
            a = _distinct(6)
            a[3] = a[other]
            assert fn(sp, *a, P, need, None) == INVALID, other
        for given in (4, 5):                          # a parameter diff needs the slabs
            a = _distinct(3) + [None] * 3
            a[given] = P + 64 * given
            assert fn(sp, *a, None, need, None) == WORKSPACE
            assert fn(sp, *a, P, need - 1, None) == WORKSPACE
            assert fn(sp, *a, P, 0, None) == WORKSPACE
            a[1] = None
            assert fn(sp, *a, None, 0, None) == INVALID      # arguments are judged before the workspace
    empty = _shape(conv, N=0)
    assert fn(C.byref(empty), *([None] * 6), None, 0, None) == OK
    assert fn(C.byref(empty), *_distinct(6), None, 0, None) == OK


def test_route(conv):
    for N in (1, 3, 50, 1517):
        for (C_, H, W, K) in V4:
            shape = conv.conv_shape(N, C_, H, W, K, 5)
            for p in (conv.PASS_FORWARD, conv.PASS_BOTTOM_DIFF, conv.PASS_PARAM_DIFF):
                assert conv.conv_route(shape, p) == conv.ROUTE_FAST, (N, C_, p)
                assert conv.conv_route_f64(shape, p) == conv.ROUTE_GENERIC
                for other in (dict(stride=2), dict(pad=2), dict(group=2), dict(stride=(1, 2)), dict(pad=(0, 1))):
                    assert conv.conv_route(conv.conv_shape(N, C_, H, W, K, 5, **other), p) == conv.ROUTE_GENERIC, other
    for p in range(3):
        assert conv.conv_route(conv.conv_shape(2, 65, 9, 9, 8, 3), p) == conv.ROUTE_GENERIC      # more than 64 channels
        assert conv.conv_route(conv.conv_shape(2, 8, 9, 9, 65, 3), p) == conv.ROUTE_GENERIC


def test_the_gpu_list_reaches_both_routes_in_every_pass(conv):
    for p in range(3):
        routes = {conv.conv_route(conv.conv_shape(s.N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group), p)
                  for s in R.GPU_SHAPES}
        assert routes == {conv.ROUTE_FAST, conv.ROUTE_GENERIC}, p


def test_workspace_query(conv):
    for (C_, H, W, K) in V4:
        nW = K * C_ * 25
        for q, item in ((conv.conv_workspace_bytes, 4), (conv.conv_workspace_bytes_f64, 8)):
            assert q(conv.conv_shape(0, C_, H, W, K, 5)) == 0
            sizes = [q(conv.conv_shape(N, C_, H, W, K, 5)) for N in (1, 2, 3, 50, 64, 65, 1517, 5000)]
            assert all(b > 0 for b in sizes)
            for b in sizes:
                assert b % ((nW + K) * item) == 0 and 1 <= b // ((nW + K) * item) <= 64      # slabs of (weights, bias)
    assert conv.conv_workspace_bytes(conv.conv_shape(2, 4, 7, 7, 6, 3, group=2)) % ((6 * 2 * 9 + 6) * 4) == 0


def test_binding_refuses_before_the_library(conv):
    import torch
    from mms_answer_selection_amd import capi
    x, w = torch.zeros(2, 4, 8, 8), torch.zeros(6, 4, 3, 3)
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, torch.zeros(6, 3, 3, 3))                 # weight does not fit the channels
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, w, group=3)
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, torch.zeros(6, 4, 9, 9))                 # an empty output
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, w, top=torch.zeros(2, 6, 5, 6))          # top's shape
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, w, bias=torch.zeros(5))
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_forward(x, w, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_backward(x, w, torch.zeros(2, 6, 6, 6))             # no output
    with pytest.raises(capi.MMSArgumentError):
        conv.conv_backward(x, w, torch.zeros(2, 6, 6, 6), weight_diff=torch.zeros(6, 4, 3, 2))
    with pytest.raises(capi.MMSError):
        conv.conv_forward(x, w)                                       # host tensors: there is no CPU path
