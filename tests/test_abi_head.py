"""CPU suite: the classifier-head calls are declared in include/mms_head.h (valid C), exported by the built library and
bound by mms_answer_selection_amd/head.py; include/mms.h, capi.py and the ABI version are as they were; every host-side
rule of the header holds without a GPU -- nothing is enqueued on any of these paths, the arrays are NULL or addresses
that are never touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import head_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
P = 4096                                  # stands for arrays that are never touched: every call here returns first
FORWARDS = ["mms_head_forward_f32", "mms_head_forward_f64", "mms_head_forward_generic_f32"]
BACKWARDS = ["mms_head_backward_f32", "mms_head_backward_f64", "mms_head_backward_generic_f32"]
# positions in the pointer lists
F_X0, F_X1, F_W1, F_B1, F_MASK, F_W2, F_B2, F_LABEL, F_H, F_PROB, F_LOSS = range(11)
B_X0, B_X1, B_W1, B_W2, B_MASK, B_H, B_PROB, B_LABEL = range(8)
BIG = 1 << 40


@pytest.fixture(scope="module")
def head(hiplib):
    from mms_answer_selection_amd import head
    head.lib()
    return head


def _declared():
    txt = open(os.path.join(ROOT, "include", "mms_head.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


def _distinct(n):
    return [P + 64 * i for i in range(n)]


def _shape(head, **kw):
    d = dict(N=50, F0=64, F1=2, H=32, C_=2, phase=head.TRAIN, dropout_ratio=0.5, normalization=head.NORM_VALID,
             ignore_label=None)
    d.update(kw)
    return head.head_shape(**d)


def fwd(fn, sp, ptrs, ws=P, nbytes=BIG):
    return fn(sp, *ptrs, ws, nbytes, None)


def bwd(fn, sp, ins, outs, ws=P, nbytes=BIG, lw=1.0):
    return fn(sp, *ins, lw, *outs, ws, nbytes, None)


def test_every_declared_name_is_exported_and_bound(head, hiplib):
    names = _declared()
    assert len(names) == 9 and all(n.startswith("mms_head_") for n in names), names
    assert sorted(head.EXPORTED_SYMBOLS) == names
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(head.lib(), n).argtypes is not None, n
    for f in ("head_workspace_bytes", "head_route", "head_forward", "head_backward"):
        assert callable(getattr(head, f)) and callable(getattr(head, f + "_f64")), f
    assert callable(head.head_forward_generic) and callable(head.head_backward_generic)
    assert callable(head.head_shape) and issubclass(head.HeadShape, C.Structure)


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "head_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(head, hiplib):
    from mms_answer_selection_amd import capi
    assert "mms_head_" not in open(os.path.join(ROOT, "include", "mms.h")).read()
    assert not [n for n in dir(capi) if n.startswith("head_") or n.startswith("_head_")]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "head" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_the_constants_of_the_header_and_the_binding_agree(head):
    txt = open(os.path.join(ROOT, "include", "mms_head.h")).read()
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(MMS_HEAD_\w+)\s+(\(?-?\d+\)?)", txt)}
    assert defs == dict(MMS_HEAD_TRAIN=head.TRAIN, MMS_HEAD_TEST=head.TEST, MMS_HEAD_NORM_FULL=head.NORM_FULL,
                        MMS_HEAD_NORM_VALID=head.NORM_VALID, MMS_HEAD_NORM_BATCH_SIZE=head.NORM_BATCH_SIZE,
                        MMS_HEAD_NORM_NONE=head.NORM_NONE, MMS_HEAD_PASS_FORWARD=head.PASS_FORWARD,
                        MMS_HEAD_PASS_BACKWARD=head.PASS_BACKWARD, MMS_HEAD_ROUTE_NONE=head.ROUTE_NONE,
                        MMS_HEAD_ROUTE_GENERIC=head.ROUTE_GENERIC, MMS_HEAD_ROUTE_FAST=head.ROUTE_FAST)
    assert (R.TRAIN, R.TEST, R.FULL, R.VALID, R.BATCH_SIZE, R.NONE) == (
        head.TRAIN, head.TEST, head.NORM_FULL, head.NORM_VALID, head.NORM_BATCH_SIZE, head.NORM_NONE)
    # the limits the header states beside mms_head_route are those of the source
    assert "F0 + F1 <= %d, H <= %d and C <= %d" % (R.MAX_F, R.MAX_H, R.MAX_C) in txt


def _bad_shapes(head):
    big = 2 ** 16
    return [_shape(head, N=-1), _shape(head, F0=0), _shape(head, F0=-3), _shape(head, F1=-1), _shape(head, H=0),
            _shape(head, H=-2), _shape(head, C_=0), _shape(head, C_=-1),
            _shape(head, dropout_ratio=0.0), _shape(head, dropout_ratio=1.0), _shape(head, dropout_ratio=-0.5),
            _shape(head, dropout_ratio=1.5), _shape(head, dropout_ratio=float("nan")),
            _shape(head, phase=head.TEST, dropout_ratio=0.0),
            _shape(head, phase=2), _shape(head, phase=-1), _shape(head, normalization=4), _shape(head, normalization=-1),
            _shape(head, N=big, F0=big),                          # x0 over INT_MAX
            _shape(head, N=big, F0=1, F1=big),                    # x1
            _shape(head, N=big, F0=1, F1=0, H=big),               # h
            _shape(head, N=big, F0=1, F1=0, H=1, C_=big),         # prob
            _shape(head, N=1, F0=big, F1=0, H=big),               # w1
            _shape(head, N=1, F0=1, F1=0, H=big, C_=big),         # w2
            _shape(head, N=1, F0=2 ** 31 - 1, F1=1, H=1),         # F0 + F1
            _shape(head, N=0, H=0)]


def test_shape_refusals_in_every_call(head, hiplib):
    for shape in _bad_shapes(head):
        sp = C.byref(shape)
        what = tuple(getattr(shape, f) for f, _ in shape._fields_)
        for p in (0, 1):
            assert hiplib.mms_head_route(sp, p) == head.ROUTE_NONE, what
        assert hiplib.mms_head_workspace_bytes(sp) == 0 and hiplib.mms_head_workspace_bytes_f64(sp) == 0, what
        for name in FORWARDS:
            assert fwd(getattr(hiplib, name), sp, [None] * 11, None, 0) == INVALID, (name, what)
            assert fwd(getattr(hiplib, name), sp, _distinct(11)) == INVALID, (name, what)
        for name in BACKWARDS:
            assert bwd(getattr(hiplib, name), sp, [None] * 8, [None] * 6, None, 0) == INVALID, (name, what)
            assert bwd(getattr(hiplib, name), sp, _distinct(8), _distinct(14)[8:]) == INVALID, (name, what)
    for name in FORWARDS:
        assert fwd(getattr(hiplib, name), None, _distinct(11)) == INVALID
    for name in BACKWARDS:
        assert bwd(getattr(hiplib, name), None, _distinct(8), _distinct(14)[8:]) == INVALID
    assert hiplib.mms_head_route(None, 0) == head.ROUTE_NONE
    assert hiplib.mms_head_workspace_bytes(None) == 0 and hiplib.mms_head_workspace_bytes_f64(None) == 0
    good = _shape(head)
    assert hiplib.mms_head_route(C.byref(good), 2) == head.ROUTE_NONE
    assert hiplib.mms_head_route(C.byref(good), -1) == head.ROUTE_NONE


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_pointer_and_workspace_rules(head, hiplib, name):
    fn = getattr(hiplib, name)
    query = hiplib.mms_head_workspace_bytes_f64 if name.endswith("f64") else hiplib.mms_head_workspace_bytes
    for shape in (_shape(head), _shape(head, N=1517, phase=head.TEST), _shape(head, N=9, F0=200, H=70, C_=20)):
        sp = C.byref(shape)
        need = query(sp)
        assert need > 0
        required = [F_X0, F_X1, F_W1, F_W2, F_H, F_PROB] + ([F_MASK] if shape.phase == head.TRAIN else [])
        for k in required:                            # b1, b2 may be NULL; the mask in TEST; label and loss together
            a = _distinct(11)
            a[k] = None
            assert fwd(fn, sp, a) == INVALID, k
        a = _distinct(11)
        a[F_LABEL] = None                             # a loss without a label
        assert fwd(fn, sp, a) == INVALID
        for out in (F_H, F_PROB, F_LOSS):             # an output that is an input or another output
            for other in range(11):
                if other != out:
                    a = _distinct(11)
                    a[out] = a[other]
                    assert fwd(fn, sp, a) == INVALID, (out, other)
        a = _distinct(11)                             # a loss needs the slabs
        assert fwd(fn, sp, a, None, need) == WORKSPACE
        assert fwd(fn, sp, a, P, need - 1) == WORKSPACE
        assert fwd(fn, sp, a, P, 0) == WORKSPACE
        a[F_W1] = None
        assert fwd(fn, sp, a, None, 0) == INVALID     # arguments are judged before the workspace
    for shape in (_shape(head, N=0), _shape(head, N=0, phase=head.TEST)):
        assert fwd(fn, C.byref(shape), [None] * 11, None, 0) == OK
        assert fwd(fn, C.byref(shape), _distinct(11), None, 0) == OK


@pytest.mark.parametrize("name", BACKWARDS)
def test_backward_pointer_and_workspace_rules(head, hiplib, name):
    fn = getattr(hiplib, name)
    query = hiplib.mms_head_workspace_bytes_f64 if name.endswith("f64") else hiplib.mms_head_workspace_bytes
    for shape in (_shape(head), _shape(head, N=1517, phase=head.TEST), _shape(head, N=9, F0=200, H=70, C_=20)):
        sp = C.byref(shape)
        need = query(sp)
        ins, outs = _distinct(8), _distinct(14)[8:]
        required = [B_X0, B_X1, B_W1, B_W2, B_H, B_PROB, B_LABEL] + ([B_MASK] if shape.phase == head.TRAIN else [])
        for k in required:
            a = list(ins)
            a[k] = None
            assert bwd(fn, sp, a, outs) == INVALID, k
        assert bwd(fn, sp, ins, [None] * 6) == INVALID            # no output asked for
        for o in range(6):
            for other in range(8):                                # an output that is an input
                b = list(outs)
                b[o] = ins[other]
                assert bwd(fn, sp, ins, b) == INVALID, (o, other)
            for o2 in range(o + 1, 6):                            # ... or another output
                b = list(outs)
                b[o2] = b[o]
                assert bwd(fn, sp, ins, b) == INVALID, (o, o2)
        for given in range(6):                                    # every backward needs the workspace
            b = [None] * 6
            b[given] = outs[given]
            assert bwd(fn, sp, ins, b, None, need) == WORKSPACE
            assert bwd(fn, sp, ins, b, P, need - 1) == WORKSPACE
            assert bwd(fn, sp, ins, b, P, 0) == WORKSPACE
            a = list(ins)
            a[B_W2] = None
            assert bwd(fn, sp, a, b, None, 0) == INVALID          # arguments are judged before the workspace
    no_x1 = _shape(head, F1=0)
    b = [None] * 6
    b[1] = P                                                      # x1_diff of no elements is no output
    assert bwd(fn, C.byref(no_x1), _distinct(8), b) == INVALID
    empty = _shape(head, N=0)
    assert bwd(fn, C.byref(empty), [None] * 8, [None] * 6, None, 0) == OK
    assert bwd(fn, C.byref(empty), _distinct(8), _distinct(14)[8:], None, 0) == OK


def test_x1_may_be_null_only_without_columns(head, hiplib):
    """With F1 == 0 a NULL x1 is no refusal: the call gets as far as the workspace check."""
    shape = _shape(head, F1=0)
    a = _distinct(11)
    a[F_X1] = None
    for name in FORWARDS:
        assert fwd(getattr(hiplib, name), C.byref(shape), a, None, 0) == WORKSPACE
    ins = _distinct(8)
    ins[B_X1] = None
    for name in BACKWARDS:
        assert bwd(getattr(hiplib, name), C.byref(shape), ins, _distinct(14)[8:], None, 0) == WORKSPACE


def test_route(head):
    for N in (1, 50, 1517, 65536):
        for phase in (head.TRAIN, head.TEST):
            for s in (R.V4, R.V4_2):
                for p in (head.PASS_FORWARD, head.PASS_BACKWARD):
                    shape = head.head_shape(N, s.F0, s.F1, s.H, s.C, phase)
                    assert head.head_route(shape, p) == head.ROUTE_FAST, (N, s, p)
                    assert head.head_route_f64(shape, p) == head.ROUTE_GENERIC
    for p in (head.PASS_FORWARD, head.PASS_BACKWARD):
        assert head.head_route(head.head_shape(9, R.MAX_F - 2, 2, R.MAX_H, R.MAX_C), p) == head.ROUTE_FAST
        assert head.head_route(head.head_shape(9, R.MAX_F - 1, 2, R.MAX_H, R.MAX_C), p) == head.ROUTE_GENERIC
        assert head.head_route(head.head_shape(9, R.MAX_F + 1, 0, 4, 2), p) == head.ROUTE_GENERIC
        assert head.head_route(head.head_shape(9, 4, 1, R.MAX_H + 1, 2), p) == head.ROUTE_GENERIC
        assert head.head_route(head.head_shape(9, 4, 1, 4, R.MAX_C + 1), p) == head.ROUTE_GENERIC
        for s in R.FAST_SHAPES:
            assert head.head_route(head.head_shape(*s), p) == head.ROUTE_FAST, s
        for s in R.GENERIC_SHAPES:
            assert head.head_route(head.head_shape(*s), p) == head.ROUTE_GENERIC, s


def test_workspace_query(head):
    for s in R.GPU_SHAPES + [R.S(65536, 64, 2, 32, 2), R.S(0, 64, 2, 32, 2)]:
        shape = head.head_shape(*s)
        assert head.head_workspace_bytes(shape) == R.workspace_bytes(s, 4), s
        assert head.head_workspace_bytes_f64(shape) == R.workspace_bytes(s, 8), s
    big = R.S(65537, 2, 1, 3, 2)                              # 205 slabs of five tiles, 20 parameters
    assert big in R.GPU_SHAPES and R.slabs(big.N) == (205, 5) and R.params(big) == 20
    assert head.head_workspace_bytes(head.head_shape(*big)) == R.workspace_bytes(big, 4) == 3088 + 205 * 20 * 4
    assert head.head_workspace_bytes_f64(head.head_shape(*big)) == R.workspace_bytes(big, 8) == 3088 + 205 * 20 * 8


def test_binding_refuses_before_the_library(head):
    import torch
    from mms_answer_selection_amd import capi
    x0, x1, w1, w2 = torch.zeros(5, 8), torch.zeros(5, 2), torch.zeros(4, 10), torch.zeros(3, 4)
    mask, label = torch.ones(5, 4, dtype=torch.int32), torch.zeros(5)
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, torch.zeros(4, 9), None, mask, w2, None)        # w1 does not fit F0 + F1
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, mask, torch.zeros(3, 5), None)        # w2 does not fit H
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, torch.zeros(4, 2), w1, None, mask, w2, None)        # rows of x1
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, None, w2, None)                       # TRAIN without a mask
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, mask, w2, None, loss=torch.zeros(1))  # a loss without a label
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, torch.zeros(5), mask, w2, None)             # b1's shape
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, mask, w2, None, label, prob=torch.zeros(5, 4))
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, mask, w2, None, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        head.head_forward(x0, x1, w1, None, mask, w2, None, phase=3)
    with pytest.raises(capi.MMSArgumentError):
        head.head_backward(x0, x1, w1, w2, mask, torch.zeros(5, 4), torch.zeros(5, 3), label)       # no output
    with pytest.raises(capi.MMSArgumentError):
        head.head_backward(x0, x1, w1, w2, mask, torch.zeros(5, 4), torch.zeros(5, 3), label, w1_diff=torch.zeros(4, 9))
    with pytest.raises(capi.MMSError):
        head.head_forward(x0, x1, w1, None, mask, w2, None)                       # host tensors: there is no CPU path
