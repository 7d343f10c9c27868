"""CPU suite: the TRAIN-phase tail's calls are declared in include/mms_train_tail.h (valid C), exported by the built
library with the declared argument lists and bound by mms_answer_selection_amd/train_tail.py; include/mms.h, capi.py and
the ABI version are as they were; every row of the header's refusal table returns its code without a GPU -- nothing is
enqueued on any of these paths, the arrays are NULL or addresses that are never touched, so a refused call cannot have
written to them -- and the workspace queries follow the header's layout."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import head_reference as HR
import train_tail_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
P = 4096                                  # stands for arrays that are never touched: every call here returns first
BIG = 1 << 40
WS = 64                                   # a workspace address that is none of the arrays'
TRAIN, TEST = 0, 1
FORWARDS = ["mms_train_tail_forward_f32", "mms_train_tail_forward_f64", "mms_train_tail_forward_sequence_f32",
            "mms_train_tail_forward_fused_f32"]
BACKWARDS = ["mms_train_tail_backward_f32", "mms_train_tail_backward_f64"]
QUERIES = ["mms_train_tail_workspace_bytes", "mms_train_tail_workspace_bytes_f64",
           "mms_train_tail_sequence_workspace_bytes", "mms_train_tail_fused_workspace_bytes"]
# the pointer lists, in the header's order
FWD = ("x weight bias scale shift running_mean running_var overlap w1 b1 mask w2 b2 label y flt save_pool save_mean "
       "save_std h prob loss").split()
BWD = ("x weight y flt save_pool scale shift save_mean save_std overlap w1 w2 mask h prob label bottom_diff weight_diff "
       "bias_diff scale_diff shift_diff overlap_diff w1_diff b1_diff w2_diff b2_diff").split()
FWD_OPTIONAL = {"bias", "b1", "b2", "label", "loss"}
BWD_OUTPUTS = BWD[16:]


@pytest.fixture(scope="module")
def tail(hiplib):
    from mms_answer_selection_amd import train_tail
    train_tail.lib()
    return train_tail


def _header():
    return open(os.path.join(ROOT, "include", "mms_train_tail.h")).read()


def _declarations():
    """{name: [parameter type, ...]} of every function the header declares."""
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|size_t)\s+(mms_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
    return out


def _distinct(names):
    return [P + 64 * i for i in range(len(names))]


def _shape(tail, t=None, pool=R.AVE, norm=HR.VALID, ignore_label=None, window=None, **conv_kw):
    from mms_answer_selection_amd import conv
    t = t or R.v4(50)
    s = t.stage.conv
    d = dict(N=s.N, C_=s.C, H=s.H, W=s.W, K=s.K, kernel=(s.kh, s.kw), stride=s.stride, pad=s.pad, group=s.group)
    d.update(conv_kw)
    return tail.train_tail_shape(conv.conv_shape(**d), window or t.stage.pool, pool, t.F1, t.H, t.C, norm, ignore_label)


def fwd(hiplib, name, sp, ptrs, ws=WS, nbytes=BIG, phase=TRAIN, ratio=0.5):
    return getattr(hiplib, name)(sp, phase, 0.9, ratio, *ptrs, ws, nbytes, None)


def bwd(hiplib, name, sp, ptrs, ws=WS, nbytes=BIG, phase=TRAIN, ratio=0.5):
    return getattr(hiplib, name)(sp, phase, ratio, 1.0, *ptrs, ws, nbytes, None)


def every_call(hiplib, sp, fptrs, bptrs, **kw):
    return ([(n, fwd(hiplib, n, sp, fptrs, **kw)) for n in FORWARDS] +
            [(n, bwd(hiplib, n, sp, bptrs, **kw)) for n in BACKWARDS])


def test_every_declared_name_is_exported_with_the_declared_argument_list(tail, hiplib):
    decl = _declarations()
    assert sorted(decl) == sorted(FORWARDS + BACKWARDS + QUERIES + ["mms_train_tail_route"])
    assert sorted(tail.EXPORTED_SYMBOLS) == sorted(decl)
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    ctype = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
    for n, params in decl.items():
        assert hasattr(hiplib, n) and n.encode() in so, n
        bound = getattr(tail.lib(), n).argtypes
        assert len(bound) == len(params), n
        for b, p in zip(bound, params):
            if p == "const mms_score_tail_shape*":
                assert b is C.POINTER(tail.TrainTailShape), (n, p)
            elif p.endswith("*"):
                assert b is C.c_void_p, (n, p)
            else:
                assert b is ctype[p], (n, p)
    for T_, suffix in (("float", "f32"), ("double", "f64")):
        f, b = decl["mms_train_tail_forward_" + suffix], decl["mms_train_tail_backward_" + suffix]
        assert f[:4] == ["const mms_score_tail_shape*", "int", T_, "float"] and len(f) == 4 + len(FWD) + 3
        assert b[:4] == ["const mms_score_tail_shape*", "int", "float", T_] and len(b) == 4 + len(BWD) + 3
        assert f[4 + FWD.index("mask")] == b[4 + BWD.index("mask")] == "const unsigned int*"
        assert f[4 + FWD.index("running_mean")] == T_ + "*" and f[4 + FWD.index("y")] == T_ + "*"
        assert all(b[4 + BWD.index(k)] == T_ + "*" for k in BWD_OUTPUTS)
        assert all(b[4 + i] in ("const %s*" % T_, "const unsigned int*") for i in range(16))
    assert decl["mms_train_tail_forward_sequence_f32"] == decl["mms_train_tail_forward_fused_f32"] == \
        decl["mms_train_tail_forward_f32"]
    for f in ("train_tail_workspace_bytes", "train_tail_route", "train_tail_forward", "train_tail_backward"):
        assert callable(getattr(tail, f)) and callable(getattr(tail, f + "_f64")), f
    assert callable(tail.train_tail_forward_sequence) and callable(tail.train_tail_forward_fused)


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "train_tail_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(tail, hiplib):
    from mms_answer_selection_amd import capi
    assert "mms_train_tail_" not in open(os.path.join(ROOT, "include", "mms.h")).read()
    assert not [n for n in dir(capi) if "train_tail" in n]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "train_tail" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_the_constants_of_the_header_and_the_binding_agree(tail):
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(MMS_T\w+)\s+(\(?-?\d+\)?)", _header())}
    assert defs == dict(MMS_TRAIN_TAIL_ROUTE_NONE=tail.ROUTE_NONE, MMS_TRAIN_TAIL_ROUTE_SEQUENCE=tail.ROUTE_SEQUENCE,
                        MMS_TRAIN_TAIL_ROUTE_FUSED=tail.ROUTE_FUSED)
    assert (R.AVE, R.MAX) == (tail.POOL_AVE, tail.POOL_MAX) and tail.TRAIN == HR.TRAIN == TRAIN
    assert "K + F1 <= %d, H <= %d, C <= %d" % (HR.MAX_F, HR.MAX_H, HR.MAX_C) in _header()


def _refused(tail):
    """(shape, code): what the shape check refuses, with the code the header's order gives it."""
    past = lambda **kw: _shape(tail, R.Tail(R.v4(50).stage, **dict(dict(F1=2, H=32, C=2), **kw)))      # noqa: E731
    big = 2 ** 16
    return [
        (_shape(tail, pool=2), INVALID), (_shape(tail, pool=-1), INVALID),
        (_shape(tail, N=-1), INVALID), (_shape(tail, K=0), INVALID), (_shape(tail, kernel=10), INVALID),
        (_shape(tail, group=3), INVALID), (_shape(tail, dilation=2, H=13, W=13), UNSUPPORTED),
        (_shape(tail, window=(2, 5)), INVALID), (_shape(tail, window=(5, 0)), INVALID), (_shape(tail, window=(3, 3)), INVALID),
        (_shape(tail, window=(1, 1)), INVALID), (_shape(tail, window=(5, 1)), INVALID),       # tile the map, not whole
        (_shape(tail, R.NOT_WHOLE_MAP), INVALID),
        (past(F1=-1), INVALID), (past(H=0), INVALID), (past(C=0), INVALID), (past(C=-2), INVALID),
        (_shape(tail, norm=4), INVALID), (_shape(tail, norm=-1), INVALID),
        (_shape(tail, R.Tail(R.v4(big).stage, big, 32, 2)), INVALID),             # overlap over INT_MAX elements
        (_shape(tail, R.Tail(R.v4(big).stage, 2, big, 2)), INVALID),              # h
        (_shape(tail, N=0, pool=7), INVALID),                                     # N == 0 excuses no shape
    ]


def test_shape_refusals_in_every_call(tail, hiplib):
    for shape, code in _refused(tail):
        sp = C.byref(shape)
        what = tuple(getattr(shape.conv, f) for f, _ in shape.conv._fields_) + tuple(
            getattr(shape, f) for f, _ in shape._fields_[1:])
        assert hiplib.mms_train_tail_route(sp) == tail.ROUTE_NONE, what
        for q in QUERIES:
            assert getattr(hiplib, q)(sp) == 0, (q, what)
        for n, rc in every_call(hiplib, sp, [None] * len(FWD), [None] * len(BWD), ws=None, nbytes=0):
            assert rc == code, (n, what)
        for n, rc in every_call(hiplib, sp, _distinct(FWD), _distinct(BWD)):
            assert rc == code, (n, what)
    for n, rc in every_call(hiplib, None, _distinct(FWD), _distinct(BWD)):
        assert rc == INVALID, n
    assert hiplib.mms_train_tail_route(None) == tail.ROUTE_NONE
    assert all(getattr(hiplib, q)(None) == 0 for q in QUERIES)


def test_phase_and_dropout_ratio(tail, hiplib):
    """phase must be TRAIN; dropout_ratio is the head's rule, (0, 1).  Both before the pointers and the workspace."""
    sp = C.byref(_shape(tail))
    for kw in (dict(phase=TEST), dict(phase=2), dict(phase=-1), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=-0.5)):
        for n, rc in every_call(hiplib, sp, [None] * len(FWD), [None] * len(BWD), ws=None, nbytes=0, **kw):
            assert rc == INVALID, (n, kw)
        for n, rc in every_call(hiplib, sp, _distinct(FWD), _distinct(BWD), **kw):
            assert rc == INVALID, (n, kw)


def test_which_code_wins(tail, hiplib):
    """The header's order: the pool, the convolution (its UNSUPPORTED included), the window, the phase, the head's
    widths; then the pointers; then, for the forced fused call, UNSUPPORTED; then the workspace."""
    dilated = lambda **kw: _shape(tail, dilation=2, H=13, W=13, **kw)               # noqa: E731: a 5 x 5 map
    bad_pool, bad_window, bad_head = dilated(pool=9), dilated(window=(2, 2)), dilated()
    bad_head.H = 0
    f, b = _distinct(FWD), _distinct(BWD)
    for n, rc in every_call(hiplib, C.byref(bad_pool), f, b):
        assert rc == INVALID, n                                                    # the pool before the convolution
    for shape in (dilated(), bad_window, bad_head):
        for n, rc in every_call(hiplib, C.byref(shape), f, b):
            assert rc == UNSUPPORTED, n                                            # the convolution before the rest
        for n, rc in every_call(hiplib, C.byref(shape), f, b, phase=TEST):
            assert rc == UNSUPPORTED, n
    past = _shape(tail, R.PAST_H)                                                  # not reached by the fused launches
    for name in FORWARDS:
        a = _distinct(FWD)
        a[FWD.index("w1")] = None                     # a pointer before UNSUPPORTED and before the workspace
        assert fwd(hiplib, name, C.byref(past), a, None, 0) == INVALID, name
        a = _distinct(FWD)
        a[FWD.index("y")] = a[FWD.index("x")]         # an alias before UNSUPPORTED and before the workspace
        assert fwd(hiplib, name, C.byref(past), a, None, 0) == INVALID, name
    fused = "mms_train_tail_forward_fused_f32"
    for t in R.SEQUENCE_TAILS:
        for pool in R.POOLS:
            assert fwd(hiplib, fused, C.byref(_shape(tail, t, pool)), _distinct(FWD), None, 0) == UNSUPPORTED, t
            assert hiplib.mms_train_tail_fused_workspace_bytes(C.byref(_shape(tail, t, pool))) == 0
            assert tail.train_tail_route(_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE


TAILS = ((R.v4(50), R.AVE), (R.v4(1517), R.MAX), (R.v5(7), R.MAX), (R.small(5), R.AVE))


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_pointer_and_workspace_rules(tail, hiplib, name):
    query = {"mms_train_tail_forward_f32": "mms_train_tail_workspace_bytes",
             "mms_train_tail_forward_f64": "mms_train_tail_workspace_bytes_f64",
             "mms_train_tail_forward_sequence_f32": "mms_train_tail_sequence_workspace_bytes",
             "mms_train_tail_forward_fused_f32": "mms_train_tail_fused_workspace_bytes"}[name]
    for t, pool in TAILS:
        sp = C.byref(_shape(tail, t, pool))
        need = getattr(hiplib, query)(sp)
        assert need > 0
        for k in FWD:
            a = _distinct(FWD)
            a[FWD.index(k)] = None
            if k in FWD_OPTIONAL - {"label"}:
                continue                               # a valid call: not made without a GPU
            assert fwd(hiplib, name, sp, a) == INVALID, k             # label == NULL with a loss included
        for i in range(len(FWD)):                     # any two arrays at one address, the workspace included
            for j in range(i):
                a = _distinct(FWD)
                a[i] = a[j]
                assert fwd(hiplib, name, sp, a) == INVALID, (FWD[i], FWD[j])
            a = _distinct(FWD)
            assert fwd(hiplib, name, sp, a, a[i], BIG) == INVALID, FWD[i]
        a = _distinct(FWD)
        assert fwd(hiplib, name, sp, a, None, need) == WORKSPACE
        assert fwd(hiplib, name, sp, a, WS, need - 1) == WORKSPACE
        assert fwd(hiplib, name, sp, a, WS, 0) == WORKSPACE
        a[FWD.index("w2")] = None
        assert fwd(hiplib, name, sp, a, None, 0) == INVALID           # arguments are judged before the workspace
    for t in (R.v4(0), R.small(0)):
        sp = C.byref(_shape(tail, t))
        assert fwd(hiplib, name, sp, [None] * len(FWD), None, 0) == OK
        assert fwd(hiplib, name, sp, _distinct(FWD), None, 0) == OK


@pytest.mark.parametrize("name", BACKWARDS)
def test_backward_pointer_and_workspace_rules(tail, hiplib, name):
    query = "mms_train_tail_workspace_bytes" + ("_f64" if name.endswith("f64") else "")
    for t, pool in TAILS:
        sp = C.byref(_shape(tail, t, pool))
        need = getattr(hiplib, query)(sp)
        for k in BWD[:16]:
            a = _distinct(BWD)
            a[BWD.index(k)] = None
            if k == "shift" and pool == R.AVE:
                continue                               # a valid call: not made without a GPU
            assert bwd(hiplib, name, sp, a) == INVALID, k
        a = _distinct(BWD)
        for k in BWD_OUTPUTS:
            a[BWD.index(k)] = None
        assert bwd(hiplib, name, sp, a) == INVALID                    # no output at all
        for i in range(len(BWD)):
            for j in range(i):
                a = _distinct(BWD)
                a[i] = a[j]
                assert bwd(hiplib, name, sp, a) == INVALID, (BWD[i], BWD[j])
            a = _distinct(BWD)
            assert bwd(hiplib, name, sp, a, a[i], BIG) == INVALID, BWD[i]
        a = _distinct(BWD)
        assert bwd(hiplib, name, sp, a, None, need) == WORKSPACE
        assert bwd(hiplib, name, sp, a, WS, need - 1) == WORKSPACE
        a[BWD.index("prob")] = None
        assert bwd(hiplib, name, sp, a, None, 0) == INVALID
    # with F1 == 0 overlap may be NULL and overlap_diff is an array of no elements: alone it is no output
    t0 = R.T(3, 3, 6, 6, 5, 3, 3, (4, 4), 0, 5, 2)
    a = _distinct(BWD)
    a[BWD.index("overlap")] = None
    assert bwd(hiplib, name, C.byref(_shape(tail, t0)), a, None, 0) == WORKSPACE
    for k in BWD_OUTPUTS:
        if k != "overlap_diff":
            a[BWD.index(k)] = None
    assert bwd(hiplib, name, C.byref(_shape(tail, t0)), a) == INVALID
    for t in (R.v4(0), R.small(0)):
        assert bwd(hiplib, name, C.byref(_shape(tail, t)), [None] * len(BWD), None, 0) == OK


def test_overlap_may_be_null_only_without_columns(tail, hiplib):
    t0 = R.T(3, 3, 6, 6, 5, 3, 3, (4, 4), 0, 5, 2)
    a = _distinct(FWD)
    a[FWD.index("overlap")] = None
    for name in FORWARDS:
        assert fwd(hiplib, name, C.byref(_shape(tail, t0)), a, None, 0) == WORKSPACE, name


def test_route_table(tail):
    for shape, _ in _refused(tail):
        assert tail.train_tail_route(shape) == tail.ROUTE_NONE and tail.train_tail_route_f64(shape) == tail.ROUTE_NONE
    for pool in R.POOLS:
        for t in R.GPU_TAILS + [R.v4(100), R.v4(400), R.v4(1517), R.v5(1517)]:
            r = tail.train_tail_route(_shape(tail, t, pool))
            assert r in (tail.ROUTE_SEQUENCE, tail.ROUTE_FUSED), (t, pool)
            assert r == tail.ROUTE_SEQUENCE or t in R.FUSED_TAILS or t.stage.conv.N > 65
            assert tail.train_tail_route_f64(_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE
        # the measured span (tools/bench_train_tail.py): 50 to 100 workgroups of one image
        for N, want in ((1, tail.ROUTE_SEQUENCE), (49, tail.ROUTE_SEQUENCE), (50, tail.ROUTE_FUSED), (65, tail.ROUTE_FUSED),
                        (100, tail.ROUTE_FUSED), (101, tail.ROUTE_SEQUENCE), (400, tail.ROUTE_SEQUENCE),
                        (1517, tail.ROUTE_SEQUENCE)):
            for t in (R.v4(N), R.v5(N), R.small(N)):
                assert tail.train_tail_route(_shape(tail, t, pool)) == want, (t, pool)
            assert tail.train_tail_route(_shape(tail, R.Tail(R.v4(N).stage, 2, HR.MAX_H + 1, 2), pool)) == tail.ROUTE_SEQUENCE


def test_workspace_queries(tail, hiplib):
    """The header's layout: [stage][x0_diff][head], each rounded up to 16 bytes; FUSED: the larger of that and
    [partials][loss]."""
    from mms_answer_selection_amd import conv_stage_train, head
    r16 = lambda v: (v + 15) // 16 * 16                                             # noqa: E731
    for pool in R.POOLS:
        for t in R.GPU_TAILS + [R.v4(1517), R.v5(1517)]:
            shape, hs, N = _shape(tail, t, pool), R.head_shape(t), t.stage.conv.N
            hshape = head.head_shape(*hs, phase=head.TRAIN)
            m = R.METHOD[pool]
            want32 = (r16(conv_stage_train.conv_stage_train_workspace_bytes(shape.conv, t.stage.pool, m)) +
                      r16(N * hs.F0 * 4) + r16(head.head_workspace_bytes(hshape)))
            want64 = (r16(conv_stage_train.conv_stage_train_workspace_bytes_f64(shape.conv, t.stage.pool, m)) +
                      r16(N * hs.F0 * 8) + r16(head.head_workspace_bytes_f64(hshape)))
            assert tail.train_tail_workspace_bytes(shape, "sequence") == want32, (t, pool)
            assert tail.train_tail_workspace_bytes_f64(shape) == want64, (t, pool)
            assert tail.train_tail_workspace_bytes_f64(shape, "sequence") == want64, (t, pool)
            groups = -(-N // R.IMAGES)
            fused = max(want32, r16(2 * hs.F0 * groups * 4) + r16(8 * N)) if t in R.FUSED_TAILS or N > 65 else 0
            assert tail.train_tail_workspace_bytes(shape, "fused") == fused, (t, pool)
            routed = tail.train_tail_route(shape) == tail.ROUTE_FUSED
            assert tail.train_tail_workspace_bytes(shape) == (fused if routed else want32), (t, pool)
        for q in QUERIES:
            assert getattr(hiplib, q)(C.byref(_shape(tail, R.v4(0), pool))) == 0


def test_binding_refuses_before_the_library(tail):
    import torch
    from mms_answer_selection_amd import capi
    x, w, k = torch.zeros(3, 2, 3, 3), torch.zeros(3, 2, 2, 2), torch.zeros(3)
    ov, w1, w2, mask = torch.zeros(3, 2), torch.zeros(4, 5), torch.zeros(2, 4), torch.zeros(3, 4, dtype=torch.int32)
    f = lambda **kw: tail.train_tail_forward(**dict(dict(                            # noqa: E731
        x=x, weight=w, bias=None, pool_window=2, pool=tail.POOL_AVE, scale=k, shift=k, running_mean=k, running_var=k,
        overlap=ov, w1=w1, b1=None, mask=mask, w2=w2, b2=None), **kw))
    for bad in (dict(pool_window=1), dict(w1=torch.zeros(4, 6)), dict(w2=torch.zeros(2, 5)), dict(overlap=torch.zeros(2, 2)),
                dict(b1=torch.zeros(5)), dict(scale=torch.zeros(4)), dict(prob=torch.zeros(3, 3)), dict(h=torch.zeros(3, 5)),
                dict(flt=torch.zeros(3, 4)), dict(y=torch.zeros(3, 3, 2, 1)), dict(mask=None),
                dict(mask=torch.zeros(3, 5, dtype=torch.int32)), dict(loss=torch.zeros(2), label=torch.zeros(3)),
                dict(route="fast")):
        with pytest.raises(capi.MMSArgumentError):
            f(**bad)
    with pytest.raises(capi.MMSArgumentError):
        tail.train_tail_forward_f64(x.double(), w.double(), None, 2, tail.POOL_AVE, k, k, k, k, ov, w1, None, mask, w2,
                                    None, route="fused")
    with pytest.raises(capi.MMSError):
        f()                                           # host tensors: there is no CPU path
