"""CPU suite: the scoring-tail calls are declared in include/mms_score_tail.h (valid C), exported by the built library and
bound by mms_answer_selection_amd/score_tail.py; include/mms.h, capi.py and the ABI version are as they were; every
host-side rule of the header holds without a GPU -- nothing is enqueued on any of these paths, the arrays are NULL or
addresses that are never touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import head_reference as HR
import score_tail_reference as R
from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
P = 4096                                  # stands for arrays that are never touched: every call here returns first
BIG = 1 << 40
CALLS = ["mms_score_tail_forward_f32", "mms_score_tail_forward_f64", "mms_score_tail_forward_sequence_f32",
         "mms_score_tail_forward_fused_f32"]
QUERIES = ["mms_score_tail_workspace_bytes", "mms_score_tail_workspace_bytes_f64",
           "mms_score_tail_sequence_workspace_bytes"]
# positions in the pointer list
X, WEIGHT, BIAS, MEAN, VAR, SCALE, SHIFT, OVERLAP, W1, B1, W2, B2, LABEL, FLT, H, PROB, LOSS = range(17)
OUTPUTS = (FLT, H, PROB, LOSS)


@pytest.fixture(scope="module")
def tail(hiplib):
    from mms_answer_selection_amd import score_tail
    score_tail.lib()
    return score_tail


def _declared():
    txt = open(os.path.join(ROOT, "include", "mms_score_tail.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


def _distinct(n=17):
    return [P + 64 * i for i in range(n)]


def _shape(tail, t=None, pool=R.AVE, norm=HR.VALID, ignore_label=None, window=None, **conv_kw):
    from mms_answer_selection_amd import conv
    t = t or R.v4(50)
    s = t.stage.conv
    d = dict(N=s.N, C_=s.C, H=s.H, W=s.W, K=s.K, kernel=(s.kh, s.kw), stride=s.stride, pad=s.pad, group=s.group)
    d.update(conv_kw)
    return tail.score_tail_shape(conv.conv_shape(**d), window or t.stage.pool, pool, t.F1, t.H, t.C, norm, ignore_label)


def call(fn, sp, ptrs, ws=P, nbytes=BIG):
    return fn(sp, *ptrs, ws, nbytes, None)


def test_every_declared_name_is_exported_and_bound(tail, hiplib):
    names = _declared()
    assert names == sorted(CALLS + QUERIES + ["mms_score_tail_route"])
    assert sorted(tail.EXPORTED_SYMBOLS) == names
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(tail.lib(), n).argtypes is not None, n
    for f in ("score_tail_workspace_bytes", "score_tail_route", "score_tail_forward"):
        assert callable(getattr(tail, f)) and callable(getattr(tail, f + "_f64")), f
    assert callable(tail.score_tail_forward_sequence) and callable(tail.score_tail_forward_fused)
    assert callable(tail.score_tail_shape) and issubclass(tail.ScoreTailShape, C.Structure)


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "score_tail_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(tail, hiplib):
    from mms_answer_selection_amd import capi
    assert "mms_score_tail_" not in open(os.path.join(ROOT, "include", "mms.h")).read()
    assert not [n for n in dir(capi) if "score_tail" in n]
    assert not [n for n in capi.EXPORTED_SYMBOLS if "score_tail" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_the_constants_of_the_header_and_the_binding_agree(tail):
    txt = open(os.path.join(ROOT, "include", "mms_score_tail.h")).read()
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(MMS_S\w+)\s+(\(?-?\d+\)?)", txt)}
    assert defs == dict(MMS_STAGE_POOL_AVE=tail.POOL_AVE, MMS_STAGE_POOL_MAX=tail.POOL_MAX,
                        MMS_SCORE_TAIL_ROUTE_NONE=tail.ROUTE_NONE, MMS_SCORE_TAIL_ROUTE_SEQUENCE=tail.ROUTE_SEQUENCE,
                        MMS_SCORE_TAIL_ROUTE_FUSED=tail.ROUTE_FUSED)
    assert (R.AVE, R.MAX) == (tail.POOL_AVE, tail.POOL_MAX)
    assert (HR.FULL, HR.VALID, HR.BATCH_SIZE, HR.NONE) == (tail.NORM_FULL, tail.NORM_VALID, tail.NORM_BATCH_SIZE,
                                                           tail.NORM_NONE)
    # the limits the header states are the head's
    assert "K + F1 <= %d, H <= %d, C <= %d" % (HR.MAX_F, HR.MAX_H, HR.MAX_C) in txt


def _refused(tail):
    """(shape, code): what tail_check refuses, with the code the header's order gives it."""
    past = lambda **kw: _shape(tail, R.Tail(R.v4(50).stage, **dict(dict(F1=2, H=32, C=2), **kw)))
    big = 2 ** 16
    return [
        (_shape(tail, pool=2), INVALID), (_shape(tail, pool=-1), INVALID),
        (_shape(tail, N=-1), INVALID), (_shape(tail, K=0), INVALID), (_shape(tail, kernel=10), INVALID),
        (_shape(tail, group=3), INVALID),
        (_shape(tail, window=(2, 5)), INVALID), (_shape(tail, window=(5, 0)), INVALID), (_shape(tail, window=(3, 3)), INVALID),
        (past(F1=-1), INVALID), (past(H=0), INVALID), (past(C=0), INVALID), (past(C=-2), INVALID),
        (_shape(tail, norm=4), INVALID), (_shape(tail, norm=-1), INVALID),
        (_shape(tail, R.Tail(R.v4(big).stage, big, 32, 2)), INVALID),             # overlap over INT_MAX elements
        (_shape(tail, R.Tail(R.v4(big).stage, 2, big, 2)), INVALID),              # h
        (_shape(tail, N=0, pool=7), INVALID),                                     # N == 0 excuses no shape
    ]


def test_shape_refusals_in_every_call(tail, hiplib):
    for shape, code in _refused(tail):
        sp = C.byref(shape)
        what = tuple(shape.conv.__getattribute__(f) for f, _ in shape.conv._fields_) + tuple(
            getattr(shape, f) for f, _ in shape._fields_[1:])
        assert hiplib.mms_score_tail_route(sp) == tail.ROUTE_NONE, what
        for q in QUERIES:
            assert getattr(hiplib, q)(sp) == 0, (q, what)
        for name in CALLS:
            assert call(getattr(hiplib, name), sp, [None] * 17, None, 0) == code, (name, what)
            assert call(getattr(hiplib, name), sp, _distinct()) == code, (name, what)
    for name in CALLS:
        assert call(getattr(hiplib, name), None, _distinct()) == INVALID
    assert hiplib.mms_score_tail_route(None) == tail.ROUTE_NONE
    assert all(getattr(hiplib, q)(None) == 0 for q in QUERIES)


def test_which_code_wins(tail, hiplib):
    """The header's order: the pool, the convolution (its UNSUPPORTED included), the window, the head's widths; then the
    pointers; then, for the forced fused call, UNSUPPORTED; then the workspace."""
    def dilated(**kw):                                          # 13 - (2 * 4 + 1) + 1 = 5: the only fault is the dilation
        s = _shape(tail, dilation=2, H=13, W=13, **kw)
        return s
    bad_pool, bad_window, bad_head = dilated(pool=9), dilated(window=(2, 2)), dilated()
    bad_head.H = 0
    past = _shape(tail, R.PAST[1])                              # not reached by the fused launch
    for name in CALLS:
        fn = getattr(hiplib, name)
        assert call(fn, C.byref(dilated()), _distinct()) == UNSUPPORTED, name
        assert call(fn, C.byref(bad_pool), _distinct()) == INVALID, name           # the pool before the convolution
        assert call(fn, C.byref(bad_window), _distinct()) == UNSUPPORTED, name     # the convolution before the window
        assert call(fn, C.byref(bad_head), _distinct()) == UNSUPPORTED, name       # ... and before the head
        assert call(fn, C.byref(dilated()), [None] * 17, None, 0) == UNSUPPORTED, name     # the shape before the pointers
        a = _distinct()
        a[W1] = None                                            # a pointer before UNSUPPORTED and before the workspace
        assert call(fn, C.byref(past), a, None, 0) == INVALID, name
    fused = hiplib.mms_score_tail_forward_fused_f32
    assert call(fused, C.byref(past), _distinct(), None, 0) == UNSUPPORTED         # before the workspace
    for t in R.SEQUENCE_TAILS:
        for pool in R.POOLS:
            assert call(fused, C.byref(_shape(tail, t, pool)), _distinct()) == UNSUPPORTED, t


@pytest.mark.parametrize("name", CALLS)
def test_pointer_and_workspace_rules(tail, hiplib, name):
    fn = getattr(hiplib, name)
    fused_only = name.endswith("fused_f32")
    query = {"mms_score_tail_forward_f32": "mms_score_tail_workspace_bytes",
             "mms_score_tail_forward_f64": "mms_score_tail_workspace_bytes_f64",
             "mms_score_tail_forward_sequence_f32": "mms_score_tail_sequence_workspace_bytes"}.get(name)
    for t, pool in ((R.v4(50), R.AVE), (R.v4(1517), R.MAX), (R.v5(7), R.MAX), (R.MINIMAL[1], R.AVE)):
        shape = _shape(tail, t, pool)
        sp = C.byref(shape)
        need = 8 * t.stage.conv.N if fused_only else getattr(hiplib, query)(sp)
        assert need > 0
        required = [X, WEIGHT, MEAN, VAR, SCALE, SHIFT, W1, W2, PROB] + ([OVERLAP] if t.F1 else [])
        for k in required:                            # bias, b1, b2, flt and h may be NULL; label and loss together
            a = _distinct()
            a[k] = None
            assert call(fn, sp, a) == INVALID, k
        a = _distinct()
        a[LABEL] = None                               # a loss without a label
        assert call(fn, sp, a) == INVALID
        for out in OUTPUTS:                           # an output that is an input or another output
            for other in range(17):
                if other != out:
                    a = _distinct()
                    a[out] = a[other]
                    assert call(fn, sp, a) == INVALID, (out, other)
        a = _distinct()
        assert call(fn, sp, a, None, need) == WORKSPACE
        assert call(fn, sp, a, P, need - 1) == WORKSPACE
        assert call(fn, sp, a, P, 0) == WORKSPACE
        a[W2] = None
        assert call(fn, sp, a, None, 0) == INVALID    # arguments are judged before the workspace
    for t in (R.v4(0), R.MINIMAL[0]._replace(stage=R.A.ST(0, 2, 3, 3, 3, 2, 2, (2, 2)))):
        sp = C.byref(_shape(tail, t))
        assert call(fn, sp, [None] * 17, None, 0) == OK
        assert call(fn, sp, _distinct(), None, 0) == OK


def test_overlap_may_be_null_only_without_columns(tail, hiplib):
    """With F1 == 0 a NULL overlap is no refusal: the call gets as far as the workspace check."""
    a = _distinct()
    a[OVERLAP] = None
    for name in CALLS:
        assert call(getattr(hiplib, name), C.byref(_shape(tail, R.MINIMAL[0])), a, None, 0) == WORKSPACE, name


def test_route_table(tail):
    """NONE, SEQUENCE and FUSED are each reached; the forced calls' reach is tests/test_gpu_score_tail.py's."""
    for shape, _ in _refused(tail):
        assert tail.score_tail_route(shape) == tail.ROUTE_NONE and tail.score_tail_route_f64(shape) == tail.ROUTE_NONE
    for pool in R.POOLS:
        for t in R.SEQUENCE_TAILS:
            assert tail.score_tail_route(_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE, (t, pool)
        for t in R.MAIN_FUSED:
            assert tail.score_tail_route(_shape(tail, t, pool)) == tail.ROUTE_FUSED, (t, pool)
            assert tail.score_tail_route_f64(_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE
        for t in R.FORCED_ONLY:                       # reached, but on fewer workgroups than measured
            assert tail.score_tail_route(_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE, (t, pool)
        # the measured span (tools/bench_score_tail.py): 17 to 506 workgroups of three images, N = 49 .. 1518
        for N, want in ((48, tail.ROUTE_SEQUENCE), (49, tail.ROUTE_FUSED), (50, tail.ROUTE_FUSED), (100, tail.ROUTE_FUSED),
                        (400, tail.ROUTE_FUSED), (1517, tail.ROUTE_FUSED), (1518, tail.ROUTE_FUSED),
                        (1519, tail.ROUTE_SEQUENCE)):
            assert tail.score_tail_route(_shape(tail, R.v4(N), pool)) == want, (N, pool)
            assert tail.score_tail_route(_shape(tail, R.v5(N), pool)) == want, (N, pool)


def test_workspace_queries(tail, hiplib):
    """SEQUENCE: the stage call's own figure, flt, h and the head call's own figure, each rounded up to 16 bytes.
    FUSED: a float and an int per sample."""
    from mms_answer_selection_amd import conv_maxpool_stage, conv_stage, head
    r16 = lambda v: (v + 15) // 16 * 16
    for pool in R.POOLS:
        stage32, stage64 = ((conv_maxpool_stage.conv_maxpool_stage_workspace_bytes,
                             conv_maxpool_stage.conv_maxpool_stage_workspace_bytes_f64) if pool == R.MAX else
                            (conv_stage.conv_stage_workspace_bytes, conv_stage.conv_stage_workspace_bytes_f64))
        for t in R.GPU_TAILS + [R.v4(1517), R.v5(1517)]:
            shape, hs, N = _shape(tail, t, pool), R.head_shape(t), t.stage.conv.N
            hshape = head.head_shape(*hs, phase=head.TEST)
            want32 = (r16(stage32(shape.conv, t.stage.pool)) + r16(N * hs.F0 * 4) + r16(N * hs.H * 4) +
                      r16(head.head_workspace_bytes(hshape)))
            want64 = (r16(stage64(shape.conv, t.stage.pool)) + r16(N * hs.F0 * 8) + r16(N * hs.H * 8) +
                      r16(head.head_workspace_bytes_f64(hshape)))
            assert tail.score_tail_workspace_bytes(shape, "sequence") == want32, (t, pool)
            assert tail.score_tail_workspace_bytes_f64(shape) == want64, (t, pool)
            assert tail.score_tail_workspace_bytes_f64(shape, "sequence") == want64, (t, pool)
            fused = tail.score_tail_route(shape) == tail.ROUTE_FUSED
            assert tail.score_tail_workspace_bytes(shape) == (8 * N if fused else want32), (t, pool)
        for q in QUERIES:
            assert getattr(hiplib, q)(C.byref(_shape(tail, R.v4(0), pool))) == 0


def test_binding_refuses_before_the_library(tail):
    import torch
    from mms_answer_selection_amd import capi
    x, w, k = torch.zeros(3, 2, 3, 3), torch.zeros(3, 2, 2, 2), torch.zeros(3)
    ov, w1, w2 = torch.zeros(3, 2), torch.zeros(4, 5), torch.zeros(2, 4)
    f = lambda **kw: tail.score_tail_forward(**dict(dict(
        x=x, weight=w, bias=None, pool_window=2, pool=tail.POOL_AVE, mean=k, var=k, scale=k, shift=k, overlap=ov, w1=w1,
        b1=None, w2=w2, b2=None), **kw))
    for bad in (dict(pool_window=3), dict(w1=torch.zeros(4, 6)), dict(w2=torch.zeros(2, 5)), dict(overlap=torch.zeros(2, 2)),
                dict(b1=torch.zeros(5)), dict(mean=torch.zeros(4)), dict(prob=torch.zeros(3, 3)), dict(h=torch.zeros(3, 5)),
                dict(flt=torch.zeros(3, 4)), dict(loss=torch.zeros(2), label=torch.zeros(3)), dict(route="fast")):
        with pytest.raises(capi.MMSArgumentError):
            f(**bad)
    with pytest.raises(capi.MMSArgumentError):
        tail.score_tail_forward_f64(x.double(), w.double(), None, 2, tail.POOL_AVE, k, k, k, k, ov, w1, None, w2, None,
                                    route="fused")
    with pytest.raises(capi.MMSError):
        f()                                           # host tensors: there is no CPU path
