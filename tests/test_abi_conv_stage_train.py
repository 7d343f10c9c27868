"""CPU suite: the TRAIN stage calls are declared in include/mms_conv_stage_train.h (valid C), exported by the built
library and bound by mms_answer_selection_amd/conv_stage_train.py; the headers and bindings that were there before and
the ABI version are as they were; every host-side rule of the header holds without a GPU -- nothing is enqueued on any
of these paths, the arrays are NULL or addresses that are never touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import conv_stage_train_reference as R
from conftest import ROOT
from pooled_stage_suite import INVALID, OK, UNSUPPORTED, WORKSPACE, P, _cshape, _refused, _shape

PREFIX = "mms_conv_stage_train_"
FORWARDS = [PREFIX + "forward_f32", PREFIX + "forward_f64", PREFIX + "forward_sequence_f32", PREFIX + "forward_fused_f32"]
BACKWARDS = [PREFIX + "backward_f32", PREFIX + "backward_f64"]
QUERIES = [PREFIX + "workspace_bytes", PREFIX + "workspace_bytes_f64", PREFIX + "sequence_workspace_bytes",
           PREFIX + "fused_workspace_bytes"]
ROUTE = PREFIX + "route"
POOLS = (0, 1)
BIG = 1 << 40
# the forward's arrays in the header's order, then the backward's
X, WEIGHT, BIAS, SCALE, SHIFT, RMEAN, RVAR, Y, TOP, SAVE_POOL, SAVE_MEAN, SAVE_STD = range(12)
F_INPUTS, F_OUTPUTS = (X, WEIGHT, BIAS, SCALE, SHIFT), (RMEAN, RVAR, Y, TOP, SAVE_POOL, SAVE_MEAN, SAVE_STD)
B_SHIFT, B_INPUTS, B_OUTPUTS = 7, tuple(range(10)), tuple(range(10, 15))


def distinct(n):
    return [P + 64 * i for i in range(n)]


@pytest.fixture(scope="module")
def stage(hiplib):
    from mms_answer_selection_amd import conv_stage_train
    conv_stage_train.lib()
    return conv_stage_train


@pytest.fixture(scope="module")
def conv(hiplib):
    from mms_answer_selection_amd import conv
    conv.lib()
    return conv


def fwd(hiplib, name, sp, ph, pw, pool, arrays, ws=P, wsb=BIG):
    return getattr(hiplib, name)(sp, ph, pw, pool, 0.5, *arrays, ws, wsb, None)


def bwd(hiplib, name, sp, ph, pw, pool, arrays, ws=P, wsb=BIG):
    return getattr(hiplib, name)(sp, ph, pw, pool, *arrays, ws, wsb, None)


def _declarations():
    txt = open(os.path.join(ROOT, "include", "mms_conv_stage_train.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(2): (m.group(1), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b(int|size_t)\s+(mms_\w+)\s*\(([^)]*)\)\s*;", txt)}


def test_every_declared_name_is_exported_and_bound(stage, hiplib):
    decl = _declarations()
    names = sorted(decl)
    assert sorted(FORWARDS + BACKWARDS + QUERIES + [ROUTE]) == names == sorted(stage.EXPORTED_SYMBOLS)
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    ctype = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        f = getattr(stage.lib(), n)
        ret, params = decl[n]
        want = []
        for p in params:                                       # the argument types as the header declares them
            t = p.rsplit(" ", 1)[0].replace("const ", "").strip()
            want.append(C.POINTER(stage.conv.ConvShape) if t == "mms_conv_shape*" else
                        C.c_void_p if t.endswith("*") else ctype[t])
        assert f.restype is ctype[ret] and list(f.argtypes) == want, n
    real = {n: [p.split()[0] for p in decl[n][1] if "bn_memory" in p] for n in FORWARDS}
    assert real == {FORWARDS[0]: ["float"], FORWARDS[1]: ["double"], FORWARDS[2]: ["float"], FORWARDS[3]: ["float"]}
    for n in FORWARDS + BACKWARDS:                             # float calls take float arrays, double calls double ones
        t = "double" if n.endswith("f64") else "float"
        arrays = [p for p in decl[n][1] if "*" in p and "void" not in p and "mms_conv_shape" not in p]
        assert len(arrays) == (12 if n in FORWARDS else 15) and all(t in p for p in arrays), n
    for f in ("conv_stage_train_route", "conv_stage_train_workspace_bytes", "conv_stage_train_forward",
              "conv_stage_train_backward"):
        assert callable(getattr(stage, f)) and callable(getattr(stage, f + "_f64")), f
    assert (stage.ROUTE_NONE, stage.ROUTE_SEQUENCE, stage.ROUTE_FUSED, stage.POOL_AVE, stage.POOL_MAX) == (-1, 0, 1, 0, 1)


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "conv_stage_train_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(stage, hiplib):
    from mms_answer_selection_amd import bn_maxpool, capi, conv, conv_maxpool_stage, conv_stage
    for f in [os.path.join("include", h) for h in ("mms.h", "mms_conv.h", "mms_bn_maxpool.h")] + \
            [os.path.join("mms_answer_selection_amd", m)
             for m in ("capi.py", "conv.py", "conv_stage.py", "conv_maxpool_stage.py", "bn_maxpool.py", "_pooled.py")]:
        assert "stage_train" not in open(os.path.join(ROOT, f)).read(), f
    for m in (capi, conv, conv_stage, conv_maxpool_stage, bn_maxpool):
        assert not [n for n in dir(m) if "stage_train" in n], m
        assert not [n for n in m.EXPORTED_SYMBOLS if "stage_train" in n], m
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_shape_window_and_pool_refusals_in_every_call(stage, conv, hiplib):
    """The TEST-phase stages' table -- what mms_conv_forward refuses with its code, then the windows -- in every call
    and with either pool, then an unknown pool; NULL arrays and never-touched addresses alike."""
    table = [(s, w, pool, code) for s, w, code in _refused(conv) for pool in POOLS]
    good = _shape(conv)
    table += [(s, (2, 5), pool, INVALID) for s in (good, _shape(conv, N=0)) for pool in (-1, 2, 7)]
    for shape, (ph, pw), pool, code in table:
        sp = C.byref(shape)
        what = tuple(getattr(shape, f) for f, _ in shape._fields_) + (ph, pw, pool)
        assert getattr(hiplib, ROUTE)(sp, ph, pw, pool) == stage.ROUTE_NONE, what
        for q in QUERIES:
            assert getattr(hiplib, q)(sp, ph, pw, pool) == 0, (q, what)
        for name in FORWARDS:
            assert fwd(hiplib, name, sp, ph, pw, pool, [None] * 12, None, 0) == code, (name, what)
            assert fwd(hiplib, name, sp, ph, pw, pool, distinct(12)) == code, (name, what)
        for name in BACKWARDS:
            assert bwd(hiplib, name, sp, ph, pw, pool, [None] * 15, None, 0) == code, (name, what)
            assert bwd(hiplib, name, sp, ph, pw, pool, distinct(15)) == code, (name, what)
    # the convolution's refusal comes first: a dilated shape with an unknown pool and a window that does not tile
    dil = C.byref(_shape(conv, dilation=2))
    assert fwd(hiplib, FORWARDS[0], dil, 3, 3, 9, distinct(12)) == UNSUPPORTED
    assert bwd(hiplib, BACKWARDS[0], dil, 3, 3, 9, distinct(15)) == UNSUPPORTED
    for name in FORWARDS:
        assert fwd(hiplib, name, None, 2, 2, 0, distinct(12)) == INVALID
    for name in BACKWARDS:
        assert bwd(hiplib, name, None, 2, 2, 0, distinct(15)) == INVALID
    assert getattr(hiplib, ROUTE)(None, 2, 2, 0) == stage.ROUTE_NONE
    for q in QUERIES:
        assert getattr(hiplib, q)(None, 2, 2, 0) == 0


def _reached_and_not(conv):
    """A shape the fused launches reach and one they do not (stride 2), with their windows."""
    return (_shape(conv, N=200), (2, 5)), (_shape(conv, stride=2, pad=1), (2, 3))


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("name", FORWARDS)
def test_forward_pointer_and_workspace_rules(stage, conv, hiplib, name, pool):
    fused = name == FORWARDS[3]
    for shape, (ph, pw) in _reached_and_not(conv):
        sp = C.byref(shape)
        for k in range(12):
            if k != BIAS:                                      # the bias may be NULL
                a = distinct(12)
                a[k] = None
                assert fwd(hiplib, name, sp, ph, pw, pool, a) == INVALID, k
        for out in F_OUTPUTS:
            for k in range(12):                                # an output equal to an input or to another output
                if k != out:
                    a = distinct(12)
                    a[out] = a[k]
                    assert fwd(hiplib, name, sp, ph, pw, pool, a) == INVALID, (out, k)
        # N == 0: nothing is judged but the shape, the window and the pool
        empty = C.byref(_shape(conv, N=0, stride=shape.stride_h, pad=shape.pad_h))
        assert fwd(hiplib, name, empty, ph, pw, pool, [None] * 12, None, 0) == OK
        assert fwd(hiplib, name, empty, ph, pw, pool, distinct(12), None, 0) == OK


def test_forward_workspace_is_judged_last(stage, conv, hiplib):
    """A large batch, whose BN sweep needs chunk sums: every forward wants a workspace, and says so after the arrays."""
    shape, pool = conv.conv_shape(1517, 4, 40, 40, 32, 5), (4, 4)
    sp = C.byref(shape)
    for m in POOLS:
        for name, q in zip(FORWARDS, QUERIES):
            total = getattr(hiplib, q)(sp, *pool, m)
            assert total > 0
            assert fwd(hiplib, name, sp, *pool, m, distinct(12), None, BIG) == WORKSPACE, name
            assert fwd(hiplib, name, sp, *pool, m, distinct(12), P, 0) == WORKSPACE, name
            a = distinct(12)
            a[WEIGHT] = None
            assert fwd(hiplib, name, sp, *pool, m, a, None, 0) == INVALID, name
        # what the forward alone needs is at most the query, which also covers the backward
        bn = hiplib.mms_bn_pool_tanh_workspace_bytes(1517, 32, 36, 36, 4, 4)
        assert 0 < bn <= getattr(hiplib, QUERIES[2])(sp, *pool, m)
        assert fwd(hiplib, FORWARDS[2], sp, *pool, m, distinct(12), P, bn - 1) == WORKSPACE


def test_fused_call_is_unsupported_exactly_where_the_test_phase_fused_call_is(stage, conv, hiplib):
    """The reach both headers state: the forward is FAST and `ph` whole rows of y (or whole images of at most 128
    pixels) fit a workgroup's 256 pixels.  Where that fails the TEST-phase fused calls say MMS_ERR_UNSUPPORTED for
    never-touched arrays, and so does this one; where it holds this one goes on to ask for its workspace (the
    TEST-phase calls would launch there, so they are not called)."""
    from mms_answer_selection_amd import conv_maxpool_stage, conv_stage
    conv_stage.lib(), conv_maxpool_stage.lib()
    cases = [(_cshape(conv, st), st.pool) for st in R.GPU_STAGES]
    cases += [(_shape(conv, N=200), (2, 5)), (_shape(conv, stride=2, pad=1), (2, 3)), (_shape(conv, group=2), (2, 5)),
              (conv.conv_shape(2, 65, 9, 9, 8, 3), (7, 1)), (conv.conv_shape(2, 8, 9, 9, 65, 3), (7, 1)),
              (conv.conv_shape(1, 2, 8, 102, 3, 3), (3, 4)), (conv.conv_shape(1, 2, 8, 102, 3, 3), (2, 4)),
              (conv.conv_shape(2, 32, 8, 8, 32, 3), (6, 6)), (conv.conv_shape(50, 32, 9, 9, 64, 5), (5, 5)),
              (conv.conv_shape(50, 4, 40, 40, 32, 5), (4, 4)), (conv.conv_shape(3, 64, 30, 30, 64, 7), (4, 4)),
              (conv.conv_shape(2, 64, 40, 40, 64, 9), (8, 8)), (conv.conv_shape(2, 16, 60, 60, 48, 5), (4, 2)),
              (conv.conv_shape(2, 32, 24, 24, 32, 5), (4, 4)), (conv.conv_shape(2, 64, 24, 24, 64, 5), (20, 4))]
    test_phase = {0: hiplib.mms_conv_stage_forward_fused_f32, 1: hiplib.mms_conv_maxpool_stage_forward_fused_f32}
    seen = set()
    for shape, (ph, pw) in cases:
        sp = C.byref(shape)
        OH, OW = conv.conv_output_dims(shape)
        reached = conv.conv_route(shape, conv.PASS_FORWARD) == conv.ROUTE_FAST and (OH * OW <= 128 or ph * OW <= 256)
        for pool in POOLS:
            got = fwd(hiplib, FORWARDS[3], sp, ph, pw, pool, distinct(12), None, 0)
            assert got == (WORKSPACE if reached else UNSUPPORTED), (OH, OW, ph, pw, pool)
            assert (getattr(hiplib, QUERIES[3])(sp, ph, pw, pool) > 0) == reached
            if not reached:
                assert test_phase[pool](sp, ph, pw, *distinct(9), None) == UNSUPPORTED
                assert getattr(hiplib, ROUTE)(sp, ph, pw, pool) == stage.ROUTE_SEQUENCE
                a = distinct(12)
                a[X] = None
                assert fwd(hiplib, FORWARDS[3], sp, ph, pw, pool, a) == INVALID      # arguments are judged first
            seen.add(got)
    assert seen == {UNSUPPORTED, WORKSPACE}


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("name", BACKWARDS)
def test_backward_pointer_and_workspace_rules(stage, conv, hiplib, name, pool):
    f64 = name.endswith("f64")
    for shape, (ph, pw) in _reached_and_not(conv):
        sp = C.byref(shape)
        for k in B_INPUTS:
            a = distinct(15)
            a[k] = None
            want = OK if (k == B_SHIFT and pool == 0) else INVALID       # AVE does not read shift
            if want == INVALID:
                assert bwd(hiplib, name, sp, ph, pw, pool, a) == INVALID, k
        a = distinct(15)
        for k in B_OUTPUTS:
            a[k] = None
        assert bwd(hiplib, name, sp, ph, pw, pool, a) == INVALID          # no output
        for out in B_OUTPUTS:
            for k in range(15):
                if k != out:
                    a = distinct(15)
                    a[out] = a[k]
                    assert bwd(hiplib, name, sp, ph, pw, pool, a) == INVALID, (out, k)
        need = getattr(hiplib, QUERIES[1] if f64 else QUERIES[0])(sp, ph, pw, pool)
        assert need > 0
        assert bwd(hiplib, name, sp, ph, pw, pool, distinct(15), None, need) == WORKSPACE
        assert bwd(hiplib, name, sp, ph, pw, pool, distinct(15), P, 0) == WORKSPACE
        a = distinct(15)
        a[0] = None
        assert bwd(hiplib, name, sp, ph, pw, pool, a, None, 0) == INVALID
        empty = C.byref(_shape(conv, N=0, stride=shape.stride_h, pad=shape.pad_h))
        assert bwd(hiplib, name, empty, ph, pw, pool, [None] * 15, None, 0) == OK
        assert bwd(hiplib, name, empty, ph, pw, pool, distinct(15), None, 0) == OK


def test_route_and_queries_are_pure_functions_of_the_shape(stage, conv, hiplib):
    for st in R.GPU_STAGES:
        s, shape = st.conv, _cshape(conv, st)
        sp = C.byref(shape)
        OH, OW = R.CR.output_dims(s)
        for pool in POOLS:
            route = getattr(hiplib, ROUTE)(sp, *st.pool, pool)
            assert route in (stage.ROUTE_SEQUENCE, stage.ROUTE_FUSED)
            assert route == getattr(hiplib, ROUTE)(sp, *st.pool, pool)
            if st in R.SEQUENCE_STAGES:
                assert route == stage.ROUTE_SEQUENCE
            assert stage.conv_stage_train_route_f64(shape, st.pool, pool) == stage.ROUTE_SEQUENCE
            f32, f64, seq, fused = (getattr(hiplib, q)(sp, *st.pool, pool) for q in QUERIES)
            # the backward's share: dy, the BN call's, the convolution's
            r16 = lambda b: (b + 15) // 16 * 16                                        # noqa: E731
            bn32 = hiplib.mms_bn_pool_tanh_workspace_bytes(s.N, s.K, OH, OW, *st.pool)
            bn64 = hiplib.mms_bn_pool_tanh_workspace_bytes_f64(s.N, s.K, OH, OW, *st.pool)
            back32 = r16(4 * s.N * s.K * OH * OW) + r16(bn32) + conv.conv_workspace_bytes(shape)
            back64 = r16(8 * s.N * s.K * OH * OW) + r16(bn64) + conv.conv_workspace_bytes_f64(shape)
            assert seq == max(bn32, back32) and f64 == max(bn64, back64) and f64 >= f32 >= seq
            assert fused == (0 if st in R.SEQUENCE_STAGES else max(back32, fused)) and f32 in (seq, fused)
            empty = C.byref(_cshape(conv, st, N=0))
            assert getattr(hiplib, ROUTE)(empty, *st.pool, pool) in (stage.ROUTE_SEQUENCE, stage.ROUTE_FUSED)
            for q in QUERIES:
                assert getattr(hiplib, q)(empty, *st.pool, pool) == 0


def test_the_gpu_lists_are_on_the_routes_they_claim(stage, conv, hiplib):
    no_x = [None] + distinct(12)[1:]
    for pool in POOLS:
        for st in R.FUSED_STAGES + R.LARGE_STAGES:
            assert fwd(hiplib, FORWARDS[3], C.byref(_cshape(conv, st)), *st.pool, pool, no_x) == INVALID, st
        for st in R.SEQUENCE_STAGES:
            assert fwd(hiplib, FORWARDS[3], C.byref(_cshape(conv, st)), *st.pool, pool, distinct(12)) == UNSUPPORTED


def test_the_nets_stages_take_the_measured_routes(stage, conv):
    """profiles/conv_stage_train_bench.txt: the spans of the header, both ends and one step outside each."""
    F, S = stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE
    v4a = lambda N: conv.conv_shape(N, 4, 40, 40, 32, 5)                               # noqa: E731 (9 bands per image)
    v3a = lambda N: conv.conv_shape(N, 1, 40, 40, 64, 5)                               # noqa: E731 (9 bands per image)
    v5a = lambda N: conv.conv_shape(N, 2, 40, 40, 32, 3)                               # noqa: E731 (7 bands per image)
    assert [stage.conv_stage_train_route(v4a(N), 4, "ave") for N in (49, 50, 51, 200, 1517)] == [S, F, S, S, S]
    assert [stage.conv_stage_train_route(v3a(N), 4, "max") for N in (49, 50, 400, 1179, 1180, 1517)] == [S, F, F, F, S, S]
    assert [stage.conv_stage_train_route(v5a(N), 2, "max") for N in (50, 64, 65, 1517, 1518)] == [S, S, F, F, S]
    for N in (50, 200, 1517):                                                          # whole images per workgroup
        assert stage.conv_stage_train_route(conv.conv_shape(N, 32, 9, 9, 64, 5), 5, "ave") == S
        assert stage.conv_stage_train_route(conv.conv_shape(N, 64, 9, 9, 64, 5), 5, "max") == S
        assert stage.conv_stage_train_route(conv.conv_shape(N, 32, 19, 19, 32, 4), 2, "max") == S
        assert stage.conv_stage_train_route(conv.conv_shape(N, 32, 8, 8, 32, 3), 6, "max") == S
        assert stage.conv_stage_train_route_f64(v4a(N), 4, "ave") == S


def test_the_large_gpu_shapes_take_the_routes_they_claim(stage, conv):
    """The shapes at which tests/test_gpu_conv_stage_train.py runs the main call inside and beside the spans: two bands
    per image (R: 12 and 8 rows; W: 10 and 10), so 2 N workgroups."""
    F, S = stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE
    r = lambda N: conv.conv_shape(N, 3, 22, 22, 7, 3)                                  # noqa: E731
    w = lambda N: conv.conv_shape(N, 2, 22, 22, 4, 3)                                  # noqa: E731
    assert [R.R_MINUS.conv.N, R.R.conv.N, R.R_PLUS.conv.N, R.W.conv.N] == [224, 225, 226, 657]
    assert [stage.conv_stage_train_route(r(N), 4, "ave") for N in (224, 225, 226)] == [S, F, S]
    assert [stage.conv_stage_train_route(r(N), 4, "max") for N in (224, 225, 226)] == [S, F, F]
    assert [stage.conv_stage_train_route(w(N), 2, m) for N in (224, 225, 657) for m in ("ave", "max")] == [S, S, F, F, S, F]
    for st in R.LARGE_STAGES:
        for method in R.METHODS:
            got = stage.conv_stage_train_route(_cshape(conv, st), st.pool, method)
            assert got == (F if R.LARGE_PLANS[st]["route"][method] == R.FUSED else S), (st, method)
            assert stage.conv_stage_train_route_f64(_cshape(conv, st), st.pool, method) == S


def test_binding_refuses_before_the_library(stage):
    import torch
    from mms_answer_selection_amd import capi
    f = stage.conv_stage_train_forward
    x, w, k = torch.zeros(2, 4, 12, 12), torch.zeros(6, 4, 3, 3), torch.zeros(6)
    with pytest.raises(capi.MMSArgumentError):
        f(x, w, None, (3, 2), "ave", k, k, k, k)                                      # 10 % 3
    with pytest.raises(capi.MMSArgumentError):
        f(x, w, None, (2, 5), "min", k, k, k, k)
    with pytest.raises(capi.MMSArgumentError):
        f(x, w, None, (2, 5), "max", k, k, k, torch.zeros(5))                         # running_var's shape
    with pytest.raises(capi.MMSArgumentError):
        f(x, w, None, (2, 5), "max", k, k, k, k, y=torch.zeros(2, 6, 5, 2))
    with pytest.raises(capi.MMSArgumentError):
        f(x, w, None, (2, 5), "ave", k, k, k, k, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_train_forward_f64(x.double(), w.double(), None, (2, 5), "ave", *([k.double()] * 4), route="fused")
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_train_backward(x, w, (2, 5), "ave", torch.zeros(2, 6, 10, 10), *([torch.zeros(2, 6, 5, 2)] * 3),
                                        k, k, k, k)                                   # no output
    with pytest.raises(capi.MMSError):
        f(x, w, None, (2, 5), "ave", k, k, k, k)                                      # host tensors: no CPU path
