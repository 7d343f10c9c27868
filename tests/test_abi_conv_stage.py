"""CPU suite: the stage calls are declared in include/mms_conv_stage.h (valid C), exported by the built library and
bound by mms_answer_selection_amd/conv_stage.py; include/mms.h, include/mms_conv.h, capi.py, conv.py and the ABI version
are as they were; every host-side rule of the header holds without a GPU -- nothing is enqueued on any of these paths,
the arrays are NULL or addresses that are never touched."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import conv_reference as CR
import conv_stage_reference as R
from conftest import ROOT
from pooled_stage_suite import (INVALID, MEAN, OK, SAVE_POOL, SCALE, SHIFT, TOP, UNSUPPORTED, VAR, WEIGHT, WORKSPACE,
                                P, X, _cshape, _distinct, _refused, _shape)

FORWARDS = ["mms_conv_stage_forward_f32", "mms_conv_stage_forward_f64", "mms_conv_stage_forward_sequence_f32"]
FUSED = "mms_conv_stage_forward_fused_f32"            # the same arguments without the workspace pair
QUERIES = ["mms_conv_stage_workspace_bytes", "mms_conv_stage_workspace_bytes_f64",
           "mms_conv_stage_sequence_workspace_bytes"]
V4 = [((4, 40, 40, 32), 4), ((32, 9, 9, 64), 5)]      # (C, H, W, K) of network_v4's two stages, 5 x 5, and the window


@pytest.fixture(scope="module")
def stage(hiplib):
    from mms_answer_selection_amd import conv_stage
    conv_stage.lib()
    return conv_stage


@pytest.fixture(scope="module")
def conv(hiplib):
    from mms_answer_selection_amd import conv
    conv.lib()
    return conv


def _declared():
    txt = open(os.path.join(ROOT, "include", "mms_conv_stage.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


def test_every_declared_name_is_exported_and_bound(stage, hiplib):
    names = _declared()
    assert len(names) == 8 and all(n.startswith("mms_conv_stage_") for n in names), names
    assert sorted(stage.EXPORTED_SYMBOLS) == names
    assert sorted(FORWARDS + QUERIES + [FUSED, "mms_conv_stage_route"]) == names
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(stage.lib(), n).argtypes is not None, n
    for f in ("conv_stage_route", "conv_stage_workspace_bytes", "conv_stage_forward"):
        assert callable(getattr(stage, f)) and callable(getattr(stage, f + "_f64")), f


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "conv_stage_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(stage, hiplib):
    from mms_answer_selection_amd import capi, conv
    for f in (os.path.join("include", "mms.h"), os.path.join("include", "mms_conv.h"),
              os.path.join("mms_answer_selection_amd", "capi.py"), os.path.join("mms_answer_selection_amd", "conv.py")):
        assert "conv_stage" not in open(os.path.join(ROOT, f)).read(), f
    assert not [n for n in dir(capi) if "conv_stage" in n]
    assert not [n for n in capi.EXPORTED_SYMBOLS + conv.EXPORTED_SYMBOLS if "stage" in n]
    assert not [n for n in dir(conv) if "stage" in n]
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_shape_and_window_refusals_in_every_call(stage, conv, hiplib):
    for shape, (ph, pw), code in _refused(conv):
        sp = C.byref(shape)
        what = tuple(getattr(shape, f) for f, _ in shape._fields_) + (ph, pw)
        assert hiplib.mms_conv_stage_route(sp, ph, pw) == stage.ROUTE_NONE, what
        for q in QUERIES:
            assert getattr(hiplib, q)(sp, ph, pw) == 0, (q, what)
        for name in FORWARDS:
            assert getattr(hiplib, name)(sp, ph, pw, *([None] * 9), None, 0, None) == code, (name, what)
            assert getattr(hiplib, name)(sp, ph, pw, *_distinct(), P, 1 << 40, None) == code, (name, what)
        assert getattr(hiplib, FUSED)(sp, ph, pw, *([None] * 9), None) == code, what
        assert getattr(hiplib, FUSED)(sp, ph, pw, *_distinct(), None) == code, what
    for name in FORWARDS:
        assert getattr(hiplib, name)(None, 2, 2, *_distinct(), P, 1 << 40, None) == INVALID
    assert getattr(hiplib, FUSED)(None, 2, 2, *_distinct(), None) == INVALID
    assert hiplib.mms_conv_stage_route(None, 2, 2) == stage.ROUTE_NONE
    for q in QUERIES:
        assert getattr(hiplib, q)(None, 2, 2) == 0


def test_the_shape_refusals_are_the_convolutions(stage, conv, hiplib):
    """A refusal for the shape carries the code the Convolution calls give that shape (mms_conv_output_dims shows it
    without enqueuing anything); a refusal for the window is of a shape they accept."""
    oh, ow = C.c_int(), C.c_int()
    for shape, (ph, pw), code in _refused(conv):
        got = hiplib.mms_conv_output_dims(C.byref(shape), C.byref(oh), C.byref(ow))
        assert got == code or (got == OK and code == INVALID and (ph < 1 or pw < 1 or oh.value % ph or ow.value % pw))


@pytest.mark.parametrize("name", FORWARDS)
def test_pointer_and_workspace_rules(stage, conv, hiplib, name):
    fn = getattr(hiplib, name)
    fused = _shape(conv, N=200)                               # 10 x 10 map, windows 2 x 5; 100 workgroups of two
    seq = _shape(conv, stride=2, pad=1)                       # 6 x 6 map, windows 2 x 3
    assert stage.conv_stage_route(fused, (2, 5)) == stage.ROUTE_FUSED
    assert stage.conv_stage_route(seq, (2, 3)) == stage.ROUTE_SEQUENCE
    big = 1 << 40
    for shape, (ph, pw) in ((fused, (2, 5)), (seq, (2, 3))):
        sp = C.byref(shape)
        for k in (X, WEIGHT, MEAN, VAR, SCALE, SHIFT, TOP):   # the bias and save_pool may be NULL
            a = _distinct()
            a[k] = None
            assert fn(sp, ph, pw, *a, P, big, None) == INVALID, k
        for out in (TOP, SAVE_POOL):
            for k in range(TOP):                              # an output equal to an input
                a = _distinct()
                a[out] = a[k]
                assert fn(sp, ph, pw, *a, P, big, None) == INVALID, (out, k)
        a = _distinct()
        a[SAVE_POOL] = a[TOP]
        assert fn(sp, ph, pw, *a, P, big, None) == INVALID
    # the workspace: judged after the arguments, and only where the route uses one
    sp = C.byref(seq)
    need = hiplib.mms_conv_stage_workspace_bytes_f64(sp, 2, 3) if name.endswith("f64") else \
        hiplib.mms_conv_stage_workspace_bytes(sp, 2, 3)
    assert need > 0
    for a in (_distinct(), _distinct()[:SAVE_POOL] + [None]):
        assert fn(sp, 2, 3, *a, None, need, None) == WORKSPACE
        assert fn(sp, 2, 3, *a, P, need - 1, None) == WORKSPACE
        assert fn(sp, 2, 3, *a, P, 0, None) == WORKSPACE
    a = _distinct()
    a[WEIGHT] = None
    assert fn(sp, 2, 3, *a, None, 0, None) == INVALID
    if name != "mms_conv_stage_forward_f32":                  # the sequence route at a shape the float call fuses
        sp = C.byref(fused)
        assert fn(sp, 2, 5, *_distinct(), None, 0, None) == WORKSPACE
        q = hiplib.mms_conv_stage_workspace_bytes_f64 if name.endswith("f64") else \
            hiplib.mms_conv_stage_sequence_workspace_bytes
        assert fn(sp, 2, 5, *_distinct(), P, q(sp, 2, 5) - 1, None) == WORKSPACE
    for empty, (ph, pw) in ((_shape(conv, N=0), (2, 5)), (_shape(conv, N=0, stride=2, pad=1), (2, 3))):
        assert fn(C.byref(empty), ph, pw, *([None] * 9), None, 0, None) == OK
        assert fn(C.byref(empty), ph, pw, *_distinct(), None, 0, None) == OK


def test_fused_call_rules(stage, conv, hiplib):
    """mms_conv_stage_forward_fused_f32: the pointer rules of the other calls, then MMS_ERR_UNSUPPORTED wherever the
    launch does not reach, whatever the arrays."""
    fn = getattr(hiplib, FUSED)
    reached = _shape(conv, N=200)                             # 10 x 10 map, windows 2 x 5
    sp = C.byref(reached)
    for k in (X, WEIGHT, MEAN, VAR, SCALE, SHIFT, TOP):
        a = _distinct()
        a[k] = None
        assert fn(sp, 2, 5, *a, None) == INVALID, k
    for out in (TOP, SAVE_POOL):
        for k in range(TOP):
            a = _distinct()
            a[out] = a[k]
            assert fn(sp, 2, 5, *a, None) == INVALID, (out, k)
    for shape, pool in ((_shape(conv, stride=2, pad=1), (2, 3)), (_shape(conv, group=2), (2, 5)),
                        (conv.conv_shape(2, 65, 9, 9, 8, 3), (7, 1)), (conv.conv_shape(1, 2, 8, 102, 3, 3), (3, 4))):
        assert stage.conv_stage_route(shape, pool) == stage.ROUTE_SEQUENCE
        assert fn(C.byref(shape), *pool, *_distinct(), None) == UNSUPPORTED
        a = _distinct()
        a[X] = None
        assert fn(C.byref(shape), *pool, *a, None) == INVALID                 # arguments are judged first
    assert fn(C.byref(_shape(conv, N=0)), 2, 5, *([None] * 9), None) == OK
    assert fn(C.byref(_shape(conv, N=0, stride=2, pad=1)), 2, 3, *_distinct(), None) == OK


def test_every_route_of_the_binding_binds_first():
    """In a fresh process, the first call of each route -- refused here for its host tensors -- leaves the signatures
    on the handle: no route reaches the library with an unbound function (pointers would go in as 32-bit ints)."""
    code = ("import torch\n"
            "from mms_answer_selection_amd import capi, conv_stage\n"
            "k = torch.zeros(6)\n"
            "try:\n"
            "    conv_stage.conv_stage_forward(torch.zeros(2, 4, 12, 12), torch.zeros(6, 4, 3, 3), None, (2, 5), k, k, k, k,"
            " route=%r)\n"
            "    raise SystemExit(3)\n"
            "except capi.MMSError:\n"
            "    pass\n"
            "assert all(getattr(capi.lib(), n).argtypes is not None for n in conv_stage.EXPORTED_SYMBOLS)\n")
    for route in ("fused", "sequence", "auto"):
        subprocess.check_call([sys.executable, "-c", code % route], cwd=ROOT)


def test_route_table(stage, conv):
    for N in (1, 3, 50, 90, 91, 200, 227, 228, 1517):
        for (C_, H, W, K), p in V4:
            shape = conv.conv_shape(N, C_, H, W, K, 5)
            if C_ == 4:     # a 4-row band where the convolution's is 6, nine per image: fused up to 2048 workgroups
                want = stage.ROUTE_FUSED if 9 * N <= 2048 else stage.ROUTE_SEQUENCE
            else:           # ten whole images per workgroup: fused from 10 workgroups
                want = stage.ROUTE_FUSED if -(-N // 10) >= 10 else stage.ROUTE_SEQUENCE
            assert stage.conv_stage_route(shape, p) == want, (N, C_)
            assert stage.conv_stage_route_f64(shape, p) == stage.ROUTE_SEQUENCE
            for other in (dict(stride=2), dict(pad=2), dict(group=2), dict(stride=(1, 2)), dict(pad=(0, 1))):
                s2 = conv.conv_shape(N, C_, H, W, K, 5, **other)
                oh, ow = conv.conv_output_dims(s2)
                assert stage.conv_stage_route(s2, (oh, 1)) == stage.ROUTE_SEQUENCE, other
    # both network_v4 stages are FUSED at the batches the rules leave them: conv0 at the training batch, conv1 at the
    # test split
    assert stage.conv_stage_route(conv.conv_shape(50, 4, 40, 40, 32, 5), 4) == stage.ROUTE_FUSED
    assert stage.conv_stage_route(conv.conv_shape(1517, 32, 9, 9, 64, 5), 5) == stage.ROUTE_FUSED
    assert stage.conv_stage_route(conv.conv_shape(2, 65, 9, 9, 8, 3), (7, 1)) == stage.ROUTE_SEQUENCE
    assert stage.conv_stage_route(conv.conv_shape(2, 8, 9, 9, 65, 3), (7, 1)) == stage.ROUTE_SEQUENCE
    assert stage.conv_stage_route(conv.conv_shape(1517, 4, 40, 40, 32, 5), 6) == stage.ROUTE_FUSED        # not shrunk
    assert stage.conv_stage_route(conv.conv_shape(5000, 32, 9, 9, 64, 5), 5) == stage.ROUTE_FUSED         # whole images
    # a row too long for one whole window per workgroup: two rows of 100 fit 256 pixels, three do not
    long_rows = conv.conv_shape(1, 2, 8, 102, 3, 3)
    assert conv.conv_route(long_rows, conv.PASS_FORWARD) == conv.ROUTE_FAST
    assert stage.conv_stage_route(long_rows, (2, 4)) == stage.ROUTE_FUSED          # the convolution's own 2-row band
    assert stage.conv_stage_route(long_rows, (1, 4)) == stage.ROUTE_FUSED
    assert stage.conv_stage_route(long_rows, (3, 4)) == stage.ROUTE_SEQUENCE
    assert stage.conv_stage_route(long_rows, (6, 100)) == stage.ROUTE_SEQUENCE
    # refused: a window that does not tile, a shape the convolution refuses
    assert stage.conv_stage_route(long_rows, (4, 4)) == stage.ROUTE_NONE
    assert stage.conv_stage_route(conv.conv_shape(2, 4, 12, 12, 6, 3, dilation=2), 2) == stage.ROUTE_NONE
    assert stage.conv_stage_route_f64(long_rows, (4, 4)) == stage.ROUTE_NONE


def test_the_gpu_lists_are_on_the_routes_they_claim(stage, conv, hiplib):
    """FUSED_STAGES: the fused launch reaches them (the forced call refuses nothing but the NULL array given here);
    SEQUENCE_STAGES: it does not.  The main call fuses network_v4's first miniature and the ten-workgroup second."""
    no_x = [None] + _distinct()[1:]
    for st in R.FUSED_STAGES:
        assert getattr(hiplib, FUSED)(C.byref(_cshape(conv, st)), *st.pool, *no_x, None) == INVALID, st
        assert stage.conv_stage_route(_cshape(conv, st), st.pool) in (stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE)
    for st in R.SEQUENCE_STAGES:
        assert getattr(hiplib, FUSED)(C.byref(_cshape(conv, st)), *st.pool, *_distinct(), None) == UNSUPPORTED, st
        assert stage.conv_stage_route(_cshape(conv, st), st.pool) == stage.ROUTE_SEQUENCE, st
    assert [stage.conv_stage_route(_cshape(conv, st), st.pool) for st in R.V4_STAGES] == \
        [stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE, stage.ROUTE_FUSED]
    assert conv.conv_route(_cshape(conv, R.SEQUENCE_STAGES[-1]), conv.PASS_FORWARD) == conv.ROUTE_FAST


def test_workspace_query(stage, conv):
    for st in R.GPU_STAGES + [R.ST(1517, 4, 40, 40, 32, 5, 5, (4, 4)), R.ST(1517, 32, 9, 9, 64, 5, 5, (5, 5))]:
        s, shape = st.conv, _cshape(conv, st)
        OH, OW = CR.output_dims(s)
        pooled = s.N * s.K * (OH // st.pool[0]) * (OW // st.pool[1])
        elems = s.N * s.K * OH * OW + 2 * s.K + pooled        # the map, save_mean / save_std, a save_pool
        fused = stage.conv_stage_route(shape, st.pool) == stage.ROUTE_FUSED
        assert stage.conv_stage_workspace_bytes(shape, st.pool) == (0 if fused else 4 * elems)
        assert stage.conv_stage_workspace_bytes(shape, st.pool, route="sequence") == 4 * elems
        assert stage.conv_stage_workspace_bytes_f64(shape, st.pool) == 8 * elems
        assert stage.conv_stage_workspace_bytes_f64(shape, st.pool, route="sequence") == 8 * elems
        assert 4 * elems >= 4 * s.N * s.K * OH * OW
        empty = _cshape(conv, st, N=0)
        for q in (stage.conv_stage_workspace_bytes, stage.conv_stage_workspace_bytes_f64):
            assert q(empty, st.pool) == 0 and q(empty, st.pool, route="sequence") == 0


def test_binding_refuses_before_the_library(stage):
    import torch
    from mms_answer_selection_amd import capi
    x, w, k = torch.zeros(2, 4, 12, 12), torch.zeros(6, 4, 3, 3), torch.zeros(6)
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (3, 2), k, k, k, k)                      # 10 % 3
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (0, 2), k, k, k, k)
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (2, 5), k, k, k, torch.zeros(5))         # shift's shape
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (2, 5), k, k, k, k, top=torch.zeros(2, 6, 10, 10))
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (2, 5), k, k, k, k, save_pool=torch.zeros(2, 6, 5, 3))
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, w, None, (2, 5), k, k, k, k, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward_f64(x.double(), w.double(), None, (2, 5), *([k.double()] * 4), route="fused")
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_stage_forward(x, torch.zeros(6, 3, 3, 3), None, (2, 5), k, k, k, k)
    with pytest.raises(capi.MMSError):
        stage.conv_stage_forward(x, w, None, (2, 5), k, k, k, k)                      # host tensors: no CPU path
