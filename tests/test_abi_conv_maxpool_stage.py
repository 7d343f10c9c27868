"""CPU suite: the MAX stage calls are declared in include/mms_conv_maxpool_stage.h (valid C), exported by the built
library and bound by mms_answer_selection_amd/conv_maxpool_stage.py; the headers and bindings that were there before and
the ABI version are as they were; every host-side rule of the header holds without a GPU -- nothing is enqueued on any
of these paths, the arrays are NULL or addresses that are never touched.  The refusal table is the AVE stage's
(tests/test_abi_conv_stage.py: _refused), by import."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import conv_reference as CR
import conv_maxpool_stage_reference as R
from conftest import ROOT
from pooled_stage_suite import (INVALID, OK, SAVE_POOL, SCALE, SHIFT, TOP, UNSUPPORTED, VAR, WEIGHT, WORKSPACE, MEAN, P, X,
                                 _cshape, _distinct, _refused, _shape)

PREFIX = "mms_conv_maxpool_stage_"
FORWARDS = [PREFIX + "forward_f32", PREFIX + "forward_f64", PREFIX + "forward_sequence_f32"]
FUSED = PREFIX + "forward_fused_f32"                  # the same arguments without the workspace pair
QUERIES = [PREFIX + "workspace_bytes", PREFIX + "workspace_bytes_f64", PREFIX + "sequence_workspace_bytes"]
ROUTE = PREFIX + "route"
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_conv_maxpool_stage as BENCH              # noqa: E402 (its restatement of the fused plan, the one copy)

# network_v3's and network_v5's five stages: (C, H, W, K, kernel, window), then the fused plan's images per workgroup
# and bands per image, by the bench tool's restatement: test_route_table holds it to the library's own plan
NETS = [(st, *BENCH.fused_plan(*st)) for st in BENCH.STAGES.values()]
# the header's rule, in workgroups: [least, most] fused, for workgroups of several whole images, of a band of rows of
# one image, and of one whole image
IMAGE_GROUPS, ROW_BAND_GROUPS, ONE_IMAGE_GROUPS = (60, 300), (54, 14000), (50, 2000)


def span(G, bands):
    return IMAGE_GROUPS if G > 1 else ROW_BAND_GROUPS if bands > 1 else ONE_IMAGE_GROUPS


def want_route(stage, N, G, bands):
    groups = -(-N // G) * bands
    lo, hi = span(G, bands)
    return stage.ROUTE_FUSED if lo <= groups <= hi else stage.ROUTE_SEQUENCE


@pytest.fixture(scope="module")
def stage(hiplib):
    from mms_answer_selection_amd import conv_maxpool_stage
    conv_maxpool_stage.lib()
    return conv_maxpool_stage


@pytest.fixture(scope="module")
def conv(hiplib):
    from mms_answer_selection_amd import conv
    conv.lib()
    return conv


def _declared():
    txt = open(os.path.join(ROOT, "include", "mms_conv_maxpool_stage.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mms_\w+)\s*\(", txt)))


def test_every_declared_name_is_exported_and_bound(stage, hiplib):
    names = _declared()
    assert len(names) == 8 and all(n.startswith(PREFIX) for n in names), names
    assert sorted(stage.EXPORTED_SYMBOLS) == names
    assert sorted(FORWARDS + QUERIES + [FUSED, ROUTE]) == names
    ave = open(os.path.join(ROOT, "include", "mms_conv_stage.h")).read()
    for n in names:                                           # name for name the AVE header's
        assert re.search(r"\b%s\s*\(" % n.replace("maxpool_", ""), ave), n
    so = open(os.path.join(ROOT, "mms_answer_selection_amd", "libmms_hip.so"), "rb").read()
    for n in names:
        assert hasattr(hiplib, n) and n.encode() in so, n
        assert getattr(stage.lib(), n).argtypes is not None, n
    for f in ("conv_maxpool_stage_route", "conv_maxpool_stage_workspace_bytes", "conv_maxpool_stage_forward"):
        assert callable(getattr(stage, f)) and callable(getattr(stage, f + "_f64")), f
    from mms_answer_selection_amd import conv_stage
    assert (stage.ROUTE_NONE, stage.ROUTE_SEQUENCE, stage.ROUTE_FUSED) == \
        (conv_stage.ROUTE_NONE, conv_stage.ROUTE_SEQUENCE, conv_stage.ROUTE_FUSED) == (-1, 0, 1)


def test_header_is_c():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "conv_maxpool_stage_abi_is_c.c")])


def test_the_frozen_surface_is_untouched(stage, hiplib):
    from mms_answer_selection_amd import bn_maxpool, capi, conv, conv_stage
    for f in [os.path.join("include", h) for h in ("mms.h", "mms_conv.h", "mms_conv_stage.h", "mms_bn_maxpool.h")] + \
            [os.path.join("mms_answer_selection_amd", m) for m in ("capi.py", "conv.py", "conv_stage.py", "bn_maxpool.py")]:
        assert "maxpool_stage" not in open(os.path.join(ROOT, f)).read(), f
    for m in (capi, conv, conv_stage, bn_maxpool):
        assert not [n for n in dir(m) if "maxpool_stage" in n], m
        assert not [n for n in m.EXPORTED_SYMBOLS if "maxpool_stage" in n], m
    assert hiplib.mms_version() == 212 and capi.MMS_VERSION == 212


def test_shape_and_window_refusals_in_every_call(stage, conv, hiplib):
    """The AVE stage's table, in every call, with the same codes: the AVE calls are asked beside the MAX ones."""
    for shape, (ph, pw), code in _refused(conv):
        sp = C.byref(shape)
        what = tuple(getattr(shape, f) for f, _ in shape._fields_) + (ph, pw)
        assert getattr(hiplib, ROUTE)(sp, ph, pw) == stage.ROUTE_NONE, what
        for q in QUERIES:
            assert getattr(hiplib, q)(sp, ph, pw) == 0, (q, what)
        for name in FORWARDS:
            ave = getattr(hiplib, name.replace("maxpool_", ""))
            for args in (([None] * 9) + [None, 0, None], _distinct() + [P, 1 << 40, None]):
                assert getattr(hiplib, name)(sp, ph, pw, *args) == code == ave(sp, ph, pw, *args), (name, what)
        assert getattr(hiplib, FUSED)(sp, ph, pw, *([None] * 9), None) == code, what
        assert getattr(hiplib, FUSED)(sp, ph, pw, *_distinct(), None) == code, what
    for name in FORWARDS:
        assert getattr(hiplib, name)(None, 2, 2, *_distinct(), P, 1 << 40, None) == INVALID
    assert getattr(hiplib, FUSED)(None, 2, 2, *_distinct(), None) == INVALID
    assert getattr(hiplib, ROUTE)(None, 2, 2) == stage.ROUTE_NONE
    for q in QUERIES:
        assert getattr(hiplib, q)(None, 2, 2) == 0


def _fused_and_sequence(stage, conv):
    """A shape and window the main call fuses (network_v5's last stage at the test split) and one it cannot."""
    fused, seq = conv.conv_shape(1517, 32, 8, 8, 32, 3), _shape(conv, stride=2, pad=1)       # 6 x 6 maps
    assert stage.conv_maxpool_stage_route(fused, 6) == stage.ROUTE_FUSED
    assert stage.conv_maxpool_stage_route(seq, (2, 3)) == stage.ROUTE_SEQUENCE
    return (fused, (6, 6)), (seq, (2, 3))


@pytest.mark.parametrize("name", FORWARDS)
def test_pointer_and_workspace_rules(stage, conv, hiplib, name):
    fn = getattr(hiplib, name)
    (fused, fpool), (seq, spool) = _fused_and_sequence(stage, conv)
    big = 1 << 40
    for shape, (ph, pw) in ((fused, fpool), (seq, spool)):
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
    f64 = name.endswith("f64")
    need = getattr(hiplib, QUERIES[1] if f64 else QUERIES[0])(sp, *spool)
    assert need > 0
    for a in (_distinct(), _distinct()[:SAVE_POOL] + [None]):
        assert fn(sp, *spool, *a, None, need, None) == WORKSPACE
        assert fn(sp, *spool, *a, P, need - 1, None) == WORKSPACE
        assert fn(sp, *spool, *a, P, 0, None) == WORKSPACE
    a = _distinct()
    a[WEIGHT] = None
    assert fn(sp, *spool, *a, None, 0, None) == INVALID
    if name != FORWARDS[0]:                                   # the sequence route at a shape the float call fuses
        sp = C.byref(fused)
        assert fn(sp, *fpool, *_distinct(), None, 0, None) == WORKSPACE
        q = getattr(hiplib, QUERIES[1] if f64 else QUERIES[2])
        assert fn(sp, *fpool, *_distinct(), P, q(sp, *fpool) - 1, None) == WORKSPACE
    for empty, (ph, pw) in ((_shape(conv, N=0), (2, 5)), (_shape(conv, N=0, stride=2, pad=1), (2, 3))):
        assert fn(C.byref(empty), ph, pw, *([None] * 9), None, 0, None) == OK
        assert fn(C.byref(empty), ph, pw, *_distinct(), None, 0, None) == OK


def test_fused_call_rules(stage, conv, hiplib):
    """mms_conv_maxpool_stage_forward_fused_f32: the pointer rules of the other calls, then MMS_ERR_UNSUPPORTED wherever
    the launch does not reach, whatever the arrays."""
    fn = getattr(hiplib, FUSED)
    for reached, pool in ((_shape(conv, N=200), (2, 5)), (conv.conv_shape(2, 32, 8, 8, 32, 3), (6, 6))):
        sp = C.byref(reached)                                 # reached whatever the main call's rule says there
        for k in (X, WEIGHT, MEAN, VAR, SCALE, SHIFT, TOP):
            a = _distinct()
            a[k] = None
            assert fn(sp, *pool, *a, None) == INVALID, k
        for out in (TOP, SAVE_POOL):
            for k in range(TOP):
                a = _distinct()
                a[out] = a[k]
                assert fn(sp, *pool, *a, None) == INVALID, (out, k)
    for shape, pool in ((_shape(conv, stride=2, pad=1), (2, 3)), (_shape(conv, group=2), (2, 5)),
                        (conv.conv_shape(2, 65, 9, 9, 8, 3), (7, 1)), (conv.conv_shape(1, 2, 8, 102, 3, 3), (3, 4))):
        assert stage.conv_maxpool_stage_route(shape, pool) == stage.ROUTE_SEQUENCE
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
            "from mms_answer_selection_amd import capi, conv_maxpool_stage as m\n"
            "k = torch.zeros(6)\n"
            "try:\n"
            "    m.conv_maxpool_stage_forward(torch.zeros(2, 4, 12, 12), torch.zeros(6, 4, 3, 3), None, (2, 5), k, k, k, k,"
            " route=%r)\n"
            "    raise SystemExit(3)\n"
            "except capi.MMSError:\n"
            "    pass\n"
            "assert all(getattr(capi.lib(), n).argtypes is not None for n in m.EXPORTED_SYMBOLS)\n")
    for route in ("fused", "sequence", "auto"):
        subprocess.check_call([sys.executable, "-c", code % route], cwd=ROOT)


def test_route_table(stage, conv):
    """The header's rule at the five stages of the nets over a range of batches, both ends of every interval included."""
    assert [(G, bands) for _, G, bands in NETS] == [(1, 9), (10, 1), (1, 7), (1, 1), (7, 1)]
    batches = {1, 6, 25, 50, 100, 200, 400, 800, 1517, 2000, 3000, 5000}
    for (C_, H, W, K, k, p), G, bands in NETS:
        ends = {n for g in span(G, bands)
                for n in (g * G // bands - G, g * G // bands, g * G // bands + 1, g * G // bands + G) if n >= 1}
        for N in sorted(batches | ends):
            shape = conv.conv_shape(N, C_, H, W, K, k)
            assert stage.conv_maxpool_stage_route(shape, p) == want_route(stage, N, G, bands), (N, C_)
            assert stage.conv_maxpool_stage_route_f64(shape, p) == stage.ROUTE_SEQUENCE
            for other in (dict(stride=2), dict(pad=2), dict(stride=(1, 2)), dict(pad=(0, 1))):
                s2 = conv.conv_shape(N, C_, H, W, K, k, **other)
                oh, ow = conv.conv_output_dims(s2)
                assert stage.conv_maxpool_stage_route(s2, (oh, 1)) == stage.ROUTE_SEQUENCE, other
    assert stage.conv_maxpool_stage_route(conv.conv_shape(2, 65, 9, 9, 8, 3), (7, 1)) == stage.ROUTE_SEQUENCE
    assert stage.conv_maxpool_stage_route(conv.conv_shape(2, 8, 9, 9, 65, 3), (7, 1)) == stage.ROUTE_SEQUENCE
    assert stage.conv_maxpool_stage_route(conv.conv_shape(2, 32, 8, 8, 32, 3, group=2), 6) == stage.ROUTE_SEQUENCE
    # a row too long for one whole window per workgroup: two rows of 100 fit 256 pixels, three do not
    long_rows = conv.conv_shape(1, 2, 8, 102, 3, 3)
    assert conv.conv_route(long_rows, conv.PASS_FORWARD) == conv.ROUTE_FAST
    assert stage.conv_maxpool_stage_route(long_rows, (3, 4)) == stage.ROUTE_SEQUENCE
    assert stage.conv_maxpool_stage_route(long_rows, (6, 100)) == stage.ROUTE_SEQUENCE
    # refused: a window that does not tile, a shape the convolution refuses
    assert stage.conv_maxpool_stage_route(long_rows, (4, 4)) == stage.ROUTE_NONE
    assert stage.conv_maxpool_stage_route(conv.conv_shape(2, 4, 12, 12, 6, 3, dilation=2), 2) == stage.ROUTE_NONE
    assert stage.conv_maxpool_stage_route_f64(long_rows, (4, 4)) == stage.ROUTE_NONE


def test_the_nets_stages_take_the_measured_routes(stage, conv):
    """profiles/conv_maxpool_stage_bench.txt at the training batch and at the test split."""
    got = [[stage.conv_maxpool_stage_route(conv.conv_shape(N, C_, H, W, K, k), p) for N in (50, 1517)]
           for (C_, H, W, K, k, p), _, _ in NETS]
    F, S = stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE
    assert got == [[F, F], [S, F], [F, F], [F, F], [S, F]]


def test_the_gpu_lists_are_on_the_routes_they_claim(stage, conv, hiplib):
    """FUSED_STAGES: the fused launch reaches them (the forced call refuses nothing but the NULL array given here);
    SEQUENCE_STAGES: it does not."""
    no_x = [None] + _distinct()[1:]
    for st in R.FUSED_STAGES:
        assert getattr(hiplib, FUSED)(C.byref(_cshape(conv, st)), *st.pool, *no_x, None) == INVALID, st
        assert stage.conv_maxpool_stage_route(_cshape(conv, st), st.pool) in (stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE)
    for st in R.SEQUENCE_STAGES:
        assert getattr(hiplib, FUSED)(C.byref(_cshape(conv, st)), *st.pool, *_distinct(), None) == UNSUPPORTED, st
        assert stage.conv_maxpool_stage_route(_cshape(conv, st), st.pool) == stage.ROUTE_SEQUENCE, st
    routes = {stage.conv_maxpool_stage_route(_cshape(conv, st), st.pool) for st in R.FUSED_STAGES}
    assert routes == {stage.ROUTE_FUSED, stage.ROUTE_SEQUENCE}            # the main call takes both on this list
    assert conv.conv_route(_cshape(conv, R.SEQUENCE_STAGES[-1]), conv.PASS_FORWARD) == conv.ROUTE_FAST


def test_workspace_query(stage, conv):
    nets = [R.ST(N, C_, H, W, K, k, k, (p, p)) for (C_, H, W, K, k, p), _, _ in NETS for N in (50, 1517)]
    for st in R.GPU_STAGES + nets:
        s, shape = st.conv, _cshape(conv, st)
        OH, OW = CR.output_dims(s)
        pooled = s.N * s.K * (OH // st.pool[0]) * (OW // st.pool[1])
        elems = s.N * s.K * OH * OW + 2 * s.K + pooled        # the map, save_mean / save_std, a save_pool
        fused = stage.conv_maxpool_stage_route(shape, st.pool) == stage.ROUTE_FUSED
        assert stage.conv_maxpool_stage_workspace_bytes(shape, st.pool) == (0 if fused else 4 * elems)
        assert stage.conv_maxpool_stage_workspace_bytes(shape, st.pool, route="sequence") == 4 * elems
        assert stage.conv_maxpool_stage_workspace_bytes(shape, st.pool, route="fused") == 0
        assert stage.conv_maxpool_stage_workspace_bytes_f64(shape, st.pool) == 8 * elems
        assert stage.conv_maxpool_stage_workspace_bytes_f64(shape, st.pool, route="sequence") == 8 * elems
        empty = _cshape(conv, st, N=0)
        for q in (stage.conv_maxpool_stage_workspace_bytes, stage.conv_maxpool_stage_workspace_bytes_f64):
            assert q(empty, st.pool) == 0 and q(empty, st.pool, route="sequence") == 0


def test_binding_refuses_before_the_library(stage):
    import torch
    from mms_answer_selection_amd import capi
    fwd = stage.conv_maxpool_stage_forward
    x, w, k = torch.zeros(2, 4, 12, 12), torch.zeros(6, 4, 3, 3), torch.zeros(6)
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (3, 2), k, k, k, k)                                           # 10 % 3
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (0, 2), k, k, k, k)
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (2, 5), k, k, k, torch.zeros(5))                              # shift's shape
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (2, 5), k, k, k, k, top=torch.zeros(2, 6, 10, 10))
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (2, 5), k, k, k, k, save_pool=torch.zeros(2, 6, 5, 3))
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, w, None, (2, 5), k, k, k, k, route="fast")
    with pytest.raises(capi.MMSArgumentError):
        stage.conv_maxpool_stage_forward_f64(x.double(), w.double(), None, (2, 5), *([k.double()] * 4), route="fused")
    with pytest.raises(capi.MMSArgumentError):
        fwd(x, torch.zeros(6, 3, 3, 3), None, (2, 5), k, k, k, k)
    with pytest.raises(capi.MMSError):
        fwd(x, w, None, (2, 5), k, k, k, k)                                           # host tensors: no CPU path
