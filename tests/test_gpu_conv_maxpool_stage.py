"""GPU suite: the TEST-phase Convolution -> BN -> MaxPool -> TanH stage (include/mms_conv_maxpool_stage.h,
csrc/conv_stage.hip) against tests/conv_maxpool_stage_reference.py.  The fused launch
(mms_conv_maxpool_stage_forward_fused_f32, at every shape it reaches, whichever route the main call's measured rules
pick there) is held to the sequence route -- the two public calls -- by EQUALITY on integer probes, whose windows are
full of ties, and on conditioned inputs too wherever both routes cut the input channels alike; the main call to the
route mms_conv_maxpool_stage_route names; every shape to the float64 model at the project's 1e-5 (float32) and 1e-12
(float64) in assert_close's metric; the fixed order and the workspace's irrelevance by equality of words between two
runs.  Every stage has a channel of scale 0, a negative one and a positive one."""
import functools

import numpy as np
import pytest
import torch

import bn_maxpool_reference as BM
import conv_maxpool_stage_reference as R
from test_gpu_conv import TORCH, Guarded, assert_words_equal, host, placed
from test_gpu_conv_stage import NAMES, GuardedWorkspace, cshape
from util import SEED, TOL, assert_bitexact, assert_close

pytestmark = pytest.mark.gpu

BAR = {np.float32: TOL, np.float64: 1e-12}
FUSED_IDS = [R.stage_id(st) for st in R.FUSED_STAGES]
ALL_IDS = [R.stage_id(st) for st in R.GPU_STAGES]


def mod():
    from mms_answer_selection_amd import conv_maxpool_stage
    return conv_maxpool_stage


def route_of(st):
    return mod().conv_maxpool_stage_route(cshape(st), st.pool)


def query(st, dtype, route):
    m = mod()
    q = m.conv_maxpool_stage_workspace_bytes if dtype == np.float32 else m.conv_maxpool_stage_workspace_bytes_f64
    return q(cshape(st), st.pool, route=route)


def run(st, inp, dtype=np.float32, route="auto", shift=0, guarded_ws=False, save_pool=True):
    """One forward.  top and save_pool start as NaN between guard zones; x, weight, top and save_pool are `shift`
    elements off a 16-byte boundary.  -> {"top"[, "save_pool"]} on the host; the inputs are checked to be unchanged."""
    m = mod()
    fwd = m.conv_maxpool_stage_forward if dtype == np.float32 else m.conv_maxpool_stage_forward_f64
    s = st.conv
    dev = {k: (None if inp[k] is None else placed(inp[k], dtype, shift)) for k in NAMES}
    nan = float("nan")
    top = Guarded(R.pooled_shape(st), dtype, nan, shift)
    sp = Guarded(R.pooled_shape(st), dtype, nan, shift) if save_pool else None
    ws = GuardedWorkspace(query(st, dtype, route)) if guarded_ws and route != "fused" else None     # fused takes none
    got = fwd(dev["x"], dev["weight"], dev["bias"], st.pool, dev["mean"], dev["var"], dev["scale"], dev["shift"], top.t,
              sp.t if sp else None, stride=s.stride, pad=s.pad, group=s.group, ws=ws, route=route)
    assert got is top.t
    torch.cuda.synchronize()
    if ws:
        ws.check()
    out = dict(top=top.host("top"))
    if sp:
        out["save_pool"] = sp.host("save_pool")
    for k in NAMES:
        if inp[k] is not None:
            assert_bitexact(host(dev[k]), np.array(inp[k], dtype=dtype), k + " is an input")
    return out


@functools.lru_cache(maxsize=None)
def inputs(st, dtype):
    return R.conditioned_inputs(st, dtype, SEED)


@functools.lru_cache(maxsize=None)
def model(st, dtype):
    """The float64 model on the inputs as the device gets them, computed once and shared (never modified)."""
    out = R.model_outputs(st, inputs(st, dtype), np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def named_route(st):
    """The forced route whose words the main call must give: the one mms_conv_maxpool_stage_route names."""
    return {mod().ROUTE_FUSED: "fused", mod().ROUTE_SEQUENCE: "sequence"}[route_of(st)]


@pytest.mark.parametrize("st", R.FUSED_STAGES, ids=FUSED_IDS)
def test_integer_probe_fused_equals_sequence(st, hiplib):
    """The map is exact whatever order its products are summed in, so both routes scan the same numbers -- small
    integers, so the windows are full of ties: the strict scan in either direction and the first-element rule of the
    zero-scale channel all show.  top and save_pool equal word for word, and save_pool equals the float32 restatement
    of the finish."""
    assert R.probe_bound(st) < 2 ** 24
    inp = R.integer_probe(st, SEED)
    fused, seq, auto = run(st, inp, route="fused"), run(st, inp, route="sequence"), run(st, inp)
    want_top, want_sp = R.probe_outputs(st, inp)
    for k in ("top", "save_pool"):
        assert not np.isnan(fused[k]).any(), k
        assert_words_equal(fused[k], seq[k], "integer probe, fused against sequence, " + k)
        assert_words_equal(auto[k], seq[k], "integer probe, the main call against sequence, " + k)
    assert_words_equal(fused["save_pool"], want_sp, "integer probe, save_pool against the float32 restatement")
    assert_close(fused["top"], want_top, TOL, "integer probe, top")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("st", R.GPU_STAGES, ids=ALL_IDS)
def test_parity_and_determinism(st, dtype, hiplib):
    """Per shape and route: the conditioned inputs against the float64 model at the bar; a second run with every
    operand one element off a 16-byte boundary and a NaN-filled workspace of exactly the queried size gives the same
    words and leaves the workspace's guard zones alone.  The main call gives the words of the route it names.  Where
    both routes have one chunk of input channels: fused and sequence, the same words."""
    from mms_answer_selection_amd import capi
    m = mod()
    inp, want = inputs(st, dtype), model(st, dtype)
    reached = st in R.FUSED_STAGES
    if not reached:
        assert route_of(st) == m.ROUTE_SEQUENCE
        with pytest.raises(capi.MMSError):
            run(st, inputs(st, np.float32), route="fused")        # refused host-side: the launch does not reach
    routes = ["fused", "sequence", "auto"] if dtype == np.float32 and reached else ["auto"]
    first = {}
    for route in routes:
        first[route] = run(st, inp, dtype, route)
        for k in ("top", "save_pool"):
            got = first[route][k]
            assert got.dtype == dtype and not np.isnan(got).any(), k
            scale = max(1.0, float(np.max(np.abs(want[k]))))
            print("%-8s %-9s %.3e" % (route, k, float(np.max(np.abs(got.astype(np.float64) - want[k]))) / scale))
    for route in routes:
        for k in ("top", "save_pool"):
            assert_close(first[route][k], want[k], BAR[dtype], "%s, %s route" % (k, route))
        second = run(st, inp, dtype, route, shift=1, guarded_ws=True)
        for k in ("top", "save_pool"):
            assert_words_equal(second[k], first[route][k], "%s, %s route, second run" % (k, route))
    if len(routes) == 3:
        for k in ("top", "save_pool"):
            assert_words_equal(first["auto"][k], first[named_route(st)][k], "the main call against the route it names, " + k)
            if st in R.SAME_CHUNK_STAGES:
                assert_words_equal(first["fused"][k], first["sequence"][k], "fused against sequence, " + k)


def test_the_main_call_reaches_both_routes_on_the_fused_list(hiplib):
    m = mod()
    assert [route_of(st) for st in R.NET_STAGES] == [m.ROUTE_SEQUENCE] * 5            # too few workgroups to pay
    assert [route_of(st) for st in R.MAIN_FUSED_STAGES] == [m.ROUTE_FUSED] * 2


@pytest.mark.parametrize("st", R.SEQUENCE_STAGES + R.NET_STAGES[:1],
                         ids=[R.stage_id(st) for st in R.SEQUENCE_STAGES + R.NET_STAGES[:1]])
def test_sequence_route_is_the_two_public_calls(st, hiplib):
    """The main call on a shape it routes to the sequence, against mms_conv_forward_f32 and
    mms_bn_maxpool_tanh_forward_f32 (TEST) issued here."""
    from mms_answer_selection_amd import bn_maxpool, conv
    assert route_of(st) == mod().ROUTE_SEQUENCE
    s, inp = st.conv, inputs(st, np.float32)
    got = run(st, inp)
    dev = {k: (None if inp[k] is None else placed(inp[k], np.float32)) for k in NAMES}
    y = conv.conv_forward(dev["x"], dev["weight"], dev["bias"], stride=s.stride, pad=s.pad, group=s.group)
    top, sp = (torch.full(R.pooled_shape(st), float("nan"), device="cuda") for _ in range(2))
    sm, ss = torch.empty(s.K, device="cuda"), torch.empty(s.K, device="cuda")
    bn_maxpool.bn_maxpool_tanh_forward(y, st.pool, dev["scale"], dev["shift"], dev["mean"], dev["var"], top, sp, sm, ss,
                                       phase=1)
    torch.cuda.synchronize()
    assert_words_equal(got["top"], host(top), "top")
    assert_words_equal(got["save_pool"], host(sp), "save_pool")


@pytest.mark.parametrize("st", [R.NET_STAGES[0], R.MAIN_FUSED_STAGES[0], R.SEQUENCE_STAGES[0]],
                         ids=[R.stage_id(st) for st in (R.NET_STAGES[0], R.MAIN_FUSED_STAGES[0], R.SEQUENCE_STAGES[0])])
def test_save_pool_is_optional(st, hiplib):
    inp = inputs(st, np.float32)
    for route in ("auto", "sequence") + (("fused",) if st in R.FUSED_STAGES else ()):
        full = run(st, inp, route=route)
        part = run(st, inp, route=route, save_pool=False, guarded_ws=True)
        assert sorted(part) == ["top"]
        assert_words_equal(part["top"], full["top"], "top without a save_pool, %s route" % route)
    st64 = run(st, inp, np.float64, save_pool=False, guarded_ws=True)
    assert_close(st64["top"], model(st, np.float32)["top"], 1e-12, "top without a save_pool, f64")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_empty_batch_writes_nothing(dtype, hiplib):
    m = mod()
    fwd = m.conv_maxpool_stage_forward if dtype == np.float32 else m.conv_maxpool_stage_forward_f64
    t = TORCH[dtype]
    x = torch.empty(0, 4, 12, 12, dtype=t, device="cuda")
    w, bias = Guarded((6, 4, 3, 3), dtype, 1.0), Guarded((6,), dtype, 2.0)
    k = [Guarded((6,), dtype, 1.5) for _ in range(4)]
    for route in ("auto", "sequence") + (("fused",) if dtype == np.float32 else ()):
        top = fwd(x, w.t, bias.t, (2, 5), *(g.t for g in k), route=route)
        assert tuple(top.shape) == (0, 6, 5, 2)
        sp = torch.empty(0, 6, 5, 2, dtype=t, device="cuda")
        fwd(x, w.t, bias.t, (2, 5), *(g.t for g in k), top, sp, route=route)
    torch.cuda.synchronize()
    assert (w.host("weight") == 1.0).all() and (bias.host("bias") == 2.0).all()
    for g in k:
        assert (g.host("a BN array") == 1.5).all()


@pytest.mark.parametrize("st", R.SAME_CHUNK_STAGES, ids=[R.stage_id(st) for st in R.SAME_CHUNK_STAGES])
def test_a_window_holding_one_nan(st, hiplib):
    """One NaN in x, in the middle of image 1: every element of y whose taps reach it is a NaN, in every channel.  The
    fused route gives the sequence route's words (a NaN for a NaN), and every window that holds none of those elements
    is at the model's value.  A window whose first element is not the NaN is finite in every channel: a NaN never wins
    a comparison; one that starts with it stays a NaN."""
    s, (ph, pw) = st.conv, st.pool
    inp = dict(inputs(st, np.float32))
    x = np.array(inp["x"])
    n, i, j = 1, s.H // 2 + 1, s.W // 2 + 1
    x[n, 0, i, j] = np.nan
    inp["x"] = x
    fused, seq = run(st, inp, route="fused"), run(st, inp, route="sequence")
    for k in ("top", "save_pool"):
        assert_bitexact(fused[k], seq[k], "a NaN in x, fused against sequence, " + k)
    y = np.zeros((s.N, s.K) + R.CR.output_dims(s), bool)
    y[n, :, max(0, i - s.kh + 1):i + 1, max(0, j - s.kw + 1):j + 1] = True            # the elements of y that are NaN
    w = BM.windows(y, ph, pw)
    touched, first = w.any(axis=-1), w[..., 0]
    assert touched.any() and not touched.all() and (touched & ~first).any()
    want = model(st, np.float32)
    for k in ("top", "save_pool"):
        got = np.where(touched, 0.0, fused[k])
        assert_close(got, np.where(touched, 0.0, want[k]), TOL, "windows without the NaN, " + k)
    assert np.isnan(fused["save_pool"][first]).all()                                  # it started the scan: it stays
    assert np.isfinite(fused["save_pool"][touched & ~first]).all() and np.isfinite(fused["top"][touched & ~first]).all()
