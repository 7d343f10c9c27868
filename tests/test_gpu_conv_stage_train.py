"""GPU suite of the TRAIN-phase stage Convolution -> BN -> AvePool / MaxPool -> TanH (include/mms_conv_stage_train.h):
both passes on every route against the float64 model, y against the convolution's own words, exact probes on which the
fused and the sequence route must agree to the word, determinism under garbage workspaces and shifted bases, padding
pixels, optional backward outputs, and the sequence route against the public calls issued here; then the same on the
launch sizes the main call routes to the fused forward (R.LARGE_STAGES: several chunks per channel in launch 2, more
than 256 partials per channel, the main call inside and beside the measured spans)."""
import functools

import numpy as np
import pytest
import torch

import conv_stage_train_reference as R
import test_gpu_conv as V
from pooled_stage_suite import BAR, GuardedWorkspace, assert_words_equal, check_parity, cshape, same_words
from util import SEED

pytestmark = pytest.mark.gpu


def IDS(stages):
    return [R.stage_id(st) for st in stages]


BACKWARD = ("bottom_diff", "weight_diff", "bias_diff", "scale_diff", "shift_diff")
FORWARD_INPUTS = ("x", "weight", "bias", "scale", "shift")


@functools.lru_cache(maxsize=None)
def inputs(st, dtype):
    return R.conditioned_inputs(st, dtype, SEED)


@functools.lru_cache(maxsize=None)
def model(st, method, dtype):
    out = R.model_outputs(st, method, inputs(st, dtype), np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probe(st):
    return R.integer_probe(st, SEED)


def mod():
    from mms_answer_selection_amd import conv_stage_train
    return conv_stage_train


class GarbageWorkspace(GuardedWorkspace):
    """GuardedWorkspace with another filling than NaN words."""

    def __init__(self, nbytes, fill):
        super().__init__(nbytes)
        self.buf[V.GUARD:V.GUARD + nbytes // 4].fill_(fill)


def run(st, method, inp, dtype=np.float32, route="auto", shift=0, ws_fill=None, outputs=(True,) * 5, memory=R.BN_MEMORY,
        backward=True):
    """Forward, then backward on top of the initial parameter diffs.  Every output starts as NaN (scale_diff and
    shift_diff as 123, weight_diff and bias_diff as the inputs' diffs) between guard zones, `shift` elements off a
    16-byte boundary; ws_fill: a workspace of exactly the queried size filled with that value, guarded.
    -> every output on the host under R.OUTPUTS' names; a backward output not asked for is absent, its prefill intact."""
    m, s, sfx = mod(), st.conv, "" if dtype == np.float32 else "_f64"
    fwd, bwd = getattr(m, "conv_stage_train_forward" + sfx), getattr(m, "conv_stage_train_backward" + sfx)
    query = getattr(m, "conv_stage_train_workspace_bytes" + sfx)
    kw = dict(stride=s.stride, pad=s.pad, group=s.group)
    dev = {k: (None if inp[k] is None else V.placed(inp[k], dtype, shift)) for k in FORWARD_INPUTS + ("top_diff",)}
    K, pooled, nan = s.K, R.pooled_shape(st), float("nan")
    OH, OW = R.CR.output_dims(s)
    g = dict(y=V.Guarded((s.N, K, OH, OW), dtype, nan, shift), top=V.Guarded(pooled, dtype, nan, shift),
             save_pool=V.Guarded(pooled, dtype, nan, shift), save_mean=V.Guarded((K,), dtype, nan, shift),
             save_std=V.Guarded((K,), dtype, nan, shift),
             running_mean=V.Guarded((K,), dtype, np.asarray(inp["running_mean"]), shift),
             running_var=V.Guarded((K,), dtype, np.asarray(inp["running_var"]), shift))

    def workspace(r):
        return None if ws_fill is None else GarbageWorkspace(query(cshape(st), st.pool, method, route=r), ws_fill)

    ws = workspace(route)
    fwd(dev["x"], dev["weight"], dev["bias"], st.pool, method, dev["scale"], dev["shift"], g["running_mean"].t,
        g["running_var"].t, g["y"].t, g["top"].t, g["save_pool"].t, g["save_mean"].t, g["save_std"].t, bn_memory=memory,
        ws=ws, route=route, **kw)
    torch.cuda.synchronize()
    if ws:
        ws.check()
    out = {k: v.host(k) for k, v in g.items()}
    if backward:
        b = dict(bottom_diff=V.Guarded(inp["x"].shape, dtype, nan, shift),
                 weight_diff=V.Guarded(inp["weight"].shape, dtype, np.asarray(inp["weight_diff0"]), shift),
                 scale_diff=V.Guarded((K,), dtype, 123.0, shift), shift_diff=V.Guarded((K,), dtype, 123.0, shift))
        if inp["bias_diff0"] is not None:
            b["bias_diff"] = V.Guarded((K,), dtype, np.asarray(inp["bias_diff0"]), shift)
        given = {k: (b[k].t if k in b and want else None) for k, want in zip(BACKWARD, outputs)}
        ws = workspace("auto")
        bwd(dev["x"], dev["weight"], st.pool, method, g["y"].t, g["top"].t, dev["top_diff"], g["save_pool"].t,
            dev["scale"], dev["shift"], g["save_mean"].t, g["save_std"].t, ws=ws, **given, **kw)
        torch.cuda.synchronize()
        if ws:
            ws.check()
        for k, v in b.items():
            h = v.host(k)
            if given[k] is not None:
                out[k] = h
            elif k == "bottom_diff":
                assert np.isnan(h).all(), k + " was not asked for"
            elif k in ("scale_diff", "shift_diff"):
                assert (h == 123.0).all(), k + " was not asked for"
            else:
                assert_words_equal(h, np.array(inp[k + "0"], dtype=dtype), k + " was not asked for")
    for k in FORWARD_INPUTS + ("top_diff",):
        if inp[k] is not None:
            assert_words_equal(V.host(dev[k]), np.array(inp[k], dtype=dtype), k + " is an input")
    return out


def routes_of(st, dtype=np.float32):
    if dtype != np.float32:
        return ("auto",)
    return ("auto", "sequence", "fused") if st in R.FUSED_STAGES else ("auto", "sequence")


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.PARITY_STAGES, ids=IDS(R.PARITY_STAGES))
def test_parity(st, method, hiplib):
    """The main call, the forced sequence and the forced fused launches in float, and the double call: every output
    of both passes against the float64 model at the project's bars."""
    from mms_answer_selection_amd import capi
    if st in R.SEQUENCE_STAGES:
        assert mod().conv_stage_train_route(cshape(st), st.pool, method) == mod().ROUTE_SEQUENCE
        with pytest.raises(capi.MMSError):
            run(st, method, inputs(st, np.float32), route="fused")
    for dtype in (np.float32, np.float64):
        for route in routes_of(st, dtype):
            print(R.stage_id(st), method, dtype.__name__, route)
            check_parity(run(st, method, inputs(st, dtype), dtype, route), model(st, method, dtype), dtype)


@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS(R.GPU_STAGES))
def test_y_is_the_convolutions_own_words(st, hiplib):
    from mms_answer_selection_amd import conv
    s, inp = st.conv, inputs(st, np.float32) if st in R.PARITY_STAGES else R._draw(st, np.float32, SEED)
    dev = {k: (None if inp[k] is None else V.placed(inp[k], np.float32)) for k in ("x", "weight", "bias")}
    want = V.host(conv.conv_forward(dev["x"], dev["weight"], dev["bias"], stride=s.stride, pad=s.pad, group=s.group))
    for method in R.METHODS:
        for route in routes_of(st):
            got = run(st, method, inp, route=route, backward=False)["y"]
            assert_words_equal(got, want, "y, %s, %s route" % (method, route))


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.FUSED_STAGES, ids=IDS(R.FUSED_STAGES))
def test_exact_probe_fused_equals_sequence(st, method, hiplib):
    """Integer y, exact partial sums: the two routes give the same words in every output of both passes, and the
    statistics are the float32 restatement from the int64 sums, bit for bit."""
    inp = probe(st)
    y, s0, s1 = R.probe_sums(st, inp)
    fused = run(st, method, inp, route="fused", memory=R.PROBE_MEMORY)
    seq = run(st, method, inp, route="sequence", memory=R.PROBE_MEMORY)
    auto = run(st, method, inp, memory=R.PROBE_MEMORY)
    for k, v in fused.items():
        assert not np.isnan(v).any(), k
    same_words(fused, seq, "exact probe, fused against sequence")
    same_words(auto, seq, "exact probe, the main call against sequence")
    assert_words_equal(fused["y"], y.astype(np.float32), "y against the int64 model")
    for k, want in zip(("save_mean", "save_std", "running_mean", "running_var"), R.probe_statistics(st, inp, s0, s1)):
        assert_words_equal(fused[k], want, k + " against the int64 sums")
    if method == R.MAX:                       # ties: the scan's winner by the sign of scale, first element for scale == 0
        w = R.BM.windows(y, *st.pool)
        mean, std = fused["save_mean"], fused["save_std"]
        for k, pick in ((R.ZERO_CHANNEL, w[:, R.ZERO_CHANNEL, ..., 0]),
                        (R.NEGATIVE_CHANNEL, w[:, R.NEGATIVE_CHANNEL].min(axis=-1)),
                        (R.POSITIVE_CHANNEL, w[:, R.POSITIVE_CHANNEL].max(axis=-1))):
            want = (pick.astype(np.float32) + (-mean[k])) / std[k]
            assert_words_equal(fused["save_pool"][:, k], want, "save_pool of channel %d" % k)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS(R.GPU_STAGES))
def test_determinism_and_independence(st, method, hiplib):
    """A second run, a workspace of exactly the queried size full of NaN words and one full of other garbage, every
    array one element off a 16-byte boundary: the same words on every route."""
    inp = inputs(st, np.float32) if st in R.PARITY_STAGES else R._draw(st, np.float32, SEED)
    for dtype in (np.float32, np.float64):
        for route in routes_of(st, dtype):
            first = run(st, method, inp, dtype, route)
            same_words(run(st, method, inp, dtype, route), first, "second run, " + route)
            same_words(run(st, method, inp, dtype, route, shift=1, ws_fill=float("nan")), first, "NaN workspace, " + route)
            same_words(run(st, method, inp, dtype, route, shift=1, ws_fill=-3.5e37), first, "garbage workspace, " + route)


@pytest.mark.parametrize("method", R.METHODS)
def test_padding_contributes_nothing(method, hiplib):
    """Shape B's 23 images against its first 20 (two full groups of ten) and its last 3 (one ragged group) run alone:
    the exact probe's sums add up, so the statistics of the whole are those of the parts' sums."""
    inp = probe(R.B)
    _, s0, s1 = R.probe_sums(R.B, inp)
    sums = []
    for lo, hi in ((0, 20), (20, 23)):
        part_st = R.ST(hi - lo, *R.B.conv[1:7], R.B.pool)
        part = dict(inp, x=inp["x"][lo:hi], top_diff=inp["top_diff"][lo:hi])
        out = run(part_st, method, part, route="fused", memory=R.PROBE_MEMORY, backward=False)
        _, p0, p1 = R.probe_sums(R.B, inp, slice(lo, hi))
        want = R.probe_statistics(part_st, part, p0, p1)
        for k, w in zip(("save_mean", "save_std", "running_mean", "running_var"), want):
            assert_words_equal(out[k], w, "%s of images %d..%d" % (k, lo, hi))
        sums.append((p0, p1))
    assert (sums[0][0] + sums[1][0] == s0).all() and (sums[0][1] + sums[1][1] == s1).all()
    whole = run(R.B, method, inp, route="fused", memory=R.PROBE_MEMORY, backward=False)
    for k, w in zip(("save_mean", "save_std", "running_mean", "running_var"), R.probe_statistics(R.B, inp, s0, s1)):
        assert_words_equal(whole[k], w, k + " of all 23 images")
    # shape A's band tail (F: bands of 12 and 8 rows) is in the exact probes by construction


@pytest.mark.parametrize("dtype", V.DTYPES, ids=V.IDS)
@pytest.mark.parametrize("method", R.METHODS)
def test_optional_backward_outputs(method, dtype, hiplib):
    """Each subset of NULL outputs leaves the others' words unchanged and its own prefill intact (run checks it);
    weight_diff and bias_diff are accumulated into, the other three overwritten; with no output the call is refused."""
    from mms_answer_selection_amd import capi
    st = R.C
    inp = inputs(st, dtype)
    full = run(st, method, inp, dtype)
    want = model(st, method, dtype)
    bar = BAR[dtype]
    # Accumulated on top of what was there: the prefill and weight_diff's batch term are both far above the bar, so the
    # model is met only by adding.  (bias_diff's batch term is the sum of dy over a channel, which BN's backward makes
    # zero: there the model is met only by KEEPING the prefill.)
    assert np.abs(want["weight_diff"] - np.asarray(inp["weight_diff0"], np.float64)).max() > 100 * bar
    for k0 in ("weight_diff0", "bias_diff0"):
        assert np.abs(np.asarray(inp[k0])).max() > 100 * bar
    check_parity(full, want, dtype)
    for mask in range(1, 31):
        outputs = tuple(bool(mask >> b & 1) for b in range(5))
        part = run(st, method, inp, dtype, outputs=outputs)
        assert len(part) == len(full) - outputs.count(False)
        for k, v in part.items():
            assert_words_equal(v, full[k], "%s with outputs %s" % (k, outputs))
    with pytest.raises(capi.MMSError):
        run(st, method, inp, dtype, outputs=(False,) * 5)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", [R.A, R.D], ids=IDS([R.A, R.D]))
def test_sequence_route_is_the_public_calls(st, method, hiplib):
    """The forced sequence forward and the backward against mms_conv_forward_f32, the float BN -> pooling -> TanH forward
    and backward of the method and mms_conv_backward_f32 issued here, word for word."""
    from mms_answer_selection_amd import bn_maxpool, capi, conv
    s, inp = st.conv, inputs(st, np.float32)
    got = run(st, method, inp, route="sequence")
    kw = dict(stride=s.stride, pad=s.pad, group=s.group)
    dev = {k: (None if inp[k] is None else V.placed(inp[k], np.float32)) for k in inp}
    y = conv.conv_forward(dev["x"], dev["weight"], dev["bias"], **kw)
    K, pooled = s.K, R.pooled_shape(st)
    top, sp = (torch.full(pooled, float("nan"), device="cuda") for _ in range(2))
    sm, ss = torch.empty(K, device="cuda"), torch.empty(K, device="cuda")
    rm, rv = dev["running_mean"].clone(), dev["running_var"].clone()
    dy, dsc, dsh = torch.empty_like(y), torch.empty(K, device="cuda"), torch.empty(K, device="cuda")
    if method == R.AVE:
        capi.bn_pool_tanh_forward(y, st.pool, dev["scale"], dev["shift"], rm, rv, top, sp, sm, ss, phase=0,
                                  bn_memory=R.BN_MEMORY)
        capi.bn_pool_tanh_backward(y, st.pool, top, dev["top_diff"], sp, dev["scale"], sm, ss, bottom_diff=dy,
                                   scale_diff=dsc, shift_diff=dsh)
    else:
        bn_maxpool.bn_maxpool_tanh_forward(y, st.pool, dev["scale"], dev["shift"], rm, rv, top, sp, sm, ss, phase=0,
                                           bn_memory=R.BN_MEMORY)
        bn_maxpool.bn_maxpool_tanh_backward(y, st.pool, top, dev["top_diff"], sp, dev["scale"], dev["shift"], sm, ss,
                                            bottom_diff=dy, scale_diff=dsc, shift_diff=dsh)
    dx, dw, db = torch.empty_like(dev["x"]), dev["weight_diff0"].clone(), dev["bias_diff0"].clone()
    conv.conv_backward(dev["x"], dev["weight"], dy, dx, dw, db, **kw)
    torch.cuda.synchronize()
    want = dict(y=y, top=top, save_pool=sp, save_mean=sm, save_std=ss, running_mean=rm, running_var=rv, bottom_diff=dx,
                weight_diff=dw, bias_diff=db, scale_diff=dsc, shift_diff=dsh)
    same_words(got, {k: V.host(v) for k, v in want.items()}, "the sequence route against the public calls")


# ---- the launch sizes the main call routes to the fused forward (R.LARGE_STAGES) ---------------------------------------
# What each shape reaches is held to the C++ by tests/test_conv_stage_train_plans.py, on the CPU; the bar is the
# project's, which float32 alone meets on the fused order of sums (same file).  Forward only beyond the exact probe: the
# fused route has no backward of its own, and the large shapes' inputs carry no top-two gap.
STATISTICS = ("save_mean", "save_std", "running_mean", "running_var")
LARGE_ROUTES = ("auto", "sequence", "fused")


@functools.lru_cache(maxsize=None)
def large_inputs(st, dtype):
    return R.forward_conditioned_inputs(st, dtype, SEED)


@functools.lru_cache(maxsize=None)
def large_model(st, method, dtype):
    out = R.model_forward(st, method, large_inputs(st, dtype))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def large_forward(st, method, route):
    """The float forward on the conditioned inputs, once per (shape, method, route); shared, never modified."""
    out = run(st, method, large_inputs(st, np.float32), route=route, backward=False)
    for v in out.values():
        v.setflags(write=False)
    return out


def routed(st, method):
    """The forced route whose words the main call must give: LARGE_PLANS' claim, which the CPU suite holds to the route
    call."""
    named = {mod().ROUTE_SEQUENCE: R.SEQ, mod().ROUTE_FUSED: R.FUSED}[mod().conv_stage_train_route(cshape(st), st.pool, method)]
    assert named == R.LARGE_PLANS[st]["route"][method]
    return named


def check_forward_parity(got, want, dtype, what):
    assert sorted(got) == sorted(want) == sorted(R.FORWARD_OUTPUTS)
    ratios = {}
    for k in R.FORWARD_OUTPUTS:
        assert got[k].dtype == dtype and np.isfinite(got[k]).all(), k
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        ratios[k] = float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) / (BAR[dtype] * scale)
    print("%-32s %s" % (what, "  ".join("%s %.3g" % (k, ratios[k]) for k in R.FORWARD_OUTPUTS)))
    for k in R.FORWARD_OUTPUTS:
        assert ratios[k] <= 1.0, "%s, %s: %.3g of the bar" % (k, what, ratios[k])


# ---- one shape per instantiation of the pooling epilogue (R.INSTANTIATION_STAGES, R.EXACT_MEAN_STAGES, R.TRAIN_ONLY_STAGES) -------------------
# They join the exact probe, y's own words and the determinism tests above through R.FUSED_STAGES; what each reaches is
# held to the C++ by tests/test_conv_stage_plans.py, on the CPU.
NEW_STAGES = R.INSTANTIATION_STAGES + R.EXACT_MEAN_STAGES + R.TRAIN_ONLY_STAGES


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", NEW_STAGES, ids=IDS(NEW_STAGES))
def test_instantiation_forward_parity(st, method, hiplib):
    """The forced fused, the forced sequence and the main call in float, and the double call: the seven forward outputs
    against the float64 model at the project's bars (printed: each output's share of its bar)."""
    for route in LARGE_ROUTES:
        got = run(st, method, large_inputs(st, np.float32), route=route, backward=False)
        check_forward_parity(got, large_model(st, method, np.float32), np.float32, "%s f32 %s" % (method, route))
    got = run(st, method, large_inputs(st, np.float64), np.float64, backward=False)
    check_forward_parity(got, large_model(st, method, np.float64), np.float64, "%s f64" % method)


@pytest.mark.parametrize("st", R.ORDER_STAGES, ids=IDS(R.ORDER_STAGES))
def test_order_probe_ave(st, hiplib):
    """R.order_probe: every element of y is one exact product, so y is the exact map word for word on both routes.
    save_pool before launch 2 is not observable; the finished save_pool, top and the statistics of the fused route are
    held to the float32 restatement of bn_pool_reference's fused TRAIN forward on that map -- the window one chain in
    (h, w) order -- at the float bar (printed: each output's share of it)."""
    ost = R.SR.order_stage(st)
    inp = R.order_probe(ost, R.SR.ORDER_SEED)
    y = R.SR.order_probe_map(ost, inp)
    assert min(R.SR.order_shares(y, ost.pool).values()) >= R.SR.ORDER_MIN_SHARE
    want = R.order_probe_forward(ost, inp, y)
    for route in ("fused", "sequence"):
        got = run(ost, R.AVE, inp, route=route, backward=False)
        assert_words_equal(got["y"], y, "order probe, y, %s route" % route)
        ratios = {}
        for k, w in want.items():
            assert np.isfinite(got[k]).all(), k
            scale = max(1.0, float(np.max(np.abs(w))))
            ratios[k] = float(np.max(np.abs(got[k].astype(np.float64) - w.astype(np.float64)))) / (BAR[np.float32] * scale)
        print("%-9s %s" % (route, "  ".join("%s %.3g" % kv for kv in ratios.items())))
        for k, v in ratios.items():
            assert v <= 1.0, "%s, %s route: %.3g of the bar" % (k, route, v)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS(R.LARGE_STAGES))
def test_large_exact_probe_fused_equals_sequence(st, method, hiplib):
    """Integer y, every partial sum exact in any order: the fused route (whatever its count of partials per thread and
    of chunks per channel), the sequence and the main call give the same words in every output of both passes; y is the
    int64 model's and the statistics are the float32 restatement from the int64 sums, bit for bit -- a statistic written
    twice, a partial dropped, doubled or read from another slot shows here."""
    inp = probe(st)
    y, s0, s1 = R.probe_sums(st, inp)
    fused = run(st, method, inp, route="fused", memory=R.PROBE_MEMORY)
    seq = run(st, method, inp, route="sequence", memory=R.PROBE_MEMORY)
    auto = run(st, method, inp, memory=R.PROBE_MEMORY)
    for k, v in fused.items():
        assert not np.isnan(v).any(), k
    same_words(fused, seq, "exact probe, fused against sequence")
    same_words(auto, seq, "exact probe, the main call against sequence")
    assert_words_equal(fused["y"], y.astype(np.float32), "y against the int64 model")
    for k, want in zip(STATISTICS, R.probe_statistics(st, inp, s0, s1)):
        assert_words_equal(fused[k], want, k + " against the int64 sums")
    if method == R.MAX:                       # ties: the scan's winner by the sign of scale, first element for scale == 0
        w = R.BM.windows(y, *st.pool)
        mean, std = fused["save_mean"], fused["save_std"]
        for k, pick in ((R.ZERO_CHANNEL, w[:, R.ZERO_CHANNEL, ..., 0]),
                        (R.NEGATIVE_CHANNEL, w[:, R.NEGATIVE_CHANNEL].min(axis=-1)),
                        (R.POSITIVE_CHANNEL, w[:, R.POSITIVE_CHANNEL].max(axis=-1))):
            want = (pick.astype(np.float32) + (-mean[k])) / std[k]
            assert_words_equal(fused["save_pool"][:, k], want, "save_pool of channel %d" % k)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS(R.LARGE_STAGES))
def test_large_forward_parity(st, method, hiplib):
    """The main call, the forced sequence and the forced fused launches in float, and the double call: the seven forward
    outputs against the float64 model at the project's bars (printed: each output's share of its bar); y is the
    convolution's own words on every float route."""
    from mms_answer_selection_amd import conv
    s, inp = st.conv, large_inputs(st, np.float32)
    dev = {k: V.placed(inp[k], np.float32) for k in ("x", "weight", "bias")}
    own = V.host(conv.conv_forward(dev["x"], dev["weight"], dev["bias"], stride=s.stride, pad=s.pad, group=s.group))
    for route in LARGE_ROUTES:
        got = large_forward(st, method, route)
        check_forward_parity(got, large_model(st, method, np.float32), np.float32, "%s f32 %s" % (method, route))
        assert_words_equal(got["y"], own, "y, %s, %s route" % (method, route))
    got = run(st, method, large_inputs(st, np.float64), np.float64, backward=False)
    check_forward_parity(got, large_model(st, method, np.float64), np.float64, "%s f64" % method)


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS(R.LARGE_STAGES))
def test_large_determinism_and_workspace(st, method, hiplib):
    """On every float route: a second run with every array one element off a 16-byte boundary, one with a workspace of
    exactly the queried size full of NaN words and one full of other garbage give the first run's words and leave the
    workspace's guard zones alone -- where the main call fuses (R.R; R.R_PLUS and R.W with MAX) the queried size is the
    main call's own, max(the partial sums, the backward's carve).  The forced fused query holds the partial sums."""
    inp = large_inputs(st, np.float32)
    partials = 2 * st.conv.K * R.LARGE_PLANS[st]["plan"]["groups"] * 4
    assert mod().conv_stage_train_workspace_bytes(cshape(st), st.pool, method, route="fused") >= partials
    for route in LARGE_ROUTES:
        first = large_forward(st, method, route)
        same_words(run(st, method, inp, route=route, shift=1, backward=False), first, "shifted second run, " + route)
        same_words(run(st, method, inp, route=route, ws_fill=float("nan"), backward=False), first, "NaN workspace, " + route)
        same_words(run(st, method, inp, route=route, ws_fill=-3.5e37, backward=False), first, "garbage workspace, " + route)


def routes_differ(st, method):
    """The outputs in which the forced fused and the forced sequence forward differ in some word."""
    fused, seq = large_forward(st, method, "fused"), large_forward(st, method, "sequence")
    return [k for k in R.FORWARD_OUTPUTS if (fused[k].view(np.uint32) != seq[k].view(np.uint32)).any()]


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.LARGE_STAGES, ids=IDS(R.LARGE_STAGES))
def test_the_main_call_fuses_inside_the_spans(st, method, hiplib):
    """On conditioned inputs the main call gives the words of the forced route the span table names: fused at R.R (both
    methods) and at R.R_PLUS and R.W with MAX; the sequence at R.R_MINUS, at R.R_PLUS and R.W with AVE and at R.P and
    R.Q.  Where the two forced routes differ in a last bit (printed) this tells which one the main call ran;
    test_the_two_routes_differ_somewhere asserts that they do."""
    named = routed(st, method)
    print("%s %s: the main call is the %s route; fused and sequence differ in %s" % (
        R.stage_id(st), method, named, routes_differ(st, method) or "no word"))
    same_words(large_forward(st, method, "auto"), large_forward(st, method, named), "the main call against " + named)


def test_the_two_routes_differ_somewhere(hiplib):
    """What makes test_the_main_call_fuses_inside_the_spans tell the routes apart: at one of its shapes at least, inside
    a span and beside one, the two routes' statistics differ in some word (their orders of sums differ)."""
    inside = [(st, m) for st in R.LARGE_STAGES for m in R.METHODS if R.LARGE_PLANS[st]["route"][m] == R.FUSED]
    beside = [(st, m) for st in (R.R_MINUS, R.R_PLUS, R.W) for m in R.METHODS if R.LARGE_PLANS[st]["route"][m] == R.SEQ]
    assert len(inside) == 4 and len(beside) == 4
    for cases in (inside, beside):
        assert any(set(routes_differ(st, m)) & set(STATISTICS + ("top", "save_pool")) for st, m in cases)


@pytest.mark.parametrize("method", R.METHODS)
def test_finish_chunks_partition_the_batch(method, hiplib):
    """R.P: 1025 pooled elements per channel, so launch 2's second workgroup of a channel finishes one element, the last
    image's last.  Every element of top and save_pool is finite (none left as the NaN prefill or as the raw pooled
    value's garbage), that element is at the model's value in every channel, and the first 40 images' y is the 40-image
    run's (one chunk), word for word."""
    st = R.P
    assert R.LARGE_PLANS[st]["finish"] == dict(windows=1025, wpc=1024, chunks=2, last=1)
    got, want = large_forward(st, method, "fused"), large_model(st, method, np.float32)
    for k in ("top", "save_pool"):
        assert np.isfinite(got[k]).all(), k
        lone_got = got[k].transpose(1, 0, 2, 3).reshape(st.conv.K, -1)[:, 1024:]
        lone_want = want[k].transpose(1, 0, 2, 3).reshape(st.conv.K, -1)[:, 1024:]
        assert lone_got.shape == (st.conv.K, 1)
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        err = float(np.max(np.abs(lone_got.astype(np.float64) - lone_want)))
        print("%s, element 1024 of each channel: %.3g of the bar" % (k, err / (BAR[np.float32] * scale)))
        assert err <= BAR[np.float32] * scale, k
    inp = large_inputs(st, np.float32)
    st40 = R.ST(40, *st.conv[1:7], st.pool)
    part = {k: (v[:40] if k in ("x", "top_diff") else v) for k, v in inp.items()}
    one_chunk = run(st40, method, part, route="fused", backward=False)
    assert np.isfinite(one_chunk["top"]).all() and np.isfinite(one_chunk["save_pool"]).all()
    assert_words_equal(one_chunk["y"], got["y"][:40], "y of images 0..39")


@pytest.mark.parametrize("dtype", V.DTYPES, ids=V.IDS)
def test_empty_batch_writes_nothing(dtype, hiplib):
    m, t = mod(), V.TORCH[dtype]
    sfx = "" if dtype == np.float32 else "_f64"
    x = torch.empty(0, 4, 12, 12, dtype=t, device="cuda")
    w, k = V.Guarded((6, 4, 3, 3), dtype, 1.0), [V.Guarded((6,), dtype, 1.5) for _ in range(4)]
    for method in R.METHODS:
        for route in ("auto", "sequence") + (("fused",) if dtype == np.float32 else ()):
            saved = getattr(m, "conv_stage_train_forward" + sfx)(x, w.t, None, (2, 5), method, *(g.t for g in k),
                                                                 route=route)
            assert tuple(saved.y.shape) == (0, 6, 10, 10) and tuple(saved.top.shape) == (0, 6, 5, 2)
    torch.cuda.synchronize()
    assert (w.host("weight") == 1.0).all()
    for g in k:
        assert (g.host("a BN array") == 1.5).all()
