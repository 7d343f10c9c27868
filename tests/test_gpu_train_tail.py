"""GPU suite of the TRAIN-phase tail (include/mms_train_tail.h): both passes on every route against the float64 model
(tests/train_tail_reference.py) with AVE and MAX pooling, y against the convolution's own words, an exact probe on which
the fused and the sequence route agree to the word, both passes against the public calls issued here, determinism under
garbage workspaces and shifted bases, optional outputs, several workgroups in the second launch, and the route table.

Bars: 1e-5 (util.TOL, the project's fp32 bar) in float and 1e-12 in double, against the float64 model, scale-aware
(util.assert_close).  Word equality is equality of every bit.
"""
import functools

import numpy as np
import pytest
import torch

import head_reference as HR
import test_gpu_conv as V
import train_tail_reference as R
from pooled_stage_suite import BAR, GuardedWorkspace, check_parity, same_words
from util import SEED, assert_close

pytestmark = pytest.mark.gpu

POOL_IDS = lambda p: R.POOL_NAME[p]                                                 # noqa: E731
INPUTS = ("x", "weight", "bias", "scale", "shift", "overlap", "w1", "b1", "w2", "b2", "label")
WORDS = ("y", "flt", "save_pool", "h", "prob")            # the same chain on both routes, the statistics aside
STATISTICS = ("save_mean", "save_std", "running_mean", "running_var")


@pytest.fixture(scope="module")
def tail(hiplib):
    from mms_answer_selection_amd import conv, conv_stage_train, head, train_tail
    # every family's signatures are on the handle before a call goes through it
    for m in (train_tail, head, conv_stage_train, conv):
        m.lib()
    return train_tail


@functools.lru_cache(maxsize=None)
def inputs(t, dtype, norm=HR.VALID, ignore_label=None, ignored=False, out_of_range=False):
    return R.conditioned_inputs(t, dtype, SEED, R.cfg(norm, ignore_label), ignored, out_of_range)


@functools.lru_cache(maxsize=None)
def model(t, pool, dtype, norm=HR.VALID, ignore_label=None, ignored=False, out_of_range=False):
    """The float64 model on the inputs as the device gets them; computed once and shared, read-only."""
    out = R.model_outputs(t, pool, inputs(t, dtype, norm, ignore_label, ignored, out_of_range), R.cfg(norm, ignore_label))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probe(t):
    return R.integer_probe(t, SEED)


class Garbage(GuardedWorkspace):
    """A workspace of exactly the queried size between guard zones, filled with NaN words or with random ones."""

    def __init__(self, nbytes, fill):
        super().__init__(nbytes)
        if fill == "random":
            self.buf[V.GUARD:V.GUARD + nbytes // 4].copy_(torch.randn(nbytes // 4, device="cuda") * 1e30)


def tail_shape(tail, t, pool):
    return tail.train_tail_shape(V.cshape(t.stage.conv), t.stage.pool, pool, t.F1, t.H, t.C)


def run(tail, t, pool, inp, dtype=np.float32, route="auto", shift=0, ws_fill=None, label=True, loss=True, backward=True,
        outputs=(True,) * 10, memory=R.BN_MEMORY, norm=HR.VALID, ignore_label=None):
    """Forward, then backward on top of the initial parameter diffs.  Every output starts as NaN (scale_diff and
    shift_diff as 123, the accumulated diffs as the inputs' diffs) between guard zones, `shift` elements off a 16-byte
    boundary; ws_fill: a guarded workspace of exactly the queried size, "nan" or "random".  -> every output on the host;
    an output not asked for is absent and its prefill is checked to be intact."""
    s, sfx = t.stage.conv, "" if dtype == np.float32 else "_f64"
    fwd, bwd = getattr(tail, "train_tail_forward" + sfx), getattr(tail, "train_tail_backward" + sfx)
    query = getattr(tail, "train_tail_workspace_bytes" + sfx)
    kw = dict(stride=s.stride, pad=s.pad, group=s.group, normalization=norm, ignore_label=ignore_label)
    dev = {k: (None if inp[k] is None else V.placed(inp[k], dtype, shift)) for k in INPUTS}
    buf = torch.empty(inp["mask"].size + shift, dtype=torch.int32, device="cuda")
    mask = buf[shift:].view(*inp["mask"].shape)         # int32, `shift` elements off a 16-byte boundary
    mask.copy_(torch.from_numpy(np.array(inp["mask"])))
    N, K, nan = s.N, s.K, float("nan")
    OH, OW = R.S.CR.output_dims(s)
    G = lambda shape, fill: V.Guarded(shape, dtype, fill, shift)                     # noqa: E731
    g = dict(y=G((N, K, OH, OW), nan), flt=G((N, K), nan), save_pool=G((N, K), nan), save_mean=G((K,), nan),
             save_std=G((K,), nan), running_mean=G((K,), np.asarray(inp["running_mean"])),
             running_var=G((K,), np.asarray(inp["running_var"])), h=G((N, t.H), nan), prob=G((N, t.C), nan),
             loss=G((1,), 77.0))
    shape = tail_shape(tail, t, pool)
    workspace = lambda r: None if ws_fill is None else Garbage(query(shape, route=r), ws_fill)     # noqa: E731
    ws = workspace(route)
    saved = fwd(dev["x"], dev["weight"], dev["bias"], t.stage.pool, pool, dev["scale"], dev["shift"],
                g["running_mean"].t, g["running_var"].t, dev["overlap"], dev["w1"], dev["b1"], mask, dev["w2"], dev["b2"],
                dev["label"] if label else None, g["y"].t, g["flt"].t, g["save_pool"].t, g["save_mean"].t,
                g["save_std"].t, g["h"].t, g["prob"].t, g["loss"].t if label and loss else None, bn_memory=memory, ws=ws,
                route=route, **kw)
    torch.cuda.synchronize()
    assert saved.prob is g["prob"].t and (saved.loss is None) == (not label)
    if ws:
        ws.check()
    out = {k: v.host(k) for k, v in g.items()}
    if not (label and loss):
        assert (out.pop("loss") == 77.0).all(), "loss was not asked for"
        if label:                                       # the binding allocated one: the call wrote it there
            assert torch.isfinite(saved.loss).all()
    if backward:
        b = dict(bottom_diff=G(inp["x"].shape, nan), weight_diff=G(inp["weight"].shape, np.asarray(inp["weight_diff0"])),
                 scale_diff=G((K,), 123.0), shift_diff=G((K,), 123.0), w1_diff=G(inp["w1"].shape, np.asarray(inp["w1_diff0"])),
                 b1_diff=G((t.H,), np.asarray(inp["b1_diff0"])), w2_diff=G(inp["w2"].shape, np.asarray(inp["w2_diff0"])),
                 b2_diff=G((t.C,), np.asarray(inp["b2_diff0"])))
        if inp["bias_diff0"] is not None:
            b["bias_diff"] = G((K,), np.asarray(inp["bias_diff0"]))
        if t.F1:
            b["overlap_diff"] = G((N, t.F1), nan)
        given = {k: (b[k].t if k in b and want else None) for k, want in zip(R.BACKWARD_OUTPUTS, outputs)}
        ws = workspace("auto")
        bwd(dev["x"], dev["weight"], t.stage.pool, pool, g["y"].t, g["flt"].t, g["save_pool"].t, dev["scale"],
            dev["shift"], g["save_mean"].t, g["save_std"].t, dev["overlap"], dev["w1"], dev["w2"], mask, g["h"].t,
            g["prob"].t, dev["label"], inp["loss_weight"], ws=ws, **given, **kw)
        torch.cuda.synchronize()
        if ws:
            ws.check()
        for k, v in b.items():
            hv = v.host(k)
            if given[k] is not None:
                out[k] = hv
            elif k in ("bottom_diff", "overlap_diff"):
                assert np.isnan(hv).all(), k + " was not asked for"
            elif k in ("scale_diff", "shift_diff"):
                assert (hv == 123.0).all(), k + " was not asked for"
            else:
                V.assert_words_equal(hv, np.array(inp[k + "0"], dtype=dtype), k + " was not asked for")
    for k in INPUTS:
        if inp[k] is not None:
            V.assert_words_equal(V.host(dev[k]), np.array(inp[k], dtype=dtype), k + " is an input")
    return out


def routes_of(t, dtype=np.float32):
    if dtype != np.float32:
        return ("auto",)
    return ("auto", "sequence", "fused") if t in R.FUSED_TAILS else ("auto", "sequence")


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", R.GPU_TAILS, ids=R.tail_id)
def test_parity(tail, t, pool):
    """The main call, the forced sequence and the forced fused launches in float, and the double call: every output of
    both passes against the float64 model at the project's bars."""
    from mms_answer_selection_amd import capi
    if t in R.SEQUENCE_TAILS:
        assert tail.train_tail_route(tail_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE
        with pytest.raises(capi.MMSError, match=r"code 2\b"):
            run(tail, t, pool, inputs(t, np.float32), route="fused")
    for dtype in (np.float32, np.float64):
        for route in routes_of(t, dtype):
            print(R.tail_id(t), R.POOL_NAME[pool], dtype.__name__, route)
            check_parity(run(tail, t, pool, inputs(t, dtype), dtype, route), model(t, pool, dtype), dtype)


PROBES = [R.small(R.IMAGES + 1), R.small(65), R.v4(7), R.v5(5)]


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", PROBES, ids=R.tail_id)
def test_exact_probe_fused_equals_sequence(tail, t, pool):
    """Integer y, exact partial sums, one label that counts: the two routes give the same words in every forward
    output, the statistics are the float32 restatement from the int64 sums, and the main call gives the words of the
    route mms_train_tail_route names."""
    inp = probe(t)
    y, s0, s1 = R.S.probe_sums(t.stage, {k: (None if inp[k] is None else np.rint(inp[k]).astype(np.int64))
                                         for k in ("x", "weight", "bias")})
    fused = run(tail, t, pool, inp, route="fused", memory=R.PROBE_MEMORY, backward=False)
    seq = run(tail, t, pool, inp, route="sequence", memory=R.PROBE_MEMORY, backward=False)
    auto = run(tail, t, pool, inp, memory=R.PROBE_MEMORY, backward=False)
    assert sorted(fused) == sorted(R.FORWARD_OUTPUTS)
    for k, v in fused.items():
        assert not np.isnan(v).any(), k
    same_words(fused, seq, "exact probe, fused against sequence")
    named = {tail.ROUTE_FUSED: fused, tail.ROUTE_SEQUENCE: seq}[tail.train_tail_route(tail_shape(tail, t, pool))]
    same_words(auto, named, "exact probe, the main call against the route it names")
    V.assert_words_equal(fused["y"], y.astype(np.float32), "y against the int64 model")
    for k, want in zip(STATISTICS, R.S.probe_statistics(t.stage, inp, s0, s1)):
        V.assert_words_equal(fused[k], want, k + " against the int64 sums")


@pytest.mark.parametrize("t", [R.small(R.IMAGES + 1), R.small(257), R.v4(50), R.v5(50)], ids=R.tail_id)
def test_y_is_the_convolutions_own_words(tail, t):
    from mms_answer_selection_amd import conv
    s, inp = t.stage.conv, inputs(t, np.float32)
    dev = {k: (None if inp[k] is None else V.placed(inp[k], np.float32)) for k in ("x", "weight", "bias")}
    want = V.host(conv.conv_forward(dev["x"], dev["weight"], dev["bias"], stride=s.stride, pad=s.pad, group=s.group))
    for pool in R.POOLS:
        for route in routes_of(t):
            got = run(tail, t, pool, inp, route=route, backward=False)["y"]
            V.assert_words_equal(got, want, "y, %s, %s route" % (R.POOL_NAME[pool], route))


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", [R.small(65), R.v4(50)], ids=R.tail_id)
def test_both_passes_are_the_public_calls(tail, t, pool):
    """The forced sequence forward, the main call where it takes the sequence, and the backward against
    mms_conv_stage_train_forward_f32, mms_head_forward_f32, mms_head_backward_f32 and mms_conv_stage_train_backward_f32
    issued here, word for word."""
    from mms_answer_selection_amd import conv_stage_train, head
    s, inp, m = t.stage.conv, inputs(t, np.float32), R.METHOD[pool]
    got = run(tail, t, pool, inp, route="sequence")
    if tail.train_tail_route(tail_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE:
        same_words(run(tail, t, pool, inp), got, "the main call against the forced sequence")
    dev = {k: (None if inp[k] is None else V.placed(np.asarray(inp[k]), np.float32)) for k in inp
           if isinstance(inp[k], np.ndarray) and k != "mask"}
    dev.update(bias=dev.get("bias"), bias_diff0=dev.get("bias_diff0"), overlap=dev.get("overlap"))
    mask = torch.from_numpy(np.array(inp["mask"])).cuda()
    rm, rv = dev["running_mean"].clone(), dev["running_var"].clone()
    sv = conv_stage_train.conv_stage_train_forward(dev["x"], dev["weight"], dev["bias"], t.stage.pool, m, dev["scale"],
                                                   dev["shift"], rm, rv, bn_memory=R.BN_MEMORY)
    flt = sv.top.view(s.N, s.K)
    h, prob, loss = head.head_forward(flt, dev["overlap"], dev["w1"], dev["b1"], mask, dev["w2"], dev["b2"], dev["label"])
    x0d = torch.empty_like(flt)
    x1d = torch.empty_like(dev["overlap"]) if t.F1 else None
    w1d, b1d, w2d, b2d = (dev[k + "_diff0"].clone() for k in ("w1", "b1", "w2", "b2"))
    head.head_backward(flt, dev["overlap"], dev["w1"], dev["w2"], mask, h, prob, dev["label"], inp["loss_weight"], x0d, x1d,
                       w1d, b1d, w2d, b2d)
    dx, dw, db = torch.empty_like(dev["x"]), dev["weight_diff0"].clone(), dev["bias_diff0"].clone()
    dsc, dsh = torch.empty(s.K, device="cuda"), torch.empty(s.K, device="cuda")
    conv_stage_train.conv_stage_train_backward(dev["x"], dev["weight"], t.stage.pool, m, sv.y, sv.top, x0d.view_as(sv.top),
                                               sv.save_pool, dev["scale"], dev["shift"], sv.save_mean, sv.save_std, dx, dw,
                                               db, dsc, dsh)
    torch.cuda.synchronize()
    want = dict(y=sv.y, flt=flt, save_pool=sv.save_pool.view(s.N, s.K), save_mean=sv.save_mean, save_std=sv.save_std,
                running_mean=rm, running_var=rv, h=h, prob=prob, loss=loss, bottom_diff=dx, weight_diff=dw, bias_diff=db,
                scale_diff=dsc, shift_diff=dsh, w1_diff=w1d, b1_diff=b1d, w2_diff=w2d, b2_diff=b2d)
    if t.F1:
        want["overlap_diff"] = x1d
    same_words(got, {k: V.host(v) for k, v in want.items()}, "the sequence route against the public calls")


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", [R.small(R.IMAGES + 1), R.small(65), R.v4(50), R.STRIDED], ids=R.tail_id)
def test_determinism_and_independence(tail, t, pool):
    """A second run, a workspace of exactly the queried size full of NaN words and one full of random ones, every array
    one element (4 bytes in float) off a 16-byte boundary: the same words on every route."""
    inp = inputs(t, np.float32)
    for dtype in (np.float32, np.float64):
        for route in routes_of(t, dtype):
            i = inputs(t, dtype)
            first = run(tail, t, pool, i, dtype, route)
            same_words(run(tail, t, pool, i, dtype, route), first, "second run, " + route)
            same_words(run(tail, t, pool, i, dtype, route, shift=1, ws_fill="nan"), first, "NaN workspace, " + route)
            same_words(run(tail, t, pool, i, dtype, route, shift=1, ws_fill="random"), first, "random workspace, " + route)
    assert inp is inputs(t, np.float32)


@pytest.mark.parametrize("route", ["fused", "sequence"])
@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", [R.small(R.IMAGES + 1), R.small(65)], ids=R.tail_id)
def test_optional_outputs(tail, t, pool, route):
    """loss NULL, label and loss both absent: every other forward word unchanged and the loss untouched (run checks its
    sentinel).  Each backward output alone and all but it: the others' words unchanged, its own prefill intact; with no
    output the call is refused.  The running blobs are required, as the stage call requires them."""
    from mms_answer_selection_amd import capi
    inp = inputs(t, np.float32)
    full = run(tail, t, pool, inp, route=route)
    for kw in (dict(loss=False), dict(label=False)):
        part = run(tail, t, pool, inp, route=route, backward=False, **kw)
        assert sorted(part) == sorted(set(R.FORWARD_OUTPUTS) - {"loss"})
        for k, v in part.items():
            V.assert_words_equal(v, full[k], "%s with %s" % (k, kw))
    if route == "sequence":
        return                                          # the backward has one route
    masks = [1 << b for b in range(10)] + [1023 ^ (1 << b) for b in range(10)] + [0b0000011111, 0b1111100000]
    for mask in masks:
        outputs = tuple(bool(mask >> b & 1) for b in range(10))
        part = run(tail, t, pool, inp, route=route, outputs=outputs)
        assert len(part) == len(full) - outputs.count(False)
        for k, v in part.items():
            V.assert_words_equal(v, full[k], "%s with outputs %s" % (k, outputs))
    with pytest.raises(capi.MMSError):
        run(tail, t, pool, inp, route=route, outputs=(False,) * 10)
    s = t.stage.conv
    k = torch.ones(s.K, device="cuda")
    with pytest.raises(capi.MMSError):                  # the binding itself asks for the running blobs
        tail.train_tail_forward(torch.zeros(s.N, s.C, s.H, s.W, device="cuda"), torch.zeros(s.K, s.C, s.kh, s.kw, device="cuda"),
                                None, t.stage.pool, pool, k, k.clone(), None, None, torch.zeros(s.N, t.F1, device="cuda"),
                                torch.zeros(t.H, s.K + t.F1, device="cuda"), None,
                                torch.zeros(s.N, t.H, dtype=torch.int32, device="cuda"), torch.zeros(t.C, t.H, device="cuda"),
                                None, route=route)


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_several_finish_workgroups_write_the_statistics_once(tail, pool):
    """N = 257 is five workgroups in the second launch: save_mean, save_std and the running blobs are the sequence's to
    the bar -- a second update of the running blobs would be far off it -- and the same on a second run."""
    t = R.small(257)
    inp = inputs(t, np.float32)
    fused = run(tail, t, pool, inp, route="fused", backward=False)
    seq = run(tail, t, pool, inp, route="sequence", backward=False)
    want = model(t, pool, np.float32)
    for k in STATISTICS:
        assert_close(fused[k], seq[k], BAR[np.float32], k + ", fused against sequence")
        assert_close(fused[k], want[k], BAR[np.float32], k)
    once = (1 - R.BN_MEMORY) * want["save_mean"] + R.BN_MEMORY * np.asarray(inp["running_mean"], np.float64)
    twice = (1 - R.BN_MEMORY) * want["save_mean"] + R.BN_MEMORY * once
    assert np.abs(twice - once).max() > 1e3 * BAR[np.float32]
    assert_close(fused["running_mean"], once, BAR[np.float32], "running_mean, updated once")
    same_words(run(tail, t, pool, inp, route="fused", backward=False), fused, "second run")


@pytest.mark.parametrize("norm", [HR.FULL, HR.VALID, HR.BATCH_SIZE, HR.NONE])
def test_loss_under_every_normalization(tail, norm):
    """With ignored and out-of-range labels, in the second launch (N = 5) and by the one-thread launch (N = 65)."""
    for t in (R.small(5), R.small(65)):
        kw = dict(norm=norm, ignore_label=1)
        inp = inputs(t, np.float32, norm, 1, True, True)
        want = model(t, R.AVE, np.float32, norm, 1, True, True)
        for route in ("auto", "sequence", "fused"):
            got = run(tail, t, R.AVE, inp, route=route, **kw)
            for k in ("loss", "w2_diff", "bottom_diff"):
                assert_close(got[k], want[k], BAR[np.float32], "%s, %s" % (k, route))
        i64 = inputs(t, np.float64, norm, 1, True, True)
        assert_close(run(tail, t, R.AVE, i64, np.float64, **kw)["loss"], model(t, R.AVE, np.float64, norm, 1, True, True)["loss"],
                     BAR[np.float64], "loss f64")


def test_route_and_the_plans_refusal(tail):
    """H = 65 is past the head's fast limit: the route is the sequence and the forced fused call says
    MMS_ERR_UNSUPPORTED; every FUSED answer of the route call is a shape the fused launches reach."""
    from mms_answer_selection_amd import capi
    for pool in R.POOLS:
        assert R.PAST_H.H == 65
        assert tail.train_tail_route(tail_shape(tail, R.PAST_H, pool)) == tail.ROUTE_SEQUENCE
        assert tail.train_tail_workspace_bytes(tail_shape(tail, R.PAST_H, pool), "fused") == 0
        with pytest.raises(capi.MMSError, match=r"code 2\b"):
            run(tail, R.PAST_H, pool, inputs(R.PAST_H, np.float32), route="fused", backward=False)
        for t in R.GPU_TAILS:
            if tail.train_tail_route(tail_shape(tail, t, pool)) == tail.ROUTE_FUSED:
                assert tail.train_tail_workspace_bytes(tail_shape(tail, t, pool), "fused") > 0, t


def test_empty_batch_writes_nothing(tail):
    k = [V.Guarded((5,), np.float32, 1.5) for _ in range(4)]
    w = V.Guarded((5, 3, 3, 3), np.float32, 1.0)
    x = torch.empty(0, 3, 6, 6, device="cuda")
    for route in ("auto", "sequence", "fused"):
        saved = tail.train_tail_forward(x, w.t, None, 4, R.AVE, *(g.t for g in k), torch.empty(0, 3, device="cuda"),
                                        torch.zeros(5, 8, device="cuda"), None, torch.empty(0, 5, dtype=torch.int32, device="cuda"),
                                        torch.zeros(2, 5, device="cuda"), None, route=route)
        assert tuple(saved.y.shape) == (0, 5, 4, 4) and tuple(saved.prob.shape) == (0, 2)
    torch.cuda.synchronize()
    assert (w.host("weight") == 1.0).all()
    for g in k:
        assert (g.host("a BN array") == 1.5).all()
