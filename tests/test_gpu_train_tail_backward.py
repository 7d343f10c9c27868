"""GPU suite of the tail's routed and fused backward (include/mms_train_tail_backward.h): the forced fused launches and
the routed call against the float64 model (tests/train_tail_reference.py) and against mms_train_tail_backward_f32, the
head's outputs against mms_head_backward_f32's words, an exact probe on which the fused route, the sequence and the
model agree to the word, MAX ties and rounding collapse, optional outputs on top of prefills, determinism under garbage
workspaces and shifted bases, and the route table.

Bar: 1e-5 (util.TOL) against the float64 model, scale-aware (util.assert_close).  Word equality is equality of every bit.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_conv as V
import train_tail_backward_cases as B
import train_tail_reference as R
from layer_plans import constants
from pooled_stage_suite import GuardedWorkspace, check_parity, same_words
from util import SEED

pytestmark = pytest.mark.gpu

POOL_IDS = lambda p: R.POOL_NAME[p]                                                 # noqa: E731
INPUTS = ("x", "weight", "scale", "shift", "overlap", "w1", "w2", "label")
SAVED = ("y", "flt", "save_pool", "save_mean", "save_std", "h", "prob")


@pytest.fixture(scope="module")
def mods(hiplib):
    from mms_answer_selection_amd import conv, conv_stage_train, head, train_tail, train_tail_backward
    for m in (train_tail_backward, train_tail, head, conv_stage_train, conv):
        m.lib()
    return train_tail, train_tail_backward, head


@functools.lru_cache(maxsize=None)
def inputs(t):
    return R.conditioned_inputs(t, np.float32, SEED)


def tail_shape(tail, t, pool):
    return tail.train_tail_shape(V.cshape(t.stage.conv), t.stage.pool, pool, t.F1, t.H, t.C)


_forwards = {}


def forward(mods, t, pool):
    """What the device's own forward (the sequence route) leaves for the backward, on the host; once per (t, pool)."""
    if (t, pool) not in _forwards:
        tail, inp, s = mods[0], inputs(t), t.stage.conv
        dev = {k: (None if inp[k] is None else V.placed(inp[k], np.float32)) for k in
               ("x", "weight", "bias", "scale", "shift", "running_mean", "running_var", "overlap", "w1", "b1", "w2", "b2",
                "label")}
        mask = torch.from_numpy(np.array(inp["mask"])).cuda()
        sv = tail.train_tail_forward(dev["x"], dev["weight"], dev["bias"], t.stage.pool, pool, dev["scale"], dev["shift"],
                                     dev["running_mean"], dev["running_var"], dev["overlap"], dev["w1"], dev["b1"], mask,
                                     dev["w2"], dev["b2"], dev["label"], stride=s.stride, pad=s.pad, group=s.group,
                                     route="sequence")
        torch.cuda.synchronize()
        _forwards[(t, pool)] = {k: V.host(getattr(sv, k)) for k in SAVED}
    return _forwards[(t, pool)]


@functools.lru_cache(maxsize=None)
def model(t, pool):
    out = R.model_outputs(t, pool, inputs(t))
    return {k: out[k] for k in R.BACKWARD_OUTPUTS if k in out}


def backward(mods, kind, t, pool, inp, fwd, shift=0, ws_fill=None, outputs=(True,) * 10, ratio=0.5):
    """One backward call of `kind` on inputs placed `shift` elements off a 16-byte boundary.  Overwritten outputs start
    as NaN (scale_diff, shift_diff as 123), accumulated ones as the inputs' diffs, all between guard zones; ws_fill: a
    guarded workspace of exactly the queried size, every word NaN.  -> the outputs asked for, on the host; the prefill
    of every other is checked to be intact, and so are the inputs."""
    tail, tb, _ = mods
    s = t.stage.conv
    N, K, nan = s.N, s.K, float("nan")
    dev = {k: (None if inp[k] is None else V.placed(np.asarray(inp[k]), np.float32, shift)) for k in INPUTS}
    dev.update({k: V.placed(fwd[k], np.float32, shift) for k in SAVED})
    buf = torch.empty(inp["mask"].size + shift, dtype=torch.int32, device="cuda")
    mask = buf[shift:].view(*inp["mask"].shape)
    mask.copy_(torch.from_numpy(np.array(inp["mask"])))
    G = lambda shape, fill: V.Guarded(shape, np.float32, fill, shift)                # noqa: E731
    b = dict(bottom_diff=G(inp["x"].shape, nan), weight_diff=G(inp["weight"].shape, np.asarray(inp["weight_diff0"])),
             scale_diff=G((K,), 123.0), shift_diff=G((K,), 123.0), w1_diff=G(inp["w1"].shape, np.asarray(inp["w1_diff0"])),
             b1_diff=G((t.H,), np.asarray(inp["b1_diff0"])), w2_diff=G(inp["w2"].shape, np.asarray(inp["w2_diff0"])),
             b2_diff=G((t.C,), np.asarray(inp["b2_diff0"])))
    if inp["bias_diff0"] is not None:
        b["bias_diff"] = G((K,), np.asarray(inp["bias_diff0"]))
    if t.F1:
        b["overlap_diff"] = G((N, t.F1), nan)
    given = {k: (b[k].t if k in b and want else None) for k, want in zip(R.BACKWARD_OUTPUTS, outputs)}
    shape = tail_shape(tail, t, pool)
    if kind == "sequence":
        call, nbytes = tail.train_tail_backward, tail.train_tail_workspace_bytes(shape)
        kw = {}
    else:
        route = "fused" if kind == "fused" else "auto"
        call, nbytes = tb.train_tail_backward_routed, tb.train_tail_backward_workspace_bytes(shape, route)
        kw = dict(route=route)
    ws = GuardedWorkspace(nbytes) if ws_fill else None
    from mms_answer_selection_amd import capi
    refusal = None
    try:
        call(dev["x"], dev["weight"], t.stage.pool, pool, dev["y"], dev["flt"], dev["save_pool"], dev["scale"],
             dev["shift"], dev["save_mean"], dev["save_std"], dev["overlap"], dev["w1"], dev["w2"], mask, dev["h"],
             dev["prob"], dev["label"], inp["loss_weight"], ws=ws, dropout_ratio=ratio, stride=s.stride, pad=s.pad,
             group=s.group, **given, **kw)
    except capi.MMSError as e:                          # a refused call: every output must hold its prefill
        refusal, given = e, {k: None for k in given}
    torch.cuda.synchronize()
    if ws and not refusal:
        ws.check()
    out = {}
    for k, v in b.items():
        hv = v.host(k)
        if given[k] is not None:
            out[k] = hv
        elif k in ("bottom_diff", "overlap_diff"):
            assert np.isnan(hv).all(), k + " was not asked for"
        elif k in ("scale_diff", "shift_diff"):
            assert (hv == 123.0).all(), k + " was not asked for"
        else:
            V.assert_words_equal(hv, np.array(inp[k + "0"], dtype=np.float32), k + " was not asked for")
    for k in INPUTS:
        if inp[k] is not None:
            V.assert_words_equal(V.host(dev[k]), np.array(inp[k], dtype=np.float32), k + " is an input")
    if refusal:
        raise refusal
    return out


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", B.PARITY_TAILS, ids=R.tail_id)
def test_parity(mods, t, pool):
    """Forced FUSED and the routed call against the float64 model, all ten outputs; FUSED against the sequence's words
    at the same bar; the five head outputs are mms_head_backward_f32's words."""
    inp, fwd, want = inputs(t), forward(mods, t, pool), model(t, pool)
    fused = backward(mods, "fused", t, pool, inp, fwd)
    for k, v in fused.items():
        assert not np.isnan(v).any(), k
    check_parity(fused, want, np.float32)
    check_parity(backward(mods, "routed", t, pool, inp, fwd), want, np.float32)
    seq = backward(mods, "sequence", t, pool, inp, fwd)
    check_parity(fused, {k: v.astype(np.float64) for k, v in seq.items()}, np.float32)
    for k in ("overlap_diff", "w1_diff", "b1_diff", "w2_diff", "b2_diff"):
        if k in seq:
            V.assert_words_equal(fused[k], seq[k], k + " against the head call's words")


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_head_outputs_are_the_head_calls_words(mods, pool):
    t = R.small(65)
    _, _, head = mods
    inp, fwd = inputs(t), forward(mods, t, pool)
    fused = backward(mods, "fused", t, pool, inp, fwd)
    d = lambda a: V.placed(np.asarray(a), np.float32)                               # noqa: E731
    x0d, x1d = torch.empty(t.stage.conv.N, t.stage.conv.K, device="cuda"), torch.empty(t.stage.conv.N, t.F1, device="cuda")
    acc = {k: d(inp[k + "_diff0"]) for k in ("w1", "b1", "w2", "b2")}
    head.head_backward(d(fwd["flt"]), d(inp["overlap"]), d(inp["w1"]), d(inp["w2"]), torch.from_numpy(np.array(inp["mask"])).cuda(),
                       d(fwd["h"]), d(fwd["prob"]), d(inp["label"]), inp["loss_weight"], x0d, x1d, acc["w1"], acc["b1"],
                       acc["w2"], acc["b2"])
    torch.cuda.synchronize()
    V.assert_words_equal(fused["overlap_diff"], V.host(x1d), "overlap_diff")
    for k, v in acc.items():
        V.assert_words_equal(fused[k + "_diff"], V.host(v), k + "_diff")


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_exact_probe(mods, pool):
    """Inputs given directly, every product and sum exact: FUSED, the sequence and the float64 model agree word for word
    on all ten outputs."""
    inp, fwd = B.exact_probe(pool)
    t = B.PROBE
    want = R.backward(t, pool, inp, {k: v.astype(np.float64) for k, v in fwd.items()}, B.probe_config())
    fused = backward(mods, "fused", t, pool, inp, fwd)
    seq = backward(mods, "sequence", t, pool, inp, fwd)
    assert sorted(fused) == sorted(R.BACKWARD_OUTPUTS)
    same_words(fused, seq, "exact probe, fused against sequence")
    same_words(fused, {k: v.astype(np.float32) for k, v in want.items()}, "exact probe, fused against the model")
    assert np.abs(fused["bottom_diff"]).max() > 0 and np.abs(fused["scale_diff"]).max() > 0


def tie_probe(kind):
    """The exact probe under MAX with y replaced: "ties" -- small integers, every window full of repeated extrema;
    "collapse" -- channel 0 (scale 1, std 2) under a shift of 1024: y = 0.5 and the next float after it have the same
    BN output, so the first maximum of BN's output is pixel 0 and arg-max y is pixel 1."""
    inp, fwd = B.exact_probe(R.MAX)
    inp, fwd = dict(inp), dict(fwd)
    y = np.array(fwd["y"])
    if kind == "ties":
        y = np.random.default_rng(11).integers(-1, 2, y.shape).astype(np.float32)
    else:
        y[:, 0] = -1.0
        y[:, 0, 0, 0] = 0.5
        y[:, 0, 0, 1] = np.nextafter(np.float32(0.5), np.float32(1))
        shift = np.array(inp["shift"])
        shift[0] = 1024.0
        inp["shift"] = shift
        bn = y[:, 0] / np.float32(2) * np.float32(1) + np.float32(1024)
        assert (bn[:, 0, 0] == bn[:, 0, 1]).all() and (y[:, 0, 0, 1] > y[:, 0, 0, 0]).all()
    fwd["y"] = y
    sp = B.pooled(R.MAX, y, inp["scale"], fwd["save_std"])
    if kind == "collapse":
        # channel 0's save_pool is given as the first maximum's, 0.5 / 2, not the scan's winner's, one ulp above it: a
        # dyadic value, so that scale_diff's sum is exact in any order.  Every other step of dy is a product of y with a
        # few-bit coefficient or a scaling by a power of two (std, N S), which round alike on both routes.
        sp[:, 0] = 0.25
    fwd["save_pool"] = sp
    return inp, fwd


@pytest.mark.parametrize("kind", ["ties", "collapse"])
def test_max_ties_and_rounding_collapse(mods, kind):
    """dz is nonzero at exactly the element the sequence picks: all ten outputs are the sequence's words on both
    probes, and the gradient's pixel is far from its neighbour's value, so a delta one pixel off cannot pass."""
    inp, fwd = tie_probe(kind)
    t = B.PROBE
    fused = backward(mods, "fused", t, R.MAX, inp, fwd)
    seq = backward(mods, "sequence", t, R.MAX, inp, fwd)
    same_words(fused, seq, kind + ", fused against sequence")
    want = R.backward(t, R.MAX, inp, {k: v.astype(np.float64) for k, v in fwd.items()}, B.probe_config())
    assert np.abs(want["bottom_diff"]).max() > 1e-3
    if kind == "ties":
        check_parity(fused, want, np.float32)
        return
    # In float64 the two BN outputs differ and the model's gradient is on pixel 1: the same-dtype model, whose BN output
    # collapses as the device's does, is the reference, and the two models are far apart.
    same = R.backward(t, R.MAX, inp, fwd, B.probe_config(), np.float32)
    check_parity(fused, {k: v.astype(np.float64) for k, v in same.items()}, np.float32)
    assert np.abs(same["bottom_diff"].astype(np.float64) - want["bottom_diff"]).max() > 1e-2


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_optional_outputs(mods, pool):
    """Each of the ten outputs alone and all but it: the others' words unchanged, its own prefill intact (backward
    checks it); accumulated outputs are on top of their nonzero prefill; no output at all is refused."""
    from mms_answer_selection_amd import capi
    t = R.small(3)
    inp, fwd = inputs(t), forward(mods, t, pool)
    full = backward(mods, "fused", t, pool, inp, fwd)
    for k in R.ACCUMULATED:
        assert np.abs(np.asarray(inp[k + "0"])).max() > 0
        assert np.abs(full[k] - np.asarray(inp[k + "0"], np.float32)).max() > 0
    masks = [1 << b for b in range(10)] + [1023 ^ (1 << b) for b in range(10)] + [0b0000011111, 0b1111100000]
    for mask in masks:
        outputs = tuple(bool(mask >> b & 1) for b in range(10))
        part = backward(mods, "fused", t, pool, inp, fwd, outputs=outputs)
        assert len(part) == outputs.count(True)
        for k, v in part.items():
            V.assert_words_equal(v, full[k], "%s with outputs %s" % (k, outputs))
    with pytest.raises(capi.MMSError):
        backward(mods, "fused", t, pool, inp, fwd, outputs=(False,) * 10)


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", [R.small(65), R.v5(3)], ids=R.tail_id)
def test_determinism_and_independence(mods, t, pool):
    inp, fwd = inputs(t), forward(mods, t, pool)
    first = backward(mods, "fused", t, pool, inp, fwd)
    same_words(backward(mods, "fused", t, pool, inp, fwd), first, "second run")
    same_words(backward(mods, "fused", t, pool, inp, fwd, ws_fill="nan"), first, "NaN workspace")
    same_words(backward(mods, "fused", t, pool, inp, fwd, shift=1, ws_fill="nan"), first, "4 bytes off, NaN workspace")


def test_route_table(mods):
    """mms_train_tail_backward_route is the table of csrc/train_tail_backward.hip: FUSED on the measured span of
    workgroup counts (one per kTrainTailBackwardImages images), the SEQUENCE at every other; past the head's fast limit
    and past 256 samples the forced call says MMS_ERR_UNSUPPORTED and its query 0."""
    from mms_answer_selection_amd import capi
    tail, tb, _ = mods
    c = constants("train_tail_backward.hip", ["kTrainTailBackwardImages"])
    images = c["kTrainTailBackwardImages"]
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "mms_answer_selection_amd", "csrc", "train_tail_backward.hip")).read()
    m = re.search(r"kTrainTailBackwardGroups\[2\] = \{\{(-?\d+), (-?\d+)\}, \{(-?\d+), (-?\d+)\}\};", src)
    spans = {R.AVE: (int(m.group(1)), int(m.group(2))), R.MAX: (int(m.group(3)), int(m.group(4)))}
    for pool in R.POOLS:
        lo, hi = spans[pool]
        counts = {1, 49, 50, 51, 99, 100, 101, 256} | {max(1, v) for v in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if hi >= lo}
        for groups in sorted(counts):
            for make in (R.v4, R.v5, R.small):
                N = min(groups * images, 256)
                want = tb.ROUTE_FUSED if lo <= -(-N // images) <= hi else tb.ROUTE_SEQUENCE
                assert tb.train_tail_backward_route(tail_shape(tail, make(N), pool)) == want, (make(N), pool)
        # an image of more than 128 pixels is reached (its rows fit one workgroup) and not measured: the sequence
        for N in (50, 100):
            shape = tail_shape(tail, B.large_image(N), pool)
            assert tb.train_tail_backward_route(shape) == tb.ROUTE_SEQUENCE, (N, pool)
            assert tb.train_tail_backward_workspace_bytes(shape, "fused") > 0
        for t in (R.PAST_H, B.PAST_N, R.STRIDED):
            shape = tail_shape(tail, t, pool)
            assert tb.train_tail_backward_route(shape) == tb.ROUTE_SEQUENCE
            assert tb.train_tail_backward_workspace_bytes(shape, "fused") == 0
            assert tb.train_tail_backward_workspace_bytes(shape) == tail.train_tail_workspace_bytes(shape)
        t = R.PAST_H
        with pytest.raises(capi.MMSError, match=r"code 2\b"):
            backward(mods, "fused", t, pool, inputs(t), forward(mods, t, pool))
        check_parity(backward(mods, "routed", t, pool, inputs(t), forward(mods, t, pool)), model(t, pool), np.float32)


def test_empty_batch_and_refused_calls_write_nothing(mods):
    from mms_answer_selection_amd import capi
    tail, tb, _ = mods
    w = V.Guarded((5, 3, 3, 3), np.float32, 1.0)
    z = lambda *s: torch.zeros(*s, device="cuda")                                    # noqa: E731
    for route in ("auto", "fused"):
        tb.train_tail_backward_routed(z(0, 3, 6, 6), z(5, 3, 3, 3), 4, R.AVE, z(0, 5, 4, 4), z(0, 5), z(0, 5), z(5), z(5),
                                      z(5), z(5), z(0, 3), z(5, 8), z(2, 5), torch.zeros(0, 5, dtype=torch.int32, device="cuda"),
                                      z(0, 5), z(0, 2), z(0), weight_diff=w.t, route=route)
    torch.cuda.synchronize()
    assert (w.host("weight_diff") == 1.0).all()
    t = R.small(3)
    inp, fwd = inputs(t), forward(mods, t, R.AVE)
    for kind in ("fused", "routed"):
        with pytest.raises(capi.MMSError):             # dropout_ratio 1 is the head's refusal: the prefills are checked
            backward(mods, kind, t, R.AVE, inp, fwd, ratio=1.0)
