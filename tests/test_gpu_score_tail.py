"""GPU suite of the scoring tail (include/mms_score_tail.h): every entry point against the float64 model
(tests/score_tail_reference.py) with AVE and MAX pooling, both sides of each fast limit of the head, the route table,
word equality of the fused launch, the sequence and the two public calls issued here, independence of alignment, of the
workspace's contents and of which optional outputs are asked for, the loss under the four normalizations, and prob into
the ranking call.

Bars: 1e-5 (util.TOL, the project's fp32 bar) in float and 1e-12 in double, against the float64 model, scale-aware
(util.assert_close).  Word equality is equality of every bit.
"""
import functools

import numpy as np
import pytest
import torch

import head_reference as HR
import score_tail_reference as R
from util import SEED, TOL, assert_bitexact, assert_close

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
POOL_IDS = lambda p: R.POOL_NAME[p]
WORDS = ("flt", "h", "prob")


@pytest.fixture(scope="module")
def tail(hiplib):
    from mms_answer_selection_amd import conv_maxpool_stage, conv_stage, head, score_tail
    # Every family's signatures are on the handle before a call goes through it: head_forward without a label asks for
    # no workspace and so would not apply its own, and an unbound call passes addresses as C ints.
    for m in (score_tail, head, conv_stage, conv_maxpool_stage):
        m.lib()
    return score_tail


@functools.lru_cache(maxsize=None)
def case(t, pool, norm=HR.VALID, ignore_label=None, ignored=False, out_of_range=False):
    """(config, float64 inputs, the model's outputs): computed once and shared, read-only."""
    config = R.cfg(norm, ignore_label)
    inp = R.conditioned_inputs(t, pool, np.float64, SEED, config, ignored, out_of_range)
    # the float calls see the inputs rounded to float; the model is taken from those
    inp32 = {k: (None if v is None else v.astype(np.float32)) for k, v in inp.items()}
    out64 = R.forward(t, pool, inp, config)
    out32 = R.forward(t, pool, {k: (None if v is None else v.astype(np.float64)) for k, v in inp32.items()}, config)
    for d in (inp, inp32, out64, out32):
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
    return config, {np.float64: inp, np.float32: inp32}, {np.float64: out64, np.float32: out32}


def dev(a, off=False):
    """A device copy; off: its first element one element past a 16-byte boundary."""
    if a is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return src.cuda()
    buf = torch.empty(a.size + 8, dtype=src.dtype, device="cuda")
    view = buf[1:1 + a.size].view(a.shape)
    assert view.data_ptr() % 16 == a.itemsize
    view.copy_(src)
    return view


class OffsetNaNWorkspace:
    """capi.Workspace's interface: scratch filled with NaN words whose start is one element past a 16-byte boundary."""

    def __init__(self, itemsize):
        self.buf, self.off = None, itemsize

    def get(self, nbytes, device):
        self.buf = torch.full((int(nbytes) // 4 + 8,), float("nan"), dtype=torch.float32, device=device)
        return self.buf.data_ptr() + self.off, self.buf.numel() * 4 - self.off


def run(tail, t, pool, dtype, route="auto", want=WORDS, label=True, norm=HR.VALID, ignore_label=None, ignored=False,
        out_of_range=False, off=False):
    """-> {name: numpy} of the outputs asked for (`want` of flt / h, prob always, loss with a label)."""
    config, inps, _ = case(t, pool, norm, ignore_label, ignored, out_of_range)
    inp, s = inps[dtype], t.stage.conv
    d = {k: dev(v, off) for k, v in inp.items()}
    td = torch.float32 if dtype == np.float32 else torch.float64
    N = s.N
    outs = dict(flt=dev(np.full((N, R.F0(t)), np.nan, dtype), off) if "flt" in want else None,
                h=dev(np.full((N, t.H), np.nan, dtype), off) if "h" in want else None,
                prob=dev(np.full((N, t.C), np.nan, dtype), off),
                loss=dev(np.full((1,), np.nan, dtype), off) if label else None)
    f = tail.score_tail_forward if dtype == np.float32 else tail.score_tail_forward_f64
    prob, loss = f(d["x"], d["weight"], d["bias"], t.stage.pool, pool, d["mean"], d["var"], d["scale"], d["shift"],
                   d["overlap"], d["w1"], d["b1"], d["w2"], d["b2"], d["label"] if label else None, outs["flt"],
                   outs["h"], outs["prob"], outs["loss"], stride=s.stride, pad=s.pad, group=s.group, normalization=norm,
                   ignore_label=ignore_label, ws=OffsetNaNWorkspace(np.dtype(dtype).itemsize) if off else None, route=route)
    assert prob is outs["prob"] and loss is outs["loss"] and prob.dtype == td
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items() if v is not None}


def tail_shape(tail, t, pool):
    from mms_answer_selection_amd import conv
    s = t.stage.conv
    return tail.score_tail_shape(conv.conv_shape(s.N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group),
                                 t.stage.pool, pool, t.F1, t.H, t.C)


def check_model(got, t, pool, dtype, what, **kw):
    _, _, outs = case(t, pool, **kw)
    tol = TOL if dtype == np.float32 else F64_TOL
    for k, v in got.items():
        assert_close(v, outs[dtype][k], tol, "%s %s" % (what, k))


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", R.FUSED_TAILS, ids=R.tail_id)
def test_where_the_fused_launch_reaches(tail, t, pool):
    """Every entry point against the model; the route table says FUSED from 17 workgroups on; the fused launch, the
    sequence and the two public calls issued here give the same words of flt, h and prob."""
    from mms_answer_selection_amd import conv_maxpool_stage, conv_stage, head
    want = tail.ROUTE_FUSED if t in R.MAIN_FUSED else tail.ROUTE_SEQUENCE      # FORCED_ONLY: too few workgroups
    assert tail.score_tail_route(tail_shape(tail, t, pool)) == want
    got = {r: run(tail, t, pool, np.float32, r) for r in ("auto", "sequence", "fused")}
    for r, g in got.items():
        check_model(g, t, pool, np.float32, r)
    check_model(run(tail, t, pool, np.float64), t, pool, np.float64, "f64")
    check_model(run(tail, t, pool, np.float64, "sequence"), t, pool, np.float64, "f64 sequence")
    _, inps, _ = case(t, pool)
    d, s = {k: dev(v) for k, v in inps[np.float32].items()}, t.stage.conv
    stage = conv_maxpool_stage.conv_maxpool_stage_forward if pool == R.MAX else conv_stage.conv_stage_forward
    top = stage(d["x"], d["weight"], d["bias"], t.stage.pool, d["mean"], d["var"], d["scale"], d["shift"])
    flt = top.view(s.N, -1)
    h, prob, _ = head.head_forward(flt, d["overlap"], d["w1"], d["b1"], None, d["w2"], d["b2"], phase=head.TEST)
    torch.cuda.synchronize()
    public = dict(flt=flt.cpu().numpy(), h=h.cpu().numpy(), prob=prob.cpu().numpy())
    for k in WORDS:
        assert_bitexact(got["fused"][k], got["sequence"][k], "fused / sequence " + k)
        assert_bitexact(got["auto"][k], got["sequence"][k], "auto / sequence " + k)
        assert_bitexact(got["sequence"][k], public[k], "sequence / the two public calls " + k)


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", R.SEQUENCE_TAILS, ids=R.tail_id)
def test_where_it_does_not_reach(tail, t, pool):
    """Just past each fast limit, a pooled map larger than 1 x 1, a strided convolution: the route table says SEQUENCE,
    the forced fused call is MMS_ERR_UNSUPPORTED, every other entry point is right."""
    from mms_answer_selection_amd import capi
    assert tail.score_tail_route(tail_shape(tail, t, pool)) == tail.ROUTE_SEQUENCE
    with pytest.raises(capi.MMSError, match=r"code 2\b"):
        run(tail, t, pool, np.float32, "fused")
    for r in ("auto", "sequence"):
        check_model(run(tail, t, pool, np.float32, r), t, pool, np.float32, r)
    check_model(run(tail, t, pool, np.float64), t, pool, np.float64, "f64")


ALIGNED = [R.MINIMAL[3], R.v4(23), R.v5(7)]


@pytest.mark.parametrize("route", ["fused", "sequence"])
@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", ALIGNED, ids=R.tail_id)
def test_alignment_and_the_workspace_change_no_word(tail, t, pool, route):
    """A second run with a NaN-filled workspace and every array one element off a 16-byte boundary: the same words,
    the loss included (its order is fixed too)."""
    a, b = run(tail, t, pool, np.float32, route), run(tail, t, pool, np.float32, route, off=True)
    for k in WORDS + ("loss",):
        assert_bitexact(a[k], b[k], k)
    c = run(tail, t, pool, np.float64, off=True)
    check_model(c, t, pool, np.float64, "f64, off a boundary")


@pytest.mark.parametrize("route", ["fused", "sequence"])
@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_optional_outputs_change_no_word(tail, pool, route):
    t = R.v4(23)
    full = run(tail, t, pool, np.float32, route)
    for want, label in (((), False), (("flt",), False), (("h",), True), ((), True), (("flt", "h"), False)):
        got = run(tail, t, pool, np.float32, route, want=want, label=label)
        assert sorted(got) == sorted(want + ("prob",) + (("loss",) if label else ()))
        for k, v in got.items():
            assert_bitexact(v, full[k], "%s with %s" % (k, want))


@pytest.mark.parametrize("norm", [HR.FULL, HR.VALID, HR.BATCH_SIZE, HR.NONE])
@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_loss(tail, pool, norm):
    """With ignored and out-of-range labels, on every entry point; v4's tail on eight workgroups and the minimal one."""
    for t in (R.v4(23), R.MINIMAL[3]):
        kw = dict(norm=norm, ignore_label=1, ignored=True, out_of_range=True)
        _, inps, outs = case(t, pool, **kw)
        lv, ok = HR.valid_of(inps[np.float64]["label"], t.C, R.cfg(norm, 1))
        assert t.stage.conv.N < 23 or (0 < ok.sum() < ok.size)
        for r in ("auto", "sequence", "fused"):
            got = run(tail, t, pool, np.float32, r, **kw)
            assert_close(got["loss"], outs[np.float32]["loss"], TOL, "loss " + r)
        assert_close(run(tail, t, pool, np.float64, **kw)["loss"], outs[np.float64]["loss"], F64_TOL, "loss f64")


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_prob_goes_straight_to_the_ranking_call(tail, pool):
    """prob (N, 2) of the tail into mms_rank_map_mrr_f32 (which ranks by column 1) with three groups: the MAP, MRR and
    effective groups of the model's prob."""
    from mms_answer_selection_amd import capi
    t = R.v4(21)
    _, inps, outs = case(t, pool)
    label = dev(inps[np.float32]["label"])
    group = dev(np.repeat(np.arange(3), 7).astype(np.float32))
    assert 0 < inps[np.float32]["label"].sum() < 21
    want = capi.rank_map_mrr(dev(outs[np.float32]["prob"].astype(np.float32)), label, group)
    for r in ("fused", "sequence"):
        prob = dev(run(tail, t, pool, np.float32, r)["prob"])
        assert capi.rank_map_mrr(prob, label, group) == want, r
