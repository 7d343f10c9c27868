"""GPU suite: the classifier-head calls (include/mms_head.h, csrc/head.hip) against tests/head_reference.py, on the fast
route, the generic route in float, and in double.  The conditioned inputs (tests/test_head_reference.py shows them fit
for it) are held to the float64 model at the project's 1e-5 (float32) and 1e-12 (float64) in assert_close's metric;
indexing, the x0 | x1 seam, the mask, the accumulate / overwrite rule and NULL outputs are tested by EQUALITY on dyadic
probes of the backward, whatever order a kernel sums in; the fixed order and the workspace's irrelevance by equality of
words between two runs.  R.LARGE_SHAPES (more than 256 tiles: several slabs of several tiles each) go through all of it
and have three tests of their own at the end."""
import functools

import numpy as np
import pytest
import torch

import head_reference as R
from util import SEED, TOL, assert_close

pytestmark = pytest.mark.gpu

VARIANTS = [("fast", np.float32, "auto"), ("generic", np.float32, "generic"), ("f64", np.float64, "auto")]
VARIANT_IDS = [v[0] for v in VARIANTS]
BAR = {np.float32: TOL, np.float64: 1e-12}
TORCH = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32}
GUARD, SENTINEL = 64, -777.0
SHAPE_IDS = [R.sid(s) for s in R.GPU_SHAPES]
PARAM_DIFFS = ("w1_diff", "b1_diff", "w2_diff", "b2_diff")


def api(dtype):
    from mms_answer_selection_amd import head
    if dtype == np.float32:
        return head.head_forward, head.head_backward
    return head.head_forward_f64, head.head_backward_f64


def host(t):
    return t.detach().cpu().numpy()


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    w = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(got.reshape(-1).view(w) != want.reshape(-1).view(w))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


class Guarded:
    """An array between two zones of 64 sentinel elements, `shift` elements off its buffer's (16-byte aligned) start."""

    def __init__(self, shape, dtype, fill, shift=0):
        self.n = int(np.prod(shape))
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=TORCH[dtype], device="cuda")
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.array(fill, dtype=dtype)))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (shift * self.t.element_size()) % 16

    def host(self, what):
        b = host(self.buf)
        assert (b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all(), what + ": guard overwritten"
        return b[self.lo:self.lo + self.n].reshape(tuple(self.t.shape)).copy()


def placed(a, dtype, shift=0):
    """a on the device, `shift` elements off a 16-byte boundary; None stays None."""
    if a is None:
        return None
    buf = torch.empty(a.size + shift, dtype=TORCH[dtype], device="cuda")
    t = buf[shift:shift + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(np.array(a, dtype=dtype)))
    return t


def nan_workspace(s, dtype):
    """A Workspace of the size the calls ask for, every word a NaN."""
    from mms_answer_selection_amd import capi, head
    q = head.head_workspace_bytes if dtype == np.float32 else head.head_workspace_bytes_f64
    ws = capi.Workspace()
    ws.get(q(head.head_shape(*s)), torch.device("cuda", torch.cuda.current_device()))
    ws.buf.fill_(255)
    return ws


class ExactWorkspace:
    """In place of a capi.Workspace: exactly the bytes the call asks for, `shift` bytes off a 16-byte boundary, every
    byte of them `fill`, between two guard zones as long as one slab's partial sums."""

    def __init__(self, s, dtype, fill, shift):
        from mms_answer_selection_amd import head
        q = head.head_workspace_bytes if dtype == np.float32 else head.head_workspace_bytes_f64
        self.nbytes = q(head.head_shape(*s))
        assert self.nbytes == R.workspace_bytes(s, np.dtype(dtype).itemsize)
        self.lo = 16 * (-(-R.params(s) * np.dtype(dtype).itemsize // 16)) + shift
        self.buf = torch.full((self.lo + self.nbytes + self.lo,), 0x5A, dtype=torch.uint8, device="cuda")
        self.buf[self.lo:self.lo + self.nbytes] = fill
        assert self.buf.data_ptr() % 16 == 0 and (self.buf.data_ptr() + self.lo) % 16 == shift

    def get(self, nbytes, device):
        assert nbytes == self.nbytes, (nbytes, self.nbytes)
        return self.buf.data_ptr() + self.lo, self.nbytes

    def check(self, what):
        b = host(self.buf)
        assert (b[:self.lo] == 0x5A).all() and (b[self.lo + self.nbytes:] == 0x5A).all(), what + ": written past the workspace"


def kwargs(cfg, route, ws):
    return dict(phase=cfg.phase, dropout_ratio=cfg.ratio, normalization=cfg.norm, ignore_label=cfg.ignore_label, ws=ws,
                route=route)


def run_forward(s, cfg, inp, dtype, route, shift=0, ws=None, label=True):
    """-> {"h", "prob"[, "loss"]} on the host; the outputs start as NaN between guard zones."""
    fwd, _ = api(dtype)
    dev = {k: placed(inp[k], dtype, shift) for k in ("x0", "x1", "w1", "b1", "w2", "b2")}
    mask = placed(inp["mask"], np.int32, shift) if cfg.phase == R.TRAIN else None
    lab = placed(inp["label"], dtype, shift) if label else None
    nan = float("nan")
    h, prob = Guarded((s.N, s.H), dtype, nan, shift), Guarded((s.N, s.C), dtype, nan, shift)
    loss = Guarded((1,), dtype, nan, shift) if label else None
    got = fwd(dev["x0"], dev["x1"], dev["w1"], dev["b1"], mask, dev["w2"], dev["b2"], lab, h.t, prob.t,
              loss.t if label else None, **kwargs(cfg, route, ws))
    assert got[0] is h.t and got[1] is prob.t and (got[2] is loss.t if label else got[2] is None)
    out = dict(h=h.host("h"), prob=prob.host("prob"))
    if label:
        out["loss"] = loss.host("loss")
    for k, t in dev.items():
        if t is not None:
            assert_words_equal(host(t), np.array(inp[k], dtype=dtype), k + " is an input")
    return out


def run_backward(s, cfg, inp, h, prob, dtype, route, shift=0, ws=None, outputs=(True,) * 6):
    """-> the diffs asked for, on the host.  x*_diff start as NaN, the parameter diffs as inp[*_diff0], all between guard
    zones; an output not asked for is absent from the result and checked to be untouched."""
    _, bwd = api(dtype)
    dev = {k: placed(inp[k], dtype, shift) for k in ("x0", "x1", "w1", "w2", "label")}
    mask = placed(inp["mask"], np.int32, shift) if cfg.phase == R.TRAIN else None
    hd, pd = placed(h, dtype, shift), placed(prob, dtype, shift)
    F = s.F0 + s.F1
    shapes = dict(x0_diff=(s.N, s.F0), x1_diff=(s.N, s.F1), w1_diff=(s.H, F), b1_diff=(s.H,), w2_diff=(s.C, s.H),
                  b2_diff=(s.C,))
    g = {}
    for k, want in zip(R.OUTPUTS_BWD, outputs):
        if k == "x1_diff" and not s.F1:
            continue
        g[k] = Guarded(shapes[k], dtype, inp[k + "0"] if k in PARAM_DIFFS else float("nan"), shift)
    given = {k: (g[k].t if k in g and want else None) for k, want in zip(R.OUTPUTS_BWD, outputs)}
    bwd(dev["x0"], dev["x1"], dev["w1"], dev["w2"], mask, hd, pd, dev["label"], inp["loss_weight"], **given,
        **kwargs(cfg, route, ws))
    out = {}
    for k, v in g.items():
        a = v.host(k)
        if given[k] is not None:
            out[k] = a
        elif k in PARAM_DIFFS:
            assert_words_equal(a, np.array(inp[k + "0"], dtype=dtype), k + " was not asked for")
        else:
            assert np.isnan(a).all(), k + " was not asked for"
    assert_words_equal(host(hd), np.array(h, dtype=dtype), "h is an input")
    assert_words_equal(host(pd), np.array(prob, dtype=dtype), "prob is an input")
    return out


@functools.lru_cache(maxsize=None)
def case(s, dtype, k):
    """(cfg, inputs, the float64 model's forward, its backward from h and prob as the device gets them); shared, frozen."""
    cfg, ignored, oor = R.CASES[k]
    inp = R.conditioned_inputs(s, dtype, SEED, cfg, ignored, oor)
    fwd = R.forward(s, cfg, inp)
    h, prob = fwd["h"].astype(dtype), fwd["prob"].astype(dtype)
    bwd = R.backward(s, cfg, inp, h, prob)
    for v in list(fwd.values()) + list(bwd.values()) + [h, prob]:
        v.setflags(write=False)
    return cfg, inp, fwd, bwd, h, prob


def report(got, want, tag):
    for k in sorted(want):
        scale = max(1.0, float(np.max(np.abs(want[k])))) if want[k].size else 1.0
        err = float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) if want[k].size else 0.0
        print("%-8s %-8s %.3e" % (tag, k, err / scale))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("s", R.GPU_SHAPES, ids=SHAPE_IDS)
def test_accuracy_and_determinism(s, variant, hiplib):
    """Per shape and call: every case of R.CASES (TRAIN at ratio 0.5 and 0.1, TEST, the four normalizations, ignored and
    out-of-range labels) against the float64 model at the bar, forward and backward; then one case again with a
    NaN-filled workspace and every array one element off a 16-byte boundary: the same words."""
    _, dtype, route = variant
    first = None
    for k in range(len(R.CASES)):
        cfg, inp, fwant, bwant, h, prob = case(s, dtype, k)
        fgot = run_forward(s, cfg, inp, dtype, route)
        bgot = run_backward(s, cfg, inp, h, prob, dtype, route)
        assert sorted(fgot) == sorted(fwant) and sorted(bgot) == sorted(bwant)
        report(fgot, fwant, "case %d" % k)
        report(bgot, bwant, "case %d" % k)
        for key in sorted(fwant):
            assert fgot[key].dtype == dtype
            assert_close(fgot[key], fwant[key], BAR[dtype], "case %d, %s" % (k, key))
        for key in sorted(bwant):
            assert bgot[key].dtype == dtype
            assert_close(bgot[key], bwant[key], BAR[dtype], "case %d, %s" % (k, key))
        if k == (s.N + s.H) % len(R.CASES):
            first = (k, fgot, bgot)
    k, fgot, bgot = first
    cfg, inp, _, _, h, prob = case(s, dtype, k)
    again = run_forward(s, cfg, inp, dtype, route, shift=1, ws=nan_workspace(s, dtype))
    again.update(run_backward(s, cfg, inp, h, prob, dtype, route, shift=1, ws=nan_workspace(s, dtype)))
    for key, v in list(fgot.items()) + list(bgot.items()):
        assert_words_equal(again[key], v, key + ", second run: NaN workspace, arrays off by one element")


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("s", [R.V4, R.V4_TEST, R.GPU_SHAPES[7], R.GENERIC_SHAPES[0]], ids=R.sid)
def test_deploy_form(s, variant, hiplib):
    """label == NULL: h and prob have the words of the call with a label, and there is no loss."""
    _, dtype, route = variant
    for k in (0, 2):
        cfg, inp, fwant, _, _, _ = case(s, dtype, k)
        with_label = run_forward(s, cfg, inp, dtype, route)
        deploy = run_forward(s, cfg, inp, dtype, route, label=False)
        assert sorted(deploy) == ["h", "prob"]
        for key in deploy:
            assert_words_equal(deploy[key], with_label[key], key)
            assert_close(deploy[key], fwant[key], BAR[dtype], key)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("s", R.GPU_SHAPES, ids=SHAPE_IDS)
def test_dyadic_probes_of_the_backward(s, variant, hiplib):
    """Every output equals the int64 reference word for word, on top of integer initial diffs; with outputs left out,
    those given keep their words and the others are untouched."""
    _, dtype, route = variant
    for k in range(2):
        cfg, inp, h, prob, want, bound = R.shared_probe(s, SEED, k)
        assert bound < 2 ** 24
        got = run_backward(s, cfg, inp, h, prob, dtype, route)
        assert sorted(got) == sorted(want)
        for key, v in want.items():
            assert_words_equal(got[key], v.astype(dtype), "probe %d, %s" % (k, key))
        outputs = tuple(bool((0b101101 if k else 0b010110) >> b & 1) for b in range(6))
        part = run_backward(s, cfg, inp, h, prob, dtype, route, outputs=outputs)
        assert sorted(part) == sorted(key for key, o in zip(R.OUTPUTS_BWD, outputs) if o and key in want)
        for key, v in part.items():
            assert_words_equal(v, want[key].astype(dtype), "probe %d, %s with outputs %s" % (k, key, outputs))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_accumulation_is_on_top_of_what_is_there(variant, hiplib):
    """Two backward calls into the same diffs add twice; x0_diff and x1_diff are overwritten each time."""
    _, dtype, route = variant
    _, bwd = api(dtype)
    for s in (R.V4, R.GPU_SHAPES[14]):
        cfg, inp, h, prob, _, _ = R.dyadic_probe(s, SEED)
        dev = [placed(inp[k], dtype) for k in ("x0", "x1", "w1", "w2")] + [placed(inp["mask"], np.int32)] + \
              [placed(a, dtype) for a in (h, prob, inp["label"])]
        F = s.F0 + s.F1
        t = TORCH[dtype]
        diffs = [torch.full((s.N, s.F0), 55.0, dtype=t, device="cuda"), torch.full((s.N, s.F1), 55.0, dtype=t, device="cuda"),
                 torch.zeros(s.H, F, dtype=t, device="cuda"), torch.zeros(s.H, dtype=t, device="cuda"),
                 torch.zeros(s.C, s.H, dtype=t, device="cuda"), torch.zeros(s.C, dtype=t, device="cuda")]
        bwd(*dev, inp["loss_weight"], *diffs, **kwargs(cfg, route, None))
        once = [host(d).copy() for d in diffs]
        bwd(*dev, inp["loss_weight"], *diffs, **kwargs(cfg, route, None))
        for k, (d, o) in enumerate(zip(diffs, once)):
            assert_words_equal(host(d), o if k < 2 else 2 * o, R.OUTPUTS_BWD[k] + ", second call")


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_clamp(variant, hiplib):
    """z2 gaps of 240 with the label on the losing class: every loss term is -log(FLT_MIN), in float and in double."""
    from test_head_reference import clamp_case
    _, dtype, route = variant
    s, inp = clamp_case(dtype)
    for norm, div in ((R.NONE, 1), (R.VALID, s.N)):
        cfg = R.Cfg(R.TEST, 0.5, norm, None)
        got = run_forward(s, cfg, inp, dtype, route)
        want = -s.N * np.log(np.float64(R.FLT_MIN)) / div
        assert_close(got["loss"], np.array([want]), BAR[dtype], "loss")
        assert_close(got["prob"], np.tile(np.array([1.0, 0.0]), (s.N, 1)), BAR[dtype], "prob")


@pytest.mark.parametrize("s", [R.V4, R.V4_TEST, R.V4_2, R.INDEPENDENCE_SHAPE], ids=R.sid)
def test_fast_and_generic_routes_agree(s, hiplib):
    from mms_answer_selection_amd import head
    for p in (head.PASS_FORWARD, head.PASS_BACKWARD):
        assert head.head_route(head.head_shape(*s), p) == head.ROUTE_FAST
    for k in (0, 1, 2):
        cfg, inp, _, _, h, prob = case(s, np.float32, k)
        fast = run_forward(s, cfg, inp, np.float32, "auto")
        fast.update(run_backward(s, cfg, inp, h, prob, np.float32, "auto"))
        generic = run_forward(s, cfg, inp, np.float32, "generic")
        generic.update(run_backward(s, cfg, inp, h, prob, np.float32, "generic"))
        for key in sorted(generic):
            assert_close(fast[key], generic[key], TOL, "case %d, %s: fast against generic" % (k, key))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_refused_calls_and_empty_batches_write_nothing(variant, hiplib):
    from mms_answer_selection_amd import capi
    _, dtype, route = variant
    s = R.V4
    cfg, inp, _, _, h, prob = case(s, dtype, 0)
    small = capi.Workspace()
    small.get(64, torch.device("cuda", torch.cuda.current_device()))
    small.get = lambda nbytes, device: (small.buf.data_ptr(), 64)          # a workspace that is too small
    with pytest.raises(capi.MMSError):
        run_forward(s, cfg, inp, dtype, route, ws=small)                    # outputs start as NaN ...
    fwd, bwd = api(dtype)
    dev = [placed(inp[k], dtype) for k in ("x0", "x1", "w1", "b1")] + [placed(inp["mask"], np.int32)] + \
          [placed(inp[k], dtype) for k in ("w2", "b2", "label")]
    outs = [Guarded((s.N, s.H), dtype, 5.0), Guarded((s.N, s.C), dtype, 5.0), Guarded((1,), dtype, 5.0)]
    with pytest.raises(capi.MMSError):
        fwd(*dev, *[o.t for o in outs], **kwargs(cfg, route, small))
    with pytest.raises(capi.MMSError):
        fwd(*dev, outs[0].t, outs[1].t, outs[1].t.view(-1)[:1], **kwargs(cfg, route, None))       # loss is prob's start
    for o in outs:
        assert (o.host("refused forward") == 5.0).all()
    F = s.F0 + s.F1
    diffs = [Guarded(sh, dtype, 5.0) for sh in ((s.N, s.F0), (s.N, s.F1), (s.H, F), (s.H,), (s.C, s.H), (s.C,))]
    bdev = [dev[0], dev[1], dev[2], dev[5], dev[4], placed(h, dtype), placed(prob, dtype), dev[7]]
    with pytest.raises(capi.MMSError):
        bwd(*bdev, 1.0, *[d.t for d in diffs], **kwargs(cfg, route, small))
    t = TORCH[dtype]
    e = lambda *sh: torch.empty(*sh, dtype=t, device="cuda")
    got = fwd(e(0, s.F0), e(0, s.F1), dev[2], dev[3], torch.empty(0, s.H, dtype=torch.int32, device="cuda"), dev[5], dev[6],
              e(0), e(0, s.H), e(0, s.C), outs[2].t, **kwargs(cfg, route, None))
    assert tuple(got[0].shape) == (0, s.H)
    bwd(e(0, s.F0), e(0, s.F1), dev[2], dev[5], torch.empty(0, s.H, dtype=torch.int32, device="cuda"), e(0, s.H),
        e(0, s.C), e(0), 1.0, e(0, s.F0), e(0, s.F1), *[d.t for d in diffs[2:]], **kwargs(cfg, route, None))
    for o in outs + diffs:
        assert (o.host("refused or empty call") == 5.0).all()


def test_prob_goes_straight_to_the_ranking_calls(hiplib):
    """prob of head_forward (TEST) fed to capi's MRR / MAP / AUC calls gives what they give on the model's prob rounded
    to float: the scores are spaced far above 1e-5, so the order is not in question."""
    from mms_answer_selection_amd import capi
    s = R.S(40, 2, 0, 2, 2)
    cfg = R.Cfg(R.TEST, 0.5, R.VALID, None)
    r = np.random.default_rng(SEED)
    x = np.linspace(-1, 1, s.N)[r.permutation(s.N)]
    inp = dict(x0=np.stack([x, 0.5 * x], axis=1).astype(np.float32), x1=None,
               w1=np.array([[2, 0], [0, 2]], dtype=np.float32), b1=None,
               w2=np.array([[-1, -0.5], [1, 0.5]], dtype=np.float32), b2=np.array([0.1, -0.1], dtype=np.float32),
               mask=None, label=(r.random(s.N) < 0.4).astype(np.float32), loss_weight=1.0)
    want = R.forward(s, cfg, inp)["prob"]
    assert np.diff(np.sort(want[:, 1])).min() > 100 * TOL
    got = run_forward(s, cfg, inp, np.float32, "auto")["prob"]
    assert_close(got, want, TOL, "prob")
    label = placed(inp["label"], np.float32)
    group = placed(np.repeat(np.arange(5), 8).astype(np.float32), np.float32)
    mine, model = placed(got, np.float32), placed(want.astype(np.float32), np.float32)
    assert capi.rank_map_mrr(mine, label, group) == capi.rank_map_mrr(model, label, group)
    assert capi.rank_auc(mine, label) == capi.rank_auc(model, label)
    assert capi.rank_map_mrr(mine, label, group)[2] > 0


# ---- batches of more than kHeadMaxSlabs tiles: several slabs of several tiles each ------------------------------------
LARGE_IDS = [R.sid(s) for s in R.LARGE_SHAPES]


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("s", R.LARGE_SHAPES, ids=LARGE_IDS)
def test_large_batches_leave_no_workspace_word_unwritten(s, variant, hiplib):
    """Forward with a loss and backward with every diff, on a zeroed workspace and on one of NaNs that starts one element
    off a 16-byte boundary, both of exactly mms_head_workspace_bytes: the same words in every output, and not a byte
    written outside either workspace.  A slab whose partial sums or loss term were read without having been written
    -- a clipped last slab, a slab taken for empty -- would show as NaN in one run and as a missing term in the other."""
    _, dtype, route = variant
    cfg, inp, _, _, h, prob = case(s, dtype, (s.N + s.H) % len(R.CASES))
    runs = []
    for fill, shift in ((0, 0), (255, np.dtype(dtype).itemsize)):
        wf, wb = ExactWorkspace(s, dtype, fill, shift), ExactWorkspace(s, dtype, fill, shift)
        out = run_forward(s, cfg, inp, dtype, route, ws=wf)
        out.update(run_backward(s, cfg, inp, h, prob, dtype, route, ws=wb))
        wf.check("forward")
        wb.check("backward")
        runs.append(out)
    assert sorted(runs[0]) == sorted(R.OUTPUTS_FWD + R.OUTPUTS_BWD if s.F1 else
                                     [k for k in R.OUTPUTS_FWD + R.OUTPUTS_BWD if k != "x1_diff"])
    for key in sorted(runs[0]):
        assert np.isfinite(runs[0][key]).all(), key
        assert_words_equal(runs[1][key], runs[0][key], key + ": NaN workspace against zeroed workspace")


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_large_batches_samples_are_independent(variant, hiplib):
    """h, prob, x0_diff and x1_diff of the first 16384 samples are the same words whether the call has 16385 samples
    (129 slabs of two tiles) or those 16384 alone (256 slabs of one tile): the cut moves no per-sample word.  The diffs
    under NONE normalization, whose coef does not depend on the batch."""
    _, dtype, route = variant
    s = R.INDEPENDENCE_SHAPE
    short = s._replace(N=s.N - 1)
    assert R.slabs(s.N) == (129, 2) and R.slabs(short.N) == (256, 1)
    cfg = R.Cfg(R.TRAIN, 0.5, R.NONE, 1)
    inp = R.conditioned_inputs(s, dtype, SEED, cfg, True, True)
    cut = {k: (v[:short.N] if k in ("x0", "x1", "mask", "label") else v) for k, v in inp.items()}
    fwd = R.forward(s, cfg, inp)
    h, prob = fwd["h"].astype(dtype), fwd["prob"].astype(dtype)
    whole = run_forward(s, cfg, inp, dtype, route)
    whole.update(run_backward(s, cfg, inp, h, prob, dtype, route))
    part = run_forward(short, cfg, cut, dtype, route)
    part.update(run_backward(short, cfg, cut, h[:short.N], prob[:short.N], dtype, route))
    for key in ("h", "prob", "x0_diff", "x1_diff"):
        assert whole[key].shape[0] == s.N and part[key].shape[0] == short.N
        assert np.count_nonzero(part[key]) > part[key].size // 4, key
        assert_words_equal(whole[key][:short.N], part[key], key + " of the first %d samples" % short.N)
