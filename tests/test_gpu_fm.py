"""GPU suite: the FM calls of the C ABI (include/mms.h mms_fm_*, csrc/fm.hip) against tests/fm_reference.py, the numpy
restatement of the reference's loops.  Every comparison is equality of the 32-bit (or 64-bit) words: FM's results are
fixed by loop order, so there is no tolerance anywhere (the one exception is the loss scalar of the chained test,
which is PairRankLoss's own long sum and keeps its existing 1e-5)."""
import functools

import numpy as np
import pytest
import torch

import fm_reference as R
from util import SEED, TOL, assert_close

pytestmark = pytest.mark.gpu

# (N, C, dim): the smallest shapes at which each thing can go wrong
SHAPES = [
    (1, 1, 1), (2, 4, 1),      # no latent columns: the score is the linear sum, the gradient is top_diff
    (3, 1, 2),                 # one channel
    (5, 2, 301),               # odd sample stride: 2408 bytes, 8-byte aligned only
    (7, 3, 50),
    (65, 80, 51),              # 16-KB samples (LDS panelling), one sample past a wave of 64
    (130, 2, 1025),            # long rows, three waves of samples with a ragged tail
    (4099, 2, 9),              # the N-long bias_diff chain across many workgroups
]
NULLABLE = [(5, 2, 301), (65, 80, 51)]
BIAS = 0.25
GUARD, SENTINEL = 64, -777.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nan_like(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, want.dtype, got.shape, want.shape)
    w = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(got.reshape(-1).view(w) != want.reshape(-1).view(w))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@functools.lru_cache(maxsize=None)
def case(shape, dtype=np.float32, scale=1.0, zero_linear=False):
    """Inputs and the reference's results for one shape, computed once and shared (never modified)."""
    N, C, dim = shape
    r = np.random.default_rng(SEED)
    x = ((r.standard_normal(shape) * 0.4).astype(dtype) * dtype(scale)).astype(dtype)
    if zero_linear:
        x[:, :, 0] = 0
    g = r.standard_normal(N).astype(dtype)
    top = R.fm_forward(x, dtype(BIAS))
    top_nobias = R.fm_forward(x, None)
    bd, db = R.fm_backward(x, g)
    out = dict(x=x, g=g, top=top, top_nobias=top_nobias, bottom_diff=bd, bias_diff=np.array([db], dtype))
    for v in out.values():
        v.setflags(write=False)
    return out


def run_three_calls(c, shape):
    """forward, backward and the fused call on fresh NaN outputs (bias_diff pre-filled with 123)."""
    from mms_answer_selection_amd import capi
    N = shape[0]
    x, g, bias = dev(c["x"]), dev(c["g"]), dev(np.array([BIAS], np.float32))
    top, bd, db = nan_like((N,)), nan_like(shape), torch.full((1,), 123.0, device="cuda")
    capi.fm_forward(x, top, bias=bias)
    capi.fm_backward(x, g, bd, db)
    top2, bd2, db2 = nan_like((N,)), nan_like(shape), torch.full((1,), 123.0, device="cuda")
    capi.fm_forward_backward(x, g, top2, bd2, bias=bias, bias_diff=db2)
    return [host(t) for t in (top, bd, db, top2, bd2, db2)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_backward_and_fused_f32(shape, hiplib):
    """Cases 1, 5 and 6: all three calls at every shape; bias_diff (pre-filled with 123) is overwritten with the plain
    sum; every element of bottom_diff (pre-filled with NaN) is written; the fused call's words are the separate calls'."""
    c = case(shape)
    top, bd, db, top2, bd2, db2 = run_three_calls(c, shape)
    assert_words_equal(top, c["top"], "top")
    assert_words_equal(bd, c["bottom_diff"], "bottom_diff")
    assert_words_equal(db, c["bias_diff"], "bias_diff")
    assert not np.isnan(bd).any() and not np.isnan(bd2).any()
    assert_words_equal(top2, c["top"], "fused top")
    assert_words_equal(bd2, c["bottom_diff"], "fused bottom_diff")
    assert_words_equal(db2, c["bias_diff"], "fused bias_diff")
    assert_words_equal(top2, top, "fused top against forward")
    assert_words_equal(bd2, bd, "fused bottom_diff against backward")
    assert_words_equal(db2, db, "fused bias_diff against backward")
    if shape[2] == 1:
        assert_words_equal(bd, np.broadcast_to(c["g"][:, None, None], shape), "no latent columns: gradient is top_diff")


@pytest.mark.parametrize("shape", NULLABLE, ids=str)
def test_optional_arrays_f32(shape, hiplib):
    """Cases 2, 3 and 4: bias = NULL (no bias term in the score), bias_diff = NULL (bottom_diff unchanged),
    bottom_diff = NULL (bias_diff alone is produced)."""
    from mms_answer_selection_amd import capi
    c = case(shape)
    N = shape[0]
    x, g, bias = dev(c["x"]), dev(c["g"]), dev(np.array([BIAS], np.float32))
    top = nan_like((N,))
    capi.fm_forward(x, top)
    assert_words_equal(host(top), c["top_nobias"], "top without bias")
    bd = nan_like(shape)
    capi.fm_backward(x, g, bd, None)
    assert_words_equal(host(bd), c["bottom_diff"], "bottom_diff with bias_diff = NULL")
    db = torch.full((1,), 123.0, device="cuda")
    capi.fm_backward(x, g, None, db)
    assert_words_equal(host(db), c["bias_diff"], "bias_diff with bottom_diff = NULL")
    capi.fm_backward(x, g, None, None)                       # nothing asked for: a no-op
    # the fused call: bias and bias_diff are optional each on their own
    for use_bias, use_db in ((False, False), (True, False), (False, True)):
        top2, bd2, db2 = nan_like((N,)), nan_like(shape), torch.full((1,), 123.0, device="cuda")
        capi.fm_forward_backward(x, g, top2, bd2, bias=bias if use_bias else None, bias_diff=db2 if use_db else None)
        assert_words_equal(host(top2), c["top"] if use_bias else c["top_nobias"], "fused top")
        assert_words_equal(host(bd2), c["bottom_diff"], "fused bottom_diff")
        if use_db:
            assert_words_equal(host(db2), c["bias_diff"], "fused bias_diff")
        else:
            assert host(db2)[0] == 123.0
    with pytest.raises(capi.MMSError):
        capi.fm_forward_backward(x, g, top, None)


@pytest.mark.parametrize("shape", [(65, 80, 51), (5, 2, 301)], ids=str)
def test_nothing_outside_the_outputs_is_written(shape, hiplib):
    """Case 7: top and bottom_diff sit between 64 guard elements on either side; the guards survive all three calls."""
    from mms_answer_selection_amd import capi
    c = case(shape)
    N, n = shape[0], int(np.prod(shape))
    x, g, bias = dev(c["x"]), dev(c["g"]), dev(np.array([BIAS], np.float32))

    def guarded(count):
        buf = torch.full((count + 2 * GUARD,), SENTINEL, device="cuda")
        return buf, buf[GUARD:GUARD + count]

    def intact(buf, count, want, what):
        b = host(buf)
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + count:] == SENTINEL).all(), what + ": guard overwritten"
        assert_words_equal(b[GUARD:GUARD + count], want.reshape(-1), what)

    tbuf, top = guarded(N)
    capi.fm_forward(x, top, bias=bias)
    intact(tbuf, N, c["top"], "forward top")
    bbuf, bd = guarded(n)
    dbuf, db = guarded(1)
    capi.fm_backward(x, g, bd, db)
    intact(bbuf, n, c["bottom_diff"], "backward bottom_diff")
    intact(dbuf, 1, c["bias_diff"], "backward bias_diff")
    tbuf, top = guarded(N)
    bbuf, bd = guarded(n)
    dbuf, db = guarded(1)
    capi.fm_forward_backward(x, g, top, bd, bias=bias, bias_diff=db)
    intact(tbuf, N, c["top"], "fused top")
    intact(bbuf, n, c["bottom_diff"], "fused bottom_diff")
    intact(dbuf, 1, c["bias_diff"], "fused bias_diff")


@pytest.mark.parametrize("scale", [2.0 ** -68, 2.0 ** 40], ids=["2^-68", "2^40"])
def test_extreme_scales_keep_the_reference_bits(scale, hiplib):
    """Case 8: with x scaled by 2^-68 the squares are subnormal (0.4^2 2^-136): the device must not flush what the
    x86 reference keeps; by 2^40 they are huge.  The words are still equal."""
    shape = (5, 2, 301)
    c = case(shape, np.float32, scale)
    if scale < 1:
        sq = c["x"] * c["x"]
        assert ((sq != 0) & (np.abs(sq) < np.finfo(np.float32).tiny)).mean() > 0.9      # the inputs do what they are for
    top, bd, db, top2, bd2, db2 = run_three_calls(c, shape)
    assert_words_equal(top, c["top"], "top")
    assert_words_equal(bd, c["bottom_diff"], "bottom_diff")
    assert_words_equal(db, c["bias_diff"], "bias_diff")
    assert_words_equal(top2, c["top"], "fused top")
    assert_words_equal(bd2, c["bottom_diff"], "fused bottom_diff")
    assert_words_equal(db2, c["bias_diff"], "fused bias_diff")


def test_a_subnormal_chain_reaches_the_output(hiplib):
    """Beside case 8: there the linear column (2^-68) and the bias swallow the subnormal chain in the score.  With the
    linear column zero and no bias the score IS the chain's subnormal value."""
    from mms_answer_selection_amd import capi
    shape = (5, 2, 301)
    c = case(shape, np.float32, 2.0 ** -68, True)
    tiny = np.finfo(np.float32).tiny
    assert ((c["top_nobias"] != 0) & (np.abs(c["top_nobias"]) < tiny)).all()
    x, g = dev(c["x"]), dev(c["g"])
    top, top2, bd2 = nan_like((5,)), nan_like((5,)), nan_like(shape)
    capi.fm_forward(x, top)
    capi.fm_forward_backward(x, g, top2, bd2)
    assert_words_equal(host(top), c["top_nobias"], "subnormal top")
    assert_words_equal(host(top2), c["top_nobias"], "subnormal fused top")
    assert_words_equal(host(bd2), c["bottom_diff"], "bottom_diff")


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 2, 301), (7, 3, 50), (65, 80, 51)], ids=str)
def test_forward_and_backward_f64(shape, hiplib):
    """Case 9: the double instantiation, 64-bit word equality."""
    from mms_answer_selection_amd import capi
    c = case(shape, np.float64)
    N = shape[0]
    D = torch.float64
    x, g, bias = dev(c["x"]), dev(c["g"]), dev(np.array([BIAS], np.float64))
    top, bd, db = nan_like((N,), D), nan_like(shape, D), torch.full((1,), 123.0, dtype=D, device="cuda")
    capi.fm_forward_f64(x, top, bias=bias)
    capi.fm_backward_f64(x, g, bd, db)
    assert_words_equal(host(top), c["top"], "top f64")
    assert_words_equal(host(bd), c["bottom_diff"], "bottom_diff f64")
    assert_words_equal(host(db), c["bias_diff"], "bias_diff f64")
    top2 = nan_like((N,), D)
    capi.fm_forward_f64(x, top2)
    assert_words_equal(host(top2), c["top_nobias"], "top f64 without bias")
    db2 = torch.full((1,), 123.0, dtype=D, device="cuda")
    capi.fm_backward_f64(x, g, None, db2)
    assert_words_equal(host(db2), c["bias_diff"], "bias_diff f64 alone")


def test_fused_call_is_deterministic_and_stream_agnostic(hiplib):
    """Cases 10 and 11: two runs of the fused call at (130, 2, 1025) give identical words, and so does a run on a
    non-default stream."""
    from mms_answer_selection_amd import capi
    shape = (130, 2, 1025)
    c = case(shape)
    x, g, bias = dev(c["x"]), dev(c["g"]), dev(np.array([BIAS], np.float32))

    def run():
        top, bd, db = nan_like((shape[0],)), nan_like(shape), nan_like((1,))
        capi.fm_forward_backward(x, g, top, bd, bias=bias, bias_diff=db)
        return top, bd, db

    first = [host(t) for t in run()]
    second = [host(t) for t in run()]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = run()
        top_s, bd_s, db_s = nan_like((shape[0],)), nan_like(shape), nan_like((1,))
        capi.fm_forward(x, top_s, bias=bias)
        capi.fm_backward(x, g, bd_s, db_s)
    s.synchronize()
    third = [host(t) for t in outs]
    fourth = [host(t) for t in (top_s, bd_s, db_s)]
    for name, a, b, d, e, want in zip(("top", "bottom_diff", "bias_diff"), first, second, third, fourth,
                                      (c["top"], c["bottom_diff"], c["bias_diff"])):
        assert_words_equal(a, want, name)
        assert_words_equal(b, a, name + ", second run")
        assert_words_equal(d, a, name + ", side stream")
        assert_words_equal(e, a, name + ", separate calls on the side stream")


def test_chained_with_pairrank_loss(oracle, hiplib):
    """Case 12: fm_forward on both halves of a triplet batch -> PairRankLoss forward / backward -> fm_backward, against
    the same chain computed with tests/fm_reference.py and the oracle's PairRankLoss.  Per-element outputs and the
    bottom diffs bitwise; the loss scalar at the existing 1e-5."""
    from mms_answer_selection_amd import capi
    N, C, dim = 64, 2, 301
    r = np.random.default_rng(SEED)
    q = (r.standard_normal((N, 1, dim)) * 0.4).astype(np.float32)
    ap = (r.standard_normal((N, 1, dim)) * 0.4).astype(np.float32)
    an = (r.standard_normal((N, 1, dim)) * 0.4).astype(np.float32)
    xp, xn = np.concatenate([q, ap], axis=1), np.concatenate([q, an], axis=1)
    y = (r.uniform(size=(N, 1)) < 0.8).astype(np.float32)
    margin, lw = 1.0, 1.0
    b = np.float32(BIAS)

    sp_ref, sn_ref = R.fm_forward(xp, b).reshape(N, 1), R.fm_forward(xn, b).reshape(N, 1)
    loss_ref, o_ref, s_ref = oracle.pairrank_forward(sp_ref, sn_ref, y, margin)
    gp_ref, gn_ref = oracle.pairrank_backward(y, o_ref, s_ref, top_diff=lw)
    bdp_ref, dbp_ref = R.fm_backward(xp, gp_ref.reshape(N))
    bdn_ref, dbn_ref = R.fm_backward(xn, gn_ref.reshape(N))

    xpd, xnd, yd, bias = dev(xp), dev(xn), dev(y), dev(np.array([BIAS], np.float32))
    sp, sn = nan_like((N, 1)), nan_like((N, 1))
    capi.fm_forward(xpd, sp, bias=bias)
    capi.fm_forward(xnd, sn, bias=bias)
    o, s, loss = nan_like((N, 1)), nan_like((N, 1)), nan_like((1,))
    capi.pairrank_forward(sp, sn, yd, o, s, loss, margin=margin)
    gp, gn = nan_like((N, 1)), nan_like((N, 1))
    capi.pairrank_backward(yd, o, s, gp, gn, top_diff=lw)
    bdp, bdn, dbp, dbn = nan_like(xp.shape), nan_like(xn.shape), nan_like((1,)), nan_like((1,))
    capi.fm_backward(xpd, gp, bdp, dbp)
    capi.fm_backward(xnd, gn, bdn, dbn)

    assert_words_equal(host(sp), sp_ref, "s_pos")
    assert_words_equal(host(sn), sn_ref, "s_neg")
    assert_words_equal(host(o), o_ref, "ordered_diff_")
    assert_words_equal(host(s), s_ref, "similar_diff_")
    assert_close(host(loss)[0], loss_ref, TOL, "loss")
    assert_words_equal(host(gp), gp_ref, "d s_pos")
    assert_words_equal(host(gn), gn_ref, "d s_neg")
    assert_words_equal(host(bdp), bdp_ref, "bottom_diff, positive half")
    assert_words_equal(host(bdn), bdn_ref, "bottom_diff, negative half")
    assert_words_equal(host(dbp), np.array([dbp_ref], np.float32), "bias_diff, positive half")
    assert_words_equal(host(dbn), np.array([dbn_ref], np.float32), "bias_diff, negative half")
