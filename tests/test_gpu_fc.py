"""GPU suite of the InnerProduct, Softmax, SoftmaxWithLoss and Concat calls (include/mms_fc.h) against tests/fc_reference.py:
Concat's copies word for word at every alignment; InnerProduct on integer probes bit for bit with an int64 reference on
every route, on every variant and flag (the test asserts the shape list reaches each route in each pass), on dense data at the project's bars for
BLAS-ordered layers, the same words twice over a workspace of NaN and with every array shifted off its 16-byte boundary; Softmax and SoftmaxWithLoss against the model,
the loss word for word on dyadic probes; the per-layer chain against the fused head's generic route; and the SimMatrix
net's four-bottom Concat -> InnerProduct(64)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import fc_reference as R
import head_reference as H
from util import SEED, TOL

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
F64_TOL = 1e-12
TOLS = {np.float32: TOL, np.float64: F64_TOL}


@pytest.fixture(scope="module")
def fc(hiplib):
    from mms_answer_selection_amd import fc
    fc.lib()
    return fc


def tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def dev(a, off=0):
    """a on the device; off = 1: its first element one element past a 16-byte boundary (torch's blocks are aligned)."""
    t = torch.from_numpy(np.array(a))
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def empty(shape, dtype, off=0, fill=None):
    buf = torch.empty(int(np.prod(shape)) + off, dtype=tdt(dtype), device="cuda")
    if fill is not None:
        buf.fill_(fill)
    return buf[off:].view(tuple(shape))


def host(t):
    return t.cpu().numpy()


def same_words(got, want, what):
    got, want = np.ascontiguousarray(host(got) if isinstance(got, torch.Tensor) else got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.itemsize]
    bad = np.flatnonzero(got.ravel().view(u) != want.ravel().view(u))
    assert not bad.size, "%s: %d of %d words differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def close(got, want, tol, what):
    got, want = np.asarray(host(got) if isinstance(got, torch.Tensor) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    assert np.isfinite(err) and err <= tol * scale, "%s: max abs err %.3e > %.1e * %.3g" % (what, err, tol, scale)


# ---- Concat ----------------------------------------------------------------------------------------------------------
EXTENTS = {1: (64,), 2: (3, 4), 4: (1, 3, 4, 64), 8: (1, 3, 4, 64, 64, 4, 3, 1)}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-by-one"])
@pytest.mark.parametrize("inner", [1, 5, 16])
@pytest.mark.parametrize("num_concats", [1, 7])
@pytest.mark.parametrize("nb", [1, 2, 4, 8])
def test_concat_moves_the_words(fc, nb, num_concats, inner, off, dtype):
    ext = EXTENTS[nb]
    r = np.random.default_rng(SEED + nb + inner)
    bottoms = [r.standard_normal((num_concats, e, inner)).astype(dtype) for e in ext]
    bottoms[0].reshape(-1).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize])[0] |= 1   # any bit pattern moves
    want = R.concat_forward(bottoms)
    top = empty(want.shape, dtype, off)
    fc.concat_forward([dev(b, off) for b in bottoms], out=top)
    same_words(top, want, "top")
    td = r.standard_normal(want.shape).astype(dtype)
    skip = nb // 2                                                   # one NULL diff: propagate_down false
    outs = [empty(b.shape, dtype, off, fill=-7.0) for b in bottoms]
    keep = outs[skip]
    got = fc.concat_backward(dev(td, off), [b.shape for b in bottoms], [None if i == skip and nb > 1 else o
                                                                       for i, o in enumerate(outs)])
    for i, (g, w) in enumerate(zip(got, R.concat_backward(td, ext))):
        if g is None:
            assert i == skip and (host(keep) == -7.0).all()
        else:
            same_words(g, w, "bottom diff %d" % i)


def test_concat_mixed_alignment_and_binding_axis(fc):
    """bottoms whose runs are and are not multiples of 16 bytes in one call, through the binding's axis arithmetic"""
    r = np.random.default_rng(SEED)
    bottoms = [r.standard_normal((2, 3, e, 4)).astype(np.float32) for e in (4, 1, 8)]
    same_words(fc.concat_forward([dev(b) for b in bottoms], axis=2), np.concatenate(bottoms, axis=2), "top")
    same_words(fc.concat_forward([dev(b) for b in bottoms], axis=-2), np.concatenate(bottoms, axis=2), "top")


# ---- InnerProduct ----------------------------------------------------------------------------------------------------
KC = R.K
M_EDGE = KC["kFcSlabRows"]
IP_SHAPES = sorted(set(
    list(itertools.product((1, 7, 50, 257), (1, 3, 68, 205), (1, 2, 32, 33, 64)))
    + [(16, 20, 17), (17, 20, 17), (17, 16, 17), (17, 17, 16), (17, 17, 17), (50, 17, 16)]      # around kFcNarrowMax
    + [(M_EDGE - 1, 4, 5), (M_EDGE, 4, 5), (M_EDGE + 1, 4, 5), (2 * M_EDGE + 1, 20, 18)]        # slab boundaries
    + [(31, 32, 2), (32, 32, 2), (1, 2047, 1), (1, 2048, 1), (129, 3, 5)]                       # around kFcFastMinMacs
    + [(50, KC["kFcFastFwdMinK"] - 1, 32), (50, KC["kFcFastFwdMinK"], 32), (M_EDGE, 66, 32), (M_EDGE + 1, 66, 32)]   # the routes' edges
    + [(KC["kFcSlabRows"] * KC["kFcMaxSlabs"] + 1, 3, 2)]                                       # the slabs grow: 160 rows
    + [(64, 64, 64), (65, 33, 65), (130, 36, 70), (144, 32, 16)]))                              # whole and ragged tiles


def ip_run(fc, d, dtype, transpose, bias, route, ws_fill=None, off=0):
    """forward, then backward onto the initial diffs -> (top, w_diff, b_diff, bottom_diff) on the host.  off = 1: every
    array of both calls begins one element past a 16-byte boundary."""
    x, w, td = (dev(d[k].astype(dtype), off) for k in ("x", "w", "td"))
    b = dev(d["b"].astype(dtype), off) if bias else None
    top = empty(d["td"].shape, dtype, off)
    fc.inner_product_forward(x, w, b, out=top, transpose=transpose, route=route)
    dw, db = dev(d["w_diff0"].astype(dtype), off), dev(d["b_diff0"].astype(dtype), off) if bias else None
    from mms_answer_selection_amd import capi
    ws = capi.Workspace()
    if ws_fill is not None:
        M, Kd = d["x"].shape
        need = R.ip_workspace_bytes(M, Kd, d["td"].shape[1], np.dtype(dtype).itemsize)
        ws.get(need, x.device)
        ws.buf.view(torch.uint8).fill_(0xFF)                          # every word a NaN
    dx = empty(d["x"].shape, dtype, off, fill=float("nan"))
    fc.inner_product_backward(x, w, td, dw, db, dx, transpose=transpose, ws=ws, route=route)
    return host(top), host(dw), host(db) if bias else None, host(dx)


VARIANTS = [("auto", np.float32), ("generic", np.float32), ("auto", np.float64)]
VARIANT_IDS = ["f32", "generic_f32", "f64"]


@pytest.mark.parametrize("bias", [False, True], ids=["no-bias", "bias"])
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transpose"])
@pytest.mark.parametrize("how,dtype", VARIANTS, ids=VARIANT_IDS)
def test_inner_product_integer_probes_are_exact(fc, how, dtype, transpose, bias):
    """|x| <= 8 integers: every partial sum is an exactly representable float, so each route and slab count must give
    the int64 reference's words.  Every shape of IP_SHAPES runs on every variant with every value of transpose and
    bias_term; which route each pass of the float call took is read from mms_inner_product_route, and the list must
    reach each route in each pass, one, two and more slabs, the long slabs, and ragged and whole tiles."""
    reached = set()
    for M, Kd, N in IP_SHAPES:
        d = R.ip_integers(M, Kd, N, SEED, transpose)
        want = R.ip_exact(d["x"], d["w"], d["b"] if bias else None, d["td"], transpose, d["w_diff0"], d["b_diff0"])
        assert max(int(np.abs(v).max()) for v in want) < 2 ** 24
        shape = fc.inner_product_shape(M, Kd, N, transpose, bias)
        fr, br = (fc.inner_product_route(shape, p) for p in (fc.PASS_FORWARD, fc.PASS_BACKWARD))
        assert (fr, br) == (R.ip_route(M, Kd, N, R.FORWARD), R.ip_route(M, Kd, N, R.BACKWARD))
        assert fc.inner_product_workspace_bytes(shape) == R.ip_workspace_bytes(M, Kd, N, 4)
        assert fc.inner_product_workspace_bytes_f64(shape) == R.ip_workspace_bytes(M, Kd, N, 8)
        got = ip_run(fc, d, dtype, transpose, bias, how)
        for name, g, w in zip(("top", "w_diff", "b_diff", "bottom_diff"), got, want):
            if g is not None:
                same_words(g, w.astype(dtype), "%s %s" % ((M, Kd, N), name))
        reached.update([("fwd", fr), ("bwd", br), ("slabs", min(R.slabs(M), 3))])
        if fr == R.ROUTE_FAST:
            reached.update([("fwd tiles ragged", bool(M % 16 or N % 16)), ("fwd K % 32", bool(Kd % 32))])
        if br == R.ROUTE_FAST:
            reached.update([("bwd slabs", min(R.slabs(M), 3)), ("bwd long slabs", R.slab_rows(M) > M_EDGE),
                            ("bwd tiles ragged", bool(M % 16 or N % 16 or Kd % 16))])
    for need in [("fwd", R.ROUTE_FAST), ("fwd", R.ROUTE_GENERIC), ("bwd", R.ROUTE_FAST), ("bwd", R.ROUTE_GENERIC),
                 ("slabs", 1), ("slabs", 2), ("slabs", 3), ("bwd slabs", 2), ("bwd slabs", 3), ("bwd long slabs", True),
                 ("bwd long slabs", False), ("fwd tiles ragged", True), ("fwd tiles ragged", False), ("fwd K % 32", True),
                 ("fwd K % 32", False), ("bwd tiles ragged", True), ("bwd tiles ragged", False)]:
        assert need in reached, (need, sorted(map(str, reached)))


DENSE = [(50, 66, 32), (50, 32, 2), (257, 205, 64), (1517, 66, 32), (7, 3, 2), (50, 205, 64), (50, 203, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transpose"])
@pytest.mark.parametrize("shape", DENSE, ids=str)
def test_inner_product_dense_repeatable_and_blind_to_alignment(fc, shape, transpose, dtype):
    """1e-5 / 1e-12 against the float64 model; a second call over a workspace of NaN gives the same words; and so does
    the call with every array shifted by one element off its 16-byte boundary: the order of the sums is a function of
    the shape and the route alone."""
    M, Kd, N = shape
    d = R.ip_dense(M, Kd, N, dtype, SEED, transpose)
    want_top = R.ip_forward(d["x"], d["w"], d["b"], transpose)
    want = (want_top,) + R.ip_backward(d["x"], d["w"], d["td"], transpose, d["w_diff0"], d["b_diff0"])
    routes = ["auto", "generic"] if dtype == np.float32 else ["auto"]
    for route in routes:
        first = ip_run(fc, d, dtype, transpose, True, route, ws_fill=True)
        again = ip_run(fc, d, dtype, transpose, True, route, ws_fill=True)
        shifted = ip_run(fc, d, dtype, transpose, True, route, ws_fill=True, off=1)
        for name, g, g2, g3, w in zip(("top", "w_diff", "b_diff", "bottom_diff"), first, again, shifted, want):
            close(g, w, TOLS[dtype], "%s %s" % (route, name))
            same_words(g2, g, "%s %s, second call" % (route, name))
            same_words(g3, g, "%s %s, arrays one element off a 16-byte boundary" % (route, name))


def test_refused_calls_leave_their_outputs_untouched(fc, hiplib):
    """Rows of the refusal table on real buffers: a short workspace, an output that aliases an input, an unknown
    normalization, nine bottoms.  Each call returns its code and every output keeps its words."""
    import ctypes as C
    d = R.ip_dense(129, 20, 18, np.float32, SEED)
    x, w, td = dev(d["x"]), dev(d["w"]), dev(d["td"])
    dw, db, dx, ws = dev(d["w_diff0"]), dev(d["b_diff0"]), empty((129, 20), np.float32, fill=-7.0), empty((8192,), np.float32, fill=-7.0)
    shape = fc.inner_product_shape(129, 20, 18)
    need = fc.inner_product_workspace_bytes(shape)
    bwd = hiplib.mms_inner_product_backward_f32
    p = lambda t: C.c_void_p(t.data_ptr())
    assert bwd(C.byref(shape), p(x), p(w), p(td), p(dw), p(db), p(dx), p(ws), need - 1, None) == R.WORKSPACE
    assert bwd(C.byref(shape), p(x), p(w), p(td), p(dw), p(db), p(x), p(ws), need, None) == R.INVALID      # bottom_diff is x
    top = empty((129, 18), np.float32, fill=-7.0)
    assert hiplib.mms_inner_product_forward_f32(C.byref(shape), p(x), p(w), None, p(top), None) == R.INVALID   # bias_term, no b
    torch.cuda.synchronize()
    same_words(dw, d["w_diff0"], "w_diff")
    same_words(db, d["b_diff0"], "b_diff")
    same_words(x, d["x"], "x")
    for t in (dx, ws, top):
        assert (host(t) == -7.0).all()
    z, lab = dev(d["td"]), dev(np.zeros(129, np.float32))
    prob, loss, lws = empty((129, 18), np.float32, fill=-7.0), empty((1,), np.float32, fill=-7.0), empty((64,), np.float32, fill=-7.0)
    bad = fc.softmax_loss_shape(129, 18, 1, normalization=4)
    assert hiplib.mms_softmax_loss_forward_f32(C.byref(bad), p(z), p(lab), p(prob), p(loss), p(lws), 256, None) == R.INVALID
    ok = fc.softmax_loss_shape(129, 18, 1)
    short = fc.softmax_loss_workspace_bytes(ok) - 1
    assert hiplib.mms_softmax_loss_forward_f32(C.byref(ok), p(z), p(lab), p(prob), p(loss), p(lws), short, None) == R.WORKSPACE
    assert hiplib.mms_softmax_forward_f32(C.byref(fc.SoftmaxShape(129, 18, 1)), p(z), p(z), None) == R.INVALID
    nine = fc.ConcatShape(129, 1, 9, (C.c_int * 8)(*[2] * 8))
    ptrs = (C.c_void_p * 9)(*[z.data_ptr()] * 9)
    assert hiplib.mms_concat_forward_f32(C.byref(nine), ptrs, p(prob), None) == R.INVALID
    one = fc.ConcatShape(129, 1, 1, (C.c_int * 8)(18, 0, 0, 0, 0, 0, 0, 0))
    assert hiplib.mms_concat_forward_f32(C.byref(one), (C.c_void_p * 1)(prob.data_ptr()), p(prob), None) == R.INVALID   # aliases top
    torch.cuda.synchronize()
    same_words(z, d["td"], "bottom")
    for t in (prob, loss, lws):
        assert (host(t) == -7.0).all()


def test_inner_product_null_outputs_are_not_computed(fc):
    d = R.ip_dense(50, 66, 32, np.float32, SEED)
    x, w, td = dev(d["x"]), dev(d["w"]), dev(d["td"])
    want = R.ip_backward(d["x"], d["w"], d["td"], False, d["w_diff0"], d["b_diff0"])
    dw = dev(d["w_diff0"])
    fc.inner_product_backward(x, w, td, w_diff=dw)
    close(dw, want[0], TOL, "w_diff alone")
    db = dev(d["b_diff0"])
    fc.inner_product_backward(None, w, td, b_diff=db)
    close(db, want[1], TOL, "b_diff alone")
    dx = empty((50, 66), np.float32)
    fc.inner_product_backward(None, w, td, bottom_diff=dx)
    close(dx, want[2], TOL, "bottom_diff alone")


# ---- Softmax ---------------------------------------------------------------------------------------------------------
TR = KC["kSoftmaxThreadRowMax"]
SOFTMAX_SHAPES = [(1, 1, 1), (50, 2, 1), (3, 17, 1), (5, 130, 1), (2, 3, 7), (4, 2, 65),
                  (3, TR, 1), (3, TR + 1, 1), (9, 64, 1), (2, 65, 1), (2, 40, 3)]          # both sides of the wave kernel


@functools.lru_cache(maxsize=None)
def softmax_case(shape, dtype):
    r = np.random.default_rng(SEED + sum(shape))
    x = (r.standard_normal(shape) * 3).astype(dtype)
    td = r.standard_normal(shape).astype(dtype)
    return x, td


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=str)
def test_softmax_against_the_model(fc, shape, dtype):
    x, td = softmax_case(shape, dtype)
    top = fc.softmax_forward(dev(x))
    want = R.softmax_forward(x)
    close(top, want, TOLS[dtype], "top")
    sums = host(top).astype(np.float64).sum(axis=1)
    eps = np.finfo(dtype).eps
    assert np.abs(sums - 1).max() <= 2 * eps * shape[1], np.abs(sums - 1).max()
    tdd = dev(td)
    out = fc.softmax_backward(top, tdd)
    close(out, R.softmax_backward(host(top), td), TOLS[dtype], "bottom_diff")
    same_words(fc.softmax_backward(top, tdd, out=tdd), host(out), "in place")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(3, 17, 1), (5, 130, 1), (2, 3, 7)], ids=str)
def test_softmax_spread_of_80_does_not_overflow(fc, shape, dtype):
    x = softmax_case(shape, dtype)[0].copy()
    x[:, 0, :] += 80
    top = host(fc.softmax_forward(dev(x)))
    assert np.isfinite(top).all()
    close(top, R.softmax_forward(x), TOLS[dtype], "top")


# ---- SoftmaxWithLoss -------------------------------------------------------------------------------------------------
NORMS = [R.FULL, R.VALID, R.BATCH_SIZE, R.NONE]
NORM_IDS = ["FULL", "VALID", "BATCH_SIZE", "NONE"]
LOSS_SHAPES = [(50, 2, 1), (9, 5, 7), (300, 3, 1), (3, 40, 1)]            # (300, 3, 1): five slabs of positions


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ignore", [None, 1], ids=["no-ignore", "ignore-1"])
@pytest.mark.parametrize("norm", NORMS, ids=NORM_IDS)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_softmax_loss_dense(fc, shape, norm, ignore, dtype):
    O, C, I = shape
    r = np.random.default_rng(SEED + 13 * O + C + I)
    x = (r.standard_normal(shape) * 2).astype(dtype)
    lab = R.labels(r, O, I, C, ignore, ignored=0.3, out_of_range=0.1).astype(dtype)
    want_prob, want_loss = R.loss_forward(x, lab, norm, ignore)
    prob, loss = fc.softmax_loss_forward(dev(x), dev(lab), normalization=norm, ignore_label=ignore)
    close(prob, want_prob, TOLS[dtype], "prob")
    close(loss, want_loss, TOLS[dtype], "loss")
    diff = fc.softmax_loss_backward(prob, dev(lab), 1.7, normalization=norm, ignore_label=ignore)
    close(diff, R.loss_backward(host(prob), lab, 1.7, norm, ignore), TOLS[dtype], "bottom_diff")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ignore", [None, 1], ids=["no-ignore", "ignore-1"])
@pytest.mark.parametrize("norm", NORMS, ids=NORM_IDS)
@pytest.mark.parametrize("inner", [1, 7])
def test_softmax_loss_dyadic_probes_word_for_word(fc, inner, norm, ignore, dtype):
    """Logits with c equal entries at the top and the rest 2000 below: the softmax is exactly 1/c for c a power of two
    and exactly 0 elsewhere (exp(-2000) is 0 in both types; a label there meets the FLT_MIN clamp), the log argument
    and the counts are exact, and with loss_weight 2 and a power-of-two normalizer so is every diff.  The model sums
    in the library's slabs."""
    O, C = 64, 4
    r = np.random.default_rng(SEED + inner)
    x = np.full((O, C, inner), -1997.0)
    ties = r.choice([1, 2, 4], size=(O, inner))
    for o in range(O):
        for k in range(inner):
            x[o, r.permutation(C)[:ties[o, k]], k] = 3.0
    lab = R.labels(r, O, inner, C, ignore, ignored=0.25, out_of_range=0.1)
    if norm == R.VALID:                                              # a power-of-two count of valid labels
        ok = R.valid_of(lab, C, ignore)[1]
        flat, okf = lab.reshape(-1), ok.reshape(-1)
        want_valid = 1 << (int(okf.sum()).bit_length() - 1)
        flat[np.flatnonzero(okf)[want_valid:]] = -1
        assert int(R.valid_of(lab, C, ignore)[1].sum()) == want_valid
    x, lab = x.astype(dtype), lab.astype(dtype)
    want_prob, want_loss = R.loss_forward(x, lab, norm, ignore, dtype, slab_len=R.loss_slab_len(O * inner))
    assert set(np.unique(want_prob)) <= {0.0, 0.25, 0.5, 1.0}
    prob, loss = fc.softmax_loss_forward(dev(x), dev(lab), normalization=norm, ignore_label=ignore)
    same_words(prob, want_prob, "prob")
    same_words(loss, want_loss, "loss")
    diff = fc.softmax_loss_backward(prob, dev(lab), 2.0, normalization=norm, ignore_label=ignore)
    same_words(diff, R.loss_backward(want_prob, lab, 2.0, norm, ignore, dtype), "bottom_diff")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("norm", NORMS, ids=NORM_IDS)
def test_softmax_loss_with_every_label_ignored(fc, norm, dtype):
    r = np.random.default_rng(SEED)
    x = r.standard_normal((6, 3, 2)).astype(dtype)
    for lab, ignore in ((np.full((6, 2), 2.0), 2), (np.full((6, 2), 3.0), None), (np.full((6, 2), -1.0), None)):
        prob, loss = fc.softmax_loss_forward(dev(x), dev(lab.astype(dtype)), normalization=norm, ignore_label=ignore)
        assert host(loss)[0] == 0.0
        diff = host(fc.softmax_loss_backward(prob, dev(lab.astype(dtype)), 1.0, normalization=norm, ignore_label=ignore))
        assert not diff.any()
        close(prob, R.softmax_forward(x), TOLS[dtype], "prob")


# ---- the chains ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [H.TRAIN, H.TEST], ids=["TRAIN", "TEST"])
def test_the_chain_agrees_with_the_head(fc, phase):
    """network_v4's head shape at N = 50: Concat -> InnerProduct -> TanH -> Dropout -> InnerProduct -> SoftmaxWithLoss
    as per-layer calls, with the mask of mms_dropout_mask_u32, against mms_head_*_generic_f32 on the same mask."""
    from mms_answer_selection_amd import dropout, head, pool
    s, ratio, seed, seq = H.V4, 0.5, 1234, 7
    cfg = H.Cfg(phase, ratio, H.VALID, None)
    inp = H.conditioned_inputs(s, np.float32, SEED, cfg)
    x0, x1, w1, b1, w2, b2, label = (dev(inp[k]) for k in ("x0", "x1", "w1", "b1", "w2", "b2", "label"))
    mask = dropout.dropout_mask((s.N, s.H), ratio, seed, seq)
    train = phase == H.TRAIN
    # the chain
    feat = fc.concat_forward([x0, x1])
    h = pool.tanh_forward(fc.inner_product_forward(feat, w1, b1))
    d = dropout.dropout_forward(h, ratio, seed, seq, train=train)
    z2 = fc.inner_product_forward(d, w2, b2)
    prob, loss = fc.softmax_loss_forward(z2, label)
    dz2 = fc.softmax_loss_backward(prob, label, 1.0)
    dw2, db2, dd = dev(inp["w2_diff0"]), dev(inp["b2_diff0"]), torch.empty_like(d)
    fc.inner_product_backward(d, w2, dz2, dw2, db2, dd)
    dz1 = pool.tanh_backward(h, dropout.dropout_backward(dd, ratio, seed, seq, train=train))
    dw1, db1, dfeat = dev(inp["w1_diff0"]), dev(inp["b1_diff0"]), torch.empty_like(feat)
    fc.inner_product_backward(feat, w1, dz1, dw1, db1, dfeat)
    dx0, dx1 = fc.concat_backward(dfeat, [x0.shape, x1.shape])
    # the head
    kw = dict(phase=phase, dropout_ratio=ratio, normalization=H.VALID)
    hh, hprob, hloss = head.head_forward_generic(x0, x1, w1, b1, mask, w2, b2, label, **kw)
    want = dict(x0_diff=torch.empty_like(x0), x1_diff=torch.empty_like(x1), w1_diff=dev(inp["w1_diff0"]),
                b1_diff=dev(inp["b1_diff0"]), w2_diff=dev(inp["w2_diff0"]), b2_diff=dev(inp["b2_diff0"]))
    head.head_backward_generic(x0, x1, w1, w2, mask, hh, hprob, label, 1.0, **want, **kw)
    got = dict(h=h, prob=prob, loss=loss, x0_diff=dx0, x1_diff=dx1, w1_diff=dw1, b1_diff=db1, w2_diff=dw2, b2_diff=db2)
    want.update(h=hh, prob=hprob, loss=hloss)
    words = {}
    for k in got:
        close(got[k], host(want[k]), TOL, k)
        words[k] = bool((host(got[k]).view(np.uint32) == host(want[k]).view(np.uint32)).all())
    print("words coincide:", words)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_four_bottom_chain(fc, dtype):
    """The SimMatrix net: Concat(flt_q 100, flt_a 100, sim 1, overlap_feat 4) -> InnerProduct(64), and its backward."""
    N, ext = 50, (100, 100, 1, 4)
    r = np.random.default_rng(SEED)
    bottoms = [r.uniform(-1, 1, (N, e)).astype(dtype) for e in ext]
    d = R.ip_dense(N, sum(ext), 64, dtype, SEED)
    feat_want = R.concat_forward([b[:, :, None] for b in bottoms])[:, :, 0]
    feat = fc.concat_forward([dev(b) for b in bottoms])
    same_words(feat, feat_want, "feat")
    w, b, td = dev(d["w"]), dev(d["b"]), dev(d["td"])
    close(fc.inner_product_forward(feat, w, b), R.ip_forward(feat_want, d["w"], d["b"]), TOLS[dtype], "top")
    dw, db, dfeat = dev(d["w_diff0"]), dev(d["b_diff0"]), torch.empty_like(feat)
    fc.inner_product_backward(feat, w, td, dw, db, dfeat)
    want = R.ip_backward(feat_want, d["w"], d["td"], False, d["w_diff0"], d["b_diff0"])
    close(dw, want[0], TOLS[dtype], "w_diff")
    close(db, want[1], TOLS[dtype], "b_diff")
    close(dfeat, want[2], TOLS[dtype], "feat diff")
    diffs = fc.concat_backward(dfeat, [b.shape for b in bottoms])
    for g, wnt in zip(diffs, R.concat_backward(host(dfeat)[:, :, None], ext)):
        same_words(g, wnt[:, :, 0], "a bottom diff")
