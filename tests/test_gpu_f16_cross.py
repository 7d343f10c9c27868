"""The fp16-storage word-grid calls (mms_simcross_forward_f16, mms_simcross_backward_f16, mms_simcross_forward_backward_f16;
csrc/simcross_cross_f16.hip) on every kernel instantiation: the Euclid forward and the reference-rounding backward bit for bit, the
default backward mode and the cosine gradients held to the half bracket, exact-sum probes, the fused call, edge inputs, guard bands and
refusals.  tests/f16_cross_model.py has the routing, the shapes, the references and the bars; tests/test_f16_cross_model.py proves them
on the CPU.  Every output sits inside a sentinel-filled buffer and starts as NaN.

Route table, (N, W1, W2, D) -> launch, read off launch_cross_fwd<_Float16> / cross_backward<_Float16> (MODE 0 cosine, 1 Euclid, both run):
 forward
  (   3,  5,  7, 50)  cross_fwd_kernel<_Float16, 1, 1>: one ragged tile, 100-byte rows
  (   2,  9, 17, 33)  cross_fwd_kernel<_Float16, 1, 1>: 2 x 3 ragged tiles, odd D, a chunk of one d, rows only 2-byte aligned
  (1024, 40, 40,  8)  cross_fwd_kernel<_Float16, 5, 5>          (1024, 40, 24, 34)  cross_fwd_kernel<_Float16, 5, 3>: accq and accs of CrossAcc
  (1024, 24, 40, 50)  cross_fwd_image_kernel<_Float16, 3, 5>    (1025,  8,  8, 50)  cross_fwd_image_kernel<_Float16, 1, 1>, last workgroup one wave
  (1024, 24, 40, 50), q one half past a 16-byte boundary: cross_fwd_kernel<_Float16, 3, 5>, the image kernel's bits
  f16_cross_model.GENERIC_TILES: cross_fwd_kernel<_Float16, rj, rk> for every rj, rk in 1..5 (N = 1024, ragged widths, D in 3, 8, 33, 34)
  f16_cross_model.IMAGE_TILES:   cross_fwd_image_kernel<_Float16, J, K> for every J, K in 1..5 (N = 1024, D = 50)
  cosine: row_norm_kernel<_Float16> twice in front of either
 backward: cross_bwd_tiled_kernel<_Float16, 0, true> (cosine), <1, true> (Euclid, reference rounding), <1, false> (Euclid, fp32 arithmetic)
  (   3,  5,  7, 50)  tiled, split        (  2,  9, 17, 33)  tiled, split, a chunk of one d      (70, 40, 40, 50)  tiled, split
  ( 512, 16, 24, 50)  tiled, not split    (  2, 12, 20, 70)  tiled, split, three chunks
  (   2, 60, 60, 16)  cross_bwd_plain_kernel<_Float16, MODE>: the tables exceed 64 KB
"""
import ctypes

import numpy as np
import pytest
import torch

import cosine_model as cm
import f16_cross_model as xm
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
SENTINEL16 = -1234.0        # exact as a half
PAD = 64                    # elements on each side of an output: a multiple of 8 halves, so the output keeps its alignment
OK, INVALID_ARG, UNSUPPORTED = xm.OK, xm.INVALID_ARG, xm.UNSUPPORTED
H = torch.float16


def dev(x, off=0):
    """x on the device; off: halves past a 16-byte boundary."""
    x = np.ascontiguousarray(x)
    if not off:
        return torch.from_numpy(np.array(x, copy=True)).cuda()
    buf = torch.zeros(x.size + 8, dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + x.size].view(*x.shape)
    t.copy_(torch.from_numpy(np.array(x, copy=True)))
    return t


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output allocated inside a larger buffer filled with a sentinel and itself filled with NaN; off: elements of misalignment."""

    def __init__(self, shape, dtype=torch.float32, off=0):
        n = int(np.prod(shape))
        self.sentinel = SENTINEL if dtype == torch.float32 else SENTINEL16
        self.buf = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype, device="cuda")
        self.lo = PAD + off
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        self.t.fill_(float("nan"))
        self.n = n

    def intact(self):
        b = host(self.buf)
        s = b.dtype.type(self.sentinel)
        return bool((b[:self.lo] == s).all() and (b[self.lo + self.n:] == s).all())

    def untouched(self):
        return self.intact() and bool(np.isnan(host(self.t)).all())


def outputs(shape, dtype=H, off=0):
    N, W1, W2, D = shape
    return dict(top=Guarded((N, 1, W1, W2)), n0=Guarded((N, W1)), n1=Guarded((N, W2)), dq=Guarded((N, W1, D), dtype, off),
                da=Guarded((N, W2, D), dtype, off))


def finish(out, names, what):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside %s" % (what, k)
    for k in set(out) - set(names):
        assert np.isnan(host(out[k].t)).all(), "%s: %s was written by a call that does not own it" % (what, k)
    return {k: host(out[k].t).copy() for k in names}


def shape_of(qh, ah):
    return (qh.shape[0], qh.shape[1], ah.shape[1], qh.shape[2])


def fwd_names(mode):
    return ("top", "n0", "n1") if mode == 0 else ("top",)


def norms(mode, out):
    return dict(norm0=out["n0"].t, norm1=out["n1"].t) if mode == 0 else {}


def forward16(capi, mode, qh, ah, what, q_off=0):
    out = outputs(shape_of(qh, ah))
    capi.simcross_forward_f16(mode, dev(qh, q_off), dev(ah), out["top"].t, **norms(mode, out))
    return finish(out, fwd_names(mode), what + " forward_f16")


def backward16(capi, mode, qh, ah, fw, dT, what, off=0):
    """mms_simcross_backward_f16 from the forward `fw` (top and, for cosine, the norms)."""
    out = outputs(shape_of(qh, ah), off=off)
    n = dict(norm0=dev(fw["n0"]), norm1=dev(fw["n1"])) if mode == 0 else {}
    capi.simcross_backward_f16(mode, dev(qh), dev(ah), dev(fw["top"]), dev(dT), out["dq"].t, out["da"].t, **n)
    return finish(out, ("dq", "da"), what + " backward_f16")


def fused16(capi, mode, qh, ah, dT, what):
    out = outputs(shape_of(qh, ah))
    capi.simcross_forward_backward_f16(mode, dev(qh), dev(ah), dev(dT), out["top"].t, out["dq"].t, out["da"].t, **norms(mode, out))
    return finish(out, fwd_names(mode) + ("dq", "da"), what + " forward_backward_f16")


def forward32(capi, mode, q32, a32, what):
    out = outputs(shape_of(q32, a32), torch.float32)
    capi.simcross_forward(mode, dev(q32), dev(a32), out["top"].t, **norms(mode, out))
    return finish(out, fwd_names(mode), what + " forward_f32")


def fused32(capi, mode, q32, a32, dT, what):
    out = outputs(shape_of(q32, a32), torch.float32)
    capi.simcross_forward_backward(mode, dev(q32), dev(a32), dev(dT), out["top"].t, out["dq"].t, out["da"].t, **norms(mode, out))
    return finish(out, fwd_names(mode) + ("dq", "da"), what + " forward_backward_f32")


def assert_halves(got, want, what):
    """uint16 for uint16; NaNs match NaNs."""
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, what
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d halves differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def assert_same(got, want, names, what):
    for k in names:
        (assert_halves if got[k].dtype == np.float16 else assert_bitexact)(got[k], want[k].reshape(got[k].shape), "%s: %s" % (what, k))


def to_half(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def check_against_fp64(c, got, names, what):
    """fp32 outputs within dense_bar(e_o) of fp64 over the finite elements; the non-finite ones are the oracle's, element for element."""
    fails = []
    for k in names:
        ref64, scale = c["ref"][k]
        g = got[k].reshape(ref64.shape)
        o = c[k].reshape(g.shape)
        fin = np.isfinite(ref64) & np.isfinite(scale)
        assert (np.isnan(g) == np.isnan(o)).all() and (np.isinf(g) == np.isinf(o)).all(), "%s %s: the NaNs / Infs are not where the oracle has them" % (what, k)
        assert np.isfinite(g[fin]).all(), "%s %s: a finite element came out non-finite" % (what, k)
        ek = cm.scaled_error(g[fin], ref64[fin], scale[fin])[0] if fin.any() else 0.0
        msg = "%s %s: e(kernel) = %.2f, e(oracle) = %.2f, bar %.2f (x 2^-24)" % (what, k, ek / cm.U24, c["e_o"][k] / cm.U24, cm.dense_bar(c["e_o"][k]) / cm.U24)
        print(msg)
        if not ek <= cm.dense_bar(c["e_o"][k]):
            fails.append(msg)
    assert not fails, "; ".join(fails)


def check_gradients(got, refs, bars, what, pinned=True):
    """dq, da inside the half bracket around refs = ((dq64, scale), (da64, scale)) at bars = (b_dq, b_da)."""
    for k, (ref64, scale), b in zip(("dq", "da"), refs, bars):
        lo, hi = xm.check_bracket("%s %s" % (what, k), got[k], ref64, scale, b)
        share = xm.pinned_share(lo, hi)
        print("%s %s: inside the bracket, b = %.2f x 2^-24, pinned %.3f %%" % (what, k, b / cm.U24, 100 * share))
        if pinned:
            assert share >= xm.PINNED_MIN, "%s %s: only %.2f %% of the elements are pinned to one half" % (what, k, 100 * share)


# ----------------------------------------------------------------------------------------------------------------------
# 1. Euclid forward: bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.FWD, ids=xm.shape_id)
def test_euclid_forward_bit_for_bit(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "euclid %s" % (shape,)
    c = xm.forward_case(oracle, 1, shape)
    fw = forward16(capi, 1, c["qh"], c["ah"], what)
    assert_bitexact(fw["top"], c["top"], what + ": top against the oracle on the widened inputs")
    assert_same(fw, forward32(capi, 1, c["q"], c["a"], what), ("top",), what + " against the fp32 call")
    assert_same(forward16(capi, 1, c["qh"], c["ah"], what), fw, ("top",), what + ": second call")


@pytest.mark.parametrize("mode", [0, 1])
def test_misaligned_q_falls_back_from_the_image_kernel(mode, oracle, hiplib):
    """q one half past a 16-byte boundary: the generic kernel serves the call (alignment never refuses) with the image kernel's bits."""
    from mms_answer_selection_amd import capi
    what = "mode %d %s, q + 2 bytes" % (mode, xm.MISALIGNED)
    c = xm.forward_case(oracle, mode, xm.MISALIGNED)
    aligned = forward16(capi, mode, c["qh"], c["ah"], what)
    assert_same(forward16(capi, mode, c["qh"], c["ah"], what, q_off=1), aligned, fwd_names(mode), what)
    assert_same(aligned, c, fwd_names(mode), what + " against the oracle")


# ----------------------------------------------------------------------------------------------------------------------
# 2. Euclid backward, reference rounding: the oracle's halves
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_euclid_backward_reference_rounding_is_the_oracles_halves(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    assert capi.get_euclid_backward_mode() == "reference"
    what = "euclid reference %s" % (shape,)
    c = xm.backward_case(oracle, 1, shape, "dense")
    bw = backward16(capi, 1, c["qh"], c["ah"], c, c["dT"], what)
    assert_halves(bw["dq"], to_half(c["dq"]), what + ": dq against the oracle's halves")
    assert_halves(bw["da"], to_half(c["da"]), what + ": da against the oracle's halves")
    assert_same(backward16(capi, 1, c["qh"], c["ah"], c, c["dT"], what), bw, ("dq", "da"), what + ": second call")
    # dq / da one half past a 4-byte boundary: every packed store falls back, the same halves
    assert_same(backward16(capi, 1, c["qh"], c["ah"], c, c["dT"], what, off=1), bw, ("dq", "da"), what + ": dq, da + 2 bytes")


# ----------------------------------------------------------------------------------------------------------------------
# 3. Euclid backward, default mode: the half brackets
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_euclid_backward_default_mode_in_the_half_brackets(shape, oracle, hiplib):
    """f16_cross_model: (a) the bracket of the bar tests/test_gpu_parity.py holds the fp32 backward to in this mode, around the
    oracle's gradient; (b) the bracket around the fp64 gradient from the stored top at dense_bar(e_o) + 4 x 2^-24 of sum |tt|, which
    pins at least 99 % of the elements."""
    from mms_answer_selection_amd import capi
    what = "euclid fp32 arithmetic %s" % (shape,)
    c = xm.backward_case(oracle, 1, shape, "aligned")
    before = capi.get_euclid_backward_mode()
    capi.set_euclid_backward_mode("fp32")
    try:
        bw = backward16(capi, 1, c["qh"], c["ah"], c, c["dT"], what)
        again = backward16(capi, 1, c["qh"], c["ah"], c, c["dT"], what)
        fu = fused16(capi, 1, c["qh"], c["ah"], c["dT"], what)
    finally:
        capi.set_euclid_backward_mode(before)
    assert_same(again, bw, ("dq", "da"), what + ": second call")
    assert_bitexact(fu["top"], c["top"], what + ": fused top")
    assert_same(fu, bw, ("dq", "da"), what + ": fused against forward, then backward")
    for k in ("dq", "da"):
        xm.check_bracket("%s %s, parity bar" % (what, k), bw[k], *xm.parity_bracket(c, k))
    check_gradients(bw, xm.euclid_grad_ref(c, c["top"]), (xm.term_bar(c, "dq"), xm.term_bar(c, "da")), what)


# ----------------------------------------------------------------------------------------------------------------------
# 4. cosine, exact-sum probes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.FWD, ids=xm.shape_id)
def test_cosine_probe_bit_for_bit(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "cosine probe %s" % (shape,)
    c = xm.forward_case(oracle, 0, shape)
    fw = forward16(capi, 0, c["qh"], c["ah"], what)
    assert_same(fw, c, ("top", "n0", "n1"), what + " against the oracle")
    assert_same(fw, forward32(capi, 0, c["q"], c["a"], what), ("top", "n0", "n1"), what + " against the fp32 call")
    assert_same(forward16(capi, 0, c["qh"], c["ah"], what), fw, ("top", "n0", "n1"), what + ": second call")


# ----------------------------------------------------------------------------------------------------------------------
# 5. cosine, dense
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_cosine_dense_against_fp64(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "cosine %s" % (shape,)
    c = xm.backward_case(oracle, 0, shape, "aligned")
    fu = fused16(capi, 0, c["qh"], c["ah"], c["dT"], what)
    check_against_fp64(c, fu, ("top", "n0", "n1"), what)
    check_gradients(fu, xm.cosine_grad_ref(c, fu["top"], fu["n0"], fu["n1"]), (cm.dense_bar(c["e_o"]["dq"]), cm.dense_bar(c["e_o"]["da"])), what)
    # 6. the fused call is the forward, then the backward
    fw = forward16(capi, 0, c["qh"], c["ah"], what)
    assert_same(fw, fu, ("top", "n0", "n1"), what + ": forward against fused")
    assert_same(backward16(capi, 0, c["qh"], c["ah"], fw, c["dT"], what), fu, ("dq", "da"), what + ": forward, then backward against fused")
    assert_same(fused16(capi, 0, c["qh"], c["ah"], c["dT"], what), fu, ("top", "n0", "n1", "dq", "da"), what + ": second fused call")


# ----------------------------------------------------------------------------------------------------------------------
# 6. the fused call, Euclid, reference rounding
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_euclid_fused_is_forward_then_backward(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "euclid fused %s" % (shape,)
    c = xm.backward_case(oracle, 1, shape, "dense")
    fu = fused16(capi, 1, c["qh"], c["ah"], c["dT"], what)
    fw = forward16(capi, 1, c["qh"], c["ah"], what)
    assert_same(fw, fu, ("top",), what + ": forward against fused")
    assert_same(backward16(capi, 1, c["qh"], c["ah"], fw, c["dT"], what), fu, ("dq", "da"), what + ": forward, then backward against fused")
    assert_bitexact(fu["top"], c["top"], what + ": top against the oracle")
    assert_halves(fu["dq"], to_half(c["dq"]), what + ": dq against the oracle's halves")


# ----------------------------------------------------------------------------------------------------------------------
# 7. edge inputs
# ----------------------------------------------------------------------------------------------------------------------
def test_euclid_edges(oracle, hiplib):
    """f16_cross_model.edge_inputs: wherever the oracle is finite its bits (top) and its halves (dq, da, Inf where the half
    overflows); elsewhere NaN for NaN and Inf for Inf like the fp32 call."""
    from mms_answer_selection_amd import capi
    what = "euclid edges"
    c = xm.edge_case(oracle, 1)
    fu = fused16(capi, 1, c["qh"], c["ah"], c["dT"], what)
    k32 = fused32(capi, 1, c["q"], c["a"], c["dT"], what)
    for k in ("top", "dq", "da"):
        o = c[k].reshape(fu[k].shape)
        fin = np.isfinite(o)
        want = o if k == "top" else to_half(o)
        same = fu[k].view(np.uint32 if k == "top" else np.uint16) == want.view(np.uint32 if k == "top" else np.uint16)
        assert same[fin].all(), "%s %s: %d finite elements differ from the oracle, first at %s" % (
            what, k, int((~same[fin]).sum()), tuple(int(v) for v in np.argwhere(fin & ~same)[0]))
        g32 = k32[k] if k == "top" else to_half(k32[k])
        assert (np.isnan(fu[k]) == np.isnan(g32)).all() and (np.isposinf(fu[k]) == np.isposinf(g32)).all() and \
            (np.isneginf(fu[k]) == np.isneginf(g32)).all(), "%s %s: NaN / Inf positions differ from the fp32 call's" % (what, k)
    assert np.isinf(fu["dq"][2]).any() and not np.isnan(fu["dq"][2]).any(), "top_diff 1e8 on a short distance overflows half"
    assert (np.diagonal(fu["top"][7, 0]) == 1.0).all() and not fu["dq"][4].any() and not fu["da"][4].any()
    assert not np.signbit(fu["dq"][4]).any() and not np.signbit(fu["da"][4]).any(), "top_diff == 0: 0 + (-0) is +0"


def test_cosine_edges(oracle, hiplib):
    """Zero rows (0 / 0), Inf, NaN, 65504-magnitude rows against subnormal ones: NaN and Inf in top and the norms where the oracle and
    the fp32 call have them; the finite ones at the dense bars; gradients inside the bracket, NaN where the fp32 call's are."""
    from mms_answer_selection_amd import capi
    what = "cosine edges"
    c = xm.edge_case(oracle, 0)
    fu = fused16(capi, 0, c["qh"], c["ah"], c["dT"], what)
    check_against_fp64(c, fu, ("top", "n0", "n1"), what)
    k32 = fused32(capi, 0, c["q"], c["a"], c["dT"], what)
    assert_same(fu, k32, ("top", "n0", "n1"), what + ": the forward against the fp32 call")
    check_gradients(fu, xm.cosine_grad_ref(c, fu["top"], fu["n0"], fu["n1"]), (cm.dense_bar(c["e_o"]["dq"]), cm.dense_bar(c["e_o"]["da"])), what,
                    pinned=False)
    for k in ("dq", "da"):
        assert (np.isnan(fu[k]) == np.isnan(k32[k])).all(), "%s %s: the NaNs are not where the fp32 call has them" % (what, k)
        assert (np.isnan(fu[k]) == np.isnan(c[k])).all(), "%s %s: the NaNs are not where the oracle has them" % (what, k)
    assert np.isnan(fu["top"][6, 0, 0]).all() and fu["n0"][6, 0] == 0 and fu["n1"][8, 4] == 0 and np.isinf(fu["dq"][4]).any()


# ----------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ----------------------------------------------------------------------------------------------------------------------
ENTRY = ["forward", "backward", "fused"]


def raw_call(capi, entry, mode, shape, t, out, null=()):
    """The C entry point itself: its return code.  null: arguments passed as NULL."""
    N, W1, W2, D = shape
    p = dict(q=t["q"].data_ptr(), a=t["a"].data_ptr(), dT=t["dT"].data_ptr(), top_in=t["top"].data_ptr(), n0_in=t["n0"].data_ptr(),
             n1_in=t["n1"].data_ptr(), top=out["top"].t.data_ptr(), n0=out["n0"].t.data_ptr(), n1=out["n1"].t.data_ptr(),
             dq=out["dq"].t.data_ptr(), da=out["da"].t.data_ptr())
    p = {k: (None if k in null else ctypes.c_void_p(v)) for k, v in p.items()}
    s = torch.cuda.current_stream().cuda_stream
    lib = capi.lib()
    if entry == "forward":
        return lib.mms_simcross_forward_f16(mode, N, W1, W2, D, p["q"], p["a"], p["top"], p["n0"], p["n1"], s)
    if entry == "backward":
        return lib.mms_simcross_backward_f16(mode, N, W1, W2, D, p["q"], p["a"], p["top_in"], p["dT"], p["n0_in"], p["n1_in"], p["dq"], p["da"], s)
    return lib.mms_simcross_forward_backward_f16(mode, N, W1, W2, D, p["q"], p["a"], p["dT"], p["top"], p["n0"], p["n1"], p["dq"], p["da"], s)


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_write_nothing(entry, hiplib):
    """dist_mode 2 and W1 == W2 == 1: MMS_ERR_UNSUPPORTED; an unknown mode, a negative or zero size, a NULL required pointer:
    MMS_ERR_INVALID_ARG; N == 0: MMS_OK; none of them writes anything.  The accepted call next to them writes only what it owns."""
    from mms_answer_selection_amd import capi
    big = (4, 5, 7, 50)                                                      # every operand is allocated for this
    t = dict(q=torch.full((4 * 5 * 50,), 0.5, dtype=H, device="cuda"), a=torch.full((4 * 7 * 50,), 0.25, dtype=H, device="cuda"),
             dT=torch.ones(4 * 35, device="cuda"), top=torch.full((4 * 35,), 0.5, device="cuda"), n0=torch.ones(4 * 5, device="cuda"),
             n1=torch.ones(4 * 7, device="cuda"))
    reads = dict(forward=("q", "a"), backward=("q", "a", "top_in", "dT"), fused=("q", "a", "dT"))[entry]
    writes = dict(forward=("top",), backward=("dq", "da"), fused=("top", "dq", "da"))[entry]
    norm_args = dict(forward=("n0", "n1"), backward=("n0_in", "n1_in"), fused=("n0", "n1"))[entry]

    def refused(mode, shape, code, **kw):
        out = outputs(big)
        assert raw_call(capi, entry, mode, shape, t, out, **kw) == code, (entry, mode, shape, kw)
        assert xm.refusal(mode, *shape) == code or kw, "the model's refusal disagrees"
        torch.cuda.synchronize()
        for k, g in out.items():
            assert g.untouched(), "%s mode %d %s %s: %s was written" % (entry, mode, shape, kw, k)

    for mode in (0, 1):
        refused(2, big, UNSUPPORTED)
        refused(mode, (4, 1, 1, 50), UNSUPPORTED)
        for shape in ((-1, 5, 7, 50), (4, 0, 7, 50), (4, 5, -7, 50), (4, 5, 7, 0), (4, -5, 7, 50)):
            refused(mode, shape, INVALID_ARG)
        refused(3, big, INVALID_ARG)
        refused(-1, big, INVALID_ARG)
        for which in reads + writes:
            refused(mode, big, INVALID_ARG, null=(which,))
        refused(mode, (0, 5, 7, 50), OK)
    for which in norm_args:
        refused(0, big, INVALID_ARG, null=(which,))                          # cosine: the norms are required
    # accepted: Euclid takes NULL norms; each mode writes only what it owns
    for mode, null in ((1, norm_args), (1, ()), (0, ())):
        out = outputs(big)
        assert raw_call(capi, entry, mode, big, t, out, null=null) == OK
        owns = writes + (("n0", "n1") if mode == 0 and entry != "backward" else ())
        got = finish(out, owns, "%s mode %d" % (entry, mode))
        assert all(np.isfinite(v).all() for v in got.values())


def test_wrappers_check_dtype_and_shape(hiplib):
    from mms_answer_selection_amd import capi
    q, a = torch.zeros((2, 3, 8), dtype=H, device="cuda"), torch.zeros((2, 4, 8), dtype=H, device="cuda")
    top = torch.zeros((2, 1, 3, 4), device="cuda")
    with pytest.raises(capi.MMSError):
        capi.simcross_forward_f16(1, q.float(), a, top)
    with pytest.raises(capi.MMSError):
        capi.simcross_forward_f16(1, q, a, torch.zeros((2, 1, 4, 3), device="cuda"))
    with pytest.raises(capi.MMSError):
        capi.simcross_backward_f16(1, q, a, top, top, torch.zeros_like(q).float(), torch.zeros_like(a))
    with pytest.raises(capi.MMSError):
        capi.simcross_forward_f16(2, q, a, top)
    capi.simcross_forward_f16(1, q, a, top)
    torch.cuda.synchronize()
    assert (host(top) == 1.0).all()
