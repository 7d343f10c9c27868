"""The fp32 word-grid SimCross (csrc/simcross_cross.hip, csrc/cross_acc.h; dist_mode 0 and 1) on every kernel instantiation and on both
sides of every routing threshold.  tests/cross_grid_model.py has the routing, the shapes and the inputs; tests/test_cross_grid_model.py
proves on the CPU which launch each shape takes.

 forward   cross_fwd_kernel<float, rj, rk, MODE> for every rj, rk in 1..5 (GENERIC_TILES: ragged widths, chunks of 3, 8, 32 + 1, 32 + 2),
           cross_fwd_image_kernel<float, j, k, MODE, 50> for every j, k in 1..5 (IMAGE_TILES, odd and even N); the same shapes with q and a one
           float off a 16-byte boundary (the image declines: cross_fwd_kernel<float, j, k> on whole tiles); N, D and W1 next to the image's
           conditions (FWD_EDGES); all of them through the Embed-fused call's gathering loads, with and without the Embed bias.
           Euclid: the oracle's words.  Cosine: top, norm0, norm1 at the dense bar of tests/test_gpu_cosine_accuracy.py.
 backward  BWD in both euclid_backward_modes: cross_bwd_lane_kernel<W2, true> and <W2, false, 2> at all seven widths, D below the
           wave, one row of q; cross_bwd_tiled_kernel<float, 1, true> and <1, false> split and unsplit; cross_bwd_plain_kernel<float, 1>.  Reference
           rounding: the oracle's words from simcross_backward and simcross_forward_backward.  fp32 arithmetic: the bound of
           tests/test_gpu_bwd_modes.py (cross_grid_model.assert_fp32_mode).  One shape per route again with every operand one float off
           a 16-byte boundary.
 edges     EDGE_PAIRS: a case and its extension by one pair, one row or one column take different kernels; what they share carries
           the same words.
Every output sits between two zones of sentinel words and starts as NaN; every input is read back unchanged.  In pair 1 and in the last
pair the last row of a is the last row of q (T = 1, the divisor 1e-9): a remainder lane of the last tile owns that output.
"""
import numpy as np
import pytest
import torch

import cosine_model as cm
import cross_grid_model as gm
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
PAD = 64          # floats on each side of an output: keeps the output's own alignment


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output allocated inside a larger buffer filled with a sentinel, itself filled with NaN; off: floats of misalignment."""

    def __init__(self, shape, off=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lo = PAD + off
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        self.t.fill_(float("nan"))
        self.n = n
        assert self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        b = host(self.buf)
        return bool((b[:self.lo] == np.float32(SENTINEL)).all() and (b[self.lo + self.n:] == np.float32(SENTINEL)).all())


class Call:
    """The operands of one call: inputs on the device `off` floats past a 16-byte boundary, outputs guarded (dq and da `off` floats
    past one as well).  finish() checks the guards, that only `names` were written and that every input still holds its words."""

    def __init__(self, shape, what, off=0, **inputs):
        N, W1, W2, D = shape
        self.what, self.src, self.inp = what, inputs, {}
        for k, x in inputs.items():
            if x is None:
                self.inp[k] = None
                continue
            buf = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
            self.inp[k] = buf[off:off + x.size].view(*x.shape)
            self.inp[k].copy_(torch.from_numpy(np.array(x, copy=True, order="C")))
            assert self.inp[k].data_ptr() % 16 == 4 * off
        self.out = dict(top=Guarded((N, 1, W1, W2)), n0=Guarded((N, W1)), n1=Guarded((N, W2)), dq=Guarded((N, W1, D), off),
                        da=Guarded((N, W2, D), off))

    def finish(self, names):
        torch.cuda.synchronize()
        for k, g in self.out.items():
            assert g.intact(), "%s: a store landed outside %s" % (self.what, k)
        for k in set(self.out) - set(names):
            assert np.isnan(host(self.out[k].t)).all(), "%s: %s was written by a call that does not own it" % (self.what, k)
        for k, x in self.src.items():
            if x is not None:
                assert_bitexact(host(self.inp[k]), x, "%s: input %s after the call" % (self.what, k))
        return {k: host(self.out[k].t).copy() for k in names}


def shape_of(q, a):
    return (q.shape[0], q.shape[1], a.shape[1], q.shape[2])


def forward(capi, mode, q, a, what, off=0):
    c = Call(shape_of(q, a), what + " forward", off, q=q, a=a)
    n = dict(norm0=c.out["n0"].t, norm1=c.out["n1"].t) if mode == 0 else {}
    capi.simcross_forward(mode, c.inp["q"], c.inp["a"], c.out["top"].t, **n)
    return c.finish(("top", "n0", "n1") if mode == 0 else ("top",))


def backward(capi, q, a, top, dT, what, off=0):
    c = Call(shape_of(q, a), what + " backward", off, q=q, a=a, top=top, dT=dT)
    capi.simcross_backward(1, c.inp["q"], c.inp["a"], c.inp["top"], c.inp["dT"], c.out["dq"].t, c.out["da"].t)
    return c.finish(("dq", "da"))


def fused(capi, q, a, dT, what, off=0):
    c = Call(shape_of(q, a), what + " forward_backward", off, q=q, a=a, dT=dT)
    capi.simcross_forward_backward(1, c.inp["q"], c.inp["a"], c.inp["dT"], c.out["top"].t, c.out["dq"].t, c.out["da"].t)
    return c.finish(("top", "dq", "da"))


def assert_same(got, want, names, what):
    for k in names:
        assert_bitexact(got[k], want[k], "%s: %s" % (what, k))


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def routes(shape):
    return "%s, off a 16-byte boundary %s" % (gm.fwd_route(*shape), gm.fwd_route(*shape, aligned=False))


@pytest.mark.parametrize("shape", gm.FWD, ids=gm.shape_id)
def test_euclid_forward_is_the_oracles_words(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "euclid %s (%s)" % (shape, routes(shape))
    c = gm.forward_case(oracle, 1, shape)
    assert c["top"][1, 0, -1, -1] == 1.0 and c["top"][-1, 0, -1, -1] == 1.0
    fw = forward(capi, 1, c["q"], c["a"], what)
    assert_bitexact(fw["top"], c["top"], what + ": top against the oracle")
    off = forward(capi, 1, c["q"], c["a"], what + ", q and a + 4 bytes", off=1)
    assert_bitexact(off["top"], c["top"], what + ", q and a + 4 bytes: top against the oracle")


def check_cosine_forward(c, got, what):
    """The bar of tests/test_gpu_cosine_accuracy.py::test_dense_error_within_twice_the_references: the kernel's scaled error against
    fp64 (cosine_model.scaled_error) at most cosine_model.dense_bar of the CPU oracle's own; top at the scale sum |q_i a_i| / (n0 n1),
    the norms relative."""
    fails = []
    for k in ("top", "n0", "n1"):
        ek, idx = cm.scaled_error(got[k], *c["ref"][k])
        eo = c["e_o"][k]
        msg = "%s %s: e(kernel) = %.2f, e(oracle) = %.2f, bar %.2f (x 2^-24), worst at %s" % (what, k, ek / cm.U24, eo / cm.U24, cm.dense_bar(eo) / cm.U24, idx)
        print(msg)
        if not ek <= cm.dense_bar(eo):
            fails.append(msg)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("shape", gm.FWD, ids=gm.shape_id)
def test_cosine_forward_at_the_dense_bar(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "cosine %s (%s)" % (shape, routes(shape))
    c = gm.forward_case(oracle, 0, shape)
    fw = forward(capi, 0, c["q"], c["a"], what)
    check_cosine_forward(c, fw, what)
    off = forward(capi, 0, c["q"], c["a"], what + ", q and a + 4 bytes", off=1)
    check_cosine_forward(c, off, what + ", q and a + 4 bytes")
    # both kernels run CrossAcc's d-ascending sums behind the same row_norm_kernel
    assert_same(off, fw, ("top", "n0", "n1"), what + ": q and a + 4 bytes against aligned")


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", gm.FWD, ids=gm.shape_id)
def test_embed_fused_forward_is_the_oracles_words(shape, bias, oracle, hiplib):
    """mms_embed_simcross_forward_f32, mode 1: rowoff[] and the gathering loads of cross_fwd_kernel, the float2 gather of
    cross_fwd_image_kernel (ids clamped separately for q and a where W1 != W2), the Embed bias added in one rounding."""
    from mms_answer_selection_amd import capi
    what = "embed + euclid %s bias=%s (%s)" % (shape, bias, gm.fwd_route(*shape))
    c = gm.embed_case(oracle, shape, bias)
    assert c["top"][1, 0, -1, -1] == 1.0 and c["top"][-1, 0, -1, -1] == 1.0
    call = Call(shape, what, iq=c["iq"], ia=c["ia"], table=c["table"], bias=c["bias"])
    capi.embed_simcross_forward(1, call.inp["iq"], call.inp["ia"], call.inp["table"], call.out["top"].t, embed_bias=call.inp["bias"])
    assert_bitexact(call.finish(("top",))["top"], c["top"], what + ": top against the oracle on the gathered blobs")


# ----------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------
_budgets = {}


def budget(c, key):
    if key not in _budgets:
        _budgets[key] = gm.term_budget(c["q"], c["a"], c["top"], c["dT"])
    return _budgets[key]


def run_backward(capi, c, what, off=0):
    """Forward, backward from the library's own top, and the one-call sequence; top is the oracle's in all of them."""
    fw = forward(capi, 1, c["q"], c["a"], what, off)
    assert_bitexact(fw["top"], c["top"], what + ": top against the oracle")
    bw = backward(capi, c["q"], c["a"], fw["top"], c["dT"], what, off)
    fu = fused(capi, c["q"], c["a"], c["dT"], what, off)
    assert_bitexact(fu["top"], c["top"], what + ": fused top against the oracle")
    return bw, fu


@pytest.mark.parametrize("mode", ["reference", "fp32"])
@pytest.mark.parametrize("shape", list(gm.BWD), ids=gm.shape_id)
def test_euclid_backward(shape, mode, oracle, hiplib):
    from mms_answer_selection_amd import capi
    exact = mode == "reference"
    route = gm.BWD[shape][0 if exact else 1]
    what = "euclid %s %s %s" % (mode, shape, route)
    c = gm.backward_case(oracle, shape)
    capi.set_euclid_backward_mode(mode)
    try:
        assert capi.get_euclid_backward_mode() == mode
        bw, fu = run_backward(capi, c, what)
        again = run_backward(capi, c, what + ", every operand + 4 bytes", off=1) if shape in gm.one_per_route(exact) else None
    finally:
        capi.set_euclid_backward_mode("reference")
    assert_same(fu, bw, ("dq", "da"), what + ": forward_backward against forward, then backward")
    if exact:
        assert_same(bw, c, ("dq", "da"), what + " against the oracle")
    else:
        mag_q, mag_a = budget(c, shape)
        gm.assert_fp32_mode(bw["dq"], c["dq"], mag_q)
        gm.assert_fp32_mode(bw["da"], c["da"], mag_a)
    if again is not None:
        assert_same(again[0], bw, ("dq", "da"), what + ": every operand + 4 bytes, backward")
        assert_same(again[1], bw, ("dq", "da"), what + ": every operand + 4 bytes, forward_backward")


@pytest.mark.parametrize("small,large,axis", gm.EDGE_PAIRS, ids=["%s-%s" % (gm.shape_id(s), gm.shape_id(l)) for s, l, _ in gm.EDGE_PAIRS])
def test_routing_edges_share_their_words(small, large, axis, oracle, hiplib):
    """Reference rounding.  The larger case is the smaller one with one more pair, one more row of q (top_diff 0 there) or one more
    column (q - a = 0 there): top, dq and da of the smaller case are a sub-block of the larger one's, word for word, although the
    two calls take the kernels of gm.BWD[small] and gm.BWD[large]."""
    from mms_answer_selection_amd import capi
    what = "%s %s | %s %s" % (small, gm.BWD[small][0], large, gm.BWD[large][0])
    assert capi.get_euclid_backward_mode() == "reference"
    cs, cl = gm.backward_case(oracle, small), gm.backward_case(oracle, large, extend=(small, axis))
    N, W1, W2, D = small
    (bs, fs), (bl, fl) = run_backward(capi, cs, what + ", smaller"), run_backward(capi, cl, what + ", larger")
    assert_same(bs, cs, ("dq", "da"), what + ", smaller, against the oracle")
    assert_same(bl, cl, ("dq", "da"), what + ", larger, against the oracle")
    assert_bitexact(fl["top"][:N, :, :W1], fs["top"], what + ": top of the shared block")
    for got in (bl, fl):
        assert_bitexact(got["dq"][:N, :W1, :D], bs["dq"], what + ": dq of the shared block")
        assert_bitexact(got["da"][:N, :, :D], bs["da"], what + ": da of the shared block")
