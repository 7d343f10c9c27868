"""The fp16-storage bilinear word-grid calls (mms_simcross_bilinear_forward_f16, _backward_f16, _forward_backward_f16,
mms_embed_simcross_bilinear_forward_f16; csrc/bilinear_f16.hip, csrc/bilinear_pair.h) on every kernel instantiation.
tests/bilinear_f16_model.py has the routing, the shape table and the inputs; tests/test_bilinear_f16_model.py proves them on the CPU.

The reference is the fp32 entry point on the widened inputs in ordinary device tensors (tests/test_gpu_bilinear_grid_accuracy.py holds
that call to fp64 bars): top, dW, dbias 32-bit word for word, dq / da its gradients rounded once to half, 16-bit word for word.  One
case per route also goes against the CPU oracle.  Every output sits inside a sentinel-filled buffer and starts as NaN (dW: the NaN is
the sentinel an overwriting call must erase); the workspace is followed by a guard band.

Route table, (N, W1, W2, D, M, bias) -> launches:
  ( 512,  5,  7, 50, 2, yes)  bilinear_pair_fwd_kernel<13, half>, 4-byte staging loads; backward: widen, the fp32 layer, narrow
  ( 513, 40, 40, 52, 4, yes)  bilinear_pair_fwd_kernel<13, half>, 16-byte loads; q + 2 bytes: 2-byte loads, the same bits
  ( 512, 17, 33, 53, 1, no )  bilinear_pair_fwd_kernel<16, half>, 2-byte loads        (512, 48, 48, 64, 2, yes)  <16>, 16-byte loads
  (   3,  5,  7, 50, 4, yes)  bilinear_pairm_fwd_kernel<13, half>; bilinear_pair_bwd_kernel<10, 13, half, float> + the half reduction
  (   2, 40, 40, 52, 1, no )  pairm<13>; pair_bwd<10, 13, half, half>: the kernel stores dq / da        (1, 1, 2, 1, 1, yes) likewise
  (   2, 41,  9, 33, 2, yes)  pairm<13>; pair_bwd<12, 16, half, float> + reduction      (2, 48, 48, 64, 1, no)  pairm<16>; <12, 16, half, half>
  ( 256,  3,  2, 64, 2, yes)  pairm<16>; pair_bwd<12, 16, half, float> + reduction
  (3, 5, 7, 65, 2, yes), (2, 49, 3, 8, 1, no), (300, 5, 7, 50, 2, yes)  widen_pair_kernel, bilinear_forward / bilinear_backward, narrow_pair_kernel
"""
import ctypes

import numpy as np
import pytest
import torch

import bilinear_f16_model as bm
import bilinear_grid_model as gm
from util import TOL, assert_bitexact, assert_close

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
SENTINEL16 = -1234.0        # exact as a half
PAD = 64                    # elements on each side of an output: a multiple of 8 halves, so the output keeps its alignment
WS_GUARD = 512              # bytes behind the workspace
H = torch.float16
OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = bm.OK, bm.INVALID_ARG, bm.UNSUPPORTED, bm.WORKSPACE


def dev(x, off=0):
    """x on the device; off: elements past a 16-byte boundary."""
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    if not off:
        return torch.from_numpy(np.array(x, copy=True)).cuda()
    buf = torch.zeros(x.size + 8, dtype=torch.from_numpy(np.zeros(0, x.dtype)).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + x.size].view(*x.shape)
    t.copy_(torch.from_numpy(np.array(x, copy=True)))
    return t


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output inside a larger buffer filled with a sentinel; itself NaN, or `init`.  off: elements of misalignment."""

    def __init__(self, shape, dtype=torch.float32, off=0, init=None):
        n = int(np.prod(shape))
        self.sentinel = SENTINEL if dtype == torch.float32 else SENTINEL16
        self.buf = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype, device="cuda")
        self.lo = PAD + off
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(torch.from_numpy(np.array(init, copy=True)))
        self.n = n

    def intact(self):
        b = host(self.buf)
        s = b.dtype.type(self.sentinel)
        return bool((b[:self.lo] == s).all() and (b[self.lo + self.n:] == s).all())

    def untouched(self):
        return self.intact() and bool(np.isnan(host(self.t)).all())


class GuardedWs:
    """Exactly the bytes the library asks for, followed by a guard band (the `ws=` object of the capi wrappers)."""

    def __init__(self):
        self.buf, self.need = None, 0

    def get(self, nbytes, device):
        self.need = int(nbytes)
        self.buf = torch.full((self.need + WS_GUARD,), 0xA5, dtype=torch.uint8, device=device)
        return self.buf.data_ptr(), self.need

    def intact(self):
        return self.buf is None or bool((host(self.buf[self.need:]) == 0xA5).all())


def outputs(shape, off=0, dtype=H, dbias0=None):
    N, W1, W2, D, M, _ = shape
    return dict(top=Guarded((N, M, W1, W2)), dq=Guarded((N, W1, D), dtype, off), da=Guarded((N, W2, D), dtype, off),
                dW=Guarded((M, D, D)), dbias=Guarded((M, W1, W2), init=dbias0))


def finish(out, names, what, ws=None):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside %s" % (what, k)
    for k in set(out) - set(names) - {"dbias"}:
        assert np.isnan(host(out[k].t)).all(), "%s: %s was written by a call that does not own it" % (what, k)
    assert ws is None or ws.intact(), "%s: a store landed behind the workspace" % what
    return {k: host(out[k].t).copy() for k in names}


def bwd_names(c):
    return ("dq", "da", "dW") + (("dbias",) if c["bias"] is not None else ())


def forward16(capi, shape, what, q_off=0):
    c = bm.inputs(shape)
    out, ws = outputs(shape), GuardedWs()
    capi.simcross_bilinear_forward_f16(dev(c["qh"], q_off), dev(c["ah"]), dev(c["W"]), dev(c["bias"]), out["top"].t, ws=ws)
    return finish(out, ("top",), what + " forward_f16", ws)


def backward16(capi, shape, what, off=0, dT=None):
    c = bm.inputs(shape)
    out, ws = outputs(shape, off, dbias0=c["dbias0"]), GuardedWs()
    capi.simcross_bilinear_backward_f16(dev(c["qh"], off), dev(c["ah"]), dev(c["W"]), dev(c["dT"] if dT is None else dT), out["dq"].t,
                                        out["da"].t, out["dW"].t, out["dbias"].t if c["bias"] is not None else None, ws=ws)
    return finish(out, bwd_names(c), what + " backward_f16", ws)


def fused16(capi, shape, what):
    c = bm.inputs(shape)
    out, ws = outputs(shape, dbias0=c["dbias0"]), GuardedWs()
    capi.simcross_bilinear_forward_backward_f16(dev(c["qh"]), dev(c["ah"]), dev(c["W"]), dev(c["bias"]), dev(c["dT"]), out["top"].t,
                                                out["dq"].t, out["da"].t, out["dW"].t,
                                                out["dbias"].t if c["bias"] is not None else None, ws=ws)
    return finish(out, ("top",) + bwd_names(c), what + " forward_backward_f16", ws)


_ref32 = {}


def ref32(capi, shape, dT=None):
    """The fp32 entry point on the widened inputs, forward then backward: computed once per shape, shared read-only."""
    key = shape if dT is None else shape + ("scaled",)
    if key not in _ref32:
        c = bm.inputs(shape)
        out = outputs(shape, dtype=torch.float32, dbias0=c["dbias0"])
        qd, ad, Wd = dev(c["q"]), dev(c["a"]), dev(c["W"])
        capi.simcross_forward(2, qd, ad, out["top"].t, W=Wd, bias=dev(c["bias"]))
        capi.simcross_backward(2, qd, ad, out["top"].t, dev(c["dT"] if dT is None else dT), out["dq"].t, out["da"].t, W=Wd,
                               bias_term=c["bias"] is not None, dW=out["dW"].t, dbias=out["dbias"].t if c["bias"] is not None else None)
        r = finish(out, ("top",) + bwd_names(c), "fp32 call %s" % (shape,))
        for v in r.values():
            v.setflags(write=False)
        _ref32[key] = r
    return _ref32[key]


def to_half(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def assert_halves(got, want, what):
    """uint16 for uint16; NaNs match NaNs."""
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, what
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d halves differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def assert_same(got, want, names, what):
    for k in names:
        w = want[k] if want[k].dtype == got[k].dtype else to_half(want[k])
        (assert_halves if got[k].dtype == np.float16 else assert_bitexact)(got[k], w, "%s: %s" % (what, k))


# ----------------------------------------------------------------------------------------------------------------------
# 1, 2, 4, 5: the bits of the fp32 call
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bm.FWD, ids=bm.shape_id)
def test_forward_carries_the_fp32_calls_bits(shape, hiplib):
    from mms_answer_selection_amd import capi
    what = "%s fwd %s" % (shape, bm.fwd_route(*shape[:5]))
    fw = forward16(capi, shape, what)
    assert np.isfinite(fw["top"]).all()
    assert_same(fw, ref32(capi, shape), ("top",), what + " against the fp32 call")
    assert_same(forward16(capi, shape, what), fw, ("top",), what + ": second call")


@pytest.mark.parametrize("shape", bm.BWD, ids=bm.shape_id)
def test_backward_carries_the_fp32_calls_bits_and_its_halves(shape, hiplib):
    from mms_answer_selection_amd import capi
    what = "%s bwd %s" % (shape, bm.bwd_route(*shape[:5]))
    c, r = bm.inputs(shape), ref32(capi, shape)
    bw = backward16(capi, shape, what)
    assert all(np.isfinite(v).all() for v in bw.values()), what + ": dW's sentinel was not overwritten, or a gradient is not finite"
    assert_same(bw, r, bwd_names(c), what + " against the fp32 call")             # dq, da: fp32_call.half(); dW, dbias: its words
    if c["bias"] is not None:
        assert_bitexact(bw["dbias"], gm.dbias_in_order(c["dT"], c["dbias0"]), what + ": dbias = dT_n + dbias, n ascending")
    # the fused call gives the bits of the two calls
    fu = fused16(capi, shape, what)
    assert_same(fu, bw, bwd_names(c), what + ": fused against backward")
    assert_same(fu, forward16(capi, shape, what), ("top",), what + ": fused against forward")
    assert_same(backward16(capi, shape, what), bw, bwd_names(c), what + ": second call")


@pytest.mark.parametrize("shape", [bm.MISALIGNED_EVAL, bm.MISALIGNED_TRAIN], ids=bm.shape_id)
def test_misaligned_q_and_dq_give_the_aligned_bits(shape, hiplib):
    """q (and dq, da) one half past a 16-byte boundary, a aligned: the 2-byte staging path serves the call with the same bits."""
    from mms_answer_selection_amd import capi
    what = "%s, q + 2 bytes" % (shape,)
    assert bm.stage_width(shape[1], shape[2], shape[3]) == 8 and bm.stage_width(shape[1], shape[2], shape[3], q=2) == 1
    assert_same(forward16(capi, shape, what, q_off=1), forward16(capi, shape, what), ("top",), what)
    if bm.bwd_route(*shape[:5]) != ("generic",):
        c = bm.inputs(shape)
        assert_same(backward16(capi, shape, what, off=1), backward16(capi, shape, what), bwd_names(c), what)


# ----------------------------------------------------------------------------------------------------------------------
# 3: the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bm.ORACLE, ids=bm.shape_id)
def test_against_the_cpu_oracle(shape, oracle, hiplib):
    """top, dW at the suite's TOL; dq / da (halves) at 1e-3 of max(1, max |oracle|): half precision (include/mms.h states the same bar
    for mms_simmatrix_backward_f16)."""
    from mms_answer_selection_amd import capi
    what = "%s against the oracle" % (shape,)
    c = bm.inputs(shape)
    top_o, _, _ = oracle.simcross_forward(2, c["q"], c["a"], c["W"], c["bias"])
    dq_o, da_o, dW_o, db_o = oracle.simcross_backward(2, c["q"], c["a"], top_o, c["dT"], W=c["W"], bias_term=c["bias"] is not None,
                                                     dbias_in=c["dbias0"])
    fu = fused16(capi, shape, what)
    assert_close(fu["top"], top_o, TOL, what + ": top")
    assert_close(fu["dW"], dW_o, TOL, what + ": dW")
    for k, o in (("dq", dq_o), ("da", da_o)):
        err, scale = float(np.abs(fu[k].astype(np.float64) - o).max()), max(1.0, float(np.abs(o).max()))
        print("%s %s: max error %.3g of scale %.3g" % (what, k, err, scale))
        assert err <= 1e-3 * scale, "%s %s: %.3g > 1e-3 x %.3g" % (what, k, err, scale)
    if c["bias"] is not None:
        assert_bitexact(fu["dbias"], db_o, what + ": dbias")


# ----------------------------------------------------------------------------------------------------------------------
# 6: the Embed call
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["no_embed_bias", "embed_bias"])
@pytest.mark.parametrize("shape", bm.EMBED, ids=bm.shape_id)
def test_embed_call(shape, with_bias, hiplib):
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M, _ = shape
    what = "embed %s" % (shape,)
    c = bm.inputs(shape)
    table, iq, ia, ebias = bm.embed_inputs(shape)
    eb = ebias if with_bias else None
    out = outputs(shape)
    capi.embed_simcross_bilinear_forward_f16(dev(iq), dev(ia), dev(table), dev(c["W"]), dev(c["bias"]), out["top"].t, embed_bias=dev(eb))
    got = finish(out, ("top",), what + " f16")
    out = outputs(shape)
    capi.embed_simcross_bilinear_forward(dev(iq), dev(ia), dev(table.astype(np.float32)), dev(c["W"]), dev(c["bias"]), out["top"].t,
                                         embed_bias=dev(eb))
    assert_same(got, finish(out, ("top",), what + " f32"), ("top",), what + " against the fp32 twin on the widened table")
    assert np.isfinite(got["top"]).all()
    if not with_bias:
        out, ws = outputs(shape), GuardedWs()
        qh, ah = table[bm.clamp_ids(iq, bm.EMBED_K)], table[bm.clamp_ids(ia, bm.EMBED_K)]
        capi.simcross_bilinear_forward_f16(dev(qh), dev(ah), dev(c["W"]), dev(c["bias"]), out["top"].t, ws=ws)
        assert_same(got, finish(out, ("top",), what + " grid call", ws), ("top",), what + " against the f16 grid call on the gathered rows")


def test_embed_call_refuses_the_generic_geometry(hiplib):
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = bm.EMBED_UNSUPPORTED
    K = bm.EMBED_K
    out = Guarded((N, M, W1, W2))
    z = lambda *s: torch.zeros(s, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    table = torch.zeros((K, D), dtype=H, device="cuda")
    rc = capi.lib().mms_embed_simcross_bilinear_forward_f16(N, W1, W2, D, M, K, p(z(N, W1)), p(z(N, W2)), p(table), None, p(z(M, D, D)), None,
                                                           p(out.t), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED == bm.embed_refusal(N, W1, W2, D, M, K) and out.untouched()


# ----------------------------------------------------------------------------------------------------------------------
# 7: overflow
# ----------------------------------------------------------------------------------------------------------------------
def test_gradients_past_65504_are_infinite(hiplib):
    from mms_answer_selection_amd import capi
    shape = bm.OVERFLOW
    c = bm.inputs(shape)
    dT = np.ldexp(c["dT"], 16)
    r = ref32(capi, shape, dT)
    bw = backward16(capi, shape, "overflow", dT=dT)
    for k in ("dq", "da"):
        over = np.abs(r[k].astype(np.float64)) >= 65520.0          # the RNE boundary between 65504 and Inf
        assert over.any() and not over.all() and np.isfinite(r[k]).all(), "the case must hold both kinds of element"
        assert np.isinf(bw[k][over]).all() and (np.sign(bw[k][over]) == np.sign(r[k][over])).all()
        assert np.isfinite(bw[k][~over]).all()
        assert_halves(bw[k], to_half(r[k]), "overflow: %s" % k)
    assert_bitexact(bw["dW"], r["dW"], "overflow: dW")


# ----------------------------------------------------------------------------------------------------------------------
# 8: canaries (finish() checks every guard band and the workspace's)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bm.CANARY, ids=bm.shape_id)
def test_nothing_outside_the_outputs_or_past_the_workspace_changes(shape, hiplib):
    from mms_answer_selection_amd import capi
    what = "canary %s" % (shape,)
    c, r = bm.inputs(shape), ref32(capi, shape)
    for off in (0, 1):                           # dq, da inside their sentinel buffers, aligned and one half off
        fw = forward16(capi, shape, what, q_off=off)
        bw = backward16(capi, shape, what, off=off)
        assert_same(fw, r, ("top",), what)
        assert_same(bw, r, bwd_names(c), what)
    assert_same(fused16(capi, shape, what), r, ("top",) + bwd_names(c), what + " fused")


# ----------------------------------------------------------------------------------------------------------------------
# 9: refusals
# ----------------------------------------------------------------------------------------------------------------------
ENTRY = ["forward", "backward", "fused"]
BIG = (4, 5, 7, 50, 2)


def raw_call(capi, entry, shape, t, out, ws, ws_bytes, null=(), bias_term=1):
    """The C entry point itself: its return code.  null: arguments passed as NULL."""
    N, W1, W2, D, M = shape
    p = dict(q=t["q"], a=t["a"], W=t["W"], bias=t["bias"], dT=t["dT"], top=out["top"].t, dq=out["dq"].t, da=out["da"].t, dW=out["dW"].t,
             dbias=out["dbias"].t, ws=ws)
    p = {k: (None if k in null else ctypes.c_void_p(v.data_ptr())) for k, v in p.items()}
    s = torch.cuda.current_stream().cuda_stream
    lib = capi.lib()
    if entry == "forward":
        return lib.mms_simcross_bilinear_forward_f16(N, W1, W2, D, M, p["q"], p["a"], p["W"], p["bias"], p["top"], p["ws"], ws_bytes, s)
    if entry == "backward":
        return lib.mms_simcross_bilinear_backward_f16(N, W1, W2, D, M, p["q"], p["a"], p["W"], bias_term, p["dT"], p["dq"], p["da"], p["dW"],
                                                      p["dbias"], p["ws"], ws_bytes, s)
    return lib.mms_simcross_bilinear_forward_backward_f16(N, W1, W2, D, M, p["q"], p["a"], p["W"], p["bias"], p["dT"], p["top"], p["dq"],
                                                          p["da"], p["dW"], p["dbias"], p["ws"], ws_bytes, s)


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_write_nothing(entry, hiplib):
    """Bad sizes, M <= 0 and a NULL required pointer: MMS_ERR_INVALID_ARG; a workspace one byte short or missing: MMS_ERR_WORKSPACE;
    W1 == W2 == 1: MMS_ERR_UNSUPPORTED; N == 0: MMS_OK; none of them writes anything.  The accepted call next to them writes what it owns."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = BIG
    t = dict(q=torch.full((N * W1 * D,), 0.5, dtype=H, device="cuda"), a=torch.full((N * W2 * D,), 0.25, dtype=H, device="cuda"),
             W=torch.full((M * D * D,), 0.125, device="cuda"), bias=torch.ones(M * W1 * W2, device="cuda"),
             dT=torch.ones(N * M * W1 * W2, device="cuda"))
    need = capi.simcross_bilinear_workspace_bytes_f16(*BIG)
    wsbuf = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    required = dict(forward=("q", "a", "W", "top"), backward=("q", "a", "W", "dT", "dq", "da", "dW", "dbias"),
                    fused=("q", "a", "W", "top", "dT", "dq", "da", "dW", "dbias"))[entry]
    writes = dict(forward=("top",), backward=("dq", "da", "dW", "dbias"), fused=("top", "dq", "da", "dW", "dbias"))[entry]

    def refused(shape, code, ws_bytes=need, **kw):
        out = outputs(BIG + (True,))
        assert raw_call(capi, entry, shape, t, out, wsbuf, ws_bytes, **kw) == code, (entry, shape, ws_bytes, kw)
        assert bm.refusal(*shape) == code or kw or ws_bytes != need or shape[0] == 0, "the model's refusal disagrees"
        torch.cuda.synchronize()
        for k, g in out.items():
            assert g.untouched(), "%s %s %s: %s was written" % (entry, shape, kw, k)
        assert (host(wsbuf) == 0xA5).all(), "%s %s %s: the workspace was written" % (entry, shape, kw)

    for shape in ((-1, 5, 7, 50, 2), (4, 0, 7, 50, 2), (4, 5, -7, 50, 2), (4, 5, 7, 0, 2), (4, -5, 7, 50, 2), (4, 5, 7, 50, 0), (4, 5, 7, 50, -3)):
        refused(shape, INVALID_ARG)
    for which in required:
        refused(BIG, INVALID_ARG, null=(which,))
    refused(BIG, WORKSPACE, ws_bytes=need - 1)
    refused(BIG, WORKSPACE, null=("ws",))
    refused((4, 1, 1, 50, 1), UNSUPPORTED)
    refused((0, 5, 7, 50, 2), OK)
    # accepted: without a bias term bias / dbias may be NULL and dbias stays as it was; with one, everything owned is written
    for null in (("bias", "dbias"), ()):
        out = outputs(BIG + (True,), dbias0=np.full((M, W1, W2), 3.0, np.float32))
        assert raw_call(capi, entry, BIG, t, out, wsbuf, need, null=null, bias_term=0 if null else 1) == OK
        owns = tuple(k for k in writes if not (null and k == "dbias"))
        got = finish(out, owns, "%s accepted, null %s" % (entry, null))
        assert all(np.isfinite(v).all() for v in got.values())
        if null or entry == "forward":
            assert (host(out["dbias"].t) == 3.0).all(), "no bias term: dbias is not touched"
        else:
            assert (got["dbias"] == 3.0 + N).all(), "dbias += dT_n, n ascending"
        assert (host(wsbuf[need:]) == 0xA5).all()


# ----------------------------------------------------------------------------------------------------------------------
# 10: the capi wrappers
# ----------------------------------------------------------------------------------------------------------------------
def test_wrappers_check_dtype_and_shape(hiplib):
    from mms_answer_selection_amd import capi
    z = lambda *s, **k: torch.zeros(s, device="cuda", **k)
    q, a, W, top = z(2, 3, 8, dtype=H), z(2, 4, 8, dtype=H), z(2, 8, 8), z(2, 2, 3, 4)
    dq, da, dW = torch.zeros_like(q), torch.zeros_like(a), torch.zeros_like(W)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_forward_f16(q.float(), a, W, None, top)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_forward_f16(q, a, W, None, z(2, 2, 4, 3))
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_forward_f16(q, a, z(2, 8, 7), None, top)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_forward_f16(q, a, W, z(2, 4, 3), top)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_backward_f16(q, a, W, top, dq.float(), da, dW)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_backward_f16(q, a, W, top, dq, z(2, 3, 8, dtype=H), dW)
    with pytest.raises(capi.MMSError):
        capi.simcross_bilinear_forward_backward_f16(q, a, W, None, top, top.clone(), dq, da, z(2, 8, 7))
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_bilinear_forward_f16(z(2, 3), z(2, 4), z(5, 8), W, None, top)          # a float32 table
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_bilinear_forward_f16(z(2, 3), z(3, 4), z(5, 8, dtype=H), W, None, top)
    capi.simcross_bilinear_forward_f16(q, a, W, None, top)
    capi.simcross_bilinear_backward_f16(q, a, W, top, dq, da, dW)
    torch.cuda.synchronize()
    assert (host(top) == 0).all() and (host(dW) == 0).all()
