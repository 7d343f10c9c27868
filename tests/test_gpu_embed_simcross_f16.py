"""mms_embed_simcross_forward_f16 (csrc/simcross_cross_f16.hip, the gather of csrc/cross_gather.h): SimCross dist_mode 0 / 1 scored from word
ids and a HALF embedding table, on both forward kernels and the norm kernel, without and with the Embed bias.  tests/embed_f16_cross_model.py
has the routing, the cases, their data and references; tests/test_embed_f16_cross_model.py proves them on the CPU.  Every output sits
inside a sentinel-filled buffer and starts as NaN.

Route table, ((N, W1, W2, D), K, halves past a 16-byte boundary) -> the forward launch (embed_f16_cross_model.EXPECTED_ROUTE):
  (   3,  5,  7, 33) K 97      cross_fwd_kernel<_Float16, 1, 1>: ragged tile, chunks of 32 + 1            the same, K 1: every id is row 0
  (   2,  1,  1,  1) K 97      cross_fwd_kernel<_Float16, 1, 1>: W1 == W2 == 1 stays on the word-grid kernels
  (   2,  1,  9, 64) K 97      cross_fwd_kernel<_Float16, 1, 1>: two k tiles, two full chunks
  (   4, 40, 40, 50) K 97      cross_fwd_kernel<_Float16, 1, 1>: small N, 25 tiles per pair
  (1024, 40, 40, 48) K 97      cross_fwd_kernel<_Float16, 5, 5>
  (1024,  8, 16, 50) K 97      cross_fwd_image_kernel<_Float16, 1, 2>;  + 1 half: cross_fwd_kernel<_Float16, 1, 2>;  + 2 halves: the image kernel again
  (1024, 40, 40, 50) K 97      cross_fwd_image_kernel<_Float16, 5, 5>;  + 1 half: cross_fwd_kernel<_Float16, 5, 5>
  cosine: row_norm_kernel<_Float16> twice in front of either
"""
import ctypes

import numpy as np
import pytest
import torch

import cosine_model as cm
import embed_f16_cross_model as em
import f16_cross_model as xm
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
PAD = 64
H = torch.float16
BIAS = [False, True]
BIAS_IDS = ["nobias", "bias"]


def dev(x):
    return torch.from_numpy(np.array(np.ascontiguousarray(x), copy=True)).cuda()


def dev_table(th, off):
    """The half table on the device, `off` halves past a 16-byte boundary."""
    buf = torch.zeros(th.size + 8, dtype=H, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + th.size].view(*th.shape)
    t.copy_(torch.from_numpy(np.array(th, copy=True)))
    assert t.data_ptr() % 16 == (2 * off) % 16 and t.is_contiguous()
    return t


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An fp32 output inside a larger buffer filled with a sentinel, itself filled with NaN."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, device="cuda")
        self.t = self.buf[PAD:PAD + self.n].view(*shape)
        self.t.fill_(float("nan"))

    def intact(self):
        b = host(self.buf)
        return bool((b[:PAD] == np.float32(SENTINEL)).all() and (b[PAD + self.n:] == np.float32(SENTINEL)).all())

    def untouched(self):
        return self.intact() and bool(np.isnan(host(self.t)).all())


def outputs(shape):
    N, W1, W2, D = shape
    return dict(top=Guarded((N, 1, W1, W2)), n0=Guarded((N, W1)), n1=Guarded((N, W2)))


def names_of(mode):
    return ("top", "n0", "n1") if mode == 0 else ("top",)


def finish(out, mode, what):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside %s" % (what, k)
    for k in set(out) - set(names_of(mode)):
        assert np.isnan(host(out[k].t)).all(), "%s: %s was written by a call that does not own it" % (what, k)
    return {k: host(out[k].t).copy() for k in names_of(mode)}


def norms(mode, out):
    return dict(norm0=out["n0"].t, norm1=out["n1"].t) if mode == 0 else {}


def shape_of(c):
    return (c["iq"].shape[0], c["iq"].shape[1], c["ia"].shape[1], c["table"].shape[1])


def embed16(capi, mode, c, off, what):
    """The call under test on the case's table placed `off` halves past a 16-byte boundary."""
    out = outputs(shape_of(c))
    bias = None if c["bias"] is None else dev(c["bias"])
    capi.embed_simcross_forward_f16(mode, dev(c["iq"]), dev(c["ia"]), dev_table(c["table"], off), out["top"].t, embed_bias=bias, **norms(mode, out))
    return finish(out, mode, what + " embed_simcross_forward_f16")


def embed32(capi, mode, c, what):
    """mms_embed_simcross_forward_f32 on the table widened to fp32."""
    out = outputs(shape_of(c))
    bias = None if c["bias"] is None else dev(c["bias"])
    capi.embed_simcross_forward(mode, dev(c["iq"]), dev(c["ia"]), dev(c["table"].astype(np.float32)), out["top"].t, embed_bias=bias, **norms(mode, out))
    return finish(out, mode, what + " embed_simcross_forward (fp32)")


def grid16(capi, mode, c, what):
    """mms_simcross_forward_f16 on the gathered half rows table[clamped ids]."""
    K = c["table"].shape[0]
    out = outputs(shape_of(c))
    capi.simcross_forward_f16(mode, dev(c["table"][em.clamp_ids(c["iq"], K)]), dev(c["table"][em.clamp_ids(c["ia"], K)]), out["top"].t, **norms(mode, out))
    return finish(out, mode, what + " simcross_forward_f16 on the gathered rows")


def assert_same(got, want, mode, what):
    for k in names_of(mode):
        assert_bitexact(got[k], np.asarray(want[k]).reshape(got[k].shape), "%s: %s" % (what, k))


def against_the_other_calls(capi, mode, c, got, off, what):
    """Bit for bit: the fp32 twin on the widened table; without a bias the grid call on the gathered rows; a second call."""
    assert_same(got, embed32(capi, mode, c, what), mode, what + " against the fp32 call on the widened table")
    N, W1, W2, D = shape_of(c)
    if c["bias"] is None:
        if W1 == 1 and W2 == 1:              # the grid call leaves W1 == W2 == 1 to the rows family: there is no such call to compare with
            assert xm.refusal(mode, N, W1, W2, D) == em.UNSUPPORTED
        else:
            assert_same(got, grid16(capi, mode, c, what), mode, what + " against the grid call on the gathered rows")
    assert_same(embed16(capi, mode, c, off, what), got, mode, what + ": second call")


def check_against_fp64(c, got, what):
    """top and the norms within f16_cross_model's dense_bar(e_o) of fp64; each figure is printed before it is asserted."""
    fails = []
    for k in ("top", "n0", "n1"):
        ref64, scale = c["ref"][k]
        g = got[k].reshape(ref64.shape)
        assert np.isfinite(g).all() and np.isfinite(ref64).all(), "%s %s: non-finite" % (what, k)
        ek = cm.scaled_error(g, ref64, scale)[0]
        msg = "%s %s: e(kernel) = %.2f, e(oracle) = %.2f, bar %.2f (x 2^-24)" % (what, k, ek / cm.U24, c["e_o"][k] / cm.U24, cm.dense_bar(c["e_o"][k]) / cm.U24)
        print(msg)
        if not ek <= cm.dense_bar(c["e_o"][k]):
            fails.append(msg)
    assert not fails, "; ".join(fails)


# ----------------------------------------------------------------------------------------------------------------------
# 1. Euclid: the oracle's bits on the gathered fp32 rows, the fp32 twin's, the grid call's
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=BIAS_IDS)
@pytest.mark.parametrize("case", em.CASES, ids=em.case_id)
def test_euclid_bit_for_bit(case, bias, oracle, hiplib):
    from mms_answer_selection_amd import capi
    shape, K, off = case
    what = "euclid %s %s" % (em.case_id(case), "bias" if bias else "no bias")
    c = em.reference(oracle, 1, shape, K, "dense", bias)
    got = embed16(capi, 1, c, off, what)
    assert_bitexact(got["top"], c["top"], what + ": top against the CPU oracle on bias + widen(table)[ids]")
    assert (got["top"][shape[0] - 1] == 1.0).all(), what + ": the pair of equal rows scores 1"
    against_the_other_calls(capi, 1, c, got, off, what)


# ----------------------------------------------------------------------------------------------------------------------
# 2. cosine, exact-sum probe table: the oracle's bits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=BIAS_IDS)
@pytest.mark.parametrize("case", em.CASES, ids=em.case_id)
def test_cosine_probe_bit_for_bit(case, bias, oracle, hiplib):
    from mms_answer_selection_amd import capi
    shape, K, off = case
    what = "cosine probe %s %s" % (em.case_id(case), "bias" if bias else "no bias")
    c = em.reference(oracle, 0, shape, K, "probe", bias)
    got = embed16(capi, 0, c, off, what)
    assert_same(got, c, 0, what + " against the CPU oracle")
    against_the_other_calls(capi, 0, c, got, off, what)


# ----------------------------------------------------------------------------------------------------------------------
# 3. cosine, dense: the existing fp64 bar, and the other calls' bits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=BIAS_IDS)
@pytest.mark.parametrize("case", em.CASES, ids=em.case_id)
def test_cosine_dense_against_fp64(case, bias, oracle, hiplib):
    from mms_answer_selection_amd import capi
    shape, K, off = case
    what = "cosine dense %s %s" % (em.case_id(case), "bias" if bias else "no bias")
    c = em.reference(oracle, 0, shape, K, "dense", bias)
    got = embed16(capi, 0, c, off, what)
    check_against_fp64(c, got, what)
    against_the_other_calls(capi, 0, c, got, off, what)


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals and N == 0 write nothing
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hiplib):
    """dist_mode 2 (and any other unknown one): MMS_ERR_UNSUPPORTED; bad sizes, K <= 0, K D > 2^31 - 1, a NULL required pointer:
    MMS_ERR_INVALID_ARG; N == 0: MMS_OK; none of them writes top or the norms.  The accepted call next to them writes only what it owns."""
    from mms_answer_selection_amd import capi
    big, K = em.REFUSED_SHAPE, em.REFUSED_K
    i = em.inputs(big, K, "dense")
    t = dict(iq=dev(i["iq"]), ia=dev(i["ia"]), table=dev_table(i["table"], 0), bias=dev(i["bias"]))
    lib = capi.lib()
    s = torch.cuda.current_stream().cuda_stream

    def raw(mode, shape, k, out, null=()):
        p = dict(iq=t["iq"].data_ptr(), ia=t["ia"].data_ptr(), table=t["table"].data_ptr(), bias=t["bias"].data_ptr(), top=out["top"].t.data_ptr(),
                 n0=out["n0"].t.data_ptr(), n1=out["n1"].t.data_ptr())
        p = {key: (None if key in null else ctypes.c_void_p(v)) for key, v in p.items()}
        return lib.mms_embed_simcross_forward_f16(mode, *shape, k, p["iq"], p["ia"], p["table"], p["bias"], p["top"], p["n0"], p["n1"], s)

    def refused(mode, shape, k, code, **kw):
        out = outputs(big)
        assert raw(mode, shape, k, out, **kw) == code, (mode, shape, k, kw)
        assert kw or em.refusal(mode, *shape, k) == code, "the model's refusal disagrees"
        torch.cuda.synchronize()
        for name, g in out.items():
            assert g.untouched(), "mode %d %s K %d %s: %s was written" % (mode, shape, k, kw, name)

    for mode in (2, 3, -1):
        refused(mode, big, K, em.UNSUPPORTED)
    for mode in (0, 1):
        for shape in ((-1, 5, 7, 50), (4, 0, 7, 50), (4, 5, -7, 50), (4, 5, 7, 0)):
            refused(mode, shape, K, em.INVALID_ARG)
        refused(mode, big, 0, em.INVALID_ARG)
        refused(mode, big, -5, em.INVALID_ARG)
        refused(mode, big, (1 << 31) // 50 + 1, em.INVALID_ARG)
        for which in ("iq", "ia", "table", "top"):
            refused(mode, big, K, em.INVALID_ARG, null=(which,))
        refused(mode, (0, 5, 7, 50), K, em.OK)
    for which in ("n0", "n1"):
        refused(0, big, K, em.INVALID_ARG, null=(which,))                  # cosine: the norms are required
    # accepted: Euclid takes NULL norms, a NULL bias is no bias; each mode writes only what it owns
    for mode, null in ((1, ("n0", "n1")), (1, ("bias",)), (1, ()), (0, ("bias",)), (0, ())):
        out = outputs(big)
        assert raw(mode, big, K, out, null=null) == em.OK
        got = finish(out, mode, "accepted mode %d" % mode)
        assert all(np.isfinite(v).all() for v in got.values())


# ----------------------------------------------------------------------------------------------------------------------
# 5. the wrapper's own checks come before any launch
# ----------------------------------------------------------------------------------------------------------------------
def test_wrapper_checks_dtype_and_shape(hiplib):
    from mms_answer_selection_amd import capi
    z = lambda *s: torch.zeros(*s, device="cuda")
    iq, ia, table, top = z(2, 3), z(2, 4), torch.ones((5, 8), dtype=H, device="cuda"), Guarded((2, 1, 3, 4))
    with pytest.raises(ValueError):
        capi.embed_simcross_forward_f16(1, iq, ia, table.float(), top.t)             # an fp32 table
    with pytest.raises(ValueError):
        capi.embed_simcross_forward_f16(1, iq, z(3, 4), table, top.t)                # batch sizes differ
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_forward_f16(1, iq, ia, table, z(2, 1, 4, 3))             # top's shape
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_forward_f16(1, iq, ia, table, top.t, embed_bias=z(7))    # the bias is D floats
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_forward_f16(0, iq, ia, table, top.t, norm0=z(2, 4), norm1=z(2, 4))
    with pytest.raises(capi.MMSError):
        capi.embed_simcross_forward_f16(2, iq, ia, table, top.t)                     # dist_mode 2: the library's refusal
    torch.cuda.synchronize()
    assert top.untouched()
    capi.embed_simcross_forward_f16(1, iq, ia, table, top.t)
    torch.cuda.synchronize()
    assert top.intact() and (host(top.t) == 1.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 6. capture in a graph
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0], ids=["euclid", "cosine"])
def test_graph_capture_replays_the_same_bits(mode, oracle, hiplib):
    """No workspace, no allocation, no synchronisation: the call (one launch, or three) is captured and replayed; the replay writes the eager
    call's bits, and again after the ids have changed under the graph."""
    from mms_answer_selection_amd import capi
    shape, K, off = em.GRAPH_CASE
    what = "graph %s mode %d" % (em.case_id(em.GRAPH_CASE), mode)
    c = em.reference(oracle, mode, shape, K, "dense", True)
    eager = embed16(capi, mode, c, off, what)
    iq, ia, table, bias = dev(c["iq"]), dev(c["ia"]), dev_table(c["table"], off), dev(c["bias"])
    out = outputs(shape)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            capi.embed_simcross_forward_f16(mode, iq, ia, table, out["top"].t, embed_bias=bias, **norms(mode, out))
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out.values()), what + ": capture itself ran the kernels"
    graph.replay()
    assert_same(finish(out, mode, what + " replay"), eager, mode, what + ": replay against the eager call")
    if mode == 1:
        assert_same(eager, c, mode, what + " against the oracle")
    # new ids in the captured buffers: the rows of pair 0 become those of pair 1
    iq[0].copy_(iq[1])
    ia[0].copy_(ia[1])
    graph.replay()
    again = finish(out, mode, what + " second replay")
    assert_bitexact(again["top"][0], eager["top"][1], what + ": the replay read the new ids")
    assert_bitexact(again["top"][1:], eager["top"][1:], what + ": the other pairs keep their bits")
