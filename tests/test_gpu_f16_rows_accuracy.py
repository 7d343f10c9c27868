"""The fp16-storage sentence-vector calls (mms_simcross_euclid_forward[_backward]_f16, mms_simcross_cosine_forward[_backward]_f16;
csrc/simcross_rows_f16.hip) on every kernel instantiation: the ordered Euclid kernels bit for bit, the tree sum and the cosine kernel
against fp64 with gradients held to the half bracket, exact-sum probes, edge rows, guard bands and refusals.

tests/test_gpu_parity.py runs these calls at D = 8, 304, 408, 512, 520, 1024, 2048: NIT 1, 2 and 4 of the MMS_NIT4 tables, never
3; its cosine gradients pass at |ref| 2^-10 + 1e-5 max |ref|; no edge row, no guard band and no refusal of the Euclid calls.  Here
(tests/f16_rows_model.py has the routing, the shapes, the references and the bars; tests/test_f16_rows_model.py proves them on the
CPU): every shape is run forward-only and fused, every output sits inside a sentinel-filled buffer.

Route table: (N, D) -> kernel<NIT, ...>, read off simcross_euclid_rows_f16 / simcross_cosine_rows_f16.  B = false for the forward-only
call, true for the fused one; NIT = ceil(RW D8 / 64), D8 = D / 8.  profiles/f16_routes.txt records the kernels a trace of this
file saw per test id.

 Euclid, ordered, D <= 400: euclid_rows_wave_f16_kernel<NIT, 2, B>, two pairs per wave, 8 per workgroup, 32-lane speculation windows
  ( 5,    8)  NIT 1: one lane per pair holds data; the third wave has one pair and mirrors it
  ( 9,  256)  2 D8 == 64: exactly one full trip; N % 8 == 1
  ( 6,  264)  NIT 2: two lanes in trip 2
  ( 4,  384)  NIT 2; D4 % 3 == 0: the image has no zero pad
  ( 7,  400)  NIT 2: the last width of this kernel; N % 8 == 7
  ( 1,  304)  NIT 2: a lone pair
  (16,  304)  exactly two full workgroups
 Euclid, ordered, D >= 408: euclid_rows_lanechain_f16_kernel<NIT, B, 8>, one wave per pair, 8 per workgroup, lane p of wave 0 walks pair p
  ( 3,  408)  NIT 1: the first width         ( 9,  512)  NIT 1 full; N % 8 == 1        ( 8,  520)  NIT 2, one lane in trip 2; N % 8 == 0
  ( 5, 1024)  NIT 2 full                     ( 7, 1032)  NIT 3, one lane in trip 3     ( 2, 1536)  NIT 3 full
  ( 3, 1544)  NIT 4, one lane in trip 4      ( 1, 2048)  NIT 4 full; seven waves mirror pair 0
 Euclid, distance mode tree: euclid_rows_wave_f16_kernel<NIT, 1, B, true>, one wave per pair, 4 per workgroup, no LDS
  ( 5,    8)  NIT 1     ( 6,  384)  NIT 1     ( 9,  512)  NIT 1 full     ( 4,  520)  NIT 2, one lane in trip 2; N % 4 == 0
  ( 7, 1032)  NIT 3, one lane in trip 3       ( 2, 1536)  NIT 3 full     ( 3, 2048)  NIT 4 full
 cosine: cosine_rows_wave_f16_kernel<NIT, B>, one wave per pair, 4 per workgroup
  ( 5,    8)  NIT 1     ( 9,  512)  NIT 1 full     ( 6,  520)  NIT 2     ( 7, 1032)  NIT 3, one lane in trip 3     ( 2, 1536)  NIT 3 full
  ( 3, 1544)  NIT 4, one lane in trip 4       ( 1, 2048)  NIT 4 full; three waves return early     ( 8,  304)  NIT 1; N % 4 == 0
 euclid_rows_wave_f16_kernel<3 | 4, 2, .> cannot be reached (D <= 400) and is not tested.
"""
import ctypes

import numpy as np
import pytest
import torch

import cosine_model as cm
import f16_rows_model as fm
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
SENTINEL16 = -1234.0        # exact as a half
PAD = 64                    # elements on each side of an output: a multiple of 8 halves, so the output keeps its alignment
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2      # include/mms.h


def dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()


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


def outputs(N, D, off=None):
    off = off or {}
    h = torch.float16
    return dict(top=Guarded((N, 1, 1, 1)), n0=Guarded((N, 1)), n1=Guarded((N, 1)), dq=Guarded((N, 1, D), h, off.get("dq", 0)),
                da=Guarded((N, 1, D), h, off.get("da", 0)))


def finish(out, names, what):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside %s" % (what, k)
    for k in set(out) - set(names):
        assert np.isnan(host(out[k].t)).all(), "%s: %s was written by a call that does not own it" % (what, k)
    return {k: host(out[k].t).copy() for k in names}


def euclid(capi, qh, ah, dT=None, what=""):
    """The forward-only call (dT None) or the fused one."""
    N, _, D = qh.shape
    out = outputs(N, D)
    if dT is None:
        capi.simcross_euclid_forward_f16(dev(qh), dev(ah), out["top"].t)
        return finish(out, ("top",), what + " forward")
    capi.simcross_euclid_forward_backward_f16(dev(qh), dev(ah), dev(dT), out["top"].t, out["dq"].t, out["da"].t)
    return finish(out, ("top", "dq", "da"), what + " fused")


def cosine(capi, qh, ah, dT=None, norms=True, what=""):
    N, _, D = qh.shape
    out = outputs(N, D)
    n = dict(norm0=out["n0"].t, norm1=out["n1"].t) if norms else {}
    names = ("top", "n0", "n1") if norms else ("top",)
    if dT is None:
        capi.simcross_cosine_forward_f16(dev(qh), dev(ah), out["top"].t, **n)
        return finish(out, names, what + " forward")
    capi.simcross_cosine_forward_backward_f16(dev(qh), dev(ah), dev(dT), out["top"].t, out["dq"].t, out["da"].t, **n)
    return finish(out, names + ("dq", "da"), what + " fused")


def assert_halves(got, want, what):
    """uint16 for uint16; NaNs match NaNs."""
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, what
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d halves differ, first at %s: %r vs %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def assert_same(got, want, names, what):
    for k in names:
        (assert_halves if got[k].dtype == np.float16 else assert_bitexact)(got[k], want[k], "%s: %s" % (what, k))


def to_half(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def check_ordered(capi, c, what):
    """The header's contract: top the fp32 oracle's bits on the widened inputs, dq / da its gradient's RNE halves; the forward-only
    call and a second call give the same bits."""
    fu = euclid(capi, c["qh"], c["ah"], c["dT"], what)
    assert_bitexact(fu["top"], c["top"], what + ": top against the oracle")
    assert_halves(fu["dq"], to_half(c["dq"]), what + ": dq against the oracle's halves")
    assert_halves(fu["da"], to_half(c["da"]), what + ": da against the oracle's halves")
    assert_same(euclid(capi, c["qh"], c["ah"], None, what), fu, ("top",), what + ": forward-only against fused")
    assert_same(euclid(capi, c["qh"], c["ah"], c["dT"], what), fu, ("top", "dq", "da"), what + ": second fused call")
    return fu


def check_against_fp64(c, got, names, what):
    """fp32 outputs within dense_bar(e_o) of fp64 over the finite elements; the non-finite ones are the oracle's, element for element."""
    fails = []
    for k in names:
        ref64, scale = c["ref"][k]
        g = got[k].reshape(ref64.shape)
        fin = np.isfinite(ref64) & np.isfinite(scale)
        assert (np.isnan(g) == np.isnan(c[k].reshape(g.shape))).all() and (np.isinf(g) == np.isinf(c[k].reshape(g.shape))).all(), \
            "%s %s: the NaNs / Infs are not where the oracle has them" % (what, k)
        assert np.isfinite(g[fin]).all(), "%s %s: a finite element came out non-finite" % (what, k)
        ek = cm.scaled_error(g[fin], ref64[fin], scale[fin])[0] if fin.any() else 0.0
        msg = "%s %s: e(kernel) = %.2f, e(oracle) = %.2f, bar %.2f (x 2^-24)" % (what, k, ek / cm.U24, c["e_o"][k] / cm.U24,
                                                                               cm.dense_bar(c["e_o"][k]) / cm.U24)
        print(msg)
        if not ek <= cm.dense_bar(c["e_o"][k]):
            fails.append(msg)
    assert not fails, "; ".join(fails)


def check_gradients(c, got, refs, what, bar=None, pinned=True):
    """dq, da inside the half bracket around the fp64 gradient from the forward the launch stored; b = dense_bar(e_o) or `bar`."""
    for k, (ref64, scale) in zip(("dq", "da"), refs):
        b = cm.dense_bar(c["e_o"][k]) if bar is None else bar
        lo, hi = fm.check_bracket("%s %s" % (what, k), got[k], ref64, scale, b)
        share = fm.pinned_share(lo, hi)
        print("%s %s: inside the bracket, b = %.2f x 2^-24, pinned %.3f %%" % (what, k, b / cm.U24, 100 * share))
        if pinned:
            assert share >= fm.PINNED_MIN, "%s %s: only %.2f %% of the elements are pinned to one half" % (what, k, 100 * share)


# ----------------------------------------------------------------------------------------------------------------------
# 1. Euclid, ordered: bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fm.WAVE2 + fm.LANECHAIN, ids=fm.shape_id)
def test_euclid_ordered_dense_bit_for_bit(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    assert capi.lib().mms_get_f16_distance_mode() == 0
    check_ordered(capi, fm.dense_case(oracle, fm.family(shape[1]), shape), "%s %s" % (fm.family(shape[1]), shape))


@pytest.mark.parametrize("D", fm.ADVERSARIAL_D)
def test_euclid_window_miss_re_walks_exactly(D, oracle, hiplib):
    """f16_rows_model.adversarial_rows: the tree sum that centres the 32-lane window of segment 1 is more than 12 ulp from the
    sequential sum it must hit, so the kernel re-walks -- and still gives the oracle's bits."""
    from mms_answer_selection_amd import capi
    qh, ah = fm.adversarial_rows(D)
    tree, seq = fm.first_segment_sums(qh, ah, 0)
    assert abs(int(tree.view(np.int32)) - int(seq.view(np.int32))) > fm.SPEC_WINDOW_32
    dT = np.random.default_rng(4).standard_normal((qh.shape[0], 1, 1, 1)).astype(np.float32)
    check_ordered(capi, fm.euclid_reference(oracle, qh, ah, dT), "window miss, D = %d" % D)


@pytest.mark.parametrize("fam", ["wave2", "lanechain"])
def test_euclid_ordered_edges(fam, oracle, hiplib):
    """Inf, NaN, +-65504 against -+65504, subnormal halves, top_diff 1e8 (halves overflow where astype(float16) does), a == q,
    top_diff == 0: the oracle's bits on the widened inputs, NaN for NaN."""
    from mms_answer_selection_amd import capi
    c = fm.edge_case(oracle, fam)
    fu = check_ordered(capi, c, "%s edges, D = %d" % (fam, fm.EDGE_D[fam]))
    assert np.isinf(fu["dq"][4]).any() and not np.isnan(fu["dq"][4]).any()
    assert not np.signbit(fu["dq"][8]).any() and not np.signbit(fu["da"][8]).any(), "top_diff == 0: 0 + (-0) is +0"


# ----------------------------------------------------------------------------------------------------------------------
# 2. Euclid, tree sum
# ----------------------------------------------------------------------------------------------------------------------
def tree_calls(capi, c, what):
    capi.set_f16_distance_mode("tree")
    try:
        fu = euclid(capi, c["qh"], c["ah"], c["dT"], what)
        again = euclid(capi, c["qh"], c["ah"], c["dT"], what)
        fw = euclid(capi, c["qh"], c["ah"], None, what)
    finally:
        capi.set_f16_distance_mode("ordered")
    assert_same(again, fu, ("top", "dq", "da"), what + ": second fused call")
    assert_same(fw, fu, ("top",), what + ": forward-only against fused")
    return fu


@pytest.mark.parametrize("shape", fm.TREE, ids=fm.shape_id)
def test_euclid_tree_dense_against_fp64(shape, oracle, hiplib):
    """top within twice the ordered fp32 oracle's own error against fp64 (+ 4 x 2^-24); gradients inside the half bracket around the
    fp64 backward from the stored top, at least 99 % of them pinned; deterministic; the ordered mode is bit-exact again afterwards."""
    from mms_answer_selection_amd import capi
    what = "tree %s" % (shape,)
    c = fm.dense_case(oracle, "tree", shape)
    fu = tree_calls(capi, c, what)
    check_against_fp64(c, fu, ("top",), what)
    check_gradients(c, fu, fm.euclid_grad_ref(oracle, c, fu["top"]), what)
    assert_bitexact(euclid(capi, c["qh"], c["ah"], None, what)["top"], c["top"], what + ": ordered again")


def test_euclid_tree_edges(oracle, hiplib):
    from mms_answer_selection_amd import capi
    c = fm.edge_case(oracle, "tree")
    what = "tree edges, D = %d" % fm.EDGE_D["tree"]
    fu = tree_calls(capi, c, what)
    check_against_fp64(c, fu, ("top",), what)
    assert fu["top"][0] == 0.0 and fu["top"][7] == 1.0
    check_gradients(c, fu, fm.euclid_grad_ref(oracle, c, fu["top"]), what, pinned=False)
    assert np.isinf(fu["dq"][4]).any() and np.isnan(fu["dq"][1]).all() and not fu["dq"][7].any() and not fu["dq"][8].any()
    assert not np.signbit(fu["dq"][8]).any() and not np.signbit(fu["da"][8]).any()


# ----------------------------------------------------------------------------------------------------------------------
# 3. cosine
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fm.COSINE, ids=fm.shape_id)
def test_cosine_probe_bit_for_bit(shape, oracle, hiplib):
    """Exact-sum rows: top, norm0, norm1 are the CPU oracle's bits and the fp32 call's on the widened data, forward-only and fused;
    each gradient element is one (j, k) contribution, inside the half bracket at BAR_GRAD; omitting the norms changes no bit."""
    from mms_answer_selection_amd import capi
    what = "cosine probe %s" % (shape,)
    c = fm.probe_case(oracle, shape)
    assert (c["qh"].astype(np.float32) == c["q"]).all() and (c["ah"].astype(np.float32) == c["a"]).all()
    fu = cosine(capi, c["qh"], c["ah"], c["dT"], what=what)
    assert_same(fu, c, ("top", "n0", "n1"), what + " against the oracle")
    N, D = shape
    o32 = dict(top=Guarded((N, 1, 1, 1)), n0=Guarded((N, 1)), n1=Guarded((N, 1)), dq=Guarded((N, 1, D)), da=Guarded((N, 1, D)))
    capi.simcross_forward_backward(0, dev(c["q"]), dev(c["a"]), dev(c["dT"]), o32["top"].t, o32["dq"].t, o32["da"].t, norm0=o32["n0"].t,
                                   norm1=o32["n1"].t)
    assert_same(fu, finish(o32, ("top", "n0", "n1", "dq", "da"), what + " fp32"), ("top", "n0", "n1"), what + " against the fp32 call")
    check_gradients(c, fu, (c["ref"]["dq"], c["ref"]["da"]), what, bar=cm.BAR_GRAD, pinned=False)
    assert_same(cosine(capi, c["qh"], c["ah"], None, what=what), fu, ("top", "n0", "n1"), what + ": forward-only against fused")
    assert_same(cosine(capi, c["qh"], c["ah"], c["dT"], norms=False, what=what), fu, ("top", "dq", "da"), what + ": fused without norms")
    assert_same(cosine(capi, c["qh"], c["ah"], None, norms=False, what=what), fu, ("top",), what + ": forward-only without norms")
    assert_same(cosine(capi, c["qh"], c["ah"], c["dT"], what=what), fu, ("top", "n0", "n1", "dq", "da"), what + ": second fused call")


@pytest.mark.parametrize("shape", fm.COSINE, ids=fm.shape_id)
def test_cosine_dense_against_fp64(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    what = "cosine %s" % (shape,)
    c = fm.dense_case(oracle, "cosine", shape)
    fu = cosine(capi, c["qh"], c["ah"], c["dT"], what=what)
    check_against_fp64(c, fu, ("top", "n0", "n1"), what)
    check_gradients(c, fu, fm.cosine_grad_ref(c, fu["top"], fu["n0"], fu["n1"]), what)
    assert_same(cosine(capi, c["qh"], c["ah"], None, what=what), fu, ("top", "n0", "n1"), what + ": forward-only against fused")
    assert_same(cosine(capi, c["qh"], c["ah"], c["dT"], what=what), fu, ("top", "n0", "n1", "dq", "da"), what + ": second fused call")


def test_cosine_edges(oracle, hiplib):
    """The edge rows of f16_rows_model.edge_rows, a zero q row and a zero a row (0 / 0) among them: NaN and Inf in top and the norms
    where the oracle and the fp32 kernel have them; finite pairs at the dense bars; gradients inside the bracket (NaN where it is
    NaN, +-Inf where top_diff = 1e8 overflows a half)."""
    from mms_answer_selection_amd import capi
    c = fm.edge_case(oracle, "cosine")
    what = "cosine edges, D = %d" % fm.EDGE_D["cosine"]
    fu = cosine(capi, c["qh"], c["ah"], c["dT"], what=what)
    check_against_fp64(c, fu, ("top", "n0", "n1"), what)
    check_gradients(c, fu, fm.cosine_grad_ref(c, fu["top"], fu["n0"], fu["n1"]), what, pinned=False)
    N, _, D = c["qh"].shape
    q32, a32 = c["qh"].astype(np.float32), c["ah"].astype(np.float32)
    o32 = dict(top=Guarded((N, 1, 1, 1)), n0=Guarded((N, 1)), n1=Guarded((N, 1)), dq=Guarded((N, 1, D)), da=Guarded((N, 1, D)))
    capi.simcross_forward_backward(0, dev(q32), dev(a32), dev(c["dT"]), o32["top"].t, o32["dq"].t, o32["da"].t, norm0=o32["n0"].t, norm1=o32["n1"].t)
    k32 = finish(o32, ("top", "n0", "n1", "dq", "da"), what + " fp32")
    for k in ("top", "n0", "n1", "dq", "da"):
        assert (np.isnan(fu[k]) == np.isnan(k32[k])).all(), "%s %s: the NaNs are not where the fp32 kernel has them" % (what, k)
        assert (np.isnan(fu[k]) == np.isnan(c[k])).all(), "%s %s: the NaNs are not where the oracle has them" % (what, k)
    for k in ("top", "n0", "n1"):
        assert (np.isinf(fu[k]) == np.isinf(k32[k])).all() and (np.isinf(fu[k]) == np.isinf(c[k])).all(), "%s %s: Infs" % (what, k)
    assert np.isnan(fu["top"][[0, 1, 5, 7, 8]]).all() and fu["n0"][7] == 0 and fu["n1"][8] == 0 and np.isinf(fu["dq"][4]).any()
    assert_same(cosine(capi, c["qh"], c["ah"], None, what=what), fu, ("top", "n0", "n1"), what + ": forward-only against fused")


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
ENTRY = ["euclid_forward", "euclid_fused", "cosine_forward", "cosine_fused"]


def raw_call(capi, entry, N, D, q, a, dT, out, skew=None, null=None):
    """The C entry point itself: its return code.  skew: {argument: bytes added to its address}; null: arguments passed as NULL."""
    skew, null = skew or {}, null or ()
    p = dict(q=q.data_ptr(), a=a.data_ptr(), dT=dT.data_ptr(), top=out["top"].t.data_ptr(), n0=out["n0"].t.data_ptr(),
             n1=out["n1"].t.data_ptr(), dq=out["dq"].t.data_ptr(), da=out["da"].t.data_ptr())
    p = {k: (None if k in null else ctypes.c_void_p(v + skew.get(k, 0))) for k, v in p.items()}
    s = torch.cuda.current_stream().cuda_stream
    lib = capi.lib()
    if entry == "euclid_forward":
        return lib.mms_simcross_euclid_forward_f16(N, D, p["q"], p["a"], p["top"], s)
    if entry == "euclid_fused":
        return lib.mms_simcross_euclid_forward_backward_f16(N, D, p["q"], p["a"], p["dT"], p["top"], p["dq"], p["da"], s)
    if entry == "cosine_forward":
        return lib.mms_simcross_cosine_forward_f16(N, D, p["q"], p["a"], p["top"], p["n0"], p["n1"], s)
    return lib.mms_simcross_cosine_forward_backward_f16(N, D, p["q"], p["a"], p["dT"], p["top"], p["n0"], p["n1"], p["dq"], p["da"], s)


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_write_nothing(entry, hiplib):
    """D % 8 != 0, D > 2048 and an operand eight bytes past a 16-byte boundary: MMS_ERR_UNSUPPORTED; a NULL required pointer:
    MMS_ERR_INVALID_ARG; N == 0: MMS_OK; none of them writes anything.  The forward-only calls take no dq / da, so nothing about
    those can refuse them; the accepted call next to each refusal returns MMS_OK and writes only what it owns."""
    from mms_answer_selection_amd import capi
    N = 5
    fused = entry.endswith("fused")
    owns = (("top",) if entry.startswith("euclid") else ("top", "n0", "n1")) + (("dq", "da") if fused else ())
    dT = torch.ones((N, 1, 1, 1), device="cuda")

    def operands(D):
        # eight halves longer than N D, so that an operand eight bytes on is still inside its allocation
        q = torch.full((N * D + 8,), 0.5, dtype=torch.float16, device="cuda")
        a = torch.full((N * D + 8,), 0.25, dtype=torch.float16, device="cuda")
        assert q.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
        return q, a

    def refused(D, code, n=N, **kw):
        q, a = operands(D)
        out = outputs(N, D + 8)
        assert raw_call(capi, entry, n, D, q, a, dT, out, **kw) == code, (entry, D, kw)
        torch.cuda.synchronize()
        for k, g in out.items():
            assert g.untouched(), "%s D = %d %s: %s was written" % (entry, D, kw, k)

    refused(12, UNSUPPORTED)
    refused(2056, UNSUPPORTED)
    for which in ("q", "a") + (("dq", "da") if fused else ()):
        refused(512, UNSUPPORTED, skew={which: 8})
    for which in ("q", "a", "top") + (("dT", "dq", "da") if fused else ()):
        refused(512, INVALID_ARG, null=(which,))
    refused(512, OK, n=0)
    refused(512, INVALID_ARG, n=-1)
    # accepted: the same operands, aligned
    q, a = operands(512)
    out = outputs(N, 512)
    assert raw_call(capi, entry, N, 512, q, a, dT, out) == OK
    got = finish(out, owns, entry)
    assert np.isfinite(got["top"]).all()
    if not fused:
        # whatever dq / da hold or wherever they are: the forward-only entry points have no such argument
        assert out["dq"].untouched() and out["da"].untouched()
