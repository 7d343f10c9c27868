"""Cosine SimCross (dist_mode 0: csrc/simcross_rows_cosine.hip,csrc/simcross_cross.hip, csrc/cosine_math.h) on every kernel route: exact-sum probes
bit for bit, gradients at bars counted from the roundings, dense data against fp64, and the edge rows.

tests/test_gpu_parity.py holds cosine to 1e-5 max(1, max |ref|) on ten shapes, all with N <= 4 on grids: a score wrong by 2^-14
of itself, a lost tail element or a wrong small gradient row passes, and the unsplit tiled backward, the ragged pair32
instantiations, the scalar rows kernel on a misaligned view and the vec4 rows kernel past one trip are never run.  Here
(tests/cosine_model.py has the constructions and the bars; tests/test_cosine_model.py proves them on the CPU):

  * exact-sum probes -- q and a hold small integers times one power of two, so q.q, a.a and q.a are exact in ANY order and
    top, norm0, norm1 must be the CPU oracle's bit for bit on every route, through the Embed-fused forward and through the
    fp16-storage forward as well; a gradient element is ONE (j, k) contribution: bit for bit where the kernel spells the
    reference's expression (cosine_grad_div), within BAR_GRAD = 5 roundings of |t1| + |t2| where it uses per-pair factors;
  * the fused call gives the bits of forward + backward, two calls give the same bits, a power-of-two scaling changes none;
  * dense data -- GloVe-like rows, dT spanning 2^-10 .. 2^10 across pairs: within twice the CPU oracle's own scaled error
    against fp64 (+ 4 x 2^-24), componentwise at each element's own scale;
  * edges -- zero rows, Inf / NaN, squares that overflow, are subnormal or flush to zero; no store outside an output.

Route table: (N, W1, W2, D) -> forward | backward | fused, read off simcross_elementwise_forward, simcross_elementwise_backward,
simcross_elementwise_forward_backward and launch_cross_fwd.  pair32<d4, F, B> = cosine_pair32_kernel<d4, FWD, BWD, 8> (16 pairs per
workgroup, 32 lanes per pair, NIT = ceil(d4 / 32) loads per lane); rows<V, F, B> = cosine_rows_kernel<VEC4, FWD, BWD> (4 pairs per
workgroup); fwd<J, K> = row_norm_kernel x 2 + cross_fwd_kernel<float, J, K, 0>; image<J, K> = row_norm_kernel x 2 +
cross_fwd_image_kernel<float, J, K, 0, 50>; tiled(split) = cross_bwd_tiled_kernel<float, 0, true>, split = 1 while N ceil(D / 32) < 1024.  On
word grids the fused call is the forward followed by the backward.  profiles/cosine_routes.txt records the kernels a trace of
this file saw per test id.

 one word per sentence, D = 100 / 200 / 300, 16-byte aligned: pair32 forward | pair32 backward | pair32 fused
  (   1, 1, 1,  100)  pair32<25, ., .>: NIT 1, 7 idle lanes per pair (the clamp i < D4C ? i : 0); N = 1: the second half-wave and
                      seven waves have no pair (row clamped to N - 1, stores masked by `have`)
  (  17, 1, 1,  100)  N % 16 == 1: a second workgroup with one pair
  (  31, 1, 1,  200)  pair32<50, ., .>: NIT 2, 14 idle lanes in the second trip; N % 16 == 15: one half-wave without a pair
  (  33, 1, 1,  300)  pair32<75, ., .>: NIT 3, 21 idle lanes; three workgroups, the last with one pair
  (  16, 1, 1,  300)  N % 16 == 0: exactly one full workgroup
 one word, D % 4 == 0 at other widths, aligned: rows<true, T, F> | rows<true, F, T> | rows<true, T, T>
  (   5, 1, 1,    4)  one float4 per row: 63 idle lanes; N % 4 == 1: the last workgroup's waves 1..3 return early
  (   9, 1, 1,  256)  D / 4 == 64: exactly one trip of the lane loop
  (   9, 1, 1,  260)  D / 4 == 65: a second trip for lane 0 only
  (   3, 1, 1, 1028)  257 float4: a fifth trip for lane 0; N < 4
  (   2, 1, 1, 2100)  525 float4: nine trips, the last with 13 lanes
  (   7, 1, 1,  304)  the width next to pair32's 300: 76 float4
 one word, D % 4 != 0: rows<false, T, F> | rows<false, F, T> | rows<false, T, T>
  (   9, 1, 1,    7)  fewer elements than lanes
  (   5, 1, 1,    1)  D = 1: T = +-1, every gradient element cancels to zero or one rounding
  (   6, 1, 1,   65)  a second trip for lane 0
  (   4, 1, 1,  301)  next to pair32's 300, five trips
 one word, D = 100 / 300 / 304 through a view offset by one float (test_misaligned_views): q or a offset -> rows<false, ., .> in
  forward, backward and fused; dq or da offset -> forward stays pair32 / rows<true>, backward and fused rows<false, ., .>
 word grids, forward | backward
  (   4,  5,  7, 300)  fwd<1, 1>: one 8 x 8 tile per pair, partly filled, ten d chunks of 32 (D % 32 != 0) | tiled(split): 80 workgroups
  (1030, 40, 40,  52)  fwd<5, 5>: N >= 1024 keeps the largest register tile; D != 50 declines the image | tiled(unsplit): 2060
  (1025, 16, 24,  50)  image<2, 3>: odd N, the last workgroup's second wave idle | tiled(unsplit)
  (1024, 40,  8,  50)  image<5, 1>: N at the threshold | tiled(unsplit), 2048 workgroups
  (1023, 16, 24,  50)  N one below the image kernel: fwd<2, 2> (the tile shrinks until N tiles >= 1024) | tiled(unsplit): 2046
  (   3, 41,  9,  33)  fwd<1, 1>: 6 x 2 tiles with remainders in both, D = 33: a chunk of one column | tiled(split), dn = 1
  (   2, 40, 40,  50)  fwd<1, 1>: 5 x 5 tiles | tiled(split): the driver's grid at a small batch
  ( 511,  8,  8,  50)  fwd<1, 1> | tiled(split): 1022 < 1024, the last split size
  ( 512,  8,  8,  50)  fwd<1, 1>: N < 1024 declines the image | tiled(unsplit): 1024, the first unsplit size
  (1024,  5,  7,  20)  fwd<1, 1>: W % 8 != 0 declines the image | tiled(unsplit): D < 32, one chunk with dn = 20
  ( 600, 40, 40,  50)  fwd<4, 4>: 2 x 2 tiles of 32 x 32 with remainders | tiled(unsplit): 1200
  (   1, 70, 60,   9)  fwd<1, 1>: 9 x 8 tiles | cross_bwd_plain_kernel<float, 0>: the factor tables (84 KB) exceed LDS; the reference's expression
                       in the reference's order: bit for bit
 dense data only
  ( 520, 24, 24,  34)  fwd<2, 2> | tiled(unsplit): 1040
  (1024,  8,  8,  50)  image<1, 1> | tiled(unsplit)

A documented difference (test_scale_extremes): the factor form computes T / n0^2 per pair; with |q| below 2^-64 that quotient
leaves fp32's range although the reference's q T / n0^2 does not.  cosine_math.h states the factor form "a few ulp from the
reference's expression": that holds for normal n0^2 and 1 / n0 / n1, which is every row of the data the layer is fed
(GloVe rows have norms of order 1 to 10).  At the extremes the factor-form kernels are held to the forward only.
"""
import numpy as np
import pytest
import torch

import cosine_model as cm
from util import assert_bitexact, rng

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e33
PAD = 64          # floats on each side of an output: keeps the output's own alignment


def dev(x, off=0):
    """x on the device; off > 0: inside a larger buffer, `off` floats past its (aligned) start."""
    if x is None:
        return None
    t = torch.from_numpy(np.array(x, copy=True, order="C")).cuda()
    if off == 0:
        return t
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(*t.shape)
    v.copy_(t)
    return v


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output allocated inside a larger buffer filled with a sentinel; off: floats of misalignment."""

    def __init__(self, shape, off=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lo = PAD + off
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        self.t.fill_(float("nan"))
        self.n = n

    def intact(self):
        b = host(self.buf)
        return bool((b[:self.lo] == np.float32(SENTINEL)).all() and (b[self.lo + self.n:] == np.float32(SENTINEL)).all())


def outputs(q, a, off=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    off = off or {}
    return dict(top=Guarded((N, 1, W1, W2)), n0=Guarded((N, W1)), n1=Guarded((N, W2)),
                dq=Guarded(q.shape, off.get("dq", 0)), da=Guarded(a.shape, off.get("da", 0)))


def finish(out, names, what):
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside %s" % (what, k)
    for k in set(out) - set(names):
        assert np.isnan(host(out[k].t)).all(), "%s: %s was written by a call that does not own it" % (what, k)
    return {k: host(out[k].t).copy() for k in names}


def forward(capi, q, a, off=None, what=""):
    off = off or {}
    out = outputs(q, a, off)
    capi.simcross_forward(0, dev(q, off.get("q", 0)), dev(a, off.get("a", 0)), out["top"].t, norm0=out["n0"].t, norm1=out["n1"].t)
    return finish(out, ("top", "n0", "n1"), what + " forward")


def backward(capi, q, a, fw, dT, off=None, what="", propagate_down=(True, True)):
    """The backward from the forward results fw = dict(top, n0, n1) (host arrays)."""
    off = off or {}
    out = outputs(q, a, off)
    capi.simcross_backward(0, dev(q, off.get("q", 0)), dev(a, off.get("a", 0)), dev(fw["top"]), dev(dT), out["dq"].t, out["da"].t,
                           norm0=dev(fw["n0"]), norm1=dev(fw["n1"]), propagate_down=propagate_down)
    return finish(out, ("dq", "da"), what + " backward")


def fused(capi, q, a, dT, off=None, what=""):
    off = off or {}
    out = outputs(q, a, off)
    capi.simcross_forward_backward(0, dev(q, off.get("q", 0)), dev(a, off.get("a", 0)), dev(dT), out["top"].t, out["dq"].t,
                                   out["da"].t, norm0=out["n0"].t, norm1=out["n1"].t)
    return finish(out, ("top", "n0", "n1", "dq", "da"), what + " fused")


def assert_same(got, want, names, what):
    for k in names:
        assert_bitexact(got[k], want[k], "%s: %s" % (what, k))


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact-sum probes on every route
# ----------------------------------------------------------------------------------------------------------------------
def check_probe(capi, p, shape, off=None, factor_form=None, what=None):
    """Forward bit for bit; dq from dT_rows and da from dT_cols (bit for bit, or BAR_GRAD for the factor form); the fused call
    and a second call give the same bits."""
    what = what or "%s" % (shape,)
    factor_form = (tuple(shape) in cm.FACTOR_FORM) if factor_form is None else factor_form
    fw = forward(capi, p["q"], p["a"], off, what)
    assert_same(fw, p, ("top", "n0", "n1"), what + " forward against the oracle")
    for name, dT in (("dq", "dT_rows"), ("da", "dT_cols")):
        if name == "da" and p["dT_cols"] is p["dT_rows"]:
            break
        bw = backward(capi, p["q"], p["a"], fw, p[dT], off, what)
        for k in ("dq", "da") if p["dT_cols"] is p["dT_rows"] else (name,):
            if factor_form:
                cm.check("%s %s" % (what, k), bw[k], *p[k + "_ref"], cm.BAR_GRAD)
            else:
                assert_bitexact(bw[k], p[k + "_o"], "%s %s against the oracle" % (what, k))
        fu = fused(capi, p["q"], p["a"], p[dT], off, what)
        assert_same(fu, fw, ("top", "n0", "n1"), what + " fused against forward")
        assert_same(fu, bw, ("dq", "da"), what + " fused against backward (%s)" % dT)
        assert_same(fused(capi, p["q"], p["a"], p[dT], off, what), fu, ("top", "n0", "n1", "dq", "da"), what + " second fused call")
    return fw


@pytest.mark.parametrize("shape", cm.ROUTES, ids=cm.shape_id)
def test_probe_every_route(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    check_probe(capi, cm.probe_case(oracle, shape), shape)


@pytest.mark.parametrize("which", ["q", "a", "dq", "da"])
@pytest.mark.parametrize("shape", [(5, 1, 1, 100), (6, 1, 1, 300), (7, 1, 1, 304)], ids=cm.shape_id)
def test_misaligned_views(shape, which, oracle, hiplib):
    """One operand at a time one float past a 16-byte boundary: pair32 and vec4 are both declined where that operand is used
    (the forward looks at q and a only), the scalar rows kernel runs, and every result is the oracle's bit for bit."""
    from mms_answer_selection_amd import capi
    check_probe(capi, cm.probe_case(oracle, shape), shape, off={which: 1}, factor_form=False, what="%s, %s offset" % (shape, which))


@pytest.mark.parametrize("shape", [(31, 1, 1, 200), (9, 1, 1, 256), (7, 1, 1, 304), (3, 1, 1, 1024), (5, 1, 1, 8)], ids=cm.shape_id)
def test_fp16_storage_forward_has_the_same_bits(shape, oracle, hiplib):
    """Small integers are exact as halves: mms_simcross_cosine_forward_f16 (D % 8 == 0) on the same data gives the bits of the
    fp32 call; with the norms omitted (the ABI allows null there) top keeps its bits."""
    from mms_answer_selection_amd import capi
    N, _, _, D = shape
    p = cm.probe_inputs(rng(cm.shape_seed(shape)), *shape)
    qh, ah = p["q"].astype(np.float16), p["a"].astype(np.float16)
    assert (qh.astype(np.float32) == p["q"]).all() and (ah.astype(np.float32) == p["a"]).all()
    top_o, n0_o, n1_o = oracle.simcross_forward(0, p["q"], p["a"])
    fw = forward(capi, p["q"], p["a"], what="%s" % (shape,))
    out = outputs(p["q"], p["a"])
    capi.simcross_cosine_forward_f16(dev(qh), dev(ah), out["top"].t, norm0=out["n0"].t, norm1=out["n1"].t)
    h = finish(out, ("top", "n0", "n1"), "f16 forward %s" % (shape,))
    assert_same(h, fw, ("top", "n0", "n1"), "f16 against f32 %s" % (shape,))
    assert_same(h, dict(top=top_o, n0=n0_o, n1=n1_o), ("top", "n0", "n1"), "f16 against the oracle %s" % (shape,))
    out = outputs(p["q"], p["a"])
    capi.simcross_cosine_forward_f16(dev(qh), dev(ah), out["top"].t)
    assert_bitexact(finish(out, ("top",), "f16 forward without norms")["top"], h["top"], "top without norms")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(4, 5, 7, 300), (1030, 40, 40, 52), (1025, 16, 24, 50), (1023, 16, 24, 50), (3, 41, 9, 33)],
                         ids=cm.shape_id)
def test_embed_fused_forward_bit_for_bit(shape, bias, oracle, hiplib):
    """mms_embed_simcross_forward_f32, mode 0: the gather (and the Embed bias, chosen so that bias + table stays a small integer)
    feeds the same exact sums through row_norm_kernel and the gathering loads of cross_fwd_kernel / cross_fwd_image_kernel."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D = shape
    r = rng(cm.shape_seed(shape) + int(bias))
    K = 37
    table = cm.exact_rows(r, K, D, 0, 5, 2)                         # integers in [-4, 4]
    b = r.integers(-3, 4, D).astype(np.float32) if bias else None     # |bias + table| <= 7: squares sum below 49 D < 2^24
    iq = r.integers(0, K, (N, W1)).astype(np.float32)
    ia = r.integers(0, K, (N, W2)).astype(np.float32)
    rows = table if b is None else (b[None, :] + table)
    q, a = rows[iq.astype(np.int64)], rows[ia.astype(np.int64)]
    top_o, n0_o, n1_o = oracle.simcross_forward(0, q, a)
    out = outputs(q, a)
    capi.embed_simcross_forward(0, dev(iq), dev(ia), dev(table), out["top"].t, norm0=out["n0"].t, norm1=out["n1"].t, embed_bias=dev(b))
    got = finish(out, ("top", "n0", "n1"), "embed + simcross %s" % (shape,))
    assert_same(got, dict(top=top_o, n0=n0_o, n1=n1_o), ("top", "n0", "n1"), "embed + simcross %s bias=%s" % (shape, bias))
    if not bias:
        assert_same(got, forward(capi, q, a), ("top", "n0", "n1"), "embed + simcross against simcross %s" % (shape,))


# one shape per family: pair32 (NIT 2, 3), rows vec4, rows scalar, tiled split, tiled unsplit + 2 x 2 tiles, image, generic backward
SCALED = [(31, 1, 1, 200), (33, 1, 1, 300), (9, 1, 1, 260), (6, 1, 1, 65), (3, 41, 9, 33), (520, 24, 24, 34), (1024, 8, 8, 50), (1, 70, 60, 9)]


@pytest.mark.parametrize("shape", SCALED, ids=cm.shape_id)
def test_power_of_two_scaling_changes_no_bit(shape, hiplib):
    """q x 2^s, a x 2^t on dense data, nothing leaving the normal range: top keeps its bits, norm0 x 2^s, norm1 x 2^t, dq x 2^-s,
    da x 2^-t exactly -- in any summation order, and through the factors 1 / n0 / n1 and T / n^2 too."""
    from mms_answer_selection_amd import capi
    q, a, dT = cm.dense_inputs(rng(cm.shape_seed(shape) + 3), *shape)
    base = fused(capi, q, a, dT)
    for s, t in ((7, -5), (-12, 9), (20, 20)):
        qs, as_ = cm.ldexp32(q, s), cm.ldexp32(a, t)
        want = dict(top=base["top"], n0=cm.ldexp32(base["n0"], s), n1=cm.ldexp32(base["n1"], t), dq=cm.ldexp32(base["dq"], -s),
                    da=cm.ldexp32(base["da"], -t))
        n0s, n1s = want["n0"].astype(np.float64), want["n1"].astype(np.float64)
        for x in (qs, as_, qs.astype(np.float64) ** 2, as_.astype(np.float64) ** 2, n0s ** -2, n1s ** -2,
                  1.0 / (n0s[:, :, None] * n1s[:, None, :])) + tuple(want.values()):
            assert cm.all_normal(x), "a scaled value left the normal range"
        assert_same(fused(capi, qs, as_, dT), want, ("top", "n0", "n1", "dq", "da"), "%s scaled by 2^%d, 2^%d" % (shape, s, t))


# ----------------------------------------------------------------------------------------------------------------------
# 3. dense data against fp64
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cm.DENSE, ids=cm.shape_id)
def test_dense_error_within_twice_the_references(shape, oracle, hiplib):
    """e(kernel) <= 2 e(CPU oracle) + 4 x 2^-24 for top, dq and da, each element at its own scale (cosine_model.dense_case); the
    backward is given the oracle's fp32 forward, as the fp64 reference is.  The fused call from the kernel's own forward gives
    the bits of the two calls.  Measured ratios: profiles/cosine_routes.txt."""
    from mms_answer_selection_amd import capi
    c = cm.dense_case(oracle, shape)
    fw = forward(capi, c["q"], c["a"])
    got = dict(fw, **backward(capi, c["q"], c["a"], dict(top=c["top"], n0=c["n0"], n1=c["n1"]), c["dT"]))
    fails = []
    for name in ("top", "dq", "da"):
        ek, idx = cm.scaled_error(got[name], *c["ref"][name])
        eo = c["e_o"][name]
        msg = "%s %s: e(kernel) = %.2f, e(oracle) = %.2f, bar %.2f (x 2^-24), worst at %s" % (
            name, cm.shape_id(shape), ek / cm.U24, eo / cm.U24, cm.dense_bar(eo) / cm.U24, idx)
        print(msg)
        if not ek <= cm.dense_bar(eo):
            fails.append(msg)
    # the norms are square roots of one sum each: same bar as top's, relative
    for name, x in (("n0", c["q"]), ("n1", c["a"])):
        n64 = np.sqrt((x.astype(np.float64) ** 2).sum(-1))
        ek, eo = cm.scaled_error(got[name], n64, n64)[0], cm.scaled_error(c[name], n64, n64)[0]
        print("%s %s: e(kernel) = %.2f, e(oracle) = %.2f (x 2^-24)" % (name, cm.shape_id(shape), ek / cm.U24, eo / cm.U24))
        if not ek <= cm.dense_bar(eo):
            fails.append("%s: %.3g > bar(%.3g)" % (name, ek, eo))
    assert not fails, "; ".join(fails)
    fu = fused(capi, c["q"], c["a"], c["dT"])
    assert_same(fu, fw, ("top", "n0", "n1"), "%s fused against forward" % (shape,))
    assert_same(fu, backward(capi, c["q"], c["a"], fw, c["dT"]), ("dq", "da"), "%s fused against backward" % (shape,))


# ----------------------------------------------------------------------------------------------------------------------
# 4. edges
# ----------------------------------------------------------------------------------------------------------------------
# pair32 (ragged N), rows vec4, rows scalar, tiled split, tiled unsplit, generic backward
EDGE = [(17, 1, 1, 100), (33, 1, 1, 300), (9, 1, 1, 260), (6, 1, 1, 65), (3, 41, 9, 33), (512, 8, 8, 50), (3, 70, 60, 9)]


def oracle_all(oracle, q, a, dT):
    with np.errstate(all="ignore"):
        top, n0, n1 = oracle.simcross_forward(0, q, a)
        dq, da, _, _ = oracle.simcross_backward(0, q, a, top, dT, norm0=n0, norm1=n1)
    return dict(top=top, n0=n0, n1=n1, dq=dq, da=da)


def check_spoilt_pairs(capi, oracle, shape, q, a, dT, qb, ab, pairs, what):
    """Pairs `pairs` of (qb, ab) differ from (q, a): non-finiteness is the oracle's element for element, the forward of the
    spoilt pairs is the oracle's bit for bit (exact sums), and every other pair keeps the bits of the clean run."""
    clean, got, want = fused(capi, q, a, dT), fused(capi, qb, ab, dT), oracle_all(oracle, qb, ab, dT)
    others = np.ones(shape[0], bool)
    others[list(pairs)] = False
    for k in ("top", "n0", "n1", "dq", "da"):
        assert (np.isnan(got[k]) == np.isnan(want[k])).all(), "%s %s: the NaNs are not where the oracle has them" % (what, k)
        assert (np.isinf(got[k]) == np.isinf(want[k])).all(), "%s %s: the Infs are not where the oracle has them" % (what, k)
        assert np.isfinite(got[k][others]).all(), "%s %s: another pair is not finite" % (what, k)
        assert_bitexact(got[k][others], clean[k][others], "%s %s: the other pairs" % (what, k))
    assert_same(got, want, ("top", "n0", "n1"), what + " forward against the oracle")
    assert not np.isfinite(got["top"][list(pairs)]).all(), what + ": the case spoils nothing"
    two = forward(capi, qb, ab)
    assert_same(dict(two, **backward(capi, qb, ab, two, dT)), got, ("top", "n0", "n1", "dq", "da"), what + " two calls against fused")


@pytest.mark.parametrize("shape", EDGE, ids=cm.shape_id)
def test_zero_rows(shape, oracle, hiplib):
    """The zero-pad word: a zero q row, a zero a row, and both (in different pairs; on a grid one word of the pair, i.e. one
    row / one column of top).  The reference divides by the norm with no epsilon: 0 / 0 = NaN exactly where the CPU has it."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D = shape
    p = cm.probe_inputs(rng(cm.shape_seed(shape) + 41), *shape)
    dT = cm.g_values(rng(5), (N, 1, W1, W2))
    qb, ab = p["q"].copy(), p["a"].copy()
    pairs = sorted({0, N // 2, N - 1})
    qb[pairs[0], W1 - 1] = 0
    ab[pairs[-1], 0] = 0
    qb[pairs[len(pairs) // 2], 0] = 0
    ab[pairs[len(pairs) // 2], W2 // 2] = 0
    check_spoilt_pairs(capi, oracle, shape, p["q"], p["a"], dT, qb, ab, pairs, "%s zero rows" % (shape,))


@pytest.mark.parametrize("shape", EDGE, ids=cm.shape_id)
def test_inf_and_nan_stay_in_their_pair(shape, oracle, hiplib):
    from mms_answer_selection_amd import capi
    N, W1, W2, D = shape
    p = cm.probe_inputs(rng(cm.shape_seed(shape) + 43), *shape)
    dT = cm.g_values(rng(6), (N, 1, W1, W2))
    qb, ab = p["q"].copy(), p["a"].copy()
    pairs = sorted({N // 3, N - 1})
    qb[pairs[0], W1 // 2, D - 1] = np.inf
    ab[pairs[-1], W2 - 1, 0] = np.nan
    check_spoilt_pairs(capi, oracle, shape, p["q"], p["a"], dT, qb, ab, pairs, "%s Inf / NaN" % (shape,))


@pytest.mark.parametrize("shape", EDGE, ids=cm.shape_id)
def test_scale_extremes(shape, oracle, hiplib):
    """Exact-sum rows scaled so that the squares overflow (2^70: sqq = Inf, T = 0 or NaN), are subnormal (2^-70: the sums stay
    exact multiples of 2^-149 -- a kernel that flushes gives norm 0) or vanish (2^-80: norm 0, T = +-Inf or NaN), one pair
    each in q and in a.  The order-free sums make the oracle's forward the only right answer: bit for bit, like the Euclid
    kernels (tests/test_gpu_parity.py: test_euclid_subnormal_squares, "must not flush").  The backward is held to the
    oracle's bits where the kernel spells the reference's expression; the factor form is a documented difference here (see the
    module docstring) and is held to the forward alone."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D = shape
    r = rng(cm.shape_seed(shape) + 47)
    q = cm.exact_rows(r, N * W1, D, 0, 5, 2).reshape(N, W1, D)
    a = cm.exact_rows(r, N * W2, D, 0, 7, 3).reshape(N, W2, D)
    dT = cm.g_values(rng(7), (N, 1, W1, W2), -1, 1)
    for e in (70, -70, -80):
        qb, ab = q.copy(), a.copy()
        qb[0] = cm.ldexp32(q[0], e)
        ab[N - 1] = cm.ldexp32(a[N - 1], e)
        if N > 2:
            qb[1], ab[1] = cm.ldexp32(q[1], e), cm.ldexp32(a[1], e)
        want = oracle_all(oracle, qb, ab, dT)
        if e == -70:
            assert (want["n0"][0] > 0).all() and ((qb[0].astype(np.float64) ** 2).sum(-1) < 2.0 ** -126).all(), "subnormal sums"
        got = fused(capi, qb, ab, dT)
        names = ("top", "n0", "n1") if tuple(shape) in cm.FACTOR_FORM else ("top", "n0", "n1", "dq", "da")
        assert_same(got, want, names, "%s rows scaled by 2^%d" % (shape, e))


def test_optional_arguments(oracle, hiplib):
    """include/mms.h: the cosine calls need norm0 and norm1 (MMS_ERR_INVALID_ARG without, nothing written), and the backward
    needs dq and da whatever propagate_down says -- sim_cross_layer.cpp:176-201 zeroes both and computes both if either flag is
    set: (1, 0) and (0, 1) give the bits of (1, 1), (0, 0) gives zeros."""
    from mms_answer_selection_amd import capi
    for shape in [(17, 1, 1, 100), (9, 1, 1, 260), (3, 41, 9, 33)]:
        p = cm.probe_case(oracle, shape)
        fw = dict(top=p["top"], n0=p["n0"], n1=p["n1"])
        both = backward(capi, p["q"], p["a"], fw, p["dT_rows"])
        for pd in ((True, False), (False, True)):
            assert_same(backward(capi, p["q"], p["a"], fw, p["dT_rows"], propagate_down=pd), both, ("dq", "da"), "%s propagate_down %s" % (shape, pd))
        none = backward(capi, p["q"], p["a"], fw, p["dT_rows"], propagate_down=(False, False))
        assert not none["dq"].any() and not none["da"].any()
        for call in ("forward", "fused"):
            out = outputs(p["q"], p["a"])
            with pytest.raises(capi.MMSError):
                if call == "forward":
                    capi.simcross_forward(0, dev(p["q"]), dev(p["a"]), out["top"].t, norm0=out["n0"].t)
                else:
                    capi.simcross_forward_backward(0, dev(p["q"]), dev(p["a"]), dev(p["dT_rows"]), out["top"].t, out["dq"].t, out["da"].t,
                                                   norm1=out["n1"].t)
            finish(out, (), "%s refused %s" % (shape, call))
