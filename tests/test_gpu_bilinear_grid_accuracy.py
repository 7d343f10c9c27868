"""The bilinear SimCross layer on word grids (csrc/bilinear.hip, dist_mode 2) held to fp64, componentwise, on every kernel route.

tests/test_gpu_parity.py compares these paths with the fp32 CPU oracle at 1e-5 of the LARGEST element of an array, on data of
one magnitude, with an N(0, 1) bias on scores of size 0.4: a score wrong by 2^-13 of its non-bias part passes, and a small
dq / da row or dW entry is hardly checked.  Here (tests/bilinear_grid_model.py has the constructions and the bars):

  * single-product probes -- every element of top, dq, da and dW is ONE fp32 product (dq, da: one per measure) against fp64
    at a bar COUNTED from the roundings on its path: top (2 + 9/8 with bias) x 2^-24, dq and da M x 2^-24, dW 2^-24; dbias
    bit for bit.  Every k, j, word row and measure carries its own value, so a failure names the index that went wrong;
  * dense data -- within twice the CPU oracle's own componentwise error, and power-of-two scaling changes no bit;
  * edges -- no store outside an output, two calls give the same bits, a NaN / Inf in one pair stays in that pair.

Route table: (N, W1, W2, D, M, bias_term) -> forward route | backward route, read off bilinear_forward, pair_fwd_launch,
bilinear_backward, pair_bwd_eligible, gemm_launch, gemm_fast_variant, gemm_launch_group and pick_ksplit.  fast<FK, VW> =
gemm32_fast_kernel (FK 32 = "deep", a grid of at most 512 workgroups), group<FK, VW> = gemm32_group_kernel, generic =
gemm32_kernel; s1 / s2 = the two GEMMs of the generic forward; reduce(n) = ordered_slab_sum over n slabs (batches of 8 up to
eight slabs, of 32 above).  profiles/bilinear_grid_routes.txt records the kernels a trace of this file saw per test id (it agrees
with every row; the last slice of a sliced launch is small and runs the deep variant).

 fused forward, one workgroup per pair (N >= 512); backward generic
  (512, 48,  5, 52, 1, T)  pair_fwd<13>: D = 52, W1 = 48, W2 % 16 != 0 | dbias_chain; U, V generic (W2 odd); dq/da/dW group<16,4>
                           (680 workgroups, ksplit 256 > 8 slabs); splitk_reduce
  (512,  3, 48, 53, 2, F)  pair_fwd<16>: D = 53, W2 = 48 | odd D: every product generic; M > 1 stacked; reduce group (2, 24)
  (513, 17, 40, 64, 3, T)  pair_fwd<16>: D = 64 | dbias_kernel (per_n 2040); U fast<16,4> 1539 workgroups (group DECLINED: > 1536),
                           V generic (W1 odd); dq fast<32,4>, da fast<16,4>, dW generic (K = N W1 odd)
 fused forward and backward, one workgroup per (pair, measure) (N <= 256, N M <= 65535)
  (  1, 40, 40, 52, 1, T)  pairm_fwd<13> | pair_bwd<10,13> at both limits, M = 1: dq / da direct; N = ksplit = 1; reduce(1)
  (  2, 40,  3, 50, 1, F)  pairm_fwd<13> | pair_bwd<10,13>; N = ksplit = 2 (workspace slabs sized by ksplit); reduce(2)
  (  8, 41,  7, 52, 2, T)  pairm_fwd<13> | pair_bwd<12,16> (W1 = 41: one past <10,13>), M > 1: partials + grouped reduce(2), (8)
  (  9,  5, 40, 53, 1, F)  pairm_fwd<16> (D = 53) | pair_bwd<12,16> (D = 53: one past), M = 1; reduce(9): first batch of 32
  ( 32, 48, 48, 64, 1, T)  pairm_fwd<16> at both limits | pair_bwd<12,16> at both limits, M = 1; reduce(32): one full batch
  ( 33, 16, 33, 64, 4, T)  pairm_fwd<16> | pair_bwd<12,16>, M > 1; reduce(33): a second batch of one slab
  (256,  2,  3,  8, 2, T)  pairm_fwd<13> at N = 256 | pair_bwd<10,13>, M > 1; reduce(256)
 generic forward and backward: N between the fused kernels
  (257,  3,  2,  8, 1, T)  s1, s2 fast<32,4> | dbias_chain; U fast<32,2>, V generic; dq, da fast<32,4>, dW generic; splitk_reduce(7)
  (511,  2,  2,  6, 2, F)  s1 fast<32,2>, s2 fast<16,2> (1022 workgroups: not deep) | U, V group<16,2> (2044 workgroups: TAKEN);
                           dq/da/dW group<32,2> stacked over M, ksplit 16; reduce group
 generic: one past the fused kernels' W and D
  (  3, 49,  4, 52, 1, T)  W1 = 49: s1, s2 fast<32,4> | dbias_chain; U fast, V generic; dq, da fast<32,4>, dW generic; ksplit 3 = N
  (  2,  4, 49, 52, 2, T)  W2 = 49 | dbias_kernel (per_n 392); U, V generic; dq/da/dW group<32,4>, ksplit 1
  (  5,  7,  6, 65, 2, T)  D = 65: gemm32_kernel everywhere, forward and backward | dbias_chain; M > 1
  (  3,  5,  4, 66, 1, T)  D = 66 (D % 4 == 2): fast<32,2> | U fast<32,2>, V generic, dq, da fast<32,2>, dW generic
  ( 40,  9,  5, 68, 1, F)  D = 68: fast<32,4> | U, V generic; dq/da/dW group<32,4>, ksplit 6; splitk_reduce(6)
  (  5, 40, 40, 68, 1, T)  D = 68 at the driver's grid | dbias_kernel (per_n 1600); U, V group<32,4> TAKEN; dq/da/dW group<32,4>
  (400,  8,  8, 72, 4, T)  s1 fast<32,4>, s2 fast<16,4> (1600) | U, V fast<16,4> 3200 workgroups each (group DECLINED);
                           dq/da/dW group<16,4> 1344 workgroups, stacked, ksplit 34 (> 8 slabs, two batches of 32)
  (5600, 8,  8, 68, 1, F)  dq 1400, da 1400, dW 700 workgroups: each within 1536, together 3500 > 3072: group DECLINED on the total;
                           dq, da, dW fast<16,4>, ksplit 175; U, V fast<16,4> 11200 each; splitk_reduce(175)
 generic: gridDim.z sliced (pairs x measures > 65535)
  (16385, 2, 1, 68, 4, T)  s2 sliced at z = 65532 | U, V generic and sliced; dq, da fast<16,4> (4104 workgroups: g3 group DECLINED),
                           dW fast<16,2>, ksplit 47
  (256,  2,  2,  4, 256, T) N M = 65536: one past pairm_fwd; s2 sliced at z = 65280 | dbias_kernel; U, V fast<16,2> sliced;
                           stacked split over 256 measures; reduce(256)
 one word per sentence, several measures
  (300,  1,  1, 24, 3, T)  s1 fast<32,4>, rowdot_kernel per measure | dbias_chain (per_n 3); U, V generic; dq/da/dW group<32,4>
 (W1 = W2 = M = 1 is SimMatrix's route: tests/test_gpu_matrix_pipe_accuracy.py; its dbias_scalar_kernel is checked below.)
"""
import numpy as np
import pytest
import torch

import bilinear_grid_model as bg
import matrix_pipe_model as mp
from util import assert_bitexact, rng

pytestmark = pytest.mark.gpu

T, F = True, False
SHAPES = [
    (512, 48, 5, 52, 1, T), (512, 3, 48, 53, 2, F), (513, 17, 40, 64, 3, T),
    (1, 40, 40, 52, 1, T), (2, 40, 3, 50, 1, F), (8, 41, 7, 52, 2, T), (9, 5, 40, 53, 1, F), (32, 48, 48, 64, 1, T),
    (33, 16, 33, 64, 4, T), (256, 2, 3, 8, 2, T),
    (257, 3, 2, 8, 1, T), (511, 2, 2, 6, 2, F),
    (3, 49, 4, 52, 1, T), (2, 4, 49, 52, 2, T), (5, 7, 6, 65, 2, T), (3, 5, 4, 66, 1, T), (40, 9, 5, 68, 1, F),
    (5, 40, 40, 68, 1, T), (400, 8, 8, 72, 4, T), (5600, 8, 8, 68, 1, F),
    (16385, 2, 1, 68, 4, T), (256, 2, 2, 4, 256, T),
    (300, 1, 1, 24, 3, T),
]
# one shape per route family for the dense-data tests: fused forward per pair (backward generic, grouped); fused forward and
# backward <10,13> and <12,16>; generic fast (vw 4, stacked), generic gemm32_kernel (odd D), generic vw 2
DENSE = [(512, 7, 9, 52, 2), (33, 40, 40, 50, 4), (9, 41, 7, 53, 2), (300, 6, 5, 68, 2), (40, 9, 5, 65, 1), (511, 2, 2, 6, 2)]

SENTINEL = -7.25e33
PAD = 64          # floats on each side of an output: keeps the output's own alignment


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output allocated inside a larger buffer filled with a sentinel."""

    def __init__(self, shape, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.t.fill_(float("nan"))
        if init is not None:
            self.t.copy_(dev(init))
        self.n = n

    def intact(self):
        b = host(self.buf)
        return bool((b[:PAD] == np.float32(SENTINEL)).all() and (b[PAD + self.n:] == np.float32(SENTINEL)).all())


def run_layer(capi, q, a, W, bias, dT, dbias0=None, forward=True):
    """One forward and one backward call, every output guarded.  Returns the host arrays and asserts the guards."""
    N, W1, D = q.shape
    W2, M = a.shape[1], W.shape[0]
    qd, ad, Wd = dev(q), dev(a), dev(W)
    out = dict(top=Guarded((N, M, W1, W2)), dq=Guarded(q.shape), da=Guarded(a.shape), dW=Guarded(W.shape))
    if bias is not None:
        out["dbias"] = Guarded((M, W1, W2), init=dbias0 if dbias0 is not None else np.zeros((M, W1, W2), np.float32))
    if forward:
        capi.simcross_forward(2, qd, ad, out["top"].t, W=Wd, bias=dev(bias))
    capi.simcross_backward(2, qd, ad, out["top"].t, dev(dT), out["dq"].t, out["da"].t, W=Wd, bias_term=bias is not None,
                           dW=out["dW"].t, dbias=out["dbias"].t if bias is not None else None)
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.intact(), "%s: a store landed outside the output (shape %s)" % (k, (N, W1, W2, D, M))
    return {k: host(g.t).copy() for k, g in out.items()}


# ----------------------------------------------------------------------------------------------------------------------
# 2. single-product probes on every route
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_probe_every_route(shape, hiplib):
    """Three calls per shape (bilinear_grid_model.probe_inputs): forward + backward with dT one per row (top, dq, dbias), backward
    with dT one per column (da), backward with q one per column and a dense (dW).  Bars: bilinear_grid_model, counted roundings."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M, bias_term = shape
    p = bg.probe_inputs(rng(sum(shape[:5]) + 17), *shape)
    what = "%s " % (shape,)
    g = run_layer(capi, p["q"], p["a"], p["W"], p["bias"], p["dT_rows"], p["dbias0"])
    bg.check(what + "top", g["top"], bg.ref_top(p["q"], p["a"], p["W"], p["bias"]), bg.bar_top(bias_term))
    bg.check(what + "dq", g["dq"], bg.ref_dq(p["a"], p["W"], p["dT_rows"]), bg.bar_dq(M))
    if bias_term:
        assert_bitexact(g["dbias"], bg.dbias_in_order(p["dT_rows"], p["dbias0"]), what + "dbias (n ascending)")
    g = run_layer(capi, p["q"], p["a"], p["W"], p["bias"], p["dT_cols"], p["dbias0"], forward=False)
    bg.check(what + "da", g["da"], bg.ref_da(p["q"], p["W"], p["dT_cols"]), bg.bar_da(M))
    if bias_term:
        assert_bitexact(g["dbias"], bg.dbias_in_order(p["dT_cols"], p["dbias0"]), what + "dbias, second call")
    g = run_layer(capi, p["q_cols"], p["a_dense"], p["W"], p["bias"], p["dT_rows"], p["dbias0"], forward=False)
    bg.check(what + "dW", g["dW"], bg.ref_dW(p["q_cols"], p["a_dense"], p["dT_rows"]), bg.BAR_DW)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 300])
def test_dbias_of_one_scalar_bias(N, hiplib):
    """per_n == 1 (W1 = W2 = M = 1): dbias_scalar_kernel, 64 terms per load and 256 per round -- both edges; bit for bit."""
    from mms_answer_selection_amd import capi
    r = rng(N)
    q, a, W, dT = bg.dense_inputs(r, N, 1, 1, 20, 1)
    db0 = np.full((1, 1, 1), 0.375, np.float32)
    g = run_layer(capi, q, a, W, np.zeros((1, 1, 1), np.float32), dT, db0)
    assert_bitexact(g["dbias"], bg.dbias_in_order(dT, db0), "dbias N=%d" % N)


# ----------------------------------------------------------------------------------------------------------------------
# 3. dense data
# ----------------------------------------------------------------------------------------------------------------------
def dense_refs(q, a, W, dT, bias=None):
    return dict(top=bg.ref_top(q, a, W, bias), dq=bg.ref_dq(a, W, dT), da=bg.ref_da(q, W, dT), dW=bg.ref_dW(q, a, dT))


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "x".join(str(v) for v in s))
def test_dense_error_within_twice_the_references(shape, positive, oracle, hiplib):
    """e(kernel) <= 2 e(CPU oracle) + 2^-24 for top, dq, da and dW, componentwise against fp64, on the suite's dense data and on
    an all-positive variant (no cancellation: errors add up); dbias bit for bit.  The measured values are in DESIGN.md (Numerics)."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = shape
    r = rng(sum(shape) + 13 + int(positive))
    q, a, W, dT = bg.dense_inputs(r, N, W1, W2, D, M, positive)
    bias = np.zeros((M, W1, W2), np.float32)          # the products alone: a bias of the scores' size would hide their error
    db0 = r.standard_normal((M, W1, W2)).astype(np.float32)
    g = run_layer(capi, q, a, W, bias, dT, db0)
    top_o, _, _ = oracle.simcross_forward(2, q, a, W, bias)
    dq_o, da_o, dW_o, db_o = oracle.simcross_backward(2, q, a, top_o, dT, W=W, bias_term=True, dbias_in=db0)
    o = dict(top=top_o, dq=dq_o, da=da_o, dW=dW_o)
    assert_bitexact(g["dbias"], db_o, "dbias %s" % (shape,))
    fails = []
    for name, ref in dense_refs(q, a, W, dT).items():
        ek = mp.componentwise_error(g[name], ref[0], ref[1], name)[0]
        eo = mp.componentwise_error(o[name], ref[0], ref[1], name)[0]
        msg = "%s %s%s: e(kernel) = %.3g, e(oracle) = %.3g" % (name, shape, " positive" if positive else "", ek, eo)
        print(msg)
        if not ek <= 2.0 * eo + 2.0 ** -24:
            fails.append(msg)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "x".join(str(v) for v in s))
def test_dense_power_of_two_scaling_changes_no_bit(shape, hiplib):
    """q column k up by 2^s_k and W row k down, W column j up by 2^c_j and a column j down, q word rows up by 2^r and the
    matching dT rows down (exponents within +-20): top, dq, da and dW are the unscaled results times the corresponding
    power of two, bit for bit."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = shape
    r = rng(sum(shape) + 11)
    q, a, W, dT = bg.dense_inputs(r, N, W1, W2, D, M)
    sc = bg.scaling(r, N, W1, W2, D)
    qs, as_, Ws, dTs = bg.scale_inputs(q, a, W, dT, sc)
    for x in (qs, as_, Ws, dTs):
        assert bg.all_normal(x), "a scaled input left the normal range"
    refs_s = dense_refs(qs, as_, Ws, dTs)
    for k, (c64, dm) in refs_s.items():
        assert bg.all_normal(c64) and bg.all_normal(dm), "the fp64 prediction of the scaled %s leaves the normal range" % k
    base = run_layer(capi, q, a, W, None, dT)
    got = run_layer(capi, qs, as_, Ws, None, dTs)
    want = dict(zip(("top", "dq", "da", "dW"), bg.scale_outputs(base["top"], base["dq"], base["da"], base["dW"], sc)))
    for k in ("top", "dq", "da", "dW"):
        assert_bitexact(got[k], want[k], "%s %s under scaling" % (k, shape))


# ----------------------------------------------------------------------------------------------------------------------
# 4. edges
# ----------------------------------------------------------------------------------------------------------------------
# partial tiles in every dimension: fused forward and backward; fused per-pair forward + generic backward; gemm32_kernel; fast
@pytest.mark.parametrize("shape", [(9, 41, 7, 53, 2), (513, 17, 5, 53, 2), (40, 9, 5, 65, 2), (300, 6, 5, 68, 2)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_no_stray_stores_and_two_calls_agree(shape, hiplib):
    """Every output sits inside a sentinel-filled buffer (run_layer asserts the sentinel after the calls); a second forward +
    backward into fresh buffers gives the same bits."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = shape
    r = rng(sum(shape) + 5)
    q, a, W, dT = bg.dense_inputs(r, N, W1, W2, D, M)
    bias = r.standard_normal((M, W1, W2)).astype(np.float32)
    db0 = r.standard_normal((M, W1, W2)).astype(np.float32)
    one = run_layer(capi, q, a, W, bias, dT, db0)
    two = run_layer(capi, q, a, W, bias, dT, db0)
    for k in one:
        assert np.isfinite(one[k]).all(), "%s %s: an element was not written" % (k, shape)
        assert_bitexact(one[k], two[k], "%s %s: two calls" % (k, shape))


# fused forward per pair (backward generic); fused forward and backward per (pair, measure); generic
@pytest.mark.parametrize("shape", [(512, 5, 6, 52, 2), (9, 41, 7, 52, 2), (40, 9, 5, 68, 2)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_non_finite_values_stay_in_their_pair(shape, oracle, hiplib):
    """One NaN and one Inf in q of ONE pair: the non-finite elements of top, dq and da are the oracle's, and every other pair's
    top, dq and da keep the bits of a clean run (the zero-padded LDS images: "steps past the real extent add exact zeros")."""
    from mms_answer_selection_amd import capi
    N, W1, W2, D, M = shape
    r = rng(sum(shape) + 29)
    q, a, W, dT = bg.dense_inputs(r, N, W1, W2, D, M)
    bias = r.standard_normal((M, W1, W2)).astype(np.float32)
    clean = run_layer(capi, q, a, W, bias, dT)
    pair = N // 2
    qb = q.copy()
    qb[pair, 0, D - 1] = np.nan
    qb[pair, W1 - 1, 1] = np.inf
    got = run_layer(capi, qb, a, W, bias, dT)
    top_o, _, _ = oracle.simcross_forward(2, qb, a, W, bias)
    dq_o, da_o, _, _ = oracle.simcross_backward(2, qb, a, top_o, dT, W=W, bias_term=True)
    others = np.arange(N) != pair
    for k, o in (("top", top_o), ("dq", dq_o), ("da", da_o)):
        assert (np.isfinite(got[k]) == np.isfinite(o)).all(), "%s %s: the non-finite elements are not the oracle's" % (k, shape)
        assert_bitexact(got[k][others], clean[k][others], "%s %s: the other pairs" % (k, shape))
    assert not np.isfinite(got["top"][pair]).all() and not np.isfinite(got["da"][pair]).all()


def test_empty_batch_and_short_workspace(hiplib):
    """N = 0 is a no-op on this geometry (nothing is written); a workspace one byte short is refused with MMS_ERR_WORKSPACE."""
    from mms_answer_selection_amd import capi
    W1, W2, D, M = 5, 4, 68, 2
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    gW, gb = Guarded((M, D, D)), Guarded((M, W1, W2))
    capi.simcross_forward(2, e(0, W1, D), e(0, W2, D), e(0, M, W1, W2), W=e(M, D, D), bias=e(M, W1, W2))
    capi.simcross_backward(2, e(0, W1, D), e(0, W2, D), e(0, M, W1, W2), e(0, M, W1, W2), e(0, W1, D), e(0, W2, D), W=e(M, D, D),
                           bias_term=True, dW=gW.t, dbias=gb.t)
    torch.cuda.synchronize()
    assert np.isnan(host(gW.t)).all() and np.isnan(host(gb.t)).all() and gW.intact() and gb.intact()
    lib = capi.lib()
    for N in (3, 40):                                # generic route; and (3, 5, 4, 64) below the fused kernels' limits
        for Dd in (68, 64):
            need = capi.simcross_workspace_bytes(2, N, W1, W2, Dd, M)
            assert need > 0
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            q, a, Wt, top = e(N, W1, Dd).zero_(), e(N, W2, Dd).zero_(), e(M, Dd, Dd).zero_(), Guarded((N, M, W1, W2))
            s = torch.cuda.current_stream().cuda_stream
            args = (2, N, W1, W2, Dd, M, q.data_ptr(), a.data_ptr(), Wt.data_ptr(), None, top.t.data_ptr(), None, None, ws.data_ptr())
            assert lib.mms_simcross_forward_f32(*args, need - 1, s) == 3, "forward: MMS_ERR_WORKSPACE"
            gq, ga = e(N, W1, Dd), e(N, W2, Dd)
            rc = lib.mms_simcross_backward_f32(2, N, W1, W2, Dd, M, q.data_ptr(), a.data_ptr(), Wt.data_ptr(), 0, top.t.data_ptr(),
                                               top.t.data_ptr(), None, None, 1, 1, gq.data_ptr(), ga.data_ptr(), gW.t.data_ptr(),
                                               None, ws.data_ptr(), need - 1, s)
            assert rc == 3, "backward: MMS_ERR_WORKSPACE"
            torch.cuda.synchronize()
            assert np.isnan(host(top.t)).all() and top.intact(), "a refused call wrote nothing"
            assert lib.mms_simcross_forward_f32(*args, need, s) == 0
