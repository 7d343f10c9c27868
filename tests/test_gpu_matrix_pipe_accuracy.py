"""The split-bf16 matrix products (csrc/bx3_gemm.h) held to the accuracy include/mms.h states, componentwise against fp64.

The rest of the suite compares these products at 1e-5 of the LARGEST output, on data of one magnitude: a product that
lost one of its six plane terms (a 2^-18 error) passes it (tests/test_matrix_pipe_model.py keeps that on record).  Here:

  * plane probes -- the streamed operand holds ONE nonzero per output row (for the weight gradient: per column of q),
    its position cycling over every k, every value is built from three populated bf16 planes, so each output element is
    a single fp32 x fp32 product whose six (five for a half operand) plane terms are each >= 0.9 * 2^-18 of it.  Bar:
    e <= 2^-20 (matrix_pipe_model.BAR: derived from the number of fp32 roundings, not measured), e = max |C - C64| / (|A|.|B|);
  * da is not a product but one fp32 multiply of the kernel's own Q.W: bit-exact;
  * dense data of the suite's kind: power-of-two scaling of rows and columns changes no bit, and the error stays within
    2 x the reference's own (the CPU oracle's sgemm, the fp32-MFMA pipe as a second witness).

Every entry point that reaches the bf16 pipe runs in both matrix modes: "fp32" is the other implementation of the same
contract and is held to the same bar.
"""
import numpy as np
import pytest
import torch

import matrix_pipe_model as mp
from matrix_pipe_model import check_probe, diag_of
from util import assert_bitexact, rng

pytestmark = pytest.mark.gpu

# (N, K1, K2).  Forward = bx3_kernel<NTW(K2)> over K1, dq = bx3_kernel<NTW(K1)> over K2, dW = bx3_tn_kernel, K1 x K2 output.
#   (2049, 300, 300): two column groups NTW 5 both ways, K % 16 = 12, ragged last panel (1 row), dW four quadrants
#   (2125, 52, 304):  forward two groups NTW 5, K % 16 = 4; dq NTW 2; dW two quadrants; N % 32 != 0
#   (2049, 64, 160):  forward one group NTW 5; dq NTW 2; dW one quadrant
#   (2048, 24, 8):    NTW 1 both ways, K % 16 = 8 and a single 8-deep step, the side job's 8-column minimum
#   (2125, 96, 128):  NTW 4 / NTW 3
#   (2085, 200, 72):  NTW 3 / two groups NTW 4, K % 16 = 8
#   (2088, 16, 64):   NTW 2 / NTW 1; the side job's regimes below
# The loader waves' side job (da, in the dq launch: csrc/bx3_waits.h) per shape, as (ksteps = ceil(K2 / 16), cnt = ceil(rows *
# nc / 256) per loader lane, column groups of the dq launch: nc = K2 / 4 float4 columns, or its halves with two groups);
# "full" = the 128-row panels, "last" = the ragged last panel:
#   (2049, 300, 300): (19, 19, 2) full: cnt == ksteps, every store but the last three inside the loop, steady-state waits;
#                     (19, 1, 2) last: one request, its store at barrier 3, then side steps that issue nothing
#   (2125, 52, 304):  (19, 38, 1) full, (19, 23, 1) last: cnt > ksteps + 1, finish requests and stores one index at a time
#   (2049, 64, 160):  (10, 20, 1) full: the same with a short steady state; (10, 1, 1) last
#   (2048, 24, 8):    (1, 1, 1): one k-step, nothing but tail waits, the only store is finish's
#   (2125, 96, 128):  (8, 16, 1) full, (8, 10, 1) last: steady state for barriers 0 .. 3 only
#   (2085, 200, 72):  (5, 5, 2) full: ksteps == NS - 1, one barrier that leaves three steps in flight; (5, 2, 2) last
#   (2088, 16, 64):   (4, 8, 1) full: ksteps == NS - 2, every wait a tail wait (side operations not counted) with stores
#                     and requests in each side step, then finish's one-at-a-time part; (4, 3, 1) last: cnt == 3, the
#                     last request in side step 2, the first store in side step 3, the rest in finish
# The forward has no side job (cnt == 0) at ksteps = ceil(K1 / 16) = 19, 4, 4, 2, 6, 13, 1.
SHAPES = [(2049, 300, 300), (2125, 52, 304), (2049, 64, 160), (2048, 24, 8), (2125, 96, 128), (2085, 200, 72), (2088, 16, 64)]
# the fp16-storage family needs K1 % 8 == 0 and K2 % 8 == 0: bx3_kernel<NTW, true> 5 (two groups), 5 / 2, 1, 4 / 3, 3 / 4,
# 2 / 1; side job (19, 19, 2) + (19, 1, 2), (10, 20, 1) + (10, 13, 1), (1, 1, 1), (8, 16, 1) + (8, 10, 1), (5, 5, 2) + (5, 2, 2),
# (4, 8, 1) + (4, 3, 1)
HALF_SHAPES = [(2049, 304, 304), (2125, 64, 160), (2048, 24, 8), (2125, 96, 128), (2085, 200, 72), (2088, 16, 64)]

def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.fixture(params=["bf16x3", "fp32"])
def matrix_mode(request, hiplib):
    from mms_answer_selection_amd import capi
    capi.set_matrix_mode(request.param)
    yield request.param
    capi.set_matrix_mode("bf16x3")


# ----------------------------------------------------------------------------------------------------------------------
# plane probes: SimMatrix forward and backward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_probe_simmatrix_forward(shape, matrix_mode, hiplib):
    """Q.W and the scores.  q and a hold one nonzero per row (k = i % K1, j = (i + 3) % K2), rows scaled by 2^-8 .. 2^8;
    W is dense.  The score is then a single triple product: one more fp32 multiply, inside the bar's budget."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(N + 3 * K1 + 7 * K2)
    q = mp.one_per_row(mp.probe_values(r, (N,))[0] * mp.pow2(r, (N,), -8, 8, signed=False), K1)
    a = mp.one_per_row(mp.probe_values(r, (N,))[0] * mp.pow2(r, (N,), -8, 8, signed=False), K2, offset=3)
    W = mp.probe_values(r, (K1, K2))[0]
    top, qw = nan_like((N, 1)), nan_like((N, K2))
    capi.simmatrix_forward(dev(q), dev(a), dev(W), top, qw)
    i = np.arange(N)
    check_probe("Q.W %s %s" % (shape, matrix_mode), host(qw), q, W, single=(diag_of(q, K1)[:, None], W[i % K1, :]))
    av = diag_of(a, K2, 3)
    wv = W[i % K1, (i + 3) % K2]
    # top_i = a_i . (q_i W): as a (N, 1) product of the row vector q_i W (fp64) with a_i
    qw64, D = mp.reference(q, W)
    t64 = np.sum(qw64 * a.astype(np.float64), axis=1, keepdims=True)
    tD = np.sum(D * np.abs(a.astype(np.float64)), axis=1, keepdims=True)
    e, idx = mp.componentwise_error(host(top), t64, tD, "scores")
    print("scores %s %s: e = %.3g" % (shape, matrix_mode, e))
    assert e <= mp.BAR, "scores %s: componentwise error %.3g > %.3g at row %d; %s" % (
        shape, e, mp.BAR, idx[0], mp.name_lost_term(diag_of(q, K1), wv, host(top)[:, 0].astype(np.float64) / av))


@pytest.mark.parametrize("cached", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_probe_simmatrix_backward(shape, cached, matrix_mode, hiplib):
    """dq = diag(dT) A W^T (a: one nonzero per row), da = dT_i * (Q.W)_i bit for bit from the kernel's own Q.W, and -- in a
    second call whose q holds one nonzero per COLUMN, spread over every split-K chunk -- dW accumulated onto a nonzero dW."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(2 * N + 3 * K1 + 7 * K2 + int(cached))
    W = mp.probe_values(r, (K1, K2))[0]
    dT = mp.pow2(r, (N, 1), -4, 4)
    # call 1: dq and da
    q = mp.probe_values(r, (N, K1))[0]
    a = mp.one_per_row(mp.probe_values(r, (N,))[0], K2)
    qd, ad, Wd, dTd = dev(q), dev(a), dev(W), dev(dT)
    top, qw = nan_like((N, 1)), nan_like((N, K2))
    capi.simmatrix_forward(qd, ad, Wd, top, qw)
    gq, ga, gW = nan_like((N, K1)), nan_like((N, K2)), dev(np.zeros((K1, K2), np.float32))
    capi.simmatrix_backward(qd, ad, Wd, dTd, gq, ga, gW, qw=qw if cached else None)
    i = np.arange(N)
    check_probe("dq %s %s" % (shape, matrix_mode), host(gq), a, W.T, rowscale=dT,
                single=(diag_of(a, K2)[:, None], W[:, i % K2].T))
    assert_bitexact(host(ga), dT * host(qw), "da = dT * (the kernel's own Q.W), one fp32 multiply")
    assert np.isfinite(host(gW)).all()
    # call 2: dW
    rows = mp.tn_rows(N, K1)
    qc = mp.one_per_column(mp.probe_values(r, (K1,))[0], N)
    a2 = mp.probe_values(r, (N, K2))[0]
    # a nonzero dW to accumulate onto: 1/8 of the product's magnitude, few bits (the sum's one rounding is in the budget)
    dW0 = (0.125 * np.abs(dT[rows]) * r.integers(-4, 5, (K1, K2)) / 4.0).astype(np.float32)
    gq, ga, gW = nan_like((N, K1)), nan_like((N, K2)), dev(dW0)
    capi.simmatrix_forward(dev(qc), dev(a2), Wd, top, qw)
    capi.simmatrix_backward(dev(qc), dev(a2), Wd, dTd, gq, ga, gW, qw=qw if cached else None)
    U = dT.astype(np.float64) * a2.astype(np.float64)          # exact: dT is a power of two
    check_probe("dW %s %s" % (shape, matrix_mode), host(gW), qc.T, U, extra=dW0,
                single=(qc[rows, np.arange(K1)][:, None], U[rows, :].astype(np.float32)))
    assert_bitexact(host(ga), dT * host(qw), "da (second call)")


# ----------------------------------------------------------------------------------------------------------------------
# plane probes: the triplet step at shapes its fused route refuses -- the layers one by one, inside the call
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2125, 300, 300), (2049, 64, 160)])
def test_probe_triplet_simmatrix_step(shape, matrix_mode, oracle, hiplib):
    """Both shapes have fewer than 6081 triplets (and odd N): tripsim_fused refuses them and mms_triplet_simmatrix_step_f32 runs
    SimMatrix x 2 -> PairRankLoss -> SimMatrix backward x 2 -> Split sum (profiles/learned_metric_routes.txt).  This holds THAT
    route's backward to the bar; the fused route has its own module, tests/test_gpu_triplet_simmatrix_fused.py.
    dq = dq+ + dq- and dW += both branches' terms.  a- = 0, loss_weight = N and a margin no score reaches make them g+ a+ W^T
    and Q^T (g+ a+) with g+ = +-1 (asserted from PairRankLoss evaluated at the GPU's own scores), so the probes apply as they
    are."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(5 * N + K1 + K2)
    W = mp.probe_values(r, (K1, K2))[0]
    y = np.ones((N, 1), np.float32)
    an = np.zeros((N, K2), np.float32)
    margin, lw = 1.0e6, float(N)
    rows = mp.tn_rows(N, K1)

    def step(q, ap, dW0):
        out = dict(s_pos=nan_like((N, 1)), s_neg=nan_like((N, 1)), loss=nan_like((1,)), dq=nan_like((N, K1)),
                   da_pos=nan_like((N, K2)), da_neg=nan_like((N, K2)), dW=dev(dW0))
        capi.triplet_simmatrix_step(dev(q), dev(ap), dev(an), dev(y), dev(W), margin=margin, loss_weight=lw, **out)
        g = {k: host(v) for k, v in out.items()}
        _, o, s = oracle.pairrank_forward(g["s_pos"], g["s_neg"], y, margin)
        gp, _ = oracle.pairrank_backward(y, o, s, top_diff=lw)
        assert (np.abs(gp) == 1.0).all(), "the probe needs g+ = +-1 on every row"
        return g, gp

    ap = mp.one_per_row(mp.probe_values(r, (N,))[0], K2)
    g, gp = step(mp.probe_values(r, (N, K1))[0], ap, np.zeros((K1, K2), np.float32))
    i = np.arange(N)
    check_probe("triplet dq %s %s" % (shape, matrix_mode), g["dq"], ap, W.T, rowscale=gp,
                single=(diag_of(ap, K2)[:, None], W[:, i % K2].T))
    qc = mp.one_per_column(mp.probe_values(r, (K1,))[0], N)
    ap2 = mp.probe_values(r, (N, K2))[0]
    dW0 = (0.125 * r.integers(-4, 5, (K1, K2)) / 4.0).astype(np.float32)
    g, gp = step(qc, ap2, dW0)
    U = gp.astype(np.float64) * ap2.astype(np.float64)
    check_probe("triplet dW %s %s" % (shape, matrix_mode), g["dW"], qc.T, U, extra=dW0,
                single=(qc[rows, np.arange(K1)][:, None], U[rows, :].astype(np.float32)))


# ----------------------------------------------------------------------------------------------------------------------
# plane probes: a one-word bilinear SimCross layer, routed to the same launches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias_term", [False, True])
@pytest.mark.parametrize("D", [300, 64])
def test_probe_simcross_bilinear(D, bias_term, matrix_mode, hiplib):
    from mms_answer_selection_amd import capi
    N = 2304
    r = rng(N + D + int(bias_term))
    W = mp.probe_values(r, (D, D))[0]
    dT = mp.pow2(r, (N, 1), -4, 4)
    bias = np.full((1, 1, 1), 0.125, np.float32) if bias_term else None     # 1/8 of a product: one rounding, in the budget
    q = mp.one_per_row(mp.probe_values(r, (N,))[0], D)
    a = mp.one_per_row(mp.probe_values(r, (N,))[0], D, offset=5)
    i = np.arange(N)

    def run(q, a):
        qd, ad, Wd = dev(q.reshape(N, 1, D)), dev(a.reshape(N, 1, D)), dev(W.reshape(1, D, D))
        top = nan_like((N, 1, 1, 1))
        capi.simcross_forward(2, qd, ad, top, W=Wd, bias=dev(bias))
        gq, ga, gW = nan_like((N, 1, D)), nan_like((N, 1, D)), nan_like((1, D, D))
        gb = dev(np.zeros((1, 1, 1), np.float32)) if bias_term else None
        capi.simcross_backward(2, qd, ad, top, dev(dT.reshape(N, 1, 1, 1)), gq, ga, W=Wd, bias_term=bias_term, dW=gW, dbias=gb)
        return host(top).reshape(N, 1), host(gq).reshape(N, D), host(ga).reshape(N, D), host(gW).reshape(D, D)

    top, gq, ga, _ = run(q, a)
    what = "simcross D=%d bias=%s %s: " % (D, bias_term, matrix_mode)
    qw64, Dm = mp.reference(q, W)
    t64 = np.sum(qw64 * a.astype(np.float64), axis=1, keepdims=True) + (0.125 if bias_term else 0.0)
    tD = np.sum(Dm * np.abs(a.astype(np.float64)), axis=1, keepdims=True)
    e, idx = mp.componentwise_error(top, t64, tD, what + "top")
    print(what + "top e = %.3g" % e)
    assert e <= mp.BAR, what + "top: componentwise error %.3g > %.3g at row %d; %s" % (
        e, mp.BAR, idx[0], mp.name_lost_term(diag_of(q, D), W[i % D, (i + 5) % D],
                                             (top[:, 0].astype(np.float64) - (0.125 if bias_term else 0.0)) / diag_of(a, D, 5)))
    check_probe(what + "dq", gq, a, W.T, rowscale=dT, single=(diag_of(a, D, 5)[:, None], W[:, (i + 5) % D].T))
    check_probe(what + "da", ga, q, W, rowscale=dT, single=(diag_of(q, D)[:, None], W[i % D, :]))
    rows = mp.tn_rows(N, D)
    qc = mp.one_per_column(mp.probe_values(r, (D,))[0], N)
    a2 = mp.probe_values(r, (N, D))[0]
    _, _, _, gW = run(qc, a2)
    U = dT.astype(np.float64) * a2.astype(np.float64)
    check_probe(what + "dW", gW, qc.T, U, single=(qc[rows, np.arange(D)][:, None], U[rows, :].astype(np.float32)))


# ----------------------------------------------------------------------------------------------------------------------
# plane probes: the fp16-storage family (bf16 pipe whatever the matrix mode; five plane products)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HALF_SHAPES)
def test_probe_simmatrix_fp16_storage(shape, hiplib):
    """q, a (and dq, da) are halves: h + m exactly, with both planes populated.  dq and da are rounded to half at the store:
    dq gets the store's half-ulp on top of the bar, da is the RNE half of one fp32 multiply, bit for bit.  dW runs twice: with
    half probe values in a (B side = two planes) and with a = +-2^e and dT a three-plane probe value (B side = dT * a, all
    five products populated)."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(4 * N + K1 + 9 * K2)
    h16 = torch.float16
    W = mp.probe_values(r, (K1, K2))[0]
    dT = mp.pow2(r, (N, 1), -3, 3)
    q = mp.one_per_row(mp.probe_values(r, (N,), half=True)[0] * mp.pow2(r, (N,), -3, 3, signed=False), K1)
    a = mp.one_per_row(mp.probe_values(r, (N,), half=True)[0] * mp.pow2(r, (N,), -3, 3, signed=False), K2, offset=3)
    qh, ah = q.astype(np.float16), a.astype(np.float16)
    assert (qh.astype(np.float32) == q).all() and (ah.astype(np.float32) == a).all()
    qd, ad, Wd, dTd = dev(qh), dev(ah), dev(W), dev(dT)
    top0, top, qw = nan_like((N, 1)), nan_like((N, 1)), nan_like((N, K2))
    capi.simmatrix_forward_f16(qd, ad, Wd, top0)
    capi.simmatrix_forward_train_f16(qd, ad, Wd, top, qw)
    i = np.arange(N)
    what = "fp16-storage %s: " % (shape,)
    check_probe(what + "Q.W", host(qw), q, W, single=(diag_of(q, K1)[:, None], W[i % K1, :]), a_half=True)
    qw64, Dm = mp.reference(q, W)
    t64 = np.sum(qw64 * a.astype(np.float64), axis=1, keepdims=True)
    tD = np.sum(Dm * np.abs(a.astype(np.float64)), axis=1, keepdims=True)
    for name, t in (("scores (scoring entry point)", host(top0)), ("scores (training forward)", host(top))):
        e, idx = mp.componentwise_error(t, t64, tD, what + name)
        print(what + name + " e = %.3g" % e)
        assert e <= mp.BAR, what + name + ": componentwise error %.3g > %.3g at row %d; %s" % (
            e, mp.BAR, idx[0], mp.name_lost_term(diag_of(q, K1), W[i % K1, (i + 3) % K2],
                                                 t[:, 0].astype(np.float64) / diag_of(a, K2, 3), a_half=True))
    gq, ga, gW = nan_like((N, K1), h16), nan_like((N, K2), h16), dev(np.zeros((K1, K2), np.float32))
    capi.simmatrix_backward_f16(qd, ad, Wd, qw, dTd, gq, ga, gW)
    check_probe(what + "dq", host(gq).astype(np.float32), a, W.T, rowscale=dT, a_half=True, half_out=True)
    want = (dT * host(qw)).astype(np.float16)
    assert (host(ga).view(np.uint16) == want.view(np.uint16)).all(), what + "da = half(dT * the kernel's own Q.W)"
    # dW
    rows = mp.tn_rows(N, K1)
    qc = mp.one_per_column(mp.probe_values(r, (K1,), half=True)[0], N)
    for variant in ("half x half", "half x (probe dT * 2^e)"):
        if variant == "half x half":
            a2, dT2 = mp.probe_values(r, (N, K2), half=True)[0], dT
        else:
            a2, dT2 = mp.pow2(r, (N, K2), -2, 2), mp.probe_values(r, (N, 1))[0]
        U = dT2.astype(np.float64) * a2.astype(np.float64)            # exact in fp32 either way
        assert (U.astype(np.float32).astype(np.float64) == U).all()
        dW0 = (0.125 * r.integers(-4, 5, (K1, K2)) / 4.0).astype(np.float32)
        gW = dev(dW0)
        capi.simmatrix_backward_f16(dev(qc.astype(np.float16)), dev(a2.astype(np.float16)), Wd, None, dev(dT2), None, None, gW)
        check_probe(what + "dW, " + variant, host(gW), qc.T, U, extra=dW0,
                    single=(qc[rows, np.arange(K1)][:, None], U[rows, :].astype(np.float32)), a_half=True)


# ----------------------------------------------------------------------------------------------------------------------
# dense data: scale invariance, parity with the reference's own rounding
# ----------------------------------------------------------------------------------------------------------------------
DENSE = [(2125, 300, 300), (4096, 64, 160), (2049, 52, 304)]


def run_simmatrix(capi, q, a, W, dT, dW0):
    N, K1 = q.shape
    K2 = a.shape[1]
    qd, ad, Wd, dTd = dev(q), dev(a), dev(W), dev(dT)
    top, qw = nan_like((N, 1)), nan_like((N, K2))
    capi.simmatrix_forward(qd, ad, Wd, top, qw)
    gq, ga, gW = nan_like((N, K1)), nan_like((N, K2)), dev(dW0)
    capi.simmatrix_backward(qd, ad, Wd, dTd, gq, ga, gW, qw=qw)
    return dict(top=host(top), qw=host(qw), dq=host(gq), da=host(ga), dW=host(gW))


def ldexp32(x, e):
    return np.ldexp(x, e.astype(np.int32)).astype(np.float32)


@pytest.mark.parametrize("shape", DENSE)
def test_dense_power_of_two_scaling_changes_no_bit(shape, matrix_mode, hiplib):
    """q -> 2^(r_i + s_k) q, W -> 2^(-s_k + c_j) W, a -> 2^(-r_i - c_j) a, dW0 -> 2^(s_k - c_j) dW0, exponents from +-30:
    Q.W, dq, da and dW come out as the unscaled results times the corresponding power of two and the scores unchanged, bit
    for bit -- small-magnitude rows and columns get the same arithmetic as large ones."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(N + K1 + K2 + 11)
    q, a, W, dT = mp.dense_inputs(r, N, K1, K2)
    dW0 = r.standard_normal((K1, K2)).astype(np.float32)
    ri, sk, cj = r.integers(-30, 31, (N, 1)), r.integers(-30, 31, K1), r.integers(-30, 31, K2)
    qs, Ws = ldexp32(q, ri + sk[None, :]), ldexp32(W, -sk[:, None] + cj[None, :])
    as_, dW0s = ldexp32(a, -ri - cj[None, :]), ldexp32(dW0, sk[:, None] - cj[None, :])
    for x in (qs, Ws, as_, (dT * as_).astype(np.float32), dW0s):
        assert mp.all_planes_normal(x), "the scaled inputs keep every plane a normal number"
    base = run_simmatrix(capi, q, a, W, dT, dW0)
    da_host = dT * base["qw"]
    assert_bitexact(base["da"], da_host, "da = dT * (the kernel's own Q.W), dense data")
    got = run_simmatrix(capi, qs, as_, Ws, dT, dW0s)
    assert_bitexact(got["qw"], ldexp32(base["qw"], ri + cj[None, :]), "Q.W under scaling")
    assert_bitexact(got["top"], base["top"], "scores under scaling")
    assert_bitexact(got["dq"], ldexp32(base["dq"], -ri - sk[None, :]), "dq under scaling")
    assert_bitexact(got["da"], ldexp32(base["da"], ri + cj[None, :]), "da under scaling")
    assert_bitexact(got["dW"], ldexp32(base["dW"], sk[:, None] - cj[None, :]), "dW under scaling")


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("shape", DENSE)
def test_dense_error_within_twice_the_references(shape, positive, oracle, hiplib):
    """e(bf16 pipe) <= 2 * max(e(CPU oracle's sgemm), e(fp32-MFMA pipe)) + 2^-24 per output, on the suite's dense data and on
    an all-positive variant (no cancellation: errors add up).  The measured values are recorded in DESIGN.md (Numerics)."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = shape
    r = rng(N + K1 + K2 + 13 + int(positive))
    q, a, W, dT = mp.dense_inputs(r, N, K1, K2, positive)
    zero = np.zeros((K1, K2), np.float32)
    out = {}
    try:
        for mode in ("bf16x3", "fp32"):
            capi.set_matrix_mode(mode)
            out[mode] = run_simmatrix(capi, q, a, W, dT, zero)
    finally:
        capi.set_matrix_mode("bf16x3")
    top_ref, qw_ref = oracle.simmatrix_forward(q, a, W)
    dq_ref, _, dW_ref = oracle.simmatrix_backward(q, a, W, dT, dW_in=zero)
    out["oracle"] = dict(top=top_ref, qw=qw_ref, dq=dq_ref, dW=dW_ref)
    q64, a64, W64, dT64 = (x.astype(np.float64) for x in (q, a, W, dT))
    qw64, qwD = mp.reference(q, W)
    refs = {
        "qw": (qw64, qwD),
        "top": (np.sum(qw64 * a64, axis=1, keepdims=True), np.sum(qwD * np.abs(a64), axis=1, keepdims=True)),
        "dq": tuple(x * s for x, s in zip(mp.reference(a, W.T), (dT64, np.abs(dT64)))),
        "dW": mp.reference(q.T, dT64 * a64),
    }
    fails = []
    for name, (C64, Dm) in refs.items():
        e = {who: mp.componentwise_error(out[who][name], C64, Dm, name)[0] for who in ("bf16x3", "fp32", "oracle")}
        msg = "%s %s%s: e(bf16 pipe) = %.3g, e(fp32 pipe) = %.3g, e(oracle sgemm) = %.3g" % (
            name, shape, " positive" if positive else "", e["bf16x3"], e["fp32"], e["oracle"])
        print(msg)
        if not e["bf16x3"] <= 2.0 * max(e["oracle"], e["fp32"]) + 2.0 ** -24:
            fails.append(msg)
    assert not fails, "; ".join(fails)


# ----------------------------------------------------------------------------------------------------------------------
# the magnitude edges of the split (include/mms.h, beside mms_simmatrix_forward_ws_f32)
# ----------------------------------------------------------------------------------------------------------------------
def test_magnitude_edges_of_the_split(hiplib):
    """include/mms.h: "the three planes hold an operand exactly while its last mantissa bit is at least 2^-133, bf16's smallest
    subnormal, i.e. for magnitudes from 2^-110 up; a smaller element enters the product rounded to a multiple of 2^-133
    (nothing is flushed to zero: absolute error <= 2^-134 per element, relative 2^-24 at 2^-110 growing to 2^-8 at 2^-126);
    a magnitude of 2^128 - 2^119 (3.3962e38) or more rounds the first plane to infinity and, like an infinity, makes its
    row NaN."  Measured on an MI355X: e = 1.5e-7 down to 2^-110, 9.7e-7 at 2^-114, 5.4e-5 at 2^-120, 3.6e-3 at 2^-126."""
    from mms_answer_selection_amd import capi
    N, K1, K2 = 2048, 64, 64
    r = rng(4242)
    vals = mp.probe_values(r, (N,))[0]
    exps = np.array([100, 105, 110, 111, 114, 120, 124, 126])[np.arange(N) % 8]
    q = mp.one_per_row(np.ldexp(vals, -exps.astype(np.int32)).astype(np.float32), K1)
    W = mp.probe_values(r, (K1, K2))[0]
    a = np.zeros((N, K2), np.float32)
    top, qw = nan_like((N, 1)), nan_like((N, K2))
    capi.simmatrix_forward(dev(q), dev(a), dev(W), top, qw)
    got = host(qw).astype(np.float64)
    C64, D = mp.reference(q, W)
    err = np.abs(got - C64)
    assert (got != 0).all(), "nothing is flushed to zero"
    big = exps <= 110
    assert (err[big] <= mp.BAR * D[big]).all(), "from 2^-110 up the stated accuracy holds"
    i = np.arange(N)
    absW = np.abs(W[i % K1, :].astype(np.float64))
    assert (err <= 2.0 ** -134 * absW + mp.BAR * D).all(), "below: the element rounded to a multiple of 2^-133"
    # the upper edge: the largest fp32 number whose first plane stays finite, and the next one up
    below, at = np.uint32(0x7F7F7FFF).view(np.float32), np.uint32(0x7F7F8000).view(np.float32)
    qb = mp.one_per_row(vals, K1)
    qb[5, 5], qb[9, 9] = below, -at
    Ws = (W * np.float32(2.0 ** -10)).astype(np.float32)
    capi.simmatrix_forward(dev(qb), dev(a), dev(Ws), top, qw)
    g = host(qw)
    assert np.isnan(g[9]).all(), "2^128 - 2^119: NaN for its row"
    keep = np.delete(np.arange(N), 9)
    C64, D = mp.reference(qb[keep], Ws)
    e, idx = mp.componentwise_error(g[keep], C64, D, "just below the edge")
    assert e <= mp.BAR, (e, idx)
