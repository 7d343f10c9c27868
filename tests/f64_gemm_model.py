"""Routes, inputs, references and error bars for the fp64 matrix-pipe products of csrc/f64_paths.hip: the ten products that
gemm64_kernel (`tiled`) and gemm64_tallk_kernel (`tallk`) serve for mms_simcross_*_f64 (dist_mode 2) and mms_simmatrix_*_f64.

Route table (routes()).  run_g64 (f64_paths.hip:390-415) takes ONE decision per product, on the whole problem:
    tallk  iff  nseg * L >= 1024  and  ceil(N / 64) * ceil(M / 64) * nb0 * nb1 <= 64
and then slices the outer batch nb0 (gridDim.z = nb * nb1 <= 65535) and the rows (gridDim.y <= 65535); slices() restates the
slicing.  Each launcher's G64 (struct at :177-186) is restated product by product, with the lines it comes from:
    bilinear   QW  (bil_qw, :491-499)      M = W1, N = D,  L = D,  batches (N, M)      A row-major, B row-major
               top (:525-532)              M = W1, N = W2, L = D,  batches (N, M)      B = A_n^T (column-major unless D = 1), bias
               t1  (:558-565)              M = D,  N = W2, L = W1, batches (N, M)      A = Q_n^T (column-major unless D = 1)
               dW  (:566-572)              M = D,  N = D,  L = W2, nseg = N, batch (M)
               t2  (:573-580)              M = D,  N = W2, L = D,  batches (N, M)      B = A_n^T
               dq  (:581-586)              M = W1, N = D,  L = W2, nseg = M, batch (N) B = t2^T (column-major unless W2 = 1)
               da  (:588-593)              M = W2, N = D,  L = W1, nseg = M, batch (N) A = dT^T (column-major unless W2 = 1)
    SimMatrix  fwd (:602)                  M = N,  N = K2, L = K1
               dW  (:611-615)              M = K1, N = K2, L = N                       A = Q^T (column-major unless K1 = 1), kscale, beta
               dq  (:616-620)              M = N,  N = K1, L = K2                      B = W^T (column-major unless K2 = 1), rowscale
               da  (:621-625)              M = N,  N = K2, L = K1                      rowscale
a_kfast / b_nfast are the staging maps of gemm64_kernel (:199); tallk loads through the strides directly (:336-339).  The tile
flags are M, N multiples of 64 and L of 16 on `tiled` (:195, :208), M, N multiples of 32 and nseg * L of 256 on `tallk` (:313,
:325: sixteen waves x four k-steps x four k); `straddle` is a 4-wide MFMA k-step of tallk that crosses a segment boundary
(nseg > 1 and L % 4 != 0, :329-331).

Exact probes.  Every entry of q, a, W, bias, dT and the incoming dW / dbias is an integer with 0 < |x| <= 512; every fifth row
of q and every seventh of a hold a single nonzero, at a moving column (cosine_model.exact_rows).  Every partial sum of every
product chain, in ANY order, is then an integer below 2^53 (bilinear_bound / simmatrix_bound give the bound per shape), so a
correct kernel returns the int64 reference (bilinear_ref / simmatrix_ref: the formulas of sim_cross_layer.cpp mode 2 and
sim_matrix_layer.cpp in numpy int64) bit for bit.  Outputs reach 2^30 and far more with odd low bits: an fp32 accumulator or
operand cannot pass.

Dense bar (derived, not measured).  Inputs are standard_normal rounded to 20 fractional bits, so the same formulas in Python
integers (object arrays, `unit` = 2^20) are exact.  Per element |got - exact| <= gamma_n S, gamma_n = n u / (1 - n u),
u = 2^-53, S the same expression with every factor replaced by its absolute value, and n the number of roundings on the path:
    bilinear   top  D + D + 1 (+ 1 with bias)      the chained products: K_first + K_second + 1
               dW   W1 + N W2 + 1                   t1, then the N-segment sum
               dq   D + M W2 + 1                    t2, then the M-segment sum
               da   D + M W1 + 1                    QW, then the M-segment sum
               dbias N + 1                          n-ascending adds onto the incoming value
    SimMatrix  scratch K1;  top K1 + K2 + 1;  dq K2 + 1 (rowscale);  da K1 + 1 (rowscale)
               dW   N + 1 (kscale: dT_i q_ir is rounded as it is staged) + 1 (beta)
A sum of K products in any order has at most K roundings on the path of one term (Higham, Accuracy and Stability, 3.1), so the
bar does not depend on the order a kernel, or the oracle, adds in.

CPU only; tests/test_f64_gemm_model.py checks this module against the CPU oracle, tests/test_gpu_f64_accuracy.py uses it.
"""
import numpy as np

from cosine_model import shape_id, shape_seed  # noqa: F401  (re-exported for the tests)

U53 = 2.0 ** -53
FRAC = 20                                     # fractional bits of the dense inputs
B = 512                                       # largest probe magnitude
GRID_MAX = 65535

# (N, M, W1, W2, D)
BILINEAR = [(1, 2, 3, 5, 1028),               # QW, top (bias) and t2 on tallk
            (1, 2, 1030, 520, 6),             # t1 on tallk with column-major A; da, dq on tallk with segmented K; dW tiled, nseg = 1
            (3, 2, 5, 7, 1028),               # QW tiled while top is tallk (both batch indices)
            (64, 3, 40, 33, 50), (5, 2, 70, 65, 67),
            (2, 3, 1, 1, 1), (7, 1, 1, 1, 20), (4, 2, 17, 1, 3),        # L of 1, 2 and 3
            (2, 2, 516, 515, 5),              # dq, da on tallk: segmented K WITH a batch; L % 4 of 3 (dq) and 0 (da)
            (2, 1, 2, 3, 1024),               # QW, top, t2 on tallk with the pair batch only; whole 32-tiles, K a multiple of 256
            (2, 1, 1024, 3, 1),               # t1 on tallk with D = 1 (A k-fast) and a pair batch; da on tallk with nseg = 1
            (1, 1, 2, 1025, 3),               # dW and dq on tallk with nseg = 1
            (1, 1024, 2, 1, 2)]               # 1024 measures: dq (B n-fast), da (A k-fast) on tallk with L = 1 and 2 per segment
# (N, K1, K2)
SIMMATRIX = [(70, 1030, 1100),                # forward, dq, da on tallk with rowscale; dW tiled with kscale + beta
             (1023, 8, 8), (1024, 8, 8),      # K threshold on dW
             (4096, 64, 1024), (4097, 64, 1024),   # tiles64 of 64 and 65 on dq
             (37, 24, 19), (3000, 130, 70), (1, 1, 1), (65, 17, 63),
             (1030, 1, 3)]                    # dW on tallk with K1 = 1 (A k-fast)
# the batch and row limits of one launch
BILINEAR_LARGE = [(21846, 3, 1, 1, 4), (13107, 5, 2, 1, 3)]
SIMMATRIX_LARGE = [(64 * 65535 + 65, 2, 2)]
# dense data: both kernels and every epilogue, small enough for exact integer arithmetic
BILINEAR_DENSE = [(6, 3, 5, 4, 12), (2, 2, 70, 65, 9), (1, 1, 2, 3, 1030), (2, 2, 1030, 9, 3), (2, 2, 3, 520, 3), (40, 2, 3, 30, 5)]
SIMMATRIX_DENSE = [(37, 24, 19), (70, 20, 9), (3, 1030, 5), (3, 5, 1030), (1030, 3, 5)]


def gamma(n):
    return n * U53 / (1.0 - n * U53)


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------------
# route table
# ----------------------------------------------------------------------------------------------------------------------
def _route(product, M, N, L, sam, sak, sbk, sbn, nseg=1, nb0=1, nb1=1, kscale=False, rowscale=False, bias=False, beta=False):
    tiles64 = cdiv(N, 64) * cdiv(M, 64) * nb0 * nb1
    tallk = nseg * L >= 1024 and tiles64 <= 64
    tile = 32 if tallk else 64
    return dict(product=product, kernel="tallk" if tallk else "tiled", M=M, N=N, L=L, nseg=nseg, n_b0=nb0, n_b1=nb1,
                a_kfast=sak == 1, b_nfast=sbn == 1 or sbk != 1, seg=nseg > 1, nb0=nb0 > 1, nb1=nb1 > 1,
                kscale=kscale, rowscale=rowscale, bias=bias, beta=beta,
                m_full=M % tile == 0, n_full=N % tile == 0, k_full=(nseg * L) % 256 == 0 if tallk else L % 16 == 0,
                straddle=tallk and nseg > 1 and L % 4 != 0, launches=len(slices(M, nb0, nb1, tile)))


def slices(M, nb0, nb1, tile):
    """run_g64's launches: [(first b0, number of b0, first row, rows)], every one with gridDim.y, gridDim.z <= 65535."""
    max_b0 = 1 if nb1 > GRID_MAX else GRID_MAX // nb1
    max_rows = GRID_MAX * tile
    return [(b, min(nb0 - b, max_b0), r, min(M - r, max_rows)) for b in range(0, nb0, max_b0) for r in range(0, M, max_rows)]


def routes(call, shape, bias=False):
    """The products of one ABI call, in launch order: call in simcross_forward / simcross_backward (shape (N, M, W1, W2, D),
    dist_mode 2) / simmatrix_forward / simmatrix_backward (shape (N, K1, K2))."""
    if call.startswith("simcross"):
        N, M, W1, W2, D = shape
        qw = _route("bil_QW", W1, D, D, D, 1, D, 1, nb0=N, nb1=M)
        if call == "simcross_forward":
            return [qw, _route("bil_top", W1, W2, D, D, 1, 1, D, nb0=N, nb1=M, bias=bias)]
        assert call == "simcross_backward"
        return [_route("bil_t1", D, W2, W1, 1, D, W2, 1, nb0=N, nb1=M),
                _route("bil_dW", D, D, W2, W2, 1, D, 1, nseg=N, nb0=M),
                _route("bil_t2", D, W2, D, D, 1, 1, D, nb0=N, nb1=M),
                _route("bil_dq", W1, D, W2, W2, 1, 1, W2, nseg=M, nb0=N),
                qw,
                _route("bil_da", W2, D, W1, 1, W2, D, 1, nseg=M, nb0=N)]
    N, K1, K2 = shape
    if call == "simmatrix_forward":
        return [_route("sm_fwd", N, K2, K1, K1, 1, K2, 1)]
    assert call == "simmatrix_backward"
    return [_route("sm_dW", K1, K2, N, 1, K1, K2, 1, kscale=True, beta=True),
            _route("sm_dq", N, K1, K2, K2, 1, 1, K2, rowscale=True),
            _route("sm_da", N, K2, K1, K1, 1, K2, 1, rowscale=True)]


def all_routes():
    """Every product instance of the probe lists (bilinear with and without bias)."""
    out = []
    for s in BILINEAR:
        for bias in (False, True):
            out += routes("simcross_forward", s, bias)
        out += routes("simcross_backward", s)
    for s in SIMMATRIX:
        out += routes("simmatrix_forward", s) + routes("simmatrix_backward", s)
    return out


_BOTH = (True, False)
# What a launcher can produce on each kernel: {product: {kernel: {feature: values}}}.  tallk needs nseg L >= 1024 and at most 64
# 64-tiles over all batches, which is what rules a value out:
#   bil_top / bil_t2 on tallk have L = D >= 1024, so B = A_n^T is never n-fast there; sm_dq likewise (K2 >= 1024);
#   a_kfast and b_nfast of the other products are fixed by their launcher.
REQUIRED = {
    "bil_QW": {"tiled": dict(nb0=_BOTH, nb1=_BOTH), "tallk": dict(nb0=_BOTH, nb1=_BOTH)},
    "bil_top": {"tiled": dict(nb0=_BOTH, nb1=_BOTH, bias=_BOTH, b_nfast=_BOTH),
                "tallk": dict(nb0=_BOTH, nb1=_BOTH, bias=_BOTH, b_nfast=(False,))},
    "bil_t1": {"tiled": dict(nb0=_BOTH, nb1=_BOTH, a_kfast=_BOTH), "tallk": dict(nb0=_BOTH, nb1=_BOTH, a_kfast=_BOTH)},
    "bil_dW": {"tiled": dict(seg=_BOTH, nb0=_BOTH), "tallk": dict(seg=_BOTH, nb0=_BOTH)},
    "bil_t2": {"tiled": dict(nb0=_BOTH, nb1=_BOTH, b_nfast=_BOTH), "tallk": dict(nb0=_BOTH, nb1=_BOTH, b_nfast=(False,))},
    "bil_dq": {"tiled": dict(seg=_BOTH, nb0=_BOTH, b_nfast=_BOTH), "tallk": dict(seg=_BOTH, nb0=_BOTH, b_nfast=_BOTH, straddle=_BOTH)},
    "bil_da": {"tiled": dict(seg=_BOTH, nb0=_BOTH, a_kfast=_BOTH), "tallk": dict(seg=_BOTH, nb0=_BOTH, a_kfast=_BOTH, straddle=_BOTH)},
    "sm_fwd": {"tiled": dict(), "tallk": dict()},
    "sm_dW": {"tiled": dict(a_kfast=_BOTH, kscale=(True,), beta=(True,)), "tallk": dict(a_kfast=_BOTH, kscale=(True,), beta=(True,))},
    "sm_dq": {"tiled": dict(b_nfast=_BOTH, rowscale=(True,)), "tallk": dict(b_nfast=(False,), rowscale=(True,))},
    "sm_da": {"tiled": dict(rowscale=(True,)), "tallk": dict(rowscale=(True,))},
}
# per kernel, over all products: ragged and whole tiles in every dimension
REQUIRED_TILES = {"tiled": dict(m_full=_BOTH, n_full=_BOTH, k_full=_BOTH), "tallk": dict(m_full=_BOTH, n_full=_BOTH, k_full=_BOTH)}


# ----------------------------------------------------------------------------------------------------------------------
# exact probes
# ----------------------------------------------------------------------------------------------------------------------
def probe_ints(r, shape):
    """int64, 0 < |x| <= 512, odd and even alike."""
    return r.integers(1, B + 1, shape) * np.where(r.integers(0, 2, shape) == 0, -1, 1)


def probe_rows(r, rows, D, period, phase):
    """(rows, D) of probe_ints; row i with i % period == phase holds one nonzero, at column 3 i % D."""
    k = probe_ints(r, (rows, D))
    i = np.arange(phase, rows, period)
    keep = 3 * i % D
    v = k[i, keep]
    k[i] = 0
    k[i, keep] = v
    return k


def bilinear_probe(shape):
    N, M, W1, W2, D = shape
    r = np.random.default_rng(1701 + shape_seed(shape))
    return dict(q=probe_rows(r, N * W1, D, 5, 2).reshape(N, W1, D), a=probe_rows(r, N * W2, D, 7, 3).reshape(N, W2, D),
                W=probe_ints(r, (M, D, D)), bias=probe_ints(r, (M, W1, W2)), dT=probe_ints(r, (N, M, W1, W2)),
                dbias_in=probe_ints(r, (M, W1, W2)))


def simmatrix_probe(shape):
    N, K1, K2 = shape
    r = np.random.default_rng(1701 + 3 * shape_seed(shape))
    return dict(q=probe_rows(r, N, K1, 5, 2), a=probe_rows(r, N, K2, 7, 3), W=probe_ints(r, (K1, K2)), dT=probe_ints(r, (N, 1)),
                dW_in=probe_ints(r, (K1, K2)))


def _T(x):
    return np.swapaxes(x, -1, -2)


def bilinear_ref(p, bias_term, unit=1):
    """sim_cross_layer.cpp mode 2 on whatever number type p holds (int64: the probes; object: exact dense; float64 of absolute
    values: S).  `unit` is the value 1 in p's fixed-point scale: what is ADDED to a triple product is scaled by unit^2."""
    q, a, W, dT = p["q"], p["a"], p["W"], p["dT"]
    qw = np.matmul(q[:, None], W[None])                                  # (N, M, W1, D)
    top = np.matmul(qw, _T(a)[:, None])                                  # (N, M, W1, W2)
    if bias_term:
        top = top + (p["bias"] * (unit * unit))[None]
    t1 = np.matmul(_T(q)[:, None], dT)                                   # (N, M, D, W2)
    dW = np.matmul(t1, a[:, None]).sum(0)                                # (M, D, D): zeroed first (:256), summed over n
    t2 = np.matmul(W[None], _T(a)[:, None])                              # (N, M, D, W2)
    dq = np.matmul(dT, _T(t2)).sum(1)                                    # (N, W1, D)
    da = np.matmul(_T(dT), qw).sum(1)                                    # (N, W2, D)
    out = dict(top=top, dq=dq, da=da, dW=dW)
    if bias_term:
        out["dbias"] = p["dbias_in"] + dT.sum(0)
    return out


def simmatrix_ref(p, unit=1):
    """sim_matrix_layer.cpp on p's number type: scratch = Q W, top_i = a_i . scratch_i, dW += (diag(dT) Q)^T A,
    dq = diag(dT) A W^T, da = diag(dT) Q W."""
    q, a, W, dT = p["q"], p["a"], p["W"], p["dT"]
    scr = np.matmul(q, W)
    return dict(scratch=scr, top=(a * scr).sum(1, keepdims=True), dW=p["dW_in"] * (unit * unit) + np.matmul(_T(q * dT), a),
                dq=dT * np.matmul(a, _T(W)), da=dT * scr)


def bilinear_bound(shape):
    """No partial sum of any product chain on the probes, in any order, exceeds this (in absolute value)."""
    N, M, W1, W2, D = shape
    return max(B ** 3 * D * D + B, B ** 3 * W1 * N * W2, B ** 3 * D * M * W2, B ** 3 * D * M * W1, B * N + B)


def simmatrix_bound(shape):
    N, K1, K2 = shape
    return max(B ** 3 * K1 * K2, B ** 3 * N + B, B ** 3 * K2, B ** 3 * K1)


def f64(p):
    """The probe (or a reference) as the doubles the kernels are given."""
    return {k: v.astype(np.float64) for k, v in p.items()}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_bits(got, ref, what):
    """got (float64) equals the integer reference bit for bit.  An exact cancellation times a negative dT is -0.0 in double
    and 0 in int64: the sign of a zero is the one thing the integers cannot give, so both sides are passed through x + 0.0."""
    got = np.asarray(got) + 0.0
    want = np.asarray(ref).astype(np.float64).reshape(got.shape) + 0.0
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, first at %s: got %r, exact %r" % (
        what, bad.size, got.size, np.unravel_index(int(bad[0]), got.shape), got.ravel()[bad[0]], want.ravel()[bad[0]])


# ----------------------------------------------------------------------------------------------------------------------
# dense data: exact integer reference and the gamma_n bar
# ----------------------------------------------------------------------------------------------------------------------
def _dense_ints(r, shape):
    return np.rint(np.ldexp(r.standard_normal(shape), FRAC)).astype(np.int64)


def bilinear_dense(shape):
    N, M, W1, W2, D = shape
    r = np.random.default_rng(1701 + 7 * shape_seed(shape))
    return dict(q=_dense_ints(r, (N, W1, D)), a=_dense_ints(r, (N, W2, D)), W=_dense_ints(r, (M, D, D)),
                bias=_dense_ints(r, (M, W1, W2)), dT=_dense_ints(r, (N, M, W1, W2)), dbias_in=_dense_ints(r, (M, W1, W2)))


def simmatrix_dense(shape):
    N, K1, K2 = shape
    r = np.random.default_rng(1701 + 11 * shape_seed(shape))
    return dict(q=_dense_ints(r, (N, K1)), a=_dense_ints(r, (N, K2)), W=_dense_ints(r, (K1, K2)), dT=_dense_ints(r, (N, 1)),
                dW_in=_dense_ints(r, (K1, K2)))


def dense_values(p):
    """The doubles of a dense case: integer 2^-20, exact."""
    return {k: np.ldexp(v.astype(np.float64), -FRAC) for k, v in p.items()}


def bilinear_n(shape, bias_term):
    N, M, W1, W2, D = shape
    return dict(top=D + D + 1 + (1 if bias_term else 0), dW=W1 + N * W2 + 1, dq=D + M * W2 + 1, da=D + M * W1 + 1, dbias=N + 1)


def simmatrix_n(shape):
    N, K1, K2 = shape
    return dict(scratch=K1, top=K1 + K2 + 1, dq=K2 + 1, da=K1 + 1, dW=N + 2)


# fixed-point exponent of every output: the number of factors of 2^-20 in one term
SCALE = dict(top=3, dq=3, da=3, dW=3, dbias=1, scratch=2)


def exact_and_scale(kind, p, bias_term=True):
    """({name: (E, s)}, {name: S}): the exact value of an output is E 2^-s with E an array of Python integers; S is the same
    expression on absolute values, in double (its own rounding, a relative gamma_n, is covered by SLACK)."""
    obj = {k: v.astype(object) for k, v in p.items()}
    absv = {k: np.abs(v) for k, v in dense_values(p).items()}
    if kind == "bilinear":
        E, S = bilinear_ref(obj, bias_term, unit=1 << FRAC), bilinear_ref(absv, bias_term)
    else:
        E, S = simmatrix_ref(obj, unit=1 << FRAC), simmatrix_ref(absv)
    return {k: (v, FRAC * SCALE[k]) for k, v in E.items()}, S


SLACK = 1.0 + 2.0 ** -30                      # S and the final subtraction are themselves computed in double
_split = np.frompyfunc(lambda e: (float(e), e - int(float(e))), 1, 2)


def dense_error(got, E, s):
    """|got - E 2^-s| per element, to a relative 2^-52: E = hi + lo with hi = the nearest double (an integer once |E| >= 2^53,
    so lo is an exact Python integer), and (got - hi) - lo is formed in double."""
    got = np.asarray(got, dtype=np.float64)
    hi, lo = _split(E.reshape(got.shape))
    hi, lo = np.ldexp(hi.astype(np.float64), -s), np.ldexp(lo.astype(np.float64), -s)
    return np.abs((got - hi) - lo)


def check_dense(what, got, E, s, S, n):
    """Every element within gamma_n S; a failure names the worst element.  Returns the largest error in units of gamma_n S."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err, bar = dense_error(got, E, s), gamma(n) * SLACK * np.asarray(S, dtype=np.float64).reshape(got.shape)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%s: n = %d, worst error %.3g of the bar (%.3g u S) at %s" % (what, n, ratio[idx], ratio[idx] * n, idx))
    assert ratio[idx] <= 1.0, "%s: |got - exact| = %.3g > gamma_%d S = %.3g at %s; %d of %d elements over the bar" % (
        what, err[idx], n, bar[idx], idx, int((ratio > 1.0).sum()), ratio.size)
    return float(ratio[idx])


# ----------------------------------------------------------------------------------------------------------------------
# cases, computed once per shape and shared read-only by the tests that need them
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def probe_case(kind, shape):
    """(inputs as doubles, {(name, bias_term): int64 reference}); SimMatrix references are keyed (name, False)."""
    key = ("probe", kind) + tuple(shape)
    if key not in _cases:
        if kind == "bilinear":
            p = bilinear_probe(shape)
            ref = {(k, b): v for b in (False, True) for k, v in bilinear_ref(p, b).items()}
        else:
            p = simmatrix_probe(shape)
            ref = {(k, False): v for k, v in simmatrix_ref(p).items()}
        _cases[key] = (_freeze(f64(p)), _freeze(ref))
    return _cases[key]


def dense_case(kind, shape):
    """(inputs as doubles, {name: (E, s)}, {name: S}), with bias."""
    key = ("dense", kind) + tuple(shape)
    if key not in _cases:
        p = bilinear_dense(shape) if kind == "bilinear" else simmatrix_dense(shape)
        E, S = exact_and_scale(kind, p)
        _cases[key] = (_freeze(dense_values(p)), E, _freeze(S))
    return _cases[key]
