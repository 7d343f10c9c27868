"""Accuracy tools for the split-bf16 matrix products (csrc/bx3_gemm.h): the componentwise error metric against fp64,
input generators that pin every kept plane product on its own, and a numpy model of the kernels' arithmetic.

The contract under test (include/mms.h, DESIGN.md "Numerics"): an fp32 operand is the exact sum of three bf16 planes
x = h + m + l; of the nine plane products of a.b the six of weight >= 2^-16 are kept -- in the kernels' order
l.h, h.l, m.m, m.h, h.m, h.h -- and accumulated in fp32, the three of weight <= 2^-24 dropped.  A half operand is
h + m exactly (third plane zero): five products.

CPU only; tests/test_matrix_pipe_model.py checks this module, tests/test_gpu_matrix_pipe_accuracy.py uses it.
"""
import numpy as np

# (plane of A, plane of B) in the order bx3_kernel and bx3_tn_kernel issue their MFMAs per k-step
TERMS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
TERMS_HALF_A = tuple(t for t in TERMS if t[0] != "l")          # a half A operand has no third plane

# The probe bar.  One output element of a probe is ONE fp32 x fp32 product p, assembled from six exact plane products
# by five fp32 additions.  Each partial sum is <= 1.02 |p|; budgeting every addition at a whole ulp (2^-23 |p|, which
# also covers an accumulator that truncates) gives 10 * 2^-24, the three dropped products add <= 3 * 2^-24, and an
# entry point applies at most two more fp32 roundings of <= 1.125 * 2^-24 each (the score's multiply by a_i; the
# accumulation onto an existing dW, or the bias, of <= 1/8 of the product; a half-valued dq has its store's half-ulp
# allowed separately).  10 + 3 + 2.25 < 16: e <= 16 * 2^-24 = 2^-20.
BAR = 2.0 ** -20
# A kept term that is lost moves the result by at least 0.9 * 2^-18 (see probe_values): 3.6 x the bar.
LOST_TERM_MIN = 0.9 * 2.0 ** -18


# ----------------------------------------------------------------------------------------------------------------------
# bf16 rounding and the plane split, as the kernels do it
# ----------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32; integer arithmetic on the bit pattern."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def split3(x):
    """x (float32) -> planes (h, m, l), float32 arrays holding bf16 values, h + m + l == x exactly."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r1 = (x - h).astype(np.float32)          # exact in fp32
    m = bf16_rne(r1)
    r2 = (r1 - m).astype(np.float32)         # exact in fp32
    l = bf16_rne(r2)
    return h, m, l


def planes(x, half=False):
    h, m, l = split3(x)
    if half:
        l = np.zeros_like(l)                 # the half-operand code never forms the third plane
    return {"h": h, "m": m, "l": l}


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def probe_values(r, shape, half=False):
    """Values x = s (H + M + L), s = +-1, whose split is exactly (sH, sM, sL) and whose planes have known weight.

    fp32: H = 1 + i/128, i < 32 (bf16's grid in [1, 1.25)); M = 2^-9 (1.5 + i/128), i < 60 (below half an ulp of H,
    8 significant bits); L = 2^-18 (1.5 + j/32), j < 16 (below half an ulp of M; lowest bit 2^-23, so the sum is an
    fp32 number).  Relative to a product x y <= 1.25^2 the three smallest kept terms are at least
    l.h, h.l >= 1.5 * 2^-18 / 1.25^2 = 0.96 * 2^-18 and m.m >= 2.25 * 2^-18 / 1.25^2 = 1.44 * 2^-18.
    half: H as above, M = +-3 * 2^-10 (the low mantissa bits of an 11-bit half in [1, 1.25); below half an ulp of H),
    third plane zero.  Against an fp32 operand of the form above the smallest kept terms are h.l >= 0.96 * 2^-18 and
    m.m >= 3 * 2^-10 * 1.5 * 2^-9 / 1.25^2 = 1.44 * 2^-18; against another half operand m.m = 9 * 2^-20 / 1.25^2 = 1.44 * 2^-18.

    Returns (x, H, M, L) with the sign folded into the planes; dtype float32 (float16-exact when half)."""
    s = np.where(r.integers(0, 2, shape) == 0, -1.0, 1.0)
    H = 1.0 + r.integers(0, 32, shape) / 128.0
    if half:
        M = np.where((r.integers(0, 2, shape) == 0) & (H > 1.0), -3.0, 3.0) * 2.0 ** -10   # (1 - M leaves the binade)
        L = np.zeros(shape)
    else:
        M = 2.0 ** -9 * (1.5 + r.integers(0, 60, shape) / 128.0)
        L = 2.0 ** -18 * (1.5 + r.integers(0, 16, shape) / 32.0)
    x = s * (H + M + L)
    x32 = x.astype(np.float32)
    assert (x32.astype(np.float64) == x).all()
    if half:
        assert (x32.astype(np.float16).astype(np.float64) == x).all()
    return x32, (s * H).astype(np.float32), (s * M).astype(np.float32), (s * L).astype(np.float32)


def pow2(r, shape, lo, hi, signed=True):
    """+-2^e, e uniform in [lo, hi], as float32 (exact scales)."""
    v = np.ldexp(1.0, r.integers(lo, hi + 1, shape))
    if signed:
        v = v * np.where(r.integers(0, 2, shape) == 0, -1.0, 1.0)
    return v.astype(np.float32)


def one_per_row(vals, K, offset=0):
    """(N, K) matrix with ONE nonzero per row: A[i, (i + offset) % K] = vals[i] -- the streamed operand of bx3_kernel;
    over K consecutive rows every k position is hit once."""
    N = vals.shape[0]
    A = np.zeros((N, K), dtype=vals.dtype)
    A[np.arange(N), (np.arange(N) + offset) % K] = vals
    return A


def tn_rows(N, K1):
    """Pair index n_i of column i's single nonzero for the split-K weight gradient (contraction over the N pairs):
    n_i = (N - 1 - stride * i) mod N with the smallest odd stride >= N / K1 that is coprime to N.  Column 0 sits on the
    last pair (the ragged last chunk), the columns are distinct pairs, an odd stride visits every position of a 32-pair
    step within 32 columns, and the K1 columns span all N pairs, so every split-K chunk of at least `stride` pairs is hit
    (chunks are 64 pairs or more: bx3_tn_pick_chunks)."""
    stride = max(1, -(-N // K1)) | 1
    while np.gcd(stride, N) != 1:
        stride += 2
    return (N - 1 - stride * np.arange(K1)) % N


def one_per_column(vals, N, offset=0):
    """(N, K1) matrix with ONE nonzero per column i, at row (tn_rows(N, K1)[i] + offset) % N."""
    K1 = vals.shape[0]
    A = np.zeros((N, K1), dtype=vals.dtype)
    A[(tn_rows(N, K1) + offset) % N, np.arange(K1)] = vals
    return A


def dense_inputs(r, N, K1, K2, positive=False):
    """The suite's usual data (tests/util.py: qa; W ~ U(+-0.08); dT ~ N(0, 1)); positive: absolute values."""
    q = (r.standard_normal((N, K1)) * 0.4).astype(np.float32)
    a = (r.standard_normal((N, K2)) * 0.4).astype(np.float32)
    W = r.uniform(-0.08, 0.08, (K1, K2)).astype(np.float32)
    dT = r.standard_normal((N, 1)).astype(np.float32)
    if positive:
        q, a, W, dT = np.abs(q), np.abs(a), np.abs(W), np.abs(dT)
    return q, a, W, dT


def all_planes_normal(x):
    """Every nonzero plane of every element is a normal, finite fp32 (and hence bf16: same exponent range) number."""
    ok = np.isfinite(x).all()
    for p in split3(x):
        nz = p[p != 0]
        ok = ok and bool((np.abs(nz) >= 2.0 ** -126).all()) and bool(np.isfinite(nz).all())
    return bool(ok)


# ----------------------------------------------------------------------------------------------------------------------
# the metric
# ----------------------------------------------------------------------------------------------------------------------
def componentwise_error(C, C64, D, what="", allow=None):
    """e = max over D > 0 of (|C - C64| - allow) / D; elements with D == 0 must be exactly zero (either sign).
    allow (optional, same shape): an absolute allowance per element (the RNE half-ulp of an output stored as half).
    Returns (e, index of the worst element)."""
    C = np.asarray(C, dtype=np.float64)
    assert C.shape == C64.shape == D.shape, (what, C.shape, C64.shape, D.shape)
    assert np.isfinite(C).all(), "%s: non-finite output" % what
    zero = D == 0
    assert (C[zero] == 0).all(), "%s: %d elements with |A|.|B| = 0 are not zero" % (what, int((C[zero] != 0).sum()))
    err = np.abs(C - C64)
    if allow is not None:
        err = np.maximum(err - allow, 0.0)
    rel = np.where(zero, 0.0, err / np.where(zero, 1.0, D))
    idx = np.unravel_index(int(np.argmax(rel)), rel.shape) if rel.size else ()
    return (float(rel[idx]) if rel.size else 0.0), idx


def half_ulp_of_half(x64):
    """RNE half-ulp of IEEE half at the magnitude of x64 (normal range; below it the subnormal spacing 2^-24)."""
    ax = np.abs(np.asarray(x64, dtype=np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.maximum(e, -14.0)
    return 0.5 * 2.0 ** (e - 10)


def name_lost_term(x, y, got, a_half=False):
    """For single products x * y (fp32 arrays, elementwise) that came out as `got`: the kept plane product whose absence
    explains the residues best (least squares over the elements given), as "a.<plane> x b.<plane>", and the median residue in
    units of that term -- 1.00 when exactly that product is missing."""
    x, y = np.atleast_1d(np.asarray(x, dtype=np.float32)), np.atleast_1d(np.asarray(y, dtype=np.float32))
    pa, pb = planes(x, a_half), planes(y)
    prod = x.astype(np.float64) * y.astype(np.float64)
    resid = (prod - np.atleast_1d(np.asarray(got, dtype=np.float64))) / prod
    best = None
    for ta, tb in (TERMS_HALF_A if a_half else TERMS):
        t = pa[ta].astype(np.float64) * pb[tb].astype(np.float64) / prod
        if not t.any():
            continue
        score = float(np.sum((resid - t) ** 2))
        if best is None or score < best[0]:
            best = (score, "a.%s x b.%s" % (ta, tb), float(np.median(resid[t != 0] / t[t != 0])))
    return "the residues look like a lost %s (median %.2f of that term)" % (best[1], best[2])


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def model_product(A, B, drop=None, a_half=False, kstep=16, chunk=None):
    """C = A . B as the kernels form it: planes by RNE split, per k-step of `kstep` (16: bx3_kernel, 32: bx3_tn_kernel)
    one MFMA per kept term in the kernels' order, each adding the step's exact plane products to the fp32 accumulator
    with one rounding.  drop: a term of TERMS to leave out (the mutation).  chunk: split-K -- the contraction is cut into
    chunks of that many k, each accumulated from zero, the slabs then summed in order in fp32 (splitk_reduce_kernel)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32)
    K = A.shape[1]
    pa = {k: v.astype(np.float64) for k, v in planes(A, a_half).items()}
    pb = {k: v.astype(np.float64) for k, v in planes(B).items()}
    terms = [t for t in (TERMS_HALF_A if a_half else TERMS) if t != drop]
    total = None
    for c0 in range(0, K, chunk or K):
        c1 = min(K, c0 + (chunk or K))
        acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
        for k0 in range(c0, c1, kstep):
            ks = slice(k0, min(k0 + kstep, c1))
            for ta, tb in terms:
                acc = (acc.astype(np.float64) + pa[ta][:, ks] @ pb[tb][ks, :]).astype(np.float32)
        total = acc if total is None else (total + acc).astype(np.float32)
    return total


def reference(A, B):
    """(C64, D): the fp64 product and the fp64 product of absolute values."""
    A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return A64 @ B64, np.abs(A64) @ np.abs(B64)


# ----------------------------------------------------------------------------------------------------------------------
# the probe check (tests/test_gpu_matrix_pipe_accuracy.py, tests/test_gpu_triplet_simmatrix_fused.py)
# ----------------------------------------------------------------------------------------------------------------------
def check_probe(what, got, A, B, rowscale=None, extra=None, single=None, a_half=False, half_out=False):
    """got ~ rowscale * (A . B) + extra at the probe bar.  single = (x, y): the two factors of each output element (arrays that
    broadcast to got's shape), used to NAME the plane product a failure has lost."""
    C64, D = reference(A, B)
    rs = None if rowscale is None else np.asarray(rowscale, dtype=np.float64).reshape(-1, 1)
    if rs is not None:
        C64, D = C64 * rs, D * np.abs(rs)
    if extra is not None:
        C64 = C64 + np.asarray(extra, dtype=np.float64)
    allow = half_ulp_of_half(C64) if half_out else None
    e, idx = componentwise_error(got, C64, D, what, allow)
    print("%s: e = %.3g (bar %.3g), worst at %s" % (what, e, BAR, idx))
    if e > BAR:
        hint = ""
        if single is not None and not half_out:
            g = np.asarray(got, dtype=np.float64)
            if extra is not None:
                g = g - np.asarray(extra, dtype=np.float64)
            if rs is not None:
                g = g / rs
            x, y = np.broadcast_arrays(*single)
            bad = (np.abs(np.asarray(got, dtype=np.float64) - C64) > BAR * D)
            hint = "; %d of %d elements over the bar, first at %s; %s" % (
                int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]), name_lost_term(x[bad], y[bad], g[bad], a_half))
        raise AssertionError("%s: componentwise error %.3g > %.3g at %s%s" % (what, e, BAR, idx, hint))
    return e


def diag_of(A, K, offset=0):
    i = np.arange(A.shape[0])
    return A[i, (i + offset) % K]
