"""Inputs, references and error bars for the cosine SimCross layer (csrc/simcross_rows_cosine.hip,csrc/simcross_cross.hip, csrc/cosine_math.h,
dist_mode 0): q (N, W1, D), a (N, W2, D), top / dT (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2).

  n0_j = sqrt(q_j . q_j)   n1_k = sqrt(a_k . a_k)   T_jk = (q_j . a_k) / n0_j / n1_k          (sim_cross_layer.cpp:112-139)
  dq_j = sum_k g_jk (a_k / n0_j / n1_k - q_j T_jk / (n0_j n0_j))                                (:226-250)
  da_k = sum_j g_jk (q_j / n0_j / n1_k - a_k T_jk / (n1_k n1_k))

Exact-sum probes.  Every entry of q and a is a small integer in [-4, 4] times ONE power of two per operand, so a product is an
integer of at most 16 and every partial sum of a dot product, in ANY order, is an integer below 16 D <= 2^24 (times the power
of two): q.q, a.a and q.a carry no rounding whatever order a kernel or a BLAS adds them in, and what follows them is a fixed
sequence of IEEE operations (sqrtf, two divisions).  The forward is therefore bit for bit the CPU oracle's on every route.
Dense rows hold no zero (a dropped, doubled or misplaced element changes q.q or a.a by at least 1); every fifth row of q and
every seventh of a hold a single nonzero, whose position moves with the row.

Backward bars, counted in roundings of at most u = 2^-24 each of the value rounded; t1 = g other / (n0 n1) and
t2 = g self T / n^2 are the two terms of ONE (j, k) contribution, in exact arithmetic on the fp32 inputs (q, a, g and the
forward's fp32 T, n0, n1):
  factor form (cosine_factors / cosine_grad_fac: cosine_pair32_kernel, cross_bwd_tiled_kernel<float, 0, .>):
      1/n0 and /n1: 2, x other: 1             -> 3 u |t1|
      n0 n0: 1, T / that: 1, x self: 1        -> 3 u |t2|
      the subtraction: 1, x g: 1              -> 2 u |t1 - t2|           total 5 u (|t1| + |t2|), "0 +" is exact
  reference form (cosine_grad_div: cosine_rows_kernel, cross_bwd_plain_kernel<float, 0>, and the CPU oracle):
      other / n0 / n1: 2;  self T: 1, n0 n0: 1, the division: 1;  the subtraction and x g: 2      total 5 u (|t1| + |t2|)
so both forms are held to BAR_GRAD = 5 u / (1 - 5 u) of |t1| + |t2| (the denominator carries the second-order terms).  With
one nonzero g per row (dq) or per column (da) of a word grid an element is ONE such contribution -- the others are g = 0
times a finite value: exact zeros -- and the same bar holds on grids.  The kernels that spell the reference's expression in
the reference's order are compared with the oracle bit for bit instead.

CPU only; tests/test_cosine_model.py checks this module against the CPU oracle, tests/test_gpu_cosine_accuracy.py uses it.
"""
import numpy as np

U24 = 2.0 ** -24
BAR_GRAD = 5.0 * U24 / (1.0 - 5.0 * U24)      # 5 roundings on the path to one term pair (see above)
DENSE_MARGIN = 2.0                            # a tree or butterfly order is no worse than the oracle's sequential one
DENSE_FLOOR = 4.0 * U24                       # where the oracle happens to be exact: a few units of 2^-24

# (N, W1, W2, D) per kernel family; tests/test_gpu_cosine_accuracy.py has the route of every shape
PAIR32 = [(1, 1, 1, 100), (17, 1, 1, 100), (31, 1, 1, 200), (33, 1, 1, 300), (16, 1, 1, 300)]
VEC4 = [(5, 1, 1, 4), (9, 1, 1, 256), (9, 1, 1, 260), (3, 1, 1, 1028), (2, 1, 1, 2100), (7, 1, 1, 304)]
SCALAR = [(9, 1, 1, 7), (5, 1, 1, 1), (6, 1, 1, 65), (4, 1, 1, 301)]
GRID_TILED = [(4, 5, 7, 300), (1030, 40, 40, 52), (1025, 16, 24, 50), (1024, 40, 8, 50), (1023, 16, 24, 50), (3, 41, 9, 33),
              (2, 40, 40, 50), (511, 8, 8, 50), (512, 8, 8, 50), (1024, 5, 7, 20), (600, 40, 40, 50)]
GRID_GENERIC = [(1, 70, 60, 9)]
ROUTES = PAIR32 + VEC4 + SCALAR + GRID_TILED + GRID_GENERIC
FACTOR_FORM = set(PAIR32 + GRID_TILED)        # backward through cosine_factors: held to BAR_GRAD; the others bit for bit
# dense data, one shape per family: pair32, rows vec4 (two trips), rows scalar, 1x1 tiles + tiled split, 2x2 tiles + tiled
# unsplit, image kernel + tiled unsplit, generic backward
DENSE = [(33, 1, 1, 300), (9, 1, 1, 260), (6, 1, 1, 65), (3, 41, 9, 33), (520, 24, 24, 34), (1024, 8, 8, 50), (1, 70, 60, 9)]


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def shape_seed(s):
    return sum((i + 1) * int(v) for i, v in enumerate(s))


# ----------------------------------------------------------------------------------------------------------------------
# exact-sum probes
# ----------------------------------------------------------------------------------------------------------------------
def exact_rows(r, rows, D, e, period, phase):
    """(rows, D) float32, integers in [-4, 4] \\ {0} times 2^e; row i with i % period == phase holds one nonzero, at column
    3 i % D (q: period 5, a: period 7 -- a row that is sparse in both has T = +-1, in one only a one-product q.a)."""
    k = r.integers(1, 5, (rows, D)) * np.where(r.integers(0, 2, (rows, D)) == 0, -1, 1)
    for i in range(phase, rows, period):
        keep = 3 * i % D
        v = k[i, keep]
        k[i] = 0
        k[i, keep] = v
    return np.ldexp(k.astype(np.float64), e).astype(np.float32)


def g_values(r, shape, lo=-4, hi=4):
    """+-{1, 3, 5} 2^e, e in [lo, hi]: three significant bits, so a product with g is exact only by accident."""
    m = r.choice(np.array([1.0, 3.0, 5.0]), shape) * np.where(r.integers(0, 2, shape) == 0, -1.0, 1.0)
    return np.ldexp(m, r.integers(lo, hi + 1, shape)).astype(np.float32)


def dT_one_per_row(r, N, W1, W2):
    """One nonzero per row of each (W1, W2) grid, at column (i + n) % W2: dq elements are single-term."""
    dT = np.zeros((N, 1, W1, W2), np.float32)
    n, i = np.meshgrid(np.arange(N), np.arange(W1), indexing="ij")
    dT[n, 0, i, (i + n) % W2] = g_values(r, (N, W1))
    return dT


def dT_one_per_column(r, N, W1, W2):
    """One nonzero per column, at row (j + n) % W1: da elements are single-term."""
    dT = np.zeros((N, 1, W1, W2), np.float32)
    n, j = np.meshgrid(np.arange(N), np.arange(W2), indexing="ij")
    dT[n, 0, (j + n) % W1, j] = g_values(r, (N, W2))
    return dT


def probe_inputs(r, N, W1, W2, D):
    """q, a: exact-sum rows at their own power of two each (eq, ea); dT_rows / dT_cols: one nonzero per row / column
    (W1 = W2 = 1: the same dense array twice)."""
    eq, ea = int(r.integers(-6, 7)), int(r.integers(-6, 7))
    p = dict(eq=eq, ea=ea, q=exact_rows(r, N * W1, D, eq, 5, 2).reshape(N, W1, D),
             a=exact_rows(r, N * W2, D, ea, 7, 3).reshape(N, W2, D))
    p["dT_rows"] = dT_one_per_row(r, N, W1, W2)
    p["dT_cols"] = p["dT_rows"] if W1 == 1 and W2 == 1 else dT_one_per_column(r, N, W1, W2)
    return p


def integer_sums(q, a, eq, ea):
    """The three dot products in the scaled integers, int64: (sqq (N, W1), saa (N, W2), sqa (N, W1, W2), bound), bound = the
    largest sum of |products| of any of them -- no partial sum of any order exceeds it."""
    qi = np.rint(np.ldexp(q.astype(np.float64), -eq)).astype(np.int64)
    ai = np.rint(np.ldexp(a.astype(np.float64), -ea)).astype(np.int64)
    assert (np.ldexp(qi.astype(np.float64), eq) == q).all() and (np.ldexp(ai.astype(np.float64), ea) == a).all()
    sqq, saa = (qi * qi).sum(-1), (ai * ai).sum(-1)
    sqa = np.matmul(qi, ai.transpose(0, 2, 1))
    bound = max(int(sqq.max()), int(saa.max()), int(np.matmul(np.abs(qi), np.abs(ai).transpose(0, 2, 1)).max()))
    return sqq, saa, sqa, bound


def closed_form_forward(q, a, eq, ea):
    """top, norm0, norm1 in fp32 from the exact sums: sqrtf, then two successive divisions (cosine_math.h: cosine_score)."""
    sqq, saa, sqa, _ = integer_sums(q, a, eq, ea)
    f = lambda s, e: np.ldexp(s.astype(np.float64), e).astype(np.float32)
    with np.errstate(all="ignore"):
        n0, n1 = np.sqrt(f(sqq, 2 * eq)), np.sqrt(f(saa, 2 * ea))
        top = (f(sqa, eq + ea) / n0[:, :, None]) / n1[:, None, :]
    assert top.dtype == np.float32 and n0.dtype == np.float32
    return top[:, None], n0, n1


# ----------------------------------------------------------------------------------------------------------------------
# fp64: the sum of the absolute values of an element's terms (the scale of its error), and the values for cross-checks
# ----------------------------------------------------------------------------------------------------------------------
def top_ref(q, a):
    """(top64 (N, 1, W1, W2), scale): scale = sum_i |q_i a_i| / (n0 n1)."""
    q, a = q.astype(np.float64), a.astype(np.float64)
    n0, n1 = np.sqrt((q * q).sum(-1)), np.sqrt((a * a).sum(-1))
    den = n0[:, :, None] * n1[:, None, :]
    with np.errstate(all="ignore"):
        return (np.matmul(q, a.transpose(0, 2, 1)) / den)[:, None], (np.matmul(np.abs(q), np.abs(a).transpose(0, 2, 1)) / den)[:, None]


def grad_ref(q, a, top, n0, n1, dT):
    """((dq64, dq_scale), (da64, da_scale)) from the fp32 inputs of the backward, all cast to fp64; scale = the sum over the
    element's (j, k) contributions of |t1| + |t2|."""
    q, a, T, n0, n1, g = (np.asarray(x, dtype=np.float64) for x in (q, a, top[:, 0], n0, n1, dT[:, 0]))
    c1 = g / (n0[:, :, None] * n1[:, None, :])                    # (N, W1, W2)
    gT = g * T
    sq, sa = gT.sum(2) / (n0 * n0), gT.sum(1) / (n1 * n1)
    aq, aa = np.abs(gT).sum(2) / (n0 * n0), np.abs(gT).sum(1) / (n1 * n1)
    dq = np.matmul(c1, a) - q * sq[:, :, None]
    da = np.matmul(c1.transpose(0, 2, 1), q) - a * sa[:, :, None]
    mq = np.matmul(np.abs(c1), np.abs(a)) + np.abs(q) * aq[:, :, None]
    ma = np.matmul(np.abs(c1).transpose(0, 2, 1), np.abs(q)) + np.abs(a) * aa[:, :, None]
    return (dq, mq), (da, ma)


def scaled_error(got, ref64, scale):
    """max |got - ref64| / scale and its index; where scale == 0 the element must be exactly ref64."""
    got64 = np.asarray(got, dtype=np.float64)
    assert got64.shape == ref64.shape == scale.shape, (got64.shape, ref64.shape, scale.shape)
    assert np.isfinite(got64).all() and np.isfinite(ref64).all(), "non-finite value in a finite comparison"
    diff = np.abs(got64 - ref64)
    zero = scale == 0
    assert (diff[zero] == 0).all(), "an element whose terms are all zero is not zero"
    e = np.where(zero, 0.0, diff / np.where(zero, 1.0, scale))
    idx = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[idx]), tuple(int(v) for v in idx)


def check(what, got, ref64, scale, bar):
    """scaled_error held to bar; a failure names the worst element.  Returns e."""
    e, idx = scaled_error(got, ref64, scale)
    print("%s: e = %.2f x 2^-24 (bar %.2f x 2^-24), worst at %s" % (what, e / U24, bar / U24, idx))
    if e > bar:
        bad = np.abs(np.asarray(got, dtype=np.float64) - ref64) > bar * scale
        raise AssertionError("%s: scaled error %.3g > %.3g at %s (got %r, fp64 %r); %d of %d elements over the bar, first at %s"
                             % (what, e, bar, idx, np.asarray(got)[idx], ref64[idx], int(bad.sum()), bad.size,
                                tuple(int(v) for v in np.argwhere(bad)[0])))
    return e


def dense_bar(e_oracle):
    """The bar of a dense-data case from the CPU oracle's own scaled error against fp64."""
    return DENSE_MARGIN * e_oracle + DENSE_FLOOR


# ----------------------------------------------------------------------------------------------------------------------
# dense data
# ----------------------------------------------------------------------------------------------------------------------
def dense_inputs(r, N, W1, W2, D):
    """GloVe-like rows (tests/util.py: qa) and a dense dT ~ N(0, 1) 2^s_n, s_n uniform in [-10, 10] per pair."""
    from util import qa
    q, a = qa(r, N, W1, W2, D)
    s = r.integers(-10, 11, (N, 1, 1, 1))
    dT = np.ldexp(r.standard_normal((N, 1, W1, W2)), s).astype(np.float32)
    return q, a, dT


def ldexp32(x, e):
    return np.ldexp(x, np.broadcast_to(e, x.shape).astype(np.int32)).astype(np.float32)


def all_normal(x):
    """Every nonzero element is a finite, normal fp32 magnitude."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    nz = ax[ax != 0]
    return bool(np.isfinite(ax).all() and (nz >= 2.0 ** -126).all() and (nz < 2.0 ** 127).all())


# ----------------------------------------------------------------------------------------------------------------------
# references, computed once per shape and shared read-only by the tests that need them
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def probe_case(oracle, shape):
    """The probe of one shape with the fp32 CPU oracle's forward (top, n0, n1) and, per dT, the fp64 value and scale of dq / da
    from that forward (grad_ref).  The oracle's fp32 backward (dq_o, da_o) only where a kernel is held to its bits."""
    key = ("probe",) + tuple(shape)
    if key not in _cases:
        N, W1, W2, D = shape
        p = probe_inputs(np.random.default_rng(1701 + shape_seed(shape)), *shape)
        p["top"], p["n0"], p["n1"] = oracle.simcross_forward(0, p["q"], p["a"])
        p["dq_ref"], _ = grad_ref(p["q"], p["a"], p["top"], p["n0"], p["n1"], p["dT_rows"])
        _, p["da_ref"] = grad_ref(p["q"], p["a"], p["top"], p["n0"], p["n1"], p["dT_cols"])
        if tuple(shape) not in FACTOR_FORM:
            p["dq_o"], _, _, _ = oracle.simcross_backward(0, p["q"], p["a"], p["top"], p["dT_rows"], norm0=p["n0"], norm1=p["n1"])
            _, p["da_o"], _, _ = oracle.simcross_backward(0, p["q"], p["a"], p["top"], p["dT_cols"], norm0=p["n0"], norm1=p["n1"])
        _cases[key] = _freeze(p)
    return _cases[key]


def dense_case(oracle, shape):
    """Dense data of one shape: the fp32 oracle's results, the fp64 oracle's (on float64 casts of the same fp32 inputs; the
    backward from the fp32 forward's top, n0, n1, which is what the kernels are given too), the per-element scales and the
    oracle's own scaled errors e_o[name]."""
    key = ("dense",) + tuple(shape)
    if key not in _cases:
        q, a, dT = dense_inputs(np.random.default_rng(1701 + 7 * shape_seed(shape)), *shape)
        c = dict(q=q, a=a, dT=dT)
        c["top"], c["n0"], c["n1"] = oracle.simcross_forward(0, q, a)
        c["dq"], c["da"], _, _ = oracle.simcross_backward(0, q, a, c["top"], dT, norm0=c["n0"], norm1=c["n1"])
        f64 = lambda x: x.astype(np.float64)
        top64, _, _ = oracle.simcross_forward(0, f64(q), f64(a))
        dq64, da64, _, _ = oracle.simcross_backward(0, f64(q), f64(a), f64(c["top"]), f64(dT), norm0=f64(c["n0"]), norm1=f64(c["n1"]))
        (dq_np, mq), (da_np, ma) = grad_ref(q, a, c["top"], c["n0"], c["n1"], dT)
        top_np, mt = top_ref(q, a)
        # the vectorised fp64 expressions (used for the scales, and as the probes' reference) agree with the fp64 oracle
        for x, y, m in ((top_np, top64, mt), (dq_np, dq64, mq), (da_np, da64, ma)):
            assert scaled_error(x, y, m)[0] < 2.0 ** -40
        c["ref"] = dict(top=(top64, mt), dq=(dq64, mq), da=(da64, ma))
        c["e_o"] = {k: scaled_error(c[k], *c["ref"][k])[0] for k in ("top", "dq", "da")}
        _cases[key] = _freeze(c)
    return _cases[key]
