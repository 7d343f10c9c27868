"""Inputs, fp64 references and error bars for the bilinear SimCross layer on word grids (csrc/bilinear.hip, dist_mode 2):
q (N, W1, D), a (N, W2, D), W (M, D, D), top / dT (N, M, W1, W2), bias (M, W1, W2).

  T_nm = Q_n W_m A_n^T (+ bias_m)         dQ_n = sum_m dT_nm A_n W_m^T        dA_n = sum_m dT_nm^T Q_n W_m
  dW_m = sum_n Q_n^T dT_nm A_n            dbias = dbias + dT_0 + dT_1 + ...  (n ascending)

The probes make every output element ONE product (for dq and da: one per measure), whichever way an implementation
groups the products -- the kernels form U = dT A and V = dT^T Q first, the CPU oracle (Q^T dT) A, W A^T and Q W:

  * q and a hold one nonzero per word row, at column (row + offset) % D over the flattened (N * W, D) rows, so the
    positions cycle over every k and every j; values are matrix_pipe_model.probe_values (24 significant bits: every
    product is inexact) times 2^e, e in [-8, 8];
  * dT holds +-2^e with one nonzero per ROW of each (W1, W2) grid (probe "rows": U and dq single-term) or one per COLUMN
    (probe "cols": V and da single-term), at a column / row that moves with the pair and the measure; a product with dT is exact;
  * for dW, q holds one nonzero per COLUMN of the flattened (N * W1, D) matrix, a is dense, dT is the "rows" kind;
  * bias is +-2^-(3 + m % 6) of the power-of-two scale of its score: at most 1/8 of the product, its own size per measure.

The bars count fp32 roundings on the path to an element, each at most 2^-24 of the value rounded (derived, not measured):
  top   2 multiplies (x W, then . y); with bias one addition of a value <= 9/8 of the product: 2 + 9/8
  dq    dT . y is exact, one multiply by W per measure and M - 1 additions of partial sums <= sum |p_m|: M
  da    likewise: M
  dW    dT . a is exact, one multiply; every other term of the sum over pairs and words is an exact zero: 1
An accumulation whose other terms are exact zeros adds no rounding.

CPU only; tests/test_bilinear_grid_model.py checks this module against the CPU oracle,
tests/test_gpu_bilinear_grid_accuracy.py uses it on the kernels.
"""
import numpy as np

import matrix_pipe_model as mp

U24 = 2.0 ** -24


def bar_top(bias_term):
    return (2.0 + (9.0 / 8.0 if bias_term else 0.0)) * U24


def bar_dq(M):
    return M * U24


bar_da = bar_dq
BAR_DW = 1.0 * U24


# ----------------------------------------------------------------------------------------------------------------------
# probe inputs
# ----------------------------------------------------------------------------------------------------------------------
def one_per_word_row(r, N, Wn, D, offset, exps):
    """(N, Wn, D) with one nonzero per word row at column (n * Wn + i + offset) % D; exps (N | 1, Wn): the row's power of two."""
    vals = mp.probe_values(r, (N * Wn,))[0].reshape(N, Wn)
    vals = np.ldexp(vals, np.broadcast_to(exps, (N, Wn)).astype(np.int32)).astype(np.float32)
    return mp.one_per_row(vals.reshape(-1), D, offset).reshape(N, Wn, D)


def dT_one_per_row(r, N, M, W1, W2):
    """+-2^e, e in [-4, 4], at dT[n, m, i, (i + n + m) % W2]; zero elsewhere."""
    dT = np.zeros((N, M, W1, W2), np.float32)
    n, m, i = np.meshgrid(np.arange(N), np.arange(M), np.arange(W1), indexing="ij")
    dT[n, m, i, (i + n + m) % W2] = mp.pow2(r, (N, M, W1), -4, 4)
    return dT


def dT_one_per_column(r, N, M, W1, W2):
    """+-2^e, e in [-4, 4], at dT[n, m, (j + n + m) % W1, j]; zero elsewhere."""
    dT = np.zeros((N, M, W1, W2), np.float32)
    n, m, j = np.meshgrid(np.arange(N), np.arange(M), np.arange(W2), indexing="ij")
    dT[n, m, (j + n + m) % W1, j] = mp.pow2(r, (N, M, W2), -4, 4)
    return dT


def probe_inputs(r, N, W1, W2, D, M, bias_term):
    """The three probe calls of one shape: a dict of float32 arrays.
    q, a, W, bias, dT_rows, dT_cols: the forward, dq (dT_rows) and da (dT_cols); q_cols, a_dense: dW (with dT_rows)."""
    # a bias is shared by the pairs, so with one the scale of a score may depend on its word rows only
    eq = r.integers(-8, 9, (1 if bias_term else N, W1))
    ea = r.integers(-8, 9, (1 if bias_term else N, W2))
    p = dict(q=one_per_word_row(r, N, W1, D, 0, eq), a=one_per_word_row(r, N, W2, D, 3, ea),
             W=mp.probe_values(r, (M, D, D))[0], bias=None, dbias0=None)
    if bias_term:
        sign = np.where(r.integers(0, 2, (M, W1, W2)) == 0, -1.0, 1.0)
        # measure m at 2^-(3 + m % 6) of the scale: a bias read from another measure is off by at least 2^-9 of the product
        em = -3 - np.arange(M) % 6
        p["bias"] = (sign * np.ldexp(1.0, (em[:, None, None] + eq[0][None, :, None] + ea[0][None, None, :]))).astype(np.float32)
        p["dbias0"] = (r.integers(-8, 9, (M, W1, W2)) / 4.0).astype(np.float32)
    p["dT_rows"] = dT_one_per_row(r, N, M, W1, W2)
    p["dT_cols"] = dT_one_per_column(r, N, M, W1, W2)
    p["q_cols"] = mp.one_per_column(mp.probe_values(r, (D,))[0], N * W1).reshape(N, W1, D)
    p["a_dense"] = mp.probe_values(r, (N, W2, D))[0]
    return p


def dense_inputs(r, N, W1, W2, D, M, positive=False):
    """The suite's usual data (tests/util.py: qa; W ~ U(+-0.08); bias, dT, dbias0 ~ N(0, 1)); positive: absolute values."""
    q = (r.standard_normal((N, W1, D)) * 0.4).astype(np.float32)
    a = (r.standard_normal((N, W2, D)) * 0.4).astype(np.float32)
    W = r.uniform(-0.08, 0.08, (M, D, D)).astype(np.float32)
    dT = r.standard_normal((N, M, W1, W2)).astype(np.float32)
    if positive:
        q, a, W, dT = np.abs(q), np.abs(a), np.abs(W), np.abs(dT)
    return q, a, W, dT


# ----------------------------------------------------------------------------------------------------------------------
# fp64 references: (value, the same expression over absolute values)
# ----------------------------------------------------------------------------------------------------------------------
def _both(f, *xs):
    xs64 = [np.asarray(x, dtype=np.float64) for x in xs]
    return f(*xs64), f(*[np.abs(x) for x in xs64])


def ref_top(q, a, W, bias=None):
    """(top64, D): top64 includes the bias, D = |q| |W| |a|^T does not (the bias is no product)."""
    t, d = _both(lambda q, a, W: np.matmul(np.matmul(q[:, None], W[None]), a[:, None].transpose(0, 1, 3, 2)), q, a, W)
    if bias is not None:
        t = t + np.asarray(bias, dtype=np.float64)[None]
    return t, d


def ref_dq(a, W, dT):
    return _both(lambda a, W, dT: np.matmul(np.matmul(dT, a[:, None]), W.transpose(0, 2, 1)[None]).sum(axis=1), a, W, dT)


def ref_da(q, W, dT):
    return _both(lambda q, W, dT: np.matmul(np.matmul(dT.transpose(0, 1, 3, 2), q[:, None]), W[None]).sum(axis=1), q, W, dT)


def ref_dW(q, a, dT):
    def f(q, a, dT):
        U = np.matmul(dT, a[:, None])                                   # (N, M, W1, D)
        N, M, W1, D = U.shape
        return np.matmul(q.reshape(N * W1, D).T[None], U.transpose(1, 0, 2, 3).reshape(M, N * W1, D))
    return _both(f, q, a, dT)


def dbias_in_order(dT, dbias0):
    """dbias = dT_n + dbias for n ascending, in fp32 (sim_cross_layer.cpp:301-304): the bits the layer must produce."""
    s = np.array(dbias0, dtype=np.float32, copy=True)
    for n in range(dT.shape[0]):
        s = (dT[n].astype(np.float32) + s).astype(np.float32)
    return s


def check(what, got, ref, bar):
    """Componentwise error of got against ref = (C64, D) held to bar; a failure names the worst element's index.  Returns e."""
    C64, Dm = ref
    e, idx = mp.componentwise_error(got, C64, Dm, what)
    idx = tuple(int(v) for v in idx)
    print("%s: e = %.3g = %.2f x 2^-24 (bar %.3g x 2^-24), worst at %s" % (what, e, e / U24, bar / U24, idx))
    if e > bar:
        bad = np.abs(np.asarray(got, dtype=np.float64) - C64) > bar * Dm
        raise AssertionError("%s: componentwise error %.3g > %.3g at index %s (got %r, fp64 %r); %d of %d elements over the "
                             "bar, first at %s" % (what, e, bar, idx, np.asarray(got)[idx], C64[idx], int(bad.sum()), bad.size,
                                                   tuple(int(v) for v in np.argwhere(bad)[0])))
    return e


# ----------------------------------------------------------------------------------------------------------------------
# power-of-two scaling that must change no bit
# ----------------------------------------------------------------------------------------------------------------------
def ldexp32(x, e):
    return np.ldexp(x, np.broadcast_to(e, x.shape).astype(np.int32)).astype(np.float32)


def scaling(r, N, W1, W2, D, lim=20):
    """Exponents s_k (q column k up, W row k down), c_j (W column j up, a column j down), r_ni (q word row up, dT row down)."""
    return dict(s=r.integers(-lim, lim + 1, D), c=r.integers(-lim, lim + 1, D), r=r.integers(-lim, lim + 1, (N, W1)))


def scale_inputs(q, a, W, dT, sc):
    s, c, rr = sc["s"], sc["c"], sc["r"]
    return (ldexp32(q, rr[:, :, None] + s[None, None, :]), ldexp32(a, -c[None, None, :]),
            ldexp32(W, -s[None, :, None] + c[None, None, :]), ldexp32(dT, -rr[:, None, :, None]))


def scale_outputs(top, dq, da, dW, sc):
    """What the unscaled results become: top rows by 2^r, dq by 2^(-r - s_k), da by 2^(c_j), dW by 2^(s_k - c_j)."""
    s, c, rr = sc["s"], sc["c"], sc["r"]
    return (ldexp32(top, rr[:, None, :, None]), ldexp32(dq, -rr[:, :, None] - s[None, None, :]),
            ldexp32(da, c[None, None, :]), ldexp32(dW, s[None, :, None] - c[None, None, :]))


def all_normal(x):
    """Every nonzero element is a finite, normal fp32 magnitude (x: float32 or an fp64 prediction of an fp32 result)."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    nz = ax[ax != 0]
    return bool(np.isfinite(ax).all() and (nz >= 2.0 ** -126).all() and (nz < 2.0 ** 127).all())
