"""The FM layer's two loops (the reference's fm_layer.cpp:42-61 and :76-98) restated in numpy for the FM tests.

Vectorised over the samples only: a Python loop over the columns j and the channels k, one numpy operation in the
array's own dtype (float32 or float64) per operation of the reference, in the reference's order.  So every sample's
score is the reference's ordered chain  t1 -= x*x (a rounded product, then a subtraction) ... t1 += t2*t2 ... t1 /= 2,
the linear column, the bias; and bias_diff is a sequential sum from 0 in ascending i."""
import numpy as np


def fm_forward(x, bias=None):
    """x: (N, C, dim) float32 or float64; bias: None or a scalar.  Returns top, shape (N,), dtype of x."""
    x = np.ascontiguousarray(x)
    dt = x.dtype.type
    N, C, dim = x.shape
    t1 = np.zeros(N, dtype=dt)
    for j in range(1, dim):
        t2 = np.zeros(N, dtype=dt)
        for k in range(C):
            v = x[:, k, j]
            t2 = t2 + v
            t1 = t1 - v * v
        t1 = t1 + t2 * t2
    t1 = t1 / dt(2)
    for k in range(C):
        t1 = t1 + x[:, k, 0]
    if bias is not None:
        t1 = t1 + dt(bias)
    assert t1.dtype == x.dtype
    return t1


def fm_backward(x, top_diff):
    """Returns (bottom_diff (N, C, dim), bias_diff scalar), dtype of x."""
    x = np.ascontiguousarray(x)
    dt = x.dtype.type
    N, C, dim = x.shape
    g = np.asarray(top_diff, dtype=x.dtype).reshape(N)
    bias_diff = dt(0)
    for i in range(N):
        bias_diff = dt(bias_diff + g[i])
    bottom_diff = np.empty_like(x)
    for k in range(C):
        bottom_diff[:, k, 0] = g
    for j in range(1, dim):
        tt = np.zeros(N, dtype=dt)
        for k in range(C):
            tt = tt + x[:, k, j]
        for k in range(C):
            bottom_diff[:, k, j] = g * (tt - x[:, k, j])
    return bottom_diff, bias_diff


def fm_closed_form_f64(x, bias=0.0):
    """1/2 sum_j [(sum_k x)^2 - sum_k x^2] + sum_k x_0 + b, in float64 with numpy's own (pairwise) sums."""
    x = np.asarray(x, dtype=np.float64)
    lat = x[:, :, 1:]
    return 0.5 * ((lat.sum(axis=1) ** 2).sum(axis=1) - (lat * lat).sum(axis=(1, 2))) + x[:, :, 0].sum(axis=1) + bias
