"""The reference's ConvolutionLayer (conv_layer.cpp, base_conv_layer.cpp) as numpy, generic over the dtype of its
inputs -- float32, float64, and int64 for the exact probes: explicit im2col, one matmul per image and group, the bias
as a rank-one update, col2im for the bottom diff and parameter diffs that are accumulated INTO what the caller passes.

    x, bottom_diff (N, C, H, W)   weight, weight_diff (K, C/group, kh, kw)   bias, bias_diff (K)   top, top_diff (N, K, OH, OW)
"""
import collections

import numpy as np

Shape = collections.namedtuple("Shape", "N C H W K kh kw stride pad group bias")


def S(N, C, H, W, K, kh, kw, stride=1, pad=0, group=1, bias=True):
    return Shape(N, C, H, W, K, kh, kw, stride, pad, group, bias)


# The shapes of the GPU tests (tests/test_gpu_conv.py): the smallest at which each thing can go wrong.
V4_SHAPES = [
    S(3, 4, 40, 40, 32, 5, 5),              # network_v4's first layer in miniature: six row bands per image
    S(3, 32, 9, 9, 64, 5, 5),               # its second: OH*OW = 25, a ragged pixel tile; the weights in chunks
]
GPU_SHAPES = V4_SHAPES + [
    S(1, 5, 11, 13, 7, 3, 3),               # N = 1; OW = 11, odd and smaller than a tile; K = 7, a ragged channel tile
    S(2, 3, 8, 7, 5, 3, 3, bias=False),     # C * kh * kw = 27, no multiple of the MFMA k-step; OW = 5; no bias
    S(2, 4, 10, 6, 6, 5, 1),                # kh != kw
    S(2, 3, 9, 8, 4, 5, 5, pad=2),          # the borders
    S(2, 3, 10, 10, 4, 3, 3, stride=2, pad=1),      # (H + 2 pad - kh) % stride == 1: a row and a column are left over
    S(2, 4, 7, 7, 6, 3, 3, group=2, bias=False),
    S(2, 6, 5, 5, 3, 1, 1),                 # 1 x 1
    S(2, 3, 6, 6, 1, 3, 3),                 # K = 1
    S(70, 2, 14, 14, 3, 3, 3),              # more (image, band) units and more (n, oy) rows than slabs
    S(2, 6, 8, 8, 4, 3, 3, stride=(2, 1), pad=(0, 1), group=2),     # everything at once, h and w apart
]

# The shapes at which the fast route's launch plans (csrc/conv_tile.h: conv_prod_plan; csrc/conv_plans.h:
# conv_wdiff_plan) leave by another branch than the shapes above, which all fit the LDS on the first pass.  What a
# comment says of a plan, tests/test_conv_plans.py reads from the C++ itself (PLANS there); tests/test_gpu_conv_plans.py
# runs the kernels.  Per entry: the shape, the routes of forward, bottom_diff and the parameter diffs (F fast,
# G generic), and mms_conv_workspace_bytes: max(generic slabs, fast slabs) * (K C kh kw + K) * 4.
PLAN_CASES = [
    # forward: a 2 x 2 map, G halves 64 -> 1, then R 2 -> 1 (two bands), and leaves with 3 of 4 channels per chunk
    # (chunks of 3 and 1), MT 2; parameter diff: G decrements 64 -> 23, eight column groups
    (S(3, 4, 12, 12, 17, 11, 11), "FFF", 197880),
    # bottom_diff: MT 4, G 3 -> 1, R 9 -> 1 (nine bands), 3 of 5 channels per chunk; forward: a 1 x 1 map, G 256 -> 32,
    # nine chunks of 4 channels, the last of 1; parameter diff: 42 column groups, G 256 -> 6
    (S(2, 33, 9, 9, 5, 9, 9), "FFF", 106960),
    # a 1 x 1 map with one channel each way, the kernel as large as the image; C kh kw = 81
    (S(3, 1, 9, 9, 1, 9, 9), "FFF", 984),
    # OW = 256, the widest a tile takes: one row per workgroup; W = 258 is too wide for the bottom_diff's tile
    (S(1, 1, 3, 258, 1, 3, 3, bias=False), "FGF", 40),
    # parameter diff: R decrements 6 -> 5, bands of 5 rows and of 1 row, MT 4, four slabs
    (S(2, 3, 6, 40, 33, 1, 1), "FFF", 6336),
    # parameter diff: G 2 -> 1, then R 9 -> 8; forward: 64 channels in chunks of 51 and 13; bottom_diff: MT 4 on two
    # whole images per workgroup
    (S(2, 64, 9, 14, 33, 1, 1), "FFF", 154440),
    # conv_wdiff_plan refuses (one row of 40 channels and its top_diff tile exceed the LDS): the parameter diffs take
    # the generic kernel behind two fast products, and the workspace is the generic kernel's
    (S(2, 40, 3, 130, 1, 3, 1), "FFG", 968),
    # parameter diff: 70 (image, band) units on 35 slabs of 2 with 14 bands per image: slab boundaries inside images
    (S(5, 1, 14, 130, 1, 1, 1), "FFF", 280),
    # forward: two chunks (6 + 2 channels) x two bands of 5 rows; 16 column groups in the parameter diff
    (S(2, 8, 20, 40, 1, 11, 11), "FFF", 77520),
    # forward: G halves 7 -> 4 and stays above one: image groups of 4, 4 and 1; MT 4
    (S(9, 4, 12, 12, 33, 7, 7), "FFF", 1404216),
]
PLAN_SHAPES = [c[0] for c in PLAN_CASES]


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def output_dims(s):
    """conv_layer.cpp:14-21 with dilation 1: (H + 2 pad - kernel) / stride + 1, the division truncating."""
    (sh, sw), (ph, pw) = pair(s.stride), pair(s.pad)
    return (s.H + 2 * ph - s.kh) // sh + 1, (s.W + 2 * pw - s.kw) // sw + 1


def im2col(img, s):
    """(C, H, W) -> (C * kh * kw, OH * OW), zeros where the window leaves the image."""
    (sh, sw), (ph, pw) = pair(s.stride), pair(s.pad)
    OH, OW = output_dims(s)
    C = img.shape[0]
    xp = np.zeros((C, s.H + 2 * ph, s.W + 2 * pw), img.dtype)
    xp[:, ph:ph + s.H, pw:pw + s.W] = img
    col = np.empty((C, s.kh, s.kw, OH, OW), img.dtype)
    for i in range(s.kh):
        for j in range(s.kw):
            col[:, i, j] = xp[:, i:i + sh * (OH - 1) + 1:sh, j:j + sw * (OW - 1) + 1:sw]
    return col.reshape(C * s.kh * s.kw, OH * OW)


def col2im(col, s):
    """(C * kh * kw, OH * OW) -> (C, H, W): every column entry added to the element it was copied from."""
    (sh, sw), (ph, pw) = pair(s.stride), pair(s.pad)
    OH, OW = output_dims(s)
    C = col.shape[0] // (s.kh * s.kw)
    col = col.reshape(C, s.kh, s.kw, OH, OW)
    xp = np.zeros((C, s.H + 2 * ph, s.W + 2 * pw), col.dtype)
    for i in range(s.kh):
        for j in range(s.kw):
            xp[:, i:i + sh * (OH - 1) + 1:sh, j:j + sw * (OW - 1) + 1:sw] += col[:, i, j]
    return xp[:, ph:ph + s.H, pw:pw + s.W].copy()


def conv_forward(s, x, weight, bias=None):
    OH, OW = output_dims(s)
    Cg, Kg, ck = s.C // s.group, s.K // s.group, (s.C // s.group) * s.kh * s.kw
    top = np.empty((s.N, s.K, OH * OW), x.dtype)
    w = weight.reshape(s.K, ck)
    for n in range(s.N):
        col = im2col(x[n], s)
        for g in range(s.group):
            top[n, g * Kg:(g + 1) * Kg] = np.matmul(w[g * Kg:(g + 1) * Kg], col[g * ck:(g + 1) * ck])
        if bias is not None:
            top[n] += bias[:, None] * np.ones((1, OH * OW), x.dtype)
    return top.reshape(s.N, s.K, OH, OW)


def conv_backward(s, x, weight, top_diff, weight_diff=None, bias_diff=None):
    """-> bottom_diff (new), weight_diff, bias_diff (new arrays: the ones passed plus this batch's sums, or None)."""
    OH, OW = output_dims(s)
    Kg, ck = s.K // s.group, (s.C // s.group) * s.kh * s.kw
    w = weight.reshape(s.K, ck)
    td = top_diff.reshape(s.N, s.K, OH * OW)
    dw = None if weight_diff is None else weight_diff.reshape(s.K, ck).copy()
    db = None if bias_diff is None else bias_diff.copy()
    dx = np.empty_like(x)
    for n in range(s.N):
        if db is not None:
            db += np.matmul(td[n], np.ones(OH * OW, x.dtype))
        col = im2col(x[n], s)
        dcol = np.empty_like(col)
        for g in range(s.group):
            k0, k1 = g * Kg, (g + 1) * Kg
            if dw is not None:
                dw[k0:k1] += np.matmul(td[n, k0:k1], col[g * ck:(g + 1) * ck].T)
            dcol[g * ck:(g + 1) * ck] = np.matmul(w[k0:k1].T, td[n, k0:k1])
        dx[n] = col2im(dcol, s)
    return dx, (None if dw is None else dw.reshape(weight.shape)), db


def _arrays(s):
    OH, OW = output_dims(s)
    return dict(x=(s.N, s.C, s.H, s.W), weight=(s.K, s.C // s.group, s.kh, s.kw), bias=(s.K,),
                top_diff=(s.N, s.K, OH, OW), weight_diff0=(s.K, s.C // s.group, s.kh, s.kw), bias_diff0=(s.K,))


# Scales of the conditioned inputs: x ~ 0.5 N(0, 1); weight ~ U(-a, a) with a = 1 / sqrt(C/group * kh * kw), so that top
# is O(1); bias ~ 0.1 N(0, 1); top_diff ~ 0.1 N(0, 1); the diffs to accumulate into ~ 0.1 N(0, 1).
def conditioned_inputs(s, dtype, seed):
    r = np.random.default_rng(seed)
    sh = _arrays(s)
    a = 1.0 / np.sqrt((s.C // s.group) * s.kh * s.kw)
    out = dict(x=0.5 * r.standard_normal(sh["x"]), weight=r.uniform(-a, a, sh["weight"]),
               bias=0.1 * r.standard_normal(sh["bias"]), top_diff=0.1 * r.standard_normal(sh["top_diff"]),
               weight_diff0=0.1 * r.standard_normal(sh["weight_diff0"]),
               bias_diff0=0.1 * r.standard_normal(sh["bias_diff0"]))
    out = {k: v.astype(dtype) for k, v in out.items()}
    if not s.bias:
        out["bias"] = out["bias_diff0"] = None
    return out


def integer_probe(s, seed):
    """Every array as int64 in [-4, 4]: a product is at most 16 in size, so a sum of `count` of them is exact in float32
    while count * 16 < 2^24 (probe_bound)."""
    r = np.random.default_rng(seed)
    out = {k: r.integers(-4, 5, v, dtype=np.int64) for k, v in _arrays(s).items()}
    if not s.bias:
        out["bias"] = out["bias_diff0"] = None
    return out


def probe_bound(s):
    """The largest |partial sum| any order of any path can meet on integer_probe inputs, from the shape alone."""
    OH, OW = output_dims(s)
    forward = 16 * (s.C // s.group) * s.kh * s.kw + 4              # the products, then the bias
    bottom = 16 * (s.K // s.group) * s.kh * s.kw
    weight = 16 * s.N * OH * OW + 4                                 # the batch's products, then the diff passed in
    bias = 4 * s.N * OH * OW + 4
    return max(forward, bottom, weight, bias)


def model_outputs(s, inp, dtype):
    """Forward and backward at `dtype` on inp (cast to it) -> {"top", "bottom_diff", "weight_diff"[, "bias_diff"]}."""
    c = {k: (None if v is None else v.astype(dtype)) for k, v in inp.items()}
    top = conv_forward(s, c["x"], c["weight"], c["bias"])
    dx, dw, db = conv_backward(s, c["x"], c["weight"], c["top_diff"], c["weight_diff0"], c["bias_diff0"])
    out = dict(top=top, bottom_diff=dx, weight_diff=dw)
    if db is not None:
        out["bias_diff"] = db
    return out
