"""The model of include/mms_pool.h: pooling_layer.cpp's loops (:90-105 the output size, :140-220 the forward, :229-307 the
backward) and tanh_layer.cpp's backward (:29-32), restated literally in numpy.  The loops over (ph, pw) and over a
window's (h, w) are the reference's, in its order; the planes, which the reference walks one after another and which
share nothing, are carried along as one array axis.  Every operation is one numpy operation on arrays of the element
type, so it is rounded once in that type.

Also the shape lists of tests/test_gpu_pool.py, each shape chosen for a way a kernel can go wrong."""
import collections

import numpy as np

AVE, MAX, STOCHASTIC = 0, 1, 2                     # MMS_POOL_*
METHODS = {"ave": AVE, "max": MAX}
OK, INVALID, UNSUPPORTED = 0, 1, 2                # include/mms.h
FLT_MAX = np.finfo(np.float32).max

# dims (N, C, H, W); kernel, stride, pad as (h, w)
Shape = collections.namedtuple("Shape", "dims kernel stride pad")


def S(dims, k, s=1, p=0):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return Shape(tuple(dims), pair(k), pair(s), pair(p))


def shape_id(sh):
    return "x".join(map(str, sh.dims)) + "_k%dx%d_s%dx%d_p%dx%d" % (sh.kernel + sh.stride + sh.pad)


def _out_dim(size, k, s, p, any_pad):
    o = int(np.ceil(np.float32(size + 2 * p - k) / np.float32(s))) + 1
    if any_pad:
        while o > 1 and (o - 1) * s >= size + p:
            o -= 1
    return o


def judge(sh, method=AVE):
    """(return code, PH, PW) as the header's refusal table has it for a shape (up to the element counts)."""
    (N, C, H, W), (kh, kw), (sh_, sw), (ph, pw) = sh
    if N < 0 or min(C, H, W, kh, kw, sh_, sw) < 1 or ph < 0 or pw < 0 or ph >= kh or pw >= kw:
        return INVALID, None, None
    if method == STOCHASTIC:
        return UNSUPPORTED, None, None
    if method not in (AVE, MAX):
        return INVALID, None, None
    any_pad = ph != 0 or pw != 0
    PH, PW = _out_dim(H, kh, sh_, ph, any_pad), _out_dim(W, kw, sw, pw, any_pad)
    if PH < 1 or PW < 1:
        return INVALID, None, None
    if (PH - 1) * sh_ >= H + ph or (PW - 1) * sw >= W + pw:
        return UNSUPPORTED, None, None
    return OK, PH, PW


def output_dims(sh):
    rc, PH, PW = judge(sh)
    assert rc == OK, (sh, rc)
    return PH, PW


def _windows(sh):
    """(ph, pw) in the reference's order"""
    PH, PW = output_dims(sh)
    return [(ph, pw) for ph in range(PH) for pw in range(PW)]


def _max_window(sh, ph, pw):
    (_, _, H, W), (kh, kw), (sh_, sw), (pad_h, pad_w) = sh
    hs, ws = ph * sh_ - pad_h, pw * sw - pad_w
    he, we = min(hs + kh, H), min(ws + kw, W)
    return max(hs, 0), he, max(ws, 0), we


def _ave_window(sh, ph, pw):
    """-> the clipped window and pool_size, which is taken before the clip to the image"""
    (_, _, H, W), (kh, kw), (sh_, sw), (pad_h, pad_w) = sh
    hs, ws = ph * sh_ - pad_h, pw * sw - pad_w
    he, we = min(hs + kh, H + pad_h), min(ws + kw, W + pad_w)
    pool_size = (he - hs) * (we - ws)
    return max(hs, 0), min(he, H), max(ws, 0), min(we, W), pool_size


def forward(sh, method, bottom):
    """-> top, mask (int32; None for AVE); top_mask is mask in the element type"""
    N, C, H, W = sh.dims
    T = bottom.dtype.type
    PH, PW = output_dims(sh)
    b = bottom.reshape(N * C, H, W)
    if method == MAX:
        top = np.full((N * C, PH, PW), T(-FLT_MAX), dtype=T)
        mask = np.full((N * C, PH, PW), -1, dtype=np.int32)
        for ph, pw in _windows(sh):
            hs, he, ws, we = _max_window(sh, ph, pw)
            for h in range(hs, he):
                for w in range(ws, we):
                    v = b[:, h, w]
                    rep = v > top[:, ph, pw]
                    top[:, ph, pw] = np.where(rep, v, top[:, ph, pw])
                    mask[:, ph, pw] = np.where(rep, h * W + w, mask[:, ph, pw])
        return top.reshape(N, C, PH, PW), mask.reshape(N, C, PH, PW)
    top = np.zeros((N * C, PH, PW), dtype=T)
    for ph, pw in _windows(sh):
        hs, he, ws, we, pool_size = _ave_window(sh, ph, pw)
        for h in range(hs, he):
            for w in range(ws, we):
                top[:, ph, pw] = top[:, ph, pw] + b[:, h, w]
        top[:, ph, pw] = top[:, ph, pw] / T(pool_size)
    return top.reshape(N, C, PH, PW), None


def backward(sh, method, top_diff, mask=None, swap=None):
    """bottom_diff.  mask: int32 or the element type (a top_mask).  The header's two deviations: an entry of -1, or one
    outside its own window, adds nothing.  swap = k exchanges steps k and k + 1 of the (ph, pw) walk: what the order
    probes hold against."""
    N, C, H, W = sh.dims
    T = top_diff.dtype.type
    PH, PW = output_dims(sh)
    td = top_diff.reshape(N * C, PH, PW)
    bd = np.zeros((N * C, H * W), dtype=T)
    walk = _windows(sh)
    if swap is not None:
        walk[swap], walk[swap + 1] = walk[swap + 1], walk[swap]
    rows = np.arange(N * C)
    for ph, pw in walk:
        if method == MAX:
            m = mask.reshape(N * C, PH, PW)[:, ph, pw]
            if m.dtype != np.int32:                          # a top_mask: 0 <= entry < H * W counts as (int)entry
                okv = (m >= 0) & (m < H * W)
                m = np.where(okv, m, -1).astype(np.int64)
            m = m.astype(np.int64)
            hs, he, ws, we = _max_window(sh, ph, pw)
            h, w = m // W, m % W
            inside = (m >= 0) & (h >= hs) & (h < he) & (w >= ws) & (w < we)
            r, i = rows[inside], m[inside]
            bd[r, i] = bd[r, i] + td[r, ph, pw]
        else:
            hs, he, ws, we, pool_size = _ave_window(sh, ph, pw)
            q = td[:, ph, pw] / T(pool_size)
            for h in range(hs, he):
                for w in range(ws, we):
                    bd[:, h * W + w] = bd[:, h * W + w] + q
    return bd.reshape(N, C, H, W)


def tanh_backward(top, top_diff):
    t = top * top
    u = top.dtype.type(1) - t
    return top_diff * u


# ---- the shapes of tests/test_gpu_pool.py ---------------------------------------------------------------------------
SHAPES = [
    S((2, 3, 8, 8), 4, 4),                        # tiling
    S((2, 32, 36, 36), 4, 4),                     # network_v4 pool0
    S((3, 64, 5, 5), 5, 1),                       # pool1 of all three nets: the whole map
    S((3, 2, 8, 10), 3, 2),                       # clipped last window, no padding
    S((2, 2, 7, 7), 3, 2, 1),                     # padding
    S((1, 1, 3, 3), 2, 2, 1),                     # the padding decrement fires
    S((1, 2, 5, 6), 3, 1, 2),                     # maximal pad
    S((1, 2, 5, 6), (3, 2), 1, (2, 0)),           # unequal pads
    S((2, 2, 6, 11), (2, 5), (1, 3)),             # non-square kernel and stride
    S((1, 2, 7, 7), 2, 3),                        # stride > kernel: elements no window reaches
    S((2, 4, 36, 36), 36, 1),                     # the whole map, a 1296-long chain
    S((2, 3, 7, 9), 3, 1),                        # a W for every residue mod 4
    S((2, 3, 7, 10), 3, 1),
    S((2, 3, 7, 11), 3, 1),
    S((2, 3, 7, 12), 3, 1),
    S((70000, 1, 2, 2), 2, 1),                    # more than 65,535 planes
]
# One shape on each side of every branch of the forward's plan (csrc/pool_plans.h), for the float and the double cap
# of 4096 and 2048 elements: the largest plane that is staged whole and the smallest that is cut into bands; a window as
# high as the map whose rows just fit and one whose rows do not (the direct route).  The call whose items outnumber
# the workgroups is test_gpu_pool's own (it tiles one plane).
PLAN_SHAPES = [
    S((1, 2, 64, 64), 3, 2, 1),                   # float: 4096 elements, staged whole;  double: bands
    S((1, 2, 65, 64), 3, 2, 1),                   # float: bands
    S((1, 2, 32, 64), 3, 2, 1),                   # double: 2048 elements, staged whole
    S((1, 2, 33, 64), 3, 2, 1),                   # double: bands
    S((1, 2, 65, 64), (64, 3), 1),                # float: 64 rows of 64 just fit a band;  double: direct
    S((1, 2, 66, 64), (65, 3), 1),                # float: direct
    S((1, 2, 34, 64), (33, 64), 1, (0, 3)),       # double: direct, padded
]
PLAN_ROUTES = {                                    # shape -> (float route, double route): 0 staged, 1 banded, 2 direct
    0: (0, 1), 1: (1, 1), 2: (0, 0), 3: (0, 1), 4: (1, 2), 5: (2, 2), 6: (0, 2),
}


# Calls whose items outnumber the workgroups of the largest grid (2048), by element size: the staged route, 3 planes
# (float) and 1 plane (double) per item; and the direct route, 256 outputs per item.  The planes repeat a few distinct
# ones (tests/test_gpu_pool.py), so the model runs on those.
LOOP_SHAPES = {4: S((6145, 1, 36, 36), 3, 2), 8: S((2049, 1, 36, 36), 3, 2)}
DIRECT_LOOP_SHAPES = {4: S((1025, 1, 1, 4097), (1, 8), (1, 8)), 8: S((2050, 1, 1, 2049), (1, 8), (1, 8))}


def order_probe(method, dtype):
    """-> shape, bottom, top_diff, swap: a (1, 1, 5, 5) map whose centre receives the nine contributions
    big, 1, -big, -big, big, 1, 1, -big, big in the order of the walk, big = 2^24 in float and 2^53 in double, so that
    big + 1 rounds to big and the sum (2 in this order) depends on the order; exchanging steps swap and swap + 1 of the
    walk, the centre's second and third contribution, changes it to 3.  MAX: 3 x 3 windows at
    stride 1, the centre the maximum of all nine.  AVE: the same windows padded by 1 (every pool_size is 9), top_diff
    in multiples of 9."""
    big = float(2 ** 24 if dtype == np.float32 else 2 ** 53)
    pattern = (big, 1.0, -big)
    x = np.zeros((1, 1, 5, 5), dtype)
    x[0, 0, 2, 2] = 1
    if method == MAX:
        sh, scale, swap = S((1, 1, 5, 5), 3, 1), 1.0, 1
    else:
        sh, scale, swap = S((1, 1, 5, 5), 3, 1, 1), 9.0, 7
    PH, PW = output_dims(sh)
    if method == MAX:                       # the nine windows are the nine contributions
        seq = [pattern[i] for i in (0, 1, 2, 2, 0, 1, 1, 2, 0)]
    else:                                   # windows 6-8, 11-13, 16-18 of the 25 hold the centre: k % 3 gives the same
        seq = [scale * pattern[k % 3] for k in range(PH * PW)]
    td = np.array(seq, dtype).reshape(1, 1, PH, PW)
    return sh, x, td, swap


def integer_bottom(sh, dtype, rng, lo=-8, hi=9):
    return rng.integers(lo, hi, sh.dims).astype(dtype)
