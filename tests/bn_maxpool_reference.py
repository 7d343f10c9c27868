"""BN -> max pooling over windows that tile the map -> in-place TanH as numpy, generic over the dtype of its inputs.

(a) forward / backward: the THREE reference layers in sequence -- bn_reference.bn_forward; pooling_layer.cpp:149-170
    restated for stride == kernel and no padding: the window's BN outputs scanned in (h, w) order, an element taken
    where it is strictly greater than the best so far, its index kept as the mask (the scan starts from the window's
    first element, not from -FLT_MAX: the same on finite inputs); tanh_layer.cpp:13-33 -- and their backwards: TanH,
    the scatter of top_diff to the mask (:269-287), bn_reference.bn_backward.
(b) fused_forward / fused_backward: the algebra of include/mms_bn_maxpool.h in the inputs' dtype with bn_reference's
    plainly sequential sums, which tests/test_bn_maxpool_reference.py holds against the float64 run of (a) to show that
    the inputs leave the kernels room under the 1e-5 bar.

x and bottom_diff are (N, C, H, W); top, top_diff, save_pool are (N, C, H/kh, W/kw); everything else has C elements.
"""
import numpy as np

import bn_pool_reference as P
import bn_reference as B

TRAIN, TEST, BN_MEMORY, VAR_EPS = B.TRAIN, B.TEST, B.BN_MEMORY, B.VAR_EPS

# bn_pool_reference's shapes plus network_v5's three windows (2 x 2 on an even map of 38 and of 16, 6 x 6 on a 6 x 6 map)
PARITY_SHAPES = P.PARITY_SHAPES + [(2, 3, 38, 38, 2, 2), (3, 2, 16, 16, 2, 2), (3, 2, 6, 6, 6, 6)]
THRESHOLD_SHAPES = P.THRESHOLD_SHAPES
ZERO_SCALE_SHAPE = (2, 3, 4, 6, 2, 3)      # its last channel has scale == 0
GAP = 1e-4                                 # the least top-two gap of a window's BN outputs, relative to max(1, |y|)
OUTPUTS = P.OUTPUTS
pooled_shape = P.pooled_shape


def windows(a, kh, kw):
    """(N, C, H, W) -> (N, C, H/kh, W/kw, kh*kw): each window's elements in (h, w) order (a copy)."""
    N, C, H, W = a.shape
    return a.reshape(N, C, H // kh, kh, W // kw, kw).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, H // kh, W // kw, kh * kw)


def unwindows(w, kh, kw):
    """The inverse of windows."""
    N, C, PH, PW, _ = w.shape
    return np.ascontiguousarray(w.reshape(N, C, PH, PW, kh, kw).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, PH * kh, PW * kw))


def first_max(y, kh, kw):
    """-> (the window maxima, the mask: each window's index of the first element strictly greater than all before)."""
    w = windows(y, kh, kw)
    best, mask = w[..., 0].copy(), np.zeros(w.shape[:-1], np.int64)
    for k in range(1, kh * kw):
        take = w[..., k] > best
        best = np.where(take, w[..., k], best)
        mask = np.where(take, k, mask)
    return best, mask


def scatter(g, mask, kh, kw):
    """(N, C, PH, PW) -> (N, C, H, W): g at each window's mask, 0 elsewhere."""
    w = np.zeros(g.shape + (kh * kw,), g.dtype)
    np.put_along_axis(w, mask[..., None], g[..., None], axis=-1)
    return unwindows(w, kh, kw)


def forward(x, kernel, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY, phase=TRAIN):
    """-> top, save_pool, save_mean, save_std, running_mean, running_var (the layers in sequence; save_pool is BN's
    normalised map at the mask, which the layers never form on its own)."""
    kh, kw = kernel
    N, C, H, W = x.shape
    y, mean, std, rm, rv = B.bn_forward(x.reshape(N, C, H * W), scale, shift, running_mean, running_var, bn_memory, phase)
    best, mask = first_max(y.reshape(N, C, H, W), kh, kw)
    xn = (x + (-mean)[None, :, None, None]) / std[None, :, None, None]
    return np.tanh(best), np.take_along_axis(windows(xn, kh, kw), mask[..., None], axis=-1)[..., 0], mean, std, rm, rv


def backward(x, kernel, top, top_diff, scale, shift, save_mean, save_std):
    """-> bottom_diff, scale_diff, shift_diff: TanH's backward, the pooling's (the mask made again from BN's output, as
    the forward made it), BN's."""
    kh, kw = kernel
    N, C, H, W = x.shape
    xn = (x + (-save_mean)[None, :, None, None]) / save_std[None, :, None, None]
    y = xn * scale[None, :, None, None] + shift[None, :, None, None]
    _, mask = first_max(y, kh, kw)
    bn_diff = scatter(top_diff * (1 - top * top), mask, kh, kw).reshape(N, C, H * W)
    dx, dscale, dshift = B.bn_backward(x.reshape(N, C, H * W), bn_diff, scale, save_mean, save_std)
    return dx.reshape(N, C, H, W), dscale, dshift


def top_two_gap(y, kh, kw):
    """(N, C, PH, PW): each window's largest minus second largest BN output, over max(1, |largest|); inf for windows
    of one element."""
    w = np.sort(windows(y, kh, kw), axis=-1)
    if w.shape[-1] == 1:
        return np.full(w.shape[:-1], np.inf)
    return (w[..., -1] - w[..., -2]) / np.maximum(1.0, np.abs(w[..., -1]))


def bn_outputs64(inp):
    """BN's output in float64 on the inputs as given, (TRAIN, TEST)."""
    i = {k: v.astype(np.float64) for k, v in inp.items()}
    N, C, H, W = i["x"].shape
    return tuple(B.bn_forward(i["x"].reshape(N, C, H * W), i["scale"], i["shift"], i["running_mean"], i["running_var"],
                              BN_MEMORY, phase)[0].reshape(N, C, H, W) for phase in (TRAIN, TEST))


def close_windows(inp, kernel):
    """(N, C, PH, PW) bool: windows of a non-zero-scale channel whose top-two gap is below GAP in either phase."""
    bad = np.zeros(inp["top_diff"].shape, bool)
    for y in bn_outputs64(inp):
        bad |= top_two_gap(y, *kernel) < GAP
    return bad & (inp["scale"] != 0)[None, :, None, None]


def conditioned_inputs(shape, dtype, seed):
    """bn_pool_reference.conditioned_inputs with the scale of every odd channel negated (every shape with C >= 2 has a
    negative-scale channel) and, at ZERO_SCALE_SHAPE, the last channel's scale 0; then every window whose two largest
    BN outputs (float64 model, TRAIN or TEST) are closer than GAP*max(1, |y|) is drawn again, from the channel's own
    distribution, until none is left.  Read-only arrays."""
    N, C, H, W, kh, kw = shape
    out = {k: np.array(v) for k, v in P.conditioned_inputs(shape, dtype, seed).items()}
    out["scale"][1::2] *= -1
    if shape == ZERO_SCALE_SHAPE:
        out["scale"][-1] = 0
    r = np.random.default_rng(seed + 1234)
    for _ in range(100):
        bad = close_windows(out, (kh, kw))
        if not bad.any():
            break
        w = windows(out["x"], kh, kw)
        mu, sd = w.mean(axis=(0, 2, 3, 4)), w.std(axis=(0, 2, 3, 4))
        n, c, _, _ = np.nonzero(bad)
        w[bad] = (mu[c, None] + sd[c, None] * r.standard_normal((n.size, kh * kw))).astype(dtype)
        out["x"] = unwindows(w, kh, kw)
    else:
        raise AssertionError("windows with a top-two gap below %g remain at %r" % (GAP, shape))
    for v in out.values():
        v.setflags(write=False)
    return out


def _outputs(inp, kernel, dtype, fwd, bwd):
    i = {k: v.astype(dtype) if dtype is not None else v for k, v in inp.items()}
    out = {}
    for name, phase in (("train", TRAIN), ("test", TEST)):
        f = fwd(i["x"], kernel, i["scale"], i["shift"], i["running_mean"], i["running_var"], BN_MEMORY, phase)
        top, save_pool, mean, std = f[:4]
        b = bwd(i["x"], kernel, top, i["top_diff"], save_pool, i["scale"], i["shift"], mean, std)
        for k, v in zip(OUTPUTS, tuple(f) + tuple(b)):
            out[name + "_" + k] = v
    return out


def model_outputs(inp, kernel, dtype=None):
    """Every output the parity tests compare, from the inputs converted to `dtype` (default: as they are), by the
    three layers in sequence: TRAIN forward, TEST forward, and the backward after each."""
    return _outputs(inp, kernel, dtype, forward,
                    lambda x, k, top, td, sp, scale, shift, mean, std: backward(x, k, top, td, scale, shift, mean, std))


def bn_out(x, mean, std, scale, shift):
    """((x + (-mean)) / std)*scale + shift per channel of a 4-D array, every operation rounded once; -> (xn, y)."""
    c = (None, slice(None), None, None)
    xn = (x + (-mean)[c]) / std[c]
    return xn, xn * scale[c] + shift[c]


def extremum(x, kernel, scale):
    """(N, C, PH, PW): each window's largest x in channels of positive scale, its smallest in channels of negative
    scale (a strict scan in (h, w) order from the first element), its first element in channels of scale 0."""
    kh, kw = kernel
    w = windows(x, kh, kw)
    lo, hi = ((scale < 0)[None, :, None, None], (scale > 0)[None, :, None, None])
    e = w[..., 0].copy()
    for k in range(1, kh * kw):
        e = np.where(np.where(lo, w[..., k] < e, hi & (w[..., k] > e)), w[..., k], e)
    return e


def fused_forward(x, kernel, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY, phase=TRAIN):
    """The forward of include/mms_bn_maxpool.h in x's dtype, sums plainly sequential."""
    N, C, H, W = x.shape
    t = x.dtype.type
    if phase == TRAIN:
        mean, var = B.batch_statistics(x.reshape(N, C, H * W))
        keep, take = t(bn_memory), t(1) - t(bn_memory)
        rm, rv = take * mean + keep * running_mean, take * var + keep * running_var
    else:
        mean, var, rm, rv = running_mean.copy(), running_var.copy(), running_mean.copy(), running_var.copy()
    std = np.sqrt(var + t(VAR_EPS))
    save_pool, y = bn_out(extremum(x, kernel, scale), mean, std, scale, shift)
    return np.tanh(y), save_pool, mean, std, rm, rv


def fused_backward(x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std):
    """The backward of include/mms_bn_maxpool.h in x's dtype: its two sums run over the pooled tensor."""
    kh, kw = kernel
    N, C, H, W = x.shape
    t = x.dtype.type
    c = (None, slice(None), None, None)
    gp = top_diff * (1 - top * top)
    shift_diff = P._sequential(gp)
    scale_diff = P._sequential(gp * save_pool)
    a, b = scale * scale_diff, scale * shift_diff
    xn, y = bn_out(x, save_mean, save_std, scale, shift)
    _, mask = first_max(y, kh, kw)
    g = scatter(gp * scale[c], mask, kh, kw)
    dx = (g + t(-1.0 / (N * H * W)) * (xn * a[c] + b[c])) / save_std[c]
    return dx, scale_diff, shift_diff


def fused_outputs(inp, kernel, dtype=None):
    """model_outputs' keys by the fused algebra."""
    return _outputs(inp, kernel, dtype, fused_forward, fused_backward)
