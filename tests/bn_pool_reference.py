"""BN -> average pooling over windows that tile the map -> in-place TanH as numpy, generic over the dtype of its inputs:
the THREE reference layers in sequence (bn_reference.py; pooling_layer.cpp:197-212 / :291-317 restated for stride ==
kernel, no padding, so every pool_size is kh*kw; tanh_layer.cpp:13-33), not the fused algebra of csrc/bn_pool.hip.  x
and bottom_diff are (N, C, H, W); top, top_diff, save_pool are (N, C, H/kh, W/kw); everything else has C elements.

fused_outputs is the other thing here: the fused algebra of include/mms.h (mms_bn_pool_tanh_*) in the inputs' dtype
with plainly sequential sums -- bn_reference's: a map's elements one after another, then the N map sums one after
another -- which tests/test_bn_pool_reference.py holds against the float64 model to show that the inputs leave the
kernels room under the 1e-5 bar.  (ONE running sum over a whole channel is not what is meant: at (65, 5, 9, 37, 3, 37)
its 21645 float32 additions put 1.2e-6 on the mean, which every window's save_pool then carries with the same sign,
and scale_diff = sum gp*save_pool ends 2.1e-5 off.  No layer and no kernel here sums that way.)
"""
import numpy as np

import bn_reference as B

TRAIN, TEST, BN_MEMORY, VAR_EPS = B.TRAIN, B.TEST, B.BN_MEMORY, B.VAR_EPS

# (N, C, H, W, kh, kw) of the GPU parity tests (tests/test_gpu_bn_pool.py), the smallest at which each thing can go wrong
PARITY_SHAPES = [
    (1, 1, 1, 1, 1, 1),         # zero variance, identity pooling
    (2, 3, 4, 6, 2, 3),         # small, non-square window
    (7, 64, 5, 5, 5, 5),        # network_v4's second BN: one window per map, 100-byte runs
    (3, 2, 36, 36, 4, 4),       # its first BN: 16-byte window rows
    (65, 5, 9, 37, 3, 37),      # odd W, a window as wide as the map, a ragged wave; past the one-workgroup route
    (130, 3, 25, 41, 5, 1),     # kw = 1, several chunks
    (20, 3, 36, 36, 4, 4),      # the first BN's geometry on the two-launch route
    (4099, 2, 3, 3, 1, 3),      # many short runs, kh = 1
]
# Either side of the routing threshold of csrc/bn_pool.hip (BN's: 4096 16-byte groups of x per channel): the largest
# channel one workgroup takes and the next batch size up.  Their 2 x 4 windows are 16-byte rows whose size the kernels
# learn at run time (one access per row in float, two in double), which no shape above has.
THRESHOLD_SHAPES = {
    np.float32: ((128, 3, 8, 16, 2, 4), (129, 3, 8, 16, 2, 4)),      # 16384 and 16512 floats per channel
    np.float64: ((64, 3, 8, 16, 2, 4), (65, 3, 8, 16, 2, 4)),        # 8192 and 8320 doubles
}
TOP_DIFF_SEED_OFFSET = 77        # top_diff comes from its own generator: SEED + this


def pooled_shape(shape):
    N, C, H, W, kh, kw = shape
    return (N, C, H // kh, W // kw)


def ave_pool(a, kh, kw):
    """(N, C, H, W) -> (N, C, H/kh, W/kw): each window's elements added in (h, w) order, then / pool_size."""
    acc = np.zeros(a.shape[:2] + (a.shape[2] // kh, a.shape[3] // kw), a.dtype)
    for i in range(kh):
        for j in range(kw):
            acc = acc + a[:, :, i::kh, j::kw]
    return acc / a.dtype.type(kh * kw)


def ave_pool_backward(g, kh, kw):
    """(N, C, PH, PW) -> (N, C, H, W): every element of a window receives top_diff / pool_size."""
    return np.repeat(np.repeat(g / g.dtype.type(kh * kw), kh, axis=2), kw, axis=3)


def forward(x, kernel, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY, phase=TRAIN):
    """-> top, save_pool, save_mean, save_std, running_mean, running_var (the layers in sequence; save_pool is the
    pooling of BN's normalised map, which the layers never form on its own)."""
    kh, kw = kernel
    N, C, H, W = x.shape
    bn_top, mean, std, rm, rv = B.bn_forward(x.reshape(N, C, H * W), scale, shift, running_mean, running_var, bn_memory,
                                             phase)
    top = np.tanh(ave_pool(bn_top.reshape(N, C, H, W), kh, kw))
    xn = (x + (-mean)[None, :, None, None]) / std[None, :, None, None]
    return top, ave_pool(xn, kh, kw), mean, std, rm, rv


def backward(x, kernel, top, top_diff, scale, save_mean, save_std):
    """-> bottom_diff, scale_diff, shift_diff: TanH's backward, the pooling's, BN's."""
    kh, kw = kernel
    N, C, H, W = x.shape
    pooled_diff = top_diff * (1 - top * top)
    bn_diff = ave_pool_backward(pooled_diff, kh, kw).reshape(N, C, H * W)
    dx, dscale, dshift = B.bn_backward(x.reshape(N, C, H * W), bn_diff, scale, save_mean, save_std)
    return dx.reshape(N, C, H, W), dscale, dshift


def conditioned_inputs(shape, dtype, seed):
    """bn_reference.conditioned_inputs for the (N, C, H*W) blob, x reshaped to 4-D, plus top_diff ~ N(0, 1) of the
    pooled shape from its own seed.  Read-only arrays."""
    N, C, H, W, kh, kw = shape
    i = B.conditioned_inputs((N, C, H * W), dtype, seed)
    out = {k: i[k] for k in ("scale", "shift", "running_mean", "running_var")}
    out["x"] = i["x"].reshape(N, C, H, W)
    r = np.random.default_rng(seed + TOP_DIFF_SEED_OFFSET)
    out["top_diff"] = np.ascontiguousarray(r.standard_normal(pooled_shape(shape)).astype(dtype))
    for v in out.values():
        v.setflags(write=False)
    return out


OUTPUTS = ("top", "save_pool", "save_mean", "save_std", "running_mean", "running_var", "bottom_diff", "scale_diff",
           "shift_diff")


def _outputs(inp, kernel, dtype, fwd, bwd):
    i = {k: v.astype(dtype) if dtype is not None else v for k, v in inp.items()}
    out = {}
    for name, phase in (("train", TRAIN), ("test", TEST)):
        f = fwd(i["x"], kernel, i["scale"], i["shift"], i["running_mean"], i["running_var"], BN_MEMORY, phase)
        top, save_pool, mean, std = f[:4]
        b = bwd(i["x"], kernel, top, i["top_diff"], save_pool, i["scale"], mean, std)
        for k, v in zip(OUTPUTS, tuple(f) + tuple(b)):
            out[name + "_" + k] = v
    return out


def model_outputs(inp, kernel, dtype=None):
    """Every output the parity tests compare, from the inputs converted to `dtype` (default: as they are), by the
    three layers in sequence: TRAIN forward, TEST forward, and the backward after each."""
    return _outputs(inp, kernel, dtype, forward,
                    lambda x, k, top, td, save_pool, scale, mean, std: backward(x, k, top, td, scale, mean, std))


def _sequential(v):
    """(N, C, h, w) -> (C,): bn_reference's ordered sum -- each map's elements in ascending order, then the N map sums
    in ascending order, in v's dtype."""
    return B._ordered_sum(v.reshape(v.shape[0], v.shape[1], -1))


def fused_forward(x, kernel, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY, phase=TRAIN):
    """The forward of include/mms.h (mms_bn_pool_tanh_forward) in x's dtype, sums plainly sequential."""
    kh, kw = kernel
    N, C, H, W = x.shape
    t = x.dtype.type
    if phase == TRAIN:
        mean, var = B.batch_statistics(x.reshape(N, C, H * W))
        keep, take = t(bn_memory), t(1) - t(bn_memory)
        rm, rv = take * mean + keep * running_mean, take * var + keep * running_var
    else:
        mean, var, rm, rv = running_mean.copy(), running_var.copy(), running_mean.copy(), running_var.copy()
    std = np.sqrt(var + t(VAR_EPS))
    c = (None, slice(None), None, None)
    save_pool = (ave_pool(x, kh, kw) + (-mean)[c]) / std[c]
    top = np.tanh(save_pool * scale[c] + shift[c])
    return top, save_pool, mean, std, rm, rv


def fused_backward(x, kernel, top, top_diff, save_pool, scale, save_mean, save_std):
    """The backward of include/mms.h (mms_bn_pool_tanh_backward) in x's dtype: its two sums run over the pooled tensor."""
    kh, kw = kernel
    N, C, H, W = x.shape
    t = x.dtype.type
    c = (None, slice(None), None, None)
    gp = top_diff * (1 - top * top)
    shift_diff = _sequential(gp)
    scale_diff = _sequential(gp * save_pool)
    a, b = scale * scale_diff, scale * shift_diff
    xn = (x + (-save_mean)[c]) / save_std[c]
    g = np.repeat(np.repeat(gp / t(kh * kw) * scale[c], kh, axis=2), kw, axis=3)
    dx = (g + t(-1.0 / (N * H * W)) * (xn * a[c] + b[c])) / save_std[c]
    return dx, scale_diff, shift_diff


def fused_outputs(inp, kernel, dtype=None):
    """model_outputs' keys by the fused algebra."""
    return _outputs(inp, kernel, dtype, fused_forward, fused_backward)
