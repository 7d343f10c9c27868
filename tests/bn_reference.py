"""The fork's BN layer (bn_layer.cpp, the `#if 1` backward) as numpy, generic over the dtype of its inputs: a model
written from the formulas, every intermediate rounded to the dtype, every sum in ascending index order (s inside n: a
run's S elements first, then the N run sums).  x, top, dy, dx are (N, C, S); everything else has C elements.

    TRAIN  m_nc = (1/S) sum_s x;  mean = (1/N) sum_n m_nc;  q_nc = (1/S) sum_s x*x;  ex2 = (1/N) sum_n q_nc
           var = ex2 - mean*mean;  running = (1 - bn_memory)*batch + bn_memory*running  (two products, then the add)
    TEST   mean, var = the running blobs, which stay as they are
    std = sqrt(var + 1e-9);  xn = (x + (-mean)) / std;  top = xn*scale + shift
    backward  scale_diff = sum xn*dy;  shift_diff = sum dy;  g = dy*scale;  a = sum xn*g;  b = sum g
              dx = (g + (-1/(N S)) * (xn*a + b)) / std
"""
import numpy as np

# (N, C, S) of the GPU parity tests (tests/test_gpu_bn.py), the smallest at which each thing can go wrong
PARITY_SHAPES = [
    (1, 1, 1),          # zero variance: top == shift and dx == 0 exactly
    (2, 3, 5),          # small general case
    (7, 64, 25),        # network_v4's second BN: 100-byte runs, one access per element
    (3, 2, 1296),       # its first BN's runs: 16-byte accesses
    (65, 5, 333),       # odd S, a ragged wave; past the one-workgroup route
    (4099, 2, 9),       # many short runs
    (130, 3, 1025),     # long runs with a ragged tail, several chunks
    (20, 3, 1296),      # the first BN's runs past the one-workgroup route: 16-byte accesses in both of its launches
]
# Either side of the routing threshold of csrc/bn.hip (4096 16-byte groups per channel): the largest channel that one
# workgroup takes, and one element more -- 4097 groups, the last of them a single element, in three chunks.
THRESHOLD_SHAPES = {
    np.float32: ((128, 3, 128), (113, 3, 145)),      # 16384 and 16385 floats per channel
    np.float64: ((64, 3, 128), (2731, 3, 3)),        # 8192 and 8193 doubles
}

TRAIN, TEST = 0, 1
VAR_EPS = 1e-9
BN_MEMORY = 0.9


def _ordered_sum(v):
    """(N, C, S) -> (C,): ascending s inside each run, then ascending n, in v's dtype."""
    runs = np.cumsum(v, axis=2, dtype=v.dtype)[:, :, -1]
    return np.cumsum(runs, axis=0, dtype=v.dtype)[-1]


def _scaled_mean(v):
    """(1/N) sum_n ((1/S) sum_s v): the two gemv's, alpha applied to each finished sum."""
    N, _, S = v.shape
    t = v.dtype.type
    runs = t(1.0 / S) * np.cumsum(v, axis=2, dtype=v.dtype)[:, :, -1]
    return t(1.0 / N) * np.cumsum(runs, axis=0, dtype=v.dtype)[-1]


def batch_statistics(x):
    """-> mean, var of each channel as TRAIN computes them (var = E[x^2] - E[x]^2, not clamped)."""
    mean = _scaled_mean(x)
    return mean, _scaled_mean(x * x) - mean * mean


def bn_forward(x, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY, phase=TRAIN):
    """-> top, save_mean, save_std, running_mean, running_var (the last two new arrays; the inputs are not written)."""
    t = x.dtype.type
    if phase == TRAIN:
        mean, var = batch_statistics(x)
        keep, take = t(bn_memory), t(1) - t(bn_memory)
        new_mean = take * mean + keep * running_mean
        new_var = take * var + keep * running_var
    else:
        mean, var = running_mean.copy(), running_var.copy()
        new_mean, new_var = running_mean.copy(), running_var.copy()
    std = np.sqrt(var + t(VAR_EPS))
    xn = (x + (-mean)[None, :, None]) / std[None, :, None]
    top = xn * scale[None, :, None] + shift[None, :, None]
    return top, mean, std, new_mean, new_var


def bn_backward(x, dy, scale, save_mean, save_std):
    """-> dx, scale_diff, shift_diff, from the mean and std the last forward saved."""
    N, _, S = x.shape
    t = x.dtype.type
    xn = (x + (-save_mean)[None, :, None]) / save_std[None, :, None]
    scale_diff = _ordered_sum(xn * dy)
    shift_diff = _ordered_sum(dy)
    g = dy * scale[None, :, None]
    a = _ordered_sum(xn * g)
    b = _ordered_sum(g)
    dx = (g + t(-1.0 / (N * S)) * (xn * a[None, :, None] + b[None, :, None])) / save_std[None, :, None]
    return dx, scale_diff, shift_diff


def conditioned_inputs(shape, dtype, seed):
    """The parity inputs: per channel a standard deviation from [0.5, 1.5] and a mean 0.5 N(0, 1), so that
    E[x^2] - E[x]^2 loses little (a mean of 3 sigma would triple the float32 error of var)."""
    N, C, S = shape
    r = np.random.default_rng(seed)
    sd = r.uniform(0.5, 1.5, C)
    mu = 0.5 * r.standard_normal(C)
    out = dict(
        x=mu[None, :, None] + sd[None, :, None] * r.standard_normal(shape),
        dy=r.standard_normal(shape),
        scale=r.uniform(0.5, 1.5, C),
        shift=0.5 * r.standard_normal(C),
        running_mean=0.5 * r.standard_normal(C),
        running_var=r.uniform(0.5, 1.5, C))
    out = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def model_outputs(inp, dtype=None):
    """Every output the parity tests compare, from the inputs converted to `dtype` (default: as they are): TRAIN
    forward, TEST forward, and backward after each."""
    i = {k: v.astype(dtype) if dtype is not None else v for k, v in inp.items()}
    out = {}
    for name, phase in (("train", TRAIN), ("test", TEST)):
        top, mean, std, rm, rv = bn_forward(i["x"], i["scale"], i["shift"], i["running_mean"], i["running_var"],
                                            BN_MEMORY, phase)
        dx, dscale, dshift = bn_backward(i["x"], i["dy"], i["scale"], mean, std)
        out.update({name + "_top": top, name + "_save_mean": mean, name + "_save_std": std,
                    name + "_running_mean": rm, name + "_running_var": rv, name + "_bottom_diff": dx,
                    name + "_scale_diff": dscale, name + "_shift_diff": dshift})
    return out
