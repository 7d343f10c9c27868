"""What the suites of the tail's fused backward (include/mms_train_tail_backward.h) share: the shape lists, the closed
forms of the fused route in float64 (the header's algebra, spelt out in numpy) and the exact probe, whose inputs are
given to the backward directly."""
import numpy as np

import head_reference as HR
import train_tail_reference as R

AVE, MAX = R.AVE, R.MAX


def v3(N):
    """network_v3's tail: 64 x 9 x 9 -> 64 x 5 x 5 under a 5 x 5 window (MAX in the net), 64 hidden units."""
    return R.T(N, 64, 9, 9, 64, 5, 5, (5, 5), 2, 64, 2)


def large_image(N):
    """A 12 x 12 input, 144 pixels in one workgroup of the bottom_diff launch: reached, past the measured class."""
    return R.T(N, 3, 12, 12, 5, 3, 3, (10, 10), 3, 5, 2)


def k17(N):
    """17 output channels: past one 16-row tile of the parameter diffs and of the product's operand."""
    return R.T(N, 3, 6, 6, 17, 3, 3, (4, 4), 3, 5, 2)


def no_overlap(N):
    return R.T(N, 3, 6, 6, 5, 3, 3, (4, 4), 0, 5, 2)


BATCHES = (1, 3, 50, 65, 256)
# every batch at the small tail; the nets' tails at 3 and 50, v4's at 65 and v5's at 256 too; v5's K = 32 is cut into two
# chunks of input channels by the bottom_diff plan (tests/test_abi_train_tail_backward.py reads that from the plan itself)
TWO_CHUNKS = R.v5(3)
PARITY_TAILS = ([R.small(N) for N in BATCHES] + [R.v4(3), R.v4(50), R.v4(65), v3(3), TWO_CHUNKS, R.v5(50), R.v5(256),
                                                  k17(3), k17(65), no_overlap(3), no_overlap(65), large_image(3)])
PAST_N = R.small(257)                      # one image past the coefficients' chain: not reached


def closed_forms(t, pool, y, flt, x0_diff, save_pool, save_mean, save_std, scale, shift):
    """dy (N, K, OH, OW), scale_diff, shift_diff by the header's closed forms, in the dtype of the inputs."""
    N, K, OH, OW = y.shape
    S, M = OH * OW, N * OH * OW
    g = x0_diff * (1 - flt * flt)
    shift_diff = g.sum(axis=0)
    scale_diff = (g * save_pool).sum(axis=0)
    cs = scale / save_std
    B = -(cs * scale_diff / M) / save_std
    A0 = -(cs * shift_diff / M) - B * save_mean
    dy = A0[None, :, None, None] + B[None, :, None, None] * y
    if pool == AVE:
        dy = dy + (g / S * cs)[:, :, None, None]
    else:
        bn = (y - save_mean[None, :, None, None]) / save_std[None, :, None, None] * scale[None, :, None, None] \
            + shift[None, :, None, None]
        first = bn.reshape(N, K, S).argmax(axis=2)                # numpy's argmax is the first maximum
        delta = np.zeros((N, K, S), dtype=y.dtype)
        np.put_along_axis(delta, first[:, :, None], (g * cs)[:, :, None], axis=2)
        dy = dy + delta.reshape(N, K, OH, OW)
    return dy, scale_diff, shift_diff


def pooled(pool, y, scale, save_std, save_mean=None):
    """save_pool (N, K) of y in y's dtype: the window's mean (AVE) or its extremum in the direction of the channel's
    scale (MAX), normalised."""
    N, K = y.shape[:2]
    flat = y.reshape(N, K, -1)
    if pool == AVE:
        p = flat.sum(axis=2) / y.dtype.type(flat.shape[2])
    else:
        p = np.where(np.asarray(scale)[None, :] < 0, flat.min(axis=2), flat.max(axis=2))
    if save_mean is not None:
        p = p - save_mean[None, :]
    return (p / save_std[None, :]).astype(y.dtype)


PROBE = R.T(4, 2, 6, 6, 3, 3, 3, (4, 4), 2, 4, 2)     # a 4 x 4 map: N S = 64


def exact_probe(pool, seed=7):
    """-> (inp, fwd): the backward's inputs given directly.  flt = 0, h = 0, save_mean = 0, save_std = 2, |scale| a
    power of two (one channel negative), prob, the weights, x and y small dyadic values, every label valid (the
    normalizer is N = 4), dropout_ratio 0.5: every product and every partial sum of the backward is exact in float32."""
    t, r = PROBE, np.random.default_rng(seed)
    s = t.stage.conv
    N, K, F1, H, C = s.N, s.K, t.F1, t.H, t.C
    OH, OW = R.S.CR.output_dims(s)
    f = np.float32
    dy = lambda shape, lo, hi, q: (r.integers(lo, hi + 1, shape) / q).astype(f)       # noqa: E731
    x = dy((N, s.C, s.H, s.W), -2, 2, 1)
    y = np.empty((N, K, OH, OW), f)
    for n in range(N):                                   # distinct values in every window: MAX has no ties here
        for k in range(K):
            y[n, k] = (r.permutation(OH * OW).reshape(OH, OW) - 8).astype(f)
    scale = np.array([1.0, -0.5, 2.0], f)
    shift = np.array([0.5, -1.0, 0.0], f)
    save_mean, save_std = np.zeros(K, f), np.full(K, 2.0, f)
    save_pool = pooled(pool, y, scale, save_std)
    label = r.integers(0, C, N).astype(f)
    p0 = r.choice([0.25, 0.5, 0.75], N).astype(f)
    prob = np.stack([p0, 1 - p0], axis=1).astype(f)
    inp = dict(x=x, weight=dy((K, s.C, s.kh, s.kw), -2, 2, 2), bias=np.zeros(K, f), scale=scale, shift=shift,
               overlap=dy((N, F1), -2, 2, 2), w1=dy((H, K + F1), -2, 2, 2), b1=np.zeros(H, f), w2=dy((C, H), -2, 2, 2),
               b2=np.zeros(C, f), mask=r.integers(0, 2, (N, H)).astype(np.int32), label=label, loss_weight=1.0,
               weight_diff0=dy((K, s.C, s.kh, s.kw), -2, 2, 2), bias_diff0=dy((K,), -2, 2, 2),
               w1_diff0=dy((H, K + F1), -2, 2, 2), b1_diff0=dy((H,), -2, 2, 2), w2_diff0=dy((C, H), -2, 2, 2),
               b2_diff0=dy((C,), -2, 2, 2))
    fwd = dict(y=y, flt=np.zeros((N, K), f), save_pool=save_pool, save_mean=save_mean, save_std=save_std,
               h=np.zeros((N, H), f), prob=prob)
    return inp, fwd


def probe_config():
    return R.cfg(HR.VALID, None, 0.5)
