"""A numpy model of network_v4's classifier head (include/mms_head.h) -- Concat, InnerProduct, TanH, Dropout,
InnerProduct, SoftmaxWithLoss -- and its backward, written from the reference's layers:

  concat_layer.cpp:57-74            feat = [x0 | x1]
  inner_product_layer.cpp:84-97     z = bottom . weight^T + bias
  tanh_layer.cpp:11-36              h = tanh(z);  dz = dh * (1 - h * h)
  dropout_layer.cpp:14-18, 37-65    d = h * mask * scale in TRAIN, scale = 1 / (1 - ratio);  dh = dd * mask * scale
  softmax_layer.cpp:28-60           prob = exp(z - max) / sum
  softmax_loss_layer.cpp:59-149     loss = -sum log(max(prob[label], FLT_MIN)) / max(1, normalizer);
                                    dz2 = (prob - onehot) * loss_weight / max(1, normalizer), 0 for an ignored label

with the one rule the header adds: a label outside [0, C) is ignored.  Also here, for tests/test_head_reference.py,
tests/test_abi_head.py and tests/test_gpu_head.py: the shape lists, the input generators, the dyadic probes with their
int64 reference, and a reader of the fast route's named constants in csrc/head.hip.
"""
import collections
import functools

import numpy as np

from layer_plans import constants

TRAIN, TEST = 0, 1
FULL, VALID, BATCH_SIZE, NONE = 0, 1, 2, 3
FLT_MIN = float(np.finfo(np.float32).tiny)

K = constants("head.hip", ["kHeadTileSamples", "kHeadSingleSamples", "kHeadMaxSlabs", "kHeadMaxFeatures",
                           "kHeadMaxHidden", "kHeadMaxClasses", "kHeadHeaderBytes"])
TILE, SINGLE = K["kHeadTileSamples"], K["kHeadSingleSamples"]
MAX_F, MAX_H, MAX_C = K["kHeadMaxFeatures"], K["kHeadMaxHidden"], K["kHeadMaxClasses"]

S = collections.namedtuple("S", "N F0 F1 H C")
Cfg = collections.namedtuple("Cfg", "phase ratio norm ignore_label")
OUTPUTS_FWD = ("h", "prob", "loss")
OUTPUTS_BWD = ("x0_diff", "x1_diff", "w1_diff", "b1_diff", "w2_diff", "b2_diff")

V4 = S(50, 64, 2, 32, 2)                 # network_v4's training batch
V4_TEST = S(1517, 64, 2, 32, 2)          # ... and the test split
V4_2 = S(33, 32, 2, 64, 2)               # network_v4_2's head
# More than kHeadMaxSlabs tiles (N > 16384): several slabs of several tiles each, the plan no smaller batch takes.  F, H
# and C stay tiny but for one shape; (tiles, tiles per slab, slabs) beside each, tests/test_head_reference.py holds
# slabs() to them.  The table these came from needed no other N.
LARGE_PLANS = {
    S(16385, 3, 2, 5, 3): (257, 2, 129),                     # the fewest samples with two tiles per slab; the last slab
                                                             # has one tile of one sample
    S(16449, MAX_F - 2, 2, MAX_H, MAX_C): (258, 2, 129),     # at every fast limit: all accumulators of a thread carried
                                                             # over two tiles into slab partials; the last tile one sample
    S(32833, 1, 0, 1, 2): (514, 3, 172),                     # the last slab clipped to one of its three tiles; no x1
    S(65537, 2, 1, 3, 2): (1025, 5, 205),                    # 320 samples per slab: head_out_kernel's second trip
    S(16385, 4, 1, MAX_H + 1, 2): (257, 2, 129),             # past a fast limit: generic by route, not by request
}
LARGE_SHAPES = list(LARGE_PLANS)
INDEPENDENCE_SHAPE = LARGE_SHAPES[0]       # ... and its prefix of 16384 samples, cut with one tile per slab

# The (tiles per slab, slabs) the list covers, FAST_PLANS below: one slab of 1, 2 or 4 tiles up to SINGLE samples; 5, 8
# and 24 slabs of one tile from there to 16384 samples; (2, 129), (3, 172) and (5, 205) in LARGE_SHAPES.
FAST_PLANS = {(1, 1), (2, 1), (4, 1), (1, 5), (1, 8), (1, 24), (2, 129), (3, 172), (5, 205)}
FAST_SHAPES = [
    V4, V4_TEST, V4_2,                                                       # V4_TEST: 24 slabs of one tile
    S(1, 1, 0, 1, 1), S(1, 1, 0, 1, 2),                                      # minimal
    S(17, 5, 3, 31, 3), S(65, 63, 2, 33, 5), S(16, 64, 0, 32, 2),            # the seam inside a K step, ragged tiles
    S(TILE - 1, 6, 1, 8, 2), S(TILE, 6, 1, 8, 2), S(TILE + 1, 6, 1, 8, 2),   # around one tile of samples
    S(SINGLE - 1, 3, 2, 5, 3), S(SINGLE, 3, 2, 5, 3), S(SINGLE + 1, 3, 2, 5, 3),     # around the single-launch limit:
                                                                             # one slab of four tiles, five slabs of one
    S(3 * TILE + SINGLE + 7, 9, 2, 17, 4),                                   # eight slabs of one tile, the last with 7 samples
    S(20, MAX_F - 2, 2, MAX_H, MAX_C),                                       # at every limit
] + LARGE_SHAPES[:4]
GENERIC_SHAPES = [S(9, MAX_F, 1, 4, 2), S(9, 4, 1, MAX_H + 1, 2), S(9, 4, 1, 4, MAX_C + 1)     # just past each limit
                  ] + LARGE_SHAPES[4:]
GPU_SHAPES = FAST_SHAPES + GENERIC_SHAPES

# (cfg, ignored labels among the inputs?, out-of-range labels?)
CASES = [
    (Cfg(TRAIN, 0.5, VALID, None), False, False),
    (Cfg(TRAIN, 0.1, FULL, 1), True, False),
    (Cfg(TEST, 0.5, VALID, 0), True, True),
    (Cfg(TRAIN, 0.5, BATCH_SIZE, None), False, True),
    (Cfg(TEST, 0.5, NONE, None), False, False),
]


def sid(s):
    return "-".join(str(v) for v in s)


def slabs(N):
    """csrc/head.hip, head_slabs: (slabs, tiles per slab)."""
    tiles = (N + TILE - 1) // TILE
    if N <= SINGLE:
        return 1, tiles
    want = min(tiles, K["kHeadMaxSlabs"])
    tps = (tiles + want - 1) // want
    return (tiles + tps - 1) // tps, tps


def params(s):
    return s.H * (s.F0 + s.F1) + s.H + s.C * s.H + s.C


def workspace_bytes(s, itemsize):
    return 0 if s.N == 0 else K["kHeadHeaderBytes"] + slabs(s.N)[0] * params(s) * itemsize


# ---- inputs ----------------------------------------------------------------------------------------------------------
def labels(s, r, ignored, out_of_range, ignore_label):
    lab = r.integers(0, s.C, size=s.N).astype(np.float64)
    if ignored and ignore_label is not None:
        lab[r.random(s.N) < 0.25] = ignore_label
    if out_of_range:
        lab[r.random(s.N) < 0.15] = s.C
        lab[r.random(s.N) < 0.15] = -1
    return lab


def conditioned_inputs(s, dtype, seed, cfg=CASES[0][0], ignored=False, out_of_range=False):
    """x0 in tanh's range (it is pool1's TanH), x1 in [0, 1], Xavier-sized weights; everything rounded to `dtype`."""
    r = np.random.default_rng(seed + 7919 * s.N + 31 * s.F0 + s.H)
    F = s.F0 + s.F1
    inp = dict(
        x0=r.uniform(-1, 1, (s.N, s.F0)), x1=r.uniform(0, 1, (s.N, s.F1)) if s.F1 else None,
        w1=r.uniform(-1, 1, (s.H, F)) * np.sqrt(3.0 / F), b1=r.uniform(-0.2, 0.2, s.H),
        w2=r.uniform(-1, 1, (s.C, s.H)) * np.sqrt(6.0 / s.H), b2=r.uniform(-0.2, 0.2, s.C),
        w1_diff0=r.uniform(-0.1, 0.1, (s.H, F)), b1_diff0=r.uniform(-0.1, 0.1, s.H),
        w2_diff0=r.uniform(-0.1, 0.1, (s.C, s.H)), b2_diff0=r.uniform(-0.1, 0.1, s.C))
    inp = {k: (None if v is None else v.astype(dtype)) for k, v in inp.items()}
    inp["mask"] = (r.random((s.N, s.H)) >= cfg.ratio).astype(np.int32)
    inp["label"] = labels(s, r, ignored, out_of_range, cfg.ignore_label).astype(dtype)
    inp["loss_weight"] = 1.0
    return inp


# ---- the model -------------------------------------------------------------------------------------------------------
def feat_of(inp, t):
    x0 = inp["x0"].astype(t)
    return x0 if inp["x1"] is None else np.concatenate([x0, inp["x1"].astype(t)], axis=1)


def valid_of(label, C, cfg):
    lv = np.trunc(np.asarray(label, dtype=np.float64)).astype(np.int64)        # static_cast<int>
    ok = (lv >= 0) & (lv < C)
    if cfg.ignore_label is not None:
        ok &= lv != cfg.ignore_label
    return np.where(ok, lv, 0), ok


def normalizer(cfg, N, count):
    n = {FULL: N, VALID: count, BATCH_SIZE: N, NONE: 1}[cfg.norm]
    return max(1, n)


def scale_of(cfg, t):
    return t(1.0 / (1.0 - float(np.float32(cfg.ratio))))      # threshold_ is a float, scale_ = Dtype(1. / (1. - threshold_))


def dropout(v, mask, cfg, t):
    return (v * mask.astype(t)) * scale_of(cfg, t) if cfg.phase == TRAIN else v


SLAB_ORDER = "slabs"         # for `reverse`: the order csrc/head.hip adds a slab's samples and then the slabs in


def slab_sum(v, t):
    """The sum over samples (axis 0) one term at a time in `t`: ascending within a slab of slabs(N), each slab from 0,
    then the slabs' partial sums ascending from slab 0's -- head_param_kernel and head_param_finish_kernel."""
    n_slabs, tps = slabs(len(v))
    per = tps * TILE
    pad = np.zeros((n_slabs * per,) + v.shape[1:], dtype=t)           # + 0 after the last sample changes no sum
    pad[:len(v)] = v
    part = np.add.accumulate(pad.reshape((n_slabs, per) + v.shape[1:]), axis=1, dtype=t)[:, -1]
    return np.add.accumulate(part, axis=0, dtype=t)[-1]


def slab_products(a, b, t):
    """a^T b, the sum over samples of the outer products: each slab's product on its own (the order within a slab is the
    matrix product's), then the slabs' partial sums one at a time, ascending, in `t`."""
    n_slabs, tps = slabs(len(a))
    per = tps * TILE
    pa, pb = np.zeros((n_slabs * per, a.shape[1]), dtype=t), np.zeros((n_slabs * per, b.shape[1]), dtype=t)
    pa[:len(a)], pb[:len(b)] = a, b
    part = np.matmul(pa.reshape(n_slabs, per, -1).transpose(0, 2, 1), pb.reshape(n_slabs, per, -1))
    assert part.dtype == t
    return np.add.accumulate(part, axis=0, dtype=t)[-1]


def nsum(v, t, reverse):
    """The sum over samples (axis 0), in `t`; reversed: the samples taken last to first; SLAB_ORDER: slab_sum."""
    if reverse == SLAB_ORDER:
        return slab_sum(v.astype(t), t)
    return np.add.reduce(v[::-1] if reverse else v, axis=0, dtype=t)


def forward(s, cfg, inp, dtype=np.float64, reverse=False):
    """-> {"h", "prob"[, "loss"]}; the loss (1,) only with a label."""
    t = np.dtype(dtype).type
    feat = feat_of(inp, t)
    z1 = feat @ inp["w1"].astype(t).T
    if inp["b1"] is not None:
        z1 = z1 + inp["b1"].astype(t)
    h = np.tanh(z1)
    d = dropout(h, inp["mask"], cfg, t) if cfg.phase == TRAIN else h
    z2 = d @ inp["w2"].astype(t).T
    if inp["b2"] is not None:
        z2 = z2 + inp["b2"].astype(t)
    e = np.exp(z2 - z2.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True, dtype=t)
    out = dict(h=h, prob=prob)
    if inp.get("label") is not None:
        lv, ok = valid_of(inp["label"], s.C, cfg)
        terms = -np.log(np.maximum(prob[np.arange(s.N), lv], t(FLT_MIN)))
        total = nsum(np.where(ok, terms, t(0)), t, reverse)
        out["loss"] = np.array([total / t(normalizer(cfg, s.N, int(ok.sum())))], dtype=t)
    assert all(v.dtype == t for v in out.values())
    return out


def backward(s, cfg, inp, h, prob, dtype=np.float64, reverse=False):
    """The six diffs from the saved h and prob; the parameter diffs on top of inp[*_diff0]."""
    t = np.dtype(dtype).type
    h, prob = h.astype(t), prob.astype(t)
    feat = feat_of(inp, t)
    w1, w2 = inp["w1"].astype(t), inp["w2"].astype(t)
    lv, ok = valid_of(inp["label"], s.C, cfg)
    coef = t(inp["loss_weight"]) / t(normalizer(cfg, s.N, int(ok.sum())))
    onehot = np.zeros((s.N, s.C), dtype=t)
    onehot[np.arange(s.N), lv] = 1
    dz2 = np.where(ok[:, None], (prob - onehot) * coef, t(0))
    d = dropout(h, inp["mask"], cfg, t) if cfg.phase == TRAIN else h
    dh = dropout(dz2 @ w2, inp["mask"], cfg, t) if cfg.phase == TRAIN else dz2 @ w2
    dz1 = dh * (t(1) - h * h)
    order = slice(None, None, -1) if reverse is True else slice(None)
    tn = slab_products if reverse == SLAB_ORDER else (lambda a, b, t_: a[order].T @ b[order])
    dx = dz1 @ w1
    out = dict(x0_diff=dx[:, :s.F0],
               w1_diff=inp["w1_diff0"].astype(t) + tn(dz1, feat, t),
               b1_diff=inp["b1_diff0"].astype(t) + nsum(dz1, t, reverse),
               w2_diff=inp["w2_diff0"].astype(t) + tn(dz2, d, t),
               b2_diff=inp["b2_diff0"].astype(t) + nsum(dz2, t, reverse))
    if s.F1:
        out["x1_diff"] = dx[:, s.F0:]
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    assert all(v.dtype == t for v in out.values())
    return out


def model_outputs(s, cfg, inp, dtype=np.float64, reverse=False):
    """Forward, then backward from the forward's own h and prob."""
    out = forward(s, cfg, inp, dtype, reverse)
    out.update(backward(s, cfg, inp, out["h"], out["prob"], dtype, reverse))
    return out


# ---- dyadic probes for the backward ------------------------------------------------------------------------------------
PROBE_RATIO = 0.5            # scale 2
PROBE_LOSS_WEIGHT = 2.0


def probe_cfg(s, k=0):
    """TRAIN, ratio 0.5; normalization NONE unless N is a power of two (then FULL / BATCH_SIZE by turns, whose
    normalizer is N whatever is ignored)."""
    pow2 = s.N & (s.N - 1) == 0
    return Cfg(TRAIN, PROBE_RATIO, (FULL, BATCH_SIZE)[k % 2] if pow2 else NONE, 1 if s.C > 1 else None)


def imatmul(a, b):
    """a @ b of integer arrays as int64, through float64's matrix product: exact in any order, the largest sum of
    absolute products being below 2^53."""
    fa, fb = a.astype(np.float64), b.astype(np.float64)
    assert (np.abs(fa) @ np.abs(fb)).max(initial=0.0) < 2.0 ** 53
    return (fa @ fb).astype(np.int64)


def dyadic_probe(s, seed, k=0):
    """(cfg, inputs, saved h, saved prob, int64 reference, bound).  h in multiples of 1/4, prob rows from {0, 1/4, 3/4, 1},
    small-integer x, w1, w2 and initial diffs, loss_weight 2, some labels ignored and some out of range.  The reference
    is computed in int64 in units of 1 / (64 normalizer); `bound` is the largest sum of absolute terms of any output in
    those units: below 2^24, every partial sum in any order is an exactly representable float."""
    cfg = probe_cfg(s, k)
    r = np.random.default_rng(seed + 104729 * s.N + 17 * s.F0 + s.H + k)
    F = s.F0 + s.F1
    x = r.integers(-2, 3, (s.N, F))
    w1, w2 = r.integers(-2, 3, (s.H, F)), r.integers(-2, 3, (s.C, s.H))
    mask = r.integers(0, 2, (s.N, s.H))
    h4 = r.integers(-4, 5, (s.N, s.H))
    p4 = np.zeros((s.N, s.C), dtype=np.int64)
    one = (r.random(s.N) < 0.3) | (s.C == 1)                         # a row of one 1; else 3/4 and 1/4 in two classes
    a = r.integers(0, s.C, s.N)
    b = (a + r.integers(1, max(2, s.C), s.N)) % s.C
    p4[np.arange(s.N), a] = np.where(one, 4, 3)
    p4[np.arange(s.N)[~one], b[~one]] = 1
    lab = labels(s, r, True, True, cfg.ignore_label)
    diff0 = dict(w1_diff0=r.integers(-3, 4, (s.H, F)), b1_diff0=r.integers(-3, 4, s.H),
                 w2_diff0=r.integers(-3, 4, (s.C, s.H)), b2_diff0=r.integers(-3, 4, s.C))
    lv, ok = valid_of(lab, s.C, cfg)
    norm = normalizer(cfg, s.N, int(ok.sum()))
    assert norm & (norm - 1) == 0
    unit = 64 * norm
    lw = int(PROBE_LOSS_WEIGHT)
    onehot = np.zeros((s.N, s.C), dtype=np.int64)
    onehot[np.arange(s.N), lv] = 4
    dz2 = np.where(ok[:, None], (p4 - onehot) * lw, 0)               # units of 1 / (4 norm)
    d4 = h4 * mask * 2                                               # units of 1 / 4
    dz1 = imatmul(dz2, w2) * mask * 2 * (16 - h4 * h4)                     # units of 1 / (64 norm)
    ref = dict(x_diff=imatmul(dz1, w1), w1_diff=diff0["w1_diff0"] * unit + imatmul(dz1.T, x), b1_diff=diff0["b1_diff0"] * unit + dz1.sum(0),
               w2_diff=diff0["w2_diff0"] * unit + 4 * imatmul(dz2.T, d4), b2_diff=diff0["b2_diff0"] * unit + 16 * dz2.sum(0))
    a1, a2 = np.abs(dz1), np.abs(dz2)
    bound = max(int(imatmul(a1, np.abs(w1)).max()), int((3 * unit + imatmul(a1.T, np.abs(x))).max()), int((3 * unit + a1.sum(0)).max()),
                int((3 * unit + 4 * imatmul(a2.T, np.abs(d4))).max()), int((3 * unit + 16 * a2.sum(0)).max()),
                int(16 * imatmul(a2, np.abs(w2)).max() * 2 * 16))
    want = {k_: v.astype(np.float64) / unit for k_, v in ref.items()}
    want["x0_diff"] = np.ascontiguousarray(want["x_diff"][:, :s.F0])
    if s.F1:
        want["x1_diff"] = np.ascontiguousarray(want["x_diff"][:, s.F0:])
    del want["x_diff"]
    inp = dict(x0=x[:, :s.F0].astype(np.float64), x1=x[:, s.F0:].astype(np.float64) if s.F1 else None,
               w1=w1.astype(np.float64), w2=w2.astype(np.float64), b1=None, b2=None, mask=mask.astype(np.int32),
               label=lab, loss_weight=PROBE_LOSS_WEIGHT)
    inp.update({k_: v.astype(np.float64) for k_, v in diff0.items()})
    return cfg, inp, h4 / 4.0, p4 / 4.0, want, bound


@functools.lru_cache(maxsize=None)
def shared_probe(s, seed, k=0):
    """dyadic_probe(s, seed, k), made once for all the tests that take it, its arrays read-only."""
    probe = dyadic_probe(s, seed, k)
    cfg, inp, h, prob, want, bound = probe
    for v in list(inp.values()) + [h, prob] + list(want.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return probe
