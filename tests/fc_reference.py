"""Numpy restatements of the four layers of include/mms_fc.h, written from the reference's CPU loops:

  inner_product_layer.cpp:84-141    top = x . w^T + b;  w_diff += top_diff^T . x;  b_diff += sum_m top_diff;
                                    bottom_diff = top_diff . w   (`transpose`: w is (K, N_out))
  softmax_layer.cpp:28-90           per (o, k): e = exp(x - max); top = e / sum;  bottom_diff = (top_diff - dot) * top
  softmax_loss_layer.cpp:59-149     loss = -sum log(max(prob[label], FLT_MIN)) / max(1, normalizer);
                                    bottom_diff = (prob - onehot) * (loss_weight / max(1, normalizer)), 0 where ignored
  concat_layer.cpp:57-96            top = the bottoms side by side along the axis;  the diffs are top_diff's slices

with the one rule the header adds: a label outside [0, channels) is ignored.  Also here, for the three test files of
the family: the plan constants of csrc/fc_plans.h restated (slabs, route, kernel of a product), and the input makers.
"""
import numpy as np

from layer_plans import constants

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
ROUTE_NONE, ROUTE_GENERIC, ROUTE_FAST = -1, 0, 1
FORWARD, BACKWARD = 0, 1
FULL, VALID, BATCH_SIZE, NONE = 0, 1, 2, 3
FLT_MIN = float(np.finfo(np.float32).tiny)
MAX_BOTTOMS = 8

K = constants("fc_plans.h", ["kFcSlabRows", "kFcMaxSlabs", "kFcFastMinMacs", "kFcFastFwdMinK", "kFcNarrowMax", "kSoftmaxThreadRowMax",
                             "kLossSlabMin", "kLossMaxSlabs"])


# ---- the plan, restated ----------------------------------------------------------------------------------------------
def slab_rows(M):
    per = -(-M // K["kFcMaxSlabs"])
    return max(K["kFcSlabRows"], -(-per // 32) * 32)


def slabs(M):
    return -(-M // slab_rows(M))


def ip_workspace_bytes(M, Kdim, N, itemsize):
    return 0 if M == 0 else slabs(M) * (Kdim * N + N) * itemsize


def ip_route(M, Kdim, N, pass_):
    if M * Kdim * N < K["kFcFastMinMacs"]:
        return ROUTE_GENERIC
    narrow = M <= K["kFcNarrowMax"] or N <= K["kFcNarrowMax"]
    fast = (narrow or Kdim >= K["kFcFastFwdMinK"]) if pass_ == FORWARD else slabs(M) > 1
    return ROUTE_FAST if fast else ROUTE_GENERIC


def loss_slab_len(P):
    return max(K["kLossSlabMin"], -(-P // K["kLossMaxSlabs"]))


def loss_workspace_bytes(P, itemsize):
    if P == 0:
        return 0
    s = -(-P // loss_slab_len(P))
    return (s + 1) * itemsize + 4 * s


# ---- InnerProduct ----------------------------------------------------------------------------------------------------
def ip_forward(x, w, b=None, transpose=False, dtype=np.float64):
    t = np.dtype(dtype).type
    x, w = x.astype(t), w.astype(t)
    top = x @ (w if transpose else w.T)
    if b is not None:
        top = top + b.astype(t)
    return np.ascontiguousarray(top)


def ip_backward(x, w, top_diff, transpose=False, w_diff0=None, b_diff0=None, dtype=np.float64):
    """-> (w_diff, b_diff, bottom_diff); the parameter diffs on top of w_diff0 / b_diff0 (zeros when None)."""
    t = np.dtype(dtype).type
    x, w, td = x.astype(t), w.astype(t), top_diff.astype(t)
    dw = x.T @ td if transpose else td.T @ x
    db = np.add.reduce(td, axis=0, dtype=t)
    if w_diff0 is not None:
        dw = w_diff0.astype(t) + dw
    if b_diff0 is not None:
        db = b_diff0.astype(t) + db
    dx = td @ (w.T if transpose else w)
    return np.ascontiguousarray(dw), np.ascontiguousarray(db), np.ascontiguousarray(dx)


def ip_exact(x, w, b, td, transpose, w_diff0, b_diff0):
    """The same four results of integer arrays in int64: (top, w_diff, b_diff, bottom_diff)."""
    x, w, td = (a.astype(np.int64) for a in (x, w, td))
    top = x @ (w if transpose else w.T)
    if b is not None:
        top = top + b.astype(np.int64)
    dw = w_diff0.astype(np.int64) + (x.T @ td if transpose else td.T @ x)
    db = b_diff0.astype(np.int64) + td.sum(axis=0)
    return top, dw, db, td @ (w.T if transpose else w)


# ---- Softmax ---------------------------------------------------------------------------------------------------------
def softmax_forward(x, dtype=np.float64):
    """x (outer, channels, inner)"""
    t = np.dtype(dtype).type
    x = x.astype(t)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    s = np.zeros((x.shape[0], 1, x.shape[2]), dtype=t)
    for c in range(x.shape[1]):                                    # ascending, every add rounded in t
        s[:, 0, :] += e[:, c, :]
    return e / s


def softmax_backward(top, top_diff, dtype=np.float64):
    t = np.dtype(dtype).type
    top, td = top.astype(t), top_diff.astype(t)
    dot = np.zeros((top.shape[0], 1, top.shape[2]), dtype=t)
    for c in range(top.shape[1]):
        dot[:, 0, :] += td[:, c, :] * top[:, c, :]
    return (td - dot) * top


# ---- SoftmaxWithLoss -------------------------------------------------------------------------------------------------
def valid_of(label, channels, ignore_label):
    """(labels with 0 where not valid, validity), both (outer, inner)"""
    lv = np.trunc(np.asarray(label, dtype=np.float64)).astype(np.int64)          # static_cast<int>
    ok = (lv >= 0) & (lv < channels)
    if ignore_label is not None:
        ok &= lv != ignore_label
    return np.where(ok, lv, 0), ok


def normalizer(norm, outer, inner, count):
    return max(1, {FULL: outer * inner, VALID: count, BATCH_SIZE: outer, NONE: 1}[norm])


def loss_forward(x, label, norm=VALID, ignore_label=None, dtype=np.float64, slab_len=None):
    """-> (prob, loss (1,)).  x (outer, channels, inner), label (outer, inner).  slab_len: the positions are summed in
    slabs of that length and the slabs then added in ascending order (the library's order); None: one chain, the
    reference's."""
    t = np.dtype(dtype).type
    prob = softmax_forward(x, dtype)
    O, C, I = prob.shape
    lv, ok = valid_of(np.asarray(label).reshape(O, I), C, ignore_label)
    picked = np.take_along_axis(prob, lv[:, None, :], axis=1)[:, 0, :]
    logs = np.log(np.maximum(picked, t(FLT_MIN))).astype(t).ravel()
    okf = ok.ravel()
    P = O * I
    step = slab_len or max(P, 1)
    parts = []
    for p0 in range(0, P, step):
        acc = t(0)
        for p in range(p0, min(P, p0 + step)):
            if okf[p]:
                acc = t(acc - logs[p])
        parts.append(acc)
    total = parts[0] if parts else t(0)
    for v in parts[1:]:
        total = t(total + v)
    return prob, np.array([total / t(normalizer(norm, O, I, int(ok.sum())))], dtype=t)


def loss_backward(prob, label, loss_weight=1.0, norm=VALID, ignore_label=None, dtype=np.float64):
    t = np.dtype(dtype).type
    prob = prob.astype(t)
    O, C, I = prob.shape
    lv, ok = valid_of(np.asarray(label).reshape(O, I), C, ignore_label)
    onehot = np.zeros_like(prob)
    np.put_along_axis(onehot, lv[:, None, :], t(1), axis=1)
    scale = t(t(loss_weight) / t(normalizer(norm, O, I, int(ok.sum()))))
    return np.where(ok[:, None, :], prob - onehot, t(0)) * scale


# ---- Concat ----------------------------------------------------------------------------------------------------------
def concat_forward(bottoms):
    """bottoms (num_concats, extent_b, inner) -> top"""
    return np.concatenate(bottoms, axis=1)


def concat_backward(top_diff, extents):
    offs = np.concatenate([[0], np.cumsum(extents)])
    return [np.ascontiguousarray(top_diff[:, offs[b]:offs[b + 1], :]) for b in range(len(extents))]


# ---- inputs ----------------------------------------------------------------------------------------------------------
def ip_dense(M, Kdim, N, dtype, seed, transpose=False):
    r = np.random.default_rng(seed + 7919 * M + 31 * Kdim + N)
    wshape = (Kdim, N) if transpose else (N, Kdim)
    d = dict(x=r.uniform(-1, 1, (M, Kdim)), w=r.uniform(-1, 1, wshape) * np.sqrt(3.0 / Kdim), b=r.uniform(-0.2, 0.2, N),
             td=r.uniform(-1, 1, (M, N)), w_diff0=r.uniform(-0.1, 0.1, wshape), b_diff0=r.uniform(-0.1, 0.1, N))
    return {k: v.astype(dtype) for k, v in d.items()}


def ip_integers(M, Kdim, N, seed, transpose=False):
    """|values| <= 8: every product is at most 64 and every sum of the largest shape here far below 2^24"""
    r = np.random.default_rng(seed + 104729 * M + 17 * Kdim + N)
    wshape = (Kdim, N) if transpose else (N, Kdim)
    return dict(x=r.integers(-8, 9, (M, Kdim)), w=r.integers(-8, 9, wshape), b=r.integers(-8, 9, N),
                td=r.integers(-8, 9, (M, N)), w_diff0=r.integers(-8, 9, wshape), b_diff0=r.integers(-8, 9, N))


def labels(r, outer, inner, channels, ignore_label=None, ignored=0.0, out_of_range=0.0):
    lab = r.integers(0, channels, size=(outer, inner)).astype(np.float64)
    if ignore_label is not None and ignored:
        lab[r.random((outer, inner)) < ignored] = ignore_label
    if out_of_range:
        lab[r.random((outer, inner)) < out_of_range] = channels
        lab[r.random((outer, inner)) < out_of_range] = -1
    return lab
