"""ctypes binding of the TRAIN-phase tail Convolution -> BN -> Pool -> TanH -> head of libmms_hip.so
(include/mms_train_tail.h) for torch device tensors: the forward as one call and the backward as one call.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`, `conv`, `head` or `score_tail`.  Errors are capi's: a refusal of this module's own checks raises
`capi.MMSArgumentError` before the library is called, a library error code goes through `capi.check`.  The stream is
torch's current one.  The argument rules are the library's: this module checks the shapes of the tensors it is given
against each other and leaves the rest to the call.
"""
import collections
import ctypes as C

import torch

from . import capi, conv, head, score_tail

POOL_AVE, POOL_MAX = score_tail.POOL_AVE, score_tail.POOL_MAX  # MMS_STAGE_POOL_*
ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = -1, 0, 1             # include/mms_train_tail.h: MMS_TRAIN_TAIL_ROUTE_*
TRAIN = head.TRAIN
NORM_FULL, NORM_VALID, NORM_BATCH_SIZE, NORM_NONE = (head.NORM_FULL, head.NORM_VALID, head.NORM_BATCH_SIZE,
                                                     head.NORM_NONE)
_PREFIX = "mms_train_tail_"
_LABEL = "Train tail"
TrainTailShape = score_tail.ScoreTailShape                     # the calls take an mms_score_tail_shape
train_tail_shape = score_tail.score_tail_shape


def _signatures():
    sp, vp, i, sz, fl = C.POINTER(TrainTailShape), C.c_void_p, C.c_int, C.c_size_t, C.c_float
    query = (sz, [sp])
    fwd = lambda real: (i, [sp, i, real, fl] + [vp] * 22 + [vp, sz, vp])            # noqa: E731
    bwd = lambda real: (i, [sp, i, fl, real] + [vp] * 26 + [vp, sz, vp])            # noqa: E731
    return {
        _PREFIX + "route": (i, [sp]),
        _PREFIX + "workspace_bytes": query,
        _PREFIX + "workspace_bytes_f64": query,
        _PREFIX + "sequence_workspace_bytes": query,
        _PREFIX + "fused_workspace_bytes": query,
        _PREFIX + "forward_f32": fwd(C.c_float),
        _PREFIX + "forward_f64": fwd(C.c_double),
        _PREFIX + "forward_sequence_f32": fwd(C.c_float),
        _PREFIX + "forward_fused_f32": fwd(C.c_float),
        _PREFIX + "backward_f32": bwd(C.c_float),
        _PREFIX + "backward_f64": bwd(C.c_double),
    }


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

Saved = collections.namedtuple("Saved", "y flt save_pool save_mean save_std h prob loss")


def lib():
    """capi.lib(), with the mms_train_tail_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def train_tail_route(shape):
    """ROUTE_FUSED or ROUTE_SEQUENCE of train_tail_forward; ROUTE_NONE for what the calls refuse (mms_train_tail_route)."""
    return lib().mms_train_tail_route(C.byref(shape))


def train_tail_route_f64(shape):
    """The double call has one route: ROUTE_SEQUENCE wherever train_tail_route does not say ROUTE_NONE."""
    return ROUTE_NONE if train_tail_route(shape) == ROUTE_NONE else ROUTE_SEQUENCE


def _query(e, route):
    """The name of the workspace query for `route`."""
    if route == "auto":
        return _PREFIX + "workspace_bytes" + e.query
    if route == "sequence":
        return _PREFIX + ("workspace_bytes_f64" if e.suffix == "f64" else "sequence_workspace_bytes")
    if route == "fused" and e.suffix == "f32":
        return _PREFIX + "fused_workspace_bytes"
    raise capi.MMSArgumentError("%s: route must be 'auto', 'sequence' or (float) 'fused', got %r" % (_LABEL, route))


def _bytes(e, route, shape):
    return getattr(lib(), _query(e, route))(C.byref(shape))


def train_tail_workspace_bytes(shape, route="auto"):
    """Bytes that cover the forward on `route` and the backward of one step (mms_train_tail_workspace_bytes,
    _sequence_workspace_bytes, _fused_workspace_bytes)."""
    return _bytes(capi._F32, route, shape)


def train_tail_workspace_bytes_f64(shape, route="auto"):
    return _bytes(capi._F64, route, shape)


_expect = lambda t, shape, name: capi._expect(_LABEL, t, shape, name)              # noqa: E731


def _geometry(x, weight, pool_window, pool, overlap, w1, w2, stride, pad, group, normalization, ignore_label):
    cshape, (N, K, OH, OW) = conv._shape_of(x, weight, stride, pad, group)
    ph, pw = conv._pair(pool_window, "pool_window")
    if (ph, pw) != (OH, OW):
        raise capi.MMSArgumentError("%s: the %d x %d window is not the convolution's whole %d x %d map"
                                    % (_LABEL, ph, pw, OH, OW))
    if w1 is None or w2 is None or w1.dim() != 2 or w2.dim() != 2 or (overlap is not None and overlap.dim() != 2):
        raise capi.MMSArgumentError("%s: overlap must be (N, F1) or None, w1 (H, K + F1) and w2 (C, H)" % _LABEL)
    F1 = 0 if overlap is None else int(overlap.shape[1])
    H, C_ = int(w1.shape[0]), int(w2.shape[0])
    shape = train_tail_shape(cshape, (ph, pw), pool, F1, H, C_, normalization, ignore_label)
    for t, want, name in ((overlap, (N, F1), "overlap"), (w1, (H, K + F1), "w1"), (w2, (C_, H), "w2")):
        _expect(t, want, name)
    return shape, (N, K, OH, OW), F1, H, C_


def _forward(e, x, weight, bias, pool_window, pool, scale, shift, running_mean, running_var, overlap, w1, b1, mask, w2,
             b2, label, y, flt, save_pool, save_mean, save_std, h, prob, loss, bn_memory, dropout_ratio, stride, pad,
             group, normalization, ignore_label, ws, route):
    lib()                                          # the signatures are on the handle before capi._call uses it
    query = _query(e, route)                       # the route's name is judged first
    shape, (N, K, OH, OW), F1, H, C_ = _geometry(x, weight, pool_window, pool, overlap, w1, w2, stride, pad, group,
                                                 normalization, ignore_label)
    dt, dev = e.dtype, x.device
    new = lambda s: torch.empty(s, dtype=dt, device=dev)                           # noqa: E731
    y = new((N, K, OH, OW)) if y is None else y
    flt = new((N, K)) if flt is None else flt
    save_pool = new((N, K)) if save_pool is None else save_pool
    save_mean = new((K,)) if save_mean is None else save_mean
    save_std = new((K,)) if save_std is None else save_std
    h = new((N, H)) if h is None else h
    prob = new((N, C_)) if prob is None else prob
    if loss is None and label is not None:
        loss = new((1,))
    if mask is None:
        raise capi.MMSArgumentError("%s: TRAIN needs Dropout's mask" % _LABEL)
    for t, want, name in ((y, (N, K, OH, OW), "y"), (flt, (N, K), "flt"), (save_pool, (N, K), "save_pool"),
                          (h, (N, H), "h"), (prob, (N, C_), "prob"), (mask, (N, H), "mask"), (label, (N,), "label"),
                          (b1, (H,), "b1"), (b2, (C_,), "b2"), (bias, (K,), "bias"), (scale, (K,), "scale"),
                          (shift, (K,), "shift"), (running_mean, (K,), "running_mean"),
                          (running_var, (K,), "running_var"), (save_mean, (K,), "save_mean"),
                          (save_std, (K,), "save_std")):
        _expect(t, want, name)
    if loss is not None and loss.numel() != 1:
        raise capi.MMSArgumentError("%s: loss must hold one element, got %s" % (_LABEL, tuple(loss.shape)))
    p = lambda t, name, none=False: capi._ptr(t, name, none, dt)                   # noqa: E731
    wsp, wsb = capi._scratch(ws, getattr(lib(), query)(C.byref(shape)), dev)
    symbol = _PREFIX + ("forward_" + e.suffix if route == "auto" or e.suffix == "f64" else "forward_%s_f32" % route)
    capi._call(symbol, C.byref(shape), TRAIN, float(bn_memory), float(dropout_ratio), p(x, "x"), p(weight, "weight"),
               p(bias, "bias", True), p(scale, "scale"), p(shift, "shift"), p(running_mean, "running_mean"),
               p(running_var, "running_var"), p(overlap, "overlap", True), p(w1, "w1"), p(b1, "b1", True),
               capi._ptr(mask, "mask", False, torch.int32), p(w2, "w2"), p(b2, "b2", True), p(label, "label", True),
               p(y, "y"), p(flt, "flt"), p(save_pool, "save_pool"), p(save_mean, "save_mean"), p(save_std, "save_std"),
               p(h, "h"), p(prob, "prob"), p(loss, "loss", True), wsp, wsb)
    return Saved(y, flt, save_pool, save_mean, save_std, h, prob, loss)


def _backward(e, x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2,
              mask, h, prob, label, loss_weight, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff,
              overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, dropout_ratio, stride, pad, group, normalization,
              ignore_label, ws):
    lib()
    shape, (N, K, OH, OW), F1, H, C_ = _geometry(x, weight, pool_window, pool, overlap, w1, w2, stride, pad, group,
                                                 normalization, ignore_label)
    dt = e.dtype
    if overlap_diff is not None and overlap is None:
        raise capi.MMSArgumentError("%s backward: overlap_diff without overlap" % _LABEL)
    for t, want, name in ((y, (N, K, OH, OW), "y"), (flt, (N, K), "flt"), (save_pool, (N, K), "save_pool"),
                          (h, (N, H), "h"), (prob, (N, C_), "prob"), (mask, (N, H), "mask"), (label, (N,), "label"),
                          (scale, (K,), "scale"), (shift, (K,), "shift"), (save_mean, (K,), "save_mean"),
                          (save_std, (K,), "save_std"), (bottom_diff, x.shape, "bottom_diff"),
                          (weight_diff, weight.shape, "weight_diff"), (bias_diff, (K,), "bias_diff"),
                          (scale_diff, (K,), "scale_diff"), (shift_diff, (K,), "shift_diff"),
                          (overlap_diff, (N, F1), "overlap_diff"), (w1_diff, w1.shape, "w1_diff"),
                          (b1_diff, (H,), "b1_diff"), (w2_diff, w2.shape, "w2_diff"), (b2_diff, (C_,), "b2_diff")):
        _expect(t, want, name)
    if all(t is None for t in (bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, overlap_diff, w1_diff,
                               b1_diff, w2_diff, b2_diff)):
        raise capi.MMSArgumentError("%s backward: no output was given" % _LABEL)
    p = lambda t, name, none=False: capi._ptr(t, name, none, dt)                   # noqa: E731
    wsp, wsb = capi._scratch(ws, getattr(lib(), _query(e, "auto"))(C.byref(shape)), x.device)
    scalar = C.c_float if e.suffix == "f32" else C.c_double
    capi._call(_PREFIX + "backward_" + e.suffix, C.byref(shape), TRAIN, float(dropout_ratio), scalar(float(loss_weight)),
               p(x, "x"), p(weight, "weight"), p(y, "y"), p(flt, "flt"), p(save_pool, "save_pool"), p(scale, "scale"),
               p(shift, "shift", pool == POOL_AVE), p(save_mean, "save_mean"), p(save_std, "save_std"),
               p(overlap, "overlap", True), p(w1, "w1"), p(w2, "w2"), capi._ptr(mask, "mask", False, torch.int32),
               p(h, "h"), p(prob, "prob"), p(label, "label"), p(bottom_diff, "bottom_diff", True),
               p(weight_diff, "weight_diff", True), p(bias_diff, "bias_diff", True), p(scale_diff, "scale_diff", True),
               p(shift_diff, "shift_diff", True), p(overlap_diff, "overlap_diff", True), p(w1_diff, "w1_diff", True),
               p(b1_diff, "b1_diff", True), p(w2_diff, "w2_diff", True), p(b2_diff, "b2_diff", True), wsp, wsb)


def train_tail_forward(x, weight, bias, pool_window, pool, scale, shift, running_mean, running_var, overlap, w1, b1,
                       mask, w2, b2, label=None, y=None, flt=None, save_pool=None, save_mean=None, save_std=None,
                       h=None, prob=None, loss=None, *, bn_memory=0.9, dropout_ratio=0.5, stride=1, pad=0, group=1,
                       normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    """The TRAIN-phase tail Convolution -> BN (batch statistics) -> pooling over the whole map (POOL_AVE / POOL_MAX) ->
    TanH -> Flatten -> [. | overlap] -> fc1 -> TanH -> Dropout(mask) -> fc2 -> SoftmaxWithLoss
    (include/mms_train_tail.h: mms_train_tail_forward_f32).  x (N, C, H, W), weight (K, C/group, kh, kw), bias (K) or
    None; scale, shift (K); running_mean, running_var (K) are updated in place with `bn_memory`; overlap (N, F1) or None;
    w1 (H, K + F1), b1 (H) or None, mask (N, H) int32 of 0 / 1, w2 (C, H), b2 (C) or None; label (N) of the element type
    or None (no loss).  -> Saved(y, flt, save_pool, save_mean, save_std, h, prob, loss), each allocated when None (loss
    only with a label): what train_tail_backward reads.  route: "auto" (mms_train_tail_route decides), "sequence" (the
    two public calls at every shape) or "fused" (the fused launches wherever they reach, an error elsewhere)."""
    return _forward(capi._F32, x, weight, bias, pool_window, pool, scale, shift, running_mean, running_var, overlap, w1,
                    b1, mask, w2, b2, label, y, flt, save_pool, save_mean, save_std, h, prob, loss, bn_memory,
                    dropout_ratio, stride, pad, group, normalization, ignore_label, ws, route)


def train_tail_forward_f64(x, weight, bias, pool_window, pool, scale, shift, running_mean, running_var, overlap, w1, b1,
                           mask, w2, b2, label=None, y=None, flt=None, save_pool=None, save_mean=None, save_std=None,
                           h=None, prob=None, loss=None, *, bn_memory=0.9, dropout_ratio=0.5, stride=1, pad=0, group=1,
                           normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    return _forward(capi._F64, x, weight, bias, pool_window, pool, scale, shift, running_mean, running_var, overlap, w1,
                    b1, mask, w2, b2, label, y, flt, save_pool, save_mean, save_std, h, prob, loss, bn_memory,
                    dropout_ratio, stride, pad, group, normalization, ignore_label, ws, route)


def train_tail_forward_sequence(*args, **kw):
    """train_tail_forward on the SEQUENCE route (mms_train_tail_forward_sequence_f32)."""
    return train_tail_forward(*args, route="sequence", **kw)


def train_tail_forward_fused(*args, **kw):
    """train_tail_forward on the FUSED route (mms_train_tail_forward_fused_f32)."""
    return train_tail_forward(*args, route="fused", **kw)


def train_tail_backward(x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1,
                        w2, mask, h, prob, label, loss_weight=1.0, bottom_diff=None, weight_diff=None, bias_diff=None,
                        scale_diff=None, shift_diff=None, overlap_diff=None, w1_diff=None, b1_diff=None, w2_diff=None,
                        b2_diff=None, *, dropout_ratio=0.5, stride=1, pad=0, group=1, normalization=NORM_VALID,
                        ignore_label=None, ws=None):
    """The tail's backward (mms_train_tail_backward_f32) from what the forward left.  Each of the ten outputs may be None
    (skipped, untouched), at least one is required: bottom_diff, scale_diff, shift_diff and overlap_diff are
    overwritten; weight_diff, bias_diff, w1_diff, b1_diff, w2_diff and b2_diff are accumulated into.  shift may be None
    for POOL_AVE."""
    _backward(capi._F32, x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1,
              w2, mask, h, prob, label, loss_weight, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff,
              overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, dropout_ratio, stride, pad, group, normalization,
              ignore_label, ws)


def train_tail_backward_f64(x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap,
                            w1, w2, mask, h, prob, label, loss_weight=1.0, bottom_diff=None, weight_diff=None,
                            bias_diff=None, scale_diff=None, shift_diff=None, overlap_diff=None, w1_diff=None,
                            b1_diff=None, w2_diff=None, b2_diff=None, *, dropout_ratio=0.5, stride=1, pad=0, group=1,
                            normalization=NORM_VALID, ignore_label=None, ws=None):
    _backward(capi._F64, x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1,
              w2, mask, h, prob, label, loss_weight, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff,
              overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, dropout_ratio, stride, pad, group, normalization,
              ignore_label, ws)
