"""ctypes binding of the routed and the fused backward of the TRAIN-phase tail (include/mms_train_tail_backward.h) for
torch device tensors.  The argument list, the shape checks and the errors are train_tail.train_tail_backward's; the
signatures are applied to the handle `capi.lib()` loads and nothing is added to `capi` or `train_tail`.
"""
import ctypes as C

import torch

from . import capi, train_tail

ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = train_tail.ROUTE_NONE, train_tail.ROUTE_SEQUENCE, train_tail.ROUTE_FUSED
POOL_AVE, POOL_MAX = train_tail.POOL_AVE, train_tail.POOL_MAX
_PREFIX = "mms_train_tail_backward_"
_LABEL = "Train tail backward"


def _signatures():
    sp, vp, i, sz, fl = C.POINTER(train_tail.TrainTailShape), C.c_void_p, C.c_int, C.c_size_t, C.c_float
    bwd = (i, [sp, i, fl, fl] + [vp] * 26 + [vp, sz, vp])
    return {
        _PREFIX + "route": (i, [sp]),
        _PREFIX + "workspace_bytes": (sz, [sp]),
        _PREFIX + "fused_workspace_bytes": (sz, [sp]),
        _PREFIX + "routed_f32": bwd,
        _PREFIX + "fused_f32": bwd,
    }


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_train_tail_backward_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def train_tail_backward_route(shape):
    """ROUTE_FUSED or ROUTE_SEQUENCE of train_tail_backward_routed; ROUTE_NONE for what the calls refuse."""
    return lib().mms_train_tail_backward_route(C.byref(shape))


def train_tail_backward_workspace_bytes(shape, route="auto"):
    """Bytes of train_tail_backward_routed ("auto") or train_tail_backward_fused ("fused": 0 where it does not reach)."""
    if route not in ("auto", "fused"):
        raise capi.MMSArgumentError("%s: route must be 'auto' or 'fused', got %r" % (_LABEL, route))
    name = _PREFIX + ("workspace_bytes" if route == "auto" else "fused_workspace_bytes")
    return getattr(lib(), name)(C.byref(shape))


def _backward(route, x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2,
              mask, h, prob, label, loss_weight, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff,
              overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, dropout_ratio, stride, pad, group, normalization,
              ignore_label, ws):
    lib()
    train_tail.lib()
    if route not in ("auto", "fused"):
        raise capi.MMSArgumentError("%s: route must be 'auto' or 'fused', got %r" % (_LABEL, route))
    shape, (N, K, OH, OW), F1, H, C_ = train_tail._geometry(x, weight, pool_window, pool, overlap, w1, w2, stride, pad,
                                                            group, normalization, ignore_label)
    dt = torch.float32
    if overlap_diff is not None and overlap is None:
        raise capi.MMSArgumentError("%s: overlap_diff without overlap" % _LABEL)
    for t, want, name in ((y, (N, K, OH, OW), "y"), (flt, (N, K), "flt"), (save_pool, (N, K), "save_pool"),
                          (h, (N, H), "h"), (prob, (N, C_), "prob"), (mask, (N, H), "mask"), (label, (N,), "label"),
                          (scale, (K,), "scale"), (shift, (K,), "shift"), (save_mean, (K,), "save_mean"),
                          (save_std, (K,), "save_std"), (bottom_diff, x.shape, "bottom_diff"),
                          (weight_diff, weight.shape, "weight_diff"), (bias_diff, (K,), "bias_diff"),
                          (scale_diff, (K,), "scale_diff"), (shift_diff, (K,), "shift_diff"),
                          (overlap_diff, (N, F1), "overlap_diff"), (w1_diff, w1.shape, "w1_diff"),
                          (b1_diff, (H,), "b1_diff"), (w2_diff, w2.shape, "w2_diff"), (b2_diff, (C_,), "b2_diff")):
        capi._expect(_LABEL, t, want, name)
    if all(t is None for t in (bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, overlap_diff, w1_diff,
                               b1_diff, w2_diff, b2_diff)):
        raise capi.MMSArgumentError("%s: no output was given" % _LABEL)
    p = lambda t, name, none=False: capi._ptr(t, name, none, dt)                   # noqa: E731
    wsp, wsb = capi._scratch(ws, train_tail_backward_workspace_bytes(shape, route), x.device)
    capi._call(_PREFIX + ("routed_f32" if route == "auto" else "fused_f32"), C.byref(shape), train_tail.TRAIN,
               float(dropout_ratio), C.c_float(float(loss_weight)),
               p(x, "x"), p(weight, "weight"), p(y, "y"), p(flt, "flt"), p(save_pool, "save_pool"), p(scale, "scale"),
               p(shift, "shift", pool == POOL_AVE), p(save_mean, "save_mean"), p(save_std, "save_std"),
               p(overlap, "overlap", True), p(w1, "w1"), p(w2, "w2"), capi._ptr(mask, "mask", False, torch.int32),
               p(h, "h"), p(prob, "prob"), p(label, "label"), p(bottom_diff, "bottom_diff", True),
               p(weight_diff, "weight_diff", True), p(bias_diff, "bias_diff", True), p(scale_diff, "scale_diff", True),
               p(shift_diff, "shift_diff", True), p(overlap_diff, "overlap_diff", True), p(w1_diff, "w1_diff", True),
               p(b1_diff, "b1_diff", True), p(w2_diff, "w2_diff", True), p(b2_diff, "b2_diff", True), wsp, wsb)


def train_tail_backward_routed(x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std,
                               overlap, w1, w2, mask, h, prob, label, loss_weight=1.0, bottom_diff=None,
                               weight_diff=None, bias_diff=None, scale_diff=None, shift_diff=None, overlap_diff=None,
                               w1_diff=None, b1_diff=None, w2_diff=None, b2_diff=None, *, dropout_ratio=0.5, stride=1,
                               pad=0, group=1, normalization=train_tail.NORM_VALID, ignore_label=None, ws=None,
                               route="auto"):
    """train_tail.train_tail_backward's arguments and rules (mms_train_tail_backward_routed_f32): the fused launches
    where mms_train_tail_backward_route says so, mms_train_tail_backward_f32 itself elsewhere.  route="fused": the fused
    launches wherever they reach, an error elsewhere (mms_train_tail_backward_fused_f32)."""
    _backward(route, x, weight, pool_window, pool, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2,
              mask, h, prob, label, loss_weight, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff,
              overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, dropout_ratio, stride, pad, group, normalization,
              ignore_label, ws)


def train_tail_backward_fused(*args, **kw):
    """train_tail_backward_routed on the FUSED route (mms_train_tail_backward_fused_f32)."""
    train_tail_backward_routed(*args, route="fused", **kw)
