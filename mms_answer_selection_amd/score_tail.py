"""ctypes binding of the scoring tail Convolution -> BN -> Pool -> TanH -> head -> prob of libmms_hip.so
(include/mms_score_tail.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`, `conv` or `head`.  Errors are capi's: a refusal of this module's own checks raises
`capi.MMSArgumentError` before the library is called, a library error code goes through `capi.check`.  The stream is
torch's current one.  The argument rules are the library's: this module checks the shapes of the tensors it is given
against each other and leaves the rest to the call.
"""
import ctypes as C

import torch

from . import capi, conv, head

POOL_AVE, POOL_MAX = 0, 1                                      # include/mms_score_tail.h: MMS_STAGE_POOL_*
ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = -1, 0, 1             # MMS_SCORE_TAIL_ROUTE_*
NORM_FULL, NORM_VALID, NORM_BATCH_SIZE, NORM_NONE = (head.NORM_FULL, head.NORM_VALID, head.NORM_BATCH_SIZE,
                                                     head.NORM_NONE)


class ScoreTailShape(C.Structure):
    """mms_score_tail_shape"""
    _fields_ = [("conv", conv.ConvShape), ("ph", C.c_int), ("pw", C.c_int), ("pool", C.c_int), ("F1", C.c_int),
                ("H", C.c_int), ("C", C.c_int), ("normalization", C.c_int), ("has_ignore_label", C.c_int),
                ("ignore_label", C.c_int)]


_sp, _vp, _i, _sz = C.POINTER(ScoreTailShape), C.c_void_p, C.c_int, C.c_size_t
_FWD = (_i, [_sp] + [_vp] * 17 + [_vp, _sz, _vp])

_SIGNATURES = {
    "mms_score_tail_route": (_i, [_sp]),
    "mms_score_tail_workspace_bytes": (_sz, [_sp]),
    "mms_score_tail_workspace_bytes_f64": (_sz, [_sp]),
    "mms_score_tail_sequence_workspace_bytes": (_sz, [_sp]),
    "mms_score_tail_forward_f32": _FWD,
    "mms_score_tail_forward_f64": _FWD,
    "mms_score_tail_forward_sequence_f32": _FWD,
    "mms_score_tail_forward_fused_f32": _FWD,
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_score_tail_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def score_tail_shape(conv_shape, pool_window, pool, F1, H, C_, normalization=NORM_VALID, ignore_label=None):
    """An mms_score_tail_shape from a ConvShape (conv.conv_shape), the pooling window (one int or (ph, pw)), POOL_AVE /
    POOL_MAX and the head's widths.  ignore_label: None (has_ignore_label false) or the label to ignore."""
    ph, pw = conv._pair(pool_window, "pool_window")
    return ScoreTailShape(conv_shape, ph, pw, int(pool), int(F1), int(H), int(C_), int(normalization),
                          0 if ignore_label is None else 1, 0 if ignore_label is None else int(ignore_label))


def score_tail_route(shape):
    """ROUTE_FUSED or ROUTE_SEQUENCE of score_tail_forward; ROUTE_NONE for what the calls refuse
    (mms_score_tail_route)."""
    return lib().mms_score_tail_route(C.byref(shape))


def score_tail_route_f64(shape):
    """The double call has one route: ROUTE_SEQUENCE wherever score_tail_route does not say ROUTE_NONE."""
    return ROUTE_NONE if score_tail_route(shape) == ROUTE_NONE else ROUTE_SEQUENCE


def _query(e, route):
    """The name of the workspace query for `route`."""
    if route == "auto":
        return "mms_score_tail_workspace_bytes" + e.query
    if route == "sequence":
        return "mms_score_tail_workspace_bytes_f64" if e.suffix == "f64" else "mms_score_tail_sequence_workspace_bytes"
    if route == "fused" and e.suffix == "f32":
        return None                                            # 8 N, with a loss only
    raise capi.MMSArgumentError("Score tail: route must be 'auto', 'sequence' or (float) 'fused', got %r" % (route,))


def _bytes(e, route, shape):
    q = _query(e, route)
    return getattr(lib(), q)(C.byref(shape)) if q else 8 * shape.conv.N


def score_tail_workspace_bytes(shape, route="auto"):
    """Bytes score_tail_forward needs (mms_score_tail_workspace_bytes; with route="sequence" the SEQUENCE figure at every
    shape; with route="fused" the FUSED one, which only a call with a loss uses)."""
    return _bytes(capi._F32, route, shape)


def score_tail_workspace_bytes_f64(shape, route="auto"):
    return _bytes(capi._F64, route, shape)


def _symbol(e, route):
    if route == "auto" or e.suffix == "f64":       # double has the sequence route only, and no entry point of that name
        return "mms_score_tail_forward_" + e.suffix
    return "mms_score_tail_forward_%s_f32" % route


_expect = lambda t, shape, name: capi._expect("Score tail", t, shape, name)


def _forward(e, x, weight, bias, pool_window, pool, mean, var, scale, shift, overlap, w1, b1, w2, b2, label, flt, h,
             prob, loss, stride, pad, group, normalization, ignore_label, ws, route):
    lib()                                          # the signatures are on the handle before capi._call uses it
    _query(e, route)                               # the route's name is judged first
    cshape, (N, K, OH, OW) = conv._shape_of(x, weight, stride, pad, group)
    ph, pw = conv._pair(pool_window, "pool_window")
    if ph < 1 or pw < 1 or OH % ph or OW % pw:
        raise capi.MMSArgumentError("Score tail: %d x %d windows do not tile the convolution's %d x %d map"
                                    % (ph, pw, OH, OW))
    if w1 is None or w2 is None or w1.dim() != 2 or w2.dim() != 2 or (overlap is not None and overlap.dim() != 2):
        raise capi.MMSArgumentError("Score tail: overlap must be (N, F1) or None, w1 (H, F0 + F1) and w2 (C, H)")
    F0 = K * (OH // ph) * (OW // pw)
    F1 = 0 if overlap is None else int(overlap.shape[1])
    H, C_ = int(w1.shape[0]), int(w2.shape[0])
    shape = score_tail_shape(cshape, (ph, pw), pool, F1, H, C_, normalization, ignore_label)
    dt, dev = e.dtype, x.device
    if prob is None:
        prob = torch.empty((N, C_), dtype=dt, device=dev)
    if loss is None and label is not None:
        loss = torch.empty((1,), dtype=dt, device=dev)
    for t, want, name in ((overlap, (N, F1), "overlap"), (w1, (H, F0 + F1), "w1"), (w2, (C_, H), "w2"), (b1, (H,), "b1"),
                          (b2, (C_,), "b2"), (label, (N,), "label"), (flt, (N, F0), "flt"), (h, (N, H), "h"),
                          (prob, (N, C_), "prob"), (bias, (K,), "bias"), (mean, (K,), "mean"), (var, (K,), "var"),
                          (scale, (K,), "scale"), (shift, (K,), "shift")):
        _expect(t, want, name)
    if loss is not None and loss.numel() != 1:
        raise capi.MMSArgumentError("Score tail: loss must hold one element, got %s" % (tuple(loss.shape),))
    p = lambda t, name, none=False: capi._ptr(t, name, none, dt)
    wsp, wsb = capi._scratch(ws, _bytes(e, route, shape), dev)
    capi._call(_symbol(e, route), C.byref(shape), p(x, "x"), p(weight, "weight"), p(bias, "bias", True), p(mean, "mean"),
               p(var, "var"), p(scale, "scale"), p(shift, "shift"), p(overlap, "overlap", True), p(w1, "w1"),
               p(b1, "b1", True), p(w2, "w2"), p(b2, "b2", True), p(label, "label", True), p(flt, "flt", True),
               p(h, "h", True), p(prob, "prob"), p(loss, "loss", True), wsp, wsb)
    return prob, loss


def score_tail_forward(x, weight, bias, pool_window, pool, mean, var, scale, shift, overlap, w1, b1, w2, b2, label=None,
                       flt=None, h=None, prob=None, loss=None, *, stride=1, pad=0, group=1, normalization=NORM_VALID,
                       ignore_label=None, ws=None, route="auto"):
    """The TEST-phase tail Convolution -> BN -> pooling (POOL_AVE / POOL_MAX, window = stride) -> TanH -> Flatten ->
    [. | overlap] -> fc1 -> TanH -> fc2 -> Softmax (include/mms_score_tail.h: mms_score_tail_forward_f32).  x (N, C, H,
    W), weight (K, C/group, kh, kw), bias (K) or None; mean, var, scale, shift (K); overlap (N, F1) or None; w1 (H, F0 +
    F1), b1 (H) or None, w2 (C, H), b2 (C) or None; label (N) of the element type or None (the deploy form: no loss).
    -> (prob, loss): prob (N, C) is allocated when None; loss is allocated when there is a label, else None.  flt (N, F0)
    and h (N, H) are written when given.  route: "auto" (mms_score_tail_route decides), "sequence" (the two public calls
    at every shape, mms_score_tail_forward_sequence_f32) or "fused" (the one launch wherever it reaches, an error
    elsewhere, mms_score_tail_forward_fused_f32)."""
    return _forward(capi._F32, x, weight, bias, pool_window, pool, mean, var, scale, shift, overlap, w1, b1, w2, b2,
                    label, flt, h, prob, loss, stride, pad, group, normalization, ignore_label, ws, route)


def score_tail_forward_f64(x, weight, bias, pool_window, pool, mean, var, scale, shift, overlap, w1, b1, w2, b2,
                           label=None, flt=None, h=None, prob=None, loss=None, *, stride=1, pad=0, group=1,
                           normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    return _forward(capi._F64, x, weight, bias, pool_window, pool, mean, var, scale, shift, overlap, w1, b1, w2, b2,
                    label, flt, h, prob, loss, stride, pad, group, normalization, ignore_label, ws, route)


def score_tail_forward_sequence(*args, **kw):
    """score_tail_forward on the SEQUENCE route (mms_score_tail_forward_sequence_f32)."""
    return score_tail_forward(*args, route="sequence", **kw)


def score_tail_forward_fused(*args, **kw):
    """score_tail_forward on the FUSED route (mms_score_tail_forward_fused_f32)."""
    return score_tail_forward(*args, route="fused", **kw)
