"""ctypes binding of the classifier-head calls of libmms_hip.so (include/mms_head.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.
"""
import ctypes as C
import functools

import torch

from . import capi

TRAIN, TEST = 0, 1                                             # include/mms_head.h: MMS_HEAD_TRAIN / _TEST
NORM_FULL, NORM_VALID, NORM_BATCH_SIZE, NORM_NONE = 0, 1, 2, 3  # MMS_HEAD_NORM_*
PASS_FORWARD, PASS_BACKWARD = 0, 1                             # MMS_HEAD_PASS_*
ROUTE_NONE, ROUTE_GENERIC, ROUTE_FAST = -1, 0, 1               # MMS_HEAD_ROUTE_*


class HeadShape(C.Structure):
    """mms_head_shape"""
    _fields_ = [("N", C.c_int), ("F0", C.c_int), ("F1", C.c_int), ("H", C.c_int), ("C", C.c_int), ("phase", C.c_int),
                ("dropout_ratio", C.c_float), ("normalization", C.c_int), ("has_ignore_label", C.c_int),
                ("ignore_label", C.c_int)]


_sp, _vp, _i, _sz = C.POINTER(HeadShape), C.c_void_p, C.c_int, C.c_size_t


_FWD = (_i, [_sp] + [_vp] * 11 + [_vp, _sz, _vp])


def _bwd(scalar):
    """loss_weight, the one argument by value, has the element type"""
    return (_i, [_sp] + [_vp] * 8 + [scalar] + [_vp] * 6 + [_vp, _sz, _vp])


_SIGNATURES = {
    "mms_head_workspace_bytes": (_sz, [_sp]),
    "mms_head_workspace_bytes_f64": (_sz, [_sp]),
    "mms_head_route": (_i, [_sp, _i]),
    "mms_head_forward_f32": _FWD,
    "mms_head_backward_f32": _bwd(C.c_float),
    "mms_head_forward_f64": _FWD,
    "mms_head_backward_f64": _bwd(C.c_double),
    "mms_head_forward_generic_f32": _FWD,
    "mms_head_backward_generic_f32": _bwd(C.c_float),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_head_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def head_shape(N, F0, F1, H, C_, phase=TRAIN, dropout_ratio=0.5, normalization=NORM_VALID, ignore_label=None):
    """An mms_head_shape.  ignore_label: None (has_ignore_label false) or the label to ignore."""
    return HeadShape(int(N), int(F0), int(F1), int(H), int(C_), int(phase), float(dropout_ratio), int(normalization),
                     0 if ignore_label is None else 1, 0 if ignore_label is None else int(ignore_label))


def head_workspace_bytes(shape):
    """Bytes either pass needs for its slabs (mms_head_workspace_bytes)."""
    return lib().mms_head_workspace_bytes(C.byref(shape))


def head_workspace_bytes_f64(shape):
    return lib().mms_head_workspace_bytes_f64(C.byref(shape))


def head_route(shape, pass_):
    """ROUTE_FAST or ROUTE_GENERIC for PASS_FORWARD / PASS_BACKWARD of the float calls; ROUTE_NONE for a shape they
    refuse (mms_head_route)."""
    return lib().mms_head_route(C.byref(shape), int(pass_))


def head_route_f64(shape, pass_):
    """The double calls have one route: ROUTE_GENERIC wherever head_route does not say ROUTE_NONE."""
    return ROUTE_NONE if head_route(shape, pass_) == ROUTE_NONE else ROUTE_GENERIC


_expect = functools.partial(capi._expect, "Head")
_symbol = functools.partial(capi._route_symbol, "Head", "head")


def _shape_of(x0, x1, w1, w2, phase, dropout_ratio, normalization, ignore_label):
    if x0 is None or w1 is None or w2 is None or x0.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or \
            (x1 is not None and x1.dim() != 2):
        raise capi.MMSArgumentError("Head: x0 must be (N, F0), x1 (N, F1) or None, w1 (H, F0 + F1) and w2 (C, H)")
    N, F0 = (int(v) for v in x0.shape)
    F1 = 0 if x1 is None else int(x1.shape[1])
    H, C_ = int(w1.shape[0]), int(w2.shape[0])
    if x1 is not None and int(x1.shape[0]) != N:
        raise capi.MMSArgumentError("Head: x1 has %d rows, x0 %d" % (int(x1.shape[0]), N))
    _expect(w1, (H, F0 + F1), "w1")
    _expect(w2, (C_, H), "w2")
    if phase not in (TRAIN, TEST):
        raise capi.MMSArgumentError("Head: phase must be TRAIN or TEST, got %r" % (phase,))
    return head_shape(N, F0, F1, H, C_, phase, dropout_ratio, normalization, ignore_label)


def _head_forward(e, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, phase, dropout_ratio, normalization,
                  ignore_label, ws, route):
    shape = _shape_of(x0, x1, w1, w2, phase, dropout_ratio, normalization, ignore_label)
    N, H, C_ = shape.N, shape.H, shape.C
    dt = e.dtype
    if h is None:
        h = torch.empty((N, H), dtype=dt, device=x0.device)
    if prob is None:
        prob = torch.empty((N, C_), dtype=dt, device=x0.device)
    if loss is None and label is not None:
        loss = torch.empty((1,), dtype=dt, device=x0.device)
    if loss is not None and label is None:
        raise capi.MMSArgumentError("Head: a loss needs a label (the deploy form has neither)")
    if phase == TRAIN and mask is None:
        raise capi.MMSArgumentError("Head: TRAIN needs Dropout's mask")
    _expect(h, (N, H), "h")
    _expect(prob, (N, C_), "prob")
    _expect(b1, (H,), "b1")
    _expect(b2, (C_,), "b2")
    _expect(mask, (N, H), "mask")
    _expect(label, (N,), "label")
    if loss is not None and loss.numel() != 1:
        raise capi.MMSArgumentError("Head: loss must hold one element, got %s" % (tuple(loss.shape),))
    symbol = _symbol("forward", e, route)
    need = getattr(lib(), "mms_head_workspace_bytes" + e.query)(C.byref(shape)) if loss is not None else 0
    wsp, wsb = capi._scratch(ws, need, x0.device)
    capi._call(symbol, C.byref(shape), capi._ptr(x0, "x0", dtype=dt), capi._ptr(x1, "x1", True, dt),
               capi._ptr(w1, "w1", dtype=dt), capi._ptr(b1, "b1", True, dt),
               capi._ptr(mask, "mask", True, torch.int32), capi._ptr(w2, "w2", dtype=dt),
               capi._ptr(b2, "b2", True, dt), capi._ptr(label, "label", True, dt), capi._ptr(h, "h", dtype=dt),
               capi._ptr(prob, "prob", dtype=dt), capi._ptr(loss, "loss", True, dt), wsp, wsb)
    return h, prob, loss


def _head_backward(e, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff, w2_diff,
                   b2_diff, phase, dropout_ratio, normalization, ignore_label, ws, route):
    shape = _shape_of(x0, x1, w1, w2, phase, dropout_ratio, normalization, ignore_label)
    N, H, C_ = shape.N, shape.H, shape.C
    if phase == TRAIN and mask is None:
        raise capi.MMSArgumentError("Head: TRAIN needs Dropout's mask")
    _expect(h, (N, H), "h")
    _expect(prob, (N, C_), "prob")
    _expect(mask, (N, H), "mask")
    _expect(label, (N,), "label")
    _expect(x0_diff, x0.shape, "x0_diff")
    if x1_diff is not None and x1 is None:
        raise capi.MMSArgumentError("Head backward: x1_diff without x1")
    if x1 is not None:
        _expect(x1_diff, x1.shape, "x1_diff")
    _expect(w1_diff, w1.shape, "w1_diff")
    _expect(b1_diff, (H,), "b1_diff")
    _expect(w2_diff, w2.shape, "w2_diff")
    _expect(b2_diff, (C_,), "b2_diff")
    if all(t is None for t in (x0_diff, x1_diff, w1_diff, b1_diff, w2_diff, b2_diff)):
        raise capi.MMSArgumentError("Head backward: none of the six diffs was given")
    dt = e.dtype
    symbol = _symbol("backward", e, route)
    need = getattr(lib(), "mms_head_workspace_bytes" + e.query)(C.byref(shape))
    wsp, wsb = capi._scratch(ws, need, x0.device)
    scalar = C.c_float if e.suffix == "f32" else C.c_double
    capi._call(symbol, C.byref(shape), capi._ptr(x0, "x0", dtype=dt), capi._ptr(x1, "x1", True, dt),
               capi._ptr(w1, "w1", dtype=dt), capi._ptr(w2, "w2", dtype=dt),
               capi._ptr(mask, "mask", True, torch.int32), capi._ptr(h, "h", dtype=dt),
               capi._ptr(prob, "prob", dtype=dt), capi._ptr(label, "label", dtype=dt), scalar(float(loss_weight)),
               capi._ptr(x0_diff, "x0_diff", True, dt), capi._ptr(x1_diff, "x1_diff", True, dt),
               capi._ptr(w1_diff, "w1_diff", True, dt), capi._ptr(b1_diff, "b1_diff", True, dt),
               capi._ptr(w2_diff, "w2_diff", True, dt), capi._ptr(b2_diff, "b2_diff", True, dt), wsp, wsb)


def head_forward(x0, x1, w1, b1, mask, w2, b2, label=None, h=None, prob=None, loss=None, *, phase=TRAIN,
                 dropout_ratio=0.5, normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    """The head's forward (include/mms_head.h: mms_head_forward_f32).  x0 (N, F0), x1 (N, F1) or None, w1 (H, F0 + F1),
    b1 (H) or None, mask (N, H) int32 of 0 / 1 (Dropout's rand_vec_; None in TEST), w2 (C, H), b2 (C) or None, label (N)
    of the element type or None (the deploy form: no loss).  -> (h, prob, loss), each allocated when None; loss is None
    without a label.  route: "auto" (mms_head_route decides) or "generic"."""
    return _head_forward(capi._F32, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, phase, dropout_ratio,
                         normalization, ignore_label, ws, route)


def head_forward_f64(x0, x1, w1, b1, mask, w2, b2, label=None, h=None, prob=None, loss=None, *, phase=TRAIN,
                     dropout_ratio=0.5, normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    return _head_forward(capi._F64, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, phase, dropout_ratio,
                         normalization, ignore_label, ws, route)


def head_forward_generic(x0, x1, w1, b1, mask, w2, b2, label=None, h=None, prob=None, loss=None, **kw):
    """head_forward on the generic route (mms_head_forward_generic_f32)."""
    return head_forward(x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, route="generic", **kw)


def head_backward(x0, x1, w1, w2, mask, h, prob, label, loss_weight=1.0, x0_diff=None, x1_diff=None, w1_diff=None,
                  b1_diff=None, w2_diff=None, b2_diff=None, *, phase=TRAIN, dropout_ratio=0.5,
                  normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    """The head's backward (mms_head_backward_f32) from the forward's h and prob.  x0_diff and x1_diff are OVERWRITTEN;
    w1_diff, b1_diff, w2_diff and b2_diff are ACCUMULATED INTO (zero them for a fresh gradient).  Each of the six may be
    None (skipped, untouched); at least one must be given.  loss_weight: the loss top's diff, a host number."""
    _head_backward(capi._F32, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff,
                   w2_diff, b2_diff, phase, dropout_ratio, normalization, ignore_label, ws, route)


def head_backward_f64(x0, x1, w1, w2, mask, h, prob, label, loss_weight=1.0, x0_diff=None, x1_diff=None, w1_diff=None,
                      b1_diff=None, w2_diff=None, b2_diff=None, *, phase=TRAIN, dropout_ratio=0.5,
                      normalization=NORM_VALID, ignore_label=None, ws=None, route="auto"):
    _head_backward(capi._F64, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff,
                   w2_diff, b2_diff, phase, dropout_ratio, normalization, ignore_label, ws, route)


def head_backward_generic(x0, x1, w1, w2, mask, h, prob, label, loss_weight=1.0, x0_diff=None, x1_diff=None,
                          w1_diff=None, b1_diff=None, w2_diff=None, b2_diff=None, **kw):
    """head_backward on the generic route (mms_head_backward_generic_f32)."""
    head_backward(x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff, w2_diff,
                  b2_diff, route="generic", **kw)
