"""ctypes binding of the InnerProduct, Softmax, SoftmaxWithLoss and Concat calls of libmms_hip.so (include/mms_fc.h) for
torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.  The element
type is the tensor's: float32 tensors go to the _f32 calls, float64 tensors to the _f64 calls.

    feat = concat_forward([q, a, sim, overlap])                            # axis 1 of (N, *) blobs
    z = inner_product_forward(feat, w1, b1)                                # transpose=True: w1 is (K, N_out)
    prob, loss = softmax_loss_forward(z2, label)
    dz2 = softmax_loss_backward(prob, label)
    inner_product_backward(d, w2, dz2, w_diff=dw2, b_diff=db2, bottom_diff=dd)     # dw2, db2: accumulated into
    dq, da, dsim, dov = concat_backward(dfeat, [q.shape, a.shape, sim.shape, overlap.shape])
"""
import ctypes as C

import torch

from . import capi

ROUTE_NONE, ROUTE_GENERIC, ROUTE_FAST = -1, 0, 1               # include/mms_fc.h: MMS_FC_ROUTE_*
PASS_FORWARD, PASS_BACKWARD = 0, 1                             # MMS_FC_PASS_*
NORM_FULL, NORM_VALID, NORM_BATCH_SIZE, NORM_NONE = 0, 1, 2, 3  # MMS_LOSS_NORM_*
CONCAT_MAX_BOTTOMS = 8                                         # MMS_CONCAT_MAX_BOTTOMS


class InnerProductShape(C.Structure):
    """mms_inner_product_shape"""
    _fields_ = [(n, C.c_int) for n in ("M", "K", "N_out", "transpose", "bias_term")]


class SoftmaxShape(C.Structure):
    """mms_softmax_shape"""
    _fields_ = [(n, C.c_int) for n in ("outer", "channels", "inner")]


class SoftmaxLossShape(C.Structure):
    """mms_softmax_loss_shape"""
    _fields_ = [(n, C.c_int) for n in ("outer", "channels", "inner", "normalization", "has_ignore_label",
                                       "ignore_label")]


class ConcatShape(C.Structure):
    """mms_concat_shape"""
    _fields_ = [("num_concats", C.c_int), ("concat_input_size", C.c_int), ("num_bottoms", C.c_int),
                ("axis_extent", C.c_int * CONCAT_MAX_BOTTOMS)]


_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_ip, _sm, _sl, _cc = (C.POINTER(t) for t in (InnerProductShape, SoftmaxShape, SoftmaxLossShape, ConcatShape))
_IP_FWD = (_i, [_ip, _vp, _vp, _vp, _vp, _vp])
_IP_BWD = (_i, [_ip, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp])
_SM_FWD = (_i, [_sm, _vp, _vp, _vp])
_SM_BWD = (_i, [_sm, _vp, _vp, _vp, _vp])
_SL_FWD = (_i, [_sl, _vp, _vp, _vp, _vp, _vp, _sz, _vp])
_CC = (_i, [_cc, _vp, _vp, _vp])


def _sl_bwd(scalar):
    """loss_weight, the one argument by value, has the element type"""
    return (_i, [_sl, _vp, _vp, scalar, _vp, _vp, _sz, _vp])


_SIGNATURES = {
    "mms_inner_product_workspace_bytes": (_sz, [_ip]),
    "mms_inner_product_workspace_bytes_f64": (_sz, [_ip]),
    "mms_inner_product_route": (_i, [_ip, _i]),
    "mms_inner_product_forward_f32": _IP_FWD,
    "mms_inner_product_forward_f64": _IP_FWD,
    "mms_inner_product_backward_f32": _IP_BWD,
    "mms_inner_product_backward_f64": _IP_BWD,
    "mms_inner_product_forward_generic_f32": _IP_FWD,
    "mms_inner_product_backward_generic_f32": _IP_BWD,
    "mms_softmax_forward_f32": _SM_FWD,
    "mms_softmax_forward_f64": _SM_FWD,
    "mms_softmax_backward_f32": _SM_BWD,
    "mms_softmax_backward_f64": _SM_BWD,
    "mms_softmax_loss_workspace_bytes": (_sz, [_sl]),
    "mms_softmax_loss_workspace_bytes_f64": (_sz, [_sl]),
    "mms_softmax_loss_forward_f32": _SL_FWD,
    "mms_softmax_loss_forward_f64": _SL_FWD,
    "mms_softmax_loss_backward_f32": _sl_bwd(C.c_float),
    "mms_softmax_loss_backward_f64": _sl_bwd(C.c_double),
    "mms_concat_forward_f32": _CC,
    "mms_concat_forward_f64": _CC,
    "mms_concat_backward_f32": _CC,
    "mms_concat_backward_f64": _CC,
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the signatures of include/mms_fc.h applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _elem(t, label, name="x"):
    if not isinstance(t, torch.Tensor):
        raise capi.MMSArgumentError("%s: %s must be a tensor, got %r" % (label, name, type(t).__name__))
    for e in (capi._F32, capi._F64):
        if e.dtype == t.dtype:
            return e
    raise capi.MMSArgumentError("%s: float32 or float64, got %s" % (label, t.dtype))


# ---- InnerProduct ---------------------------------------------------------------------------------------------------
def inner_product_shape(M, K, N_out, transpose=False, bias_term=True):
    return InnerProductShape(int(M), int(K), int(N_out), int(bool(transpose)), int(bool(bias_term)))


def inner_product_workspace_bytes(shape):
    """Bytes the float backward needs (mms_inner_product_workspace_bytes)."""
    return lib().mms_inner_product_workspace_bytes(C.byref(shape))


def inner_product_workspace_bytes_f64(shape):
    return lib().mms_inner_product_workspace_bytes_f64(C.byref(shape))


def inner_product_route(shape, pass_):
    """ROUTE_FAST or ROUTE_GENERIC for PASS_FORWARD / PASS_BACKWARD of the float calls; ROUTE_NONE for a shape they
    refuse (mms_inner_product_route)."""
    return lib().mms_inner_product_route(C.byref(shape), int(pass_))


def _ip_shape(x, w, transpose, bias_term, name="x"):
    e = _elem(x, "InnerProduct", name)
    if x.dim() != 2 or not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise capi.MMSArgumentError("InnerProduct: %s must be (M, *) and w (N_out, K), or (K, N_out) with transpose" % name)
    K, N_out = (int(v) for v in (w.shape if transpose else w.shape[::-1]))
    return e, inner_product_shape(x.shape[0], K, N_out, transpose, bias_term)


def inner_product_forward(x, w, b=None, out=None, *, transpose=False, route="auto"):
    """top (M, N_out) = x . w^T (+ b) (mms_inner_product_forward_f32 / _f64 by x's dtype) -> out, allocated when None.
    x (M, K); w (N_out, K), or (K, N_out) with transpose; b (N_out) or None (bias_term false).  route: "auto"
    (mms_inner_product_route decides) or "generic"."""
    e, shape = _ip_shape(x, w, transpose, b is not None)
    capi._expect("InnerProduct", x, (shape.M, shape.K), "x")
    capi._expect("InnerProduct", b, (shape.N_out,), "b")
    if out is None:
        out = torch.empty((shape.M, shape.N_out), dtype=e.dtype, device=x.device)
    capi._expect("InnerProduct", out, (shape.M, shape.N_out), "out")
    lib()
    capi._call(capi._route_symbol("InnerProduct", "inner_product", "forward", e, route), C.byref(shape),
               capi._ptr(x, "x", dtype=e.dtype), capi._ptr(w, "w", dtype=e.dtype), capi._ptr(b, "b", True, e.dtype),
               capi._ptr(out, "out", dtype=e.dtype))
    return out


def inner_product_backward(x, w, top_diff, w_diff=None, b_diff=None, bottom_diff=None, *, transpose=False, ws=None,
                           route="auto"):
    """mms_inner_product_backward_f32 / _f64 by top_diff's dtype.  w_diff (w's shape) and b_diff (N_out) are ACCUMULATED
    INTO, bottom_diff (M, K) is OVERWRITTEN; each may be None (not computed), at least one must be given.  x may be None
    without w_diff.  -> (w_diff, b_diff, bottom_diff)."""
    e, shape = _ip_shape(top_diff, w, transpose, b_diff is not None, "top_diff")
    capi._expect("InnerProduct", top_diff, (shape.M, shape.N_out), "top_diff")
    capi._expect("InnerProduct", x, (shape.M, shape.K), "x")
    capi._expect("InnerProduct", w_diff, w.shape, "w_diff")
    capi._expect("InnerProduct", b_diff, (shape.N_out,), "b_diff")
    capi._expect("InnerProduct", bottom_diff, (shape.M, shape.K), "bottom_diff")
    if w_diff is None and b_diff is None and bottom_diff is None:
        raise capi.MMSArgumentError("InnerProduct backward: none of the three diffs was given")
    need = getattr(lib(), "mms_inner_product_workspace_bytes" + e.query)(C.byref(shape)) \
        if (w_diff is not None or b_diff is not None) else 0
    wsp, wsb = capi._scratch(ws, need, top_diff.device)
    dt = e.dtype
    capi._call(capi._route_symbol("InnerProduct", "inner_product", "backward", e, route), C.byref(shape),
               capi._ptr(x, "x", True, dt), capi._ptr(w, "w", dtype=dt), capi._ptr(top_diff, "top_diff", dtype=dt),
               capi._ptr(w_diff, "w_diff", True, dt), capi._ptr(b_diff, "b_diff", True, dt),
               capi._ptr(bottom_diff, "bottom_diff", True, dt), wsp, wsb)
    return w_diff, b_diff, bottom_diff


# ---- Softmax --------------------------------------------------------------------------------------------------------
def _oci(t, axis, label):
    """(outer, channels, inner) of a blob for a softmax along `axis`"""
    if t.dim() < 1 or not -t.dim() <= axis < t.dim():
        raise capi.MMSArgumentError("%s: axis %r of a %d-axis blob" % (label, axis, t.dim()))
    axis %= t.dim()
    outer = inner = 1
    for v in t.shape[:axis]:
        outer *= int(v)
    for v in t.shape[axis + 1:]:
        inner *= int(v)
    return outer, int(t.shape[axis]), inner


def _like(t, out, label, name="out"):
    if out is None:
        return torch.empty_like(t, memory_format=torch.contiguous_format)
    if not isinstance(out, torch.Tensor) or out.shape != t.shape:
        raise capi.MMSArgumentError("%s: %s must be a tensor of shape %s" % (label, name, tuple(t.shape)))
    return out


def softmax_forward(x, out=None, *, axis=1):
    """top = softmax(x) along `axis` (mms_softmax_forward_f32 / _f64 by x's dtype) -> out, allocated when None."""
    e = _elem(x, "Softmax")
    shape = SoftmaxShape(*_oci(x, axis, "Softmax"))
    out = _like(x, out, "Softmax")
    lib()
    capi._call("mms_softmax_forward_" + e.suffix, C.byref(shape), capi._ptr(x, "x", dtype=e.dtype),
               capi._ptr(out, "out", dtype=e.dtype))
    return out


def softmax_backward(top, top_diff, out=None, *, axis=1):
    """bottom_diff = (top_diff - dot) * top (mms_softmax_backward_f32 / _f64) -> out, allocated when None; out may be
    top_diff."""
    e = _elem(top, "Softmax", "top")
    shape = SoftmaxShape(*_oci(top, axis, "Softmax"))
    top_diff = _like(top, top_diff, "Softmax", "top_diff")
    out = _like(top, out, "Softmax")
    lib()
    capi._call("mms_softmax_backward_" + e.suffix, C.byref(shape), capi._ptr(top, "top", dtype=e.dtype),
               capi._ptr(top_diff, "top_diff", dtype=e.dtype), capi._ptr(out, "out", dtype=e.dtype))
    return out


# ---- SoftmaxWithLoss ------------------------------------------------------------------------------------------------
def softmax_loss_shape(outer, channels, inner, normalization=NORM_VALID, ignore_label=None):
    """An mms_softmax_loss_shape.  ignore_label: None (has_ignore_label false) or the label to ignore."""
    return SoftmaxLossShape(int(outer), int(channels), int(inner), int(normalization),
                            0 if ignore_label is None else 1, 0 if ignore_label is None else int(ignore_label))


def softmax_loss_workspace_bytes(shape):
    return lib().mms_softmax_loss_workspace_bytes(C.byref(shape))


def softmax_loss_workspace_bytes_f64(shape):
    return lib().mms_softmax_loss_workspace_bytes_f64(C.byref(shape))


def _loss_args(blob, label, axis, normalization, ignore_label, ws):
    e = _elem(blob, "SoftmaxWithLoss")
    outer, channels, inner = _oci(blob, axis, "SoftmaxWithLoss")
    if not isinstance(label, torch.Tensor) or label.numel() != outer * inner:
        raise capi.MMSArgumentError("SoftmaxWithLoss: label must hold outer * inner = %d elements" % (outer * inner))
    shape = softmax_loss_shape(outer, channels, inner, normalization, ignore_label)
    need = getattr(lib(), "mms_softmax_loss_workspace_bytes" + e.query)(C.byref(shape))
    return e, shape, capi._scratch(ws, need, blob.device)


def softmax_loss_forward(x, label, prob=None, loss=None, *, axis=1, normalization=NORM_VALID, ignore_label=None,
                         ws=None):
    """(prob, loss) of mms_softmax_loss_forward_f32 / _f64 by x's dtype, each allocated when None.  label holds
    outer * inner elements of x's dtype."""
    e, shape, (wsp, wsb) = _loss_args(x, label, axis, normalization, ignore_label, ws)
    prob = _like(x, prob, "SoftmaxWithLoss", "prob")
    if loss is None:
        loss = torch.empty((1,), dtype=e.dtype, device=x.device)
    if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
        raise capi.MMSArgumentError("SoftmaxWithLoss: loss must hold one element")
    dt = e.dtype
    capi._call("mms_softmax_loss_forward_" + e.suffix, C.byref(shape), capi._ptr(x, "x", dtype=dt),
               capi._ptr(label, "label", dtype=dt), capi._ptr(prob, "prob", dtype=dt), capi._ptr(loss, "loss", dtype=dt),
               wsp, wsb)
    return prob, loss


def softmax_loss_backward(prob, label, loss_weight=1.0, out=None, *, axis=1, normalization=NORM_VALID,
                          ignore_label=None, ws=None):
    """bottom_diff of mms_softmax_loss_backward_f32 / _f64 from the forward's prob -> out, allocated when None and
    overwritten.  loss_weight: the loss top's diff, a host number."""
    e, shape, (wsp, wsb) = _loss_args(prob, label, axis, normalization, ignore_label, ws)
    out = _like(prob, out, "SoftmaxWithLoss")
    dt = e.dtype
    scalar = C.c_float if e.suffix == "f32" else C.c_double
    capi._call("mms_softmax_loss_backward_" + e.suffix, C.byref(shape), capi._ptr(prob, "prob", dtype=dt),
               capi._ptr(label, "label", dtype=dt), scalar(float(loss_weight)), capi._ptr(out, "out", dtype=dt), wsp, wsb)
    return out


# ---- Concat ---------------------------------------------------------------------------------------------------------
def _concat_shape(shapes, axis):
    """(ConcatShape, top's shape) of bottoms of these shapes"""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    if not 1 <= len(shapes) <= CONCAT_MAX_BOTTOMS:
        raise capi.MMSArgumentError("Concat: 1 to %d bottoms, got %d" % (CONCAT_MAX_BOTTOMS, len(shapes)))
    nd = len(shapes[0])
    if nd < 1 or not -nd <= axis < nd:
        raise capi.MMSArgumentError("Concat: axis %r of a %d-axis blob" % (axis, nd))
    axis %= nd
    for s in shapes:
        if len(s) != nd or s[:axis] != shapes[0][:axis] or s[axis + 1:] != shapes[0][axis + 1:]:
            raise capi.MMSArgumentError("Concat: bottoms must agree in every axis but %d, got %s" % (axis, shapes))
    outer = inner = 1
    for v in shapes[0][:axis]:
        outer *= v
    for v in shapes[0][axis + 1:]:
        inner *= v
    ext = (C.c_int * CONCAT_MAX_BOTTOMS)(*[s[axis] for s in shapes])
    top = shapes[0][:axis] + (sum(s[axis] for s in shapes),) + shapes[0][axis + 1:]
    return ConcatShape(outer, inner, len(shapes), ext), top


def _pointers(tensors, dt):
    return (C.c_void_p * len(tensors))(*[capi._ptr(t, "bottom %d" % i, True, dt) for i, t in enumerate(tensors)])


def concat_forward(bottoms, out=None, *, axis=1):
    """top = the bottoms side by side along `axis` (mms_concat_forward_f32 / _f64 by their dtype), one launch -> out,
    allocated when None."""
    bottoms = list(bottoms)
    e = _elem(bottoms[0] if bottoms else None, "Concat", "bottoms[0]")
    for t in bottoms:
        _elem(t, "Concat", "a bottom")
    shape, top = _concat_shape([t.shape for t in bottoms], axis)
    if out is None:
        out = torch.empty(top, dtype=e.dtype, device=bottoms[0].device)
    capi._expect("Concat", out, top, "out")
    lib()
    capi._call("mms_concat_forward_" + e.suffix, C.byref(shape), _pointers(bottoms, e.dtype),
               capi._ptr(out, "out", dtype=e.dtype))
    return out


def concat_backward(top_diff, shapes, outs=None, *, axis=1):
    """The bottom diffs of mms_concat_backward_f32 / _f64: top_diff split along `axis` into blobs of `shapes`, one
    launch.  outs: None (all allocated), or a list with a tensor, True (allocate) or None / False (propagate_down false:
    skipped) per bottom.  -> the list of diffs, None where skipped."""
    e = _elem(top_diff, "Concat", "top_diff")
    shape, top = _concat_shape(shapes, axis)
    capi._expect("Concat", top_diff, top, "top_diff")
    outs = [True] * len(shapes) if outs is None else list(outs)
    if len(outs) != len(shapes):
        raise capi.MMSArgumentError("Concat backward: %d outs for %d bottoms" % (len(outs), len(shapes)))
    diffs = []
    for o, s in zip(outs, shapes):
        if o is True:
            o = torch.empty(tuple(s), dtype=e.dtype, device=top_diff.device)
        elif o is False or o is None:
            o = None
        else:
            capi._expect("Concat", o, tuple(s), "a bottom diff")
        diffs.append(o)
    lib()
    capi._call("mms_concat_backward_" + e.suffix, C.byref(shape), capi._ptr(top_diff, "top_diff", dtype=e.dtype),
               _pointers(diffs, e.dtype))
    return diffs


# The _f64 forms: the element type is the tensor's, so these are the same functions under the names the other families use.
inner_product_forward_f64, inner_product_backward_f64 = inner_product_forward, inner_product_backward
softmax_forward_f64, softmax_backward_f64 = softmax_forward, softmax_backward
softmax_loss_forward_f64, softmax_loss_backward_f64 = softmax_loss_forward, softmax_loss_backward
concat_forward_f64, concat_backward_f64 = concat_forward, concat_backward
