"""ctypes binding of the Convolution calls of libmms_hip.so (include/mms_conv.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.
"""
import ctypes as C
import functools

import torch

from . import capi

PASS_FORWARD, PASS_BOTTOM_DIFF, PASS_PARAM_DIFF = 0, 1, 2      # include/mms_conv.h: MMS_CONV_PASS_*
ROUTE_NONE, ROUTE_GENERIC, ROUTE_FAST = -1, 0, 1               # include/mms_conv.h: MMS_CONV_ROUTE_*


class ConvShape(C.Structure):
    """mms_conv_shape"""
    _fields_ = [(n, C.c_int) for n in ("N", "C", "H", "W", "K", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w",
                                       "dilation_h", "dilation_w", "group")]


_sp, _vp, _i, _sz = C.POINTER(ConvShape), C.c_void_p, C.c_int, C.c_size_t
_FWD = (_i, [_sp] + [_vp] * 5 + [_sz, _vp])
_BWD = (_i, [_sp] + [_vp] * 7 + [_sz, _vp])

_SIGNATURES = {
    "mms_conv_output_dims": (_i, [_sp, C.POINTER(_i), C.POINTER(_i)]),
    "mms_conv_workspace_bytes": (_sz, [_sp]),
    "mms_conv_workspace_bytes_f64": (_sz, [_sp]),
    "mms_conv_route": (_i, [_sp, _i]),
    "mms_conv_forward_f32": _FWD,
    "mms_conv_backward_f32": _BWD,
    "mms_conv_forward_f64": _FWD,
    "mms_conv_backward_f64": _BWD,
    "mms_conv_forward_generic_f32": _FWD,
    "mms_conv_backward_generic_f32": _BWD,
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_conv_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _pair(v, name):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise capi.MMSArgumentError("Convolution: %s must be one int or (h, w), got %r" % (name, v))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def conv_shape(N, C_, H, W, K, kernel, stride=1, pad=0, group=1, dilation=1):
    """An mms_conv_shape.  kernel, stride, pad and dilation are one int or (h, w)."""
    kh, kw = _pair(kernel, "kernel")
    sh, sw = _pair(stride, "stride")
    ph, pw = _pair(pad, "pad")
    dh, dw = _pair(dilation, "dilation")
    return ConvShape(int(N), int(C_), int(H), int(W), int(K), kh, kw, sh, sw, ph, pw, dh, dw, int(group))


def conv_output_dims(shape):
    """(OH, OW) of a ConvShape (mms_conv_output_dims); a shape the library refuses raises."""
    oh, ow = _i(), _i()
    capi.check(lib().mms_conv_output_dims(C.byref(shape), C.byref(oh), C.byref(ow)), "mms_conv_output_dims")
    return oh.value, ow.value


conv_output_dims_f64 = conv_output_dims         # the shape arithmetic has no element type


def conv_workspace_bytes(shape):
    """Bytes conv_backward needs for the slabs of weight_diff / bias_diff (mms_conv_workspace_bytes)."""
    return lib().mms_conv_workspace_bytes(C.byref(shape))


def conv_workspace_bytes_f64(shape):
    return lib().mms_conv_workspace_bytes_f64(C.byref(shape))


def conv_route(shape, pass_):
    """ROUTE_FAST or ROUTE_GENERIC for PASS_FORWARD / PASS_BOTTOM_DIFF / PASS_PARAM_DIFF of the float calls; ROUTE_NONE for
    a shape they refuse (mms_conv_route)."""
    return lib().mms_conv_route(C.byref(shape), int(pass_))


def conv_route_f64(shape, pass_):
    """The double calls have one route: ROUTE_GENERIC wherever conv_route does not say ROUTE_NONE."""
    return ROUTE_NONE if conv_route(shape, pass_) == ROUTE_NONE else ROUTE_GENERIC


def _shape_of(x, weight, stride, pad, group):
    if x.dim() != 4 or weight.dim() != 4:
        raise capi.MMSArgumentError("Convolution: x must be (N, C, H, W) and weight (K, C/group, kh, kw), got %s and %s"
                                    % (tuple(x.shape), tuple(weight.shape)))
    N, C_, H, W = (int(v) for v in x.shape)
    K, Cg, kh, kw = (int(v) for v in weight.shape)
    group = int(group)
    if group <= 0 or C_ % group or K % group or Cg != C_ // group:
        raise capi.MMSArgumentError("Convolution: weight %s does not fit %d input channels in %d group(s)"
                                    % (tuple(weight.shape), C_, group))
    shape = conv_shape(N, C_, H, W, K, (kh, kw), stride, pad, group)
    oh, ow = _i(), _i()
    if lib().mms_conv_output_dims(C.byref(shape), C.byref(oh), C.byref(ow)) != capi.MMS_OK:
        raise capi.MMSArgumentError("Convolution: kernel %s, stride %r, pad %r on a %d x %d image is refused"
                                    % ((kh, kw), stride, pad, H, W))
    return shape, (N, K, oh.value, ow.value)


_expect = functools.partial(capi._expect, "Convolution")
_symbol = functools.partial(capi._route_symbol, "Convolution", "conv")


def _conv_forward(e, x, weight, bias, top, stride, pad, group, route):
    shape, top_shape = _shape_of(x, weight, stride, pad, group)
    if top is None:
        top = torch.empty(top_shape, dtype=e.dtype, device=x.device)
    _expect(top, top_shape, "top")
    _expect(bias, (shape.K,), "bias")
    dt = e.dtype
    capi._call(_symbol("forward", e, route), C.byref(shape), capi._ptr(x, "x", dtype=dt),
               capi._ptr(weight, "weight", dtype=dt), capi._ptr(bias, "bias", True, dt), capi._ptr(top, "top", dtype=dt),
               None, 0)
    return top


def _conv_backward(e, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, stride, pad, group, ws, route):
    shape, top_shape = _shape_of(x, weight, stride, pad, group)
    _expect(top_diff, top_shape, "top_diff")
    _expect(bottom_diff, x.shape, "bottom_diff")
    _expect(weight_diff, weight.shape, "weight_diff")
    _expect(bias_diff, (shape.K,), "bias_diff")
    if bottom_diff is None and weight_diff is None and bias_diff is None:
        raise capi.MMSArgumentError("Convolution backward: none of bottom_diff, weight_diff, bias_diff was given")
    dt = e.dtype
    need = 0
    if weight_diff is not None or bias_diff is not None:
        need = getattr(lib(), "mms_conv_workspace_bytes" + e.query)(C.byref(shape))
    wsp, wsb = capi._scratch(ws, need, x.device)
    capi._call(_symbol("backward", e, route), C.byref(shape), capi._ptr(x, "x", dtype=dt),
               capi._ptr(weight, "weight", dtype=dt), capi._ptr(top_diff, "top_diff", dtype=dt),
               capi._ptr(bottom_diff, "bottom_diff", True, dt), capi._ptr(weight_diff, "weight_diff", True, dt),
               capi._ptr(bias_diff, "bias_diff", True, dt), wsp, wsb)


def conv_forward(x, weight, bias=None, top=None, *, stride=1, pad=0, group=1, ws=None, route="auto"):
    """Convolution forward (include/mms_conv.h: mms_conv_forward_f32).  x (N, C, H, W), weight (K, C/group, kh, kw),
    bias (K) or None (bias_term false); top (N, K, OH, OW) is written and returned (allocated when None).  stride and
    pad: one int or (h, w).  route: "auto" (mms_conv_route decides) or "generic" (the direct kernels at every shape,
    mms_conv_forward_generic_f32).  The forward needs no workspace; `ws` is accepted for symmetry."""
    return _conv_forward(capi._F32, x, weight, bias, top, stride, pad, group, route)


def conv_forward_f64(x, weight, bias=None, top=None, *, stride=1, pad=0, group=1, ws=None, route="auto"):
    return _conv_forward(capi._F64, x, weight, bias, top, stride, pad, group, route)


def conv_backward(x, weight, top_diff, bottom_diff=None, weight_diff=None, bias_diff=None, *, stride=1, pad=0, group=1,
                  ws=None, route="auto"):
    """Convolution backward (mms_conv_backward_f32).  bottom_diff is OVERWRITTEN; weight_diff and bias_diff are
    ACCUMULATED INTO (zero them for a fresh gradient).  Each of the three may be None (skipped, untouched); at least one
    must be given."""
    _conv_backward(capi._F32, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, stride, pad, group, ws, route)


def conv_backward_f64(x, weight, top_diff, bottom_diff=None, weight_diff=None, bias_diff=None, *, stride=1, pad=0,
                      group=1, ws=None, route="auto"):
    _conv_backward(capi._F64, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, stride, pad, group, ws, route)
