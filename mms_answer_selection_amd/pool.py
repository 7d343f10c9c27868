"""ctypes binding of the Pooling and TanH calls of libmms_hip.so (include/mms_pool.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.  The element
type is the tensor's: float32 tensors go to the _f32 calls, float64 tensors to the _f64 calls.

    top, mask = pool_forward(x, 'max', 3, stride=2, pad=1, mask=True)      # max_idx_; top_mask=True: the second top
    dx = pool_backward(dtop, x.shape, 'max', 3, stride=2, pad=1, mask=mask)
    y = tanh_forward(top)                                                  # out=top: in place
    dtop = tanh_backward(y, dy)
"""
import ctypes as C

import torch

from . import capi

AVE, MAX, STOCHASTIC = 0, 1, 2             # include/mms_pool.h: MMS_POOL_AVE / _MAX / _STOCHASTIC
METHODS = {"ave": AVE, "max": MAX}


class PoolShape(C.Structure):
    """mms_pool_shape"""
    _fields_ = [(n, C.c_int) for n in ("N", "C", "H", "W", "kernel_h", "kernel_w", "stride_h", "stride_w", "pad_h",
                                       "pad_w", "method")]


_vp, _i, _ll, _sp = C.c_void_p, C.c_int, C.c_longlong, C.POINTER(PoolShape)
_FWD = (_i, [_sp, _vp, _vp, _vp, _vp, _vp])
_BWD = (_i, [_sp, _vp, _vp, _vp, _vp, _vp])

_SIGNATURES = {
    "mms_pool_output_dims": (_i, [_sp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mms_pool_forward_f32": _FWD,
    "mms_pool_forward_f64": _FWD,
    "mms_pool_backward_f32": _BWD,
    "mms_pool_backward_f64": _BWD,
    "mms_tanh_forward_f32": (_i, [_ll, _vp, _vp, _vp]),
    "mms_tanh_forward_f64": (_i, [_ll, _vp, _vp, _vp]),
    "mms_tanh_backward_f32": (_i, [_ll, _vp, _vp, _vp, _vp]),
    "mms_tanh_backward_f64": (_i, [_ll, _vp, _vp, _vp, _vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_pool_* / mms_tanh_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _elem(dtype, label):
    for e in (capi._F32, capi._F64):
        if e.dtype == dtype:
            return e
    raise capi.MMSArgumentError("%s: float32 or float64, got %s" % (label, dtype))


def _pair(v, name):
    try:
        a, b = (v, v) if isinstance(v, int) else v
        return int(a), int(b)
    except (TypeError, ValueError):
        raise capi.MMSArgumentError("Pooling: %s is an integer or a pair of integers, got %r" % (name, v))


def pool_shape(dims, method, kernel, stride=1, pad=0):
    """The mms_pool_shape of a (N, C, H, W) blob: method 'ave' or 'max' (or one of the header's integers); kernel,
    stride and pad each k or (k_h, k_w).  The default stride is 1, as the reference's is."""
    if len(dims) != 4:
        raise capi.MMSArgumentError("Pooling: a blob is (N, C, H, W), got %s" % (tuple(dims),))
    if isinstance(method, str):
        if method not in METHODS:
            raise capi.MMSArgumentError("Pooling: method is 'ave' or 'max', got %r" % (method,))
        method = METHODS[method]
    return PoolShape(*(int(d) for d in dims), *_pair(kernel, "kernel"), *_pair(stride, "stride"), *_pair(pad, "pad"),
                     int(method))


def pool_output_dims(dims, method, kernel, stride=1, pad=0):
    """(PH, PW) of the shape (mms_pool_output_dims).  Host only."""
    shape, ph, pw = pool_shape(dims, method, kernel, stride, pad), C.c_int(0), C.c_int(0)
    capi.check(lib().mms_pool_output_dims(C.byref(shape), C.byref(ph), C.byref(pw)), "mms_pool_output_dims")
    return ph.value, pw.value


def _tensor(t, label, name):
    if not isinstance(t, torch.Tensor):
        raise capi.MMSArgumentError("%s: %s must be a tensor, got %r" % (label, name, type(t).__name__))
    return t


def pool_forward(x, method, kernel, stride=1, pad=0, mask=False, top_mask=False, out=None):
    """top of mms_pool_forward_f32 / _f64 by x's dtype, x (N, C, H, W) -> out, allocated when None.  mask / top_mask:
    True allocates the array (int32 / x's dtype), a tensor is written into, False or None passes NULL.  Returns top,
    followed by mask and / or top_mask where they were asked for.  AVE writes neither."""
    x = _tensor(x, "Pooling", "x")
    e = _elem(x.dtype, "Pooling")
    shape = pool_shape(tuple(x.shape), method, kernel, stride, pad)
    pooled = tuple(x.shape[:2]) + pool_output_dims(tuple(x.shape), method, kernel, stride, pad)
    if out is None:
        out = torch.empty(pooled, dtype=e.dtype, device=x.device)
    capi._expect("Pooling", _tensor(out, "Pooling", "out"), pooled, "out")
    extra = []
    for name, want, dt in (("mask", mask, torch.int32), ("top_mask", top_mask, e.dtype)):
        if want is True:
            want = torch.empty(pooled, dtype=dt, device=x.device)
        elif want is False or want is None:
            want = None
        else:
            capi._expect("Pooling", _tensor(want, "Pooling", name), pooled, name)
        extra.append(want)
    capi._call("mms_pool_forward_" + e.suffix, C.byref(shape), capi._ptr(x, "x", dtype=e.dtype),
               capi._ptr(out, "out", dtype=e.dtype), capi._ptr(extra[0], "mask", True, torch.int32),
               capi._ptr(extra[1], "top_mask", True, e.dtype))
    res = (out,) + tuple(t for t in extra if t is not None)
    return res[0] if len(res) == 1 else res


def pool_backward(top_diff, dims, method, kernel, stride=1, pad=0, mask=None, top_mask=None, out=None):
    """bottom_diff (dims = (N, C, H, W)) of mms_pool_backward_f32 / _f64 by top_diff's dtype -> out, allocated when
    None and overwritten.  MAX needs the forward's mask or top_mask; with both, mask is read."""
    top_diff = _tensor(top_diff, "Pooling", "top_diff")
    e = _elem(top_diff.dtype, "Pooling")
    dims = tuple(int(d) for d in dims)
    shape = pool_shape(dims, method, kernel, stride, pad)
    pooled = dims[:2] + pool_output_dims(dims, method, kernel, stride, pad)
    capi._expect("Pooling", top_diff, pooled, "top_diff")
    capi._expect("Pooling", mask, pooled, "mask")
    capi._expect("Pooling", top_mask, pooled, "top_mask")
    if out is None:
        out = torch.empty(dims, dtype=e.dtype, device=top_diff.device)
    capi._expect("Pooling", _tensor(out, "Pooling", "out"), dims, "out")
    capi._call("mms_pool_backward_" + e.suffix, C.byref(shape), capi._ptr(top_diff, "top_diff", dtype=e.dtype),
               capi._ptr(mask, "mask", True, torch.int32), capi._ptr(top_mask, "top_mask", True, e.dtype),
               capi._ptr(out, "out", dtype=e.dtype))
    return out


def _like(t, out, label):
    if out is None:
        return torch.empty_like(t, memory_format=torch.contiguous_format)
    if not isinstance(out, torch.Tensor) or out.shape != t.shape:
        raise capi.MMSArgumentError("%s: out must be a tensor of shape %s" % (label, tuple(t.shape)))
    return out


def tanh_forward(x, out=None):
    """top = tanh(x) (mms_tanh_forward_f32 / _f64 by x's dtype) -> out, allocated when None; out may be x."""
    x = _tensor(x, "TanH", "x")
    e = _elem(x.dtype, "TanH")
    out = _like(x, out, "TanH")
    lib()
    capi._call("mms_tanh_forward_" + e.suffix, x.numel(), capi._ptr(x, "x", dtype=e.dtype),
               capi._ptr(out, "out", dtype=e.dtype))
    return out


def tanh_backward(top, top_diff, out=None):
    """bottom_diff = top_diff * (1 - top * top) (mms_tanh_backward_f32 / _f64) -> out, allocated when None; out may be
    top_diff."""
    top, top_diff = _tensor(top, "TanH", "top"), _tensor(top_diff, "TanH", "top_diff")
    e = _elem(top.dtype, "TanH")
    if top_diff.shape != top.shape:
        raise capi.MMSArgumentError("TanH: top_diff must have top's shape %s" % (tuple(top.shape),))
    out = _like(top_diff, out, "TanH")
    lib()
    capi._call("mms_tanh_backward_" + e.suffix, top.numel(), capi._ptr(top, "top", dtype=e.dtype),
               capi._ptr(top_diff, "top_diff", dtype=e.dtype), capi._ptr(out, "out", dtype=e.dtype))
    return out


# The _f64 forms: the element type is the tensor's, so these are the same functions under the names the other families use.
pool_forward_f64, pool_backward_f64 = pool_forward, pool_backward
tanh_forward_f64, tanh_backward_f64 = tanh_forward, tanh_backward
