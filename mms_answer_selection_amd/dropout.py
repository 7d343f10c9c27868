"""ctypes binding of the Dropout calls of libmms_hip.so (include/mms_dropout.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.  The element
type is the tensor's: float32 tensors go to the _f32 calls, float64 tensors to the _f64 calls.

    y = dropout_forward(x, 0.1, seed, sequence=it)             # no mask is kept ...
    dx = dropout_backward(dy, 0.1, seed, sequence=it)          # ... the backward regenerates it
    mask = dropout_mask((N, H), 0.5, seed, sequence=it)        # 0 / 1 int32 words: head.head_forward's `mask`
"""
import ctypes as C
import operator

import torch

from . import capi

TRAIN, TEST = 0, 1                         # include/mms_dropout.h: MMS_DROPOUT_TRAIN / _TEST
THREADS, MAX_BLOCKS, GROUPS_PER_TRIP = 256, 2048, 2   # MMS_DROPOUT_THREADS / _MAX_BLOCKS / _GROUPS_PER_TRIP

_vp, _i, _ll, _u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_ulonglong


def _apply(scalar):
    return (_i, [_vp, _vp, _ll, scalar, _i, _u64, _u64, _u64, _vp])


def _mask(scalar):
    return (_i, [_vp, _ll, scalar, _u64, _u64, _u64, _vp])


_SIGNATURES = {
    "mms_dropout_threshold_f32": (_i, [C.c_float, C.POINTER(C.c_uint), C.POINTER(C.c_float)]),
    "mms_dropout_threshold_f64": (_i, [C.c_double, C.POINTER(C.c_uint), C.POINTER(C.c_double)]),
    "mms_dropout_forward_f32": _apply(C.c_float),
    "mms_dropout_forward_f64": _apply(C.c_double),
    "mms_dropout_backward_f32": _apply(C.c_float),
    "mms_dropout_backward_f64": _apply(C.c_double),
    "mms_dropout_mask_u32": _mask(C.c_float),
    "mms_dropout_mask_u32_f64": _mask(C.c_double),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_dropout_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _elem(dtype):
    for e in (capi._F32, capi._F64):
        if e.dtype == dtype:
            return e
    raise capi.MMSArgumentError("Dropout: float32 or float64, got %s" % (dtype,))


def _u64_arg(v, name):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise capi.MMSArgumentError("Dropout: %s must fit 64 unsigned bits, got %d" % (name, v))
    return v


def dropout_threshold(ratio, dtype=torch.float32):
    """(thr, scale) the calls compute from `ratio` in `dtype` (mms_dropout_threshold_f32 / _f64): keep is word > thr.
    Host only."""
    e = _elem(dtype)
    scalar = C.c_float if e.suffix == "f32" else C.c_double
    thr, scale = C.c_uint(0), scalar(0)
    capi.check(getattr(lib(), "mms_dropout_threshold_" + e.suffix)(float(ratio), C.byref(thr), C.byref(scale)),
               "mms_dropout_threshold_" + e.suffix)
    return thr.value, scale.value


def _dropout(stem, x, ratio, seed, sequence, offset, train, out):
    if not isinstance(x, torch.Tensor):
        raise capi.MMSArgumentError("Dropout: a tensor is required, got %r" % type(x).__name__)
    e = _elem(x.dtype)
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape:
        raise capi.MMSArgumentError("Dropout: out must be a tensor of x's shape %s" % (tuple(x.shape),))
    words = (_u64_arg(seed, "seed"), _u64_arg(sequence, "sequence"), _u64_arg(offset, "offset"))
    lib()
    capi._call("mms_dropout_%s_%s" % (stem, e.suffix), capi._ptr(x, "x", dtype=e.dtype),
               capi._ptr(out, "out", dtype=e.dtype), x.numel(), float(ratio), TRAIN if train else TEST, *words)
    return out


def dropout_forward(x, ratio, seed, sequence, offset=0, train=True, out=None):
    """y = (x * keep) * scale (mms_dropout_forward_f32 / _f64 by x's dtype) -> out, allocated when None; out may be x
    (in place).  keep of element i is a function of (seed, sequence, offset + i) alone; train=False is the TEST phase,
    a copy.  The host picks `sequence`, one per (layer, iteration); a shard of a larger blob passes as `offset` the
    number of elements in front of it."""
    return _dropout("forward", x, ratio, seed, sequence, offset, train, out)


def dropout_backward(dy, ratio, seed, sequence, offset=0, train=True, out=None):
    """dx = (dy * keep) * scale with the forward's (ratio, seed, sequence, offset): the mask is regenerated."""
    return _dropout("backward", dy, ratio, seed, sequence, offset, train, out)


def dropout_mask(count_or_shape, ratio, seed, sequence, offset=0, dtype=torch.float32, device=None, out=None):
    """keep as 0 / 1 words, int32 (mms_dropout_mask_u32; dtype=torch.float64: its _f64 twin, whose threshold is
    computed in double) -> out, allocated with the given count or shape on `device` (default: the current GPU) when
    None.  This is Dropout's rand_vec_ as head.head_forward / head_backward take it."""
    e = _elem(dtype)
    try:
        shape = (operator.index(count_or_shape),)                   # a Python or numpy integer: a count
    except TypeError:
        try:
            shape = tuple(operator.index(v) for v in count_or_shape)
        except TypeError:
            raise capi.MMSArgumentError("Dropout: a count or a shape of integers, got %r" % (count_or_shape,))
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=device if device is not None else "cuda")
    elif not isinstance(out, torch.Tensor) or out.numel() != torch.Size(shape).numel():
        raise capi.MMSArgumentError("Dropout: out must be a tensor of %s elements" % (shape,))
    words = (_u64_arg(seed, "seed"), _u64_arg(sequence, "sequence"), _u64_arg(offset, "offset"))
    lib()
    capi._call("mms_dropout_mask_u32" + e.query, capi._ptr(out, "mask", dtype=torch.int32), out.numel(), float(ratio),
               *words)
    return out
