"""ctypes binding of the BN -> MaxPool -> TanH calls of libmms_hip.so (include/mms_bn_maxpool.h) for torch device
tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Arguments follow capi's bn_pool_tanh_* wrappers -- the backward also takes `shift`, which the mask is
made from.  Errors are capi's: a library error code goes through `capi.check`.  The stream is torch's current one.
The binding itself is _pooled.py's, shared with capi's AvePool calls.
"""
import ctypes as C

from . import _pooled, capi

_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_QUERY = (_sz, [_i] * 6)

_SIGNATURES = {
    "mms_bn_maxpool_tanh_workspace_bytes": _QUERY,
    "mms_bn_maxpool_tanh_forward_f32": (_i, [_i] * 7 + [C.c_float] + [_vp] * 10 + [_sz, _vp]),
    "mms_bn_maxpool_tanh_backward_f32": (_i, [_i] * 6 + [_vp] * 12 + [_sz, _vp]),
    "mms_bn_maxpool_tanh_workspace_bytes_f64": _QUERY,
    "mms_bn_maxpool_tanh_forward_f64": (_i, [_i] * 7 + [C.c_double] + [_vp] * 10 + [_sz, _vp]),
    "mms_bn_maxpool_tanh_backward_f64": (_i, [_i] * 6 + [_vp] * 12 + [_sz, _vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_bn_maxpool_tanh_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


_FAMILY = _pooled.Family("mms_bn_maxpool_tanh_", "BN + pooling", lib, shift=True)


def bn_maxpool_tanh_workspace_bytes(N, C, H, W, kh, kw):
    """mms_bn_pool_tanh_workspace_bytes' figure: 0 where one workgroup per channel serves."""
    return _pooled.bn_pool_workspace_bytes(_FAMILY, capi._F32, N, C, H, W, kh, kw)


def bn_maxpool_tanh_workspace_bytes_f64(N, C, H, W, kh, kw):
    return _pooled.bn_pool_workspace_bytes(_FAMILY, capi._F64, N, C, H, W, kh, kw)


def bn_maxpool_tanh_forward(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                            phase=0, bn_memory=0.9, ws=None):
    """BN -> MaxPool(kernel = stride, windows tile the map) -> TanH (include/mms_bn_maxpool.h:
    mms_bn_maxpool_tanh_forward_f32).  x (N, C, H, W); kernel k or (kh, kw); top, save_pool (N, C, H/kh, W/kw); the
    other six C floats.  phase as in capi.bn_forward.  save_pool, save_mean, save_std and top are what
    bn_maxpool_tanh_backward needs."""
    _pooled.bn_pool_forward(_FAMILY, capi._F32, x, kernel, scale, shift, running_mean, running_var, top, save_pool,
                            save_mean, save_std, phase, bn_memory, ws)


def bn_maxpool_tanh_forward_f64(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean,
                                save_std, phase=0, bn_memory=0.9, ws=None):
    _pooled.bn_pool_forward(_FAMILY, capi._F64, x, kernel, scale, shift, running_mean, running_var, top, save_pool,
                            save_mean, save_std, phase, bn_memory, ws)


def bn_maxpool_tanh_backward(x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std, bottom_diff=None,
                             scale_diff=None, shift_diff=None, ws=None):
    """Each of bottom_diff (N, C, H, W), scale_diff, shift_diff (C) may be None (skipped); those given are overwritten.
    scale and shift are the forward's."""
    _pooled.bn_pool_backward(_FAMILY, capi._F32, x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                             bottom_diff, scale_diff, shift_diff, ws)


def bn_maxpool_tanh_backward_f64(x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                                 bottom_diff=None, scale_diff=None, shift_diff=None, ws=None):
    _pooled.bn_pool_backward(_FAMILY, capi._F64, x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                             bottom_diff, scale_diff, shift_diff, ws)
