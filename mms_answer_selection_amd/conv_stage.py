"""ctypes binding of the TEST-phase Convolution -> BN -> AvePool -> TanH stage of libmms_hip.so
(include/mms_conv_stage.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi` or to `conv`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError`
before the library is called, a library error code goes through `capi.check`.  The stream is torch's current one.
The binding itself is _pooled.py's, shared with the MaxPool form of the stage.
"""
from . import _pooled, capi

ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = -1, 0, 1             # include/mms_conv_stage.h: MMS_CONV_STAGE_ROUTE_*

_SIGNATURES = _pooled.conv_stage_signatures("mms_conv_stage_")
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_conv_stage_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


_FAMILY = _pooled.Family("mms_conv_stage_", "Conv stage", lib)


def conv_stage_route(shape, pool):
    """ROUTE_FUSED or ROUTE_SEQUENCE of conv_stage_forward for a ConvShape (conv.conv_shape) and a pooling window (one
    int or (ph, pw)); ROUTE_NONE for what the calls refuse (mms_conv_stage_route)."""
    return _pooled.conv_stage_route(_FAMILY, shape, pool)


def conv_stage_route_f64(shape, pool):
    """The double call has one route: ROUTE_SEQUENCE wherever conv_stage_route does not say ROUTE_NONE."""
    return ROUTE_NONE if conv_stage_route(shape, pool) == ROUTE_NONE else ROUTE_SEQUENCE


def conv_stage_workspace_bytes(shape, pool, route="auto"):
    """Bytes conv_stage_forward needs: 0 on ROUTE_FUSED; on ROUTE_SEQUENCE (and with route="sequence" at every shape)
    the convolution's map, 2 K elements and a save_pool (mms_conv_stage_workspace_bytes); 0 with route="fused"."""
    return _pooled.conv_stage_workspace_bytes(_FAMILY, capi._F32, shape, pool, route)


def conv_stage_workspace_bytes_f64(shape, pool, route="auto"):
    return _pooled.conv_stage_workspace_bytes(_FAMILY, capi._F64, shape, pool, route)


def conv_stage_forward(x, weight, bias, pool, mean, var, scale, shift, top=None, save_pool=None, *, stride=1, pad=0,
                       group=1, ws=None, route="auto"):
    """TEST-phase Convolution -> BN -> AvePool(pool = stride, windows tile the map) -> TanH
    (include/mms_conv_stage.h: mms_conv_stage_forward_f32).  x (N, C, H, W), weight (K, C/group, kh, kw), bias (K) or
    None; mean, var, scale, shift (K): BN's running blobs and parameters; top (N, K, OH/ph, OW/pw) is written and
    returned (allocated when None); save_pool, the same shape, receives the pooled normalised map when given.  route:
    "auto" (mms_conv_stage_route decides), "sequence" (the two calls at every shape,
    mms_conv_stage_forward_sequence_f32) or "fused" (the one launch wherever it reaches, an error elsewhere,
    mms_conv_stage_forward_fused_f32)."""
    return _pooled.conv_stage_forward(_FAMILY, capi._F32, x, weight, bias, pool, mean, var, scale, shift, top,
                                      save_pool, stride, pad, group, ws, route)


def conv_stage_forward_f64(x, weight, bias, pool, mean, var, scale, shift, top=None, save_pool=None, *, stride=1, pad=0,
                           group=1, ws=None, route="auto"):
    return _pooled.conv_stage_forward(_FAMILY, capi._F64, x, weight, bias, pool, mean, var, scale, shift, top,
                                      save_pool, stride, pad, group, ws, route)
