"""ctypes binding of the TEST-phase Convolution -> BN -> MaxPool -> TanH stage of libmms_hip.so
(include/mms_conv_maxpool_stage.h) for torch device tensors: conv_stage.py's calls, name for name, for the MAX form.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`, `conv`, `conv_stage` or `bn_maxpool`.  Errors are capi's: a refusal of this module's own checks raises
`capi.MMSArgumentError` before the library is called, a library error code goes through `capi.check`.  The stream is
torch's current one.
"""
import ctypes as C

import torch

from . import capi, conv

ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = -1, 0, 1     # include/mms_conv_maxpool_stage.h: MMS_CONV_MAXPOOL_STAGE_ROUTE_*

_PREFIX = "mms_conv_maxpool_stage_"
_sp, _vp, _i, _sz = C.POINTER(conv.ConvShape), C.c_void_p, C.c_int, C.c_size_t
_QUERY = (_sz, [_sp, _i, _i])
_FWD = (_i, [_sp, _i, _i] + [_vp] * 10 + [_sz, _vp])
_FWD_FUSED = (_i, [_sp, _i, _i] + [_vp] * 9 + [_vp])           # no workspace

_SIGNATURES = {
    _PREFIX + "route": (_i, [_sp, _i, _i]),
    _PREFIX + "workspace_bytes": _QUERY,
    _PREFIX + "workspace_bytes_f64": _QUERY,
    _PREFIX + "sequence_workspace_bytes": _QUERY,
    _PREFIX + "forward_f32": _FWD,
    _PREFIX + "forward_f64": _FWD,
    _PREFIX + "forward_sequence_f32": _FWD,
    _PREFIX + "forward_fused_f32": _FWD_FUSED,
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_conv_maxpool_stage_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _window(pool):
    return conv._pair(pool, "pool")


def conv_maxpool_stage_route(shape, pool):
    """ROUTE_FUSED or ROUTE_SEQUENCE of conv_maxpool_stage_forward for a ConvShape (conv.conv_shape) and a pooling
    window (one int or (ph, pw)); ROUTE_NONE for what the calls refuse (mms_conv_maxpool_stage_route)."""
    ph, pw = _window(pool)
    return lib().mms_conv_maxpool_stage_route(C.byref(shape), ph, pw)


def conv_maxpool_stage_route_f64(shape, pool):
    """The double call has one route: ROUTE_SEQUENCE wherever conv_maxpool_stage_route does not say ROUTE_NONE."""
    return ROUTE_NONE if conv_maxpool_stage_route(shape, pool) == ROUTE_NONE else ROUTE_SEQUENCE


def _query(e, route):
    """The name of the workspace query for `route`, None where the route needs none."""
    if route == "auto":
        return _PREFIX + "workspace_bytes" + e.query
    if route == "sequence":
        return _PREFIX + ("workspace_bytes_f64" if e.suffix == "f64" else "sequence_workspace_bytes")
    if route == "fused" and e.suffix == "f32":
        return None
    raise capi.MMSArgumentError("Conv MaxPool stage: route must be 'auto', 'sequence' or (float) 'fused', got %r"
                                % (route,))


def _bytes(e, route, shape, ph, pw):
    q = _query(e, route)
    return getattr(lib(), q)(C.byref(shape), ph, pw) if q else 0


def conv_maxpool_stage_workspace_bytes(shape, pool, route="auto"):
    """Bytes conv_maxpool_stage_forward needs: 0 on ROUTE_FUSED; on ROUTE_SEQUENCE (and with route="sequence" at every
    shape) the convolution's map, 2 K elements and a save_pool (mms_conv_maxpool_stage_workspace_bytes); 0 with
    route="fused"."""
    ph, pw = _window(pool)
    return _bytes(capi._F32, route, shape, ph, pw)


def conv_maxpool_stage_workspace_bytes_f64(shape, pool, route="auto"):
    ph, pw = _window(pool)
    return _bytes(capi._F64, route, shape, ph, pw)


def _symbol(e, route):
    if route == "auto" or e.suffix == "f64":       # double has the sequence route only, and no entry point of that name
        return _PREFIX + "forward_" + e.suffix
    return _PREFIX + "forward_%s_f32" % route


def _forward(e, x, weight, bias, pool, mean, var, scale, shift, top, save_pool, stride, pad, group, ws, route):
    lib()                                          # the signatures are on the handle before capi._call uses it
    ph, pw = _window(pool)
    _query(e, route)                               # the route's name is judged first
    shape, (N, K, OH, OW) = conv._shape_of(x, weight, stride, pad, group)
    if ph < 1 or pw < 1 or OH % ph or OW % pw:
        raise capi.MMSArgumentError("Conv MaxPool stage: %d x %d windows do not tile the convolution's %d x %d map"
                                    % (ph, pw, OH, OW))
    pooled = (N, K, OH // ph, OW // pw)
    if top is None:
        top = torch.empty(pooled, dtype=e.dtype, device=x.device)
    conv._expect(top, pooled, "top")
    conv._expect(save_pool, pooled, "save_pool")
    conv._expect(bias, (K,), "bias")
    for name, t in (("mean", mean), ("var", var), ("scale", scale), ("shift", shift)):
        conv._expect(t, (K,), name)
    dt = e.dtype
    args = [C.byref(shape), ph, pw, capi._ptr(x, "x", dtype=dt), capi._ptr(weight, "weight", dtype=dt),
            capi._ptr(bias, "bias", True, dt), capi._ptr(mean, "mean", dtype=dt), capi._ptr(var, "var", dtype=dt),
            capi._ptr(scale, "scale", dtype=dt), capi._ptr(shift, "shift", dtype=dt), capi._ptr(top, "top", dtype=dt),
            capi._ptr(save_pool, "save_pool", True, dt)]
    if route != "fused":
        args += capi._scratch(ws, _bytes(e, route, shape, ph, pw), x.device)
    capi._call(_symbol(e, route), *args)
    return top


def conv_maxpool_stage_forward(x, weight, bias, pool, mean, var, scale, shift, top=None, save_pool=None, *, stride=1,
                               pad=0, group=1, ws=None, route="auto"):
    """TEST-phase Convolution -> BN -> MaxPool(pool = stride, windows tile the map) -> TanH
    (include/mms_conv_maxpool_stage.h: mms_conv_maxpool_stage_forward_f32).  x (N, C, H, W), weight (K, C/group, kh, kw),
    bias (K) or None; mean, var, scale, shift (K): BN's running blobs and parameters; top (N, K, OH/ph, OW/pw) is written
    and returned (allocated when None); save_pool, the same shape, receives the normalised extremum of each window when
    given.  route: "auto" (mms_conv_maxpool_stage_route decides), "sequence" (the two calls at every shape,
    mms_conv_maxpool_stage_forward_sequence_f32) or "fused" (the one launch wherever it reaches, an error elsewhere,
    mms_conv_maxpool_stage_forward_fused_f32)."""
    return _forward(capi._F32, x, weight, bias, pool, mean, var, scale, shift, top, save_pool, stride, pad, group, ws,
                    route)


def conv_maxpool_stage_forward_f64(x, weight, bias, pool, mean, var, scale, shift, top=None, save_pool=None, *,
                                   stride=1, pad=0, group=1, ws=None, route="auto"):
    return _forward(capi._F64, x, weight, bias, pool, mean, var, scale, shift, top, save_pool, stride, pad, group, ws,
                    route)
