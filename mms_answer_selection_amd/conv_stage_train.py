"""ctypes binding of the TRAIN-phase Convolution -> BN -> AvePool / MaxPool -> TanH stage of libmms_hip.so
(include/mms_conv_stage_train.h) for torch device tensors: the forward as one call and the backward as one call.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`, `conv` or the TEST-phase stage modules.  Errors are capi's: a refusal of this module's own checks raises
`capi.MMSArgumentError` before the library is called, a library error code goes through `capi.check`.  The stream is
torch's current one.
"""
import collections
import ctypes as C

import torch

from . import capi, conv

POOL_AVE, POOL_MAX = 0, 1                                      # include/mms_conv_stage_train.h: MMS_STAGE_POOL_*
ROUTE_NONE, ROUTE_SEQUENCE, ROUTE_FUSED = -1, 0, 1             # MMS_CONV_STAGE_TRAIN_ROUTE_*
_PREFIX = "mms_conv_stage_train_"
_LABEL = "Conv stage (TRAIN)"


def _signatures():
    sp, vp, i, sz = C.POINTER(conv.ConvShape), C.c_void_p, C.c_int, C.c_size_t
    query = (sz, [sp, i, i, i])
    fwd = lambda real: (i, [sp, i, i, i, real] + [vp] * 13 + [sz, vp])             # noqa: E731
    bwd = (i, [sp, i, i, i] + [vp] * 16 + [sz, vp])
    return {
        _PREFIX + "route": (i, [sp, i, i, i]),
        _PREFIX + "workspace_bytes": query,
        _PREFIX + "workspace_bytes_f64": query,
        _PREFIX + "sequence_workspace_bytes": query,
        _PREFIX + "fused_workspace_bytes": query,
        _PREFIX + "forward_f32": fwd(C.c_float),
        _PREFIX + "forward_f64": fwd(C.c_double),
        _PREFIX + "forward_sequence_f32": fwd(C.c_float),
        _PREFIX + "forward_fused_f32": fwd(C.c_float),
        _PREFIX + "backward_f32": bwd,
        _PREFIX + "backward_f64": bwd,
    }


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

Saved = collections.namedtuple("Saved", "y top save_pool save_mean save_std")


def lib():
    """capi.lib(), with the mms_conv_stage_train_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def _pool_method(method):
    if method in ("ave", POOL_AVE):
        return POOL_AVE
    if method in ("max", POOL_MAX):
        return POOL_MAX
    raise capi.MMSArgumentError("%s: method must be 'ave' or 'max', got %r" % (_LABEL, method))


def _query(e, route):
    if route == "auto":
        return _PREFIX + "workspace_bytes" + e.query
    if route == "sequence":
        return _PREFIX + ("workspace_bytes_f64" if e.suffix == "f64" else "sequence_workspace_bytes")
    if route == "fused" and e.suffix == "f32":
        return _PREFIX + "fused_workspace_bytes"
    raise capi.MMSArgumentError("%s: route must be 'auto', 'sequence' or (float) 'fused', got %r" % (_LABEL, route))


def conv_stage_train_route(shape, pool, method):
    """ROUTE_FUSED or ROUTE_SEQUENCE of conv_stage_train_forward for a ConvShape (conv.conv_shape), a pooling window
    (one int or (ph, pw)) and a pooling method ('ave' / 'max'); ROUTE_NONE for what the calls refuse."""
    ph, pw = conv._pair(pool, "pool")
    return lib().mms_conv_stage_train_route(C.byref(shape), ph, pw, _pool_method(method))


def conv_stage_train_route_f64(shape, pool, method):
    """The double call has one route: ROUTE_SEQUENCE wherever conv_stage_train_route does not say ROUTE_NONE."""
    return ROUTE_NONE if conv_stage_train_route(shape, pool, method) == ROUTE_NONE else ROUTE_SEQUENCE


def _bytes(e, shape, pool, method, route):
    ph, pw = conv._pair(pool, "pool")
    return getattr(lib(), _query(e, route))(C.byref(shape), ph, pw, _pool_method(method))


def conv_stage_train_workspace_bytes(shape, pool, method, route="auto"):
    """Bytes that cover the forward on `route` and the backward of one step (mms_conv_stage_train_workspace_bytes,
    _sequence_workspace_bytes, _fused_workspace_bytes)."""
    return _bytes(capi._F32, shape, pool, method, route)


def conv_stage_train_workspace_bytes_f64(shape, pool, method, route="auto"):
    return _bytes(capi._F64, shape, pool, method, route)


def _geometry(x, weight, pool, stride, pad, group):
    ph, pw = conv._pair(pool, "pool")
    shape, (N, K, OH, OW) = conv._shape_of(x, weight, stride, pad, group)
    if ph < 1 or pw < 1 or OH % ph or OW % pw:
        raise capi.MMSArgumentError("%s: %d x %d windows do not tile the convolution's %d x %d map"
                                    % (_LABEL, ph, pw, OH, OW))
    return shape, ph, pw, (N, K, OH, OW), (N, K, OH // ph, OW // pw)


_expect = conv._expect


def _forward(e, x, weight, bias, pool, method, scale, shift, running_mean, running_var, y, top, save_pool, save_mean,
             save_std, bn_memory, stride, pad, group, ws, route):
    lib()                                          # the signatures are on the handle before capi._call uses it
    m = _pool_method(method)
    query = _query(e, route)                       # the route's name is judged first
    shape, ph, pw, full, pooled = _geometry(x, weight, pool, stride, pad, group)
    K, dt = full[1], e.dtype
    new = lambda s: torch.empty(s, dtype=dt, device=x.device)                      # noqa: E731
    y = new(full) if y is None else y
    top = new(pooled) if top is None else top
    save_pool = new(pooled) if save_pool is None else save_pool
    save_mean = new((K,)) if save_mean is None else save_mean
    save_std = new((K,)) if save_std is None else save_std
    _expect(y, full, "y")
    _expect(top, pooled, "top")
    _expect(save_pool, pooled, "save_pool")
    for name, t in (("bias", bias), ("scale", scale), ("shift", shift), ("running_mean", running_mean),
                    ("running_var", running_var), ("save_mean", save_mean), ("save_std", save_std)):
        _expect(t, (K,), name)
    p = capi._ptr
    wsp, wsb = capi._scratch(ws, getattr(lib(), query)(C.byref(shape), ph, pw, m), x.device)
    symbol = _PREFIX + ("forward_" + e.suffix if route == "auto" or e.suffix == "f64" else "forward_%s_f32" % route)
    capi._call(symbol, C.byref(shape), ph, pw, m, float(bn_memory), p(x, "x", dtype=dt), p(weight, "weight", dtype=dt),
               p(bias, "bias", True, dt), p(scale, "scale", dtype=dt), p(shift, "shift", dtype=dt),
               p(running_mean, "running_mean", dtype=dt), p(running_var, "running_var", dtype=dt), p(y, "y", dtype=dt),
               p(top, "top", dtype=dt), p(save_pool, "save_pool", dtype=dt), p(save_mean, "save_mean", dtype=dt),
               p(save_std, "save_std", dtype=dt), wsp, wsb)
    return Saved(y, top, save_pool, save_mean, save_std)


def _backward(e, x, weight, pool, method, y, top, top_diff, save_pool, scale, shift, save_mean, save_std, bottom_diff,
              weight_diff, bias_diff, scale_diff, shift_diff, stride, pad, group, ws):
    lib()
    m = _pool_method(method)
    shape, ph, pw, full, pooled = _geometry(x, weight, pool, stride, pad, group)
    K, dt = full[1], e.dtype
    _expect(y, full, "y")
    for name, t in (("top", top), ("top_diff", top_diff), ("save_pool", save_pool)):
        _expect(t, pooled, name)
    for name, t in (("scale", scale), ("shift", shift), ("save_mean", save_mean), ("save_std", save_std),
                    ("bias_diff", bias_diff), ("scale_diff", scale_diff), ("shift_diff", shift_diff)):
        _expect(t, (K,), name)
    _expect(bottom_diff, x.shape, "bottom_diff")
    _expect(weight_diff, weight.shape, "weight_diff")
    if all(t is None for t in (bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff)):
        raise capi.MMSArgumentError("%s backward: no output was given" % _LABEL)
    p = capi._ptr
    wsp, wsb = capi._scratch(ws, getattr(lib(), _query(e, "auto"))(C.byref(shape), ph, pw, m), x.device)
    capi._call(_PREFIX + "backward_" + e.suffix, C.byref(shape), ph, pw, m, p(x, "x", dtype=dt),
               p(weight, "weight", dtype=dt), p(y, "y", dtype=dt), p(top, "top", dtype=dt),
               p(top_diff, "top_diff", dtype=dt), p(save_pool, "save_pool", dtype=dt), p(scale, "scale", dtype=dt),
               p(shift, "shift", m == POOL_AVE, dt), p(save_mean, "save_mean", dtype=dt),
               p(save_std, "save_std", dtype=dt), p(bottom_diff, "bottom_diff", True, dt),
               p(weight_diff, "weight_diff", True, dt), p(bias_diff, "bias_diff", True, dt),
               p(scale_diff, "scale_diff", True, dt), p(shift_diff, "shift_diff", True, dt), wsp, wsb)


def conv_stage_train_forward(x, weight, bias, pool, method, scale, shift, running_mean, running_var, y=None, top=None,
                             save_pool=None, save_mean=None, save_std=None, *, bn_memory=0.9, stride=1, pad=0, group=1,
                             ws=None, route="auto"):
    """TRAIN-phase Convolution -> BN -> Pool(method 'ave' or 'max'; pool = stride, windows tile the map) -> TanH
    (include/mms_conv_stage_train.h: mms_conv_stage_train_forward_f32).  x (N, C, H, W), weight (K, C/group, kh, kw),
    bias (K) or None; scale, shift (K); running_mean, running_var (K) are updated in place with `bn_memory`.  Writes
    and returns Saved(y (N, K, OH, OW), top, save_pool (N, K, OH/ph, OW/pw), save_mean, save_std (K)), each allocated
    when None: what conv_stage_train_backward reads.  route: "auto" (mms_conv_stage_train_route decides), "sequence"
    (the two public calls at every shape) or "fused" (the two launches wherever they reach, an error elsewhere)."""
    return _forward(capi._F32, x, weight, bias, pool, method, scale, shift, running_mean, running_var, y, top,
                    save_pool, save_mean, save_std, bn_memory, stride, pad, group, ws, route)


def conv_stage_train_forward_f64(x, weight, bias, pool, method, scale, shift, running_mean, running_var, y=None,
                                 top=None, save_pool=None, save_mean=None, save_std=None, *, bn_memory=0.9, stride=1,
                                 pad=0, group=1, ws=None, route="auto"):
    return _forward(capi._F64, x, weight, bias, pool, method, scale, shift, running_mean, running_var, y, top,
                    save_pool, save_mean, save_std, bn_memory, stride, pad, group, ws, route)


def conv_stage_train_backward(x, weight, pool, method, y, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                              bottom_diff=None, weight_diff=None, bias_diff=None, scale_diff=None, shift_diff=None, *,
                              stride=1, pad=0, group=1, ws=None):
    """The stage's backward (mms_conv_stage_train_backward_f32) from what the forward left.  Each output may be None
    (skipped), at least one is required: bottom_diff, scale_diff and shift_diff are overwritten, weight_diff and
    bias_diff are accumulated into.  shift may be None for 'ave'."""
    _backward(capi._F32, x, weight, pool, method, y, top, top_diff, save_pool, scale, shift, save_mean, save_std,
              bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, stride, pad, group, ws)


def conv_stage_train_backward_f64(x, weight, pool, method, y, top, top_diff, save_pool, scale, shift, save_mean,
                                  save_std, bottom_diff=None, weight_diff=None, bias_diff=None, scale_diff=None,
                                  shift_diff=None, *, stride=1, pad=0, group=1, ws=None):
    _backward(capi._F64, x, weight, pool, method, y, top, top_diff, save_pool, scale, shift, save_mean, save_std,
              bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, stride, pad, group, ws)
