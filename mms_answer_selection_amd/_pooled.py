"""The binding of the pooled stages, written once for the AvePool and the MaxPool family of each: BN -> pooling -> TanH
(capi's bn_pool_tanh_*, bn_maxpool.py) and TEST-phase Convolution -> BN -> pooling -> TanH (conv_stage.py,
conv_maxpool_stage.py).  Private: the public functions, their docstrings, the `lib()` that applies a family's
signatures and the EXPORTED_SYMBOLS stay in the module that owns the names, which hands its `Family` to the calls here.
"""
import collections
import ctypes as C

import torch

from . import capi, conv

# prefix: what every entry point of the family starts with.  label: what its error messages start with.  lib: the
# owning module's lib().  shift: the BN-pool backward also takes `shift` (MaxPool makes its mask from it).
Family = collections.namedtuple("Family", "prefix label lib shift", defaults=(False,))


# ---- BN -> pooling -> TanH ---------------------------------------------------------------------------------------
def bn_pool_shape(f, x, kernel):
    """(N, C, H, W, kh, kw) of a 4-D blob and a pooling kernel (k or (kh, kw))."""
    if x.dim() != 4:
        raise capi.MMSArgumentError("%s: x must be (N, C, H, W), got %s" % (f.label, tuple(x.shape)))
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    return tuple(int(d) for d in x.shape) + (int(kh), int(kw))


def bn_pool_workspace_bytes(f, e, *dims):
    return getattr(f.lib(), f.prefix + "workspace_bytes" + e.query)(*dims)


def bn_pool_forward(f, e, x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                    phase, bn_memory, ws):
    dims, dt, p = bn_pool_shape(f, x, kernel), e.dtype, capi._ptr
    wsp, wsb = capi._scratch(ws, bn_pool_workspace_bytes(f, e, *dims), x.device)    # binds the family's signatures
    capi._call(f.prefix + "forward_" + e.suffix, int(phase), *dims, float(bn_memory), p(x, "x", dtype=dt),
               p(scale, "scale", dtype=dt), p(shift, "shift", dtype=dt), p(running_mean, "running_mean", dtype=dt),
               p(running_var, "running_var", dtype=dt), p(top, "top", dtype=dt), p(save_pool, "save_pool", dtype=dt),
               p(save_mean, "save_mean", dtype=dt), p(save_std, "save_std", dtype=dt), wsp, wsb)


def bn_pool_backward(f, e, x, kernel, top, top_diff, save_pool, scale, shift, save_mean, save_std, bottom_diff,
                     scale_diff, shift_diff, ws):
    """`shift` is passed on by the families whose backward takes it and ignored by the others."""
    dims, dt, p = bn_pool_shape(f, x, kernel), e.dtype, capi._ptr
    wsp, wsb = capi._scratch(ws, bn_pool_workspace_bytes(f, e, *dims), x.device)
    capi._call(f.prefix + "backward_" + e.suffix, *dims, p(x, "x", dtype=dt), p(top, "top", dtype=dt),
               p(top_diff, "top_diff", dtype=dt), p(save_pool, "save_pool", dtype=dt), p(scale, "scale", dtype=dt),
               *((p(shift, "shift", dtype=dt),) if f.shift else ()),
               p(save_mean, "save_mean", dtype=dt), p(save_std, "save_std", dtype=dt),
               p(bottom_diff, "bottom_diff", True, dt), p(scale_diff, "scale_diff", True, dt),
               p(shift_diff, "shift_diff", True, dt), wsp, wsb)


# ---- TEST-phase Convolution -> BN -> pooling -> TanH -------------------------------------------------------------
def conv_stage_signatures(prefix):
    """The signature table of a conv-stage family: its header's entry points, in the header's order."""
    sp, vp, i, sz = C.POINTER(conv.ConvShape), C.c_void_p, C.c_int, C.c_size_t
    query = (sz, [sp, i, i])
    fwd = (i, [sp, i, i] + [vp] * 10 + [sz, vp])
    fwd_fused = (i, [sp, i, i] + [vp] * 9 + [vp])                # no workspace
    return {
        prefix + "route": (i, [sp, i, i]),
        prefix + "workspace_bytes": query,
        prefix + "workspace_bytes_f64": query,
        prefix + "sequence_workspace_bytes": query,
        prefix + "forward_f32": fwd,
        prefix + "forward_f64": fwd,
        prefix + "forward_sequence_f32": fwd,
        prefix + "forward_fused_f32": fwd_fused,
    }


def conv_stage_route(f, shape, pool):
    ph, pw = conv._pair(pool, "pool")
    return getattr(f.lib(), f.prefix + "route")(C.byref(shape), ph, pw)


def _query(f, e, route):
    """The name of the workspace query for `route`, None where the route needs none."""
    if route == "auto":
        return f.prefix + "workspace_bytes" + e.query
    if route == "sequence":
        return f.prefix + ("workspace_bytes_f64" if e.suffix == "f64" else "sequence_workspace_bytes")
    if route == "fused" and e.suffix == "f32":
        return None
    raise capi.MMSArgumentError("%s: route must be 'auto', 'sequence' or (float) 'fused', got %r" % (f.label, route))


def _bytes(f, e, route, shape, ph, pw):
    q = _query(f, e, route)
    return getattr(f.lib(), q)(C.byref(shape), ph, pw) if q else 0


def conv_stage_workspace_bytes(f, e, shape, pool, route):
    return _bytes(f, e, route, shape, *conv._pair(pool, "pool"))


def _symbol(f, e, route):
    if route == "auto" or e.suffix == "f64":       # double has the sequence route only, and no entry point of that name
        return f.prefix + "forward_" + e.suffix
    return f.prefix + "forward_%s_f32" % route


def conv_stage_forward(f, e, x, weight, bias, pool, mean, var, scale, shift, top, save_pool, stride, pad, group, ws,
                       route):
    f.lib()                                        # the signatures are on the handle before capi._call uses it
    ph, pw = conv._pair(pool, "pool")
    _query(f, e, route)                            # the route's name is judged first
    shape, (N, K, OH, OW) = conv._shape_of(x, weight, stride, pad, group)
    if ph < 1 or pw < 1 or OH % ph or OW % pw:
        raise capi.MMSArgumentError("%s: %d x %d windows do not tile the convolution's %d x %d map"
                                    % (f.label, ph, pw, OH, OW))
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
        args += capi._scratch(ws, _bytes(f, e, route, shape, ph, pw), x.device)
    capi._call(_symbol(f, e, route), *args)
    return top
