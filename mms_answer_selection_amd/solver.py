"""ctypes binding of the solver-update calls of libmms_hip.so (include/mms_solver.h) for torch device tensors.

The calls live in the library `capi.lib()` loads; their signatures are applied here, to that handle, and nothing is
added to `capi`.  Errors are capi's: a refusal of this module's own checks raises `capi.MMSArgumentError` before the
library is called, a library error code goes through `capi.check`.  The stream is torch's current one.

    blobs = solver_blobs([(w, w_diff, hist, hist2, lr_mult, decay_mult), ...])     # once: the addresses do not change
    param = solver_param(ADADELTA, momentum=0.95, delta=5e-7, weight_decay=5e-4, diff_out=DIFF_ZERO)
    solver_step(param, blobs, rate)                                                # after every backward
"""
import ctypes as C

import torch

from . import capi

SGD, ADADELTA = 0, 1                       # include/mms_solver.h: MMS_SOLVER_SGD / _ADADELTA
L2, L1 = 0, 1                              # MMS_SOLVER_L2 / _L1
DIFF_UPDATE, DIFF_ZERO = 0, 1              # MMS_SOLVER_DIFF_UPDATE / _ZERO
CHUNK = 2048                               # MMS_SOLVER_CHUNK
BLOBS_PER_LAUNCH = 32                      # MMS_SOLVER_BLOBS_PER_LAUNCH


class SolverBlob(C.Structure):
    """mms_solver_blob"""
    _fields_ = [("data", C.c_void_p), ("diff", C.c_void_p), ("hist_grad", C.c_void_p), ("hist_update", C.c_void_p),
                ("count", C.c_longlong), ("lr_mult", C.c_float), ("decay_mult", C.c_float)]


class SolverParam(C.Structure):
    """mms_solver_param"""
    _fields_ = [("type", C.c_int), ("regularization", C.c_int), ("iter_size", C.c_int), ("diff_out", C.c_int),
                ("momentum", C.c_float), ("delta", C.c_float), ("weight_decay", C.c_float),
                ("clip_gradients", C.c_float)]


_pp, _bp, _vp, _i, _sz = C.POINTER(SolverParam), C.POINTER(SolverBlob), C.c_void_p, C.c_int, C.c_size_t

_SIGNATURES = {
    "mms_solver_workspace_bytes": (_sz, [_pp, _bp, _i]),
    "mms_solver_workspace_bytes_f64": (_sz, [_pp, _bp, _i]),
    "mms_solver_step_f32": (_i, [_pp, _bp, _i, C.c_float, _vp, _vp, _sz, _vp]),
    "mms_solver_step_f64": (_i, [_pp, _bp, _i, C.c_double, _vp, _vp, _sz, _vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """capi.lib(), with the mms_solver_* signatures applied to it (once)."""
    return capi._bound_lib(_SIGNATURES)


def solver_param(type=ADADELTA, regularization=L2, iter_size=1, diff_out=DIFF_UPDATE, momentum=0.0, delta=1e-8,
                 weight_decay=0.0, clip_gradients=-1.0):
    """An mms_solver_param; the defaults are caffe.proto's (SolverParameter), but for the type."""
    return SolverParam(int(type), int(regularization), int(iter_size), int(diff_out), float(momentum), float(delta),
                       float(weight_decay), float(clip_gradients))


class SolverBlobs:
    """A host array of mms_solver_blob and the tensors it points into (kept alive with it)."""

    def __init__(self, array, array_len, tensors, dtype, device):
        self.array, self.array_len, self.tensors, self.dtype, self.device = array, array_len, tensors, dtype, device

    def __len__(self):
        return self.array_len


def _address(t, name, dtype, device, count):
    if not isinstance(t, torch.Tensor):
        raise capi.MMSArgumentError("Solver: %s must be a tensor, got %r" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise capi.MMSArgumentError("Solver: %s must be %s like the first tensor (got %s)" % (name, dtype, t.dtype))
    if t.device != device or not t.is_cuda:
        raise capi.MMSArgumentError("Solver: %s must live in GPU memory on %s (got %s); there is no CPU path"
                                    % (name, device, t.device))
    if not t.is_contiguous():
        raise capi.MMSArgumentError("Solver: %s must be contiguous" % name)
    if t.numel() != count:
        raise capi.MMSArgumentError("Solver: %s holds %d elements, its data %d" % (name, t.numel(), count))
    return t.data_ptr()


def solver_blobs(entries):
    """[(data, diff, hist_grad, hist_update or None, lr_mult, decay_mult), ...] of torch device tensors, in the order
    of Net::learnable_params() -> SolverBlobs.  All tensors share one dtype (float32 or float64) and one device, are
    contiguous, and the four of a blob hold equally many elements."""
    entries = list(entries)
    array = (SolverBlob * max(1, len(entries)))()
    tensors, dtype, device = [], None, None
    for k, entry in enumerate(entries):
        if len(entry) != 6:
            raise capi.MMSArgumentError("Solver: blob %d is not (data, diff, hist_grad, hist_update, lr_mult, decay_mult)"
                                        % k)
        data, diff, hist, hist2, lr_mult, decay_mult = entry
        if not isinstance(data, torch.Tensor):
            raise capi.MMSArgumentError("Solver: blob %d: data must be a tensor" % k)
        if dtype is None:
            dtype, device = data.dtype, data.device
            if dtype not in (torch.float32, torch.float64):
                raise capi.MMSArgumentError("Solver: float32 or float64 tensors, got %s" % dtype)
        n = data.numel()
        b = array[k]
        b.data = _address(data, "blob %d data" % k, dtype, device, n)
        b.diff = _address(diff, "blob %d diff" % k, dtype, device, n)
        b.hist_grad = _address(hist, "blob %d hist_grad" % k, dtype, device, n)
        b.hist_update = None if hist2 is None else _address(hist2, "blob %d hist_update" % k, dtype, device, n)
        b.count, b.lr_mult, b.decay_mult = n, float(lr_mult), float(decay_mult)
        tensors.append((data, diff, hist, hist2))
    return SolverBlobs(array, len(entries), tensors, dtype, device)


def _elem(blobs, e):
    if not isinstance(blobs, SolverBlobs):
        raise capi.MMSArgumentError("Solver: blobs must come from solver_blobs()")
    if blobs.dtype is not None and blobs.dtype != e.dtype:
        raise capi.MMSArgumentError("Solver: the blobs are %s, this call is for %s" % (blobs.dtype, e.dtype))


def _solver_workspace_bytes(e, param, blobs):
    _elem(blobs, e)
    return getattr(lib(), "mms_solver_workspace_bytes" + e.query)(C.byref(param), blobs.array, blobs.array_len)


def solver_workspace_bytes(param, blobs):
    """Bytes a step needs for the chunk sums of the gradient norm: 0 without clipping (mms_solver_workspace_bytes)."""
    return _solver_workspace_bytes(capi._F32, param, blobs)


def solver_workspace_bytes_f64(param, blobs):
    return _solver_workspace_bytes(capi._F64, param, blobs)


def _solver_step(e, param, blobs, rate, clip_info, ws):
    _elem(blobs, e)
    if not isinstance(param, SolverParam):
        raise capi.MMSArgumentError("Solver: param must come from solver_param()")
    if clip_info is not None:
        if blobs.device is None:
            raise capi.MMSArgumentError("Solver: clip_info without blobs")
        _address(clip_info, "clip_info", e.dtype, blobs.device, 2)
    need = _solver_workspace_bytes(e, param, blobs)
    wsp, wsb = capi._scratch(ws, need, blobs.device) if need else (None, 0)
    scalar = C.c_float if e.suffix == "f32" else C.c_double
    capi._call("mms_solver_step_" + e.suffix, C.byref(param), blobs.array, blobs.array_len, scalar(float(rate)),
               None if clip_info is None else clip_info.data_ptr(), wsp, wsb)


def solver_step(param, blobs, rate, clip_info=None, ws=None):
    """One solver step over all blobs (include/mms_solver.h: mms_solver_step_f32): data, diff and the histories are
    updated in place.  rate: the learning rate of this iteration.  clip_info: a 2-element device tensor that receives
    the gradient norm and the scale applied, with clipping on; or None."""
    _solver_step(capi._F32, param, blobs, rate, clip_info, ws)


def solver_step_f64(param, blobs, rate, clip_info=None, ws=None):
    _solver_step(capi._F64, param, blobs, rate, clip_info, ws)
