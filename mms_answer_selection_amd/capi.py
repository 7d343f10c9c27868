"""ctypes binding of libmms_hip.so (include/mms.h) for torch device tensors.

torch is plumbing here: it owns device memory and the HIP stream; every
computation goes through the C ABI.  There is NO fallback: if the library is
missing or a tensor is not on the GPU the call raises.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmms_hip.so")

MMS_OK = 0
_lib = None

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

_SIGNATURES = {
    "mms_version": (C.c_int, []),
    "mms_error_string": (C.c_char_p, [_i]),
    "mms_simcross_workspace_bytes": (_sz, [_i] * 6),
    "mms_simcross_forward_f32": (_i, [_i] * 6 + [_vp] * 8 + [_sz, _vp]),
    "mms_simcross_backward_f32": (_i, [_i] * 6 + [_vp] * 3 + [_i] + [_vp] * 4 + [_i, _i] + [_vp] * 5 + [_sz, _vp]),
    "mms_simcross_forward_backward_f32": (_i, [_i] * 6 + [_vp] * 13 + [_sz, _vp]),
    "mms_simmatrix_workspace_bytes": (_sz, [_i] * 3),
    "mms_embed_simcross_forward_f32": (_i, [_i] * 6 + [_vp] * 8),
    "mms_embed_simcross_bilinear_forward_f32": (_i, [_i] * 6 + [_vp] * 8),
    "mms_simmatrix_forward_f32": (_i, [_i] * 3 + [_vp] * 6),
    "mms_simmatrix_forward_ws_f32": (_i, [_i] * 3 + [_vp] * 6 + [_sz, _vp]),
    "mms_simmatrix_forward_f16": (_i, [_i] * 3 + [_vp] * 5 + [_sz, _vp]),
    "mms_simmatrix_forward_train_f16": (_i, [_i] * 3 + [_vp] * 6 + [_sz, _vp]),
    "mms_simmatrix_backward_f16": (_i, [_i] * 3 + [_vp] * 9 + [_sz, _vp]),
    "mms_set_matrix_mode": (_i, [_i]),
    "mms_get_matrix_mode": (_i, []),
    "mms_simmatrix_backward_f32": (_i, [_i] * 3 + [_vp] * 4 + [_i] * 3 + [_vp] * 4 + [_sz, _vp]),
    "mms_simmatrix_backward_cached_f32": (_i, [_i] * 3 + [_vp] * 5 + [_i] * 3 + [_vp] * 4 + [_sz, _vp]),
    "mms_pairrank_workspace_bytes": (_sz, [_i]),
    "mms_pairrank_forward_f32": (_i, [_i, _f] + [_vp] * 7 + [_sz, _vp]),
    "mms_pairrank_backward_f32": (_i, [_i, _f] + [_vp] * 3 + [_i, _i] + [_vp] * 3),
    "mms_triplet_workspace_bytes": (_sz, [_i]),
    "mms_triplet_workspace_init": (_i, [_vp, _sz, _vp]),
    "mms_triplet_simmatrix_workspace_bytes": (_sz, [_i, _i, _i]),
    "mms_triplet_simmatrix_step_f32": (_i, [_i, _i, _i, _f, _f] + [_vp] * 12 + [_vp, _sz, _vp]),
    "mms_triplet_euclid_step_f32": (_i, [_i, _i, _f, _f] + [_vp] * 11 + [_sz, _vp]),
    "mms_triplet_cosine_step_f32": (_i, [_i, _i, _f, _f] + [_vp] * 14 + [_sz, _vp]),
    "mms_simcross_euclid_forward_f16": (_i, [_i, _i, _vp, _vp, _vp, _vp]),
    "mms_simcross_euclid_forward_backward_f16": (_i, [_i, _i] + [_vp] * 7),
    "mms_simcross_cosine_forward_f16": (_i, [_i, _i] + [_vp] * 5 + [_vp]),
    "mms_simcross_cosine_forward_backward_f16": (_i, [_i, _i] + [_vp] * 8 + [_vp]),
    "mms_simcross_forward_f16": (_i, [_i] * 5 + [_vp] * 5 + [_vp]),
    "mms_simcross_backward_f16": (_i, [_i] * 5 + [_vp] * 8 + [_vp]),
    "mms_simcross_forward_backward_f16": (_i, [_i] * 5 + [_vp] * 8 + [_vp]),
    "mms_simcross_bilinear_workspace_bytes_f16": (_sz, [_i] * 5),
    "mms_simcross_bilinear_forward_f16": (_i, [_i] * 5 + [_vp] * 6 + [_sz, _vp]),
    "mms_simcross_bilinear_backward_f16": (_i, [_i] * 5 + [_vp] * 3 + [_i] + [_vp] * 6 + [_sz, _vp]),
    "mms_simcross_bilinear_forward_backward_f16": (_i, [_i] * 5 + [_vp] * 11 + [_sz, _vp]),
    "mms_embed_simcross_bilinear_forward_f16": (_i, [_i] * 6 + [_vp] * 8),
    "mms_embed_simcross_forward_f16": (_i, [_i] * 6 + [_vp] * 8),
    "mms_embed_workspace_bytes": (_sz, [_i, _i]),
    "mms_embed_forward_f32": (_i, [_i, _i, _i] + [_vp] * 5),
    "mms_embed_backward_f32": (_i, [_i, _i, _i] + [_vp] * 5 + [_sz, _vp]),
    "mms_embed_backward_pair_f32": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_embed_pair_index_supported": (_i, [_i, _i, _i]),
    "mms_embed_forward_pair_f32": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_embed_backward_pair_indexed_f32": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_embed_forward_f16": (_i, [_i, _i, _i] + [_vp] * 5),
    "mms_embed_forward_pair_f16": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_embed_backward_f16": (_i, [_i, _i, _i] + [_vp] * 5 + [_sz, _vp]),
    "mms_embed_backward_pair_f16": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_embed_backward_pair_indexed_f16": (_i, [_i, _i, _i, _i] + [_vp] * 6 + [_vp, _sz, _vp]),
    "mms_feed_gather_rows_f32": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "mms_simcross_workspace_bytes_f64": (_sz, [_i] * 6),
    "mms_simcross_forward_f64": (_i, [_i] * 6 + [_vp] * 8 + [_sz, _vp]),
    "mms_simcross_backward_f64": (_i, [_i] * 6 + [_vp] * 3 + [_i] + [_vp] * 4 + [_i, _i] + [_vp] * 5 + [_sz, _vp]),
    "mms_simmatrix_forward_f64": (_i, [_i] * 3 + [_vp] * 6),
    "mms_simmatrix_backward_f64": (_i, [_i] * 3 + [_vp] * 4 + [_i] * 3 + [_vp] * 4),
    "mms_pairrank_forward_f64": (_i, [_i, C.c_double] + [_vp] * 7),
    "mms_pairrank_backward_f64": (_i, [_i, C.c_double] + [_vp] * 3 + [_i, _i] + [_vp] * 3),
    "mms_fm_forward_f32": (_i, [_i] * 3 + [_vp] * 4),
    "mms_fm_backward_f32": (_i, [_i] * 3 + [_vp] * 5),
    "mms_fm_forward_backward_f32": (_i, [_i] * 3 + [_vp] * 7),
    "mms_fm_forward_f64": (_i, [_i] * 3 + [_vp] * 4),
    "mms_fm_backward_f64": (_i, [_i] * 3 + [_vp] * 5),
    "mms_bn_workspace_bytes": (_sz, [_i] * 3),
    "mms_bn_forward_f32": (_i, [_i] * 4 + [_f] + [_vp] * 9 + [_sz, _vp]),
    "mms_bn_backward_f32": (_i, [_i] * 3 + [_vp] * 9 + [_sz, _vp]),
    "mms_bn_workspace_bytes_f64": (_sz, [_i] * 3),
    "mms_bn_forward_f64": (_i, [_i] * 4 + [C.c_double] + [_vp] * 9 + [_sz, _vp]),
    "mms_bn_backward_f64": (_i, [_i] * 3 + [_vp] * 9 + [_sz, _vp]),
    "mms_bn_pool_tanh_workspace_bytes": (_sz, [_i] * 6),
    "mms_bn_pool_tanh_forward_f32": (_i, [_i] * 7 + [_f] + [_vp] * 10 + [_sz, _vp]),
    "mms_bn_pool_tanh_backward_f32": (_i, [_i] * 6 + [_vp] * 11 + [_sz, _vp]),
    "mms_bn_pool_tanh_workspace_bytes_f64": (_sz, [_i] * 6),
    "mms_bn_pool_tanh_forward_f64": (_i, [_i] * 7 + [C.c_double] + [_vp] * 10 + [_sz, _vp]),
    "mms_bn_pool_tanh_backward_f64": (_i, [_i] * 6 + [_vp] * 11 + [_sz, _vp]),
    "mms_set_euclid_backward_mode": (_i, [_i]),
    "mms_get_euclid_backward_mode": (_i, []),
    "mms_null_launch": (_i, [_i, _vp]),
    "mms_simcross_forward_block_f32": (_i, [_vp, _vp]),
    "mms_simcross_backward_block_f32": (_i, [_vp, _vp]),
    "mms_dot_f32": (_i, [_i, _vp, _vp, _vp, _vp]),
    "mms_split_backward_f32": (_i, [_i, _i, _vp, _vp, _vp]),
    "mms_dot_f64": (_i, [_i, _vp, _vp, _vp, _vp]),
    "mms_set_f16_distance_mode": (_i, [_i]),
    "mms_get_f16_distance_mode": (_i, []),
    "mms_set_rank_tie_mode": (_i, [_i]),
    "mms_get_rank_tie_mode": (_i, []),
    "mms_set_loss_sum_mode": (_i, [_i]),
    "mms_get_loss_sum_mode": (_i, []),
    "mms_set_triplet_finish_mode": (_i, [_i]),
    "mms_get_triplet_finish_mode": (_i, []),
    "mms_set_pairrank_hinge_mode": (_i, [_i]),
    "mms_get_pairrank_hinge_mode": (_i, []),
    "mms_rank_workspace_bytes": (_sz, [_i]),
    "mms_rank_map_mrr_f32": (_i, [_i, _i] + [_vp] * 7 + [_sz, _vp]),
    "mms_rank_auc_f32": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "mms_rank_auc_nd_f32": (_i, [_i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "mms_rank_accuracy_f32": (_i, [_i] + [_vp] * 5 + [_sz, _vp]),
    "mms_rank_workspace_bytes_f64": (_sz, [_i]),
    "mms_rank_map_mrr_f64": (_i, [_i, _i] + [_vp] * 7 + [_sz, _vp]),
    "mms_rank_auc_f64": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "mms_rank_auc_nd_f64": (_i, [_i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "mms_rank_accuracy_f64": (_i, [_i] + [_vp] * 5 + [_sz, _vp]),
    "mms_embed_workspace_bytes_f64": (_sz, [_i, _i]),
    "mms_embed_forward_f64": (_i, [_i, _i, _i] + [_vp] * 5),
    "mms_embed_backward_f64": (_i, [_i, _i, _i] + [_vp] * 5 + [_sz, _vp]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class MMSError(RuntimeError):
    pass


class MMSArgumentError(MMSError, ValueError):
    """A wrapper's own check of a tensor's shape or dtype failed, before any launch."""


MMS_VERSION = 212      # include/mms.h


def _bind(handle, signatures):
    """Apply a table {symbol: (restype, argtypes)} to a loaded library; AttributeError if a header and it diverge."""
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)
        fn.restype = res
        fn.argtypes = args
    return handle


def lib():
    """The loaded C-ABI library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MMSError(
                "libmms_hip.so is not built (%s). Run `python -m mms_answer_selection_amd.build` "
                "or __graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
        l = _bind(C.CDLL(LIB_PATH), _SIGNATURES)
        if l.mms_version() != MMS_VERSION:            # include/mms.h: a host built against another header must refuse
            raise MMSError("libmms_hip.so reports ABI version %d, this binding was written for %d: rebuild "
                           "(python -m mms_answer_selection_amd.build --force)" % (l.mms_version(), MMS_VERSION))
        _lib = l
    return _lib


_bound = {}            # id of a family's signature table -> the handle it was last applied to


def _bound_lib(signatures):
    """lib() with the signature table of a family that has a header of its own applied to it: once per handle, and
    again when the handle is replaced."""
    l = lib()
    if _bound.get(id(signatures)) is not l:
        _bound[id(signatures)] = _bind(l, signatures)
    return l


def check(rc, what):
    if rc != MMS_OK:
        raise MMSError("%s failed: %s (code %d)" % (what, lib().mms_error_string(rc).decode(), rc))


def _ptr(t, name, allow_none=False, dtype=torch.float32):
    if t is None:
        if allow_none:
            return None
        raise MMSError("%s: tensor required" % name)
    if not t.is_cuda:
        raise MMSError("%s must live in GPU memory (got %s); the HIP path has no CPU fallback"
                       % (name, t.device))
    if t.dtype != dtype:
        raise MMSError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise MMSError("%s must be contiguous" % name)
    return t.data_ptr()


def _expect(label, t, shape, name):
    """A wrapper's own shape check, under its family's label: tensor `t`, when given, has `shape`."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise MMSArgumentError("%s: %s must be %s, got %s" % (label, name, tuple(shape), tuple(t.shape)))


def _route_symbol(label, family, stem, e, route):
    """mms_<family>_<stem>_<f32|f64>, or the float call's _generic_ twin: the entry point of a family with two routes."""
    if route == "auto":
        return "mms_%s_%s_%s" % (family, stem, e.suffix)
    if route == "generic":
        # double has the generic route only, and no entry point of that name
        return "mms_%s_%s_%s" % (family, stem, "generic_f32" if e.suffix == "f32" else e.suffix)
    raise MMSArgumentError("%s: route must be 'auto' or 'generic', got %r" % (label, route))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Workspace:
    """Grow-only device scratch, owned by the caller of the C ABI (a layer)."""

    def __init__(self):
        self.buf = None
        self._retired = []          # superseded buffers stay alive: a captured hipGraph or work still queued on
                                    # another stream may hold their address (they are freed with the Workspace)

    def get(self, nbytes, device):
        if nbytes == 0:
            return None, 0
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            if self.buf is not None:
                self._retired.append(self.buf)
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf.data_ptr(), self.buf.numel()


# Calls that are not given a Workspace share this one.  It only grows, and what it outgrows is retired, not freed;
# callers that capture graphs or use several streams should still pass their own (`ws=`): the library keeps
# intermediates in it BETWEEN its own launches of one call, so two calls in flight must not share a workspace.
_default_ws = Workspace()


def _scratch(ws, nbytes, device):
    """(pointer, bytes) of at least `nbytes` of scratch from the caller's Workspace, or from the shared one."""
    return (ws or _default_ws).get(nbytes, device)


def _call(symbol, *args):
    """The one way to a launching entry point: `symbol` with `args` and the current stream, checked under that name."""
    rc = getattr(lib(), symbol)(*args, _stream())
    if rc != MMS_OK:                                  # check()'s own test, kept here to spare the common case a frame
        check(rc, symbol)


# One record per element type of the C ABI; a family is written once against it and its public _f64 (for Embed also
# _f16) names bind it.  `dtype`: what the tensors of a call hold.  `store`: the same, but for the fp16-storage Embed
# calls, which keep table / top / top_diff as half next to float32 ids, bias and gradients.  `size`: bytes of a `dtype`
# element.  `query`: the suffix of the workspace queries -- the f32 ones have none, and the f16 Embed calls share them
# (and the EmbedPairIndex buffer) with f32.
_Elem = collections.namedtuple("_Elem", "suffix dtype store size query")
_F32 = _Elem("f32", torch.float32, torch.float32, 4, "")
_F64 = _Elem("f64", torch.float64, torch.float64, 8, "_f64")
_F16_EMBED = _Elem("f16", torch.float32, torch.float16, 4, "")
_H = torch.float16


# ---- SimCross (f32, f64; there is no simcross_forward_backward_f64) --------------------------------------------
def _simcross_workspace_bytes(e, *dims):
    return getattr(lib(), "mms_simcross_workspace_bytes" + e.query)(*dims)


def simcross_workspace_bytes(mode, N, W1, W2, D, M):
    return _simcross_workspace_bytes(_F32, mode, N, W1, W2, D, M)


def _simcross_dims(mode, q, a, W):
    """(mode, N, W1, W2, D, M): the leading arguments of every SimCross call and of its workspace query."""
    N, W1, D = q.shape
    return mode, N, W1, a.shape[1], D, W.shape[0] if mode == 2 else 1


def _simcross_forward(e, mode, q, a, top, W, bias, norm0, norm1, ws):
    dims, dt = _simcross_dims(mode, q, a, W), e.dtype
    wsp, wsb = _scratch(ws, _simcross_workspace_bytes(e, *dims), q.device)
    _call("mms_simcross_forward_" + e.suffix, *dims, _ptr(q, "q", dtype=dt), _ptr(a, "a", dtype=dt),
          _ptr(W, "W", True, dt), _ptr(bias, "bias", True, dt), _ptr(top, "top", dtype=dt),
          _ptr(norm0, "norm0", True, dt), _ptr(norm1, "norm1", True, dt), wsp, wsb)


def _simcross_backward(e, mode, q, a, top, top_diff, dq, da, W, bias_term, norm0, norm1, dW, dbias, propagate_down, ws):
    dims, dt = _simcross_dims(mode, q, a, W), e.dtype
    wsp, wsb = _scratch(ws, _simcross_workspace_bytes(e, *dims), q.device)
    _call("mms_simcross_backward_" + e.suffix, *dims, _ptr(q, "q", dtype=dt), _ptr(a, "a", dtype=dt),
          _ptr(W, "W", True, dt), int(bool(bias_term)), _ptr(top, "top", dtype=dt),
          _ptr(top_diff, "top_diff", dtype=dt), _ptr(norm0, "norm0", True, dt), _ptr(norm1, "norm1", True, dt),
          int(bool(propagate_down[0])), int(bool(propagate_down[1])), _ptr(dq, "dq", dtype=dt),
          _ptr(da, "da", dtype=dt), _ptr(dW, "dW", True, dt), _ptr(dbias, "dbias", True, dt), wsp, wsb)


def simcross_forward(mode, q, a, top, W=None, bias=None, norm0=None, norm1=None, ws=None):
    _simcross_forward(_F32, mode, q, a, top, W, bias, norm0, norm1, ws)


def simcross_forward_f64(mode, q, a, top, W=None, bias=None, norm0=None, norm1=None, ws=None):
    _simcross_forward(_F64, mode, q, a, top, W, bias, norm0, norm1, ws)


def simcross_backward(mode, q, a, top, top_diff, dq, da, W=None, bias_term=False, norm0=None,
                      norm1=None, dW=None, dbias=None, propagate_down=(True, True), ws=None):
    _simcross_backward(_F32, mode, q, a, top, top_diff, dq, da, W, bias_term, norm0, norm1, dW, dbias,
                       propagate_down, ws)


def simcross_backward_f64(mode, q, a, top, top_diff, dq, da, W=None, bias_term=False, norm0=None,
                          norm1=None, dW=None, dbias=None, propagate_down=(True, True), ws=None):
    _simcross_backward(_F64, mode, q, a, top, top_diff, dq, da, W, bias_term, norm0, norm1, dW, dbias,
                       propagate_down, ws)


def simcross_forward_backward(mode, q, a, top_diff, top, dq, da, W=None, bias=None, norm0=None,
                              norm1=None, dW=None, dbias=None, ws=None):
    dims = _simcross_dims(mode, q, a, W)
    wsp, wsb = _scratch(ws, _simcross_workspace_bytes(_F32, *dims), q.device)
    _call("mms_simcross_forward_backward_f32", *dims, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W", True),
          _ptr(bias, "bias", True), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
          _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _ptr(dq, "dq"), _ptr(da, "da"),
          _ptr(dW, "dW", True), _ptr(dbias, "dbias", True), wsp, wsb)


def embed_simcross_forward(mode, index_q, index_a, weight, top, norm0=None, norm1=None, embed_bias=None):
    """top = SimCross(Embed(index_q), Embed(index_a)), dist_mode 0 / 1, the gather fused into the loads;
    embed_bias (D) = the Embed layers' bias blob, if they have one."""
    N, W1 = index_q.shape[0], index_q.shape[1]
    W2 = index_a.shape[1]
    K, D = weight.shape
    _call("mms_embed_simcross_forward_f32", mode, N, W1, W2, D, K, _ptr(index_q, "index_q"),
          _ptr(index_a, "index_a"), _ptr(weight, "weight"), _ptr(embed_bias, "embed_bias", True), _ptr(top, "top"),
          _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True))


def embed_simcross_bilinear_forward(index_q, index_a, weight, W, bias, top, embed_bias=None):
    """top (N,M,W1,W2) = SimCross dist_mode 2 of (Embed(index_q), Embed(index_a)), one launch (word grids)."""
    N, W1 = index_q.shape[0], index_q.shape[1]
    W2 = index_a.shape[1]
    K, D = weight.shape
    M = W.shape[0]
    _call("mms_embed_simcross_bilinear_forward_f32", N, W1, W2, D, M, K, _ptr(index_q, "index_q"),
          _ptr(index_a, "index_a"), _ptr(weight, "weight"), _ptr(embed_bias, "embed_bias", True), _ptr(W, "W"),
          _ptr(bias, "bias", True), _ptr(top, "top"))


# ---- SimMatrix (f32 with a workspace, fp16 storage, f64 without a workspace) -----------------------------------
def _simmatrix_scratch(ws, N, K1, K2, device):
    return _scratch(ws, lib().mms_simmatrix_workspace_bytes(N, K1, K2), device)


def _simmatrix_forward(e, q, a, W, top, qw_scratch, ws, use_workspace):
    N = q.shape[0]
    K1, K2 = W.shape
    dt = e.dtype
    scratch = _simmatrix_scratch(ws, N, K1, K2, q.device) if use_workspace else ()
    _call("mms_simmatrix_forward_ws_f32" if use_workspace else "mms_simmatrix_forward_" + e.suffix, N, K1, K2,
          _ptr(q, "q", dtype=dt), _ptr(a, "a", dtype=dt), _ptr(W, "W", dtype=dt), _ptr(top, "top", dtype=dt),
          _ptr(qw_scratch, "qw_scratch", dtype=dt), *scratch)


def simmatrix_forward(q, a, W, top, qw_scratch, ws=None, use_workspace=True):
    """With a workspace (the default one unless use_workspace=False) the call is mms_simmatrix_forward_ws_f32: Q.W on
    the bf16 matrix pipe at fp32 accuracy for N >= 2048 (include/mms.h); without, mms_simmatrix_forward_f32."""
    _simmatrix_forward(_F32, q, a, W, top, qw_scratch, ws, use_workspace)


def simmatrix_forward_f64(q, a, W, top, qw_scratch):
    _simmatrix_forward(_F64, q, a, W, top, qw_scratch, None, False)       # f64 has no workspace entry point


def simmatrix_forward_f16(q, a, W, top, ws=None):
    """fp16-storage scoring: q, a half tensors, W and top float32 (include/mms.h: mms_simmatrix_forward_f16)."""
    N = q.shape[0]
    K1, K2 = W.shape
    wsp, wsb = _simmatrix_scratch(ws, N, K1, K2, q.device)
    _call("mms_simmatrix_forward_f16", N, K1, K2, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(W, "W"),
          _ptr(top, "top"), wsp, wsb)


def simmatrix_forward_train_f16(q, a, W, top, qw_scratch, ws=None):
    N = q.shape[0]
    K1, K2 = W.shape
    wsp, wsb = _simmatrix_scratch(ws, N, K1, K2, q.device)
    _call("mms_simmatrix_forward_train_f16", N, K1, K2, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(W, "W"),
          _ptr(top, "top"), _ptr(qw_scratch, "qw_scratch"), wsp, wsb)


def simmatrix_backward_f16(q, a, W, qw, top_diff, dq, da, dW, ws=None):
    """dq, da: half tensors or None; dW: float32 (accumulated into) or None."""
    N = q.shape[0]
    K1, K2 = W.shape
    wsp, wsb = _simmatrix_scratch(ws, N, K1, K2, q.device)
    _call("mms_simmatrix_backward_f16", N, K1, K2, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(W, "W"),
          _ptr(qw, "qw", True), _ptr(top_diff, "top_diff"), _ptr(dq, "dq", True, _H), _ptr(da, "da", True, _H),
          _ptr(dW, "dW", True), wsp, wsb)


def _simmatrix_backward(e, q, a, W, top_diff, dq, da, dW, param_propagate_down, propagate_down, ws, qw):
    N = q.shape[0]
    K1, K2 = W.shape
    dt = e.dtype
    scratch = _simmatrix_scratch(ws, N, K1, K2, q.device) if e is _F32 else ()     # simmatrix_backward_f64 takes none
    head = (N, K1, K2, _ptr(q, "q", dtype=dt), _ptr(a, "a", dtype=dt), _ptr(W, "W", dtype=dt))
    if qw is not None:                                                             # the cached entry point: f32 only
        symbol, head = "mms_simmatrix_backward_cached_f32", head + (_ptr(qw, "qw"),)
    else:
        symbol = "mms_simmatrix_backward_" + e.suffix
    _call(symbol, *head, _ptr(top_diff, "top_diff", dtype=dt), int(bool(param_propagate_down)),
          int(bool(propagate_down[0])), int(bool(propagate_down[1])), _ptr(dq, "dq", True, dt),
          _ptr(da, "da", True, dt), _ptr(dW, "dW", True, dt), *scratch)


def simmatrix_backward(q, a, W, top_diff, dq, da, dW, param_propagate_down=True,
                       propagate_down=(True, True), ws=None, qw=None):
    """qw: the forward's qw_scratch (same q, W; may be `da` itself) -> the cached entry point."""
    _simmatrix_backward(_F32, q, a, W, top_diff, dq, da, dW, param_propagate_down, propagate_down, ws, qw)


def simmatrix_backward_f64(q, a, W, top_diff, dq, da, dW, param_propagate_down=True,
                           propagate_down=(True, True)):
    _simmatrix_backward(_F64, q, a, W, top_diff, dq, da, dW, param_propagate_down, propagate_down, None, None)


# ---- PairRankLoss (f32, f64; pairrank_forward_f64 takes no workspace) ------------------------------------------
def _pairrank_forward(e, a, b, y, ordered, similar, loss, margin, ws):
    count, dt = a.numel(), e.dtype
    scratch = _scratch(ws, lib().mms_pairrank_workspace_bytes(count), a.device) if e is _F32 else ()
    _call("mms_pairrank_forward_" + e.suffix, count, float(margin), _ptr(a, "a", dtype=dt), _ptr(b, "b", dtype=dt),
          _ptr(y, "y", dtype=dt), _ptr(ordered, "ordered", dtype=dt), _ptr(similar, "similar", dtype=dt),
          _ptr(loss, "loss", dtype=dt), *scratch)


def _pairrank_backward(e, y, ordered, similar, da, db, top_diff, propagate_down):
    dt = e.dtype
    _call("mms_pairrank_backward_" + e.suffix, y.numel(), float(top_diff), _ptr(y, "y", dtype=dt),
          _ptr(ordered, "ordered", dtype=dt), _ptr(similar, "similar", dtype=dt), int(bool(propagate_down[0])),
          int(bool(propagate_down[1])), _ptr(da, "da", True, dt), _ptr(db, "db", True, dt))


def pairrank_forward(a, b, y, ordered, similar, loss, margin=1.0, ws=None):
    _pairrank_forward(_F32, a, b, y, ordered, similar, loss, margin, ws)


def pairrank_forward_f64(a, b, y, ordered, similar, loss, margin=1.0):
    _pairrank_forward(_F64, a, b, y, ordered, similar, loss, margin, None)


def pairrank_backward(y, ordered, similar, da, db, top_diff=1.0, propagate_down=(True, True)):
    _pairrank_backward(_F32, y, ordered, similar, da, db, top_diff, propagate_down)


def pairrank_backward_f64(y, ordered, similar, da, db, top_diff=1.0, propagate_down=(True, True)):
    _pairrank_backward(_F64, y, ordered, similar, da, db, top_diff, propagate_down)


# ---- FM pooling (f32, f64; there is no fm_forward_backward_f64) ------------------------------------------------
def _fm_forward(e, x, top, bias):
    N, C, dim = x.shape
    dt = e.dtype
    _call("mms_fm_forward_" + e.suffix, N, C, dim, _ptr(x, "x", dtype=dt), _ptr(bias, "bias", True, dt),
          _ptr(top, "top", dtype=dt))


def _fm_backward(e, x, top_diff, bottom_diff, bias_diff):
    N, C, dim = x.shape
    dt = e.dtype
    _call("mms_fm_backward_" + e.suffix, N, C, dim, _ptr(x, "x", dtype=dt), _ptr(top_diff, "top_diff", dtype=dt),
          _ptr(bottom_diff, "bottom_diff", True, dt), _ptr(bias_diff, "bias_diff", True, dt))


def fm_forward(x, top, bias=None):
    """FM pooling (include/mms.h: mms_fm_forward_f32).  x (N, C, dim); top N floats; bias one float or None."""
    _fm_forward(_F32, x, top, bias)


def fm_forward_f64(x, top, bias=None):
    _fm_forward(_F64, x, top, bias)


def fm_backward(x, top_diff, bottom_diff=None, bias_diff=None):
    """bottom_diff None = propagate_down[0] false; bias_diff None = no bias term or param_propagate_down false.
    Both are overwritten."""
    _fm_backward(_F32, x, top_diff, bottom_diff, bias_diff)


def fm_backward_f64(x, top_diff, bottom_diff=None, bias_diff=None):
    _fm_backward(_F64, x, top_diff, bottom_diff, bias_diff)


def fm_forward_backward(x, top_diff, top, bottom_diff, bias=None, bias_diff=None):
    N, C, dim = x.shape
    _call("mms_fm_forward_backward_f32", N, C, dim, _ptr(x, "x"), _ptr(bias, "bias", True),
          _ptr(top_diff, "top_diff"), _ptr(top, "top"), _ptr(bottom_diff, "bottom_diff"),
          _ptr(bias_diff, "bias_diff", True))


# ---- BN, and BN -> average pooling -> TanH (f32, f64) ----------------------------------------------------------
def _bn_shape(x):
    """(N, C, S) of a blob (N, C, S) or (N, C, H, W): S is everything after the channel axis."""
    if x.dim() < 2:
        raise MMSArgumentError("BN: x must be (N, C, ...), got %s" % (tuple(x.shape),))
    S = 1
    for d in x.shape[2:]:
        S *= int(d)
    return int(x.shape[0]), int(x.shape[1]), S


def _bn_workspace_bytes(e, N, C, S):
    return getattr(lib(), "mms_bn_workspace_bytes" + e.query)(N, C, S)


def bn_workspace_bytes(N, C, S):
    """0 where one workgroup per channel serves (include/mms.h: mms_bn_workspace_bytes)."""
    return _bn_workspace_bytes(_F32, N, C, S)


def bn_workspace_bytes_f64(N, C, S):
    return _bn_workspace_bytes(_F64, N, C, S)


def _bn_forward(e, x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase, bn_memory, ws):
    N, C, S = _bn_shape(x)
    dt = e.dtype
    wsp, wsb = _scratch(ws, _bn_workspace_bytes(e, N, C, S), x.device)
    _call("mms_bn_forward_" + e.suffix, int(phase), N, C, S, float(bn_memory), _ptr(x, "x", dtype=dt),
          _ptr(scale, "scale", dtype=dt), _ptr(shift, "shift", dtype=dt),
          _ptr(running_mean, "running_mean", dtype=dt), _ptr(running_var, "running_var", dtype=dt),
          _ptr(top, "top", dtype=dt), _ptr(save_mean, "save_mean", dtype=dt), _ptr(save_std, "save_std", dtype=dt),
          wsp, wsb)


def _bn_backward(e, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws):
    N, C, S = _bn_shape(x)
    dt = e.dtype
    wsp, wsb = _scratch(ws, _bn_workspace_bytes(e, N, C, S), x.device)
    _call("mms_bn_backward_" + e.suffix, N, C, S, _ptr(x, "x", dtype=dt), _ptr(top_diff, "top_diff", dtype=dt),
          _ptr(scale, "scale", dtype=dt), _ptr(save_mean, "save_mean", dtype=dt), _ptr(save_std, "save_std", dtype=dt),
          _ptr(bottom_diff, "bottom_diff", True, dt), _ptr(scale_diff, "scale_diff", True, dt),
          _ptr(shift_diff, "shift_diff", True, dt), wsp, wsb)


def bn_forward(x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase=0, bn_memory=0.9, ws=None):
    """BN forward (include/mms.h: mms_bn_forward_f32).  x, top (N, C, S) or (N, C, H, W); the other six C floats.
    phase 0 = TRAIN (batch statistics; the running blobs are updated in place), 1 = TEST (running statistics, read
    only).  save_mean / save_std are what bn_backward needs."""
    _bn_forward(_F32, x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase, bn_memory, ws)


def bn_forward_f64(x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase=0, bn_memory=0.9,
                   ws=None):
    _bn_forward(_F64, x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase, bn_memory, ws)


def bn_backward(x, top_diff, scale, save_mean, save_std, bottom_diff=None, scale_diff=None, shift_diff=None, ws=None):
    """Each of bottom_diff, scale_diff, shift_diff may be None (skipped); those given are overwritten."""
    _bn_backward(_F32, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws)


def bn_backward_f64(x, top_diff, scale, save_mean, save_std, bottom_diff=None, scale_diff=None, shift_diff=None,
                    ws=None):
    _bn_backward(_F64, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws)


def _bn_pool_shape(x, kernel):
    """(N, C, H, W, kh, kw) of a 4-D blob and a pooling kernel (k or (kh, kw))."""
    return _pooled.bn_pool_shape(_BN_POOL, x, kernel)


def bn_pool_tanh_workspace_bytes(N, C, H, W, kh, kw):
    """0 where one workgroup per channel serves (include/mms.h: mms_bn_pool_tanh_workspace_bytes)."""
    return _pooled.bn_pool_workspace_bytes(_BN_POOL, _F32, N, C, H, W, kh, kw)


def bn_pool_tanh_workspace_bytes_f64(N, C, H, W, kh, kw):
    return _pooled.bn_pool_workspace_bytes(_BN_POOL, _F64, N, C, H, W, kh, kw)


def bn_pool_tanh_forward(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                         phase=0, bn_memory=0.9, ws=None):
    """BN -> AvePool(kernel = stride, windows tile the map) -> TanH (include/mms.h: mms_bn_pool_tanh_forward_f32).
    x (N, C, H, W); kernel k or (kh, kw); top, save_pool (N, C, H/kh, W/kw); the other six C floats.  phase as in
    bn_forward.  save_pool, save_mean, save_std and top are what bn_pool_tanh_backward needs."""
    _pooled.bn_pool_forward(_BN_POOL, _F32, x, kernel, scale, shift, running_mean, running_var, top, save_pool,
                            save_mean, save_std, phase, bn_memory, ws)


def bn_pool_tanh_forward_f64(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                             phase=0, bn_memory=0.9, ws=None):
    _pooled.bn_pool_forward(_BN_POOL, _F64, x, kernel, scale, shift, running_mean, running_var, top, save_pool,
                            save_mean, save_std, phase, bn_memory, ws)


def bn_pool_tanh_backward(x, kernel, top, top_diff, save_pool, scale, save_mean, save_std, bottom_diff=None,
                          scale_diff=None, shift_diff=None, ws=None):
    """Each of bottom_diff (N, C, H, W), scale_diff, shift_diff (C) may be None (skipped); those given are
    overwritten."""
    _pooled.bn_pool_backward(_BN_POOL, _F32, x, kernel, top, top_diff, save_pool, scale, None, save_mean, save_std,
                             bottom_diff, scale_diff, shift_diff, ws)


def bn_pool_tanh_backward_f64(x, kernel, top, top_diff, save_pool, scale, save_mean, save_std, bottom_diff=None,
                              scale_diff=None, shift_diff=None, ws=None):
    _pooled.bn_pool_backward(_BN_POOL, _F64, x, kernel, top, top_diff, save_pool, scale, None, save_mean, save_std,
                             bottom_diff, scale_diff, shift_diff, ws)


# ---- fused triplet steps ---------------------------------------------------------------------------------------
class TripletWorkspace:
    """The fused step's own scratch: its head holds the arrival words of the in-launch loss sum, which must be zero
    between launches (include/mms.h), so it is never shared with other entry points' scratch.  Grow-only; a buffer
    it outgrows is retired, not freed (a captured hipGraph may hold its address); every new buffer is initialised
    with mms_triplet_workspace_init on the current stream.  `reset()` re-initialises after a failed launch."""

    def __init__(self):
        self.buf = None
        self._retired = []

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            if self.buf is not None:
                self._retired.append(self.buf)
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.reset()
        return self.buf.data_ptr(), self.buf.numel()

    def reset(self):
        if self.buf is not None:
            _call("mms_triplet_workspace_init", self.buf.data_ptr(), self.buf.numel())


_default_triplet_ws = {}


def _triplet_scratch(step, ws, N, device):
    """The (pointer, bytes) of a row-pair step's TripletWorkspace: the caller's, or the device's default one."""
    if ws is None:
        ws = _default_triplet_ws.setdefault(device, TripletWorkspace())
    if not isinstance(ws, TripletWorkspace):
        raise TypeError("%s needs a capi.TripletWorkspace (its arrival words must stay zero "
                        "between launches; a general Workspace is overwritten by other calls)" % step)
    return ws.get(lib().mms_triplet_workspace_bytes(N), device)


def triplet_euclid_step(q, a_pos, a_neg, y, s_pos, s_neg, loss, dq, da_pos, da_neg, margin=1.0,
                        loss_weight=1.0, ws=None):
    """`ws`: a TripletWorkspace; calls that may be in flight together (streams, concurrently replayed graphs) must
    not share one.  Default: one per device."""
    N, D = q.shape[0], q.shape[-1]
    wsp, wsb = _triplet_scratch("triplet_euclid_step", ws, N, q.device)
    _call("mms_triplet_euclid_step_f32", N, D, float(margin), float(loss_weight), _ptr(q, "q"),
          _ptr(a_pos, "a_pos"), _ptr(a_neg, "a_neg"), _ptr(y, "y"), _ptr(s_pos, "s_pos"), _ptr(s_neg, "s_neg"),
          _ptr(loss, "loss", True), _ptr(dq, "dq"), _ptr(da_pos, "da_pos"), _ptr(da_neg, "da_neg"), wsp, wsb)


def triplet_cosine_step(q, a_pos, a_neg, y, s_pos, s_neg, loss, dq, da_pos, da_neg, margin=1.0,
                        loss_weight=1.0, norms=None, ws=None):
    """The fused cosine step (include/mms.h: mms_triplet_cosine_step_f32).  `norms`: None, or (norm_q, norm_pos,
    norm_neg) tensors of N floats, any of which may be None.  `ws`: a TripletWorkspace, as for triplet_euclid_step."""
    N, D = q.shape[0], q.shape[-1]
    wsp, wsb = _triplet_scratch("triplet_cosine_step", ws, N, q.device)
    nq, npos, nneg = norms if norms is not None else (None, None, None)
    _call("mms_triplet_cosine_step_f32", N, D, float(margin), float(loss_weight), _ptr(q, "q"),
          _ptr(a_pos, "a_pos"), _ptr(a_neg, "a_neg"), _ptr(y, "y"), _ptr(s_pos, "s_pos"), _ptr(s_neg, "s_neg"),
          _ptr(nq, "norm_q", True), _ptr(npos, "norm_pos", True), _ptr(nneg, "norm_neg", True),
          _ptr(loss, "loss", True), _ptr(dq, "dq"), _ptr(da_pos, "da_pos"), _ptr(da_neg, "da_neg"), wsp, wsb)


def triplet_simmatrix_step(q, a_pos, a_neg, y, W, s_pos, s_neg, loss, dq, da_pos, da_neg, dW, margin=1.0,
                           loss_weight=1.0, ws=None):
    """The fused learned-metric step (include/mms.h: mms_triplet_simmatrix_step_f32).  dW is ACCUMULATED into."""
    N, K1 = q.shape
    K2 = a_pos.shape[1]
    wsp, wsb = _scratch(ws, lib().mms_triplet_simmatrix_workspace_bytes(N, K1, K2), q.device)
    _call("mms_triplet_simmatrix_step_f32", N, K1, K2, float(margin), float(loss_weight), _ptr(q, "q"),
          _ptr(a_pos, "a_pos"), _ptr(a_neg, "a_neg"), _ptr(y, "y"), _ptr(W, "W"), _ptr(s_pos, "s_pos"),
          _ptr(s_neg, "s_neg"), _ptr(loss, "loss", True), _ptr(dq, "dq"), _ptr(da_pos, "da_pos"),
          _ptr(da_neg, "da_neg"), _ptr(dW, "dW"), wsp, wsb)


# ---- ranking metrics (f32, f64) --------------------------------------------------------------------------------
def _rank_workspace_bytes(e, n):
    return getattr(lib(), "mms_rank_workspace_bytes" + e.query)(n)


def _rank_map_mrr(e, prob, label, group, out, eff, fixed_axis, ws):
    n, dt = label.numel(), e.dtype
    wsp, wsb = _scratch(ws, _rank_workspace_bytes(e, n), prob.device)
    _call("mms_rank_map_mrr_" + e.suffix, n, int(fixed_axis), _ptr(prob, "prob", dtype=dt),
          _ptr(label, "label", dtype=dt), _ptr(group, "group", dtype=dt), out.data_ptr(), out.data_ptr() + e.size,
          eff.data_ptr(), wsp, wsb)


def _rank_map_mrr_host(e, prob, label, group, fixed_axis, ws):
    out = torch.empty(2, dtype=e.dtype, device=prob.device)
    eff = torch.empty(1, dtype=torch.int32, device=prob.device)
    _rank_map_mrr(e, prob, label, group, out, eff, fixed_axis, ws)
    o = out.cpu().numpy()
    return o[0], o[1], int(eff.item())


def _rank_auc(e, prob, label, fixed_axis, ignore_label, ws):
    n, dt = label.numel(), e.dtype
    wsp, wsb = _scratch(ws, _rank_workspace_bytes(e, n), prob.device)
    out = torch.empty(1, dtype=dt, device=prob.device)
    _call("mms_rank_auc_" + e.suffix, n, int(prob.shape[1]), int(fixed_axis), _ptr(prob, "prob", dtype=dt),
          _ptr(label, "label", dtype=dt), int(ignore_label is not None), int(ignore_label or 0), out.data_ptr(),
          wsp, wsb)
    return out.cpu().numpy()[0]


def _rank_auc_nd(e, prob, label, axis, fixed_axis, ignore_label, ws):
    shape, dt = tuple(prob.shape), e.dtype
    axis = axis % len(shape)
    outer = int(np.prod(shape[:axis])) if axis else 1
    inner = int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
    wsp, wsb = _scratch(ws, _rank_workspace_bytes(e, outer * inner), prob.device)
    out = torch.empty(1, dtype=dt, device=prob.device)
    _call("mms_rank_auc_nd_" + e.suffix, outer, int(shape[axis]), inner, int(fixed_axis),
          _ptr(prob, "prob", dtype=dt), _ptr(label, "label", dtype=dt), int(ignore_label is not None),
          int(ignore_label or 0), out.data_ptr(), wsp, wsb)
    return out.cpu().numpy()[0]


def _rank_accuracy(e, a, b, label, ws):
    n, dt = a.numel(), e.dtype
    wsp, wsb = _scratch(ws, max(4096, _rank_workspace_bytes(e, 1)), a.device)
    out = torch.empty(1, dtype=dt, device=a.device)
    _call("mms_rank_accuracy_" + e.suffix, n, _ptr(a, "a", dtype=dt), _ptr(b, "b", dtype=dt),
          _ptr(label, "label", dtype=dt), out.data_ptr(), wsp, wsb)
    return out.cpu().numpy()[0]


def rank_map_mrr(prob, label, group, fixed_axis=1, ws=None):
    """-> (MAP, MRR, effective groups) as Python numbers (device -> host copy of 3 scalars)."""
    return _rank_map_mrr_host(_F32, prob, label, group, fixed_axis, ws)


def rank_map_mrr_f64(prob, label, group, fixed_axis=1, ws=None):
    """-> (MAP, MRR, effective groups): two numpy float64 scalars and an int."""
    return _rank_map_mrr_host(_F64, prob, label, group, fixed_axis, ws)


def rank_map_mrr_device(prob, label, group, out, eff, fixed_axis=1, ws=None):
    """The same with the results left on the device: out (2 floats: MAP, MRR), eff (1 int32); no host sync."""
    _rank_map_mrr(_F32, prob, label, group, out, eff, fixed_axis, ws)


def rank_auc(prob, label, fixed_axis=1, ignore_label=None, ws=None):
    return _rank_auc(_F32, prob, label, fixed_axis, ignore_label, ws)


def rank_auc_f64(prob, label, fixed_axis=1, ignore_label=None, ws=None):
    return _rank_auc(_F64, prob, label, fixed_axis, ignore_label, ws)


def rank_auc_nd(prob, label, axis=1, fixed_axis=1, ignore_label=None, ws=None):
    """AUC layer for any label axis: prob (..., C, ...) with `axis` the class axis, label of the remaining shape."""
    return _rank_auc_nd(_F32, prob, label, axis, fixed_axis, ignore_label, ws)


def rank_auc_nd_f64(prob, label, axis=1, fixed_axis=1, ignore_label=None, ws=None):
    return _rank_auc_nd(_F64, prob, label, axis, fixed_axis, ignore_label, ws)


def rank_accuracy(a, b, label, ws=None):
    return _rank_accuracy(_F32, a, b, label, ws)


def rank_accuracy_f64(a, b, label, ws=None):
    return _rank_accuracy(_F64, a, b, label, ws)


# ---- fp16-storage SimCross on row pairs (N, 1, D) --------------------------------------------------------------
def simcross_euclid_forward_f16(q, a, top):
    """fp16-storage scoring (cfg 5): q, a half tensors (N,1,D); top float32."""
    N, D = q.shape[0], q.shape[-1]
    _call("mms_simcross_euclid_forward_f16", N, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(top, "top"))


def simcross_euclid_forward_backward_f16(q, a, top_diff, top, dq, da):
    N, D = q.shape[0], q.shape[-1]
    _call("mms_simcross_euclid_forward_backward_f16", N, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(top_diff, "top_diff"), _ptr(top, "top"), _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H))


def simcross_cosine_forward_backward_f16(q, a, top_diff, top, dq, da, norm0=None, norm1=None):
    N, D = q.shape[0], q.shape[-1]
    _call("mms_simcross_cosine_forward_backward_f16", N, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(top_diff, "top_diff"), _ptr(top, "top"), _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True),
          _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H))


def simcross_cosine_forward_f16(q, a, top, norm0=None, norm1=None):
    N, D = q.shape[0], q.shape[-1]
    _call("mms_simcross_cosine_forward_f16", N, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(top, "top"),
          _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True))


# ---- fp16-storage SimCross on word grids -----------------------------------------------------------------------
def _grid_f16_shape(q, a):
    """(N, W1, W2, D) of half word grids q (N, W1, D), a (N, W2, D)."""
    if q.dim() != 3 or a.dim() != 3 or q.shape[0] != a.shape[0] or q.shape[2] != a.shape[2]:
        raise MMSError("q (N, W1, D) and a (N, W2, D) expected, got %s and %s" % (tuple(q.shape), tuple(a.shape)))
    return q.shape[0], q.shape[1], a.shape[1], q.shape[2]


def _expect_shape(t, shape, name):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise MMSError("%s must have shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))


def _grid_f16_checked(q, a, top, norm0, norm1, top_diff=None, dq=None, da=None):
    """_grid_f16_shape, after holding every other tensor of a dist_mode 0 / 1 grid call to the shape that follows from
    it (a None is not looked at)."""
    N, W1, W2, D = _grid_f16_shape(q, a)
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(top_diff, (N, 1, W1, W2), "top_diff")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    return N, W1, W2, D


def simcross_forward_f16(mode, q, a, top, norm0=None, norm1=None):
    """fp16-storage SimCross forward on word grids, dist_mode 0 / 1 (include/mms.h: mms_simcross_forward_f16): q, a half
    tensors; top (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2) float32, the norms for dist_mode 0 only."""
    N, W1, W2, D = _grid_f16_checked(q, a, top, norm0, norm1)
    _call("mms_simcross_forward_f16", mode, N, W1, W2, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(top, "top"), _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True))


def simcross_backward_f16(mode, q, a, top, top_diff, dq, da, norm0=None, norm1=None):
    """The backward of simcross_forward_f16: dq, da half tensors shaped like q, a (mms_simcross_backward_f16)."""
    N, W1, W2, D = _grid_f16_checked(q, a, top, norm0, norm1, top_diff, dq, da)
    _call("mms_simcross_backward_f16", mode, N, W1, W2, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(top, "top"), _ptr(top_diff, "top_diff"), _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True),
          _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H))


def simcross_forward_backward_f16(mode, q, a, top_diff, top, dq, da, norm0=None, norm1=None):
    """simcross_forward_f16 then simcross_backward_f16 in one call (mms_simcross_forward_backward_f16)."""
    N, W1, W2, D = _grid_f16_checked(q, a, top, norm0, norm1, top_diff, dq, da)
    _call("mms_simcross_forward_backward_f16", mode, N, W1, W2, D, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(top_diff, "top_diff"), _ptr(top, "top"), _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True),
          _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H))


def simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M):
    return lib().mms_simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M)


def _bilinear_W_shape(W, D):
    """M of W (M, D, D)."""
    if W is None or W.dim() != 3 or tuple(W.shape[1:]) != (D, D):
        raise MMSError("W (M, D, D) expected with D = %d, got %s" % (D, None if W is None else tuple(W.shape)))
    return W.shape[0]


def _bilinear_f16_checked(ws, q, a, W, bias=None, dbias=None, top=None, top_diff=None, dq=None, da=None, dW=None):
    """(N, W1, W2, D, M) and the workspace of a dist_mode 2 grid call, after holding every other tensor to the shape
    that follows from q, a and W (a None is not looked at)."""
    N, W1, W2, D = _grid_f16_shape(q, a)
    M = _bilinear_W_shape(W, D)
    _expect_shape(bias, (M, W1, W2), "bias")
    _expect_shape(dbias, (M, W1, W2), "dbias")
    _expect_shape(top, (N, M, W1, W2), "top")
    _expect_shape(top_diff, (N, M, W1, W2), "top_diff")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    _expect_shape(dW, W.shape, "dW")
    return (N, W1, W2, D, M), _scratch(ws, simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M), q.device)


def simcross_bilinear_forward_f16(q, a, W, bias, top, ws=None):
    """fp16-storage SimCross dist_mode 2 on word grids (include/mms.h: mms_simcross_bilinear_forward_f16): q (N, W1, D), a (N, W2, D)
    half tensors; W (M, D, D), bias (M, W1, W2) or None and top (N, M, W1, W2) float32."""
    dims, scratch = _bilinear_f16_checked(ws, q, a, W, bias, top=top)
    _call("mms_simcross_bilinear_forward_f16", *dims, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(W, "W"),
          _ptr(bias, "bias", True), _ptr(top, "top"), *scratch)


def simcross_bilinear_backward_f16(q, a, W, top_diff, dq, da, dW, dbias=None, ws=None):
    """The backward of simcross_bilinear_forward_f16: dq, da half tensors shaped like q, a; dW like W (overwritten); dbias
    (M, W1, W2) float32 is accumulated into, None = no bias term (mms_simcross_bilinear_backward_f16)."""
    dims, scratch = _bilinear_f16_checked(ws, q, a, W, None, dbias, None, top_diff, dq, da, dW)
    _call("mms_simcross_bilinear_backward_f16", *dims, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H), _ptr(W, "W"),
          int(dbias is not None), _ptr(top_diff, "top_diff"), _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H),
          _ptr(dW, "dW"), _ptr(dbias, "dbias", True), *scratch)


def simcross_bilinear_forward_backward_f16(q, a, W, bias, top_diff, top, dq, da, dW, dbias=None, ws=None):
    """simcross_bilinear_forward_f16 then simcross_bilinear_backward_f16 in one call; the bias term is `bias is not None`, and
    then dbias is required (mms_simcross_bilinear_forward_backward_f16)."""
    dims, scratch = _bilinear_f16_checked(ws, q, a, W, bias, dbias, top, top_diff, dq, da, dW)
    _call("mms_simcross_bilinear_forward_backward_f16", *dims, _ptr(q, "q", dtype=_H), _ptr(a, "a", dtype=_H),
          _ptr(W, "W"), _ptr(bias, "bias", True), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
          _ptr(dq, "dq", dtype=_H), _ptr(da, "da", dtype=_H), _ptr(dW, "dW"), _ptr(dbias, "dbias", True), *scratch)


def _embed_grid_f16_shape(index_q, index_a, table, error):
    """(N, W1, W2, K, D) of id grids index_q (N, W1), index_a (N, W2) and a table (K, D); `error`: what a mismatch
    raises (the two callers differ: MMSError here, the ValueError MMSArgumentError there)."""
    if index_q.dim() != 2 or index_a.dim() != 2 or index_q.shape[0] != index_a.shape[0] or table.dim() != 2:
        raise error("index_q (N, W1), index_a (N, W2) and table (K, D) expected, got %s, %s and %s"
                    % (tuple(index_q.shape), tuple(index_a.shape), tuple(table.shape)))
    return tuple(index_q.shape) + (index_a.shape[1],) + tuple(table.shape)


def embed_simcross_bilinear_forward_f16(index_q, index_a, table, W, bias, top, embed_bias=None):
    """embed_simcross_bilinear_forward from a half table (K, D): index_q (N, W1), index_a (N, W2) float32 ids, W (M, D, D), bias
    (M, W1, W2) or None, embed_bias (D) or None, top (N, M, W1, W2) float32 (mms_embed_simcross_bilinear_forward_f16)."""
    N, W1, W2, K, D = _embed_grid_f16_shape(index_q, index_a, table, MMSError)
    M = _bilinear_W_shape(W, D)
    _expect_shape(bias, (M, W1, W2), "bias")
    _expect_shape(embed_bias, (D,), "embed_bias")
    _expect_shape(top, (N, M, W1, W2), "top")
    _call("mms_embed_simcross_bilinear_forward_f16", N, W1, W2, D, M, K, _ptr(index_q, "index_q"),
          _ptr(index_a, "index_a"), _ptr(table, "table", dtype=_H), _ptr(embed_bias, "embed_bias", True),
          _ptr(W, "W"), _ptr(bias, "bias", True), _ptr(top, "top"))


def embed_simcross_forward_f16(mode, index_q, index_a, table, top, norm0=None, norm1=None, embed_bias=None):
    """embed_simcross_forward from a half table (K, D), dist_mode 0 / 1: index_q (N, W1), index_a (N, W2) float32 ids, embed_bias (D)
    or None, top (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2) float32, the norms for dist_mode 0 only
    (mms_embed_simcross_forward_f16).  A table that is not half, or index_q and index_a of different batch sizes: ValueError."""
    N, W1, W2, K, D = _embed_grid_f16_shape(index_q, index_a, table, MMSArgumentError)
    if table.dtype != torch.float16:
        raise MMSArgumentError("table must be torch.float16 (got %s); an fp32 table goes to embed_simcross_forward" % table.dtype)
    _expect_shape(embed_bias, (D,), "embed_bias")
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    _call("mms_embed_simcross_forward_f16", mode, N, W1, W2, D, K, _ptr(index_q, "index_q"), _ptr(index_a, "index_a"),
          _ptr(table, "table", dtype=_H), _ptr(embed_bias, "embed_bias", True), _ptr(top, "top"),
          _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True))


# ---- Embed (f32, f64, and fp16 storage: half table / top / top_diff, float32 ids, bias and (master) gradients).
# Only forward and backward exist in f64.  The f16 calls use the f32 workspace query and the f32 calls' EmbedPairIndex:
# an index built by either pair forward serves either indexed backward.  `table`: the name the table argument has in
# the public signature ("weight", for f16 "table"), which is how a refusal speaks of it.
class EmbedPairIndex:
    """The inverted index of two Embed layers' word ids, built by embed_forward_pair and consumed by
    embed_backward_pair(index=...): its own buffer (nothing else may write it between the two calls)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf.data_ptr(), self.buf.numel()


def _embed_workspace_bytes(e, rows, N):
    return getattr(lib(), "mms_embed_workspace_bytes" + e.query)(rows, N)


def _embed_forward(e, index, weight, table, top, bias):
    M, (K, N) = index.numel(), weight.shape
    _call("mms_embed_forward_" + e.suffix, M, N, K, _ptr(index, "index", dtype=e.dtype),
          _ptr(weight, table, dtype=e.store), _ptr(bias, "bias", True, e.dtype), _ptr(top, "top", dtype=e.store))


def _embed_backward(e, index, top_diff, weight_diff, bias_diff, ws, shape):
    M, (K, N) = index.numel(), (shape if shape is not None else weight_diff.shape)
    wsp, wsb = _scratch(ws, _embed_workspace_bytes(e, M, N), index.device)
    _call("mms_embed_backward_" + e.suffix, M, N, K, _ptr(index, "index", dtype=e.dtype),
          _ptr(top_diff, "top_diff", dtype=e.store), _ptr(weight_diff, "weight_diff", True, e.dtype),
          _ptr(bias_diff, "bias_diff", True, e.dtype), wsp, wsb)


def _embed_forward_pair(e, index0, index1, weight, table, top0, top1, bias, index):
    M0, M1, (K, N) = index0.numel(), index1.numel(), weight.shape
    wsp, wsb, built = None, 0, False
    if index is not None and lib().mms_embed_pair_index_supported(M0, M1, K):
        wsp, wsb = index.get(_embed_workspace_bytes(e, M0 + M1, N), index0.device)
        built = True
    _call("mms_embed_forward_pair_" + e.suffix, M0, M1, N, K, _ptr(index0, "index0"), _ptr(index1, "index1"),
          _ptr(weight, table, dtype=e.store), _ptr(bias, "bias", True), _ptr(top0, "top0", dtype=e.store),
          _ptr(top1, "top1", dtype=e.store), wsp, wsb)
    return built


def _embed_backward_pair(e, index0, index1, top_diff0, top_diff1, weight_diff, bias_diff, shape, ws, indexed, index):
    """`indexed` false: the plain pair backward, with scratch from `ws`; true: the one that reads the built `index`."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), (shape if shape is not None else weight_diff.shape)
    if not indexed:
        symbol = "mms_embed_backward_pair_" + e.suffix
        wsp, wsb = _scratch(ws, _embed_workspace_bytes(e, M0 + M1, N), index0.device)
    elif index.buf is None:
        sfx = "" if e is _F32 else "_f16"
        raise MMSError("embed_backward_pair_indexed%s: no index was built (%s returned False); use embed_backward_pair%s"
                       % (sfx, "embed_forward_pair" if e is _F32 else "the pair forward", sfx))
    else:
        symbol = "mms_embed_backward_pair_indexed_" + e.suffix
        wsp, wsb = index.buf.data_ptr(), index.buf.numel()
    _call(symbol, M0, M1, N, K, _ptr(index0, "index0"), _ptr(top_diff0, "top_diff0", dtype=e.store),
          _ptr(index1, "index1"), _ptr(top_diff1, "top_diff1", dtype=e.store),
          _ptr(weight_diff, "weight_diff", True), _ptr(bias_diff, "bias_diff", True), wsp, wsb)


def embed_forward(index, weight, top, bias=None):
    _embed_forward(_F32, index, weight, "weight", top, bias)


def embed_forward_f64(index, weight, top, bias=None):
    _embed_forward(_F64, index, weight, "weight", top, bias)


def embed_forward_f16(index, table, top, bias=None):
    """embed_forward from a half table (K, N) into a half top (M, N); bias (N) float32 or None (mms_embed_forward_f16)."""
    _embed_forward(_F16_EMBED, index, table, "table", top, bias)


def embed_backward(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """weight_diff or bias_diff may be None; `shape` = (K, N) is then needed when weight_diff is None."""
    _embed_backward(_F32, index, top_diff, weight_diff, bias_diff, ws, shape)


def embed_backward_f64(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """weight_diff or bias_diff may be None; `shape` = (K, N) is then needed when weight_diff is None."""
    _embed_backward(_F64, index, top_diff, weight_diff, bias_diff, ws, shape)


def embed_backward_f16(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """embed_backward of a half top_diff (M, N) into float32 weight_diff / bias_diff (mms_embed_backward_f16)."""
    _embed_backward(_F16_EMBED, index, top_diff, weight_diff, bias_diff, ws, shape)


def embed_forward_pair(index0, index1, weight, top0, top1, bias=None, index=None):
    """top0 = Embed(index0), top1 = Embed(index1) in one launch; `index` (an EmbedPairIndex): also build the inverted
    index of the ids for embed_backward_pair.  Returns True if the index was built."""
    return _embed_forward_pair(_F32, index0, index1, weight, "weight", top0, top1, bias, index)


def embed_forward_pair_f16(index0, index1, table, top0, top1, bias=None, index=None):
    """embed_forward_pair from a half table into half tops; `index` (an EmbedPairIndex) as there.  Returns True if the
    index was built (mms_embed_forward_pair_f16)."""
    return _embed_forward_pair(_F16_EMBED, index0, index1, table, "table", top0, top1, bias, index)


def embed_backward_pair(index0, index1, top_diff0, top_diff1, weight_diff, bias_diff=None, ws=None, shape=None):
    """Backward of two Embed layers over one table in one pass: layer 0's rows, then layer 1's (include/mms.h).
    `shape` = (K, N) as in embed_backward."""
    _embed_backward_pair(_F32, index0, index1, top_diff0, top_diff1, weight_diff, bias_diff, shape, ws, False, None)


def embed_backward_pair_f16(index0, index1, top_diff0, top_diff1, weight_diff, bias_diff=None, ws=None, shape=None):
    """embed_backward_pair of two half top_diffs into float32 gradients (mms_embed_backward_pair_f16)."""
    _embed_backward_pair(_F16_EMBED, index0, index1, top_diff0, top_diff1, weight_diff, bias_diff, shape, ws, False,
                         None)


def embed_backward_pair_indexed(index0, index1, top_diff0, top_diff1, weight_diff, index, bias_diff=None, shape=None):
    """embed_backward_pair with the index embed_forward_pair(index0, index1, ..., index=index) built (same order)."""
    _embed_backward_pair(_F32, index0, index1, top_diff0, top_diff1, weight_diff, bias_diff, shape, None, True, index)


def embed_backward_pair_indexed_f16(index0, index1, top_diff0, top_diff1, weight_diff, index, bias_diff=None, shape=None):
    """embed_backward_pair_f16 with the index a pair forward (half or float32) built for (index0, index1)."""
    _embed_backward_pair(_F16_EMBED, index0, index1, top_diff0, top_diff1, weight_diff, bias_diff, shape, None, True,
                         index)


def feed_gather_rows(src, first, rows, dst, perm=None):
    """dst[i] = src[perm[first+i]] (perm int32 on the device, or None = identity)."""
    src_rows = src.shape[0]
    row_elems = src.numel() // max(src_rows, 1)
    _call("mms_feed_gather_rows_f32", rows, row_elems, src_rows, _ptr(src, "src"),
          _ptr(perm, "perm", True, dtype=torch.int32), first, _ptr(dst, "dst"))


class SimCrossArgs(C.Structure):
    """include/mms.h: mms_simcross_args_f32 -- the arguments of the SimCross forward / backward in one block."""
    _fields_ = [("dist_mode", C.c_int), ("N", C.c_int), ("W1", C.c_int), ("W2", C.c_int), ("D", C.c_int), ("M", C.c_int),
                ("q", C.c_void_p), ("a", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p),
                ("top", C.c_void_p), ("norm0", C.c_void_p), ("norm1", C.c_void_p),
                ("bias_term", C.c_int), ("propagate_down0", C.c_int), ("propagate_down1", C.c_int),
                ("top_diff", C.c_void_p), ("dq", C.c_void_p), ("da", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


def null_launch(workgroups=256):
    """An empty kernel of `workgroups` x 512 threads on the current stream (measurement aid: the launch floor)."""
    _call("mms_null_launch", int(workgroups))


# ---- arithmetic switches (include/mms.h: mms_set_*_mode / mms_get_*_mode) --------------------------------------
EUCLID_BWD_FP32, EUCLID_BWD_REFERENCE = 0, 1

# What a setter does with an argument that is not one of its names: _NAMES_ONLY looks everything up (KeyError for an
# int as for an unknown string); _NAMES_OR_INT looks a string up (KeyError if unknown) and hands anything else to
# int(); _ANYTHING hands whatever is not a name to int() and leaves the refusal to the library.
_NAMES_ONLY, _NAMES_OR_INT, _ANYTHING = range(3)

# (C symbol stem, the names in value order, the rule above, whether there is a get_*_mode, the setter's docstring)
_MODES = (
    ("matrix", ("bf16x3", "fp32"), _NAMES_ONLY, True,
     """"bf16x3" (default: exact three-way bf16 splits on the bf16 pipe) or "fp32" (fp32 MFMA); include/mms.h."""),
    ("euclid_backward", ("fp32", "reference"), _ANYTHING, True,
     """'fp32' (default: <= 2 ulp from the reference) or 'reference' (the reference's bits)."""),
    ("pairrank_hinge", ("cpu", "gpu"), _NAMES_OR_INT, True,
     """'cpu' (default): `ordered > 0` as PairRankLossLayer::Backward_cpu; 'gpu': `ordered >= 0` as the
    reference's .cu kernel.  Per calling thread."""),
    ("f16_distance", ("ordered", "tree"), _NAMES_OR_INT, False,
     """'ordered' (default): the reference's d-ascending fp32 sum, bit-identical scores; 'tree': fixed tree sum,
    ~1e-6 relative, no ordered chain.  Per calling thread; fp16-storage entry points only."""),
    ("rank_tie", ("input", "libstdcxx"), _NAMES_OR_INT, False,
     """'input' (default): equal scores keep the input order; 'libstdcxx': the order libstdc++'s std::sort leaves them in
    (include/mms.h: MMS_RANK_TIES_*)."""),
    ("loss_sum", ("fast", "reference"), _NAMES_OR_INT, False,
     """'fast' (default): order-free sum of the loss terms; 'reference': Forward_cpu's running fp32 sum, bit for bit
    (include/mms.h: MMS_LOSS_SUM_*)."""),
    ("triplet_finish", ("launch", "inlaunch"), _NAMES_OR_INT, False,
     """'inlaunch' (default): the loss is summed inside the step's one launch; 'launch': a second launch sums the terms
    (include/mms.h: MMS_TRIPLET_FINISH_*)."""),
)


def _mode_functions(stem, names, rule, doc):
    """(set_<stem>_mode, get_<stem>_mode) over mms_set_<stem>_mode / mms_get_<stem>_mode."""
    values = {name: value for value, name in enumerate(names)}
    set_symbol, get_symbol = "mms_set_%s_mode" % stem, "mms_get_%s_mode" % stem

    def setter(mode):
        if rule == _NAMES_ONLY or (rule == _NAMES_OR_INT and isinstance(mode, str)):
            m = values[mode]
        elif rule == _NAMES_OR_INT:
            m = int(mode)
        else:
            m = int(values.get(mode, mode))
        check(getattr(lib(), set_symbol)(m), set_symbol)

    def getter():
        return names[getattr(lib(), get_symbol)()]

    setter.__name__ = setter.__qualname__ = "set_%s_mode" % stem
    getter.__name__ = getter.__qualname__ = "get_%s_mode" % stem
    setter.__doc__ = doc
    return setter, getter


for _stem, _names, _rule, _has_getter, _doc in _MODES:
    _setter, _getter = _mode_functions(_stem, _names, _rule, _doc)
    globals()[_setter.__name__] = _setter
    if _has_getter:
        globals()[_getter.__name__] = _getter


# ---- the pooled stages' shared binding -------------------------------------------------------------------------
# _pooled.py is written against this module and conv.py, which both have to be whole before it loads: hence here.
from . import _pooled  # noqa: E402

# bn_pool_tanh_*, above; `lib` is looked up per call, like everywhere in this module
_BN_POOL = _pooled.Family("mms_bn_pool_tanh_", "BN + pooling", lambda: lib())
