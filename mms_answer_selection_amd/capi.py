"""ctypes binding of libmms_hip.so (include/mms.h) for torch device tensors.

torch is plumbing here: it owns device memory and the HIP stream; every
computation goes through the C ABI.  There is NO fallback: if the library is
missing or a tensor is not on the GPU the call raises.
"""
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


def lib():
    """The loaded C-ABI library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MMSError(
                "libmms_hip.so is not built (%s). Run `python -m mms_answer_selection_amd.build` "
                "or __graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the header and library diverge
            fn.restype = res
            fn.argtypes = args
        if l.mms_version() != MMS_VERSION:            # include/mms.h: a host built against another header must refuse
            raise MMSError("libmms_hip.so reports ABI version %d, this binding was written for %d: rebuild "
                           "(python -m mms_answer_selection_amd.build --force)" % (l.mms_version(), MMS_VERSION))
        _lib = l
    return _lib


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


def simcross_workspace_bytes(mode, N, W1, W2, D, M):
    return lib().mms_simcross_workspace_bytes(mode, N, W1, W2, D, M)


def simcross_forward(mode, q, a, top, W=None, bias=None, norm0=None, norm1=None, ws=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    M = W.shape[0] if mode == 2 else 1
    wsp, wsb = (ws or _default_ws).get(simcross_workspace_bytes(mode, N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_forward_f32(
        mode, N, W1, W2, D, M, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W", True),
        _ptr(bias, "bias", True), _ptr(top, "top"), _ptr(norm0, "norm0", True),
        _ptr(norm1, "norm1", True), wsp, wsb, _stream()), "mms_simcross_forward_f32")


def simcross_backward(mode, q, a, top, top_diff, dq, da, W=None, bias_term=False, norm0=None,
                      norm1=None, dW=None, dbias=None, propagate_down=(True, True), ws=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    M = W.shape[0] if mode == 2 else 1
    wsp, wsb = (ws or _default_ws).get(simcross_workspace_bytes(mode, N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_backward_f32(
        mode, N, W1, W2, D, M, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W", True), int(bool(bias_term)),
        _ptr(top, "top"), _ptr(top_diff, "top_diff"), _ptr(norm0, "norm0", True),
        _ptr(norm1, "norm1", True), int(bool(propagate_down[0])), int(bool(propagate_down[1])),
        _ptr(dq, "dq"), _ptr(da, "da"), _ptr(dW, "dW", True), _ptr(dbias, "dbias", True),
        wsp, wsb, _stream()), "mms_simcross_backward_f32")


def simcross_forward_backward(mode, q, a, top_diff, top, dq, da, W=None, bias=None, norm0=None,
                              norm1=None, dW=None, dbias=None, ws=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    M = W.shape[0] if mode == 2 else 1
    wsp, wsb = (ws or _default_ws).get(simcross_workspace_bytes(mode, N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_forward_backward_f32(
        mode, N, W1, W2, D, M, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W", True),
        _ptr(bias, "bias", True), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
        _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _ptr(dq, "dq"), _ptr(da, "da"),
        _ptr(dW, "dW", True), _ptr(dbias, "dbias", True), wsp, wsb, _stream()),
        "mms_simcross_forward_backward_f32")


def embed_simcross_forward(mode, index_q, index_a, weight, top, norm0=None, norm1=None, embed_bias=None):
    """top = SimCross(Embed(index_q), Embed(index_a)), dist_mode 0 / 1, the gather fused into the loads;
    embed_bias (D) = the Embed layers' bias blob, if they have one."""
    N, W1 = index_q.shape[0], index_q.shape[1]
    W2 = index_a.shape[1]
    K, D = weight.shape
    check(lib().mms_embed_simcross_forward_f32(
        mode, N, W1, W2, D, K, _ptr(index_q, "index_q"), _ptr(index_a, "index_a"), _ptr(weight, "weight"),
        _ptr(embed_bias, "embed_bias", True), _ptr(top, "top"), _ptr(norm0, "norm0", True),
        _ptr(norm1, "norm1", True), _stream()), "mms_embed_simcross_forward_f32")


def embed_simcross_bilinear_forward(index_q, index_a, weight, W, bias, top, embed_bias=None):
    """top (N,M,W1,W2) = SimCross dist_mode 2 of (Embed(index_q), Embed(index_a)), one launch (word grids)."""
    N, W1 = index_q.shape[0], index_q.shape[1]
    W2 = index_a.shape[1]
    K, D = weight.shape
    M = W.shape[0]
    check(lib().mms_embed_simcross_bilinear_forward_f32(
        N, W1, W2, D, M, K, _ptr(index_q, "index_q"), _ptr(index_a, "index_a"), _ptr(weight, "weight"),
        _ptr(embed_bias, "embed_bias", True), _ptr(W, "W"), _ptr(bias, "bias", True), _ptr(top, "top"), _stream()),
        "mms_embed_simcross_bilinear_forward_f32")


def simmatrix_forward(q, a, W, top, qw_scratch, ws=None, use_workspace=True):
    """With a workspace (the default one unless use_workspace=False) the call is mms_simmatrix_forward_ws_f32: Q.W on
    the bf16 matrix pipe at fp32 accuracy for N >= 2048 (include/mms.h); without, mms_simmatrix_forward_f32."""
    N = q.shape[0]
    K1, K2 = W.shape
    if not use_workspace:
        check(lib().mms_simmatrix_forward_f32(
            N, K1, K2, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W"), _ptr(top, "top"),
            _ptr(qw_scratch, "qw_scratch"), _stream()), "mms_simmatrix_forward_f32")
        return
    wsp, wsb = (ws or _default_ws).get(lib().mms_simmatrix_workspace_bytes(N, K1, K2), q.device)
    check(lib().mms_simmatrix_forward_ws_f32(
        N, K1, K2, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W"), _ptr(top, "top"),
        _ptr(qw_scratch, "qw_scratch"), wsp, wsb, _stream()), "mms_simmatrix_forward_ws_f32")


def simmatrix_forward_f16(q, a, W, top, ws=None):
    """fp16-storage scoring: q, a half tensors, W and top float32 (include/mms.h: mms_simmatrix_forward_f16)."""
    N = q.shape[0]
    K1, K2 = W.shape
    h = torch.float16
    wsp, wsb = (ws or _default_ws).get(lib().mms_simmatrix_workspace_bytes(N, K1, K2), q.device)
    check(lib().mms_simmatrix_forward_f16(N, K1, K2, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"),
                                          _ptr(top, "top"), wsp, wsb, _stream()), "mms_simmatrix_forward_f16")


def simmatrix_forward_train_f16(q, a, W, top, qw_scratch, ws=None):
    N = q.shape[0]
    K1, K2 = W.shape
    h = torch.float16
    wsp, wsb = (ws or _default_ws).get(lib().mms_simmatrix_workspace_bytes(N, K1, K2), q.device)
    check(lib().mms_simmatrix_forward_train_f16(N, K1, K2, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"),
                                                _ptr(top, "top"), _ptr(qw_scratch, "qw_scratch"), wsp, wsb, _stream()),
          "mms_simmatrix_forward_train_f16")


def simmatrix_backward_f16(q, a, W, qw, top_diff, dq, da, dW, ws=None):
    """dq, da: half tensors or None; dW: float32 (accumulated into) or None."""
    N = q.shape[0]
    K1, K2 = W.shape
    h = torch.float16
    wsp, wsb = (ws or _default_ws).get(lib().mms_simmatrix_workspace_bytes(N, K1, K2), q.device)
    check(lib().mms_simmatrix_backward_f16(N, K1, K2, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"),
                                           _ptr(qw, "qw", True), _ptr(top_diff, "top_diff"), _ptr(dq, "dq", True, h),
                                           _ptr(da, "da", True, h), _ptr(dW, "dW", True), wsp, wsb, _stream()),
          "mms_simmatrix_backward_f16")


def set_matrix_mode(mode):
    """"bf16x3" (default: exact three-way bf16 splits on the bf16 pipe) or "fp32" (fp32 MFMA); include/mms.h."""
    check(lib().mms_set_matrix_mode({"bf16x3": 0, "fp32": 1}[mode]), "mms_set_matrix_mode")


def get_matrix_mode():
    return ("bf16x3", "fp32")[lib().mms_get_matrix_mode()]


def simmatrix_backward(q, a, W, top_diff, dq, da, dW, param_propagate_down=True,
                       propagate_down=(True, True), ws=None, qw=None):
    """qw: the forward's qw_scratch (same q, W; may be `da` itself) -> the cached entry point."""
    N = q.shape[0]
    K1, K2 = W.shape
    wsp, wsb = (ws or _default_ws).get(lib().mms_simmatrix_workspace_bytes(N, K1, K2), q.device)
    if qw is not None:
        check(lib().mms_simmatrix_backward_cached_f32(
            N, K1, K2, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W"), _ptr(qw, "qw"), _ptr(top_diff, "top_diff"),
            int(bool(param_propagate_down)), int(bool(propagate_down[0])), int(bool(propagate_down[1])),
            _ptr(dq, "dq", True), _ptr(da, "da", True), _ptr(dW, "dW", True), wsp, wsb, _stream()),
            "mms_simmatrix_backward_cached_f32")
        return
    check(lib().mms_simmatrix_backward_f32(
        N, K1, K2, _ptr(q, "q"), _ptr(a, "a"), _ptr(W, "W"), _ptr(top_diff, "top_diff"),
        int(bool(param_propagate_down)), int(bool(propagate_down[0])), int(bool(propagate_down[1])),
        _ptr(dq, "dq", True), _ptr(da, "da", True), _ptr(dW, "dW", True), wsp, wsb, _stream()),
        "mms_simmatrix_backward_f32")


def pairrank_forward(a, b, y, ordered, similar, loss, margin=1.0, ws=None):
    count = a.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_pairrank_workspace_bytes(count), a.device)
    check(lib().mms_pairrank_forward_f32(
        count, float(margin), _ptr(a, "a"), _ptr(b, "b"), _ptr(y, "y"), _ptr(ordered, "ordered"),
        _ptr(similar, "similar"), _ptr(loss, "loss"), wsp, wsb, _stream()),
        "mms_pairrank_forward_f32")


def pairrank_backward(y, ordered, similar, da, db, top_diff=1.0, propagate_down=(True, True)):
    check(lib().mms_pairrank_backward_f32(
        y.numel(), float(top_diff), _ptr(y, "y"), _ptr(ordered, "ordered"),
        _ptr(similar, "similar"), int(bool(propagate_down[0])), int(bool(propagate_down[1])),
        _ptr(da, "da", True), _ptr(db, "db", True), _stream()), "mms_pairrank_backward_f32")


def fm_forward(x, top, bias=None):
    """FM pooling (include/mms.h: mms_fm_forward_f32).  x (N, C, dim); top N floats; bias one float or None."""
    N, C, dim = x.shape
    check(lib().mms_fm_forward_f32(N, C, dim, _ptr(x, "x"), _ptr(bias, "bias", True), _ptr(top, "top"), _stream()),
          "mms_fm_forward_f32")


def fm_backward(x, top_diff, bottom_diff=None, bias_diff=None):
    """bottom_diff None = propagate_down[0] false; bias_diff None = no bias term or param_propagate_down false.
    Both are overwritten."""
    N, C, dim = x.shape
    check(lib().mms_fm_backward_f32(
        N, C, dim, _ptr(x, "x"), _ptr(top_diff, "top_diff"), _ptr(bottom_diff, "bottom_diff", True),
        _ptr(bias_diff, "bias_diff", True), _stream()), "mms_fm_backward_f32")


def fm_forward_backward(x, top_diff, top, bottom_diff, bias=None, bias_diff=None):
    N, C, dim = x.shape
    check(lib().mms_fm_forward_backward_f32(
        N, C, dim, _ptr(x, "x"), _ptr(bias, "bias", True), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
        _ptr(bottom_diff, "bottom_diff"), _ptr(bias_diff, "bias_diff", True), _stream()),
        "mms_fm_forward_backward_f32")


def _bn_shape(x):
    """(N, C, S) of a blob (N, C, S) or (N, C, H, W): S is everything after the channel axis."""
    if x.dim() < 2:
        raise MMSArgumentError("BN: x must be (N, C, ...), got %s" % (tuple(x.shape),))
    S = 1
    for d in x.shape[2:]:
        S *= int(d)
    return int(x.shape[0]), int(x.shape[1]), S


def bn_workspace_bytes(N, C, S):
    """0 where one workgroup per channel serves (include/mms.h: mms_bn_workspace_bytes)."""
    return lib().mms_bn_workspace_bytes(N, C, S)


def bn_workspace_bytes_f64(N, C, S):
    return lib().mms_bn_workspace_bytes_f64(N, C, S)


def _bn_forward(suffix, dt, query, x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase,
                bn_memory, ws):
    N, C, S = _bn_shape(x)
    wsp, wsb = (ws or _default_ws).get(query(N, C, S), x.device)
    name = "mms_bn_forward_" + suffix
    check(getattr(lib(), name)(
        int(phase), N, C, S, float(bn_memory), _ptr(x, "x", dtype=dt), _ptr(scale, "scale", dtype=dt),
        _ptr(shift, "shift", dtype=dt), _ptr(running_mean, "running_mean", dtype=dt),
        _ptr(running_var, "running_var", dtype=dt), _ptr(top, "top", dtype=dt), _ptr(save_mean, "save_mean", dtype=dt),
        _ptr(save_std, "save_std", dtype=dt), wsp, wsb, _stream()), name)


def _bn_backward(suffix, dt, query, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws):
    N, C, S = _bn_shape(x)
    wsp, wsb = (ws or _default_ws).get(query(N, C, S), x.device)
    name = "mms_bn_backward_" + suffix
    check(getattr(lib(), name)(
        N, C, S, _ptr(x, "x", dtype=dt), _ptr(top_diff, "top_diff", dtype=dt), _ptr(scale, "scale", dtype=dt),
        _ptr(save_mean, "save_mean", dtype=dt), _ptr(save_std, "save_std", dtype=dt),
        _ptr(bottom_diff, "bottom_diff", True, dt), _ptr(scale_diff, "scale_diff", True, dt),
        _ptr(shift_diff, "shift_diff", True, dt), wsp, wsb, _stream()), name)


def bn_forward(x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase=0, bn_memory=0.9, ws=None):
    """BN forward (include/mms.h: mms_bn_forward_f32).  x, top (N, C, S) or (N, C, H, W); the other six C floats.
    phase 0 = TRAIN (batch statistics; the running blobs are updated in place), 1 = TEST (running statistics, read
    only).  save_mean / save_std are what bn_backward needs."""
    _bn_forward("f32", torch.float32, bn_workspace_bytes, x, scale, shift, running_mean, running_var, top, save_mean,
                save_std, phase, bn_memory, ws)


def bn_backward(x, top_diff, scale, save_mean, save_std, bottom_diff=None, scale_diff=None, shift_diff=None, ws=None):
    """Each of bottom_diff, scale_diff, shift_diff may be None (skipped); those given are overwritten."""
    _bn_backward("f32", torch.float32, bn_workspace_bytes, x, top_diff, scale, save_mean, save_std, bottom_diff,
                 scale_diff, shift_diff, ws)


def _bn_pool_shape(x, kernel):
    """(N, C, H, W, kh, kw) of a 4-D blob and a pooling kernel (k or (kh, kw))."""
    if x.dim() != 4:
        raise MMSArgumentError("BN + pooling: x must be (N, C, H, W), got %s" % (tuple(x.shape),))
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    return tuple(int(d) for d in x.shape) + (int(kh), int(kw))


def bn_pool_tanh_workspace_bytes(N, C, H, W, kh, kw):
    """0 where one workgroup per channel serves (include/mms.h: mms_bn_pool_tanh_workspace_bytes)."""
    return lib().mms_bn_pool_tanh_workspace_bytes(N, C, H, W, kh, kw)


def bn_pool_tanh_workspace_bytes_f64(N, C, H, W, kh, kw):
    return lib().mms_bn_pool_tanh_workspace_bytes_f64(N, C, H, W, kh, kw)


def _bn_pool_tanh_forward(suffix, dt, query, x, kernel, scale, shift, running_mean, running_var, top, save_pool,
                          save_mean, save_std, phase, bn_memory, ws):
    dims = _bn_pool_shape(x, kernel)
    wsp, wsb = (ws or _default_ws).get(query(*dims), x.device)
    name = "mms_bn_pool_tanh_forward_" + suffix
    check(getattr(lib(), name)(
        int(phase), *dims, float(bn_memory), _ptr(x, "x", dtype=dt), _ptr(scale, "scale", dtype=dt),
        _ptr(shift, "shift", dtype=dt), _ptr(running_mean, "running_mean", dtype=dt),
        _ptr(running_var, "running_var", dtype=dt), _ptr(top, "top", dtype=dt), _ptr(save_pool, "save_pool", dtype=dt),
        _ptr(save_mean, "save_mean", dtype=dt), _ptr(save_std, "save_std", dtype=dt), wsp, wsb, _stream()), name)


def _bn_pool_tanh_backward(suffix, dt, query, x, kernel, top, top_diff, save_pool, scale, save_mean, save_std,
                           bottom_diff, scale_diff, shift_diff, ws):
    dims = _bn_pool_shape(x, kernel)
    wsp, wsb = (ws or _default_ws).get(query(*dims), x.device)
    name = "mms_bn_pool_tanh_backward_" + suffix
    check(getattr(lib(), name)(
        *dims, _ptr(x, "x", dtype=dt), _ptr(top, "top", dtype=dt), _ptr(top_diff, "top_diff", dtype=dt),
        _ptr(save_pool, "save_pool", dtype=dt), _ptr(scale, "scale", dtype=dt), _ptr(save_mean, "save_mean", dtype=dt),
        _ptr(save_std, "save_std", dtype=dt), _ptr(bottom_diff, "bottom_diff", True, dt),
        _ptr(scale_diff, "scale_diff", True, dt), _ptr(shift_diff, "shift_diff", True, dt), wsp, wsb, _stream()), name)


def bn_pool_tanh_forward(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                         phase=0, bn_memory=0.9, ws=None):
    """BN -> AvePool(kernel = stride, windows tile the map) -> TanH (include/mms.h: mms_bn_pool_tanh_forward_f32).
    x (N, C, H, W); kernel k or (kh, kw); top, save_pool (N, C, H/kh, W/kw); the other six C floats.  phase as in
    bn_forward.  save_pool, save_mean, save_std and top are what bn_pool_tanh_backward needs."""
    _bn_pool_tanh_forward("f32", torch.float32, bn_pool_tanh_workspace_bytes, x, kernel, scale, shift, running_mean,
                          running_var, top, save_pool, save_mean, save_std, phase, bn_memory, ws)


def bn_pool_tanh_backward(x, kernel, top, top_diff, save_pool, scale, save_mean, save_std, bottom_diff=None,
                          scale_diff=None, shift_diff=None, ws=None):
    """Each of bottom_diff (N, C, H, W), scale_diff, shift_diff (C) may be None (skipped); those given are
    overwritten."""
    _bn_pool_tanh_backward("f32", torch.float32, bn_pool_tanh_workspace_bytes, x, kernel, top, top_diff, save_pool,
                           scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws)


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
            check(lib().mms_triplet_workspace_init(self.buf.data_ptr(), self.buf.numel(), _stream()),
                  "mms_triplet_workspace_init")


_default_triplet_ws = {}


def triplet_euclid_step(q, a_pos, a_neg, y, s_pos, s_neg, loss, dq, da_pos, da_neg, margin=1.0,
                        loss_weight=1.0, ws=None):
    """`ws`: a TripletWorkspace; calls that may be in flight together (streams, concurrently replayed graphs) must
    not share one.  Default: one per device."""
    N, D = q.shape[0], q.shape[-1]
    if ws is None:
        ws = _default_triplet_ws.setdefault(q.device, TripletWorkspace())
    if not isinstance(ws, TripletWorkspace):
        raise TypeError("triplet_euclid_step needs a capi.TripletWorkspace (its arrival words must stay zero "
                        "between launches; a general Workspace is overwritten by other calls)")
    wsp, wsb = ws.get(lib().mms_triplet_workspace_bytes(N), q.device)
    check(lib().mms_triplet_euclid_step_f32(
        N, D, float(margin), float(loss_weight), _ptr(q, "q"), _ptr(a_pos, "a_pos"),
        _ptr(a_neg, "a_neg"), _ptr(y, "y"), _ptr(s_pos, "s_pos"), _ptr(s_neg, "s_neg"),
        _ptr(loss, "loss", True), _ptr(dq, "dq"), _ptr(da_pos, "da_pos"), _ptr(da_neg, "da_neg"),
        wsp, wsb, _stream()), "mms_triplet_euclid_step_f32")


def triplet_cosine_step(q, a_pos, a_neg, y, s_pos, s_neg, loss, dq, da_pos, da_neg, margin=1.0,
                        loss_weight=1.0, norms=None, ws=None):
    """The fused cosine step (include/mms.h: mms_triplet_cosine_step_f32).  `norms`: None, or (norm_q, norm_pos,
    norm_neg) tensors of N floats, any of which may be None.  `ws`: a TripletWorkspace, as for triplet_euclid_step."""
    N, D = q.shape[0], q.shape[-1]
    if ws is None:
        ws = _default_triplet_ws.setdefault(q.device, TripletWorkspace())
    if not isinstance(ws, TripletWorkspace):
        raise TypeError("triplet_cosine_step needs a capi.TripletWorkspace (its arrival words must stay zero "
                        "between launches; a general Workspace is overwritten by other calls)")
    nq, npos, nneg = norms if norms is not None else (None, None, None)
    wsp, wsb = ws.get(lib().mms_triplet_workspace_bytes(N), q.device)
    check(lib().mms_triplet_cosine_step_f32(
        N, D, float(margin), float(loss_weight), _ptr(q, "q"), _ptr(a_pos, "a_pos"),
        _ptr(a_neg, "a_neg"), _ptr(y, "y"), _ptr(s_pos, "s_pos"), _ptr(s_neg, "s_neg"),
        _ptr(nq, "norm_q", True), _ptr(npos, "norm_pos", True), _ptr(nneg, "norm_neg", True),
        _ptr(loss, "loss", True), _ptr(dq, "dq"), _ptr(da_pos, "da_pos"), _ptr(da_neg, "da_neg"),
        wsp, wsb, _stream()), "mms_triplet_cosine_step_f32")


def triplet_simmatrix_step(q, a_pos, a_neg, y, W, s_pos, s_neg, loss, dq, da_pos, da_neg, dW, margin=1.0,
                           loss_weight=1.0, ws=None):
    """The fused learned-metric step (include/mms.h: mms_triplet_simmatrix_step_f32).  dW is ACCUMULATED into."""
    N, K1 = q.shape
    K2 = a_pos.shape[1]
    wsp, wsb = (ws or _default_ws).get(lib().mms_triplet_simmatrix_workspace_bytes(N, K1, K2), q.device)
    check(lib().mms_triplet_simmatrix_step_f32(
        N, K1, K2, float(margin), float(loss_weight), _ptr(q, "q"), _ptr(a_pos, "a_pos"), _ptr(a_neg, "a_neg"),
        _ptr(y, "y"), _ptr(W, "W"), _ptr(s_pos, "s_pos"), _ptr(s_neg, "s_neg"), _ptr(loss, "loss", True),
        _ptr(dq, "dq"), _ptr(da_pos, "da_pos"), _ptr(da_neg, "da_neg"), _ptr(dW, "dW"), wsp, wsb, _stream()),
        "mms_triplet_simmatrix_step_f32")


def rank_map_mrr(prob, label, group, fixed_axis=1, ws=None):
    """-> (MAP, MRR, effective groups) as Python numbers (device -> host copy of 3 scalars)."""
    n = label.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes(n), prob.device)
    out = torch.empty(2, dtype=torch.float32, device=prob.device)
    eff = torch.empty(1, dtype=torch.int32, device=prob.device)
    check(lib().mms_rank_map_mrr_f32(
        n, int(fixed_axis), _ptr(prob, "prob"), _ptr(label, "label"), _ptr(group, "group"),
        out.data_ptr(), out.data_ptr() + 4, eff.data_ptr(), wsp, wsb, _stream()), "mms_rank_map_mrr_f32")
    o = out.cpu().numpy()
    return o[0], o[1], int(eff.item())


def rank_map_mrr_device(prob, label, group, out, eff, fixed_axis=1, ws=None):
    """The same with the results left on the device: out (2 floats: MAP, MRR), eff (1 int32); no host sync."""
    n = label.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes(n), prob.device)
    check(lib().mms_rank_map_mrr_f32(
        n, int(fixed_axis), _ptr(prob, "prob"), _ptr(label, "label"), _ptr(group, "group"),
        out.data_ptr(), out.data_ptr() + 4, eff.data_ptr(), wsp, wsb, _stream()), "mms_rank_map_mrr_f32")


def rank_auc(prob, label, fixed_axis=1, ignore_label=None, ws=None):
    n = label.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes(n), prob.device)
    out = torch.empty(1, dtype=torch.float32, device=prob.device)
    check(lib().mms_rank_auc_f32(
        n, int(prob.shape[1]), int(fixed_axis), _ptr(prob, "prob"), _ptr(label, "label"),
        int(ignore_label is not None), int(ignore_label or 0), out.data_ptr(), wsp, wsb, _stream()),
        "mms_rank_auc_f32")
    return out.cpu().numpy()[0]


def rank_auc_nd(prob, label, axis=1, fixed_axis=1, ignore_label=None, ws=None):
    """AUC layer for any label axis: prob (..., C, ...) with `axis` the class axis, label of the remaining shape."""
    shape = tuple(prob.shape)
    axis = axis % len(shape)
    outer = int(np.prod(shape[:axis])) if axis else 1
    inner = int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
    n = outer * inner
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes(n), prob.device)
    out = torch.empty(1, dtype=torch.float32, device=prob.device)
    check(lib().mms_rank_auc_nd_f32(
        outer, int(shape[axis]), inner, int(fixed_axis), _ptr(prob, "prob"), _ptr(label, "label"),
        int(ignore_label is not None), int(ignore_label or 0), out.data_ptr(), wsp, wsb, _stream()),
        "mms_rank_auc_nd_f32")
    return out.cpu().numpy()[0]


def rank_accuracy(a, b, label, ws=None):
    n = a.numel()
    wsp, wsb = (ws or _default_ws).get(max(4096, lib().mms_rank_workspace_bytes(1)), a.device)
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(lib().mms_rank_accuracy_f32(n, _ptr(a, "a"), _ptr(b, "b"), _ptr(label, "label"),
                                      out.data_ptr(), wsp, wsb, _stream()), "mms_rank_accuracy_f32")
    return out.cpu().numpy()[0]


def simcross_euclid_forward_f16(q, a, top):
    """fp16-storage scoring (cfg 5): q, a half tensors (N,1,D); top float32."""
    N, D = q.shape[0], q.shape[-1]
    h = torch.float16
    check(lib().mms_simcross_euclid_forward_f16(N, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h),
                                                _ptr(top, "top"), _stream()),
          "mms_simcross_euclid_forward_f16")


def simcross_euclid_forward_backward_f16(q, a, top_diff, top, dq, da):
    N, D = q.shape[0], q.shape[-1]
    h = torch.float16
    check(lib().mms_simcross_euclid_forward_backward_f16(
        N, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top_diff, "top_diff"),
        _ptr(top, "top"), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h), _stream()),
        "mms_simcross_euclid_forward_backward_f16")


def simcross_cosine_forward_backward_f16(q, a, top_diff, top, dq, da, norm0=None, norm1=None):
    N, D = q.shape[0], q.shape[-1]
    h = torch.float16
    check(lib().mms_simcross_cosine_forward_backward_f16(
        N, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
        _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h),
        _stream()), "mms_simcross_cosine_forward_backward_f16")


def simcross_cosine_forward_f16(q, a, top, norm0=None, norm1=None):
    N, D = q.shape[0], q.shape[-1]
    h = torch.float16
    check(lib().mms_simcross_cosine_forward_f16(N, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top, "top"),
                                                _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _stream()),
          "mms_simcross_cosine_forward_f16")


def _grid_f16_shape(q, a):
    """(N, W1, W2, D) of half word grids q (N, W1, D), a (N, W2, D)."""
    if q.dim() != 3 or a.dim() != 3 or q.shape[0] != a.shape[0] or q.shape[2] != a.shape[2]:
        raise MMSError("q (N, W1, D) and a (N, W2, D) expected, got %s and %s" % (tuple(q.shape), tuple(a.shape)))
    return q.shape[0], q.shape[1], a.shape[1], q.shape[2]


def _expect_shape(t, shape, name):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise MMSError("%s must have shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))


def simcross_forward_f16(mode, q, a, top, norm0=None, norm1=None):
    """fp16-storage SimCross forward on word grids, dist_mode 0 / 1 (include/mms.h: mms_simcross_forward_f16): q, a half
    tensors; top (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2) float32, the norms for dist_mode 0 only."""
    N, W1, W2, D = _grid_f16_shape(q, a)
    h = torch.float16
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    check(lib().mms_simcross_forward_f16(mode, N, W1, W2, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top, "top"),
                                         _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _stream()),
          "mms_simcross_forward_f16")


def simcross_backward_f16(mode, q, a, top, top_diff, dq, da, norm0=None, norm1=None):
    """The backward of simcross_forward_f16: dq, da half tensors shaped like q, a (mms_simcross_backward_f16)."""
    N, W1, W2, D = _grid_f16_shape(q, a)
    h = torch.float16
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(top_diff, (N, 1, W1, W2), "top_diff")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    check(lib().mms_simcross_backward_f16(
        mode, N, W1, W2, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top, "top"), _ptr(top_diff, "top_diff"),
        _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h), _stream()),
        "mms_simcross_backward_f16")


def simcross_forward_backward_f16(mode, q, a, top_diff, top, dq, da, norm0=None, norm1=None):
    """simcross_forward_f16 then simcross_backward_f16 in one call (mms_simcross_forward_backward_f16)."""
    N, W1, W2, D = _grid_f16_shape(q, a)
    h = torch.float16
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(top_diff, (N, 1, W1, W2), "top_diff")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    check(lib().mms_simcross_forward_backward_f16(
        mode, N, W1, W2, D, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(top_diff, "top_diff"), _ptr(top, "top"),
        _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h), _stream()),
        "mms_simcross_forward_backward_f16")


def simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M):
    return lib().mms_simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M)


def _bilinear_f16_shape(q, a, W, bias, dbias=None):
    N, W1, W2, D = _grid_f16_shape(q, a)
    if W is None or W.dim() != 3 or tuple(W.shape[1:]) != (D, D):
        raise MMSError("W (M, D, D) expected with D = %d, got %s" % (D, None if W is None else tuple(W.shape)))
    M = W.shape[0]
    _expect_shape(bias, (M, W1, W2), "bias")
    _expect_shape(dbias, (M, W1, W2), "dbias")
    return N, W1, W2, D, M


def simcross_bilinear_forward_f16(q, a, W, bias, top, ws=None):
    """fp16-storage SimCross dist_mode 2 on word grids (include/mms.h: mms_simcross_bilinear_forward_f16): q (N, W1, D), a (N, W2, D)
    half tensors; W (M, D, D), bias (M, W1, W2) or None and top (N, M, W1, W2) float32."""
    N, W1, W2, D, M = _bilinear_f16_shape(q, a, W, bias)
    h = torch.float16
    _expect_shape(top, (N, M, W1, W2), "top")
    wsp, wsb = (ws or _default_ws).get(simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_bilinear_forward_f16(
        N, W1, W2, D, M, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"), _ptr(bias, "bias", True), _ptr(top, "top"),
        wsp, wsb, _stream()), "mms_simcross_bilinear_forward_f16")


def simcross_bilinear_backward_f16(q, a, W, top_diff, dq, da, dW, dbias=None, ws=None):
    """The backward of simcross_bilinear_forward_f16: dq, da half tensors shaped like q, a; dW like W (overwritten); dbias
    (M, W1, W2) float32 is accumulated into, None = no bias term (mms_simcross_bilinear_backward_f16)."""
    N, W1, W2, D, M = _bilinear_f16_shape(q, a, W, None, dbias)
    h = torch.float16
    _expect_shape(top_diff, (N, M, W1, W2), "top_diff")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    _expect_shape(dW, W.shape, "dW")
    wsp, wsb = (ws or _default_ws).get(simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_bilinear_backward_f16(
        N, W1, W2, D, M, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"), int(dbias is not None),
        _ptr(top_diff, "top_diff"), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h), _ptr(dW, "dW"), _ptr(dbias, "dbias", True),
        wsp, wsb, _stream()), "mms_simcross_bilinear_backward_f16")


def simcross_bilinear_forward_backward_f16(q, a, W, bias, top_diff, top, dq, da, dW, dbias=None, ws=None):
    """simcross_bilinear_forward_f16 then simcross_bilinear_backward_f16 in one call; the bias term is `bias is not None`, and
    then dbias is required (mms_simcross_bilinear_forward_backward_f16)."""
    N, W1, W2, D, M = _bilinear_f16_shape(q, a, W, bias, dbias)
    h = torch.float16
    _expect_shape(top, (N, M, W1, W2), "top")
    _expect_shape(top_diff, (N, M, W1, W2), "top_diff")
    _expect_shape(dq, q.shape, "dq")
    _expect_shape(da, a.shape, "da")
    _expect_shape(dW, W.shape, "dW")
    wsp, wsb = (ws or _default_ws).get(simcross_bilinear_workspace_bytes_f16(N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_bilinear_forward_backward_f16(
        N, W1, W2, D, M, _ptr(q, "q", dtype=h), _ptr(a, "a", dtype=h), _ptr(W, "W"), _ptr(bias, "bias", True),
        _ptr(top_diff, "top_diff"), _ptr(top, "top"), _ptr(dq, "dq", dtype=h), _ptr(da, "da", dtype=h), _ptr(dW, "dW"),
        _ptr(dbias, "dbias", True), wsp, wsb, _stream()), "mms_simcross_bilinear_forward_backward_f16")


def embed_simcross_bilinear_forward_f16(index_q, index_a, table, W, bias, top, embed_bias=None):
    """embed_simcross_bilinear_forward from a half table (K, D): index_q (N, W1), index_a (N, W2) float32 ids, W (M, D, D), bias
    (M, W1, W2) or None, embed_bias (D) or None, top (N, M, W1, W2) float32 (mms_embed_simcross_bilinear_forward_f16)."""
    if index_q.dim() != 2 or index_a.dim() != 2 or index_q.shape[0] != index_a.shape[0] or table.dim() != 2:
        raise MMSError("index_q (N, W1), index_a (N, W2) and table (K, D) expected, got %s, %s and %s"
                       % (tuple(index_q.shape), tuple(index_a.shape), tuple(table.shape)))
    N, W1 = index_q.shape
    W2 = index_a.shape[1]
    K, D = table.shape
    if W is None or W.dim() != 3 or tuple(W.shape[1:]) != (D, D):
        raise MMSError("W (M, D, D) expected with D = %d, got %s" % (D, None if W is None else tuple(W.shape)))
    M = W.shape[0]
    _expect_shape(bias, (M, W1, W2), "bias")
    _expect_shape(embed_bias, (D,), "embed_bias")
    _expect_shape(top, (N, M, W1, W2), "top")
    check(lib().mms_embed_simcross_bilinear_forward_f16(
        N, W1, W2, D, M, K, _ptr(index_q, "index_q"), _ptr(index_a, "index_a"), _ptr(table, "table", dtype=torch.float16),
        _ptr(embed_bias, "embed_bias", True), _ptr(W, "W"), _ptr(bias, "bias", True), _ptr(top, "top"), _stream()),
        "mms_embed_simcross_bilinear_forward_f16")


def embed_simcross_forward_f16(mode, index_q, index_a, table, top, norm0=None, norm1=None, embed_bias=None):
    """embed_simcross_forward from a half table (K, D), dist_mode 0 / 1: index_q (N, W1), index_a (N, W2) float32 ids, embed_bias (D)
    or None, top (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2) float32, the norms for dist_mode 0 only
    (mms_embed_simcross_forward_f16).  A table that is not half, or index_q and index_a of different batch sizes: ValueError."""
    if index_q.dim() != 2 or index_a.dim() != 2 or index_q.shape[0] != index_a.shape[0] or table.dim() != 2:
        raise MMSArgumentError("index_q (N, W1), index_a (N, W2) and table (K, D) expected, got %s, %s and %s"
                               % (tuple(index_q.shape), tuple(index_a.shape), tuple(table.shape)))
    if table.dtype != torch.float16:
        raise MMSArgumentError("table must be torch.float16 (got %s); an fp32 table goes to embed_simcross_forward" % table.dtype)
    N, W1 = index_q.shape
    W2 = index_a.shape[1]
    K, D = table.shape
    _expect_shape(embed_bias, (D,), "embed_bias")
    _expect_shape(top, (N, 1, W1, W2), "top")
    _expect_shape(norm0, (N, W1), "norm0")
    _expect_shape(norm1, (N, W2), "norm1")
    check(lib().mms_embed_simcross_forward_f16(
        mode, N, W1, W2, D, K, _ptr(index_q, "index_q"), _ptr(index_a, "index_a"), _ptr(table, "table", dtype=torch.float16),
        _ptr(embed_bias, "embed_bias", True), _ptr(top, "top"), _ptr(norm0, "norm0", True), _ptr(norm1, "norm1", True), _stream()),
        "mms_embed_simcross_forward_f16")


def embed_forward(index, weight, top, bias=None):
    M, (K, N) = index.numel(), weight.shape
    check(lib().mms_embed_forward_f32(M, N, K, _ptr(index, "index"), _ptr(weight, "weight"),
                                      _ptr(bias, "bias", True), _ptr(top, "top"), _stream()),
          "mms_embed_forward_f32")


def embed_backward(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """weight_diff or bias_diff may be None; `shape` = (K, N) is then needed when weight_diff is None."""
    M, (K, N) = index.numel(), (shape if shape is not None else weight_diff.shape)
    wsp, wsb = (ws or _default_ws).get(lib().mms_embed_workspace_bytes(M, N), index.device)
    check(lib().mms_embed_backward_f32(M, N, K, _ptr(index, "index"), _ptr(top_diff, "top_diff"),
                                       _ptr(weight_diff, "weight_diff", True),
                                       _ptr(bias_diff, "bias_diff", True), wsp, wsb, _stream()),
          "mms_embed_backward_f32")


def embed_backward_pair(index0, index1, top_diff0, top_diff1, weight_diff, bias_diff=None, ws=None, shape=None):
    """Backward of two Embed layers over one table in one pass: layer 0's rows, then layer 1's (include/mms.h).
    `shape` = (K, N) as in embed_backward."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), (shape if shape is not None else weight_diff.shape)
    wsp, wsb = (ws or _default_ws).get(lib().mms_embed_workspace_bytes(M0 + M1, N), index0.device)
    check(lib().mms_embed_backward_pair_f32(M0, M1, N, K, _ptr(index0, "index0"), _ptr(top_diff0, "top_diff0"),
                                            _ptr(index1, "index1"), _ptr(top_diff1, "top_diff1"),
                                            _ptr(weight_diff, "weight_diff", True), _ptr(bias_diff, "bias_diff", True),
                                            wsp, wsb, _stream()), "mms_embed_backward_pair_f32")


class EmbedPairIndex:
    """The inverted index of two Embed layers' word ids, built by embed_forward_pair and consumed by
    embed_backward_pair(index=...): its own buffer (nothing else may write it between the two calls)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.buf.data_ptr(), self.buf.numel()


def embed_forward_pair(index0, index1, weight, top0, top1, bias=None, index=None):
    """top0 = Embed(index0), top1 = Embed(index1) in one launch; `index` (an EmbedPairIndex): also build the inverted
    index of the ids for embed_backward_pair.  Returns True if the index was built."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), weight.shape
    wsp, wsb, built = None, 0, False
    if index is not None and lib().mms_embed_pair_index_supported(M0, M1, K):
        wsp, wsb = index.get(lib().mms_embed_workspace_bytes(M0 + M1, N), index0.device)
        built = True
    check(lib().mms_embed_forward_pair_f32(M0, M1, N, K, _ptr(index0, "index0"), _ptr(index1, "index1"),
                                           _ptr(weight, "weight"), _ptr(bias, "bias", True), _ptr(top0, "top0"),
                                           _ptr(top1, "top1"), wsp, wsb, _stream()), "mms_embed_forward_pair_f32")
    return built


def embed_backward_pair_indexed(index0, index1, top_diff0, top_diff1, weight_diff, index, bias_diff=None, shape=None):
    """embed_backward_pair with the index embed_forward_pair(index0, index1, ..., index=index) built (same order)."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), (shape if shape is not None else weight_diff.shape)
    if index.buf is None:
        raise MMSError("embed_backward_pair_indexed: no index was built (embed_forward_pair returned False); use "
                       "embed_backward_pair")
    check(lib().mms_embed_backward_pair_indexed_f32(M0, M1, N, K, _ptr(index0, "index0"), _ptr(top_diff0, "top_diff0"),
                                                    _ptr(index1, "index1"), _ptr(top_diff1, "top_diff1"),
                                                    _ptr(weight_diff, "weight_diff", True), _ptr(bias_diff, "bias_diff", True),
                                                    index.buf.data_ptr(), index.buf.numel(), _stream()),
          "mms_embed_backward_pair_indexed_f32")


# ---- fp16-storage Embed: half table / top / top_diff, float32 ids, bias and (master) gradients.  The workspace and the
# EmbedPairIndex are those of the float32 calls: an index built by either pair forward serves either indexed backward.
_H = torch.float16


def embed_forward_f16(index, table, top, bias=None):
    """embed_forward from a half table (K, N) into a half top (M, N); bias (N) float32 or None (mms_embed_forward_f16)."""
    M, (K, N) = index.numel(), table.shape
    check(lib().mms_embed_forward_f16(M, N, K, _ptr(index, "index"), _ptr(table, "table", dtype=_H),
                                      _ptr(bias, "bias", True), _ptr(top, "top", dtype=_H), _stream()),
          "mms_embed_forward_f16")


def embed_backward_f16(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """embed_backward of a half top_diff (M, N) into float32 weight_diff / bias_diff (mms_embed_backward_f16)."""
    M, (K, N) = index.numel(), (shape if shape is not None else weight_diff.shape)
    wsp, wsb = (ws or _default_ws).get(lib().mms_embed_workspace_bytes(M, N), index.device)
    check(lib().mms_embed_backward_f16(M, N, K, _ptr(index, "index"), _ptr(top_diff, "top_diff", dtype=_H),
                                       _ptr(weight_diff, "weight_diff", True),
                                       _ptr(bias_diff, "bias_diff", True), wsp, wsb, _stream()),
          "mms_embed_backward_f16")


def embed_backward_pair_f16(index0, index1, top_diff0, top_diff1, weight_diff, bias_diff=None, ws=None, shape=None):
    """embed_backward_pair of two half top_diffs into float32 gradients (mms_embed_backward_pair_f16)."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), (shape if shape is not None else weight_diff.shape)
    wsp, wsb = (ws or _default_ws).get(lib().mms_embed_workspace_bytes(M0 + M1, N), index0.device)
    check(lib().mms_embed_backward_pair_f16(M0, M1, N, K, _ptr(index0, "index0"), _ptr(top_diff0, "top_diff0", dtype=_H),
                                            _ptr(index1, "index1"), _ptr(top_diff1, "top_diff1", dtype=_H),
                                            _ptr(weight_diff, "weight_diff", True), _ptr(bias_diff, "bias_diff", True),
                                            wsp, wsb, _stream()), "mms_embed_backward_pair_f16")


def embed_forward_pair_f16(index0, index1, table, top0, top1, bias=None, index=None):
    """embed_forward_pair from a half table into half tops; `index` (an EmbedPairIndex) as there.  Returns True if the
    index was built (mms_embed_forward_pair_f16)."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), table.shape
    wsp, wsb, built = None, 0, False
    if index is not None and lib().mms_embed_pair_index_supported(M0, M1, K):
        wsp, wsb = index.get(lib().mms_embed_workspace_bytes(M0 + M1, N), index0.device)
        built = True
    check(lib().mms_embed_forward_pair_f16(M0, M1, N, K, _ptr(index0, "index0"), _ptr(index1, "index1"),
                                           _ptr(table, "table", dtype=_H), _ptr(bias, "bias", True),
                                           _ptr(top0, "top0", dtype=_H), _ptr(top1, "top1", dtype=_H), wsp, wsb, _stream()),
          "mms_embed_forward_pair_f16")
    return built


def embed_backward_pair_indexed_f16(index0, index1, top_diff0, top_diff1, weight_diff, index, bias_diff=None, shape=None):
    """embed_backward_pair_f16 with the index a pair forward (half or float32) built for (index0, index1)."""
    M0, M1, (K, N) = index0.numel(), index1.numel(), (shape if shape is not None else weight_diff.shape)
    if index.buf is None:
        raise MMSError("embed_backward_pair_indexed_f16: no index was built (the pair forward returned False); use "
                       "embed_backward_pair_f16")
    check(lib().mms_embed_backward_pair_indexed_f16(M0, M1, N, K, _ptr(index0, "index0"),
                                                    _ptr(top_diff0, "top_diff0", dtype=_H), _ptr(index1, "index1"),
                                                    _ptr(top_diff1, "top_diff1", dtype=_H),
                                                    _ptr(weight_diff, "weight_diff", True), _ptr(bias_diff, "bias_diff", True),
                                                    index.buf.data_ptr(), index.buf.numel(), _stream()),
          "mms_embed_backward_pair_indexed_f16")


def feed_gather_rows(src, first, rows, dst, perm=None):
    """dst[i] = src[perm[first+i]] (perm int32 on the device, or None = identity)."""
    src_rows = src.shape[0]
    row_elems = src.numel() // max(src_rows, 1)
    check(lib().mms_feed_gather_rows_f32(rows, row_elems, src_rows, _ptr(src, "src"),
                                         _ptr(perm, "perm", True, dtype=torch.int32), first,
                                         _ptr(dst, "dst"), _stream()),
          "mms_feed_gather_rows_f32")


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
    check(lib().mms_null_launch(int(workgroups), _stream()), "mms_null_launch")


EUCLID_BWD_FP32, EUCLID_BWD_REFERENCE = 0, 1


def set_euclid_backward_mode(mode):
    """'fp32' (default: <= 2 ulp from the reference) or 'reference' (the reference's bits)."""
    m = {"fp32": 0, "reference": 1}.get(mode, mode)
    check(lib().mms_set_euclid_backward_mode(int(m)), "mms_set_euclid_backward_mode")


def set_pairrank_hinge_mode(mode):
    """'cpu' (default): `ordered > 0` as PairRankLossLayer::Backward_cpu; 'gpu': `ordered >= 0` as the
    reference's .cu kernel.  Per calling thread."""
    m = {"cpu": 0, "gpu": 1}[mode] if isinstance(mode, str) else int(mode)
    check(lib().mms_set_pairrank_hinge_mode(m), "mms_set_pairrank_hinge_mode")


def set_f16_distance_mode(mode):
    """'ordered' (default): the reference's d-ascending fp32 sum, bit-identical scores; 'tree': fixed tree sum,
    ~1e-6 relative, no ordered chain.  Per calling thread; fp16-storage entry points only."""
    m = {"ordered": 0, "tree": 1}[mode] if isinstance(mode, str) else int(mode)
    check(lib().mms_set_f16_distance_mode(m), "mms_set_f16_distance_mode")


def set_rank_tie_mode(mode):
    """'input' (default): equal scores keep the input order; 'libstdcxx': the order libstdc++'s std::sort leaves them in
    (include/mms.h: MMS_RANK_TIES_*)."""
    m = {"input": 0, "libstdcxx": 1}[mode] if isinstance(mode, str) else int(mode)
    check(lib().mms_set_rank_tie_mode(m), "mms_set_rank_tie_mode")


def set_loss_sum_mode(mode):
    """'fast' (default): order-free sum of the loss terms; 'reference': Forward_cpu's running fp32 sum, bit for bit
    (include/mms.h: MMS_LOSS_SUM_*)."""
    m = {"fast": 0, "reference": 1}[mode] if isinstance(mode, str) else int(mode)
    check(lib().mms_set_loss_sum_mode(m), "mms_set_loss_sum_mode")


def set_triplet_finish_mode(mode):
    """'inlaunch' (default): the loss is summed inside the step's one launch; 'launch': a second launch sums the terms
    (include/mms.h: MMS_TRIPLET_FINISH_*)."""
    m = {"launch": 0, "inlaunch": 1}[mode] if isinstance(mode, str) else int(mode)
    check(lib().mms_set_triplet_finish_mode(m), "mms_set_triplet_finish_mode")


def get_pairrank_hinge_mode():
    return "gpu" if lib().mms_get_pairrank_hinge_mode() == 1 else "cpu"


def get_euclid_backward_mode():
    return "reference" if lib().mms_get_euclid_backward_mode() == 1 else "fp32"


# ---- double instantiation (functional kernels; tests/test_gpu_f64.py) -------------------------
_D = torch.float64


def simcross_forward_f64(mode, q, a, top, W=None, bias=None, norm0=None, norm1=None, ws=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    M = W.shape[0] if mode == 2 else 1
    wsp, wsb = (ws or _default_ws).get(lib().mms_simcross_workspace_bytes_f64(mode, N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_forward_f64(
        mode, N, W1, W2, D, M, _ptr(q, "q", dtype=_D), _ptr(a, "a", dtype=_D), _ptr(W, "W", True, _D),
        _ptr(bias, "bias", True, _D), _ptr(top, "top", dtype=_D), _ptr(norm0, "norm0", True, _D),
        _ptr(norm1, "norm1", True, _D), wsp, wsb, _stream()), "mms_simcross_forward_f64")


def simcross_backward_f64(mode, q, a, top, top_diff, dq, da, W=None, bias_term=False, norm0=None,
                          norm1=None, dW=None, dbias=None, propagate_down=(True, True), ws=None):
    N, W1, D = q.shape
    W2 = a.shape[1]
    M = W.shape[0] if mode == 2 else 1
    wsp, wsb = (ws or _default_ws).get(lib().mms_simcross_workspace_bytes_f64(mode, N, W1, W2, D, M), q.device)
    check(lib().mms_simcross_backward_f64(
        mode, N, W1, W2, D, M, _ptr(q, "q", dtype=_D), _ptr(a, "a", dtype=_D), _ptr(W, "W", True, _D),
        int(bool(bias_term)), _ptr(top, "top", dtype=_D), _ptr(top_diff, "top_diff", dtype=_D),
        _ptr(norm0, "norm0", True, _D), _ptr(norm1, "norm1", True, _D), int(bool(propagate_down[0])),
        int(bool(propagate_down[1])), _ptr(dq, "dq", dtype=_D), _ptr(da, "da", dtype=_D),
        _ptr(dW, "dW", True, _D), _ptr(dbias, "dbias", True, _D), wsp, wsb, _stream()),
        "mms_simcross_backward_f64")


def simmatrix_forward_f64(q, a, W, top, qw_scratch):
    N = q.shape[0]
    K1, K2 = W.shape
    check(lib().mms_simmatrix_forward_f64(
        N, K1, K2, _ptr(q, "q", dtype=_D), _ptr(a, "a", dtype=_D), _ptr(W, "W", dtype=_D),
        _ptr(top, "top", dtype=_D), _ptr(qw_scratch, "qw_scratch", dtype=_D), _stream()),
        "mms_simmatrix_forward_f64")


def simmatrix_backward_f64(q, a, W, top_diff, dq, da, dW, param_propagate_down=True,
                           propagate_down=(True, True)):
    N = q.shape[0]
    K1, K2 = W.shape
    check(lib().mms_simmatrix_backward_f64(
        N, K1, K2, _ptr(q, "q", dtype=_D), _ptr(a, "a", dtype=_D), _ptr(W, "W", dtype=_D),
        _ptr(top_diff, "top_diff", dtype=_D), int(bool(param_propagate_down)),
        int(bool(propagate_down[0])), int(bool(propagate_down[1])), _ptr(dq, "dq", True, _D),
        _ptr(da, "da", True, _D), _ptr(dW, "dW", True, _D), _stream()), "mms_simmatrix_backward_f64")


def pairrank_forward_f64(a, b, y, ordered, similar, loss, margin=1.0):
    check(lib().mms_pairrank_forward_f64(
        a.numel(), float(margin), _ptr(a, "a", dtype=_D), _ptr(b, "b", dtype=_D), _ptr(y, "y", dtype=_D),
        _ptr(ordered, "ordered", dtype=_D), _ptr(similar, "similar", dtype=_D),
        _ptr(loss, "loss", dtype=_D), _stream()), "mms_pairrank_forward_f64")


def pairrank_backward_f64(y, ordered, similar, da, db, top_diff=1.0, propagate_down=(True, True)):
    check(lib().mms_pairrank_backward_f64(
        y.numel(), float(top_diff), _ptr(y, "y", dtype=_D), _ptr(ordered, "ordered", dtype=_D),
        _ptr(similar, "similar", dtype=_D), int(bool(propagate_down[0])), int(bool(propagate_down[1])),
        _ptr(da, "da", True, _D), _ptr(db, "db", True, _D), _stream()), "mms_pairrank_backward_f64")


def fm_forward_f64(x, top, bias=None):
    N, C, dim = x.shape
    check(lib().mms_fm_forward_f64(N, C, dim, _ptr(x, "x", dtype=_D), _ptr(bias, "bias", True, _D),
                                   _ptr(top, "top", dtype=_D), _stream()), "mms_fm_forward_f64")


def fm_backward_f64(x, top_diff, bottom_diff=None, bias_diff=None):
    N, C, dim = x.shape
    check(lib().mms_fm_backward_f64(
        N, C, dim, _ptr(x, "x", dtype=_D), _ptr(top_diff, "top_diff", dtype=_D),
        _ptr(bottom_diff, "bottom_diff", True, _D), _ptr(bias_diff, "bias_diff", True, _D), _stream()),
        "mms_fm_backward_f64")


def bn_forward_f64(x, scale, shift, running_mean, running_var, top, save_mean, save_std, phase=0, bn_memory=0.9,
                   ws=None):
    _bn_forward("f64", _D, bn_workspace_bytes_f64, x, scale, shift, running_mean, running_var, top, save_mean,
                save_std, phase, bn_memory, ws)


def bn_backward_f64(x, top_diff, scale, save_mean, save_std, bottom_diff=None, scale_diff=None, shift_diff=None,
                    ws=None):
    _bn_backward("f64", _D, bn_workspace_bytes_f64, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff,
                 shift_diff, ws)


def bn_pool_tanh_forward_f64(x, kernel, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                             phase=0, bn_memory=0.9, ws=None):
    _bn_pool_tanh_forward("f64", _D, bn_pool_tanh_workspace_bytes_f64, x, kernel, scale, shift, running_mean,
                          running_var, top, save_pool, save_mean, save_std, phase, bn_memory, ws)


def bn_pool_tanh_backward_f64(x, kernel, top, top_diff, save_pool, scale, save_mean, save_std, bottom_diff=None,
                              scale_diff=None, shift_diff=None, ws=None):
    _bn_pool_tanh_backward("f64", _D, bn_pool_tanh_workspace_bytes_f64, x, kernel, top, top_diff, save_pool, scale,
                           save_mean, save_std, bottom_diff, scale_diff, shift_diff, ws)


def embed_forward_f64(index, weight, top, bias=None):
    M, (K, N) = index.numel(), weight.shape
    check(lib().mms_embed_forward_f64(M, N, K, _ptr(index, "index", dtype=_D), _ptr(weight, "weight", dtype=_D),
                                      _ptr(bias, "bias", True, _D), _ptr(top, "top", dtype=_D), _stream()),
          "mms_embed_forward_f64")


def embed_backward_f64(index, top_diff, weight_diff, bias_diff=None, ws=None, shape=None):
    """weight_diff or bias_diff may be None; `shape` = (K, N) is then needed when weight_diff is None."""
    K, N = shape if shape is not None else weight_diff.shape
    M = index.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_embed_workspace_bytes_f64(M, N), index.device)
    check(lib().mms_embed_backward_f64(M, N, K, _ptr(index, "index", dtype=_D), _ptr(top_diff, "top_diff", dtype=_D),
                                       _ptr(weight_diff, "weight_diff", True, _D),
                                       _ptr(bias_diff, "bias_diff", True, _D), wsp, wsb, _stream()),
          "mms_embed_backward_f64")


def rank_map_mrr_f64(prob, label, group, fixed_axis=1, ws=None):
    """-> (MAP, MRR, effective groups): two numpy float64 scalars and an int."""
    n = label.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes_f64(n), prob.device)
    out = torch.empty(2, dtype=_D, device=prob.device)
    eff = torch.empty(1, dtype=torch.int32, device=prob.device)
    check(lib().mms_rank_map_mrr_f64(
        n, int(fixed_axis), _ptr(prob, "prob", dtype=_D), _ptr(label, "label", dtype=_D), _ptr(group, "group", dtype=_D),
        out.data_ptr(), out.data_ptr() + 8, eff.data_ptr(), wsp, wsb, _stream()), "mms_rank_map_mrr_f64")
    o = out.cpu().numpy()
    return o[0], o[1], int(eff.item())


def rank_auc_f64(prob, label, fixed_axis=1, ignore_label=None, ws=None):
    n = label.numel()
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes_f64(n), prob.device)
    out = torch.empty(1, dtype=_D, device=prob.device)
    check(lib().mms_rank_auc_f64(
        n, int(prob.shape[1]), int(fixed_axis), _ptr(prob, "prob", dtype=_D), _ptr(label, "label", dtype=_D),
        int(ignore_label is not None), int(ignore_label or 0), out.data_ptr(), wsp, wsb, _stream()),
        "mms_rank_auc_f64")
    return out.cpu().numpy()[0]


def rank_auc_nd_f64(prob, label, axis=1, fixed_axis=1, ignore_label=None, ws=None):
    shape = tuple(prob.shape)
    axis = axis % len(shape)
    outer = int(np.prod(shape[:axis])) if axis else 1
    inner = int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
    wsp, wsb = (ws or _default_ws).get(lib().mms_rank_workspace_bytes_f64(outer * inner), prob.device)
    out = torch.empty(1, dtype=_D, device=prob.device)
    check(lib().mms_rank_auc_nd_f64(
        outer, int(shape[axis]), inner, int(fixed_axis), _ptr(prob, "prob", dtype=_D), _ptr(label, "label", dtype=_D),
        int(ignore_label is not None), int(ignore_label or 0), out.data_ptr(), wsp, wsb, _stream()),
        "mms_rank_auc_nd_f64")
    return out.cpu().numpy()[0]


def rank_accuracy_f64(a, b, label, ws=None):
    wsp, wsb = (ws or _default_ws).get(max(4096, lib().mms_rank_workspace_bytes_f64(1)), a.device)
    out = torch.empty(1, dtype=_D, device=a.device)
    check(lib().mms_rank_accuracy_f64(a.numel(), _ptr(a, "a", dtype=_D), _ptr(b, "b", dtype=_D),
                                      _ptr(label, "label", dtype=_D), out.data_ptr(), wsp, wsb, _stream()),
          "mms_rank_accuracy_f64")
    return out.cpu().numpy()[0]
