"""What the Python binding (mms_answer_selection_amd/capi.py) hands to the C ABI, pinned without a GPU.

The library is replaced by a recorder and the wrappers are fed stand-in tensors, so every wrapper's C symbol, argument
order, scalar conversions, workspace handling, return value and every refusal (exception class and message) is
recorded and compared, entry for entry, with tests/golden/capi_calls.json.  The golden was written by this module
(`python tests/test_capi_calls.py`) from the binding as it stood before its wrappers were folded into one
implementation per family; a change of the binding's internals must leave it as it is.
"""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_calls.json")

from mms_answer_selection_amd import capi  # noqa: E402

F32, F64, F16, I32 = torch.float32, torch.float64, torch.float16, torch.int32
WS_BYTES = 4096                      # what every *workspace_bytes* query of the recorder answers
FAIL_CODE = 3
STANDIN_BASE, STANDIN_STEP = 0x7E5700000000, 0x10000

# public functions with tests of their own below instead of a recording
EXCLUDED = {
    "lib",       # loads the real library: test_lib_*
    "check",     # test_check_*
}


class StandIn:
    """As much of a device tensor as the wrappers look at; `device` is the CPU so that what they allocate next to it
    (torch.empty(..., device=prob.device)) is real memory."""
    count = 0

    def __init__(self, shape, dtype=F32):
        self.shape, self.dtype = torch.Size(shape), dtype
        self.is_cuda, self.contiguous, self.name = True, True, None
        self.device = torch.device("cpu")
        StandIn.count += 1
        self.ptr = STANDIN_BASE + StandIn.count * STANDIN_STEP

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape)) if len(self.shape) else 1

    def is_contiguous(self):
        return self.contiguous

    def data_ptr(self):
        return self.ptr


def t(*shape, dtype=F32):
    return StandIn(shape, dtype)


class Recorder:
    """Stands in for the loaded library: every attribute is a C function that notes its call."""

    def __init__(self, returns=None, fail=False):
        self.calls, self.returns, self.fail = [], dict(returns or {}), fail

    def __getattr__(self, symbol):
        if symbol.startswith("__"):
            raise AttributeError(symbol)

        def call(*args):
            self.calls.append((symbol, args))
            if symbol == "mms_error_string":
                return b"recorded failure"
            if symbol in self.returns:
                return self.returns[symbol]
            if "workspace_bytes" in symbol:
                return WS_BYTES
            if "_get_" in symbol or symbol == "mms_embed_pair_index_supported":
                return 0
            return FAIL_CODE if self.fail else 0
        return call


class Session:
    """One recorded case: the recorder in place of lib(), stream 0, fresh default workspaces, and a note of every
    buffer the binding allocates so that pointers into them can be told from other integers."""

    def __init__(self, returns=None, fail=False):
        self.rec = Recorder(returns, fail)
        self.standins, self.allocs = [], []

    def __enter__(self):
        self.mp = pytest.MonkeyPatch()
        real_empty = torch.empty

        def empty(*args, **kwargs):
            buf = real_empty(*args, **kwargs).zero_()
            self.allocs.append(buf)
            return buf
        self.mp.setattr(torch, "empty", empty)
        self.mp.setattr(capi, "lib", lambda: self.rec)
        self.mp.setattr(capi, "_stream", lambda: 0)
        self.mp.setattr(capi, "_default_ws", capi.Workspace())
        self.mp.setattr(capi, "_default_triplet_ws", {})
        return self

    def __exit__(self, *exc):
        self.mp.undo()

    def name(self, kwargs):
        for key, value in kwargs.items():
            members = value if isinstance(value, tuple) else (value,)
            for i, m in enumerate(members):
                if isinstance(m, StandIn):
                    m.name = key if m is value else "%s[%d]" % (key, i)
                    self.standins.append(m)

    def _arg(self, v, bufs):
        if v is None or isinstance(v, (float, str)):
            return v
        if isinstance(v, bytes):
            return v.decode()
        v = int(v)
        for s in self.standins:
            if s.ptr <= v < s.ptr + STANDIN_STEP:
                return s.name if v == s.ptr else "%s+%d" % (s.name, v - s.ptr)
        for b in self.allocs:
            base, size = b.data_ptr(), max(b.numel() * b.element_size(), 1)
            if base <= v < base + size:
                if id(b) not in bufs:
                    bufs[id(b)] = len(bufs)
                return "buf%d+%d" % (bufs[id(b)], v - base)
        return v

    def calls(self):
        bufs = {}
        return [[sym, [self._arg(a, bufs) for a in args]] for sym, args in self.rec.calls]


def _returned(v):
    if isinstance(v, tuple):
        return [_returned(x) for x in v]
    if isinstance(v, np.generic):
        return [type(v).__name__, v.item()]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def _raised(e):
    """[class, message].  Where a required tensor is None and the wrapper reads its shape before any check of its own,
    Python raises the AttributeError; which attribute it names is only the one the wrapper happened to touch first
    (`a.numel()` in rank_accuracy, `a.device` in its _f64 twin), so that name is not recorded."""
    msg = str(e)
    if isinstance(e, AttributeError):
        msg = re.sub(r"^('NoneType' object has no attribute) '\w+'$", r"\1 <the first one touched>", msg)
    return [type(e).__name__, msg]


def record(fn, kwargs_builder, returns=None, fail=False):
    """fn: a public function's name, or a callable taking the capi module and the keyword arguments."""
    with Session(returns, fail) as s:
        kwargs = kwargs_builder()
        s.name(kwargs)
        entry = {"raises": None, "returns": None}
        try:
            out = getattr(capi, fn)(**kwargs) if isinstance(fn, str) else fn(**kwargs)
            entry["returns"] = _returned(out)
        except Exception as e:                                   # noqa: BLE001 -- the class is what is recorded
            entry["raises"] = _raised(e)
        entry["calls"] = s.calls()
        return entry


# ---------------------------------------------------------------------------------------------------------------
# The cases.  FULL[f] gives every parameter of f; DEFAULTS[f] leaves every optional at its default (and every
# pointer that may be NULL at None); EXTRA holds the branches a wrapper takes on its own.
N, W1, W2, D, M, K, K1, K2 = 3, 2, 4, 5, 2, 7, 5, 6
FULL, DEFAULTS, EXTRA = {}, {}, {}


def ws():
    return capi.Workspace()


def both(name, full, defaults=None):
    FULL[name] = full
    if defaults is not None:
        DEFAULTS[name] = defaults


both("simcross_workspace_bytes", lambda: dict(mode=2, N=N, W1=W1, W2=W2, D=D, M=M))
both("simcross_bilinear_workspace_bytes_f16", lambda: dict(N=N, W1=W1, W2=W2, D=D, M=M))
for sfx in ("", "_f64"):
    both("bn_workspace_bytes" + sfx, lambda: dict(N=N, C=4, S=10))
    both("bn_pool_tanh_workspace_bytes" + sfx, lambda: dict(N=N, C=4, H=4, W=6, kh=2, kw=3))


def simcross(dt, which, full):
    def build():
        mode = 2 if full else 1
        m = M if full else 1
        kw = dict(mode=mode, q=t(N, W1, D, dtype=dt), a=t(N, W2, D, dtype=dt), top=t(N, m, W1, W2, dtype=dt))
        if which != "forward":
            kw.update(top_diff=t(N, m, W1, W2, dtype=dt), dq=t(N, W1, D, dtype=dt), da=t(N, W2, D, dtype=dt))
        if full:
            kw.update(W=t(M, D, D, dtype=dt), norm0=t(N, W1, dtype=dt), norm1=t(N, W2, dtype=dt), ws=ws())
            if which != "forward":
                kw.update(dW=t(M, D, D, dtype=dt), dbias=t(M, W1, W2, dtype=dt))
            if which == "backward":
                kw.update(bias_term=True, propagate_down=(True, False))
            else:
                kw.update(bias=t(M, W1, W2, dtype=dt))
        return kw
    return build


for sfx, dt in (("", F32), ("_f64", F64)):
    both("simcross_forward" + sfx, simcross(dt, "forward", True), simcross(dt, "forward", False))
    both("simcross_backward" + sfx, simcross(dt, "backward", True), simcross(dt, "backward", False))

    def flags_off(dt=dt):
        kw = simcross(dt, "backward", True)()
        kw.update(bias_term=False, propagate_down=(False, True))
        return kw
    EXTRA["simcross_backward%s/flags_off" % sfx] = ("simcross_backward" + sfx, flags_off)
both("simcross_forward_backward", simcross(F32, "forward_backward", True), simcross(F32, "forward_backward", False))


def embed_simcross(f16, full):
    def build():
        kw = dict(mode=0 if full else 1, index_q=t(N, W1), index_a=t(N, W2), top=t(N, 1, W1, W2))
        kw["table" if f16 else "weight"] = t(K, D, dtype=F16 if f16 else F32)
        if full:
            kw.update(norm0=t(N, W1), norm1=t(N, W2), embed_bias=t(D))
        return kw
    return build


def embed_simcross_bilinear(f16, full):
    def build():
        kw = dict(index_q=t(N, W1), index_a=t(N, W2), W=t(M, D, D), bias=t(M, W1, W2) if full else None,
                  top=t(N, M, W1, W2))
        kw["table" if f16 else "weight"] = t(K, D, dtype=F16 if f16 else F32)
        if full:
            kw.update(embed_bias=t(D))
        return kw
    return build


for sfx, f16 in (("", False), ("_f16", True)):
    both("embed_simcross_forward" + sfx, embed_simcross(f16, True), embed_simcross(f16, False))
    both("embed_simcross_bilinear_forward" + sfx, embed_simcross_bilinear(f16, True), embed_simcross_bilinear(f16, False))


def simmatrix_forward(dt, full):
    def build():
        kw = dict(q=t(N, K1, dtype=dt), a=t(N, K2, dtype=dt), W=t(K1, K2, dtype=dt), top=t(N, dtype=dt),
                  qw_scratch=t(N, K2, dtype=dt))
        if full and dt is F32:
            kw.update(ws=ws(), use_workspace=True)
        return kw
    return build


def simmatrix_backward(dt, full):
    def build():
        kw = dict(q=t(N, K1, dtype=dt), a=t(N, K2, dtype=dt), W=t(K1, K2, dtype=dt), top_diff=t(N, dtype=dt),
                  dq=None, da=None, dW=None)
        if full:
            kw.update(dq=t(N, K1, dtype=dt), da=t(N, K2, dtype=dt), dW=t(K1, K2, dtype=dt),
                      param_propagate_down=True, propagate_down=(False, True))
            if dt is F32:
                kw.update(ws=ws(), qw=t(N, K2))
        return kw
    return build


both("simmatrix_forward", simmatrix_forward(F32, True), simmatrix_forward(F32, False))
both("simmatrix_forward_f64", simmatrix_forward(F64, True))
both("simmatrix_backward", simmatrix_backward(F32, True), simmatrix_backward(F32, False))
both("simmatrix_backward_f64", simmatrix_backward(F64, True), simmatrix_backward(F64, False))


def _no_workspace():
    kw = simmatrix_forward(F32, False)()
    kw.update(use_workspace=False, ws=ws())
    return kw


def _uncached_flags_off():
    kw = simmatrix_backward(F32, True)()
    kw.update(qw=None, param_propagate_down=False, propagate_down=(True, False))
    return kw


EXTRA["simmatrix_forward/use_workspace=False"] = ("simmatrix_forward", _no_workspace)
EXTRA["simmatrix_backward/uncached_flags_off"] = ("simmatrix_backward", _uncached_flags_off)


def simmatrix_f16(which, full):
    def build():
        kw = dict(q=t(N, K1, dtype=F16), a=t(N, K2, dtype=F16), W=t(K1, K2))
        if which == "backward":
            kw.update(qw=None, top_diff=t(N), dq=None, da=None, dW=None)
            if full:
                kw.update(qw=t(N, K2), dq=t(N, K1, dtype=F16), da=t(N, K2, dtype=F16), dW=t(K1, K2))
        else:
            kw.update(top=t(N))
            if which == "train":
                kw.update(qw_scratch=t(N, K2))
        if full:
            kw.update(ws=ws())
        return kw
    return build


both("simmatrix_forward_f16", simmatrix_f16("forward", True), simmatrix_f16("forward", False))
both("simmatrix_forward_train_f16", simmatrix_f16("train", True), simmatrix_f16("train", False))
both("simmatrix_backward_f16", simmatrix_f16("backward", True), simmatrix_f16("backward", False))


def pairrank_forward(dt, full):
    def build():
        kw = {k: t(N, dtype=dt) for k in ("a", "b", "y", "ordered", "similar")}
        kw["loss"] = t(1, dtype=dt)
        if full:
            kw.update(margin=0.25)
            if dt is F32:
                kw.update(ws=ws())
        return kw
    return build


def pairrank_backward(dt, full):
    def build():
        kw = {k: t(N, dtype=dt) for k in ("y", "ordered", "similar")}
        kw.update(da=None, db=None)
        if full:
            kw.update(da=t(N, dtype=dt), db=t(N, dtype=dt), top_diff=0.5, propagate_down=(False, True))
        return kw
    return build


def fm(dt, which, full):
    def build():
        kw = dict(x=t(N, 4, D, dtype=dt))
        if which != "forward":
            kw.update(top_diff=t(N, dtype=dt))
        if which != "backward":
            kw.update(top=t(N, dtype=dt))
        if which == "forward_backward":
            kw.update(bottom_diff=t(N, 4, D, dtype=dt))
        if full:
            if which != "backward":
                kw.update(bias=t(1, dtype=dt))
            if which != "forward":
                kw.update(bias_diff=t(1, dtype=dt))
            if which == "backward":
                kw.update(bottom_diff=t(N, 4, D, dtype=dt))
        return kw
    return build


def bn(dt, which, full, shape=(N, 4, 2, 5)):
    def build():
        C = shape[1] if len(shape) > 1 else 4
        kw = dict(x=t(*shape, dtype=dt), scale=t(C, dtype=dt), save_mean=t(C, dtype=dt), save_std=t(C, dtype=dt))
        if which == "forward":
            kw.update(shift=t(C, dtype=dt), running_mean=t(C, dtype=dt), running_var=t(C, dtype=dt),
                      top=t(*shape, dtype=dt))
            if full:
                kw.update(phase=1, bn_memory=0.5, ws=ws())
        else:
            kw.update(top_diff=t(*shape, dtype=dt))
            if full:
                kw.update(bottom_diff=t(*shape, dtype=dt), scale_diff=t(C, dtype=dt), shift_diff=t(C, dtype=dt), ws=ws())
        return kw
    return build


def bn_pool(dt, which, full):
    def build():
        kw = bn(dt, which, full, (N, 4, 4, 6))()
        pooled = (N, 4, 2, 2) if full else (N, 4, 2, 3)
        kw.update(kernel=(2, 3) if full else 2, top=t(*pooled, dtype=dt), save_pool=t(*pooled, dtype=dt))
        if which == "backward":
            kw.update(top_diff=t(*pooled, dtype=dt))
        return kw
    return build


for sfx, dt in (("", F32), ("_f64", F64)):
    both("pairrank_forward" + sfx, pairrank_forward(dt, True), pairrank_forward(dt, False))
    both("pairrank_backward" + sfx, pairrank_backward(dt, True), pairrank_backward(dt, False))
    both("fm_forward" + sfx, fm(dt, "forward", True), fm(dt, "forward", False))
    both("fm_backward" + sfx, fm(dt, "backward", True), fm(dt, "backward", False))
    for which in ("forward", "backward"):
        both("bn_%s%s" % (which, sfx), bn(dt, which, True), bn(dt, which, False))
        EXTRA["bn_%s%s/3-D" % (which, sfx)] = ("bn_%s%s" % (which, sfx), bn(dt, which, True, (N, 4, 10)))
        EXTRA["bn_%s%s/1-D" % (which, sfx)] = ("bn_%s%s" % (which, sfx), bn(dt, which, True, (N,)))
        EXTRA["bn_%s%s/2-D" % (which, sfx)] = ("bn_%s%s" % (which, sfx), bn(dt, which, True, (N, 4)))
        both("bn_pool_tanh_%s%s" % (which, sfx), bn_pool(dt, which, True), bn_pool(dt, which, False))

        def three_d(dt=dt, which=which):
            kw = bn_pool(dt, which, True)()
            kw["x"] = t(N, 4, 24, dtype=dt)
            return kw
        EXTRA["bn_pool_tanh_%s%s/3-D" % (which, sfx)] = ("bn_pool_tanh_%s%s" % (which, sfx), three_d)
both("fm_forward_backward", fm(F32, "forward_backward", True), fm(F32, "forward_backward", False))


def triplet(which, full, workspace=None):
    def build():
        kw = dict(q=t(N, D), a_pos=t(N, D), a_neg=t(N, D), y=t(N), s_pos=t(N), s_neg=t(N), loss=None,
                  dq=t(N, D), da_pos=t(N, D), da_neg=t(N, D))
        if which == "simmatrix":
            kw.update(q=t(N, K1), a_pos=t(N, K2), a_neg=t(N, K2), W=t(K1, K2), dq=t(N, K1), da_pos=t(N, K2),
                      da_neg=t(N, K2), dW=t(K1, K2))
        if full:
            kw.update(loss=t(1), margin=0.25, loss_weight=2.0,
                      ws=ws() if which == "simmatrix" else capi.TripletWorkspace())
            if which == "cosine":
                kw.update(norms=(t(N), t(N), t(N)))
        if workspace is not None:
            kw.update(ws=workspace())
        return kw
    return build


for which in ("euclid", "cosine", "simmatrix"):
    both("triplet_%s_step" % which, triplet(which, True), triplet(which, False))
for which in ("euclid", "cosine"):
    EXTRA["triplet_%s_step/plain_Workspace" % which] = ("triplet_%s_step" % which, triplet(which, False, ws))


def _some_norms():
    kw = triplet("cosine", False)()
    kw.update(norms=(None, t(N), None))
    return kw


def _twice(**kw):
    capi.triplet_euclid_step(**kw)
    return capi.triplet_euclid_step(**kw)


EXTRA["triplet_cosine_step/some_norms"] = ("triplet_cosine_step", _some_norms)
EXTRA["triplet_euclid_step/default_workspace_twice"] = (_twice, triplet("euclid", False))


def rank(dt, which, full, **more):
    def build():
        if which == "accuracy":
            kw = dict(a=t(N, dtype=dt), b=t(N, dtype=dt), label=t(N, dtype=dt))
        elif which == "auc_nd":
            kw = dict(prob=t(2, 3, 4, dtype=dt), label=t(2, 4, dtype=dt))
        else:
            kw = dict(prob=t(6, 2, dtype=dt), label=t(6, dtype=dt))
        if which.startswith("map_mrr"):
            kw.update(group=t(6, dtype=dt))
        if which == "map_mrr_device":
            kw.update(out=t(2, dtype=dt), eff=t(1, dtype=I32))
        if full:
            kw.update(ws=ws())
            if which != "accuracy":
                kw.update(fixed_axis=0)
            if which.startswith("auc"):
                kw.update(ignore_label=3)
            if which == "auc_nd":
                kw.update(axis=-1)
        kw.update(more)
        return kw
    return build


for sfx, dt in (("", F32), ("_f64", F64)):
    for which in ("map_mrr", "auc", "auc_nd", "accuracy"):
        both("rank_%s%s" % (which, sfx), rank(dt, which, True), rank(dt, which, False))
    for label in (None, 0, 3):
        EXTRA["rank_auc%s/ignore_label=%s" % (sfx, label)] = ("rank_auc" + sfx, rank(dt, "auc", False, ignore_label=label))
        EXTRA["rank_auc_nd%s/ignore_label=%s" % (sfx, label)] = ("rank_auc_nd" + sfx,
                                                                 rank(dt, "auc_nd", False, ignore_label=label))
    for axis in (0, 1, -1):
        EXTRA["rank_auc_nd%s/axis=%d" % (sfx, axis)] = ("rank_auc_nd" + sfx, rank(dt, "auc_nd", False, axis=axis))
both("rank_map_mrr_device", rank(F32, "map_mrr_device", True), rank(F32, "map_mrr_device", False))


def rows_f16(cosine, backward, full):
    def build():
        kw = dict(q=t(N, 1, D, dtype=F16), a=t(N, 1, D, dtype=F16), top=t(N))
        if backward:
            kw.update(top_diff=t(N), dq=t(N, 1, D, dtype=F16), da=t(N, 1, D, dtype=F16))
        if cosine and full:
            kw.update(norm0=t(N), norm1=t(N))
        return kw
    return build


both("simcross_euclid_forward_f16", rows_f16(False, False, True))
both("simcross_euclid_forward_backward_f16", rows_f16(False, True, True))
both("simcross_cosine_forward_f16", rows_f16(True, False, True), rows_f16(True, False, False))
both("simcross_cosine_forward_backward_f16", rows_f16(True, True, True), rows_f16(True, True, False))


def grid_f16(which, full):
    def build():
        kw = dict(mode=0 if full else 1, q=t(N, W1, D, dtype=F16), a=t(N, W2, D, dtype=F16), top=t(N, 1, W1, W2))
        if which != "forward":
            kw.update(top_diff=t(N, 1, W1, W2), dq=t(N, W1, D, dtype=F16), da=t(N, W2, D, dtype=F16))
        if full:
            kw.update(norm0=t(N, W1), norm1=t(N, W2))
        return kw
    return build


def bilinear_f16(which, full):
    def build():
        kw = dict(q=t(N, W1, D, dtype=F16), a=t(N, W2, D, dtype=F16), W=t(M, D, D))
        if which != "backward":
            kw.update(bias=t(M, W1, W2) if full else None, top=t(N, M, W1, W2))
        if which != "forward":
            kw.update(top_diff=t(N, M, W1, W2), dq=t(N, W1, D, dtype=F16), da=t(N, W2, D, dtype=F16), dW=t(M, D, D))
            if full:
                kw.update(dbias=t(M, W1, W2))
        if full:
            kw.update(ws=ws())
        return kw
    return build


for which in ("forward", "backward", "forward_backward"):
    both("simcross_%s_f16" % which, grid_f16(which, True), grid_f16(which, False))
    both("simcross_bilinear_%s_f16" % which, bilinear_f16(which, True), bilinear_f16(which, False))

    def no_W(which=which):
        kw = bilinear_f16(which, True)()
        kw["W"] = None
        return kw
    EXTRA["simcross_bilinear_%s_f16/W=None" % which] = ("simcross_bilinear_%s_f16" % which, no_W)


def _bilinear_W_2d():
    kw = embed_simcross_bilinear(True, True)()
    kw["W"] = t(D, D)
    return kw


def _bilinear_no_W():
    kw = embed_simcross_bilinear(True, True)()
    kw["W"] = None
    return kw


EXTRA["embed_simcross_bilinear_forward_f16/W_2-D"] = ("embed_simcross_bilinear_forward_f16", _bilinear_W_2d)
EXTRA["embed_simcross_bilinear_forward_f16/W=None"] = ("embed_simcross_bilinear_forward_f16", _bilinear_no_W)


def embed(kind, which, full, **more):
    """kind: "f32", "f64" or "f16" (half table / top / top_diff, everything else float32)."""
    dt = F64 if kind == "f64" else F32
    st = F16 if kind == "f16" else dt
    table = "table" if kind == "f16" else "weight"

    def build():
        if which == "forward":
            kw = {"index": t(N, W1, dtype=dt), table: t(K, D, dtype=st), "top": t(N, W1, D, dtype=st)}
            if full:
                kw.update(bias=t(D, dtype=dt))
        elif which == "backward":
            kw = dict(index=t(N, W1, dtype=dt), top_diff=t(N, W1, D, dtype=st), weight_diff=t(K, D, dtype=dt))
            if full:
                kw.update(bias_diff=t(D, dtype=dt), ws=ws(), shape=(K, D))
        elif which == "forward_pair":
            kw = {"index0": t(N, W1), "index1": t(N, W2), table: t(K, D, dtype=st), "top0": t(N, W1, D, dtype=st),
                  "top1": t(N, W2, D, dtype=st)}
            if full:
                kw.update(bias=t(D), index=capi.EmbedPairIndex())
        else:
            kw = dict(index0=t(N, W1), index1=t(N, W2), top_diff0=t(N, W1, D, dtype=st),
                      top_diff1=t(N, W2, D, dtype=st), weight_diff=t(K, D))
            if which == "backward_pair_indexed":
                kw.update(index=capi.EmbedPairIndex())
                kw["index"].get(96, torch.device("cpu"))
            if full:
                kw.update(bias_diff=t(D), shape=(K, D))
                if which == "backward_pair":
                    kw.update(ws=ws())
        kw.update(more)
        return kw
    return build


SUPPORTED = {"mms_embed_pair_index_supported": 1}
for sfx, kind in (("", "f32"), ("_f64", "f64"), ("_f16", "f16")):
    whiches = ("forward", "backward") if kind == "f64" else (
        "forward", "backward", "forward_pair", "backward_pair", "backward_pair_indexed")
    for which in whiches:
        name = "embed_%s%s" % (which, sfx)
        both(name, embed(kind, which, True), embed(kind, which, False))
        if "backward" in which:
            EXTRA[name + "/shape_only"] = (name, embed(kind, which, False, weight_diff=None, shape=(K, D)))
            EXTRA[name + "/neither"] = (name, embed(kind, which, False, weight_diff=None))
    if kind != "f64":
        EXTRA["embed_forward_pair%s/index_supported" % sfx] = ("embed_forward_pair" + sfx,
                                                               embed(kind, "forward_pair", True), SUPPORTED)
        EXTRA["embed_backward_pair_indexed%s/unbuilt" % sfx] = (
            "embed_backward_pair_indexed" + sfx, embed(kind, "backward_pair_indexed", True, index=capi.EmbedPairIndex()))

both("feed_gather_rows", lambda: dict(src=t(6, D), first=1, rows=N, dst=t(N, D), perm=t(6, dtype=I32)),
     lambda: dict(src=t(6, D), first=0, rows=N, dst=t(N, D)))
EXTRA["feed_gather_rows/no_rows"] = ("feed_gather_rows", lambda: dict(src=t(0, D), first=0, rows=0, dst=t(0, D)))
both("null_launch", lambda: dict(workgroups=7), dict)

# the arithmetic switches: name -> the strings in value order
MODES = {"matrix": ("bf16x3", "fp32"), "euclid_backward": ("fp32", "reference"), "pairrank_hinge": ("cpu", "gpu"),
         "f16_distance": ("ordered", "tree"), "rank_tie": ("input", "libstdcxx"), "loss_sum": ("fast", "reference"),
         "triplet_finish": ("launch", "inlaunch")}
GETTERS = ("matrix", "euclid_backward", "pairrank_hinge")
for stem, names in MODES.items():
    both("set_%s_mode" % stem, lambda names=names: dict(mode=names[1]))
    for value in names + (0, 1, 2, "bogus", None, 1.0, True):
        EXTRA["set_%s_mode/%r" % (stem, value)] = ("set_%s_mode" % stem, lambda value=value: dict(mode=value))
for stem in GETTERS:
    both("get_%s_mode" % stem, dict)
    for value in (0, 1):
        EXTRA["get_%s_mode/%d" % (stem, value)] = ("get_%s_mode" % stem, dict, {"mms_get_%s_mode" % stem: value})


# the three buffer classes
def _workspace_get():
    cpu, w = torch.device("cpu"), capi.Workspace()
    out = [w.get(0, cpu), w.buf is None]
    p1 = w.get(100, cpu)
    first = w.buf
    out += [p1 == (first.data_ptr(), 100), w.get(40, cpu) == p1, w.buf is first, w._retired == []]
    p2 = w.get(200, cpu)
    out += [p2 == (w.buf.data_ptr(), 200), w.buf is not first, len(w._retired) == 1 and w._retired[0] is first,
            w.buf.dtype == torch.uint8, w.get(0, cpu)]
    return tuple(out)


def _triplet_workspace():
    cpu, w = torch.device("cpu"), capi.TripletWorkspace()
    w.reset()                                         # nothing to initialise yet: no call
    p1 = w.get(64, cpu)
    first = w.buf
    same = w.get(16, cpu) == p1                       # no growth: no second init
    p2 = w.get(128, cpu)
    w.reset()
    return (p1 == (first.data_ptr(), 64), same, p2 == (w.buf.data_ptr(), 128), w._retired[0] is first,
            len(w._retired))


def _pair_index():
    cpu, ix = torch.device("cpu"), capi.EmbedPairIndex()
    p1 = ix.get(64, cpu)
    first = ix.buf
    return (p1 == (first.data_ptr(), 64), ix.get(8, cpu) == p1, ix.get(65, cpu) == (ix.buf.data_ptr(), 65),
            ix.buf is not first, hasattr(ix, "_retired"))


CLASS_METHODS = {"Workspace.get": _workspace_get, "TripletWorkspace.get+reset": _triplet_workspace,
                 "EmbedPairIndex.get": _pair_index}
for name, fn in CLASS_METHODS.items():
    EXTRA[name] = (lambda fn=fn, **kw: fn(), dict)


# ---------------------------------------------------------------------------------------------------------------
# Refusals: the full call of every wrapper with one tensor at a time spoilt.
def _spoil_cpu(s):
    s.is_cuda = False


def _spoil_dtype(s):
    s.dtype = torch.int8


def _spoil_strided(s):
    s.contiguous = False


def _spoil_last(s):
    s.shape = torch.Size(tuple(s.shape[:-1]) + (s.shape[-1] + 1,))


def _spoil_rank(s):
    s.shape = torch.Size(tuple(s.shape) + (1,))


SPOIL = {"not_on_gpu": _spoil_cpu, "wrong_dtype": _spoil_dtype, "not_contiguous": _spoil_strided, "missing": None,
         "last_dim+1": _spoil_last, "one_more_dim": _spoil_rank}


def _tensor_slots(kwargs):
    for key, value in kwargs.items():
        if isinstance(value, StandIn):
            yield key, None
        elif isinstance(value, tuple):
            for i, m in enumerate(value):
                if isinstance(m, StandIn):
                    yield key, i


def refusals(fname):
    """{tensor: {kind: [class, message] or "ok"}} plus what a non-zero return code of the C call raises."""
    out = {}
    for key, i in _tensor_slots(FULL[fname]()):
        slot = key if i is None else "%s[%d]" % (key, i)
        out[slot] = {}
        for kind, spoil in SPOIL.items():
            def build():
                kw = FULL[fname]()
                victim = kw[key] if i is None else kw[key][i]
                if spoil is not None:
                    spoil(victim)
                    return kw
                kw[key] = None if i is None else tuple(None if m is victim else m for m in kw[key])
                return kw
            raised = record(fname, build)["raises"]
            out[slot][kind] = raised if raised is not None else "ok"
    out["<non-zero return code>"] = record(fname, FULL[fname], fail=True)["raises"]
    return out


def public_functions():
    return {n: f for n, f in inspect.getmembers(capi, inspect.isfunction)
            if not n.startswith("_") and f.__module__ == capi.__name__}


def public_classes():
    return {n: c for n, c in inspect.getmembers(capi, inspect.isclass)
            if not n.startswith("_") and c.__module__ == capi.__name__}


def signatures():
    out = {n: str(inspect.signature(f)) for n, f in public_functions().items()}
    for cname, cls in public_classes().items():
        for n, f in inspect.getmembers(cls, inspect.isfunction):
            if n in cls.__dict__:
                out["%s.%s" % (cname, n)] = str(inspect.signature(f))
        out[cname + " bases"] = [b.__name__ for b in cls.__mro__[1:]]
    return out


def case_ids():
    ids = [f + "/full" for f in FULL] + [f + "/defaults" for f in DEFAULTS] + list(EXTRA)
    ids += [f + "/refusals" for f in FULL] + ["<signatures>", "<constants>"]
    return sorted(ids)


def constants():
    return {"MMS_VERSION": capi.MMS_VERSION, "MMS_OK": capi.MMS_OK, "EXPORTED_SYMBOLS": list(capi.EXPORTED_SYMBOLS),
            "EXPORTED_SYMBOLS are _SIGNATURES": list(capi._SIGNATURES) == list(capi.EXPORTED_SYMBOLS),
            "LIB_PATH": os.path.relpath(capi.LIB_PATH, ROOT),
            "EUCLID_BWD": [capi.EUCLID_BWD_FP32, capi.EUCLID_BWD_REFERENCE],
            "SimCrossArgs": [[f[0], f[1].__name__] for f in capi.SimCrossArgs._fields_]}


def run_case(case):
    if case == "<signatures>":
        return signatures()
    if case == "<constants>":
        return constants()
    if case in EXTRA:
        return record(*EXTRA[case])
    fname, kind = case.rsplit("/", 1)
    if kind == "refusals":
        return refusals(fname)
    return record(fname, (FULL if kind == "full" else DEFAULTS)[fname])


def _json(entry):
    return json.loads(json.dumps(entry))          # tuples -> lists, as the golden holds them


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", case_ids())
def test_recorded_call_matches_golden(case, golden):
    assert case in golden, "%s is not in the golden" % case
    assert _json(run_case(case)) == golden[case]


def test_golden_holds_nothing_else(golden):
    assert sorted(golden) == case_ids()


def test_every_public_function_is_exercised():
    """Each public function is on the short exclusion list or has a call with every parameter given and, where it
    has optionals, one with them left alone."""
    funcs = public_functions()
    assert len(funcs) >= 87
    assert EXCLUDED <= set(funcs)
    for name, f in funcs.items():
        if name in EXCLUDED:
            continue
        assert name in FULL, "%s is not exercised" % name
        params = inspect.signature(f).parameters
        assert set(FULL[name]()) == set(params), "%s: the full call must give every parameter" % name
        optional = [p for p, v in params.items() if v.default is not inspect.Parameter.empty]
        if optional:
            assert name in DEFAULTS, "%s has optionals and no call that leaves them alone" % name
            assert not set(DEFAULTS[name]()) & set(optional)
    assert set(FULL) | EXCLUDED == set(funcs), "a case names a function that is not public"
    for fn, *_ in EXTRA.values():
        assert not isinstance(fn, str) or fn in funcs
    assert set(public_classes()) >= {"Workspace", "TripletWorkspace", "EmbedPairIndex", "SimCrossArgs", "MMSError",
                                     "MMSArgumentError"}


def test_argument_errors_are_value_errors_and_mms_errors():
    assert issubclass(capi.MMSArgumentError, capi.MMSError) and issubclass(capi.MMSArgumentError, ValueError)
    assert issubclass(capi.MMSError, RuntimeError) and not issubclass(capi.MMSError, ValueError)


def test_check_passes_zero_and_names_the_call_otherwise():
    with Session() as s:
        assert capi.check(0, "mms_fm_forward_f32") is None
        assert s.rec.calls == []
        with pytest.raises(capi.MMSError) as e:
            capi.check(2, "mms_fm_forward_f32")
        assert str(e.value) == "mms_fm_forward_f32 failed: recorded failure (code 2)"
        assert type(e.value) is capi.MMSError
        assert s.rec.calls == [("mms_error_string", (2,))]


def test_lib_refuses_when_the_library_is_not_built(monkeypatch, tmp_path):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(tmp_path / "libmms_hip.so"))
    with pytest.raises(capi.MMSError, match="is not built .*there is no CPU fallback"):
        capi.lib()


def test_lib_binds_every_signature_and_checks_the_version(monkeypatch):
    bound = {}

    class Fn:
        def __init__(self, name):
            self.name = name

        def __call__(self):
            return version[0]

    class Lib:
        def __getattr__(self, name):
            if name not in capi._SIGNATURES:
                raise AttributeError(name)
            return bound.setdefault(name, Fn(name))

    version = [capi.MMS_VERSION]
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi.C, "CDLL", lambda path: Lib())
    monkeypatch.setattr(capi.os.path, "exists", lambda path: True)
    loaded = capi.lib()
    assert capi.lib() is loaded                                  # cached
    assert set(bound) == set(capi._SIGNATURES)
    for name, (res, args) in capi._SIGNATURES.items():
        assert bound[name].restype is res and bound[name].argtypes == args
    monkeypatch.setattr(capi, "_lib", None)
    version[0] = capi.MMS_VERSION + 1
    with pytest.raises(capi.MMSError, match="reports ABI version %d, this binding was written for %d"
                       % (capi.MMS_VERSION + 1, capi.MMS_VERSION)):
        capi.lib()
    assert capi._lib is None


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:                                  # one case per line, keys sorted
        f.write("{\n%s\n}\n" % ",\n".join(
            "%s: %s" % (json.dumps(case), json.dumps(run_case(case), sort_keys=True, separators=(",", ":")))
            for case in case_ids()))
    print("%s: %d entries, %d bytes" % (GOLDEN, len(case_ids()), os.path.getsize(GOLDEN)))
