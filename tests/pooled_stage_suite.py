"""What the GPU and ABI suites of the pooled stages share between the AvePool and the MaxPool form of a stage: the
helpers and the test bodies that differ only in the binding module and the reference module they are bound to.  Not a
test module: tests/test_gpu_{bn_pool,bn_maxpool,conv_stage,conv_maxpool_stage}.py bind a suite to their modules and
keep their own parametrisations, docstrings and method-specific tests."""
import functools
import importlib

import numpy as np
import pytest
import torch

import test_gpu_bn as B
import test_gpu_conv as V
from util import SEED, TOL, assert_close

assert_words_equal = B.assert_words_equal
BAR = {np.float32: TOL, np.float64: 1e-12}
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3       # include/mms.h: MMS_OK, MMS_ERR_*
P = 4096                                  # stands for arrays that are never touched: the ABI suites' calls return first


def shared_model(R, args):
    """-> inputs(key, dtype), model(key, dtype): R's conditioned inputs, and its float64 model on those inputs as the
    device gets them; each computed once and shared (never modified)."""
    @functools.lru_cache(maxsize=None)
    def inputs(key, dtype):
        return R.conditioned_inputs(key, dtype, SEED)

    @functools.lru_cache(maxsize=None)
    def model(key, dtype):
        out = R.model_outputs(*args(key, inputs(key, dtype)), np.float64)
        for v in out.values():
            v.setflags(write=False)
        return out

    return inputs, model


# ---- BN -> pooling -> TanH ---------------------------------------------------------------------------------------
BACKWARD_OUTPUTS = ("bottom_diff", "scale_diff", "shift_diff")


def check_parity(got, want, dtype):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == dtype and not np.isnan(got[k]).any(), k
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        print("%-22s %.3e" % (k, float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) / scale))
    for k in sorted(want):
        assert_close(got[k], want[k], BAR[dtype], k)


def same_words(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert_words_equal(got[k], want[k], "%s, %s" % (k, what))


class BnPool:
    """The calls `stem`_forward / _backward / _workspace_bytes (and their _f64 forms) of mms_answer_selection_amd's
    `module`, against reference module R; shift_in_backward: the backward takes `shift` after `scale`."""

    def __init__(self, module, stem, R, shift_in_backward):
        self.module, self.stem, self.R, self.shift_in_backward = module, stem, R, shift_in_backward
        self.inputs, self.model = shared_model(R, lambda shape, inp: (inp, shape[4:]))

    def api(self, dtype):
        """-> forward, backward, workspace query of `dtype`; the binding is imported here, after the build."""
        m = importlib.import_module("mms_answer_selection_amd." + self.module)
        sfx = "" if dtype == np.float32 else "_f64"
        return tuple(getattr(m, "%s_%s%s" % (self.stem, f, sfx)) for f in ("forward", "backward", "workspace_bytes"))

    def run(self, inp, kernel, dtype, shift=0, ws=None, outputs=(True, True, True), phases=("train", "test")):
        """TRAIN forward, backward, TEST forward (from the same running blobs), backward; every output starts as NaN
        (the two parameter diffs as 123) between guard zones; every operand is `shift` elements off a 16-byte boundary.
        -> {"train_top": ..., "test_shift_diff": ...} on the host, the keys of R.model_outputs; a backward output not
        asked for (outputs = bottom_diff, scale_diff, shift_diff) is absent, and its prefill is checked to be intact."""
        R, Guarded, placed = self.R, B.Guarded, B.placed
        fwd, bwd, _ = self.api(dtype)
        shape, pooled, C = inp["x"].shape, inp["top_diff"].shape, inp["x"].shape[1]
        x, top_diff = placed(inp["x"], dtype, shift), placed(inp["top_diff"], dtype, shift)
        scale, shift_blob = placed(inp["scale"], dtype, shift), placed(inp["shift"], dtype, shift)
        nan = float("nan")
        out = {}
        for name in phases:
            g = dict(top=Guarded(pooled, dtype, nan, shift), save_pool=Guarded(pooled, dtype, nan, shift),
                     save_mean=Guarded((C,), dtype, nan, shift), save_std=Guarded((C,), dtype, nan, shift),
                     running_mean=Guarded((C,), dtype, inp["running_mean"], shift),
                     running_var=Guarded((C,), dtype, inp["running_var"], shift))
            fwd(x, kernel, scale, shift_blob, g["running_mean"].t, g["running_var"].t, g["top"].t, g["save_pool"].t,
                g["save_mean"].t, g["save_std"].t, phase=R.TRAIN if name == "train" else R.TEST, bn_memory=R.BN_MEMORY,
                ws=ws)
            b = dict(bottom_diff=Guarded(shape, dtype, nan, shift), scale_diff=Guarded((C,), dtype, 123.0, shift),
                     shift_diff=Guarded((C,), dtype, 123.0, shift))
            given = {k: b[k].t if want else None for k, want in zip(BACKWARD_OUTPUTS, outputs)}
            extra = (shift_blob,) if self.shift_in_backward else ()
            bwd(x, kernel, g["top"].t, top_diff, g["save_pool"].t, scale, *extra, g["save_mean"].t, g["save_std"].t,
                ws=ws, **given)
            for k, v in g.items():
                out[name + "_" + k] = v.host(name + " " + k)
            for k, v in b.items():
                h = v.host(name + " " + k)
                if given[k] is not None:
                    out[name + "_" + k] = h
                else:
                    assert (h == 123.0).all() if k != "bottom_diff" else np.isnan(h).all(), k + " was not asked for"
        if "test" in phases:
            assert_words_equal(out["test_running_mean"], inp["running_mean"], "TEST phase: running mean")
            assert_words_equal(out["test_running_var"], inp["running_var"], "TEST phase: running variance")
            assert_words_equal(out["test_save_mean"], inp["running_mean"], "TEST phase: saved mean")
        return out

    def check_parity_and_determinism(self, shape, dtype):
        """Every output of TRAIN forward, TEST forward and the backward after each against the float64 model; NaN / 123
        prefills gone, guards intact, TEST leaves the running blobs' words alone (inside run); a second run on fresh
        outputs gives the same words."""
        inp = self.inputs(shape, dtype)
        first = self.run(inp, shape[4:], dtype)
        check_parity(first, self.model(shape, dtype), dtype)
        same_words(self.run(inp, shape[4:], dtype), first, "second run")

    def check_zero_variance_is_exact(self, dtype):
        inp = self.inputs((1, 1, 1, 1, 1, 1), dtype)
        out = self.run(inp, (1, 1), dtype)
        assert (out["train_save_pool"] == 0).all() and (out["train_bottom_diff"] == 0).all()
        assert (out["train_scale_diff"] == 0).all()
        assert_words_equal(out["train_save_std"], np.sqrt(np.array([1e-9], dtype)), "std == sqrt(var_eps)")
        assert_words_equal(out["train_save_mean"], inp["x"].reshape(1), "mean == x")
        t = out["train_top"].reshape(1)
        assert_words_equal(out["train_shift_diff"], inp["top_diff"].reshape(1) * (dtype(1) - t * t), "shift_diff == gp")

    def check_both_sides_of_the_routing_threshold(self, dtype):
        """The largest channel of the one-launch route and the next batch size up, found from the workspace query, both
        against the model."""
        _, _, query = self.api(dtype)
        below, above = self.R.THRESHOLD_SHAPES[dtype]
        assert query(*below) == 0 and query(*above) > 0
        for shape in (below, above):
            check_parity(self.run(self.inputs(shape, dtype), shape[4:], dtype), self.model(shape, dtype), dtype)

    def check_optional_backward_outputs(self, shape, dtype):
        """A NULL bottom_diff, scale_diff or shift_diff skips that output and nothing else (run checks the prefill of
        the ones left out); with none of the three the call is refused."""
        from mms_answer_selection_amd import capi
        inp = self.inputs(shape, dtype)
        full = self.run(inp, shape[4:], dtype)
        for mask in range(1, 7):
            outputs = tuple(bool(mask >> b & 1) for b in range(3))
            part = self.run(inp, shape[4:], dtype, outputs=outputs)
            assert len(part) == len(full) - 2 * outputs.count(False)
            for k, v in part.items():
                assert_words_equal(v, full[k], "%s with outputs %s" % (k, outputs))
        with pytest.raises(capi.MMSError):
            self.run(inp, shape[4:], dtype, outputs=(False, False, False))


# ---- TEST-phase Convolution -> BN -> pooling -> TanH -------------------------------------------------------------
NAMES = ("x", "weight", "bias", "mean", "var", "scale", "shift")


def cshape(st, N=None):
    from mms_answer_selection_amd import conv
    s = st.conv
    return conv.conv_shape(s.N if N is None else N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group)


class GuardedWorkspace:
    """What capi._scratch asks a Workspace for: exactly the queried bytes, every word a NaN, between two zones of
    sentinels."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.nbytes, self.asked = nbytes, None
        self.buf = torch.full((2 * V.GUARD + nbytes // 4,), V.SENTINEL, dtype=torch.float32, device="cuda")
        self.buf[V.GUARD:V.GUARD + nbytes // 4].fill_(float("nan"))

    def get(self, nbytes, device):
        self.asked = nbytes
        assert nbytes == self.nbytes
        return (self.buf[V.GUARD:].data_ptr(), nbytes) if nbytes else (None, 0)

    def check(self):
        b = V.host(self.buf)
        assert self.asked == self.nbytes
        assert (b[:V.GUARD] == V.SENTINEL).all() and (b[V.GUARD + self.nbytes // 4:] == V.SENTINEL).all(), \
            "workspace guard"


class ConvStage:
    """The calls `name`_route / _workspace_bytes / _forward (and their _f64 forms) of mms_answer_selection_amd's module
    `name`, against reference module R.  assert_input: what holds an input to its words after a call (the MaxPool
    suite's inputs may hold a NaN)."""

    def __init__(self, name, R, assert_input):
        self.name, self.R, self.assert_input = name, R, assert_input
        self.inputs, self.model = shared_model(R, lambda st, inp: (st, inp))

    def mod(self):
        return importlib.import_module("mms_answer_selection_amd." + self.name)

    def fn(self, stem, dtype=np.float32):
        return getattr(self.mod(), "%s_%s%s" % (self.name, stem, "" if dtype == np.float32 else "_f64"))

    def route_of(self, st):
        return self.fn("route")(cshape(st), st.pool)

    def named_route(self, st):
        """The forced route whose words the main call must give: the one the route call names."""
        return {self.mod().ROUTE_FUSED: "fused", self.mod().ROUTE_SEQUENCE: "sequence"}[self.route_of(st)]

    def query(self, st, dtype, route):
        return self.fn("workspace_bytes", dtype)(cshape(st), st.pool, route=route)

    def run(self, st, inp, dtype=np.float32, route="auto", shift=0, guarded_ws=False, save_pool=True):
        """One forward.  top and save_pool start as NaN between guard zones; x, weight, top and save_pool are `shift`
        elements off a 16-byte boundary.  -> {"top"[, "save_pool"]} on the host; the inputs are checked to be
        unchanged."""
        s, pooled = st.conv, self.R.pooled_shape(st)
        dev = {k: (None if inp[k] is None else V.placed(inp[k], dtype, shift)) for k in NAMES}
        nan = float("nan")
        top = V.Guarded(pooled, dtype, nan, shift)
        sp = V.Guarded(pooled, dtype, nan, shift) if save_pool else None
        fused = route == "fused"                                                            # fused takes no workspace
        ws = GuardedWorkspace(self.query(st, dtype, route)) if guarded_ws and not fused else None
        got = self.fn("forward", dtype)(dev["x"], dev["weight"], dev["bias"], st.pool, dev["mean"], dev["var"],
                                        dev["scale"], dev["shift"], top.t, sp.t if sp else None, stride=s.stride,
                                        pad=s.pad, group=s.group, ws=ws, route=route)
        assert got is top.t
        torch.cuda.synchronize()
        if ws:
            ws.check()
        out = dict(top=top.host("top"))
        if sp:
            out["save_pool"] = sp.host("save_pool")
        for k in NAMES:
            if inp[k] is not None:
                self.assert_input(V.host(dev[k]), np.array(inp[k], dtype=dtype), k + " is an input")
        return out

    def check_integer_probe_fused_equals_sequence(self, st):
        """top and save_pool of the fused route, the sequence route and the main call equal word for word, and
        save_pool equals the float32 restatement of the finish."""
        R, run = self.R, self.run
        assert R.probe_bound(st) < 2 ** 24
        inp = R.integer_probe(st, SEED)
        fused, seq, auto = run(st, inp, route="fused"), run(st, inp, route="sequence"), run(st, inp)
        want_top, want_sp = R.probe_outputs(st, inp)
        for k in ("top", "save_pool"):
            assert not np.isnan(fused[k]).any(), k
            assert_words_equal(fused[k], seq[k], "integer probe, fused against sequence, " + k)
            assert_words_equal(auto[k], seq[k], "integer probe, the main call against sequence, " + k)
        assert_words_equal(fused["save_pool"], want_sp, "integer probe, save_pool against the float32 restatement")
        assert_close(fused["top"], want_top, TOL, "integer probe, top")

    def check_parity_and_determinism(self, st, dtype, same_words_stages):
        """Per shape and route: the conditioned inputs against the float64 model at the bar; a second run with every
        operand one element off a 16-byte boundary and a NaN-filled workspace of exactly the queried size gives the
        same words and leaves the workspace's guard zones alone.  The main call gives the words of the route it names.
        On same_words_stages: fused and sequence, the same words."""
        from mms_answer_selection_amd import capi
        R, run = self.R, self.run
        inp, want = self.inputs(st, dtype), self.model(st, dtype)
        reached = st in R.FUSED_STAGES
        if not reached:
            assert self.route_of(st) == self.mod().ROUTE_SEQUENCE
            with pytest.raises(capi.MMSError):
                run(st, self.inputs(st, np.float32), route="fused")       # refused host-side: the launch does not reach
        routes = ["fused", "sequence", "auto"] if dtype == np.float32 and reached else ["auto"]
        first = {}
        for route in routes:
            first[route] = run(st, inp, dtype, route)
            for k in ("top", "save_pool"):
                got = first[route][k]
                assert got.dtype == dtype and not np.isnan(got).any(), k
                scale = max(1.0, float(np.max(np.abs(want[k]))))
                print("%-8s %-9s %.3e" % (route, k, float(np.max(np.abs(got.astype(np.float64) - want[k]))) / scale))
        for route in routes:
            for k in ("top", "save_pool"):
                assert_close(first[route][k], want[k], BAR[dtype], "%s, %s route" % (k, route))
            second = run(st, inp, dtype, route, shift=1, guarded_ws=True)
            for k in ("top", "save_pool"):
                assert_words_equal(second[k], first[route][k], "%s, %s route, second run" % (k, route))
        if len(routes) == 3:
            named = self.named_route(st)
            for k in ("top", "save_pool"):
                assert_words_equal(first["auto"][k], first[named][k], "the main call against the route it names, " + k)
                if st in same_words_stages:
                    assert_words_equal(first["fused"][k], first["sequence"][k], "fused against sequence, " + k)

    def check_save_pool_is_optional(self, st):
        inp = self.inputs(st, np.float32)
        for route in ("auto", "sequence") + (("fused",) if st in self.R.FUSED_STAGES else ()):
            full = self.run(st, inp, route=route)
            part = self.run(st, inp, route=route, save_pool=False, guarded_ws=True)
            assert sorted(part) == ["top"]
            assert_words_equal(part["top"], full["top"], "top without a save_pool, %s route" % route)
        st64 = self.run(st, inp, np.float64, save_pool=False, guarded_ws=True)
        assert_close(st64["top"], self.model(st, np.float32)["top"], 1e-12, "top without a save_pool, f64")

    def check_sequence_route_is_the_two_public_calls(self, st, bn_pool_forward):
        """The main call on a shape it routes to the sequence, against mms_conv_forward_f32 and `bn_pool_forward`, the
        float BN -> pooling -> TanH forward of the method (TEST), issued here."""
        from mms_answer_selection_amd import conv
        assert self.route_of(st) == self.mod().ROUTE_SEQUENCE
        s, inp, pooled = st.conv, self.inputs(st, np.float32), self.R.pooled_shape(st)
        got = self.run(st, inp)
        dev = {k: (None if inp[k] is None else V.placed(inp[k], np.float32)) for k in NAMES}
        y = conv.conv_forward(dev["x"], dev["weight"], dev["bias"], stride=s.stride, pad=s.pad, group=s.group)
        top, sp = (torch.full(pooled, float("nan"), device="cuda") for _ in range(2))
        sm, ss = torch.empty(s.K, device="cuda"), torch.empty(s.K, device="cuda")
        bn_pool_forward(y, st.pool, dev["scale"], dev["shift"], dev["mean"], dev["var"], top, sp, sm, ss, phase=1)
        torch.cuda.synchronize()
        assert_words_equal(got["top"], V.host(top), "top")
        assert_words_equal(got["save_pool"], V.host(sp), "save_pool")

    def check_empty_batch_writes_nothing(self, dtype):
        fwd, t = self.fn("forward", dtype), V.TORCH[dtype]
        x = torch.empty(0, 4, 12, 12, dtype=t, device="cuda")
        w, bias = V.Guarded((6, 4, 3, 3), dtype, 1.0), V.Guarded((6,), dtype, 2.0)
        k = [V.Guarded((6,), dtype, 1.5) for _ in range(4)]
        for route in ("auto", "sequence") + (("fused",) if dtype == np.float32 else ()):
            top = fwd(x, w.t, bias.t, (2, 5), *(g.t for g in k), route=route)
            assert tuple(top.shape) == (0, 6, 5, 2)
            sp = torch.empty(0, 6, 5, 2, dtype=t, device="cuda")
            fwd(x, w.t, bias.t, (2, 5), *(g.t for g in k), top, sp, route=route)
        torch.cuda.synchronize()
        assert (w.host("weight") == 1.0).all() and (bias.host("bias") == 2.0).all()
        for g in k:
            assert (g.host("a BN array") == 1.5).all()


# ---- the CPU (ABI) suites ----------------------------------------------------------------------------------------
# BN -> pooling -> TanH: the parameter lists the headers declare, and the shapes every call is tried on
WS = ["void* workspace", "size_t workspace_bytes", "void* stream"]
DIMS = ["int N", "int C", "int H", "int W", "int kh", "int kw"]


def bn_pool_forward_params(t):
    """The parameter list of a BN -> pooling -> TanH forward of element type t, as the header declares it."""
    c = "const %s* " % t
    m = "%s* " % t
    return (["int phase"] + DIMS + [t + " bn_memory", c + "x", c + "scale", c + "shift", m + "running_mean",
                                    m + "running_var", m + "top", m + "save_pool", m + "save_mean", m + "save_std"] + WS)


LARGE = (1517, 32, 36, 36, 4, 4)          # needs a workspace
SMALL = (50, 64, 5, 5, 5, 5)              # does not
EMPTY = (0, 64, 5, 5, 5, 5)
BAD_SHAPES = [(-1, 2, 5, 5, 5, 5), (8, 0, 5, 5, 5, 5), (8, -2, 5, 5, 5, 5), (8, 2, 0, 5, 1, 5), (8, 2, 5, 0, 5, 1),
              (8, 2, -4, 4, 2, 2), (8, 2, 4, -4, 2, 2),
              (8, 2, 4, 4, 0, 2), (8, 2, 4, 4, 2, 0), (8, 2, 4, 4, -2, 2), (8, 2, 4, 4, 2, -2),
              (8, 2, 36, 36, 5, 4),                 # H % kh != 0
              (8, 2, 36, 36, 4, 5),                 # W % kw != 0
              (8, 2, 5, 5, 3, 5), (8, 2, 5, 5, 5, 3),
              (8, 2, 4, 4, 8, 2),                   # kh > H
              (8, 2, 4, 4, 2, 8),                   # kw > W
              (4096, 1024, 32, 16, 4, 4),           # N*C*H*W = 2^31 > INT_MAX: the reference indexes with int
              (2 ** 16, 2 ** 16, 1, 1, 1, 1),       # ... already in N*C
              (2 ** 15, 2 ** 15, 2, 1, 1, 1),       # ... in N*C*H
              (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 1, 1)]      # ... and past 64 bits

# the conv stage: the nine arrays of a forward, in the header's order, and the shapes and windows every call refuses
X, WEIGHT, BIAS, MEAN, VAR, SCALE, SHIFT, TOP, SAVE_POOL = range(9)


def _distinct(n=9):
    return [P + 64 * i for i in range(n)]


def _cshape(conv, st, N=None):
    s = st.conv
    return conv.conv_shape(s.N if N is None else N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group)


def _shape(conv, **kw):
    d = dict(N=2, C_=4, H=12, W=12, K=6, kernel=3, stride=1, pad=0, group=1, dilation=1)       # a 10 x 10 map
    d.update(kw)
    return conv.conv_shape(**d)


def _refused(conv):
    """(shape, (ph, pw), code): what mms_conv_forward refuses with its code, then the windows."""
    big = 2 ** 16
    shapes = [(_shape(conv, N=-1), INVALID), (_shape(conv, C_=0), INVALID), (_shape(conv, H=0), INVALID),
              (_shape(conv, W=-1), INVALID), (_shape(conv, K=0), INVALID), (_shape(conv, kernel=(0, 3)), INVALID),
              (_shape(conv, stride=(0, 1)), INVALID), (_shape(conv, group=0), INVALID),
              (_shape(conv, dilation=(0, 1)), INVALID), (_shape(conv, pad=(-1, 0)), INVALID),
              (_shape(conv, group=3), INVALID), (_shape(conv, kernel=13), INVALID),
              (_shape(conv, N=big, C_=big, H=1, W=1, kernel=1), INVALID),
              (_shape(conv, N=1, C_=1, H=4, W=4, K=2 ** 30, kernel=3, pad=1), INVALID),
              (_shape(conv, dilation=2), UNSUPPORTED), (_shape(conv, N=0, dilation=(1, 2)), UNSUPPORTED)]
    out = [(s, (2, 5), code) for s, code in shapes]
    good = _shape(conv)
    for pool in ((0, 2), (2, 0), (-1, 2), (2, -5), (3, 2), (2, 3), (20, 2), (2, 11), (4, 4)):
        out.append((good, pool, INVALID))
        out.append((_shape(conv, N=0), pool, INVALID))
    return out
