"""GPU suite: the Convolution calls (include/mms_conv.h, csrc/conv.hip) against tests/conv_reference.py.  Indexing,
flips, groups, borders and the accumulate-into rule are tested by EQUALITY on integer probes, whatever order a kernel
sums in; the conditioned inputs (tests/test_conv_reference.py shows them fit for it) are held to the float64 model at
the project's 1e-5 (float32) and 1e-12 (float64) in assert_close's metric; the fixed order and the workspace's
irrelevance by equality of words between two runs."""
import functools

import numpy as np
import pytest
import torch

import conv_reference as R
from util import SEED, TOL, assert_close

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
BAR = {np.float32: TOL, np.float64: 1e-12}
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
GUARD, SENTINEL = 64, -777.0
SHAPE_IDS = ["-".join(str(v) for v in s) for s in R.GPU_SHAPES]
OUTPUTS = ("bottom_diff", "weight_diff", "bias_diff")


def api(dtype):
    from mms_answer_selection_amd import conv
    if dtype == np.float32:
        return conv.conv_forward, conv.conv_backward
    return conv.conv_forward_f64, conv.conv_backward_f64


def cshape(s):
    from mms_answer_selection_amd import conv
    return conv.conv_shape(s.N, s.C, s.H, s.W, s.K, (s.kh, s.kw), s.stride, s.pad, s.group)


def host(t):
    return t.detach().cpu().numpy()


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    w = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.flatnonzero(got.reshape(-1).view(w) != want.reshape(-1).view(w))
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


class Guarded:
    """An array between two zones of 64 sentinel elements, `shift` elements off its buffer's (16-byte aligned) start."""

    def __init__(self, shape, dtype, fill, shift=0):
        self.n = int(np.prod(shape))
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=TORCH[dtype], device="cuda")
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.array(fill, dtype=dtype)))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (shift * self.t.element_size()) % 16

    def host(self, what):
        b = host(self.buf)
        assert (b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all(), what + ": guard overwritten"
        return b[self.lo:self.lo + self.n].reshape(tuple(self.t.shape)).copy()


def placed(a, dtype, shift=0):
    """a on the device, `shift` elements off a 16-byte boundary."""
    buf = torch.empty(a.size + shift, dtype=TORCH[dtype], device="cuda")
    t = buf[shift:].view(*a.shape)
    t.copy_(torch.from_numpy(np.array(a, dtype=dtype)))
    return t


@functools.lru_cache(maxsize=None)
def inputs(s, dtype):
    return R.conditioned_inputs(s, dtype, SEED)


@functools.lru_cache(maxsize=None)
def model(s, dtype):
    """The float64 model on the inputs as the device gets them, computed once and shared (never modified)."""
    out = R.model_outputs(s, inputs(s, dtype), np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probe(s):
    inp = R.integer_probe(s, SEED)
    out = R.model_outputs(s, inp, np.int64)
    for v in out.values():
        v.setflags(write=False)
    return inp, out


def nan_workspace(s, dtype):
    """A Workspace of the size the backward asks for, every word a NaN."""
    from mms_answer_selection_amd import capi, conv
    q = conv.conv_workspace_bytes if dtype == np.float32 else conv.conv_workspace_bytes_f64
    ws = capi.Workspace()
    ws.get(q(cshape(s)), torch.device("cuda", torch.cuda.current_device()))
    if ws.buf is not None:
        ws.buf.view(torch.float32).fill_(float("nan"))
    return ws


def run(s, inp, dtype, shift=0, ws=None, outputs=(True, True, True), route="auto"):
    """Forward, then backward on top of the initial parameter diffs.  top and bottom_diff start as NaN, between guard
    zones; x, weight, top_diff, top, bottom_diff and weight_diff are `shift` elements off a 16-byte boundary.
    -> {"top", "bottom_diff", "weight_diff"[, "bias_diff"]} on the host; an output not asked for is absent (and checked
    to be untouched)."""
    fwd, bwd = api(dtype)
    kw = dict(stride=s.stride, pad=s.pad, group=s.group, route=route)
    x, w, dy = (placed(inp[k], dtype, shift) for k in ("x", "weight", "top_diff"))
    bias = None if inp["bias"] is None else placed(inp["bias"], dtype)
    nan = float("nan")
    top = Guarded(dy.shape, dtype, nan, shift)
    assert fwd(x, w, bias, top.t, **kw) is top.t
    b = dict(bottom_diff=Guarded(x.shape, dtype, nan, shift),
             weight_diff=Guarded(w.shape, dtype, inp["weight_diff0"], shift))
    if inp["bias_diff0"] is not None:
        b["bias_diff"] = Guarded((s.K,), dtype, inp["bias_diff0"])
    given = {k: (b[k].t if k in b and want else None) for k, want in zip(OUTPUTS, outputs)}
    bwd(x, w, dy, ws=ws, **given, **kw)
    out = dict(top=top.host("top"))
    for k, v in b.items():
        h = v.host(k)
        if given[k] is not None:
            out[k] = h
        elif k == "bottom_diff":
            assert np.isnan(h).all(), "bottom_diff was not asked for"
        else:
            assert_words_equal(h, np.array(inp[k + "0"], dtype=dtype), k + " was not asked for")
    for name, t, a in (("x", x, inp["x"]), ("weight", w, inp["weight"]), ("top_diff", dy, inp["top_diff"])):
        assert_words_equal(host(t), np.array(a, dtype=dtype), name + " is an input")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("s", R.GPU_SHAPES, ids=SHAPE_IDS)
def test_probe_parity_and_determinism(s, dtype, hiplib):
    """Per shape: (1) the integer probe equals the int64 reference, bit for bit, in all four outputs, the parameter
    diffs on top of non-zero initial diffs; (2) the conditioned inputs against the float64 model at the bar; (3) a second
    run with a NaN-filled workspace and every operand one element off a 16-byte boundary gives the same words."""
    assert R.probe_bound(s) < 2 ** 24
    pin, pwant = probe(s)
    got = run(s, pin, dtype)
    assert sorted(got) == sorted(pwant)
    for k, v in pwant.items():
        assert_words_equal(got[k], v.astype(dtype), "integer probe, " + k)
    inp = inputs(s, dtype)
    first = run(s, inp, dtype)
    want = model(s, dtype)
    for k in sorted(want):
        assert first[k].dtype == dtype and not np.isnan(first[k]).any(), k
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        print("%-12s %.3e" % (k, float(np.max(np.abs(first[k].astype(np.float64) - want[k]))) / scale))
    for k in sorted(want):
        assert_close(first[k], want[k], BAR[dtype], k)
    second = run(s, inp, dtype, shift=1, ws=nan_workspace(s, dtype))
    for k in first:
        assert_words_equal(second[k], first[k], k + ", second run: NaN workspace, operands off by one element")


def test_the_list_reaches_both_routes_in_every_pass(hiplib):
    from mms_answer_selection_amd import conv
    for p in (conv.PASS_FORWARD, conv.PASS_BOTTOM_DIFF, conv.PASS_PARAM_DIFF):
        assert {conv.conv_route(cshape(s), p) for s in R.GPU_SHAPES} == {conv.ROUTE_FAST, conv.ROUTE_GENERIC}
        for s in R.V4_SHAPES:
            assert conv.conv_route(cshape(s), p) == conv.ROUTE_FAST


@pytest.mark.parametrize("s", R.V4_SHAPES, ids=SHAPE_IDS[:2])
def test_fast_and_generic_routes_agree(s, hiplib):
    """network_v4's layers on the matrix pipe and on the direct kernels: equal on the integer probe, within TOL of each
    other (and each of the float64 model) on the conditioned inputs."""
    pin, pwant = probe(s)
    got = run(s, pin, np.float32, route="generic")
    for k, v in pwant.items():
        assert_words_equal(got[k], v.astype(np.float32), "integer probe on the generic route, " + k)
    inp = inputs(s, np.float32)
    fast, generic = run(s, inp, np.float32), run(s, inp, np.float32, route="generic")
    want = model(s, np.float32)
    for k in sorted(want):
        assert_close(generic[k], want[k], TOL, k + ", generic route against the model")
        assert_close(fast[k], generic[k], TOL, k + ", fast against generic")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_empty_batch_writes_nothing(dtype, hiplib):
    fwd, bwd = api(dtype)
    t = TORCH[dtype]
    x = torch.empty(0, 4, 9, 9, dtype=t, device="cuda")
    w = Guarded((6, 4, 3, 3), dtype, 1.0)
    top, dy = torch.empty(0, 6, 7, 7, dtype=t, device="cuda"), torch.empty(0, 6, 7, 7, dtype=t, device="cuda")
    dw, db, bias = Guarded((6, 4, 3, 3), dtype, 123.0), Guarded((6,), dtype, 123.0), Guarded((6,), dtype, 2.0)
    assert tuple(fwd(x, w.t, bias.t).shape) == (0, 6, 7, 7)
    fwd(x, w.t, bias.t, top)
    bwd(x, w.t, dy, torch.empty_like(x), dw.t, db.t)
    assert (dw.host("weight_diff") == 123.0).all() and (db.host("bias_diff") == 123.0).all()
    assert (w.host("weight") == 1.0).all() and (bias.host("bias") == 2.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("s", [R.GPU_SHAPES[1], R.GPU_SHAPES[2], R.GPU_SHAPES[5]], ids=[SHAPE_IDS[i] for i in (1, 2, 5)])
def test_optional_backward_outputs(s, dtype, hiplib):
    """Each of bottom_diff, weight_diff, bias_diff left out alone and in pairs, on both routes: those given have the
    words of the full run, the others are untouched (inside run); none of the three is refused."""
    from mms_answer_selection_amd import capi
    inp = inputs(s, dtype)
    full = run(s, inp, dtype)
    for mask in range(1, 7):
        outputs = tuple(bool(mask >> b & 1) for b in range(3))
        if not s.bias and outputs == (False, False, True):          # bias_diff alone, and the layer has no bias
            with pytest.raises(capi.MMSError):
                run(s, inp, dtype, outputs=outputs)
            continue
        part = run(s, inp, dtype, outputs=outputs)
        assert sorted(part) == sorted(["top"] + [k for k, o in zip(OUTPUTS, outputs) if o and k in full])
        for k, v in part.items():
            assert_words_equal(v, full[k], "%s with outputs %s" % (k, outputs))
    with pytest.raises(capi.MMSError):
        run(s, inp, dtype, outputs=(False, False, False))


def test_accumulation_is_on_top_of_what_is_there(hiplib):
    """Two backward calls into the same diffs add twice; bottom_diff is overwritten each time."""
    from mms_answer_selection_amd import conv
    s = R.GPU_SHAPES[2]
    pin, _ = probe(s)
    x, w, dy = (placed(pin[k], np.float32) for k in ("x", "weight", "top_diff"))
    dx = torch.full(x.shape, 55.0, device="cuda")
    dw, db = torch.zeros_like(w), torch.zeros(s.K, device="cuda")
    conv.conv_backward(x, w, dy, dx, dw, db)
    once = [host(t).copy() for t in (dx, dw, db)]
    conv.conv_backward(x, w, dy, dx, dw, db)
    assert_words_equal(host(dx), once[0], "bottom_diff, second call")
    assert_words_equal(host(dw), 2 * once[1], "weight_diff, second call")
    assert_words_equal(host(db), 2 * once[2], "bias_diff, second call")
