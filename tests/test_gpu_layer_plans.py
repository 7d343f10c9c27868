"""GPU suite: FM, BN and BN -> AvePool -> TanH on the launch plans that large batches take (tests/layer_plans.py has
the plans restated and the shapes; tests/test_layer_plans.py proves on the CPU which regime each shape reaches and that
the parity inputs are conditioned).

FM: every lane-walk width S = 8 / 16 / 32 / 64, both sides of the three N thresholds, every hand-down to a smaller S,
multi-panel and no-panel plans at S = 64, the last lane-walk shape and the one-thread float route, the bias_diff chain
at multiples of its step -- every comparison is word equality with tests/fm_reference.py.
BN and BN-pool: channels of more than 64 x 2048 groups (64 chunks of ceil(groups / 64), the last ragged; for BN-pool
also 63 chunks under a 64-chunk workspace) -- the workspace queries against the restated routes, parity at the
project's 1e-5 / 1e-12, and integer probes whose chunk sums and statistics are exact, compared word for word."""
import numpy as np
import pytest
import torch

import bn_pool_reference as BPR
import bn_reference as BNR
import layer_plans as L
import test_gpu_bn as bn
import test_gpu_bn_pool as bp
from pooled_stage_suite import check_parity, same_words
from test_gpu_bn import Guarded, assert_words_equal, host, placed
from test_gpu_fm import BIAS, case as fm_case
from util import SEED

pytestmark = pytest.mark.gpu

F32 = np.float32
WS_GUARD = 64                    # guard elements on either side of a workspace of exactly the queried size
NAN_BYTE, GUARD_BYTE = 0xFF, 0xA5


# ---- FM ----------------------------------------------------------------------------------------------------------
def fm_three_calls(c, shape, shift=0):
    """forward, backward and the fused call; top and bottom_diff start as NaN and bias_diff as 123, each between
    64-element guard zones (Guarded.host checks them); x, top_diff and bottom_diff are `shift` floats off a 16-byte
    boundary.  -> top, bottom_diff, bias_diff of the separate calls, then of the fused call."""
    from mms_answer_selection_amd import capi
    N, nan = shape[0], float("nan")
    x, g = placed(c["x"], F32, shift), placed(c["g"], F32, shift)
    bias = placed(np.array([BIAS], F32), F32)
    top, bd, db = Guarded((N,), F32, nan), Guarded(shape, F32, nan, shift), Guarded((1,), F32, 123.0)
    capi.fm_forward(x, top.t, bias=bias)
    capi.fm_backward(x, g, bd.t, db.t)
    top2, bd2, db2 = Guarded((N,), F32, nan), Guarded(shape, F32, nan, shift), Guarded((1,), F32, 123.0)
    capi.fm_forward_backward(x, g, top2.t, bd2.t, bias=bias, bias_diff=db2.t)
    names = ("top", "bottom_diff", "bias_diff", "fused top", "fused bottom_diff", "fused bias_diff")
    return [v.host(n) for n, v in zip(names, (top, bd, db, top2, bd2, db2))]


def fm_check(outs, c):
    top, bd, db, top2, bd2, db2 = outs
    assert_words_equal(top, c["top"], "top")
    assert_words_equal(bd, c["bottom_diff"], "bottom_diff")
    assert_words_equal(db, c["bias_diff"], "bias_diff")
    assert_words_equal(top2, c["top"], "fused top")
    assert_words_equal(bd2, c["bottom_diff"], "fused bottom_diff")
    assert_words_equal(db2, c["bias_diff"], "fused bias_diff")
    for a in outs:
        assert not np.isnan(a).any()                 # every element of every output was written


@pytest.mark.parametrize("shape,S,what", L.FM_SHAPES, ids=[str(s[0]) for s in L.FM_SHAPES])
def test_fm_words_do_not_depend_on_the_plan(shape, S, what, hiplib):
    """All three float calls at every shape of layer_plans.FM_SHAPES: the words of the reference's loops, whatever S,
    P and stride the plan chose and on the one-thread route, where the fused call is two launches and must still
    produce bias_diff and overwrite every element of bottom_diff."""
    plan = L.fm_plan(*shape)
    assert (plan[0] if plan else None) == S, what
    c = fm_case(shape)
    fm_check(fm_three_calls(c, shape), c)


def test_fm_placement_at_S_32(hiplib):
    """x, top_diff and bottom_diff one float off a 16-byte boundary at an S = 32 plan: the words of the aligned run."""
    shape = L.FM_PLACEMENT_SHAPE
    assert L.fm_plan(*shape)[0] == 32
    c = fm_case(shape)
    aligned, shifted = fm_three_calls(c, shape), fm_three_calls(c, shape, shift=1)
    fm_check(shifted, c)
    for a, b in zip(aligned, shifted):
        assert_words_equal(b, a, "off by one float")


# ---- workspaces of exactly the queried size ------------------------------------------------------------------------
class ExactWorkspace:
    """A capi.Workspace whose buffer is exactly `need` bytes, every word a NaN, between two guard zones of
    WS_GUARD elements."""

    def __init__(self, need, dtype):
        from mms_answer_selection_amd import capi
        self.need, self.pad = need, WS_GUARD * np.dtype(dtype).itemsize
        self.whole = torch.full((need + 2 * self.pad,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.ws = capi.Workspace()
        self.ws.buf = self.whole[self.pad:self.pad + need]
        self.ws.buf.fill_(NAN_BYTE)
        assert self.ws.buf.data_ptr() % 16 == 0 and np.isnan(self.words(dtype)).all()
        ptr, size = self.ws.get(need, self.ws.buf.device)
        assert (ptr, size) == (self.ws.buf.data_ptr(), need)

    def words(self, dtype):
        return host(self.ws.buf).view(dtype)

    def guards_intact(self):
        b = host(self.whole)
        assert self.ws.buf.numel() == self.need, "the workspace was replaced: the query asked for more"
        assert (b[:self.pad] == GUARD_BYTE).all() and (b[self.pad + self.need:] == GUARD_BYTE).all(), \
            "written outside the workspace"


def nan_outputs(shapes, dtype):
    return [torch.full(tuple(s), float("nan"), dtype=bn.TORCH[dtype], device="cuda") for s in shapes]


# ---- BN ----------------------------------------------------------------------------------------------------------
def bn_route_checked(case):
    """The library's workspace query against the restated route: 64 chunks of more than the minimum size."""
    (N, C, S), dtype = case
    item = np.dtype(dtype).itemsize
    small, chunks, gpc = L.bn_route(N, S, item)
    need = bn.api(dtype)[2](N, C, S)
    assert need == L.bn_workspace_bytes(N, C, S, item) == C * chunks * 4 * item
    assert not small and chunks == 64 and gpc > 2048
    return need, chunks, gpc


@pytest.mark.parametrize("case", L.BN_CASES, ids=L.case_id)
def test_bn_parity_past_64_minimum_chunks(case, hiplib):
    """Every output of TRAIN forward, TEST forward and both backwards against the float64 model at the existing bars;
    a second run on a workspace of exactly the queried size that starts as NaN gives the same words and writes nothing
    outside it."""
    shape, dtype = case
    need, _, _ = bn_route_checked(case)
    inp = bn.inputs(shape, dtype)
    first = bn.run(inp, dtype)
    bn.check_parity(first, bn.model(shape, dtype), dtype)
    ws = ExactWorkspace(need, dtype)
    second = bn.run(inp, dtype, ws=ws.ws)
    ws.guards_intact()
    for k in first:
        assert_words_equal(second[k], first[k], k + ", NaN-filled workspace")


@pytest.mark.parametrize("case", L.BN_CASES, ids=L.case_id)
def test_bn_integer_probe_pins_the_chunk_boundaries(case, hiplib):
    """x integer-valued, |x| <= 4: every sum over any part of a channel is an integer below 2^24 (asserted from the
    shape in probe_x), exact in any order.  After TRAIN forward each chunk's workspace slots 0 and 1 are the int64 sums
    of x and x*x over that chunk's groups as the restated route places them -- a boundary one group off changes a
    word -- and save_mean, save_std, the running blobs and top are numpy's evaluation of the documented expressions on
    the exact totals, word for word."""
    (N, C, S), dtype = case
    shape = case[0]
    need, chunks, gpc = bn_route_checked(case)
    fwd = bn.api(dtype)[0]
    inp = dict(bn.inputs(shape, dtype))
    inp["x"] = L.probe_x(shape, dtype, SEED + 5)
    ws = ExactWorkspace(need, dtype)
    top, save_mean, save_std = nan_outputs((shape, (C,), (C,)), dtype)
    rm, rv = placed(inp["running_mean"], dtype), placed(inp["running_var"], dtype)
    fwd(placed(inp["x"], dtype), placed(inp["scale"], dtype), placed(inp["shift"], dtype), rm, rv, top, save_mean,
        save_std, phase=BNR.TRAIN, bn_memory=BNR.BN_MEMORY, ws=ws.ws)
    ws.guards_intact()
    V = 16 // np.dtype(dtype).itemsize
    groups = (N * S + V - 1) // V
    xi = np.ascontiguousarray(inp["x"].transpose(1, 0, 2)).reshape(C, N * S).astype(np.int64)
    parts = np.array([[xi[:, lo * V:hi * V].sum(axis=1), (xi[:, lo * V:hi * V] ** 2).sum(axis=1)]
                      for lo, hi in L.chunk_bounds(groups, gpc, chunks)])            # (chunks, 2, C); slices clip at N*S
    assert np.abs(parts).max() < 2 ** 24 and parts[:, 1].sum(axis=0).max() < 2 ** 24
    sums = ws.words(dtype).reshape(C, chunks, 4)
    assert_words_equal(sums[:, :, 0], parts[:, 0].T.astype(dtype), "workspace slot 0: each chunk's sum of x")
    assert_words_equal(sums[:, :, 1], parts[:, 1].T.astype(dtype), "workspace slot 1: each chunk's sum of x*x")
    t = dtype
    tot = parts.sum(axis=0).astype(t)
    mean = t(1.0 / N) * (t(1.0 / S) * tot[0])
    var = t(1.0 / N) * (t(1.0 / S) * tot[1]) - mean * mean
    std = np.sqrt(var + t(1e-9))
    keep, take = t(BNR.BN_MEMORY), t(1) - t(BNR.BN_MEMORY)
    assert mean.dtype == t and std.dtype == t
    assert_words_equal(host(save_mean), mean, "save_mean on the exact totals")
    assert_words_equal(host(save_std), std, "save_std on the exact totals")
    assert_words_equal(host(rm), take * mean + keep * inp["running_mean"], "running mean: the axpby expression")
    assert_words_equal(host(rv), take * var + keep * inp["running_var"], "running variance: the axpby expression")
    c = (None, slice(None), None)
    want_top = (inp["x"] + (-mean)[c]) / std[c] * inp["scale"][c] + inp["shift"][c]
    assert_words_equal(host(top), want_top, "top: every element normalised once with these statistics")


# ---- BN -> AvePool -> TanH -------------------------------------------------------------------------------------------
def bp_route_checked(case):
    (N, C, H, W, kh, kw), dtype = case
    item = np.dtype(dtype).itemsize
    small, chunks, wpc = L.bp_route(N, H, W, kh, kw, item)
    windows, least = N * H * W // (kh * kw), L.bp_least(kh, kw, item)
    need = bp.api(dtype)[2](*case[0])
    assert need == L.bp_workspace_bytes(*case[0], item) == C * min(64, (windows + least - 1) // least) * 4 * item
    assert not small and wpc > least and chunks == (63 if case[0] == L.BP_63_CHUNKS else 64)
    assert need == C * 64 * 4 * item                 # for the 63-chunk shape too: the query answers for 64
    return need, chunks, wpc


@pytest.mark.parametrize("case", L.BP_CASES, ids=L.case_id)
def test_bn_pool_parity_past_64_minimum_chunks(case, hiplib):
    """Parity of every output at the existing bars; a second run on a NaN-filled workspace of exactly the queried size
    gives the same words, and the guard zones around that workspace stay intact (the 63-chunk shape included)."""
    shape, dtype = case
    need, _, _ = bp_route_checked(case)
    inp = bp.inputs(shape, dtype)
    first = bp.run(inp, shape[4:], dtype)
    check_parity(first, bp.model(shape, dtype), dtype)
    ws = ExactWorkspace(need, dtype)
    second = bp.run(inp, shape[4:], dtype, ws=ws.ws)
    ws.guards_intact()
    same_words(second, first, "NaN-filled workspace")


@pytest.mark.parametrize("case", L.BP_CASES, ids=L.case_id)
def test_bn_pool_integer_probe_pins_the_chunk_boundaries(case, hiplib):
    """test_gpu_bn_pool.py::test_integer_probe with |x| <= 4, its bound on N*H*W replaced by the asserted
    sum x*x < 2^24: save_mean, save_std, the running blobs and save_pool, both phases, word for word.  And the chunk
    sums themselves: after a TRAIN forward of its own, slots 0 and 1 of chunk k are the int64 sums over the windows the
    restated route gives chunk k, laid out for the route's chunk count (63 where that is the count)."""
    shape, dtype = case
    N, C, H, W, kh, kw = shape
    need, chunks, wpc = bp_route_checked(case)
    inp = dict(bp.inputs(shape, dtype))
    inp["x"] = L.probe_x(shape, dtype, SEED + 5)
    got = bp.run(inp, (kh, kw), dtype)
    want = bp.exact_statistics(inp["x"], (kh, kw), inp["running_mean"], inp["running_var"], dtype)
    for k in sorted(want):
        assert_words_equal(got[k], want[k], k)
    for k, v in got.items():
        assert not np.isnan(v).any(), k

    fwd = bp.api(dtype)[0]
    ws = ExactWorkspace(need, dtype)
    pooled = BPR.pooled_shape(shape)
    top, save_pool, save_mean, save_std = nan_outputs((pooled, pooled, (C,), (C,)), dtype)
    fwd(placed(inp["x"], dtype), (kh, kw), placed(inp["scale"], dtype), placed(inp["shift"], dtype),
        placed(inp["running_mean"], dtype), placed(inp["running_var"], dtype), top, save_pool, save_mean, save_std,
        phase=BPR.TRAIN, bn_memory=BPR.BN_MEMORY, ws=ws.ws)
    ws.guards_intact()
    windows = N * (H // kh) * (W // kw)
    per_window = inp["x"].reshape(N, C, H // kh, kh, W // kw, kw).transpose(1, 0, 2, 4, 3, 5).reshape(C, windows, kh * kw)
    wi = per_window.astype(np.int64)
    sx, sxx = wi.sum(axis=2), (wi * wi).sum(axis=2)                                  # (C, windows)
    bounds = L.chunk_bounds(windows, wpc, chunks)
    want0 = np.stack([sx[:, lo:hi].sum(axis=1) for lo, hi in bounds], axis=1)        # (C, chunks)
    want1 = np.stack([sxx[:, lo:hi].sum(axis=1) for lo, hi in bounds], axis=1)
    assert np.abs(want0).max() < 2 ** 24 and want1.sum(axis=1).max() < 2 ** 24
    used = ws.words(dtype)[:C * chunks * 4].reshape(C, chunks, 4)
    assert_words_equal(used[:, :, 0], want0.astype(dtype), "workspace slot 0: each chunk's sum of x")
    assert_words_equal(used[:, :, 1], want1.astype(dtype), "workspace slot 1: each chunk's sum of x*x")
    assert_words_equal(host(save_mean), want["train_save_mean"], "save_mean, workspace of exactly the queried size")
    assert_words_equal(host(save_pool), want["train_save_pool"], "save_pool, workspace of exactly the queried size")
