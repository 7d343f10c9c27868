"""GPU suite: the BN -> AvePool -> TanH calls of the C ABI (include/mms.h mms_bn_pool_tanh_*, csrc/bn_pool.hip) against
the float64 run of tests/bn_pool_reference.py -- the three reference layers in sequence -- on the same inputs.  Parity is
the project's 1e-5 (float32) and 1e-12 (float64) in assert_close's metric, on inputs tests/test_bn_pool_reference.py
shows to be conditioned for it; everything a tolerance would hide -- the order of the sums, strides, alignment, what the
workspace held, what is and is not written -- is tested by equality of words."""
import numpy as np
import pytest
import torch

import bn_pool_reference as R
from pooled_stage_suite import BnPool, same_words
from test_gpu_bn import DTYPES, IDS, assert_words_equal, host
from util import SEED

pytestmark = pytest.mark.gpu

S = BnPool("capi", "bn_pool_tanh", R, shift_in_backward=False)
api, inputs, model, run = S.api, S.inputs, S.model, S.run
SMALL_ROUTE = [(3, 2, 36, 36, 4, 4), (7, 4, 5, 5, 5, 5)]                      # compile-time windows, one launch
LARGE_ROUTE = [(20, 3, 36, 36, 4, 4), (65, 5, 9, 37, 3, 37)]                  # two launches; a run-time window


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", R.PARITY_SHAPES, ids=str)
def test_parity_and_determinism(shape, dtype, hiplib):
    S.check_parity_and_determinism(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_variance_is_exact(dtype, hiplib):
    S.check_zero_variance_is_exact(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_both_sides_of_the_routing_threshold(dtype, hiplib):
    """BnPool.check_both_sides_of_the_routing_threshold; the shapes' 2 x 4 windows are 16-byte rows of a size the
    kernels learn at run time."""
    below, above = R.THRESHOLD_SHAPES[dtype]
    per_group = 16 // np.dtype(dtype).itemsize
    assert below[1:] == above[1:] and above[0] == below[0] + 1
    assert below[0] * below[2] * below[3] == 4096 * per_group
    S.check_both_sides_of_the_routing_threshold(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 3, 4, 6, 2, 3), (65, 5, 9, 37, 3, 37)], ids=str)
def test_optional_backward_outputs(shape, dtype, hiplib):
    """BnPool.check_optional_backward_outputs, on both routes."""
    S.check_optional_backward_outputs(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(3, 2, 36, 36, 4, 4), (20, 3, 36, 36, 4, 4), (129, 3, 8, 16, 2, 4)], ids=str)
def test_unaligned_bases_give_the_same_words(shape, dtype, hiplib):
    """Every operand 1, 2 and 3 elements off a 16-byte boundary (window rows read and written one element at a time
    instead of 16 bytes at a time, except where 2 doubles are 16 bytes again) gives the words of the aligned run:
    compile-time and run-time windows, both routes."""
    inp = inputs(shape, dtype)
    aligned = run(inp, shape[4:], dtype)
    for shift in (1, 2, 3):
        same_words(run(inp, shape[4:], dtype, shift=shift), aligned, "off by %d elements" % shift)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(20, 3, 36, 36, 4, 4), (130, 3, 25, 41, 5, 1)], ids=str)
def test_workspace_content_and_size_do_not_matter(shape, dtype, hiplib):
    """The two-launch route with a workspace of its own that starts as NaN, then holds the previous call's content
    (this shape's, then another's), then is the largest the query can return for this C: the words of the first run."""
    from mms_answer_selection_amd import capi
    _, _, query = api(dtype)
    inp = inputs(shape, dtype)
    need = query(*shape)
    C = shape[1]
    largest = C * 64 * 4 * np.dtype(dtype).itemsize
    assert 0 < need < largest and query(2 ** 31 // (C * shape[2] * shape[3]) - 1, *shape[1:]) == largest
    want = run(inp, shape[4:], dtype)
    ws = capi.Workspace()
    ws.get(need, torch.device("cuda", torch.cuda.current_device()))
    assert ws.buf.numel() == need
    ws.buf.fill_(0xFF)                                       # every word a NaN
    assert np.isnan(host(ws.buf).view(dtype)).all()
    same_words(run(inp, shape[4:], dtype, ws=ws), want, "workspace of NaNs")
    same_words(run(inp, shape[4:], dtype, ws=ws), want, "workspace with this shape's last sums")
    other = (13, C, 36, 36, 4, 4)
    assert 0 < query(*other) <= need
    run(inputs(other, dtype), other[4:], dtype, ws=ws)
    assert ws.buf.numel() == need
    same_words(run(inp, shape[4:], dtype, ws=ws), want, "workspace with another shape's sums")
    big = capi.Workspace()
    big.get(largest, ws.buf.device)
    big.buf.fill_(0xFF)
    same_words(run(inp, shape[4:], dtype, ws=big), want, "the largest workspace of this C")


def exact_statistics(x, kernel, rm, rv, dtype):
    """The formulas of include/mms.h in `dtype` on integer-valued x, whose sums are exact in any order."""
    N, C, H, W = x.shape
    kh, kw = kernel
    t = dtype
    xi = x.astype(np.int64)
    sx, sxx = xi.sum(axis=(0, 2, 3)), (xi * xi).sum(axis=(0, 2, 3))
    assert np.abs(sx).max() <= 2 ** 24 and sxx.max() <= 2 ** 24
    mean = t(1.0 / N) * (t(1.0 / (H * W)) * sx.astype(t))
    var = t(1.0 / N) * (t(1.0 / (H * W)) * sxx.astype(t)) - mean * mean
    keep, take = t(R.BN_MEMORY), t(1) - t(R.BN_MEMORY)
    m = xi.reshape(N, C, H // kh, kh, W // kw, kw).sum(axis=(3, 5)).astype(t) / t(kh * kw)
    c = (None, slice(None), None, None)
    out = {}
    for name, mu, v in (("train", mean, var), ("test", rm, rv)):
        std = np.sqrt(v + t(1e-9))
        out[name + "_save_mean"], out[name + "_save_std"] = mu, std
        out[name + "_save_pool"] = (m + (-mu)[c]) / std[c]
    out["train_running_mean"] = take * mean + keep * rm
    out["train_running_var"] = take * var + keep * rv
    for v in out.values():
        assert v.dtype == t
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SMALL_ROUTE + LARGE_ROUTE, ids=str)
def test_integer_probe(shape, dtype, hiplib):
    """x integer-valued with |x| <= 8 and N*H*W <= 2^18: every sum is exact in any order, so save_mean, save_std, the
    running blobs and save_pool are, word for word, numpy's evaluation of the documented formulas in the element type
    -- one rounding per operation, the two scalings, sqrt and the divisions as written.  Both routes, both phases."""
    _, _, query = api(dtype)
    assert (query(*shape) == 0) == (shape in SMALL_ROUTE)
    assert shape[0] * shape[2] * shape[3] <= 2 ** 18
    inp = dict(inputs(shape, dtype))
    r = np.random.default_rng(SEED + 5)
    inp["x"] = r.integers(-8, 9, size=shape[:4]).astype(dtype)
    got = run(inp, shape[4:], dtype)
    want = exact_statistics(inp["x"], shape[4:], inp["running_mean"], inp["running_var"], dtype)
    for k in sorted(want):
        assert_words_equal(got[k], want[k], k)
    for k, v in got.items():
        assert not np.isnan(v).any(), k
