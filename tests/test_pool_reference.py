"""CPU suite: tests/pool_reference.py, the model the GPU tests of Pooling and TanH hold the kernels to, is itself held to
torch -- its output size, MAX values and indices, AVE values and both backwards equal torch's exactly on integer-valued
data, where no order of additions can show -- and the probes that are to catch a wrong order of additions are shown to
be sensitive to it: exchanging two adjacent contributions in the model changes a word."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_reference as R
from util import SEED

DTYPES = [np.float32, np.float64]
# what torch accepts: pad <= kernel / 2
TORCH_SHAPES = [s for s in R.SHAPES + R.PLAN_SHAPES if all(2 * p <= k for p, k in zip(s.pad, s.kernel))]


def _torch_forward(sh, method, x):
    if method == R.MAX:
        return F.max_pool2d(x, sh.kernel, sh.stride, sh.pad, ceil_mode=True, return_indices=True)
    return F.avg_pool2d(x, sh.kernel, sh.stride, sh.pad, ceil_mode=True, count_include_pad=True), None


def _pool_sizes(sh):
    PH, PW = R.output_dims(sh)
    return np.array([[R._ave_window(sh, ph, pw)[4] for pw in range(PW)] for ph in range(PH)])


def test_the_lists_hold_what_torch_cannot_take():
    assert len(TORCH_SHAPES) < len(R.SHAPES + R.PLAN_SHAPES) and len(TORCH_SHAPES) >= 18


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("sh", TORCH_SHAPES, ids=R.shape_id)
def test_model_equals_torch_on_integers(sh, dtype):
    r = np.random.default_rng(SEED)
    x = R.integer_bottom(sh, dtype, r)
    xt = torch.from_numpy(x).requires_grad_(True)
    for method in (R.MAX, R.AVE):
        top, mask = R.forward(sh, method, x)
        want, idx = _torch_forward(sh, method, xt)
        assert tuple(want.shape[2:]) == R.output_dims(sh)
        assert top.dtype == dtype and top.tobytes() == want.detach().numpy().tobytes(), (sh, method)
        if method == R.MAX:
            assert mask.dtype == np.int32 and (mask == idx.numpy()).all(), sh
            td = r.integers(-8, 9, top.shape).astype(dtype)
        else:
            td = (r.integers(-8, 9, top.shape) * _pool_sizes(sh)).astype(dtype)     # every quotient is an integer
        grad, = torch.autograd.grad(want, xt, torch.from_numpy(td))
        got = R.backward(sh, method, td, mask)
        assert got.dtype == dtype and (got == grad.numpy()).all(), (sh, method)
        if method == R.MAX:                                                        # a top_mask serves as the mask does
            assert R.backward(sh, method, td, mask.astype(dtype)).tobytes() == got.tobytes()


def test_output_size_over_the_sweep_equals_torch_where_both_define_it():
    n = 0
    for H in range(1, 13):
        for k in range(1, 6):
            for s in range(1, 5):
                for p in range(0, k // 2 + 1):
                    sh = R.S((1, 1, H, H), k, s, p)
                    rc, PH, PW = R.judge(sh)
                    if rc != R.OK or H + 2 * p < k:
                        continue
                    want = F.max_pool2d(torch.zeros(sh.dims), k, s, p, ceil_mode=True).shape
                    assert (PH, PW) == tuple(want[2:]), sh
                    n += 1
    assert n == 440                     # the geometries of the sweep that neither side refuses


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_order_probes_are_order_sensitive(dtype):
    for method in (R.MAX, R.AVE):
        sh, x, td, swap = R.order_probe(method, dtype)
        _, mask = R.forward(sh, method, x)
        if method == R.MAX:
            assert (mask == 2 * 5 + 2).all()                      # the centre is the maximum of all nine windows
        got = R.backward(sh, method, td, mask)
        swapped = R.backward(sh, method, td, mask, swap=swap)
        assert got.tobytes() != swapped.tobytes(), method
        assert got[0, 0, 2, 2] == 2 and swapped[0, 0, 2, 2] == 3, method
        # and in exact arithmetic the two are the same sum
        exact = R.backward(sh, method, td.astype(np.longdouble), mask)
        exact_swapped = R.backward(sh, method, td.astype(np.longdouble), mask, swap=swap)
        assert (exact == exact_swapped).all()


def test_max_selection_rules_of_the_model():
    nan, inf = np.nan, np.inf
    sh = R.S((1, 1, 2, 2), 2, 2)
    for dtype in DTYPES:
        cases = [([3, 3, 3, 3], 3, 0), ([0.0, -0.0, 0.0, -0.0], 0.0, 0), ([-0.0, 0.0, 0.0, 0.0], -0.0, 0),
                 ([1, nan, 2, nan], 2, 2), ([nan, nan, nan, nan], -R.FLT_MAX, -1), ([-inf] * 4, -R.FLT_MAX, -1),
                 ([nan, -1, nan, -1], -1, 1)]
        if dtype is np.float64:
            cases.append(([-1e300, -2e300, -1e300, -3e300], -R.FLT_MAX, -1))
        for vals, want, at in cases:
            top, mask = R.forward(sh, R.MAX, np.array(vals, dtype).reshape(sh.dims))
            assert top.ravel()[0].tobytes() == dtype(want).tobytes() and mask.ravel()[0] == at, (vals, top, mask)
            bd = R.backward(sh, R.MAX, np.ones((1, 1, 1, 1), dtype), mask)
            assert bd.sum() == (0 if at < 0 else 1) and not np.signbit(bd).any()


def test_tanh_backward_is_three_roundings():
    r = np.random.default_rng(SEED)
    for dtype in DTYPES:
        y = np.tanh(r.standard_normal(1000)).astype(dtype)
        dy = r.standard_normal(1000).astype(dtype)
        got = R.tanh_backward(y, dy)
        assert got.dtype == dtype
        exact = dy.astype(np.longdouble) * (1 - y.astype(np.longdouble) ** 2)
        assert np.abs(got - exact).max() <= 3 * np.finfo(dtype).eps
