"""CPU suite: tests/bn_maxpool_reference.py, the model the GPU tests of mms_bn_maxpool_tanh_* compare against, is right
(it is torch's max_pool2d over an explicitly written BN, then tanh, and their autograd, in double); the monotonicity
identity the kernels rest on holds word for word; and the parity inputs are conditioned well enough that the 1e-5 bar
of tests/test_gpu_bn_maxpool.py measures the kernels and nothing else."""
import numpy as np
import pytest
import torch

import bn_maxpool_reference as R
from util import SEED, TOL, assert_close

SHAPES = R.PARITY_SHAPES + list(R.THRESHOLD_SHAPES[np.float32])


def test_shape_lists():
    import bn_pool_reference as P
    assert R.PARITY_SHAPES[:len(P.PARITY_SHAPES)] == P.PARITY_SHAPES
    assert R.PARITY_SHAPES[len(P.PARITY_SHAPES):] == [(2, 3, 38, 38, 2, 2), (3, 2, 16, 16, 2, 2), (3, 2, 6, 6, 6, 6)]
    assert R.THRESHOLD_SHAPES is P.THRESHOLD_SHAPES and R.ZERO_SCALE_SHAPE in R.PARITY_SHAPES


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_model_is_torch_in_double(shape):
    """Forward and backward of the sequence model, TRAIN and TEST, against torch on the CPU in double: BN written out
    from the model's own save_mean / save_std as autograd leaves would not see them -- TRAIN differentiates through the
    batch statistics -- then max_pool2d, tanh, and autograd of sum(top * top_diff); atol 1e-12."""
    kernel = shape[4:]
    i = R.conditioned_inputs(shape, np.float64, SEED)
    N, C, H, W = i["x"].shape
    c = (None, slice(None), None, None)
    for phase in (R.TRAIN, R.TEST):
        top, save_pool, mean, std, _, _ = R.forward(i["x"], kernel, i["scale"], i["shift"], i["running_mean"],
                                                    i["running_var"], R.BN_MEMORY, phase)
        dx, dscale, dshift = R.backward(i["x"], kernel, top, i["top_diff"], i["scale"], i["shift"], mean, std)
        x, w, b = (torch.from_numpy(np.array(i[k])).requires_grad_(True) for k in ("x", "scale", "shift"))
        if phase == R.TRAIN:
            m = x.mean(dim=(0, 2, 3))
            v = (x * x).mean(dim=(0, 2, 3)) - m * m
        else:
            m, v = torch.from_numpy(np.array(i["running_mean"])), torch.from_numpy(np.array(i["running_var"]))
        xn = (x - m[c]) / torch.sqrt(v + R.VAR_EPS)[c]
        t = torch.tanh(torch.nn.functional.max_pool2d(xn * w[c] + b[c], kernel))
        (t * torch.from_numpy(np.array(i["top_diff"]))).sum().backward()
        want_dx = x.grad.numpy()
        if phase == R.TEST:
            # BNLayer's backward is the TRAIN formula whatever the phase (bn_layer.cpp:262-383): autograd's TEST-phase
            # dx is g / std alone, the mean and xn terms are the layer's own
            g = want_dx * std[c]
            xn_ = (i["x"] - mean[c]) / std[c]
            want_dx = (g - (xn_ * (xn_ * g).sum(axis=(0, 2, 3))[c] + g.sum(axis=(0, 2, 3))[c]) / (N * H * W)) / std[c]
        for got, want, name in ((top, t.detach().numpy(), "top"), (dx, want_dx, "bottom_diff"),
                                (dscale, w.grad.numpy(), "scale_diff"), (dshift, b.grad.numpy(), "shift_diff")):
            assert got.dtype == np.float64
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg="%s phase %d" % (name, phase))
        pooled = torch.nn.functional.max_pool2d(xn * w[c] + b[c], kernel).detach().numpy()
        nz = i["scale"] != 0
        np.testing.assert_allclose(save_pool[:, nz], ((pooled - i["shift"][c]) / np.where(nz, i["scale"], 1)[c])[:, nz],
                                   rtol=0, atol=1e-10, err_msg="save_pool")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_monotonicity_identity_holds_word_for_word(dtype):
    """max_i bn_out(x_i) == bn_out(ext_i x_i), ext = max for scale >= 0 and min for scale < 0, in the element type:
    random (mean, std, scale, shift) with negative and zero scale and a shift of 2^10 among them, windows of 16."""
    r = np.random.default_rng(SEED + 9)
    draws, wins = 200, 500
    mean, std = r.standard_normal(draws).astype(dtype), r.uniform(0.05, 3, draws).astype(dtype)
    scale, shift = (r.standard_normal(draws) * 2).astype(dtype), r.standard_normal(draws).astype(dtype)
    scale[::7] = 0
    scale[1::7] = -np.abs(scale[1::7])
    shift[::5] = 1024
    assert (scale < 0).any() and (scale > 0).any() and ((scale == 0) & (shift == 1024)).any()
    x = (r.standard_normal((1, draws, wins * 4, 4)) * 2).astype(dtype)          # per draw `wins` windows of 4 x 4
    # neighbours in the type, so that rounding collapses some of them
    x[:, :, 1::2, :] = np.nextafter(x[:, :, ::2, :], dtype(np.inf))
    _, y = R.bn_out(x, mean, std, scale, shift)
    assert y.dtype == dtype
    want = R.windows(y, 4, 4).max(axis=-1)
    _, got = R.bn_out(R.extremum(x, (4, 4), scale), mean, std, scale, shift)
    w = np.uint32 if dtype == np.float32 else np.uint64
    assert got.shape == want.shape == (1, draws, wins, 1)
    assert (np.ascontiguousarray(got).view(w) == np.ascontiguousarray(want).view(w)).all()
    assert (R.first_max(y, 4, 4)[0].view(w) == want.view(w)).all()


def test_zero_variance_is_exact():
    for dtype in (np.float32, np.float64):
        i = R.conditioned_inputs((1, 1, 1, 1, 1, 1), dtype, SEED)
        for fwd in (R.forward, R.fused_forward):
            top, save_pool, mean, std, _, _ = fwd(i["x"], (1, 1), i["scale"], i["shift"], i["running_mean"],
                                                  i["running_var"])
            assert save_pool.reshape(()) == 0 and top.reshape(()) == np.tanh(i["shift"][0])
            assert std[0] == np.sqrt(dtype(1e-9)) and mean[0] == i["x"].reshape(())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity_inputs_are_well_conditioned(shape):
    """On the inputs the GPU tests use in float32, the fused algebra in float32 with plainly sequential sums stays within
    TOL / 2 of the float64 model (the three layers in sequence) on every output, in assert_close's metric: the device
    has the other half of the bar."""
    kernel = shape[4:]
    i = R.conditioned_inputs(shape, np.float32, SEED)
    assert i["top_diff"].shape == R.pooled_shape(shape)
    got, want = R.fused_outputs(i, kernel), R.model_outputs(i, kernel, np.float64)
    assert sorted(got) == sorted(want) and len(want) == 2 * len(R.OUTPUTS)
    for k in sorted(want):
        assert got[k].dtype == np.float32 and want[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        print("%-22s %.3e" % (k, float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) / scale))
    for k in sorted(want):
        assert_close(got[k], want[k], TOL / 2, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_window_has_a_top_two_gap(shape, dtype):
    """The condition the parity tests rest on: in the float64 sequence model, TRAIN and TEST, the largest and second
    largest BN output of EVERY window of a non-zero-scale channel differ by at least 1e-4 max(1, |y|) -- about 10^3
    float32 ulps, so the float32 run's mask cannot differ from the model's by rounding collapse (the order of x fixes
    the order of y whatever the statistics' error).  Every shape with C >= 2 has a negative-scale channel, one shape
    a zero-scale channel too."""
    i = R.conditioned_inputs(shape, dtype, SEED)
    kernel = shape[4:]
    assert i["x"].dtype == dtype and i["x"].shape == shape[:4]
    if shape[1] >= 2:
        assert (i["scale"] < 0).any() and (i["scale"] > 0).any()
    assert (i["scale"] == 0).any() == (shape == R.ZERO_SCALE_SHAPE)
    nz = i["scale"] != 0
    for y in R.bn_outputs64(i):
        gap = R.top_two_gap(y, *kernel)
        assert gap.shape == R.pooled_shape(shape)
        assert (gap[:, nz] >= R.GAP).all(), float(gap[:, nz].min())
    assert not R.close_windows(i, kernel).any()
