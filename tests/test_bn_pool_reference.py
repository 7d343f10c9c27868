"""CPU suite: tests/bn_pool_reference.py, the model the GPU tests of mms_bn_pool_tanh_* compare against, is right (it is
torch's batch_norm -> avg_pool2d -> tanh and their autograd, in double), and the parity inputs are conditioned well
enough that the 1e-5 bar of tests/test_gpu_bn_pool.py measures the kernels and nothing else."""
import numpy as np
import pytest
import torch

import bn_pool_reference as R
from util import SEED, TOL, assert_close

SHAPES = R.PARITY_SHAPES + list(R.THRESHOLD_SHAPES[np.float32])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[2] * s[3] > 1], ids=str)
def test_model_is_torch_in_double(shape):
    """TRAIN phase against torch on the CPU in double: batch_norm(training, eps 1e-9) -> avg_pool2d -> tanh, and
    autograd of sum(top * top_diff) for bottom_diff, scale_diff, shift_diff; 1e-10.  (torch refuses a training batch of
    one value per channel, so (1, 1, 1, 1, 1, 1) is left to test_zero_variance_is_exact.)"""
    kernel = shape[4:]
    i = R.conditioned_inputs(shape, np.float64, SEED)
    top, save_pool, mean, std, _, _ = R.forward(i["x"], kernel, i["scale"], i["shift"], i["running_mean"],
                                                i["running_var"], R.BN_MEMORY, R.TRAIN)
    dx, dscale, dshift = R.backward(i["x"], kernel, top, i["top_diff"], i["scale"], mean, std)
    x, w, b = (torch.from_numpy(np.array(i[k])).requires_grad_(True) for k in ("x", "scale", "shift"))
    y = torch.nn.functional.batch_norm(x, None, None, w, b, True, 0.1, 1e-9)
    t = torch.tanh(torch.nn.functional.avg_pool2d(y, kernel))
    (t * torch.from_numpy(np.array(i["top_diff"]))).sum().backward()
    xd = i["x"]
    for got, want, name in ((top, t.detach().numpy(), "top"), (dx, x.grad.numpy(), "bottom_diff"),
                            (dscale, w.grad.numpy(), "scale_diff"), (dshift, b.grad.numpy(), "shift_diff"),
                            (mean, xd.mean(axis=(0, 2, 3)), "save_mean"),
                            (std, np.sqrt(xd.var(axis=(0, 2, 3)) + 1e-9), "save_std")):
        assert got.dtype == np.float64
        assert_close(got, want, 1e-10, name)
    # save_pool: the pooling of the normalised map, i.e. the pooled BN output with scale and shift taken off
    pooled = torch.nn.functional.avg_pool2d(y, kernel).detach().numpy()
    c = (None, slice(None), None, None)
    assert_close(save_pool, (pooled - i["shift"][c]) / i["scale"][c], 1e-10, "save_pool")


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
    TOL / 2 of the float64 model (the three layers in sequence) on every output, in assert_close's metric: the device,
    whose sums are trees over at most a few windows per thread, has the other half of the bar."""
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
