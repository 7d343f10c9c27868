"""CPU suite: tests/bn_reference.py, the model the GPU BN tests compare against, is right (its backward is the gradient
of its forward; the running blobs move as the reference moves them), and the parity inputs are conditioned well enough
that the 1e-5 bar of tests/test_gpu_bn.py measures the kernels' summation order and nothing else."""
import numpy as np
import pytest

import bn_reference as R
from util import SEED, TOL, assert_close


def _objective(x, scale, shift, rm, rv):
    top = R.bn_forward(x, scale, shift, rm, rv, R.BN_MEMORY, R.TRAIN)[0]
    return 0.5 * float(np.sum(top * top))


def test_backward_is_the_gradient_of_the_forward():
    """The reference's own GradientChecker objective, 1/2 sum top^2 (so top_diff = top), by central differences in
    float64 at (3, 2, 5): x, scale and shift, 1e-6 relative."""
    i = R.conditioned_inputs((3, 2, 5), np.float64, SEED)
    x, scale, shift, rm, rv = (i[k].copy() for k in ("x", "scale", "shift", "running_mean", "running_var"))
    top, mean, std, _, _ = R.bn_forward(x, scale, shift, rm, rv, R.BN_MEMORY, R.TRAIN)
    dx, dscale, dshift = R.bn_backward(x, top, scale, mean, std)
    h = 1e-5
    for arr, grad, name in ((x, dx, "x"), (scale, dscale, "scale"), (shift, dshift, "shift")):
        num = np.empty_like(arr)
        for idx in np.ndindex(arr.shape):
            keep = arr[idx]
            arr[idx] = keep + h
            up = _objective(x, scale, shift, rm, rv)
            arr[idx] = keep - h
            down = _objective(x, scale, shift, rm, rv)
            arr[idx] = keep
            num[idx] = (up - down) / (2 * h)
        err = np.max(np.abs(num - grad))
        print("d/d%s: max |numeric - analytic| = %.3e, max |analytic| = %.3e" % (name, err, np.max(np.abs(grad))))
        assert err <= 1e-6 * max(1.0, np.max(np.abs(grad))), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_running_blobs(dtype):
    """TEST phase leaves them alone and normalises with them; TRAIN phase moves them by exactly
    (1 - bn_memory) * batch + bn_memory * running, two rounded products and one add, 1 - bn_memory taken in the dtype."""
    i = R.conditioned_inputs((7, 3, 11), dtype, SEED)
    args = (i["x"], i["scale"], i["shift"], i["running_mean"], i["running_var"])
    top, mean, std, rm, rv = R.bn_forward(*args, 0.9, R.TEST)
    assert (rm == i["running_mean"]).all() and (rv == i["running_var"]).all()
    assert (mean == i["running_mean"]).all()
    assert (std == np.sqrt(i["running_var"] + dtype(1e-9))).all()
    _, mean, std, rm, rv = R.bn_forward(*args, 0.9, R.TRAIN)
    bmean, var = R.batch_statistics(i["x"])
    assert (bmean == mean).all() and (std == np.sqrt(var + dtype(1e-9))).all()
    keep, take = dtype(0.9), dtype(1) - dtype(0.9)
    assert rm.dtype == dtype and rv.dtype == dtype
    assert (rm == take * mean + keep * i["running_mean"]).all()
    assert (rv == take * var + keep * i["running_var"]).all()
    # the batch statistics are the plain ones
    x = i["x"].astype(np.float64)
    assert_close(mean, x.mean(axis=(0, 2)), 8 * float(np.finfo(dtype).eps), "mean")
    assert_close(var, x.var(axis=(0, 2)), 64 * float(np.finfo(dtype).eps), "var against numpy")


def test_zero_variance_is_exact():
    """(1, 1, 1): x*x - x*x is 0 without contraction, so xn = 0, top = shift and dx = 0, exactly."""
    for dtype in (np.float32, np.float64):
        i = R.conditioned_inputs((1, 1, 1), dtype, SEED)
        top, mean, std, _, _ = R.bn_forward(i["x"], i["scale"], i["shift"], i["running_mean"], i["running_var"])
        dx, dscale, dshift = R.bn_backward(i["x"], i["dy"], i["scale"], mean, std)
        assert top[0, 0, 0] == i["shift"][0] and dx[0, 0, 0] == 0 and dscale[0] == 0 and dshift[0] == i["dy"][0, 0, 0]
        assert std[0] == np.sqrt(dtype(1e-9))


@pytest.mark.parametrize("shape", R.PARITY_SHAPES + list(R.THRESHOLD_SHAPES[np.float32]), ids=str)
def test_parity_inputs_are_well_conditioned(shape):
    """On the inputs the GPU tests use in float32 (the seven shapes and float32's two threshold shapes; float64's two
    run in float64 only, at 1e-12), the float32 model (ascending sums) is within TOL / 4 of the float64 model on every
    output, in assert_close's metric: a kernel with any sane summation order has the other 3/4 of the bar."""
    i = R.conditioned_inputs(shape, np.float32, SEED)
    sd = i["x"].astype(np.float64).std(axis=(0, 2))
    if shape[0] * shape[2] >= 1000:
        assert (sd > 0.4).all() and (sd < 1.6).all()
    got, want = R.model_outputs(i), R.model_outputs(i, np.float64)
    for k in sorted(want):
        assert got[k].dtype == np.float32 and want[k].dtype == np.float64
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        print("%-22s %.3e" % (k, float(np.max(np.abs(got[k].astype(np.float64) - want[k]))) / scale))
        assert_close(got[k], want[k], TOL / 4, k)
