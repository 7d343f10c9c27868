"""CPU suite: tests/fm_reference.py, the numpy restatement of the FM layer's loops that the GPU tests compare words
against, is itself pinned: its float64 forward against the closed form within the textbook bound of a recursive sum,
its float64 backward against central finite differences of its forward."""
import numpy as np
import pytest

import fm_reference as R

SHAPES = [(5, 2, 301), (7, 3, 50), (65, 80, 51), (3, 1, 2), (2, 4, 1), (1, 1, 1)]


def _x(shape, dtype=np.float64):
    return (np.random.default_rng(1701).standard_normal(shape) * 0.4).astype(dtype)


@pytest.mark.parametrize("shape", SHAPES)
def test_f64_forward_agrees_with_the_closed_form(shape):
    """|ordered chain - exact| <= n u sum|addend| for a recursive sum of n addends with unit roundoff u = 2^-53 (the
    textbook bound; n the chain length (dim-1)(C+1) + C + 1).  The addends are the chain's own: x*x and t2*t2, at half
    size because the chain is halved exactly after them, then x[k,0] and the bias.  Nothing here is measured."""
    N, C, dim = shape
    x, b = _x(shape), 0.25
    got = R.fm_forward(x, b)
    assert got.dtype == np.float64 and got.shape == (N,)
    want = R.fm_closed_form_f64(x, b)
    lat = x[:, :, 1:]
    addends = 0.5 * ((lat * lat).sum(axis=(1, 2)) + (lat.sum(axis=1) ** 2).sum(axis=1)) + np.abs(x[:, :, 0]).sum(axis=1) + abs(b)
    n = (dim - 1) * (C + 1) + C + 1
    bound = n * 2.0 ** -53 * addends
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()


def test_no_latent_columns_is_the_linear_sum():
    x = _x((2, 4, 1))
    want = ((((0.0 + x[:, 0, 0]) + x[:, 1, 0]) + x[:, 2, 0]) + x[:, 3, 0]) + 0.25
    assert (R.fm_forward(x, 0.25) == want).all()
    bd, db = R.fm_backward(x, np.array([2.0, -3.0]))
    assert (bd == np.array([2.0, -3.0])[:, None, None]).all() and db == -1.0


def test_two_channels_is_the_dot_product_of_the_pair():
    x = _x((6, 2, 9))
    want = (x[:, 0, 1:] * x[:, 1, 1:]).sum(axis=1) + x[:, 0, 0] + x[:, 1, 0]
    assert np.allclose(R.fm_forward(x), want, rtol=0, atol=1e-13)


def test_float32_stays_float32_and_differs_from_the_closed_form():
    """The ordered fp32 chain is not the correctly rounded closed form: a bit-exact test against this restatement
    tells a kernel that sums in another order from one that keeps the reference's."""
    x = _x((65, 80, 51), np.float32)
    got = R.fm_forward(x, np.float32(0.25))
    assert got.dtype == np.float32
    rounded = R.fm_closed_form_f64(x, 0.25).astype(np.float32)
    assert (got != rounded).sum() > 32
    bd, db = R.fm_backward(x, np.ones(65, np.float32))
    assert bd.dtype == np.float32 and type(db) is np.float32


@pytest.mark.parametrize("shape", [(3, 2, 7), (2, 3, 4), (2, 1, 3), (2, 4, 1)])
def test_f64_backward_agrees_with_finite_differences(shape):
    """The reference's GradientChecker rule (tests/test_oracle.py): step 1e-2, threshold 1e-2 relative, scale floor 1."""
    N = shape[0]
    rng = np.random.default_rng(1701)
    x, b = _x(shape), 0.25
    dT = rng.standard_normal(N)
    bd, db = R.fm_backward(x, dT)
    f = lambda xx, bb: float((R.fm_forward(xx, bb) * dT).sum())
    eps = 1e-2
    ng = np.zeros_like(x)
    flat, gflat = x.reshape(-1), ng.reshape(-1)
    for i in range(flat.size):
        old = flat[i]
        flat[i] = old + eps
        fp = f(x, b)
        flat[i] = old - eps
        fm = f(x, b)
        flat[i] = old
        gflat[i] = (fp - fm) / (2 * eps)
    nb = (f(x, b + eps) - f(x, b - eps)) / (2 * eps)
    for name, num, ana in (("x", ng, bd), ("bias", np.float64(nb), db)):
        scale = np.maximum(1.0, np.maximum(np.abs(num), np.abs(ana)))
        assert (np.abs(num - ana) <= 1e-2 * scale).all(), name
