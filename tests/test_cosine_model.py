"""tests/cosine_model.py proved on the CPU: the exact-sum probes are exact, the CPU oracle's forward on them is the closed form,
the counted backward bar holds for the fp32 oracle itself against fp64, and the dense-data bars derived from the oracle's own
error are tighter than the suite's 1e-5 on every shape.  A probe whose own reference breaks its bar is a wrong probe."""
import numpy as np
import pytest

import cosine_model as cm
from util import TOL, assert_bitexact

# the fp32 oracle's backward is a scalar loop: the shapes it is run on here stay below ~5M (j, k, d) steps
SMALL = [s for s in cm.ROUTES if s[0] * s[1] * s[2] * s[3] <= 5_000_000]


def test_small_covers_every_family():
    for fam in (cm.PAIR32, cm.VEC4, cm.SCALAR, cm.GRID_GENERIC):
        assert set(fam) <= set(SMALL)
    assert len(set(cm.GRID_TILED) & set(SMALL)) >= 5


@pytest.mark.parametrize("shape", cm.ROUTES, ids=cm.shape_id)
def test_every_partial_sum_is_an_exact_integer(shape):
    """Sum of |products| < 2^24 in the scaled integers bounds every partial sum of every order; the scaled values are normal."""
    p = cm.probe_inputs(np.random.default_rng(1701 + cm.shape_seed(shape)), *shape)
    sqq, saa, sqa, bound = cm.integer_sums(p["q"], p["a"], p["eq"], p["ea"])
    print("%s: largest sum of |products| = %d = 2^%.1f" % (shape, bound, np.log2(bound)))
    assert bound < 2 ** 24
    assert (sqq > 0).all() and (saa > 0).all(), "no zero row in a probe"
    assert cm.all_normal(p["q"]) and cm.all_normal(p["a"])
    for s, e in ((sqq, 2 * p["eq"]), (saa, 2 * p["ea"]), (sqa, p["eq"] + p["ea"])):
        assert cm.all_normal(np.ldexp(s.astype(np.float64), e))
    # one nonzero per row / per column of dT, and single-nonzero rows of q and a exist where there are enough rows
    N, W1, W2, D = shape
    assert ((p["dT_rows"] != 0).sum(axis=3) == 1).all() and ((p["dT_cols"] != 0).sum(axis=2) == 1).all()
    if N * W1 > 2 and D > 1:
        assert ((p["q"] != 0).sum(-1) == 1).any()


@pytest.mark.parametrize("shape", cm.ROUTES, ids=cm.shape_id)
def test_oracle_forward_is_the_closed_form(shape, oracle):
    """sqa / sqrt(sqq) / sqrt(saa) with fp32 roundings, from the integer sums: the oracle's k-ascending dot products add nothing."""
    p = cm.probe_case(oracle, shape)
    top, n0, n1 = cm.closed_form_forward(p["q"], p["a"], p["eq"], p["ea"])
    assert_bitexact(p["top"], top, "top %s" % (shape,))
    assert_bitexact(p["n0"], n0, "norm0 %s" % (shape,))
    assert_bitexact(p["n1"], n1, "norm1 %s" % (shape,))
    assert np.isfinite(top).all() and (np.abs(top) <= 1).all()


def test_a_lost_element_changes_the_bits():
    """What the probes are for: dropping, doubling or moving ONE element of a dense row changes norm0's bits."""
    r = np.random.default_rng(5)
    q = cm.exact_rows(r, 2, 300, 0, 5, 2)[:1].reshape(1, 1, 300)
    a = cm.exact_rows(r, 2, 300, 0, 7, 3)[:1].reshape(1, 1, 300)
    base = cm.closed_form_forward(q, a, 0, 0)
    for i in (0, 1, 151, 299):
        for change in ("drop", "double"):
            q2 = q.copy()
            q2[0, 0, i] = 0 if change == "drop" else 2 * q[0, 0, i]
            got = cm.closed_form_forward(q2, a, 0, 0)
            assert got[1].view(np.uint32) != base[1].view(np.uint32) and got[0].view(np.uint32) != base[0].view(np.uint32)


@pytest.mark.parametrize("shape", SMALL, ids=cm.shape_id)
def test_oracle_backward_within_the_counted_bar(shape, oracle):
    """The fp32 oracle (the reference form) against fp64 on the single-term probes: within BAR_GRAD, as counted; and the
    vectorised fp64 reference is the fp64 oracle's."""
    p = cm.probe_case(oracle, shape)
    f64 = lambda x: x.astype(np.float64)
    for name, dT, i in (("dq", "dT_rows", 0), ("da", "dT_cols", 1)):
        bw = oracle.simcross_backward(0, p["q"], p["a"], p["top"], p[dT], norm0=p["n0"], norm1=p["n1"])
        ref64, scale = p[name + "_ref"]
        assert cm.all_normal(ref64[ref64 != 0]) and cm.all_normal(scale[scale != 0])
        cm.check("oracle %s %s" % (name, shape), bw[i], ref64, scale, cm.BAR_GRAD)
        bw64 = oracle.simcross_backward(0, f64(p["q"]), f64(p["a"]), f64(p["top"]), f64(p[dT]), norm0=f64(p["n0"]), norm1=f64(p["n1"]))
        assert cm.scaled_error(bw64[i], ref64, scale)[0] < 2.0 ** -40


@pytest.mark.parametrize("shape", cm.DENSE, ids=cm.shape_id)
def test_dense_bars_are_tighter_than_1e5(shape, oracle):
    """bar x scale < 1e-5 max(1, max |ref|) on every element, for top, dq and da: the new check asks more than the old one."""
    c = cm.dense_case(oracle, shape)
    for name in ("top", "dq", "da"):
        ref64, scale = c["ref"][name]
        bar = cm.dense_bar(c["e_o"][name])
        old = TOL * max(1.0, float(np.abs(ref64).max()))
        new = float((bar * scale).max())
        print("%s %s: e(oracle) = %.2f x 2^-24, bar %.2f x 2^-24; largest allowed |error| %.3g against %.3g before (x %.0f tighter); "
              "smallest %.3g" % (name, shape, c["e_o"][name] / cm.U24, bar / cm.U24, new, old, old / new, float((bar * scale).min())))
        assert new < old
    mags = np.abs(c["dT"]).max(axis=(1, 2, 3))
    if shape[0] >= 6:
        assert mags.max() / mags.min() >= 2.0 ** 8, "dT spans several orders of magnitude across pairs"
