"""tests/bilinear_grid_model.py checked without a GPU: the probe inputs really make every output a single product, and the CPU
oracle (oracle.simcross_forward / backward, mode 2) passes the bars the kernels are held to in
tests/test_gpu_bilinear_grid_accuracy.py -- the inputs are fair before any kernel sees them."""
import numpy as np
import pytest

import bilinear_grid_model as bg
import matrix_pipe_model as mp
from test_gpu_bilinear_grid_accuracy import DENSE, SHAPES
from util import assert_bitexact, rng


def terms(*xs):
    """Number of nonzero products behind each element of the reference expression f(|x| != 0, ...)."""
    return [(np.asarray(x) != 0).astype(np.float64) for x in xs]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_probe_inputs_are_single_products_and_the_oracle_passes_the_bars(shape, oracle):
    N, W1, W2, D, M, bias_term = shape
    p = bg.probe_inputs(rng(sum(shape[:5]) + 17), *shape)
    q, a, W, dTr, dTc = p["q"], p["a"], p["W"], p["dT_rows"], p["dT_cols"]
    # the construction: one product per element (dq, da: one per measure; elements no word row reaches: none)
    some = slice(0, min(N, 70))                                    # (the position rules do not change with n)
    tq, ta, tW, tr, tc, tad = terms(q[some], a[some], W, dTr[some], dTc[some], p["a_dense"][some])
    assert (bg.ref_top(tq, ta, tW)[0] == 1).all()
    assert bg.ref_dq(ta, tW, tr)[0].max() == M and bg.ref_da(tq, tW, tc)[0].max() == M
    assert (np.matmul(tr, tad[:, None]) == 1).all(), "U = dT A is single-term for a dense a"
    assert (q != 0).sum() == N * W1 and (a != 0).sum() == N * W2 and ((p["q_cols"] != 0).sum(axis=(0, 1)) == 1).all()
    if N * W1 >= D:
        assert (q != 0).any(axis=(0, 1)).all(), "every k position is hit"
    if N * W2 >= D:
        assert (a != 0).any(axis=(0, 1)).all(), "every j position is hit"
    if bias_term:
        t64, Dm = bg.ref_top(q[some], a[some], W)
        assert (np.abs(p["bias"])[None] <= Dm / 8).all(), "the bias is at most one eighth of its product"
    for x in (q, a, W, dTr, dTc):
        assert bg.all_normal(x)
    # the oracle; its arithmetic is per pair (dW: a sum over pairs of terms that are zero but one), so of a large batch the
    # first 40 and the last 24 pairs stand for all -- the CPU restatement takes seconds on the sliced shape
    if N > 64:
        keep = np.r_[0:40, N - 24:N]
        q, a, dTr, dTc = q[keep], a[keep], dTr[keep], dTc[keep]
        # dW: the one-nonzero-per-column q rebuilt over the kept pairs, so that every dW element still has its product
        p["q_cols"] = mp.one_per_column(mp.probe_values(rng(N), (D,))[0], keep.size * W1).reshape(keep.size, W1, D)
        p["a_dense"] = p["a_dense"][keep]
    what = "oracle %s " % (shape,)
    top, _, _ = oracle.simcross_forward(2, q, a, W, p["bias"])
    bg.check(what + "top", top, bg.ref_top(q, a, W, p["bias"]), bg.bar_top(bias_term))
    dq, _, _, db = oracle.simcross_backward(2, q, a, top, dTr, W=W, bias_term=bias_term, dbias_in=p["dbias0"])
    bg.check(what + "dq", dq, bg.ref_dq(a, W, dTr), bg.bar_dq(M))
    if bias_term:
        assert_bitexact(db, bg.dbias_in_order(dTr, p["dbias0"]), what + "dbias")
    _, da, _, _ = oracle.simcross_backward(2, q, a, top, dTc, W=W, bias_term=False)
    bg.check(what + "da", da, bg.ref_da(q, W, dTc), bg.bar_da(M))
    assert (bg.ref_dW(p["q_cols"], p["a_dense"], dTr)[1] > 0).all(), "every dW element is checked"
    _, _, dW, _ = oracle.simcross_backward(2, p["q_cols"], p["a_dense"], top, dTr, W=W, bias_term=False)
    bg.check(what + "dW", dW, bg.ref_dW(p["q_cols"], p["a_dense"], dTr), bg.BAR_DW)


def test_a_dropped_or_misrouted_term_fails_the_probe_bar():
    """The bars bite: a result with one word row's product taken from the neighbouring k, or one measure left out of dq, is
    caught, and the message names the element."""
    N, W1, W2, D, M = 9, 5, 4, 20, 2
    p = bg.probe_inputs(rng(3), N, W1, W2, D, M, True)
    t64, Dm = bg.ref_top(p["q"], p["a"], p["W"], p["bias"])
    good = t64.astype(np.float32)
    bg.check("rounded fp64", good, (t64, Dm), bg.bar_top(True))
    Wr = np.roll(p["W"], 1, axis=1)                                # every product reads W one row off
    bad = good.copy()
    bad[4, 1, 2] = bg.ref_top(p["q"], p["a"], Wr, p["bias"])[0][4, 1, 2].astype(np.float32)[...]
    with pytest.raises(AssertionError, match=r"index \(4, 1, 2, "):
        bg.check("misrouted", bad, (t64, Dm), bg.bar_top(True))
    wrong = bg.ref_top(p["q"], p["a"], p["W"], p["bias"][::-1])[0].astype(np.float32)      # the bias of the other measure
    with pytest.raises(AssertionError):
        bg.check("bias of the wrong measure", wrong, (t64, Dm), bg.bar_top(True))
    d64, Dq = bg.ref_dq(p["a"], p["W"], p["dT_rows"])
    one = bg.ref_dq(p["a"], p["W"][:1], p["dT_rows"][:, :1])[0].astype(np.float32)
    with pytest.raises(AssertionError):
        bg.check("a measure dropped", one, (d64, Dq), bg.bar_dq(M))
    # an error of 4 ulp of one score is over the bar of top (3.125 roundings of half an ulp each)
    off = good.copy()
    off[0, 0, 0, 0] = np.nextafter(np.nextafter(np.nextafter(np.nextafter(off[0, 0, 0, 0], np.float32(np.inf)), np.float32(np.inf)),
                                                np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError):
        bg.check("4 ulp off", off, (t64, Dm), bg.bar_top(True))


def test_references_agree_with_einsum():
    r = rng(5)
    N, W1, W2, D, M = 3, 4, 5, 6, 2
    q, a, W, dT = (x.astype(np.float64) for x in bg.dense_inputs(r, N, W1, W2, D, M))
    np.testing.assert_allclose(bg.ref_top(q, a, W)[0], np.einsum("nik,mkl,njl->nmij", q, W, a), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(bg.ref_dq(a, W, dT)[0], np.einsum("nmij,njl,mkl->nik", dT, a, W), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(bg.ref_da(q, W, dT)[0], np.einsum("nmij,nik,mkl->njl", dT, q, W), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(bg.ref_dW(q, a, dT)[0], np.einsum("nmij,nik,njl->mkl", dT, q, a), rtol=1e-12, atol=1e-15)
    db0 = r.standard_normal((M, W1, W2)).astype(np.float32)
    want = db0.copy()
    for n in range(N):
        want = dT[n].astype(np.float32) + want
    assert_bitexact(bg.dbias_in_order(dT.astype(np.float32), db0), want)


def test_scaling_is_exact_in_fp64_and_predicts_the_outputs():
    """scale_inputs / scale_outputs are consistent: the fp64 references of the scaled inputs ARE the scaled references."""
    r = rng(6)
    N, W1, W2, D, M = DENSE[-1]
    q, a, W, dT = bg.dense_inputs(r, N, W1, W2, D, M)
    sc = bg.scaling(r, N, W1, W2, D)
    qs, as_, Ws, dTs = bg.scale_inputs(q, a, W, dT, sc)
    for x in (qs, as_, Ws, dTs):
        assert bg.all_normal(x)
    ex = lambda e: np.ldexp(1.0, e.astype(np.int32))
    s, c, rr = ex(sc["s"]), ex(sc["c"]), ex(sc["r"])
    np.testing.assert_allclose(bg.ref_top(qs, as_, Ws)[0], bg.ref_top(q, a, W)[0] * rr[:, None, :, None], rtol=1e-12)
    np.testing.assert_allclose(bg.ref_dq(as_, Ws, dTs)[0], bg.ref_dq(a, W, dT)[0] / rr[:, :, None] / s[None, None, :], rtol=1e-12)
    np.testing.assert_allclose(bg.ref_da(qs, Ws, dTs)[0], bg.ref_da(q, W, dT)[0] * c[None, None, :], rtol=1e-12)
    np.testing.assert_allclose(bg.ref_dW(qs, as_, dTs)[0], bg.ref_dW(q, a, dT)[0] * s[None, :, None] / c[None, None, :], rtol=1e-12)
    one = np.ones((2, 3), np.float32)
    assert not bg.all_normal(one * np.float32(1e-39)) and not bg.all_normal(one * np.float32(np.inf)) and bg.all_normal(one)


@pytest.mark.parametrize("geometry", [(5, 4, 68, 2), (40, 40, 50, 4), (1, 1, 24, 3), (1, 1, 300, 1)])
def test_workspace_size_of_an_empty_batch(geometry, hiplib):
    """mms_simcross_workspace_bytes(2, N = 0, ...) answers (host code only): the split-K chunk of an empty contraction was 0
    and the split count a division by it -- the process died with SIGFPE before the N = 0 no-op was reached."""
    W1, W2, D, M = geometry
    need = hiplib.mms_simcross_workspace_bytes(2, 0, W1, W2, D, M)
    assert 0 <= need <= hiplib.mms_simcross_workspace_bytes(2, 1, W1, W2, D, M)
