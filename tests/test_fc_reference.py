"""CPU suite: tests/fc_reference.py, the numpy model the GPU suite of include/mms_fc.h is held to, is itself pinned
against torch on the CPU -- linear, softmax, cross_entropy with ignore_index and every reduction that maps to a
normalization mode, autograd for every backward in float64 at 1e-12 -- and composing the four layer models reproduces
tests/head_reference.py on the head's own shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fc_reference as R
import head_reference as H
from util import SEED

TOL64 = 1e-12


def close(got, want, what, tol=TOL64):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    assert err <= tol * max(1.0, float(np.max(np.abs(want))) if want.size else 1.0), (what, err)


def T(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transpose"])
@pytest.mark.parametrize("M,K,N", [(1, 1, 1), (7, 3, 2), (50, 68, 64), (33, 205, 5)])
def test_inner_product_is_linear_and_its_autograd(M, K, N, transpose):
    d = R.ip_dense(M, K, N, np.float64, SEED, transpose)
    x, w, b = T(d["x"], True), T(d["w"], True), T(d["b"], True)
    top = F.linear(x, w.t() if transpose else w, b)
    close(R.ip_forward(d["x"], d["w"], d["b"], transpose), top.detach().numpy(), "top")
    close(R.ip_forward(d["x"], d["w"], None, transpose), F.linear(x, w.t() if transpose else w).detach().numpy(), "no bias")
    top.backward(T(d["td"]))
    dw, db, dx = R.ip_backward(d["x"], d["w"], d["td"], transpose, d["w_diff0"], d["b_diff0"])
    close(dw, d["w_diff0"] + w.grad.numpy(), "w_diff")
    close(db, d["b_diff0"] + b.grad.numpy(), "b_diff")
    close(dx, x.grad.numpy(), "bottom_diff")
    # the integer twin agrees with the float model on integer data
    i = R.ip_integers(M, K, N, SEED, transpose)
    top_i, dw_i, db_i, dx_i = R.ip_exact(i["x"], i["w"], i["b"], i["td"], transpose, i["w_diff0"], i["b_diff0"])
    f = {k: v.astype(np.float64) for k, v in i.items()}
    assert np.array_equal(R.ip_forward(f["x"], f["w"], f["b"], transpose), top_i.astype(np.float64))
    got = R.ip_backward(f["x"], f["w"], f["td"], transpose, f["w_diff0"], f["b_diff0"])
    for g, wnt in zip(got, (dw_i, db_i, dx_i)):
        assert np.array_equal(g, wnt.astype(np.float64))


SOFTMAX_SHAPES = [(1, 1, 1), (50, 2, 1), (3, 17, 1), (5, 130, 1), (2, 3, 7), (4, 2, 65)]


@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=str)
def test_softmax_and_its_autograd(shape):
    r = np.random.default_rng(SEED + sum(shape))
    x, td = r.standard_normal(shape) * 3, r.standard_normal(shape)
    xt = T(x, True)
    top = F.softmax(xt, dim=1)
    close(R.softmax_forward(x), top.detach().numpy(), "top")
    top.backward(T(td))
    close(R.softmax_backward(R.softmax_forward(x), td), xt.grad.numpy(), "bottom_diff")
    big = x.copy()
    big[:, 0, :] += 80.0                                            # the maximum is subtracted: no overflow in float
    assert np.isfinite(R.softmax_forward(big, np.float32)).all()


REDUCTIONS = [(R.VALID, "mean", None), (R.NONE, "sum", None), (R.FULL, "sum", "P"), (R.BATCH_SIZE, "sum", "outer")]


@pytest.mark.parametrize("ignore", [None, 1], ids=["all-labels", "ignore-1"])
@pytest.mark.parametrize("norm,reduction,divide", REDUCTIONS, ids=["VALID", "NONE", "FULL", "BATCH_SIZE"])
@pytest.mark.parametrize("shape", [(50, 2, 1), (9, 5, 7), (3, 17, 1)], ids=str)
def test_softmax_loss_is_cross_entropy_and_its_autograd(shape, norm, reduction, divide, ignore):
    O, C, I = shape
    r = np.random.default_rng(SEED + 13 * O + C + I)
    x = r.standard_normal(shape) * 2
    lab = R.labels(r, O, I, C, ignore, ignored=0.3 if ignore is not None else 0.0)
    div = {None: 1, "P": O * I, "outer": O}[divide]
    xt = T(x, True)
    target = torch.tensor(lab.astype(np.int64))
    loss = F.cross_entropy(xt, target, ignore_index=-100 if ignore is None else ignore, reduction=reduction) / div
    prob, got = R.loss_forward(x, lab, norm, ignore)
    close(prob, F.softmax(xt, dim=1).detach().numpy(), "prob")
    close(got, [loss.item()], "loss")
    close(R.loss_forward(x, lab, norm, ignore, slab_len=R.K["kLossSlabMin"])[1], [loss.item()], "loss in slabs")
    loss.backward(torch.tensor(1.7, dtype=torch.float64))
    close(R.loss_backward(prob, lab, 1.7, norm, ignore), xt.grad.numpy(), "bottom_diff")


def test_softmax_loss_edge_rules():
    r = np.random.default_rng(SEED)
    x = r.standard_normal((6, 3, 2))
    lab = np.full((6, 2), 2.0)
    prob, loss = R.loss_forward(x, lab, R.VALID, 2)                  # every label ignored: normalizer 1, loss 0, diff 0
    assert loss[0] == 0.0 and not R.loss_backward(prob, lab, 1.0, R.VALID, 2).any()
    lab = R.labels(r, 6, 2, 3)
    out = lab.copy()
    out[0, 0], out[3, 1] = 3, -1                                     # out of range is ignored
    ign = lab.copy()
    ign[0, 0], ign[3, 1] = 7, 7
    for norm in (R.FULL, R.VALID, R.BATCH_SIZE, R.NONE):
        a, b = R.loss_forward(x, out, norm, None), R.loss_forward(x, ign, norm, 7)
        assert np.array_equal(a[1], b[1])
        assert np.array_equal(R.loss_backward(a[0], out, 1.0, norm, None), R.loss_backward(b[0], ign, 1.0, norm, 7))
    # static_cast<int>: the label 1.9 is 1
    assert np.array_equal(R.loss_forward(x, lab + 0.9, R.VALID, None)[1], R.loss_forward(x, lab, R.VALID, None)[1])


@pytest.mark.parametrize("extents", [(5,), (3, 4), (100, 100, 1, 4), (1, 3, 4, 64, 1, 2, 5, 7)], ids=str)
def test_concat_is_cat_and_split(extents):
    r = np.random.default_rng(SEED + len(extents))
    bottoms = [r.standard_normal((3, e, 5)) for e in extents]
    top = R.concat_forward(bottoms)
    assert np.array_equal(top, torch.cat([T(b) for b in bottoms], dim=1).numpy())
    for got, want in zip(R.concat_backward(top, extents), bottoms):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("s", [H.V4, H.V4_2, H.S(17, 5, 3, 31, 3)], ids=H.sid)
@pytest.mark.parametrize("cfg,ignored,oor", H.CASES, ids=[str(i) for i in range(len(H.CASES))])
def test_the_four_models_compose_to_the_head(s, cfg, ignored, oor):
    inp = H.conditioned_inputs(s, np.float64, SEED, cfg, ignored, oor)
    want = H.model_outputs(s, cfg, inp)
    bottoms = [inp["x0"][:, :, None]] + ([inp["x1"][:, :, None]] if s.F1 else [])
    feat = R.concat_forward(bottoms)[:, :, 0]
    h = np.tanh(R.ip_forward(feat, inp["w1"], inp["b1"]))
    d = H.dropout(h, inp["mask"], cfg, np.float64)
    z2 = R.ip_forward(d, inp["w2"], inp["b2"])
    prob, loss = R.loss_forward(z2[:, :, None], inp["label"], cfg.norm, cfg.ignore_label)
    close(h, want["h"], "h")
    close(prob[:, :, 0], want["prob"], "prob")
    close(loss, want["loss"], "loss")
    dz2 = R.loss_backward(prob, inp["label"], inp["loss_weight"], cfg.norm, cfg.ignore_label)[:, :, 0]
    dw2, db2, dd = R.ip_backward(d, inp["w2"], dz2, False, inp["w2_diff0"], inp["b2_diff0"])
    dz1 = H.dropout(dd, inp["mask"], cfg, np.float64) * (1 - h * h)
    dw1, db1, dfeat = R.ip_backward(feat, inp["w1"], dz1, False, inp["w1_diff0"], inp["b1_diff0"])
    diffs = R.concat_backward(dfeat[:, :, None], [s.F0] + ([s.F1] if s.F1 else []))
    got = dict(w2_diff=dw2, b2_diff=db2, w1_diff=dw1, b1_diff=db1, x0_diff=diffs[0][:, :, 0])
    if s.F1:
        got["x1_diff"] = diffs[1][:, :, 0]
    for k, v in got.items():
        close(v, want[k], k)


def test_the_plan_restated():
    assert [R.slabs(M) for M in (1, 128, 129, 257, 8192, 8193, 2 ** 31 - 1)] == [1, 1, 2, 3, 64, 52, 64]
    assert R.slab_rows(8193) == 160 and R.slab_rows(8192) == 128
    assert R.ip_route(32, 32, 2, R.FORWARD) == R.ROUTE_FAST and R.ip_route(31, 32, 2, R.FORWARD) == R.ROUTE_GENERIC
    assert R.ip_route(50, 66, 32, R.FORWARD) == R.ROUTE_GENERIC and R.ip_route(50, 203, 64, R.FORWARD) == R.ROUTE_FAST
    assert R.ip_route(50, 66, 32, R.BACKWARD) == R.ROUTE_GENERIC and R.ip_route(1517, 66, 32, R.BACKWARD) == R.ROUTE_FAST
    assert R.loss_slab_len(50) == 64 and R.loss_slab_len(256 * 64 + 1) == 65
