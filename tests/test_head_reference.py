"""CPU suite: tests/head_reference.py is pinned by torch's autograd in float64 on the CPU, and its inputs are shown fit
for the bars tests/test_gpu_head.py holds the kernels to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reference as R
from util import SEED, TOL, assert_close


def torch_outputs(s, cfg, inp):
    """cat -> linear -> tanh -> mask * scale -> linear -> log_softmax / nll with the head's normalisation, float64."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    leaves = {k: t(inp[k]).requires_grad_() for k in ("x0", "x1", "w1", "b1", "w2", "b2") if inp[k] is not None}
    feat = torch.cat([leaves["x0"], leaves["x1"]], dim=1) if "x1" in leaves else leaves["x0"]
    h = torch.tanh(F.linear(feat, leaves["w1"], leaves["b1"]))
    d = h * t(inp["mask"]) * (1.0 / (1.0 - float(np.float32(cfg.ratio)))) if cfg.phase == R.TRAIN else h
    logp = F.log_softmax(F.linear(d, leaves["w2"], leaves["b2"]), dim=1)
    lv = np.trunc(inp["label"]).astype(np.int64)
    ok = (lv >= 0) & (lv < s.C)
    if cfg.ignore_label is not None:
        ok &= lv != cfg.ignore_label
    keep = torch.tensor(np.flatnonzero(ok))
    total = F.nll_loss(logp[keep], torch.tensor(lv[ok]), reduction="sum") if ok.any() else logp.sum() * 0
    count = {R.FULL: s.N, R.VALID: int(ok.sum()), R.BATCH_SIZE: s.N, R.NONE: 1}[cfg.norm]
    loss = total / max(1, count)
    (loss * inp["loss_weight"]).backward()
    g = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in leaves.items()}
    out = dict(h=h.detach().numpy(), prob=logp.exp().detach().numpy(), loss=np.array([loss.item()]), x0_diff=g["x0"],
               w1_diff=inp["w1_diff0"] + g["w1"], b1_diff=inp["b1_diff0"] + g["b1"], w2_diff=inp["w2_diff0"] + g["w2"],
               b2_diff=inp["b2_diff0"] + g["b2"])
    if "x1" in g:
        out["x1_diff"] = g["x1"]
    return out


MODEL_SHAPES = [R.V4, R.S(17, 5, 3, 31, 3), R.S(9, 4, 0, 6, 1), R.S(65, 63, 2, 33, 5)]


@pytest.mark.parametrize("norm", [R.FULL, R.VALID, R.BATCH_SIZE, R.NONE])
@pytest.mark.parametrize("phase", [R.TRAIN, R.TEST])
@pytest.mark.parametrize("ignored", [False, True])
def test_model_against_autograd(phase, norm, ignored):
    for k, s in enumerate(MODEL_SHAPES):
        cfg = R.Cfg(phase, (0.5, 0.1)[k % 2], norm, (s.C - 1) if ignored else None)
        inp = R.conditioned_inputs(s, np.float64, SEED, cfg, ignored, ignored)
        inp["loss_weight"] = 0.75
        got, want = R.model_outputs(s, cfg, inp), torch_outputs(s, cfg, inp)
        assert sorted(got) == sorted(want)
        for key in sorted(want):
            assert_close(got[key], want[key], 1e-12, "%s %s" % (R.sid(s), key))


def test_ignored_rows_and_the_clamp():
    """Every label ignored: loss 0 over a normalizer of max(1, 0), zero gradients.  A probability below FLT_MIN on the
    label costs -log(FLT_MIN)."""
    s = R.S(6, 3, 1, 4, 2)
    cfg = R.Cfg(R.TEST, 0.5, R.VALID, 1)
    inp = R.conditioned_inputs(s, np.float64, SEED, cfg)
    inp["label"] = np.array([1, 1, 2, -1, 1, 7], dtype=np.float64)
    out = R.model_outputs(s, cfg, inp)
    assert out["loss"][0] == 0.0 and not out["x0_diff"].any() and not out["x1_diff"].any()
    assert np.array_equal(out["w1_diff"], inp["w1_diff0"]) and np.array_equal(out["b2_diff"], inp["b2_diff0"])
    s, inp = clamp_case(np.float64)
    out = R.forward(s, R.Cfg(R.TEST, 0.5, R.NONE, None), inp)
    assert out["loss"][0] == pytest.approx(-s.N * np.log(R.FLT_MIN), rel=1e-15)


def clamp_case(dtype):
    """z2 gaps of 120 and more (past 104, where exp(-gap) is still a float denormal), the label on the losing class."""
    s = R.S(5, 2, 0, 2, 2)
    inp = dict(x0=np.full((s.N, s.F0), 4.0), x1=None, w1=np.array([[5.0, 5.0], [-5.0, -5.0]]), b1=None,
               w2=np.array([[60.0, -60.0], [-60.0, 60.0]]), b2=None,
               mask=None, label=np.ones(s.N), loss_weight=1.0)
    inp = {k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    return s, inp


@pytest.mark.parametrize("s", R.GPU_SHAPES, ids=R.sid)
def test_conditioned_inputs_are_fit_for_the_float_bar(s):
    """The model in float32 with the sample sums reversed stays within a third of 1e-5 of the float64 model: the bar
    test_gpu_head.py sets measures a kernel, not the inputs."""
    for cfg, ignored, oor in R.CASES:
        inp = R.conditioned_inputs(s, np.float32, SEED, cfg, ignored, oor)
        want = R.model_outputs(s, cfg, inp)
        got = R.model_outputs(s, cfg, inp, np.float32, reverse=True)
        fwd = R.forward(s, cfg, inp)
        got.update(R.backward(s, cfg, inp, fwd["h"].astype(np.float32), fwd["prob"].astype(np.float32), np.float32, True))
        want.update(R.backward(s, cfg, inp, fwd["h"].astype(np.float32), fwd["prob"].astype(np.float32)))
        for key in sorted(want):
            assert got[key].dtype == np.float32
            assert_close(got[key], want[key], TOL / 3, "%s %s" % (R.sid(s), key))


@pytest.mark.parametrize("s", R.GPU_SHAPES, ids=R.sid)
def test_dyadic_probes_are_exact_in_any_order(s):
    for k in range(2):
        cfg, inp, h, prob, want, bound = R.dyadic_probe(s, SEED, k)
        assert bound < 2 ** 24, bound
        assert cfg.phase == R.TRAIN and R.scale_of(cfg, np.float32) == 2.0
        assert set(np.unique(h * 4)) <= set(range(-4, 5)) and set(np.unique(prob)) <= {0.0, 0.25, 0.75, 1.0}
        assert (prob.sum(axis=1) == 1.0).all()
        got64 = R.backward(s, cfg, inp, h, prob)                       # the float64 model agrees with the int64 one
        got32 = R.backward(s, cfg, inp, h, prob, np.float32, reverse=True)
        assert sorted(got64) == sorted(want)
        for key, v in want.items():
            assert np.array_equal(got64[key], v), key
            assert np.array_equal(got32[key].astype(np.float64), v), key
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v), key


def test_the_lists_cover_what_they_claim():
    names = [s for s in R.GPU_SHAPES]
    assert R.V4 in names and R.V4_TEST in names and R.V4_2 in names
    for n in (R.TILE - 1, R.TILE, R.TILE + 1, R.SINGLE - 1, R.SINGLE, R.SINGLE + 1):
        assert any(s.N == n for s in R.FAST_SHAPES), n
    assert any(R.slabs(s.N)[0] >= 3 and s.N % R.TILE for s in R.FAST_SHAPES)
    assert R.slabs(R.SINGLE) == (1, R.SINGLE // R.TILE) and R.slabs(R.SINGLE + 1)[0] == R.SINGLE // R.TILE + 1
    assert R.slabs(65536) == (R.K["kHeadMaxSlabs"], 4)
    for s in R.FAST_SHAPES:
        assert s.F0 + s.F1 <= R.MAX_F and s.H <= R.MAX_H and s.C <= R.MAX_C
    assert [(s.F0 + s.F1 > R.MAX_F, s.H > R.MAX_H, s.C > R.MAX_C) for s in R.GENERIC_SHAPES] == [
        (True, False, False), (False, True, False), (False, False, True)]
    assert {c[0].norm for c in R.CASES} == {R.FULL, R.VALID, R.BATCH_SIZE, R.NONE}
    assert {c[0].phase for c in R.CASES} == {R.TRAIN, R.TEST} and {c[0].ratio for c in R.CASES} == {0.5, 0.1}
