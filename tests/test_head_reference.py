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


@pytest.mark.parametrize("s", [s for s in R.GPU_SHAPES if s not in R.LARGE_SHAPES], ids=R.sid)
def test_conditioned_inputs_are_fit_for_the_float_bar(s):
    """The model in float32 with the sample sums reversed stays within a third of 1e-5 of the float64 model: the bar
    test_gpu_head.py sets measures a kernel, not the inputs.  (One chain of float32 additions over all samples: past
    16384 samples that chain's own error, some N / 2 roundings of the running sum, is the bar's size, and no kernel
    adds that way -- test_slab_ordered_float_sums_stay_within_the_bar takes R.LARGE_SHAPES in the kernels' order.)"""
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
        cfg, inp, h, prob, want, bound = R.shared_probe(s, SEED, k)
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
        (True, False, False), (False, True, False), (False, False, True), (False, True, False)]
    assert R.GENERIC_SHAPES[3:] == R.LARGE_SHAPES[4:] and R.FAST_SHAPES[-4:] == R.LARGE_SHAPES[:4]
    assert {R.slabs(s.N)[::-1] for s in R.FAST_SHAPES} == R.FAST_PLANS
    assert {c[0].norm for c in R.CASES} == {R.FULL, R.VALID, R.BATCH_SIZE, R.NONE}
    assert {c[0].phase for c in R.CASES} == {R.TRAIN, R.TEST} and {c[0].ratio for c in R.CASES} == {0.5, 0.1}


# ---- batches of more than kHeadMaxSlabs tiles ------------------------------------------------------------------------
def test_large_shapes_take_the_plans_they_are_listed_for():
    """Each of R.LARGE_SHAPES has the (tiles, tiles per slab, slabs) its line states, and the list has what it is for:
    the fewest samples with two tiles per slab, a last slab clipped to fewer tiles, a last tile of one sample, 320
    samples per slab (more than head_out_kernel's 256 threads), every fast limit at once, a shape generic by route."""
    assert len(R.LARGE_SHAPES) == 5 and all(s in R.GPU_SHAPES for s in R.LARGE_SHAPES)
    for s, (tiles, tps, n_slabs) in R.LARGE_PLANS.items():
        assert tiles == -(-s.N // R.TILE) and R.slabs(s.N) == (n_slabs, tps), s
        assert tiles > R.K["kHeadMaxSlabs"] and tps >= 2 and n_slabs > 1, s
    assert R.slabs(R.LARGE_SHAPES[0].N - 1) == (R.K["kHeadMaxSlabs"], 1)
    assert R.INDEPENDENCE_SHAPE == R.S(16385, 3, 2, 5, 3)
    clipped = [s for s, (tiles, tps, n_slabs) in R.LARGE_PLANS.items() if tps >= 3 and tiles - (n_slabs - 1) * tps < tps]
    assert clipped and any(s.F1 == 0 for s in clipped)
    assert sum(s.N % R.TILE == 1 for s in R.LARGE_SHAPES) >= 4
    assert any(tps * R.TILE > 256 and s.N > 65536 for s, (_, tps, _) in R.LARGE_PLANS.items())
    assert R.S(16449, R.MAX_F - 2, 2, R.MAX_H, R.MAX_C) in R.FAST_SHAPES
    assert any(s.H == R.MAX_H + 1 for s in R.LARGE_SHAPES[4:])


def test_the_cut_at_every_batch_size():
    """head_slabs as tests/head_reference.py restates it, at N = 1 .. 70000 and around INT_MAX / 64: never more than
    kHeadMaxSlabs slabs, the slabs hold every tile, none is empty, and there is one slab exactly up to kHeadSingleSamples."""
    int_max = 2 ** 31 - 1
    near = [int_max // R.TILE + d for d in (-2, -1, 0, 1, 2)] + [int_max - R.TILE, int_max - 1, int_max]
    for N in list(range(1, 70001)) + near:
        n_slabs, tps = R.slabs(N)
        tiles = -(-N // R.TILE)
        assert 1 <= n_slabs <= R.K["kHeadMaxSlabs"], N
        assert n_slabs * tps >= tiles, N
        assert (n_slabs - 1) * tps < tiles, N
        assert (n_slabs == 1) == (N <= R.SINGLE), N
        assert (n_slabs - 1) * tps * R.TILE < N <= int_max, N          # the last slab's first sample is an int, below N


@pytest.mark.parametrize("s", R.LARGE_SHAPES, ids=R.sid)
def test_slab_ordered_float_sums_stay_within_the_bar(s):
    """The model in float32 with the sums over samples taken in the kernels' order -- loss, b1_diff and b2_diff one term
    at a time, ascending within a slab, then the slabs ascending; w1_diff and w2_diff one matrix product per slab, then
    the slabs ascending -- is within TOL of the float64 model in every output and every case of R.CASES: the float bar
    can hold at these batch sizes.  Measured, as shares of the bar, the worst of the five cases: at 65537 samples loss
    0.038 and b2_diff 0.009; over all five shapes loss 0.038, b2_diff 0.031, any output 0.039."""
    worst = {}
    for cfg, ignored, oor in R.CASES:
        inp = R.conditioned_inputs(s, np.float32, SEED, cfg, ignored, oor)
        fwd = R.forward(s, cfg, inp)
        h, prob = fwd["h"].astype(np.float32), fwd["prob"].astype(np.float32)
        want = dict(R.backward(s, cfg, inp, h, prob), loss=fwd["loss"])
        got = dict(R.backward(s, cfg, inp, h, prob, np.float32, R.SLAB_ORDER),
                   loss=R.forward(s, cfg, inp, np.float32, R.SLAB_ORDER)["loss"])
        assert sorted(got) == sorted(want)
        for key in sorted(want):
            assert got[key].dtype == np.float32
            err = float(np.max(np.abs(got[key].astype(np.float64) - want[key])))
            worst[key] = max(worst.get(key, 0.0), err / (TOL * max(1.0, float(np.max(np.abs(want[key]))))))
            assert_close(got[key], want[key], TOL, "%s %s" % (R.sid(s), key))
    print(R.sid(s), " ".join("%s %.3f" % kv for kv in sorted(worst.items())), "of the bar")


def test_slab_sum_is_the_order_it_names():
    """R.slab_sum against the plain loops, at a batch with a clipped, ragged last slab."""
    N = 3 * 256 * R.TILE + 70
    n_slabs, tps = R.slabs(N)
    assert (n_slabs, tps) == (193, 4) and N - (n_slabs - 1) * tps * R.TILE < tps * R.TILE
    v = np.random.default_rng(SEED).uniform(-1, 1, (N, 2)).astype(np.float32)
    total = None
    for k in range(n_slabs):
        part = np.zeros(2, dtype=np.float32)
        for n in range(k * tps * R.TILE, min(N, (k + 1) * tps * R.TILE)):
            part = part + v[n]
        total = part if total is None else total + part
    got = R.slab_sum(v, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, total)
    assert not np.array_equal(got, np.add.reduce(v[::-1], axis=0, dtype=np.float32))


@pytest.mark.parametrize("s", R.LARGE_SHAPES, ids=R.sid)
def test_large_probes_fit_float32(s):
    """The dyadic probes need no narrower values at these batch sizes: the largest sum of absolute terms of any output,
    in the probe's unit of 1 / (64 normalizer), is below 2^24 (measured: at most 0.141 of it, at 65537 samples), so
    every partial sum in any order is a float.  And the probes are not degenerate: every class is a label, labels are
    ignored and out of range, in the first and in the last tile of the slabs too."""
    for k in range(2):
        cfg, inp, h, prob, want, bound = R.shared_probe(s, SEED, k)
        print(R.sid(s), "probe %d: %.4f of 2^24" % (k, bound / 2.0 ** 24))
        assert bound < 2 ** 24, bound
        assert cfg.norm == R.NONE and cfg.ignore_label == 1
        lab = inp["label"]
        assert set(range(s.C)) <= set(np.unique(lab)) and (lab == -1).any() and (lab == s.C).any()
        for key in ("w1_diff", "b1_diff", "w2_diff", "b2_diff"):
            assert np.count_nonzero(want[key]) >= want[key].size // 2, key
        _, ok = R.valid_of(lab, s.C, cfg)
        n_slabs, tps = R.slabs(s.N)
        per = tps * R.TILE
        full = ok[:(n_slabs - 1) * per].reshape(n_slabs - 1, tps, R.TILE)
        assert full.any(axis=2).all() and ok[(n_slabs - 1) * per:].size >= 1       # no tile without a live sample
