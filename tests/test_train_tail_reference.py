"""CPU suite: the float64 model of the TRAIN-phase tail (tests/train_tail_reference.py) against torch autograd in double
-- conv2d -> batch statistics -> pooling -> tanh -> cat -> linear -> tanh -> mask -> linear -> log-softmax loss -- every
output and every diff to 1e-12, and the shape lists cover what they claim."""
import numpy as np
import pytest
import torch

import conv_reference as CR
import head_reference as HR
import train_tail_reference as R
from util import SEED, assert_close

F64_TOL = 1e-12
SHAPES = [R.small(1), R.small(R.IMAGES + 1), R.small(65), R.v4(7), R.v5(5)] + R.SEQUENCE_TAILS


def _torch_outputs(t, pool, inp, config):
    s, F = t.stage.conv, torch.nn.functional
    leaves = ("x", "weight", "bias", "scale", "shift", "overlap", "w1", "b1", "w2", "b2")
    d = {k: (None if inp[k] is None else torch.tensor(np.array(inp[k], dtype=np.float64), requires_grad=True))
         for k in leaves}
    y = F.conv2d(d["x"], d["weight"], d["bias"], stride=CR.pair(s.stride), padding=CR.pair(s.pad), groups=s.group)
    c = (slice(None), None, None)
    mean, var = y.mean(dim=(0, 2, 3)), (y * y).mean(dim=(0, 2, 3)) - y.mean(dim=(0, 2, 3)) ** 2
    std = torch.sqrt(var + R.S.VAR_EPS)
    sc = d["scale"][c]
    if pool == R.AVE:
        sp = (F.avg_pool2d(y, t.stage.pool) - mean[c]) / std[c]
    else:
        xn = (y - mean[c]) / std[c]
        hi, lo = F.max_pool2d(xn, t.stage.pool), -F.max_pool2d(-xn, t.stage.pool)
        sp = torch.where(sc > 0, hi, lo)                      # the conditioned scales are never 0
    flt = torch.tanh(sp * sc + d["shift"][c]).flatten(1)
    feat = flt if d["overlap"] is None else torch.cat([flt, d["overlap"]], dim=1)
    h = torch.tanh(F.linear(feat, d["w1"], d["b1"]))
    drop = h * torch.from_numpy(inp["mask"].astype(np.float64)) * float(HR.scale_of(config, np.float64))
    z2 = F.linear(drop, d["w2"], d["b2"])
    prob = torch.softmax(z2, dim=1)
    lv, ok = HR.valid_of(inp["label"], t.C, config)
    terms = -torch.log_softmax(z2, dim=1)[torch.arange(s.N), torch.from_numpy(lv)]
    loss = (terms * torch.from_numpy(ok)).sum() / HR.normalizer(config, s.N, int(ok.sum()))
    (loss * inp["loss_weight"]).backward()
    keep, n = R.BN_MEMORY, lambda v: v.detach().numpy()                             # noqa: E731
    g = lambda k: np.zeros_like(inp[k], dtype=np.float64) if d[k].grad is None else d[k].grad.numpy()   # noqa: E731
    out = dict(y=n(y), flt=n(flt), save_pool=n(sp).reshape(s.N, -1), save_mean=n(mean), save_std=n(std),
               running_mean=(1 - keep) * n(mean) + keep * inp["running_mean"],
               running_var=(1 - keep) * n(var) + keep * inp["running_var"], h=n(h), prob=n(prob),
               loss=np.array([loss.item()]), bottom_diff=g("x"), weight_diff=inp["weight_diff0"] + g("weight"),
               scale_diff=g("scale"), shift_diff=g("shift"), w1_diff=inp["w1_diff0"] + g("w1"),
               b1_diff=inp["b1_diff0"] + g("b1"), w2_diff=inp["w2_diff0"] + g("w2"), b2_diff=inp["b2_diff0"] + g("b2"))
    if inp["bias"] is not None:
        out["bias_diff"] = inp["bias_diff0"] + g("bias")
    if t.F1:
        out["overlap_diff"] = g("overlap")
    return out


@pytest.mark.parametrize("pool", R.POOLS, ids=lambda p: R.POOL_NAME[p])
@pytest.mark.parametrize("t", SHAPES, ids=R.tail_id)
def test_float64_model_is_torch_autograd(t, pool):
    config = R.cfg(HR.VALID, 0)
    inp = R.conditioned_inputs(t, np.float64, SEED, config, ignored=True, out_of_range=True)
    got, want = R.model_outputs(t, pool, inp, config), _torch_outputs(t, pool, inp, config)
    assert sorted(got) == sorted(want) == sorted(set(R.FORWARD_OUTPUTS + R.BACKWARD_OUTPUTS))
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert_close(got[k], want[k], F64_TOL, k)


@pytest.mark.parametrize("norm", [HR.FULL, HR.VALID, HR.BATCH_SIZE, HR.NONE])
def test_every_normalization_is_torch_autograd(norm):
    t, config = R.small(9), R.cfg(norm, 1, ratio=0.1)
    inp = R.conditioned_inputs(t, np.float64, SEED + norm, config, ignored=True, out_of_range=True)
    got, want = R.model_outputs(t, R.AVE, inp, config), _torch_outputs(t, R.AVE, inp, config)
    for k in want:
        assert_close(got[k], want[k], F64_TOL, k)


def test_without_a_label_there_is_no_loss():
    t = R.small(3)
    out = R.forward(t, R.MAX, R.conditioned_inputs(t, np.float64, SEED), with_label=False)
    assert sorted(out) == sorted(set(R.FORWARD_OUTPUTS) - {"loss"})


def test_the_lists_cover_what_they_claim():
    for t in R.GPU_TAILS:
        if t is not R.STRIDED:
            assert CR.output_dims(t.stage.conv) == t.stage.pool and R.F0(t) == t.stage.conv.K, t
    s = R.small(1).stage.conv
    assert (s.C, s.K, s.kh, s.H, R.small(1).F1, R.small(1).H, R.small(1).C) == (3, 5, 3, 6, 3, 5, 2)
    assert [t.stage.conv.N for t in R.FUSED_TAILS[:len(R.SMALL_N)]] == R.SMALL_N
    assert {1, R.IMAGES, R.IMAGES + 1, 64, 65, 257} == set(R.SMALL_N) and R.FINISH == 64
    assert -(-257 // R.IMAGES) <= 256 or R.IMAGES == 1        # one image per workgroup: a thread folds two partials
    assert R.head_shape(R.v4(50))[1:] == (64, 4, 32, 2) and R.head_shape(R.v5(50))[1:] == (32, 2, 32, 2)
    assert R.PAST_H.H == HR.MAX_H + 1 and R.STRIDED.stage.conv.stride == 2
    assert R.S.pooled_shape(R.NOT_WHOLE_MAP.stage)[2:] == (2, 2)
    # the probe: one label counts, every other is out of range; y's sums are exact (integer_probe asserts it)
    p = R.integer_probe(R.small(R.IMAGES + 1), SEED)
    _, ok = HR.valid_of(p["label"], 2, R.cfg())
    assert ok.sum() == 1 and ok[0]
    assert all(v.dtype == np.float32 for k, v in p.items() if isinstance(v, np.ndarray) and k != "mask")
