"""CPU suite: the float64 model of the scoring tail (tests/score_tail_reference.py) is torch's conv2d, the affine,
avg_pool2d / max_pool2d, tanh, cat, linear and softmax to 1e-12 in double, at every shape of the GPU suite, and the
shape lists cover what they claim."""
import numpy as np
import pytest
import torch

import conv_reference as CR
import head_reference as HR
import score_tail_reference as R
from util import SEED, assert_close

F64_TOL = 1e-12


def _torch_outputs(t, pool, inp, config):
    s = t.stage.conv
    d = {k: (None if v is None else torch.from_numpy(np.array(v, dtype=np.float64))) for k, v in inp.items()}
    y = torch.nn.functional.conv2d(d["x"], d["weight"], d["bias"], stride=CR.pair(s.stride), padding=CR.pair(s.pad),
                                   groups=s.group)
    c = (slice(None), None, None)
    sc = d["scale"][c]
    if pool == R.AVE:
        sp = (torch.nn.functional.avg_pool2d(y, t.stage.pool) - d["mean"][c]) / torch.sqrt(d["var"][c] + 1e-9)
    else:
        ph, pw = t.stage.pool
        xn = (y - d["mean"][c]) / torch.sqrt(d["var"][c] + 1e-9)
        hi, lo = torch.nn.functional.max_pool2d(xn, t.stage.pool), -torch.nn.functional.max_pool2d(-xn, t.stage.pool)
        sp = torch.where(sc > 0, hi, torch.where(sc < 0, lo, xn[:, :, ::ph, ::pw][:, :, :hi.shape[2], :hi.shape[3]]))
    flt = torch.tanh(sp * sc + d["shift"][c]).flatten(1)
    feat = flt if d["overlap"] is None else torch.cat([flt, d["overlap"]], dim=1)
    h = torch.tanh(torch.nn.functional.linear(feat, d["w1"], d["b1"]))
    prob = torch.softmax(torch.nn.functional.linear(h, d["w2"], d["b2"]), dim=1)
    lv, ok = HR.valid_of(inp["label"], t.C, config)
    terms = -torch.log(torch.clamp(prob[torch.arange(s.N), torch.from_numpy(lv)], min=HR.FLT_MIN))
    loss = (terms * torch.from_numpy(ok)).sum() / HR.normalizer(config, s.N, int(ok.sum()))
    return dict(flt=flt.numpy(), h=h.numpy(), prob=prob.numpy(), loss=np.array([loss.item()]))


@pytest.mark.parametrize("pool", R.POOLS, ids=lambda p: R.POOL_NAME[p])
@pytest.mark.parametrize("t", R.GPU_TAILS, ids=R.tail_id)
def test_float64_model_is_torch(t, pool):
    config = R.cfg(HR.VALID, 0)
    inp = R.conditioned_inputs(t, pool, np.float64, SEED, config, ignored=True, out_of_range=True)
    got, want = R.forward(t, pool, inp, config), _torch_outputs(t, pool, inp, config)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert_close(got[k], want[k], F64_TOL, k)


@pytest.mark.parametrize("norm", [HR.FULL, HR.VALID, HR.BATCH_SIZE, HR.NONE])
def test_loss_under_every_normalization_is_torch(norm):
    t, config = R.v4(21), R.cfg(norm, 1)
    inp = R.conditioned_inputs(t, R.AVE, np.float64, SEED + norm, config, ignored=True, out_of_range=True)
    assert_close(R.forward(t, R.AVE, inp, config)["loss"], _torch_outputs(t, R.AVE, inp, config)["loss"], F64_TOL)


def test_without_a_label_there_is_no_loss():
    t = R.MINIMAL[0]
    inp = R.conditioned_inputs(t, R.MAX, np.float64, SEED)
    assert sorted(R.forward(t, R.MAX, inp, with_label=False)) == ["flt", "h", "prob"]


def test_the_lists_cover_what_they_claim():
    assert sorted((t.stage.conv.N, t.F1) for t in R.MINIMAL) == [(1, 0), (1, 2), (3, 0), (3, 2)]
    for t in R.MINIMAL:
        s = t.stage.conv
        assert (s.C, s.H, s.W, s.K, s.kh, s.kw, t.H, t.C) == (2, 3, 3, 3, 2, 2, 3, 2) and R.F0(t) == 3
    assert [R.F0(t) + t.F1 for t in R.INSIDE + R.PAST][::3] == [HR.MAX_F, HR.MAX_F + 1]
    assert [t.H for t in R.INSIDE + R.PAST][1::3] == [HR.MAX_H, HR.MAX_H + 1]
    assert [t.C for t in R.INSIDE + R.PAST][2::3] == [HR.MAX_C, HR.MAX_C + 1]
    v4, v5 = R.v4(21), R.v5(7)
    assert CR.output_dims(v4.stage.conv) == (5, 5) == v4.stage.pool and R.head_shape(v4)[1:] == HR.V4[1:]
    assert CR.output_dims(v5.stage.conv) == (6, 6) == v5.stage.pool
    # three images per workgroup: 21 fills seven, 23 and 7 leave a ragged last one; 50 makes the 17 the main call fuses at
    assert 21 % 3 == 0 and 23 % 3 == 2 and 7 % 3 == 1 and -(-50 // 3) == 17
    assert all(t.stage.conv.N == 50 for t in R.MAIN_FUSED + R.PAST)
    assert any(R.A.pooled_shape(t.stage)[2:] != (1, 1) for t in R.SEQUENCE_TAILS)
