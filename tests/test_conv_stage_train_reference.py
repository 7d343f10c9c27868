"""CPU suite: the float64 model of tests/conv_stage_train_reference.py is what it claims to be -- conv2d, the fork's BN
written out, avg_pool2d / max_pool2d and tanh in torch, with autograd, in double -- and the inputs of the GPU suite meet
the conditions their bar rests on.  The binding is imported: this suite belongs to the TRAIN stage."""
import numpy as np
import pytest
import torch

import conv_reference as CR
import conv_stage_train_reference as R
from util import SEED, assert_close

BAR = 1e-10                      # tests/test_bn_pool_reference.py's bar against torch in double
IDS = [R.stage_id(st) for st in R.PARITY_STAGES]


def test_the_binding_is_there():
    from mms_answer_selection_amd import conv_stage_train
    assert conv_stage_train.POOL_AVE == 0 and conv_stage_train.POOL_MAX == 1


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("st", R.PARITY_STAGES, ids=IDS)
def test_model_is_torch_in_double(st, method):
    from mms_answer_selection_amd import conv_stage_train                      # noqa: F401
    s, inp = st.conv, R.conditioned_inputs(st, np.float64, SEED)
    want = R.model_outputs(st, method, inp, np.float64)
    t = {k: torch.from_numpy(np.array(inp[k])).requires_grad_(k in ("x", "weight", "bias", "scale", "shift"))
         for k in inp if inp[k] is not None}
    y = torch.nn.functional.conv2d(t["x"], t["weight"], t.get("bias"), stride=CR.pair(s.stride), padding=CR.pair(s.pad),
                                   groups=s.group)
    mean = y.mean(dim=(0, 2, 3))
    var = (y * y).mean(dim=(0, 2, 3)) - mean * mean
    std = torch.sqrt(var + 1e-9)
    bn = (y - mean[None, :, None, None]) / std[None, :, None, None] * t["scale"][None, :, None, None] \
        + t["shift"][None, :, None, None]
    pool = torch.nn.functional.avg_pool2d if method == R.AVE else torch.nn.functional.max_pool2d
    top = torch.tanh(pool(bn, st.pool))
    (top * t["top_diff"]).sum().backward()
    got = dict(y=y, top=top, save_mean=mean, save_std=std,
               running_mean=(1 - R.BN_MEMORY) * mean + R.BN_MEMORY * t["running_mean"],
               running_var=(1 - R.BN_MEMORY) * var + R.BN_MEMORY * t["running_var"],
               bottom_diff=t["x"].grad, weight_diff=t["weight"].grad + t["weight_diff0"],
               scale_diff=t["scale"].grad, shift_diff=t["shift"].grad)
    if s.bias:
        got["bias_diff"] = t["bias"].grad + t["bias_diff0"]
    # save_pool is the pooled normalised map: (the pooled BN output - shift) / scale
    got["save_pool"] = (pool(bn, st.pool) - t["shift"][None, :, None, None]) / t["scale"][None, :, None, None]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert_close(want[k], got[k].detach().numpy(), BAR, "%s, %s" % (k, method))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("st", R.PARITY_STAGES, ids=IDS)
def test_parity_inputs_are_conditioned(st, dtype):
    from mms_answer_selection_amd import conv_stage_train                      # noqa: F401
    inp = R.conditioned_inputs(st, dtype, SEED)
    var, scale, gap = R.conditions(st, inp)
    print("least variance %.3g, least |scale| %.3g, least top-two gap %.3g" % (var, scale, gap))
    assert var >= R.MIN_VAR > 1e6 * R.VAR_EPS and scale >= R.MIN_SCALE and gap >= R.GAP > 1e-5
    assert inp["scale"][0] > 0 > inp["scale"][1]
    for method in R.METHODS:                   # the two sums whose difference is bias_diff's batch term stay small
        out = R.model_outputs(st, method, inp, np.float64)
        assert np.abs(out["shift_diff"] * inp["scale"]).max() <= R.MAX_CANCELLING


@pytest.mark.parametrize("st", R.FUSED_STAGES, ids=[R.stage_id(st) for st in R.FUSED_STAGES])
def test_probe_sums_are_exact_in_float(st):
    from mms_answer_selection_amd import conv_stage_train                      # noqa: F401
    inp = R.integer_probe(st, SEED)
    y, s0, s1 = R.probe_sums(st, inp)                                          # asserts the 2^24 bounds
    assert (y.astype(np.float32).astype(np.int64) == y).all()
    assert inp["scale"][R.ZERO_CHANNEL] == 0 and inp["scale"][R.NEGATIVE_CHANNEL] < 0 < inp["scale"][R.POSITIVE_CHANNEL]
    mean, std, _, _ = R.probe_statistics(st, inp, s0, s1)
    n = st.conv.N * int(np.prod(CR.output_dims(st.conv)))
    assert st not in [R.E, R.Ia, R.Is] + R.EXACT_MEAN_STAGES or n & (n - 1) == 0
    if n & (n - 1) == 0:                                                       # N * OH * OW a power of two (E's 256): the
        assert (mean.astype(np.float64) == s0 / float(n)).all()                # mean is exact
    # windows with ties: an extremum attained more than once, in channels of every sign of scale
    w = R.BM.windows(y, *st.pool)
    for k in (R.ZERO_CHANNEL, R.NEGATIVE_CHANNEL, R.POSITIVE_CHANNEL):
        assert ((w[:, k] == w[:, k].max(axis=-1, keepdims=True)).sum(axis=-1) > 1).any(), k
        assert ((w[:, k] == w[:, k].min(axis=-1, keepdims=True)).sum(axis=-1) > 1).any(), k
