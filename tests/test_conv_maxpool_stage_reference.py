"""CPU suite: tests/conv_maxpool_stage_reference.py is the stage, and its inputs are fit for the bars of
tests/test_gpu_conv_maxpool_stage.py.

  * in float64 the model agrees with torch on the CPU -- conv2d, the per-channel affine map of eval-mode BN with
    eps = 1e-9, max_pool2d (of the negated map for a negative scale: the smallest element; the window's first element
    for scale == 0), tanh: an independent statement of the same four layers -- to 1e-12 on every shape of the GPU list;
  * the float32 restatement of the finish, on the model's own float32 map, stays within a quarter of TOL of float64;
  * on the integer probes no element of the map leaves float32's exact range, and the windows do hold ties."""
import numpy as np
import pytest
import torch

import bn_maxpool_reference as BM
import conv_reference as CR
import conv_maxpool_stage_reference as R
from util import SEED, TOL, assert_close

IDS = [R.stage_id(st) for st in R.GPU_STAGES]


def _torch_outputs(st, inp):
    s, (ph, pw) = st.conv, st.pool
    t = {k: (None if v is None else torch.from_numpy(np.array(v, dtype=np.float64))) for k, v in inp.items()}
    y = torch.nn.functional.conv2d(t["x"], t["weight"], t["bias"], stride=CR.pair(s.stride), padding=CR.pair(s.pad),
                                   groups=s.group)
    c = (None, slice(None), None, None)
    xn = (y - t["mean"][c]) / torch.sqrt(t["var"][c] + 1e-9)
    hi, lo = torch.nn.functional.max_pool2d(xn, st.pool), -torch.nn.functional.max_pool2d(-xn, st.pool)
    sc = t["scale"][c]
    sp = torch.where(sc > 0, hi, torch.where(sc < 0, lo, xn[:, :, ::ph, ::pw]))
    return dict(top=torch.tanh(sp * sc + t["shift"][c]).numpy(), save_pool=sp.numpy())


@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS)
def test_float64_model_is_torch(st):
    inp = R.conditioned_inputs(st, np.float64, SEED)
    got, want = R.model_outputs(st, inp, np.float64), _torch_outputs(st, inp)
    for k in ("top", "save_pool"):
        assert got[k].shape == R.pooled_shape(st) and got[k].dtype == np.float64
        assert_close(got[k], want[k], 1e-12, k)


@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS)
def test_float32_finish_leaves_room_under_the_bar(st):
    inp = R.conditioned_inputs(st, np.float32, SEED)
    want = R.model_outputs(st, inp, np.float64)
    y = CR.conv_forward(st.conv, inp["x"], inp["weight"], inp["bias"])
    assert y.dtype == np.float32
    top, sp = R.finish(y, st.pool, inp["mean"], inp["var"], inp["scale"], inp["shift"])
    assert top.dtype == np.float32 and sp.dtype == np.float32
    assert_close(top, want["top"], TOL / 4, "top")
    assert_close(sp, want["save_pool"], TOL / 4, "save_pool")


@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS)
def test_integer_probe_is_exact_in_float32(st):
    assert R.probe_bound(st) < 2 ** 24
    inp = R.integer_probe(st, SEED)
    y = CR.conv_forward(st.conv, inp["x"], inp["weight"], inp["bias"])
    assert y.dtype == np.int64 and np.abs(y).max() <= R.probe_bound(st)
    for k in ("mean", "var", "scale", "shift"):
        assert inp[k].dtype == np.float32 and inp[k].shape == (st.conv.K,)
    top, sp = R.probe_outputs(st, inp)
    assert top.dtype == np.float32 and sp.shape == R.pooled_shape(st)
    # the finish of the exact map is the float64 finish rounded once or twice: nowhere near the bar
    want = R.model_outputs(st, inp, np.float64)
    assert_close(sp, want["save_pool"], 1e-6, "save_pool")
    # ties, at the shapes the fused launch reaches: some window attains its largest element more than once, and the
    # zero-scale channel's first element is not always its largest, so the first-element rule shows in save_pool
    ph, pw = st.pool
    if st in R.FUSED_STAGES:
        w = BM.windows(y, ph, pw)
        assert ((w == w.max(axis=-1, keepdims=True)).sum(axis=-1) > 1).any()
        first, best = w[:, R.ZERO_CHANNEL, ..., 0], w[:, R.ZERO_CHANNEL].max(axis=-1)
        assert (first != best).any(), "the zero-scale channel's first element is not always its largest"


@pytest.mark.parametrize("st", R.GPU_STAGES, ids=IDS)
def test_every_scan_direction_runs(st):
    for inp in (R.conditioned_inputs(st, np.float32, SEED), R.integer_probe(st, SEED)):
        sc = inp["scale"]
        assert sc[R.ZERO_CHANNEL] == 0.0 and sc[R.NEGATIVE_CHANNEL] < 0 and (sc > 0).any()
        assert np.abs(sc[sc != 0]).min() >= 0.5
    base = R.A.conditioned_inputs(st, np.float32, SEED)
    got = R.conditioned_inputs(st, np.float32, SEED)
    for k in base:                                          # everything but scale is conv_stage_reference's
        if k != "scale" and base[k] is not None:
            assert np.array_equal(base[k], got[k]), k


def test_the_lists_cover_what_they_claim():
    N, F, Q = R.NET_STAGES, R.FUSED_STAGES, R.SEQUENCE_STAGES
    assert [tuple(st.conv[:7]) + st.pool for st in N] == [
        (3, 1, 40, 40, 64, 5, 5, 4, 4), (23, 64, 9, 9, 64, 5, 5, 5, 5), (3, 2, 40, 40, 32, 3, 3, 2, 2),
        (5, 32, 19, 19, 32, 4, 4, 2, 2), (15, 32, 8, 8, 32, 3, 3, 6, 6)]
    assert [CR.output_dims(st.conv) for st in N] == [(36, 36), (5, 5), (38, 38), (16, 16), (6, 6)]
    assert 23 % (256 // 25) == 3 and 15 % (256 // 36) == 1                # the ragged last workgroups
    assert F[:5] == N and F[5:7] == R.MAIN_FUSED_STAGES and F[7:] == R.A.FUSED_STAGES and Q == R.A.SEQUENCE_STAGES
    assert 8 * 7 == 56 and -(-414 // 7) == 60 and 414 % 7 == 1
    assert any(st.conv.K == 20 and not st.conv.bias for st in F) and any(st.conv.K == 5 and not st.conv.bias for st in F)
    assert any(CR.output_dims(st.conv)[0] == 20 and st.pool[0] == 2 for st in F)
    assert any(st.conv.N == 1 for st in F) and any(st.pool[1] == CR.output_dims(st.conv)[1] for st in F)
    assert any(CR.pair(st.conv.stride) == (2, 2) for st in Q) and any(st.conv.group == 2 for st in Q)
    assert any(st.conv.C == 65 for st in Q)
    assert any(st.pool[0] * CR.output_dims(st.conv)[1] > 256 for st in Q)
    assert all(st in F for st in R.SAME_CHUNK_STAGES) and all(st.conv.C * st.conv.kh * st.conv.kw <= 25
                                                              for st in R.SAME_CHUNK_STAGES)
    for st in F + Q:
        OH, OW = CR.output_dims(st.conv)
        assert OH % st.pool[0] == 0 and OW % st.pool[1] == 0 and st.conv.K >= 3
