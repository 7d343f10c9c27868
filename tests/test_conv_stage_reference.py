"""CPU suite: tests/conv_stage_reference.py is the stage, and its inputs are fit for the bars of
tests/test_gpu_conv_stage.py.

  * in float64 the model agrees with torch on the CPU -- conv2d, eval-mode batch norm with eps = 1e-9, avg_pool2d, tanh:
    an independent statement of the same four layers -- to 1e-12 on every shape of the GPU list;
  * the float32 restatement of the finish, on the model's own float32 map, stays within a quarter of TOL of float64;
  * on the integer probes no partial sum leaves float32's exact range."""
import numpy as np
import pytest
import torch

import conv_reference as CR
import conv_stage_reference as R
from util import SEED, TOL, assert_close

IDS = [R.stage_id(st) for st in R.GPU_STAGES]


def _torch_outputs(st, inp):
    s = st.conv
    t = {k: (None if v is None else torch.from_numpy(np.array(v, dtype=np.float64))) for k, v in inp.items()}
    y = torch.nn.functional.conv2d(t["x"], t["weight"], t["bias"], stride=CR.pair(s.stride), padding=CR.pair(s.pad),
                                   groups=s.group)
    bn = torch.nn.functional.batch_norm(y, t["mean"], t["var"], t["scale"], t["shift"], training=False, eps=1e-9)
    top = torch.tanh(torch.nn.functional.avg_pool2d(bn, st.pool))
    c = (None, slice(None), None, None)
    sp = torch.nn.functional.avg_pool2d((y - t["mean"][c]) / torch.sqrt(t["var"][c] + 1e-9), st.pool)
    return dict(top=top.numpy(), save_pool=sp.numpy())


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
    assert y.dtype == np.int64
    window = sum(np.abs(y[:, :, i::st.pool[0], j::st.pool[1]]) for i in range(st.pool[0]) for j in range(st.pool[1]))
    assert window.max() <= R.probe_bound(st)
    for k in ("mean", "var", "scale", "shift"):
        assert inp[k].dtype == np.float32 and inp[k].shape == (st.conv.K,)
    top, sp = R.probe_outputs(st, inp)
    assert top.dtype == np.float32 and sp.shape == R.pooled_shape(st)
    # the finish of the exact map is the float64 finish rounded once or twice: nowhere near the bar
    want = R.model_outputs(st, inp, np.float64)
    assert_close(sp, want["save_pool"], 1e-6, "save_pool")


def test_the_list_covers_what_it_claims():
    F, Q = R.FUSED_STAGES, R.SEQUENCE_STAGES
    assert tuple(F[0].conv[:7]) == (3, 4, 40, 40, 32, 5, 5) and F[0].pool == (4, 4)
    assert tuple(F[1].conv[:7]) == (23, 32, 9, 9, 64, 5, 5) and F[1].pool == (5, 5)
    assert any(st.conv.K == 20 and not st.conv.bias for st in F) and any(st.conv.K == 5 and not st.conv.bias for st in F)
    assert any(CR.output_dims(st.conv)[0] == 20 and st.pool[0] == 2 for st in F)
    assert any(st.pool[0] == 3 and 256 // CR.output_dims(st.conv)[1] % 3 for st in F)
    assert any(st.conv.N == 1 for st in F) and tuple(F[2].conv[:7]) == (93, 32, 9, 9, 64, 5, 5)
    assert any(CR.pair(st.conv.stride) == (2, 2) for st in Q) and any(st.conv.group == 2 for st in Q)
    assert any(st.conv.C == 65 for st in Q)
    assert any(st.pool[0] * CR.output_dims(st.conv)[1] > 256 for st in Q)
    for st in F + Q:
        OH, OW = CR.output_dims(st.conv)
        assert OH % st.pool[0] == 0 and OW % st.pool[1] == 0
