"""CPU suite: tests/conv_reference.py is the layer, and its inputs are fit for the bars of tests/test_gpu_conv.py.

  * in float64 the model agrees with torch.nn.functional.conv2d and its autograd -- an independent statement of the
    same layer -- to 1e-12 on every shape of the GPU list and of the plan list (tests/test_gpu_conv_plans.py), groups,
    padding, strides and the accumulate-into rule included;
  * on the integer probes no partial sum of any path can leave float32's exact range, and the float32 run of the
    model equals the int64 run;
  * on the conditioned inputs the float32 run of the model stays within a quarter of TOL of its float64 run."""
import numpy as np
import pytest
import torch

import conv_reference as R
from util import SEED, TOL, assert_close

SHAPES = R.GPU_SHAPES + R.PLAN_SHAPES
IDS = ["-".join(str(v) for v in s) for s in SHAPES]


def _torch_outputs(s, inp):
    t = {k: (None if v is None else torch.from_numpy(v.astype(np.float64))) for k, v in inp.items()}
    x, w = t["x"].requires_grad_(), t["weight"].requires_grad_()
    b = None if t["bias"] is None else t["bias"].requires_grad_()
    top = torch.nn.functional.conv2d(x, w, b, stride=R.pair(s.stride), padding=R.pair(s.pad), groups=s.group)
    top.backward(t["top_diff"])
    out = dict(top=top.detach().numpy(), bottom_diff=x.grad.numpy(), weight_diff=(t["weight_diff0"] + w.grad).numpy())
    if b is not None:
        out["bias_diff"] = (t["bias_diff0"] + b.grad).numpy()
    return out


@pytest.mark.parametrize("s", SHAPES, ids=IDS)
def test_float64_model_is_conv2d(s):
    inp = R.conditioned_inputs(s, np.float64, SEED)
    got, want = R.model_outputs(s, inp, np.float64), _torch_outputs(s, inp)
    assert sorted(got) == sorted(want)
    assert got["top"].shape == (s.N, s.K) + R.output_dims(s)
    for k in want:
        assert_close(got[k], want[k], 1e-12, k)


@pytest.mark.parametrize("s", SHAPES, ids=IDS)
def test_integer_probe_is_exact_in_float32(s):
    assert R.probe_bound(s) < 2 ** 24
    OH, OW = R.output_dims(s)
    assert R.probe_bound(s) >= 16 * max((s.C // s.group) * s.kh * s.kw, (s.K // s.group) * s.kh * s.kw, s.N * OH * OW)
    inp = R.integer_probe(s, SEED)
    for v in inp.values():
        assert v is None or (v.dtype == np.int64 and np.abs(v).max() <= 4)
    exact = R.model_outputs(s, inp, np.int64)
    single = R.model_outputs(s, inp, np.float32)
    for k, v in exact.items():
        assert v.dtype == np.int64 and single[k].dtype == np.float32
        assert np.abs(v).max() <= R.probe_bound(s), k
        assert (single[k].astype(np.int64) == v).all() and (single[k] == v.astype(np.float32)).all(), k


@pytest.mark.parametrize("s", SHAPES, ids=IDS)
def test_conditioned_inputs_leave_room_under_the_bar(s):
    inp = R.conditioned_inputs(s, np.float32, SEED)
    single, double = R.model_outputs(s, inp, np.float32), R.model_outputs(s, inp, np.float64)
    for k, v in double.items():
        assert single[k].dtype == np.float32 and v.dtype == np.float64
        assert_close(single[k], v, TOL / 4, k)


def test_the_list_covers_what_it_claims():
    L = R.GPU_SHAPES
    assert any(s.N == 1 for s in L) and any(s.K == 1 for s in L) and any(not s.bias for s in L)
    assert any(s.kh != s.kw for s in L) and any(s.kh == s.kw == 1 for s in L) and any(s.group == 2 for s in L)
    assert any((s.C // s.group) * s.kh * s.kw % 4 for s in L)
    assert any(R.pair(s.pad) == (2, 2) and s.kh == s.kw == 5 for s in L)
    assert any(R.pair(s.stride) == (2, 2) and (s.H + 2 * R.pair(s.pad)[0] - s.kh) % 2 == 1 for s in L)
    assert any(R.output_dims(s)[1] % 2 == 1 and R.output_dims(s)[1] < 16 for s in L)
    assert (3, 4, 40, 40, 32, 5, 5) == tuple(L[0][:7]) and (3, 32, 9, 9, 64, 5, 5) == tuple(L[1][:7])
    # the plan list: what of its claims the shapes alone show (the plans themselves: tests/test_conv_plans.py)
    P = R.PLAN_SHAPES
    assert not set(P) & set(L) and len(set(P)) == len(P) == len(R.PLAN_CASES)
    assert all((R.pair(s.stride), R.pair(s.pad), s.group) == ((1, 1), (0, 0), 1) and max(s.C, s.K) <= 64 for s in P)
    assert any(R.output_dims(s) == (1, 1) for s in P) and any(R.output_dims(s) == (1, 1) and s.C == s.K == 1 for s in P)
    assert any(R.output_dims(s)[1] == 256 and s.W > 256 for s in P)
    assert any(s.C > 32 and s.W <= 256 and routes[1] == "F" for s, routes, _ in R.PLAN_CASES)
    assert any(s.C * s.kh * s.kw > 64 * 4 for s in P)
    assert any(not s.bias for s in P)
    assert {routes for _, routes, _ in R.PLAN_CASES} == {"FFF", "FGF", "FFG"}
    assert all(nbytes % ((s.K * s.C * s.kh * s.kw + s.K) * 4) == 0 for s, _, nbytes in R.PLAN_CASES)


def test_output_dims_truncate():
    assert R.output_dims(R.S(1, 1, 10, 10, 1, 3, 3, stride=2, pad=1)) == (5, 5)       # (10 + 2 - 3) / 2 = 4.5
    assert R.output_dims(R.S(1, 1, 40, 40, 1, 5, 5)) == (36, 36)
    assert R.output_dims(R.S(1, 1, 9, 9, 1, 5, 5)) == (5, 5)
