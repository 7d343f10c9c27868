"""CPU suite: the closed forms the tail's fused backward rests on (include/mms_train_tail_backward.h) against the float64
model of the sequence (tests/train_tail_reference.py), AVE and MAX, negative scales included, at 1e-12; and the exact
probe's property: every value the float64 model forms from it is a float32 value."""
import numpy as np
import pytest

import head_reference as HR
import train_tail_backward_cases as B
import train_tail_reference as R
from util import SEED, assert_close

POOL_IDS = lambda p: R.POOL_NAME[p]                                                 # noqa: E731


def x0_diff(t, inp, fwd, config, ty=np.float64):
    hb = HR.backward(R.head_shape(t), config, R._head_inputs(inp, fwd["flt"].astype(ty), ty), fwd["h"], fwd["prob"], ty)
    return hb["x0_diff"]


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
@pytest.mark.parametrize("t", [R.small(5), B.k17(3), R.v5(3)], ids=R.tail_id)
def test_closed_forms_equal_the_model(t, pool):
    inp = dict(R.conditioned_inputs(t, np.float64, SEED))
    scale = np.asarray(inp["scale"])                     # the conditioned scales come with both signs
    assert (scale < 0).any() and (scale > 0).any()
    fwd = R.forward(t, pool, inp)
    want = R.backward(t, pool, inp, fwd)
    s = t.stage.conv
    c = lambda k: np.asarray(inp[k], np.float64)                                    # noqa: E731
    dy, scale_diff, shift_diff = B.closed_forms(t, pool, fwd["y"], fwd["flt"], x0_diff(t, inp, fwd, R.cfg()),
                                                fwd["save_pool"], fwd["save_mean"], fwd["save_std"], c("scale"), c("shift"))
    dx, dw, db = R.S.CR.conv_backward(s, c("x"), c("weight"), dy, c("weight_diff0"),
                                      None if inp["bias_diff0"] is None else c("bias_diff0"))
    got = dict(scale_diff=scale_diff, shift_diff=shift_diff, bottom_diff=dx, weight_diff=dw)
    if db is not None:
        got["bias_diff"] = db
    for k, v in got.items():
        assert_close(v, want[k], 1e-12, "%s, %s" % (k, R.POOL_NAME[pool]))
    assert np.abs(want["bottom_diff"]).max() > 0


@pytest.mark.parametrize("pool", R.POOLS, ids=POOL_IDS)
def test_the_exact_probe_is_exact_in_float32(pool):
    inp, fwd = B.exact_probe(pool)
    t, cfg = B.PROBE, B.probe_config()
    N, K = fwd["flt"].shape
    OH, OW = fwd["y"].shape[2:]
    assert (N * OH * OW) & (N * OH * OW - 1) == 0                  # N S is a power of two
    assert not fwd["flt"].any() and not fwd["h"].any() and not fwd["save_mean"].any()
    for v in (fwd["save_std"], np.abs(inp["scale"])):
        m, _ = np.frexp(v)
        assert (m == 0.5).all()                                     # powers of two
    f64 = {k: v.astype(np.float64) for k, v in fwd.items()}
    want = R.backward(t, pool, inp, f64, cfg)
    g = x0_diff(t, inp, f64, cfg)
    c = lambda k: np.asarray(inp[k], np.float64)                                    # noqa: E731
    dy, sd, shd = B.closed_forms(t, pool, f64["y"], f64["flt"], g, f64["save_pool"], f64["save_mean"], f64["save_std"],
                                 c("scale"), c("shift"))
    values = dict(want, x0_diff=g, dy=dy, closed_scale_diff=sd, closed_shift_diff=shd, g_pool=g * f64["save_pool"])
    for k, v in values.items():
        v = np.asarray(v, np.float64)
        bad = np.flatnonzero(v.astype(np.float32).astype(np.float64).reshape(-1) != v.reshape(-1))
        assert bad.size == 0, (k, bad[:4])
    assert_close(sd, want["scale_diff"], 0, "scale_diff")
    assert_close(shd, want["shift_diff"], 0, "shift_diff")
    # the save_pool given is the model's own: the pooled, normalised y
    pooled = f64["y"].reshape(N, K, -1)
    ref = pooled.mean(axis=2) if pool == R.AVE else np.where(c("scale")[None] < 0, pooled.min(axis=2), pooled.max(axis=2))
    assert (ref / f64["save_std"][None] == f64["save_pool"]).all()
    assert np.abs(want["bottom_diff"]).max() > 0 and np.abs(want["scale_diff"]).max() > 0
