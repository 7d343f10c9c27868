"""GPU suite: the BN -> MaxPool -> TanH calls of the C ABI (include/mms_bn_maxpool.h, csrc/bn_pool.hip) against the
float64 run of tests/bn_maxpool_reference.py -- the three reference layers in sequence -- on the same inputs.  Parity is
the project's 1e-5 (float32) and 1e-12 (float64) in assert_close's metric, on inputs whose windows all have a top-two
gap (tests/test_bn_maxpool_reference.py); where the gradient goes among equal BN outputs, the statistics' order,
alignment, what the workspace held and what is written are tested by equality of words or on exact probes.  The bodies
that do not depend on the pooling method are tests/pooled_stage_suite.py's, bound here to these calls."""
import numpy as np
import pytest
import torch

import bn_maxpool_reference as R
import bn_pool_reference as P
from pooled_stage_suite import BAR, BnPool, same_words
from test_gpu_bn import DTYPES, IDS, assert_words_equal, host
from util import SEED, assert_close

pytestmark = pytest.mark.gpu

S = BnPool("bn_maxpool", "bn_maxpool_tanh", R, shift_in_backward=True)
AVE = BnPool("capi", "bn_pool_tanh", P, shift_in_backward=False)
api, inputs, run = S.api, S.inputs, S.run


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", R.PARITY_SHAPES, ids=str)
def test_parity_and_determinism(shape, dtype, hiplib):
    S.check_parity_and_determinism(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_both_sides_of_the_routing_threshold(dtype, hiplib):
    S.check_both_sides_of_the_routing_threshold(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(3, 2, 36, 36, 4, 4), (20, 3, 36, 36, 4, 4), (405, 2, 36, 36, 4, 4),
                                   (65, 5, 9, 37, 3, 37), (3652, 1, 12, 12, 12, 12)], ids=str)
def test_statistics_are_the_ave_calls(shape, dtype, hiplib):
    """save_mean, save_std, running_mean and running_var of the TRAIN forward are mms_bn_pool_tanh_forward's words on
    the same x, on both routes: one workgroup per channel, a few chunks, 64 ragged chunks, and 63 chunks of a window
    the kernels learn at run time."""
    query, ave_query = api(dtype)[2], AVE.api(dtype)[2]
    assert query(*shape) == ave_query(*shape)
    item = np.dtype(dtype).itemsize
    if shape[0] == 405 and dtype == np.float32:
        assert query(*shape) == shape[1] * 64 * 4 * item
    if shape[0] == 3652 and dtype == np.float32:
        assert query(*shape) >= shape[1] * 63 * 4 * item
    inp = P.conditioned_inputs(shape, dtype, SEED)
    got, want = run(inp, shape[4:], dtype, phases=("train",)), AVE.run(inp, shape[4:], dtype)
    for k in ("save_mean", "save_std", "running_mean", "running_var"):
        assert_words_equal(got["train_" + k], want["train_" + k], k)


def var_with_std(dtype, std):
    """A variance, found by search, with sqrt(var + 1e-9) == std exactly in the type (asserted)."""
    c = dtype(std * std) - dtype(1e-9)
    for _ in range(64):
        s = np.sqrt(c + dtype(1e-9))
        if s == dtype(std):
            return c
        c = np.nextafter(c, dtype(0) if s > std else dtype(np.inf))
    raise AssertionError("no variance gives std == %r in %s" % (std, dtype))


def exact_probe(shape, dtype, seed):
    """Integer x with |x| <= 4 whose window extremum -- largest in channels 0 mod 3, smallest in 1 mod 3, channel 2 mod
    3 has scale 0 -- is repeated two or three times at chosen positions; TEST-phase statistics with an integer mean and
    std == 2 exactly in the type; dyadic scale and shift: every BN output is exact."""
    N, C, H, W, kh, kw = shape
    r = np.random.default_rng(seed)
    ke = kh * kw
    w = r.integers(-3, 4, size=(N, C, H // kh, W // kw, ke)).astype(dtype)
    sign = np.array([1, -1, 0])[np.arange(C) % 3]
    reps = r.integers(2, 4, size=w.shape[:-1])
    for idx in np.ndindex(*w.shape[:-1]):
        at = r.choice(ke, size=min(int(reps[idx]), ke), replace=False)
        w[idx][at] = 4 * (sign[idx[1]] or 1)
    var = var_with_std(dtype, 2)
    assert np.sqrt(var + dtype(1e-9)) == dtype(2)
    inp = dict(x=R.unwindows(w, kh, kw), scale=(sign * np.array([0.5, 2, 1])[np.arange(C) % 3]).astype(dtype),
               shift=np.full(C, 0.25, dtype), running_mean=r.integers(-2, 3, C).astype(dtype),
               running_var=np.full(C, var, dtype),
               top_diff=r.integers(-4, 5, size=(N, C, H // kh, W // kw)).astype(dtype))
    assert (inp["scale"] > 0).any() and (inp["scale"] < 0).any() and (inp["scale"] == 0).any()
    return inp


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(3, 3, 8, 8, 4, 4), (3, 3, 4, 6, 2, 3), (20, 3, 36, 36, 4, 4), (700, 3, 4, 6, 2, 3)],
                         ids=str)
def test_ties_go_to_the_first(shape, dtype, hiplib):
    """Repeated extrema: save_pool is the model's word for word, and bottom_diff is the same-dtype sequence model's at
    the parity bar -- a gradient on the wrong element is an O(1) error.  Small and large route, compile-time 4 x 4 and
    run-time 2 x 3 windows, TEST phase."""
    _, _, query = api(dtype)
    assert (query(*shape) > 0) == (shape[0] >= 20)          # 25920 and 16800 elements per channel: two launches
    inp = exact_probe(shape, dtype, SEED + 3)
    got = run(inp, shape[4:], dtype, phases=("test",))
    want = R.model_outputs(inp, shape[4:])
    assert want["test_save_pool"].dtype == dtype
    assert_words_equal(got["test_save_pool"], want["test_save_pool"], "save_pool")
    assert_words_equal(got["test_save_std"], np.full(shape[1], 2, dtype), "std == 2")
    for k in ("test_top", "test_bottom_diff"):
        assert_close(got[k], want[k], BAR[dtype], k)
    assert np.abs(want["test_bottom_diff"]).max() > 0.1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shift", [1024, 1])
def test_rounding_collapse_follows_the_bn_output(shift, dtype, hiplib):
    """TEST phase, std == 4, scale == 1 and a shift large enough that x_1 > x_0 but bn_out(x_0) == bn_out(x_1) in the
    type (float: shift 1024, x = 0.5 and 0.5 + 2^-20; double: the same with 2^-49): the first maximum of y is element
    0, arg-max x is element 1.  bottom_diff is the same-dtype sequence model's, whose gradient is on element 0, and top
    is tanh(bn_out(x_1)).  At shift 1024 the TanH is saturated and every gradient is 0; shift 1 with x_1 the next number
    after 0.5 is the same collapse with a gradient to place."""
    eps = np.finfo(dtype).eps
    x = np.zeros((1, 1, 2, 2), dtype)
    x[0, 0] = [[0.5, 0.5 + 8 * eps if shift == 1024 else np.nextafter(dtype(0.5), dtype(1))], [-1, -2]]
    var = var_with_std(dtype, 4)
    inp = dict(x=x, scale=np.ones(1, dtype), shift=np.full(1, shift, dtype), running_mean=np.zeros(1, dtype),
               running_var=np.full(1, var, dtype), top_diff=np.ones((1, 1, 1, 1), dtype))
    y = x / dtype(4) * dtype(1) + dtype(shift)
    assert y.dtype == dtype and np.sqrt(var + dtype(1e-9)) == 4
    assert x[0, 0, 0, 1] > x[0, 0, 0, 0] and y[0, 0, 0, 0] == y[0, 0, 0, 1]
    got = run(inp, (2, 2), dtype, phases=("test",))
    want = R.model_outputs(inp, (2, 2))
    assert_close(got["test_bottom_diff"], want["test_bottom_diff"], BAR[dtype], "bottom_diff")
    assert_close(got["test_top"], np.tanh(y[:, :, :1, 1:]), BAR[dtype], "top")
    if shift == 1:
        d = want["test_bottom_diff"][0, 0]
        assert abs(d[0, 0] - d[0, 1]) > 0.01                  # the two candidates do differ in the model


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_variance_is_exact(dtype, hiplib):
    S.check_zero_variance_is_exact(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 3, 4, 6, 2, 3), (65, 5, 9, 37, 3, 37)], ids=str)
def test_optional_backward_outputs(shape, dtype, hiplib):
    S.check_optional_backward_outputs(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(3, 2, 36, 36, 4, 4), (20, 3, 36, 36, 4, 4), (129, 3, 8, 16, 2, 4),
                                   (3, 2, 16, 16, 2, 2)], ids=str)
def test_unaligned_operands_give_the_same_words(shape, dtype, hiplib):
    """Every operand one element off a 16-byte boundary: the words of the aligned run."""
    inp = inputs(shape, dtype)
    same_words(run(inp, shape[4:], dtype, shift=1), run(inp, shape[4:], dtype), "off by one element")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(20, 3, 36, 36, 4, 4), (130, 3, 25, 41, 5, 1)], ids=str)
def test_workspace_content_does_not_matter(shape, dtype, hiplib):
    """A workspace of exactly the queried size, every word a NaN, between guard zones that stay intact."""
    from mms_answer_selection_amd import capi
    _, _, query = api(dtype)
    inp = inputs(shape, dtype)
    need = query(*shape)
    assert need > 0
    want = run(inp, shape[4:], dtype)
    guard = 256
    buf = torch.full((need + 2 * guard,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = capi.Workspace()
    ws.buf = buf[guard:guard + need]
    assert ws.buf.data_ptr() % 16 == 0 and ws.buf.numel() == need
    same_words(run(inp, shape[4:], dtype, ws=ws), want, "workspace of NaNs")
    assert ws.buf.data_ptr() == buf.data_ptr() + guard
    b = host(buf)
    assert (b[:guard] == 0xFF).all() and (b[guard + need:] == 0xFF).all()
    assert not np.isnan(host(ws.buf).view(dtype)[:2]).any()          # the call did use it


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_stays_in_its_window(dtype, hiplib):
    shape = (3, 2, 8, 8, 4, 4)
    inp = dict(inputs(shape, dtype))
    clean = run(inp, shape[4:], dtype, phases=("test",))
    x = np.array(inp["x"])
    x[1, 1, 5, 2] = np.nan                                  # window (1, 0) of map (1, 1), not its first element
    inp["x"] = x
    got = run(inp, shape[4:], dtype, phases=("test",))
    hit = np.zeros(clean["test_top"].shape, bool)
    hit[1, 1, 1, 0] = True
    for k in ("test_top", "test_save_pool"):
        assert_words_equal(got[k][~hit], clean[k][~hit], k)
    assert not np.isnan(got["test_top"][hit]).any()          # a NaN never wins a comparison
