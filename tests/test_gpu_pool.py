"""GPU suite of the Pooling and TanH calls (include/mms_pool.h): word equality with tests/pool_reference.py, the literal
restatement of pooling_layer.cpp, in float and double, for top, mask, top_mask and bottom_diff, at the shapes listed
there -- each chosen for a way a kernel can go wrong -- plus MAX's selection rules, the order of the backward's
additions, the two sources of the mask, arrays off a 16-byte boundary, calls larger than the largest grid, TanH, and
the unfused chain BN -> Pooling -> TanH against the float64 model of the fused call."""
import functools

import numpy as np
import pytest
import torch

import bn_maxpool_reference as BM
import bn_pool_reference as BP
import pool_reference as R
from util import SEED, TOL

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
F64_TOL = 1e-12
METHODS = [("max", R.MAX), ("ave", R.AVE)]


@pytest.fixture(scope="module")
def pool(hiplib):
    from mms_answer_selection_amd import pool
    pool.lib()
    return pool


def dev(a, off=0):
    """a on the device; off = 1: its first element one element past a 16-byte boundary (torch's blocks are aligned)."""
    t = torch.from_numpy(np.array(a))                    # a copy: the cached cases are read-only
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def empty(shape, dtype, off=0):
    buf = torch.empty(int(np.prod(shape)) + off, dtype=dtype, device="cuda")
    return buf[off:].view(tuple(shape))


def host(t):
    return t.cpu().numpy()


def same_words(got, want, what):
    got, want = np.ascontiguousarray(host(got) if isinstance(got, torch.Tensor) else got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = {4: np.uint32, 8: np.uint64}[got.itemsize]
    bad = np.flatnonzero(got.ravel().view(u) != want.ravel().view(u))
    assert not bad.size, "%s: %d of %d words differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


@functools.lru_cache(maxsize=None)
def case(sh, dtype, method):
    """bottom, top_diff and the model's top, mask, bottom_diff: computed once, read-only."""
    r = np.random.default_rng(SEED + len(sh.dims) + sh.dims[3])
    x = r.standard_normal(sh.dims).astype(dtype)
    top, mask = R.forward(sh, method, x)
    td = r.standard_normal(top.shape).astype(dtype)
    bd = R.backward(sh, method, td, mask)
    for a in (x, top, td, bd) + ((mask,) if mask is not None else ()):
        a.setflags(write=False)
    return x, td, top, mask, bd


def run(pool, sh, mname, x, td, off=0, masks=(True, True)):
    """forward, then backward from what it left -> top, mask, top_mask, bottom_diff (device tensors)"""
    tdt = torch.float32 if x.dtype == np.float32 else torch.float64
    PH, PW = R.output_dims(sh)
    pooled = sh.dims[:2] + (PH, PW)
    xd, tdd = dev(x, off), dev(td, off)
    top = empty(pooled, tdt, off)
    mask = empty(pooled, torch.int32, off) if masks[0] else None
    tmask = empty(pooled, tdt, off) if masks[1] else None
    res = pool.pool_forward(xd, mname, sh.kernel, sh.stride, sh.pad, mask=mask, top_mask=tmask, out=top)
    assert (res[0] if isinstance(res, tuple) else res) is top
    bd = empty(sh.dims, tdt, off)
    if mname == "ave" or mask is not None or tmask is not None:
        pool.pool_backward(tdd, sh.dims, mname, sh.kernel, sh.stride, sh.pad, mask=mask, top_mask=tmask, out=bd)
    else:
        bd = None
    torch.cuda.synchronize()
    return top, mask, tmask, bd


def check(pool, sh, dtype, mname, method, off=0):
    x, td, top_w, mask_w, bd_w = case(sh, dtype, method)
    top, mask, tmask, bd = run(pool, sh, mname, x, td, off)
    what = "%s %s %s off %d" % (R.shape_id(sh), mname, dtype.__name__, off)
    same_words(top, top_w, what + " top")
    if method == R.MAX:
        same_words(mask, mask_w, what + " mask")
        same_words(tmask, mask_w.astype(dtype), what + " top_mask")
    same_words(bd, bd_w, what + " bottom_diff")
    return top, mask, tmask, bd


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mname,method", METHODS, ids=[m[0] for m in METHODS])
@pytest.mark.parametrize("sh", R.SHAPES + R.PLAN_SHAPES, ids=R.shape_id)
def test_words_equal_the_model(pool, sh, mname, method, dtype):
    check(pool, sh, dtype, mname, method)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mname,method", METHODS, ids=[m[0] for m in METHODS])
@pytest.mark.parametrize("sh", R.SHAPES[3:5] + R.SHAPES[11:15] + R.PLAN_SHAPES[1:2], ids=R.shape_id)
def test_every_array_one_element_off_a_16_byte_boundary(pool, sh, mname, method, dtype):
    top, mask, tmask, bd = check(pool, sh, dtype, mname, method, off=1)
    assert all(t.data_ptr() % 16 == top.element_size() for t in (top, tmask, bd)) and mask.data_ptr() % 16 == 4


def test_uncovered_elements_get_plus_zero(pool):
    sh = R.SHAPES[9]
    assert sh.stride > sh.kernel
    for mname, method in METHODS:
        for dtype in DTYPES:
            x, td, _, _, want = case(sh, dtype, method)
            bd = host(run(pool, sh, mname, x, td)[3])
            for a in (want, bd):                               # rows and columns 2 and 5 are in no window
                assert (a[:, :, 2::3, :] == 0).all() and not np.signbit(a[:, :, 2::3, :]).any()
                assert (a[:, :, :, 2::3] == 0).all() and not np.signbit(a[:, :, :, 2::3]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_masks_are_optional_and_a_second_run_repeats_the_words(pool, dtype):
    sh = R.SHAPES[4]
    x, td, top_w, mask_w, bd_w = case(sh, dtype, R.MAX)
    first = run(pool, sh, "max", x, td)
    again = run(pool, sh, "max", x, td)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # a TEST pass: both mask outputs NULL; then each alone, and the backward from each alone
    top, mask, tmask, bd = run(pool, sh, "max", x, td, masks=(False, False))
    assert mask is None and tmask is None and bd is None
    same_words(top, top_w, "top, no masks")
    top, mask, tmask, bd = run(pool, sh, "max", x, td, masks=(True, False))
    assert tmask is None
    same_words(top, top_w, "top, mask alone")
    same_words(mask, mask_w, "mask alone")
    same_words(bd, bd_w, "bottom_diff from mask alone")
    top, mask, tmask, bd = run(pool, sh, "max", x, td, masks=(False, True))
    assert mask is None
    same_words(tmask, mask_w.astype(dtype), "top_mask alone")
    same_words(bd, bd_w, "bottom_diff from top_mask alone")
    # both given: mask is read
    other = dev(np.full(mask_w.shape, -1, dtype))
    bd2 = pool.pool_backward(dev(td), sh.dims, "max", sh.kernel, sh.stride, sh.pad, mask=dev(mask_w), top_mask=other)
    same_words(bd2, bd_w, "bottom_diff, mask over top_mask")
    # AVE ignores and does not write them
    canary = torch.full(mask_w.shape, 12345, dtype=torch.int32, device="cuda")
    fcanary = canary.to(torch.float32 if dtype == np.float32 else torch.float64)
    pool.pool_forward(dev(x), "ave", sh.kernel, sh.stride, sh.pad, mask=canary, top_mask=fcanary)
    torch.cuda.synchronize()
    assert (canary == 12345).all() and (fcanary == 12345).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_host_mask_with_entries_that_name_nothing(pool, dtype):
    """-1, and indices outside their own window (the header's two deviations), contribute nothing; the rest does."""
    sh = R.SHAPES[4]
    x, td, _, mask_w, _ = case(sh, dtype, R.MAX)
    r = np.random.default_rng(SEED)
    mask = mask_w.copy()
    flat = mask.reshape(-1)
    pick = r.permutation(flat.size)
    flat[pick[: flat.size // 4]] = -1
    far = pick[flat.size // 4: flat.size // 2]
    H, W = sh.dims[2:]
    flat[far] = (flat[far] + 4 * W) % (H * W)                     # four rows away: outside a 3 x 3 window
    want = R.backward(sh, R.MAX, td, mask)
    assert want.tobytes() != case(sh, dtype, R.MAX)[4].tobytes()
    got = pool.pool_backward(dev(td), sh.dims, "max", sh.kernel, sh.stride, sh.pad, mask=dev(mask))
    same_words(got, want, "bottom_diff, host mask")
    tm = mask.astype(dtype)
    tm.reshape(-1)[pick[:3]] = [np.nan, -np.inf, 1e30]
    got = pool.pool_backward(dev(td), sh.dims, "max", sh.kernel, sh.stride, sh.pad, top_mask=dev(tm))
    same_words(got, R.backward(sh, R.MAX, td, tm), "bottom_diff, host top_mask")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_max_selection(pool, dtype):
    nan, inf = np.nan, np.inf
    sh = R.S((1, 8, 2, 2), 2, 2)
    planes = [[3, 3, 3, 3], [0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, 0.0, 0.0], [1, nan, 2, nan], [nan] * 4, [-inf] * 4,
              [nan, -1, nan, -1], [-R.FLT_MAX, -inf, nan, -R.FLT_MAX]]
    if dtype is np.float64:
        planes[7] = [-1e300, -2e300, -1e300, -3e300]              # below -FLT_MAX: as if nothing were there
    x = np.array(planes, dtype).reshape(sh.dims)
    top_w, mask_w = R.forward(sh, R.MAX, x)
    assert list(mask_w.ravel()) == [0, 0, 0, 2, -1, -1, 1, -1]
    assert (top_w.ravel()[[4, 5, 7]] == dtype(-R.FLT_MAX)).all()
    td = np.arange(1, 9).astype(dtype).reshape(1, 8, 1, 1)
    top, mask, tmask, bd = run(pool, sh, "max", x, td)
    same_words(top, top_w, "top")
    same_words(mask, mask_w, "mask")
    same_words(tmask, mask_w.astype(dtype), "top_mask")
    same_words(bd, R.backward(sh, R.MAX, td, mask_w), "bottom_diff")
    assert (host(bd)[0, [4, 5, 7]] == 0).all()                    # nothing in the backward
    # a constant map gives each window's first index
    sh = R.S((1, 2, 7, 9), 3, 2, 1)
    x = np.full(sh.dims, 2.5, dtype)
    top_w, mask_w = R.forward(sh, R.MAX, x)
    top, mask, _, _ = run(pool, sh, "max", x, np.ones(top_w.shape, dtype))
    same_words(mask, mask_w, "mask of a constant map")
    assert mask_w[0, 0, 0, 0] == 0 and mask_w[0, 0, 1, 1] == 1 * 9 + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("mname,method", METHODS, ids=[m[0] for m in METHODS])
def test_backward_adds_in_the_order_of_the_walk(pool, mname, method, dtype):
    sh, x, td, swap = R.order_probe(method, dtype)
    top_w, mask_w = R.forward(sh, method, x)
    want = R.backward(sh, method, td, mask_w)
    assert want.tobytes() != R.backward(sh, method, td, mask_w, swap=swap).tobytes()
    top, mask, tmask, bd = run(pool, sh, mname, x, td)
    same_words(bd, want, "bottom_diff of the order probe")


@pytest.mark.parametrize("elem", [4, 8], ids=DT_IDS)
@pytest.mark.parametrize("which", ["staged", "direct"])
def test_calls_larger_than_the_largest_grid(pool, which, elem):
    """More items than workgroups (tests/test_abi_pool.py reads that from the plan).  The planes repeat five distinct
    ones, which the model is run on: planes share nothing."""
    dtype = np.float32 if elem == 4 else np.float64
    sh = (R.LOOP_SHAPES if which == "staged" else R.DIRECT_LOOP_SHAPES)[elem]
    small = sh._replace(dims=(5,) + sh.dims[1:])
    reps = -(-sh.dims[0] // 5)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1, 1, 1))[: sh.dims[0]])
    for mname, method in METHODS:
        x, td, top_w, mask_w, bd_w = case(small, dtype, method)
        top, mask, tmask, bd = run(pool, sh, mname, tile(x), tile(td))
        same_words(top, tile(top_w), "top")
        if method == R.MAX:
            same_words(mask, tile(mask_w), "mask")
        same_words(bd, tile(bd_w), "bottom_diff")


# ---- TanH -----------------------------------------------------------------------------------------------------------
COUNTS = [1, 3, 4, 5, 2 ** 20 + 3, 2 ** 21 + 5]


def tanh_input(n, dtype):
    r = np.random.default_rng(SEED + n)
    x = (r.standard_normal(n) * 3).astype(dtype)
    tiny = np.finfo(dtype).tiny
    special = np.array([0.0, -0.0, 20, -20, tiny / 4, -tiny / 4, tiny, 1e-3, -1e-3, 9, -9], dtype)
    k = min(n, special.size)
    x[:k] = special[:k]
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off"])
@pytest.mark.parametrize("n", COUNTS)
def test_tanh(pool, n, off, dtype):
    x = tanh_input(max(n, 11), dtype)[:n]
    xd = dev(x, off)
    y = pool.tanh_forward(xd, out=empty((n,), xd.dtype, off))
    torch.cuda.synchronize()
    got = host(y)
    want = np.tanh(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want).max()
    assert err <= (TOL if dtype == np.float32 else F64_TOL), err
    # in place: the same words
    inplace = dev(x, off)
    assert pool.tanh_forward(inplace, out=inplace) is inplace
    same_words(inplace, got, "tanh in place")
    # backward: the model's words, in place too
    dy = np.random.default_rng(SEED + 2 * n + 1).standard_normal(n).astype(dtype)
    want = R.tanh_backward(got, dy)
    dyd = dev(dy, off)
    dx = pool.tanh_backward(y, dyd, out=empty((n,), xd.dtype, off))
    same_words(dx, want, "tanh backward")
    assert pool.tanh_backward(y, dyd, out=dyd) is dyd
    same_words(dyd, want, "tanh backward in place")


def test_tanh_mixed_alignment_takes_the_element_path(pool):
    x = tanh_input(1001, np.float32)
    y = pool.tanh_forward(dev(x, 1))                       # source off, destination aligned
    same_words(y, host(pool.tanh_forward(dev(x))), "tanh, mixed alignment")


# ---- the unfused chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,M", [("ave", BP), ("max", BM)], ids=["ave", "max"])
def test_the_unfused_chain_meets_the_fused_calls_model(pool, mname, M):
    """mms_bn_forward_f32 (TEST) -> mms_pool_forward_f32 -> mms_tanh_forward_f32 within TOL of the float64 model of
    mms_bn_pool_tanh_* / mms_bn_maxpool_tanh_* at a tiling shape."""
    from mms_answer_selection_amd import capi
    shape = (4, 3, 8, 8, 4, 4)
    inp = M.conditioned_inputs(shape, np.float32, SEED)
    want = M.model_outputs(inp, (4, 4), np.float64)["test_top"]
    x = dev(inp["x"])
    N, C, H, W = x.shape
    bn_top = torch.empty(N, C, H * W, device="cuda")
    sm, ss = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    capi.bn_forward(x.view(N, C, H * W), dev(inp["scale"]), dev(inp["shift"]), dev(inp["running_mean"]),
                    dev(inp["running_var"]), bn_top, sm, ss, phase=M.TEST)
    pooled = pool.pool_forward(bn_top.view(N, C, H, W), mname, 4, 4)
    top = pool.tanh_forward(pooled, out=pooled)
    torch.cuda.synchronize()
    err = np.abs(host(top).astype(np.float64) - want).max()
    assert err <= TOL * max(1.0, np.abs(want).max()), err
