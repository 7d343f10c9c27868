"""The kernels that run AROUND the layer kernels on every Net iteration, called through the raw C symbols
(include/mms.h): mms_dot_f32 / _f64 (every loss top in GPU mode), mms_split_backward_f32 (every blob with two
consumers), mms_feed_gather_rows_f32 (every batch), and standalone PairRankLoss at the sizes where its grids stop
growing and the grid-stride loops start.

Discipline of every case: outputs start as NaN inside a buffer with 64 guard elements on both sides, which must still
be NaN afterwards; inputs are compared bit for bit with their host copies afterwards.

Grid caps (the first count that takes a second trip of the stride loop is cap * 256 * elements-per-thread + 1):
  split_sum_kernel      2048 blocks      524 288 elements
  feed_gather_kernel    8192 blocks    2 097 152 elements
  pairrank_fwd_kernel   1024 blocks    1 048 576 elements (4 per thread)
  pairrank_bwd_kernel   2048 blocks      524 288 elements
The double PairRankLoss kernels cap at 65 536 blocks (16 777 216 elements): out of reach of a test that takes
seconds (its loss is ONE thread's running sum), so that cap is not exercised here.

No bound in this file is measured: results are exact (integer-valued probes, copies, a fixed association), the dot
accuracy bound is derived below, and the fast loss is held to the 2e-6 of include/mms.h.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from util import assert_bitexact, rng

pytestmark = pytest.mark.gpu

GUARD = 64
INVALID, WORKSPACE = 1, 3                     # include/mms.h: MMS_ERR_INVALID_ARG, MMS_ERR_WORKSPACE


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """`n` NaN elements (`.t`, a view) with GUARD NaN elements before and after them in one allocation."""

    def __init__(self, n, dtype=torch.float32, shape=None):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if shape is not None:
            self.t = self.t.view(shape)
        self.ptr = self.t.data_ptr()

    def load(self, x):
        self.t.copy_(dev(x).view(self.t.shape))
        return self

    def check(self, what):
        h = host(self.buf)
        assert np.isnan(h[:GUARD]).all(), "%s: wrote before its start" % what
        assert np.isnan(h[GUARD + self.n:]).all(), "%s: wrote past its end" % what

    def untouched(self, what):
        assert np.isnan(host(self.buf)).all(), "%s: written although the call refused or had nothing to do" % what


def same_bits(t, x, what):
    """A device tensor still holds exactly the bytes of the host array it was made from."""
    assert host(t).tobytes() == np.ascontiguousarray(x).tobytes(), "%s was modified" % what


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def lib(hiplib):
    return hiplib


# --------------------------------------------------------------------------------------------------------------- #
# mms_dot_f32 / mms_dot_f64
# --------------------------------------------------------------------------------------------------------------- #
DOT = {"f32": (np.float32, torch.float32, "mms_dot_f32", 8, 2.0 ** 23, 2.0 ** -24),
       "f64": (np.float64, torch.float64, "mms_dot_f64", 2 ** 15, 2.0 ** 47, 2.0 ** -53)}


def run_dot(lib, kind, x, y, stream=None, xd=None, yd=None):
    """One call on NaN-initialised guarded output; returns the result as a 1-element host array."""
    npdt, tdt, sym = DOT[kind][:3]
    xd = dev(x) if xd is None else xd
    yd = dev(y) if yd is None else yd
    out = Guarded(1, tdt)
    torch.cuda.synchronize()
    rc = getattr(lib, sym)(x.size, xd.data_ptr(), yd.data_ptr(), out.ptr, stream)
    assert rc == 0, "%s(n=%d) returned %d" % (sym, x.size, rc)
    torch.cuda.synchronize()
    out.check("%s out" % sym)
    same_bits(xd, x, "x")
    same_bits(yd, y, "y")
    return host(out.t).copy()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_dot_exact_probes(kind, lib):
    """Integer-valued operands small enough that every product and every partial sum, in any order and with or
    without FMA contraction, is exact: the result IS the integer dot product."""
    npdt, _, _, amp, limit, _ = DOT[kind]
    r = rng(401)
    for n in (0, 1, 63, 64, 255, 256, 257, 511, 512, 513, 4097, 131071):
        x = r.integers(-amp, amp + 1, n).astype(npdt)
        y = r.integers(-amp, amp + 1, n).astype(npdt)
        xi, yi = x.astype(np.int64), y.astype(np.int64)
        assert int(np.abs(xi * yi).sum()) <= limit and n * amp * amp <= limit      # every partial sum is exact
        got = run_dot(lib, kind, x, y)
        assert got[0] == npdt(int((xi * yi).sum())), "n=%d: %r, want %d" % (n, got[0], int((xi * yi).sum()))
        if n == 0:
            assert bits(got)[0] == 0, "n = 0 writes +0.0"


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_dot_position_probes(kind, lib):
    """One non-zero in x against y = 1..n: a dropped, doubled or misplaced element shows as the wrong multiple of 3."""
    npdt = DOT[kind][0]
    n = 777
    y = np.arange(1, n + 1).astype(npdt)
    for i in (0, 1, 255, 256, 257, 511, 512, 776):
        x = np.zeros(n, npdt)
        x[i] = 3
        assert run_dot(lib, kind, x, y)[0] == 3 * (i + 1), "element %d" % i


def two_product(a, b):
    """Dekker: p + e == a * b exactly for float64 arrays (no overflow or underflow at these magnitudes)."""
    p = a * b
    split = 134217729.0                                                  # 2^27 + 1
    ah = a * split; ah = ah - (ah - a); al = a - ah
    bh = b * split; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dot(x, y):
    """The dot product of two float arrays, exactly summed and rounded once to float64."""
    p, e = two_product(x.astype(np.float64), y.astype(np.float64))
    return math.fsum(itertools.chain(p.tolist(), e.tolist()))


def model_dot(x, y):
    """dot_kernel's shape at the working precision: lane t adds elements t, t + 256, ... then a halving tree."""
    dt = x.dtype.type
    k = -(-x.size // 256)
    p = np.zeros(k * 256, x.dtype)
    p[:x.size] = x * y
    s = np.zeros(256, x.dtype)
    for row in p.reshape(k, 256):
        s = s + row
    o = 128
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o >>= 1
    return dt(s[0])


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_dot_accuracy_determinism_stream_alignment(kind, lib):
    """N(0,1) data at n = 100 003 against the exactly summed dot product.  Each lane adds k = ceil(n/256) rounded
    products and 8 tree levels follow, so |err| <= (k + 9) u sum|x_i y_i| (one u per product, per lane add and per
    level, one more for the second-order terms)."""
    npdt, tdt, sym, _, _, u = DOT[kind]
    n = 100003
    r = rng(402)
    x = r.standard_normal(n).astype(npdt)
    y = r.standard_normal(n).astype(npdt)
    exact = exact_dot(x, y)
    k = -(-n // 256)
    bound = (k + 9) * u * float(np.abs(x.astype(np.float64) * y.astype(np.float64)).sum())
    assert abs(float(model_dot(x, y)) - exact) <= bound, "the bound is not reachable by the kernel's own shape"
    xd, yd = dev(x), dev(y)
    got = run_dot(lib, kind, x, y, xd=xd, yd=yd)
    err = abs(float(got[0]) - exact)
    print("%s: |err| = %.3e, bound %.3e" % (sym, err, bound))
    assert err <= bound, "%s: %r is %.3e from %.17g, bound %.3e" % (sym, got[0], err, exact, bound)
    again = run_dot(lib, kind, x, y, xd=xd, yd=yd)
    assert bits(again)[0] == bits(got)[0], "two calls differ"
    side = torch.cuda.Stream()
    on_side = run_dot(lib, kind, x, y, stream=side.cuda_stream, xd=xd, yd=yd)
    assert bits(on_side)[0] == bits(got)[0], "a non-default stream changes the result"
    # one element past a 16-byte boundary (allocations are at least 256-byte aligned)
    xo = torch.empty(n + 1, dtype=tdt, device="cuda")[1:]
    yo = torch.empty(n + 1, dtype=tdt, device="cuda")[1:]
    xo.copy_(xd)
    yo.copy_(yd)
    assert xd.data_ptr() % 16 == 0 and xo.data_ptr() % 16 == x.itemsize
    assert run_dot(lib, kind, x, y, xd=xo, yd=yo)[0] == got[0], "misaligned inputs change the value"


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_dot_refusals(kind, lib):
    _, tdt, sym = DOT[kind][:3]
    f = getattr(lib, sym)
    x = torch.ones(8, dtype=tdt, device="cuda")
    out = Guarded(1, tdt)
    assert f(-1, x.data_ptr(), x.data_ptr(), out.ptr, None) == INVALID
    assert f(8, x.data_ptr(), x.data_ptr(), None, None) == INVALID
    assert f(8, None, x.data_ptr(), out.ptr, None) == INVALID
    assert f(8, x.data_ptr(), None, out.ptr, None) == INVALID
    torch.cuda.synchronize()
    out.untouched("%s out" % sym)


# --------------------------------------------------------------------------------------------------------------- #
# mms_split_backward_f32
# --------------------------------------------------------------------------------------------------------------- #
STRIDE_COUNT = 2048 * 256 + 257               # first use of split_sum_kernel's stride loop, ragged last block
SPLIT_CASES = ([(ntop, count, False) for count in (257, STRIDE_COUNT) for ntop in (1, 2, 7, 8, 9, 16, 17)]
               + [(9, count, False) for count in (1, 255, 256, 2048 * 256, 2048 * 256 + 1)]
               + [(ntop, count, True) for count in (257, STRIDE_COUNT) for ntop in (9, 17)])


def split_tops(ntop, count):
    r = rng(500 + ntop)
    return [(r.standard_normal(count) * 10.0 ** r.integers(-3, 4)).astype(np.float32) for _ in range(ntop)]


def left_to_right(tops):
    want = tops[0].copy()
    for t in tops[1:]:
        want = want + t
    return want


@pytest.mark.parametrize("ntop,count,in_place", SPLIT_CASES,
                         ids=["%dx%d%s" % (n, c, "-inplace" if p else "") for n, c, p in SPLIT_CASES])
def test_split_backward_order(ntop, count, in_place, lib):
    """((t0 + t1) + t2) + ... in float32, across the chunks of 8 pointers (the second and third launch carry the
    running sum in `bottom_diff`) and across the grid cap; in place on top 0 as SplitLayer::Backward does."""
    tops = split_tops(ntop, count)
    want = left_to_right(tops)
    if ntop >= 3:                             # (one or two tops have one association only)
        assert (bits(left_to_right(tops[::-1])) != bits(want)).any(), "this data would not notice a wrong order"
    out = Guarded(count)
    if in_place:
        out.load(tops[0])
    devs = [out.t if in_place and j == 0 else dev(t) for j, t in enumerate(tops)]
    arr = (C.c_void_p * ntop)(*[d.data_ptr() for d in devs])
    torch.cuda.synchronize()
    assert lib.mms_split_backward_f32(count, ntop, arr, out.ptr, None) == 0
    torch.cuda.synchronize()
    assert_bitexact(host(out.t), want, "ntop=%d count=%d" % (ntop, count))
    out.check("bottom_diff")
    for j, (d, t) in enumerate(zip(devs, tops)):
        if not (in_place and j == 0):
            same_bits(d, t, "top %d" % j)


def test_split_backward_nothing_to_do_and_refusals(lib):
    f = lib.mms_split_backward_f32
    tops = [torch.ones(16, device="cuda") for _ in range(3)]
    arr = (C.c_void_p * 3)(*[t.data_ptr() for t in tops])
    out = Guarded(16)
    assert f(0, 3, arr, out.ptr, None) == 0                              # count = 0: nothing is written
    assert f(-1, 3, arr, out.ptr, None) == INVALID
    assert f(16, 0, arr, out.ptr, None) == INVALID
    assert f(16, 3, None, out.ptr, None) == INVALID
    holed = (C.c_void_p * 3)(tops[0].data_ptr(), None, tops[2].data_ptr())
    assert f(16, 3, holed, out.ptr, None) == INVALID
    torch.cuda.synchronize()
    out.untouched("bottom_diff")


# --------------------------------------------------------------------------------------------------------------- #
# mms_feed_gather_rows_f32: a copy, compared as 32-bit words
# --------------------------------------------------------------------------------------------------------------- #
PLANTED = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff80beef,      # quiet and signalling NaNs with payloads
                    0x80000000, 0x00000001, 0x807fffff, 0x007fffff,      # -0.0 and subnormals
                    0x7f800000, 0xff800000, 0x00000000, 0x3f800000], dtype=np.uint32)
POISON = 0x7fdead00                           # around `src`: a NaN that is in no source row


def feed_source(src_rows, row_elems, seed):
    """Random 32-bit words (so: every class of float) with the PLANTED ones spread over the rows; the device copy
    sits between two poisoned rows, so a row index one off either end would copy poison instead of faulting."""
    r = rng(600 + seed)
    words = r.integers(0, 2 ** 32, (src_rows, row_elems), dtype=np.uint64).astype(np.uint32)
    words[words == POISON] = 0
    flat = words.reshape(-1)
    flat[r.permutation(flat.size)[:min(flat.size, PLANTED.size)]] = PLANTED[:min(flat.size, PLANTED.size)]
    buf = np.full((src_rows + 2, row_elems), POISON, np.uint32)
    buf[1:-1] = words
    d = dev(buf.view(np.int32))
    return words, buf, d, d[1:-1]


def run_feed(lib, rows, row_elems, src_rows, first, perm, seed=0):
    words, buf, dbuf, dsrc = feed_source(src_rows, row_elems, seed)
    dst = Guarded(rows * row_elems)
    dperm = None if perm is None else dev(np.asarray(perm, np.int32))
    torch.cuda.synchronize()
    rc = lib.mms_feed_gather_rows_f32(rows, row_elems, src_rows, dsrc.data_ptr(),
                                      None if dperm is None else dperm.data_ptr(), first, dst.ptr, None)
    assert rc == 0
    torch.cuda.synchronize()
    idx = np.arange(first, first + rows) if perm is None else np.asarray(perm, np.int64)[first:first + rows]
    idx = np.clip(idx, 0, src_rows - 1)       # include/mms.h: an entry outside [0, src_rows) reads the nearest valid row
    got = host(dst.t).view(np.uint32).reshape(rows, row_elems)
    bad = np.argwhere(got != words[idx])
    assert bad.size == 0, "%d words differ, first at row %d col %d: %08x, want %08x" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], words[idx][tuple(bad[0])])
    dst.check("dst")
    same_bits(dbuf, buf.view(np.int32), "src")
    if dperm is not None:
        same_bits(dperm, np.asarray(perm, np.int32), "perm")


FEED_CASES = [(1, 1, 1, 0), (5, 1, 9, 4), (33, 7, 50, 0), (4100, 513, 4200, 100)]


@pytest.mark.parametrize("use_perm", [False, True], ids=["identity", "perm"])
@pytest.mark.parametrize("case", FEED_CASES, ids=["%dx%d-of-%d-from-%d" % c for c in FEED_CASES])
def test_feed_gather_bit_preserving(case, use_perm, lib):
    """row_elems = 1, a batch that ends exactly at src_rows, a permutation that repeats rows, and 2 103 300 elements
    (past the 8192-block cap: the stride loop's second trip)."""
    rows, row_elems, src_rows, first = case
    perm = None
    if use_perm:
        r = rng(650 + rows)
        perm = r.integers(0, src_rows, src_rows) if rows == 33 else r.permutation(src_rows)
        if rows == 33:
            perm[5] = perm[6] = perm[20] = perm[0]
            assert len(set(perm[:33].tolist())) < 33
    if rows == 4100:
        assert rows * row_elems > 8192 * 256 and first + rows == src_rows
    run_feed(lib, rows, row_elems, src_rows, first, perm, seed=rows)


def test_feed_gather_clamps_out_of_range_perm_entries(lib):
    """The Layer never sends such a `perm`; the header promises the nearest valid row, i.e. nothing is read out of
    bounds: -1 and -2^31 read row 0, src_rows and 2^31 - 1 read the last row."""
    src_rows = 9
    perm = [3, -1, -2 ** 31, src_rows, 2 ** 31 - 1, 5, 0, 8, 2]
    run_feed(lib, 9, 7, src_rows, 0, perm, seed=99)


def test_feed_gather_nothing_to_do_and_refusals(lib):
    f = lib.mms_feed_gather_rows_f32
    src = torch.ones(9, 7, device="cuda")
    s = src.data_ptr()
    dst = Guarded(9 * 7)
    assert f(0, 7, 9, s, None, 0, dst.ptr, None) == 0                    # rows = 0: dst untouched
    assert f(0, 7, 9, None, None, 9, None, None) == 0                    # ... and no pointer is needed
    assert f(-1, 7, 9, s, None, 0, dst.ptr, None) == INVALID
    assert f(9, 0, 9, s, None, 0, dst.ptr, None) == INVALID
    assert f(9, -7, 9, s, None, 0, dst.ptr, None) == INVALID
    assert f(9, 7, 0, s, None, 0, dst.ptr, None) == INVALID
    assert f(9, 7, 9, s, None, -1, dst.ptr, None) == INVALID
    assert f(65536, 65536, 65536, s, None, 0, dst.ptr, None) == INVALID   # rows * row_elems > 2^31 - 1
    assert f(9, 7, 9, s, None, 1, dst.ptr, None) == INVALID              # first + rows > src_rows
    assert f(1, 7, 9, s, None, 2 ** 31 - 1, dst.ptr, None) == INVALID    # ... also where the int sum would wrap
    assert f(9, 7, 9, None, None, 0, dst.ptr, None) == INVALID
    assert f(9, 7, 9, s, None, 0, None, None) == INVALID
    torch.cuda.synchronize()
    dst.untouched("dst")


# --------------------------------------------------------------------------------------------------------------- #
# Standalone PairRankLoss at the grid caps
# --------------------------------------------------------------------------------------------------------------- #
CAP_COUNT = 1024 * 256 * 4 + 259              # forward: second trip of the stride loop; backward: third
CAP_MARGIN = 0.5


def pairrank_inputs(N, margin, dtype=np.float32):
    """(a, b, y) of test_gpu_parity.py::test_pairrank, with its four planted rows."""
    r = rng(N + 1)
    a = r.uniform(0, 1, (N, 1)).astype(dtype)
    b = r.uniform(0, 1, (N, 1)).astype(dtype)
    y = (r.uniform(size=(N, 1)) < 0.2).astype(dtype)
    a[0] = b[0]                                                          # similar == 0 exactly
    a[1, 0], b[1, 0], y[1, 0] = 0.25, 0.25 + margin, 1.0                 # tie at the hinge
    a[2, 0], b[2, 0], y[2, 0] = 0.75, 0.25, 0.0                          # (1-y)*similar > 0
    a[3, 0], b[3, 0], y[3, 0] = 0.25, 0.75, 0.0                          # (1-y)*similar < 0
    return a, b, y


def exact_mean(y, ordered, similar):
    o, s, yy = ordered.astype(np.float64), similar.astype(np.float64), y.astype(np.float64)
    return math.fsum((np.maximum(0.0, o) + np.abs((1.0 - yy) * s)).ravel().tolist()) / y.size


@pytest.fixture(scope="module")
def cap_case(oracle):
    """Inputs and every reference of the cap-sized case, computed once; nothing below modifies them."""
    a, b, y = pairrank_inputs(CAP_COUNT, CAP_MARGIN)
    loss_ref, o_ref, s_ref = oracle.pairrank_forward(a, b, y, CAP_MARGIN)
    da_ref, db_ref = oracle.pairrank_backward(y, o_ref, s_ref, top_diff=2.0)
    exact = exact_mean(y, o_ref, s_ref)
    # the two sums are only told apart where the reference's running sum has visibly drifted
    assert abs(float(loss_ref) - exact) > 1e-5 * max(1.0, abs(exact)), (loss_ref, exact)
    return dict(a=a, b=b, y=y, loss_ref=np.float32(loss_ref), o_ref=o_ref, s_ref=s_ref, da_ref=da_ref, db_ref=db_ref,
                exact=exact)


def cap_forward(capi, c):
    N = CAP_COUNT
    ad, bd, yd = dev(c["a"]), dev(c["b"]), dev(c["y"])
    o, s, loss = Guarded(N, shape=(N, 1)), Guarded(N, shape=(N, 1)), Guarded(1)
    capi.pairrank_forward(ad, bd, yd, o.t, s.t, loss.t, margin=CAP_MARGIN)
    torch.cuda.synchronize()
    assert_bitexact(host(o.t), c["o_ref"], "ordered_diff_")
    assert_bitexact(host(s.t), c["s_ref"], "similar_diff_")
    for g, what in ((o, "ordered"), (s, "similar"), (loss, "loss")):
        g.check(what)
    for d, k in ((ad, "a"), (bd, "b"), (yd, "y")):
        same_bits(d, c[k], k)
    return host(loss.t).copy()


def test_pairrank_forward_past_the_grid_cap(cap_case, lib):
    """count = 1 048 835: pairrank_fwd_kernel's 1024 blocks take a second trip.  The fast loss is held to the
    header's 2e-6 of the float64 mean of the bit-exact terms -- not to the oracle's running sum, which at this
    length is itself more than 1e-5 away from that mean (asserted in the fixture)."""
    from mms_answer_selection_amd import capi
    assert lib.mms_get_loss_sum_mode() == 0                              # MMS_LOSS_SUM_FAST, the default
    loss = cap_forward(capi, cap_case)
    exact = cap_case["exact"]
    err = abs(float(loss[0]) - exact)
    print("fast loss %r, exact mean %.17g, |err| %.3e, oracle's running sum %r" % (loss[0], exact, err, cap_case["loss_ref"]))
    assert err <= 2e-6 * max(1.0, abs(exact))


def test_pairrank_reference_loss_sum_past_the_grid_cap(cap_case, lib):
    """MMS_LOSS_SUM_REFERENCE at 257 chunks of loss_running_sum_kernel: the oracle's bits, drift and all."""
    from mms_answer_selection_amd import capi
    capi.set_loss_sum_mode("reference")
    try:
        loss = cap_forward(capi, cap_case)
    finally:
        capi.set_loss_sum_mode("fast")
    assert -(-CAP_COUNT // 4096) == 257
    assert_bitexact(loss, np.array([cap_case["loss_ref"]], np.float32), "loss, reference sum")


@pytest.mark.parametrize("propagate_down", [(True, True), (False, True)], ids=["both", "only-b"])
def test_pairrank_backward_past_the_grid_cap(propagate_down, cap_case, lib):
    """pairrank_bwd_kernel's 2048 blocks cover 524 288 elements per trip: this count takes three."""
    from mms_answer_selection_amd import capi
    c, N = cap_case, CAP_COUNT
    yd, od, sd = dev(c["y"]), dev(c["o_ref"]), dev(c["s_ref"])
    ga, gb = Guarded(N, shape=(N, 1)), Guarded(N, shape=(N, 1))
    capi.pairrank_backward(yd, od, sd, ga.t, gb.t, top_diff=2.0, propagate_down=propagate_down)
    torch.cuda.synchronize()
    if propagate_down[0]:
        assert_bitexact(host(ga.t), c["da_ref"], "da")
        ga.check("da")
    else:
        ga.untouched("da without propagate_down[0]")
    assert_bitexact(host(gb.t), c["db_ref"], "db")
    gb.check("db")
    for d, k in ((yd, "y"), (od, "o_ref"), (sd, "s_ref")):
        same_bits(d, c[k], k)


def test_pairrank_workspace_contract(oracle, lib):
    """count = 8193, the first count of the multi-block forward, through the raw symbol: without its workspace, or
    with one byte too few, the call returns MMS_ERR_WORKSPACE before it launches anything; the size the query
    reports is enough, and no byte past it is written."""
    N, margin = 8193, 0.5
    a, b, y = pairrank_inputs(N, margin)
    loss_ref, o_ref, s_ref = oracle.pairrank_forward(a, b, y, margin)
    need = lib.mms_pairrank_workspace_bytes(N)
    assert need > 0
    ad, bd, yd = dev(a), dev(b), dev(y)
    o, s, loss = Guarded(N), Guarded(N), Guarded(1)
    ws = torch.full((need + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    args = (N, margin, ad.data_ptr(), bd.data_ptr(), yd.data_ptr(), o.ptr, s.ptr, loss.ptr)
    assert lib.mms_pairrank_forward_f32(*args, None, 0, None) == WORKSPACE
    assert lib.mms_pairrank_forward_f32(*args, None, need, None) == WORKSPACE
    assert lib.mms_pairrank_forward_f32(*args, ws.data_ptr(), need - 1, None) == WORKSPACE
    torch.cuda.synchronize()
    for g, what in ((o, "ordered"), (s, "similar"), (loss, "loss")):
        g.untouched(what)
    assert (host(ws) == 0xAB).all(), "a refused call wrote its workspace"
    assert lib.mms_pairrank_forward_f32(*args, ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert_bitexact(host(o.t), o_ref.ravel(), "ordered_diff_")
    assert_bitexact(host(s.t), s_ref.ravel(), "similar_diff_")
    exact = exact_mean(y, o_ref, s_ref)
    assert abs(float(host(loss.t)[0]) - exact) <= 2e-6 * max(1.0, abs(exact))
    for g, what in ((o, "ordered"), (s, "similar"), (loss, "loss")):
        g.check(what)
    assert (host(ws)[need:] == 0xAB).all(), "wrote past the workspace size the query reports"
    for d, x, k in ((ad, a, "a"), (bd, b, "b"), (yd, y, "y")):
        same_bits(d, x, k)


@pytest.mark.parametrize("count", [8193, 100003])
def test_pairrank_f64_bitexact_including_loss(count, oracle, lib):
    """tests/test_gpu_f64.py's check beyond 4096: several blocks of the element kernels, and the one-thread running
    sum of the loss over a length at which a reordered sum would not have the same bits."""
    from mms_answer_selection_amd import capi
    r = np.random.default_rng(count)
    a = r.standard_normal((count, 1))
    b = r.standard_normal((count, 1))
    y = (r.uniform(size=(count, 1)) < 0.7).astype(np.float64)
    loss_ref, o_ref, s_ref = oracle.pairrank_forward(a, b, y, 0.3)
    da_ref, db_ref = oracle.pairrank_backward(y, o_ref, s_ref, top_diff=1.5)
    ad, bd, yd = dev(a), dev(b), dev(y)
    f64 = torch.float64
    o, s, loss = Guarded(count, f64, (count, 1)), Guarded(count, f64, (count, 1)), Guarded(1, f64)
    capi.pairrank_forward_f64(ad, bd, yd, o.t, s.t, loss.t, margin=0.3)
    torch.cuda.synchronize()
    assert (bits(host(o.t)) == bits(o_ref)).all() and (bits(host(s.t)) == bits(s_ref)).all()
    assert bits(host(loss.t))[0] == bits(np.array([loss_ref]))[0], "the sequential sum is reproduced"
    da, db = Guarded(count, f64, (count, 1)), Guarded(count, f64, (count, 1))
    capi.pairrank_backward_f64(y=yd, ordered=o.t, similar=s.t, da=da.t, db=db.t, top_diff=1.5)
    torch.cuda.synchronize()
    assert (bits(host(da.t)) == bits(da_ref)).all() and (bits(host(db.t)) == bits(db_ref)).all()
    for g, what in ((o, "ordered"), (s, "similar"), (loss, "loss"), (da, "da"), (db, "db")):
        g.check(what)
    for d, x, k in ((ad, a, "a"), (bd, b, "b"), (yd, y, "y")):
        same_bits(d, x, k)
