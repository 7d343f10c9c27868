"""GPU suite: the Dropout calls (include/mms_dropout.h, mms_answer_selection_amd/dropout.py) equal the numpy model
tests/dropout_reference.py word for word -- forward, backward and mask, float and double, on the vector path and on the
ragged one, for every phase of the offset and every misalignment of the arrays, with nothing written beside the output.

Every comparison is of words (view(int32) / view(int64)), so -0 is told from +0.  One thing has no word: the NaN of a
DROPPED Inf or NaN, which is Inf * 0 or NaN * 0: its sign and payload are the multiplier's (x86, where the model runs,
and the GPU differ, and neither the reference nor IEEE 754 pins them).  At exactly those elements -- the model says
which: not kept, input not finite -- the library's result must be a NaN, of any word.  Everywhere else, a KEPT NaN
(NaN * 1 * scale, which carries the input's word through) included, the result must be the model's exact word; and two
results of the library are compared word for word with no exception.

The model's words are computed once per (seed, sequence) and shared; every call of a sweep is checked on the device and
the verdicts are read back together."""
import numpy as np
import pytest
import torch

import dropout_reference as R

pytestmark = pytest.mark.gpu

SEED, SEQUENCE = 0x1234567890ABCDEF, 0x0FEDCBA987654321
NP = {torch.float32: np.float32, torch.float64: np.float64}
INT = {torch.float32: torch.int32, torch.float64: torch.int64}
GUARD = 12345.0
FRONT = 4                                  # guard elements in front of an output view, before its misalignment


@pytest.fixture(scope="module")
def D(hiplib):
    from mms_answer_selection_amd import dropout
    dropout.lib()
    return dropout


@pytest.fixture(scope="module")
def past_one_grid(D):
    """past what one trip of the largest grid covers (lanes x groups per trip x 4 elements; forward and backward take
    GROUPS_PER_TRIP groups per trip, the mask writer one): every lane goes round its loop again, the first few with a
    second group in that trip (count % 4 == 1 puts a ragged last group there on the vector path too), the rest without"""
    return D.GROUPS_PER_TRIP * D.MAX_BLOCKS * D.THREADS * 4 + D.MAX_BLOCKS * D.THREADS * 4 + 5


@pytest.fixture(scope="module")
def model_words(past_one_grid):
    """word(g) for g = 0 .. past_one_grid + 3 under (SEED, SEQUENCE): every sweep below slices it, none changes it"""
    w = R.words(SEED, SEQUENCE, 0, past_one_grid + 4)
    w.setflags(write=False)
    return w


def values(n, dtype):
    """n inputs: +-0, negatives, +-Inf and NaN among the first eight and every 13th after, the rest normal"""
    r = np.random.default_rng(1701)
    x = r.standard_normal(n).astype(dtype)
    special = np.array([1.5, -0.0, 0.0, -2.0, np.inf, -np.inf, np.nan, 3.0], dtype=dtype)
    x[:min(n, 8)] = special[:min(n, 8)]
    tail = np.arange(8, n, 13)
    x[tail] = special[(tail // 13) % 8]
    return x


def model_apply(x, keep, ratio):
    _, scale = R.threshold(ratio, x.dtype)
    with np.errstate(invalid="ignore"):
        return (x * keep.astype(x.dtype)) * scale


def free_nan(x, keep):
    """where a result is a NaN without a pinned word: a dropped Inf or NaN"""
    return ~keep & ~np.isfinite(x)


def same_words(got, want):
    """two device tensors, word for word"""
    return torch.equal(got.view(INT[got.dtype]), want.view(INT[want.dtype]))


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025]


class Sweep:
    """calls whose verdicts are read back at the end, in one transfer"""

    def __init__(self):
        self.cases, self.flags = [], []

    def add(self, case, *conds):
        self.cases.append(case)
        self.flags.append(torch.stack([c if isinstance(c, torch.Tensor) else torch.tensor(c, device="cuda")
                                       for c in conds]).all())

    def finish(self):
        flags = torch.stack(self.flags).cpu().numpy()
        bad = [c for c, f in zip(self.cases, flags) if not f]
        assert not bad, "%d of %d cases differ, the first: %s" % (len(bad), len(flags), bad[:8])
        return len(flags)


def eq(got, want, free):
    """got equals the model's want word for word but where `free` (free_nan), where it must be a NaN"""
    return ((got.view(INT[got.dtype]) == want.view(INT[want.dtype])) | free).all() & (torch.isnan(got) | ~free).all()


def out_view(n, b, dtype):
    """a guard-filled buffer and its view of n elements at element misalignment b"""
    buf = torch.full((FRONT + 3 + n + FRONT,), GUARD, dtype=dtype, device="cuda")
    return buf, buf[FRONT + b:FRONT + b + n]


def guards_intact(buf, b, n):
    return ((buf[:FRONT + b] == GUARD).all() & (buf[FRONT + b + n:] == GUARD).all())


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("ratio", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_equals_the_model_on_every_path(D, model_words, past_one_grid, dtype, ratio, direction):
    """every count x every offset % 4 x every misalignment of x and of y (views into larger buffers): the vector
    path is (offset % 4, x, y) = (0, aligned, aligned), everything else the ragged one; guards around y untouched"""
    call = getattr(D, "dropout_" + direction)
    nmax = past_one_grid
    x_host = values(nmax, NP[dtype])
    thr, _ = R.threshold(ratio, NP[dtype])
    xs = []
    for a in range(4):                                              # the same values at four misalignments
        buf = torch.empty(nmax + 4, dtype=dtype, device="cuda")
        buf[a:a + nmax] = upload(x_host)
        xs.append(buf[a:a + nmax])
    sweep = Sweep()
    for o in range(4):
        offset = 4 * 1000003 + o                                    # not a prefix of the index space either
        keep = R.words(SEED, SEQUENCE, offset, 1025) > np.uint32(thr)
        want, free = upload(model_apply(x_host[:1025], keep, ratio)), upload(free_nan(x_host[:1025], keep))
        for n in COUNTS:
            for a in range(4):
                for b in range(4):
                    buf, y = out_view(n, b, dtype)
                    got = call(xs[a][:n], ratio, SEED, SEQUENCE, offset=offset, out=y)
                    assert got is y
                    sweep.add((n, o, a, b), eq(y, want[:n], free[:n]), guards_intact(buf, b, n))
        # past one pass of the largest grid, from the words shared by the module
        keep = model_words[o:o + nmax] > np.uint32(thr)
        want, free = upload(model_apply(x_host, keep, ratio)), upload(free_nan(x_host, keep))
        for a, b in ((0, 0), (o, 0), (0, o), (1, 3), (2, 2)):
            buf, y = out_view(nmax, b, dtype)
            call(xs[a], ratio, SEED, SEQUENCE, offset=o, out=y)
            sweep.add((nmax, o, a, b), eq(y, want, free), guards_intact(buf, b, nmax))
    assert sweep.finish() == 4 * (len(COUNTS) * 16 + 5)


@pytest.mark.parametrize("ratio", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["thr-f32", "thr-f64"])
def test_mask_equals_the_model_on_every_path(D, model_words, past_one_grid, dtype, ratio):
    thr, _ = R.threshold(ratio, NP[dtype])
    nmax = past_one_grid
    sweep = Sweep()
    for o in range(4):
        offset = 4 * 1000003 + o
        want = upload((R.words(SEED, SEQUENCE, offset, 1025) > np.uint32(thr)).astype(np.int32))
        for n in COUNTS:
            for b in range(4):
                buf, m = out_view(n, b, torch.int32)
                got = D.dropout_mask(n, ratio, SEED, SEQUENCE, offset=offset, dtype=dtype, out=m)
                assert got is m
                sweep.add((n, o, b), (m == want[:n]).all(), guards_intact(buf, b, n))
        want = upload((model_words[o:o + nmax] > np.uint32(thr)).astype(np.int32))
        for b in (0, 1, 2, 3):
            buf, m = out_view(nmax, b, torch.int32)
            D.dropout_mask(nmax, ratio, SEED, SEQUENCE, offset=o, dtype=dtype, out=m)
            sweep.add((nmax, o, b), (m == want).all(), guards_intact(buf, b, nmax))
    assert sweep.finish() == 4 * (len(COUNTS) * 4 + 4)
    # the allocating form, by count and by shape
    m = D.dropout_mask((5, 7), ratio, SEED, SEQUENCE, dtype=dtype)
    assert m.dtype == torch.int32 and tuple(m.shape) == (5, 7) and m.is_cuda
    assert (m.cpu().numpy().reshape(-1) == R.mask(35, ratio, SEED, SEQUENCE, dtype=NP[dtype]).astype(np.int32)).all()
    assert torch.equal(D.dropout_mask(35, ratio, SEED, SEQUENCE, dtype=dtype), m.reshape(-1))


def test_the_two_thresholds_give_two_masks(D):
    """float(UINT_MAX) is 2^32, double(UINT_MAX) is not: at ratio 0.5 the word 2^31 itself is dropped by the float
    threshold (2^31) and kept by the double one (2^31 - 1).  The model says which mask is which; the calls agree with it
    over 2^20 words (whether or not that word occurs among them)."""
    n = 1 << 20
    for dtype in (torch.float32, torch.float64):
        got = D.dropout_mask(n, 0.5, 3, 4, dtype=dtype).cpu().numpy()
        assert (got == R.mask(n, 0.5, 3, 4, dtype=NP[dtype]).astype(np.int32)).all()
    assert R.threshold(0.5, np.float32)[0] == 1 << 31 and R.threshold(0.5, np.float64)[0] == (1 << 31) - 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_special_values_word_for_word(D, dtype):
    """-0 from a dropped negative, +0 from a dropped positive, NaN from a dropped Inf or NaN, the kept ones scaled"""
    x_host = np.array([1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, -3.0] * 16, dtype=NP[dtype])
    keep = R.mask(x_host.size, 0.5, 21, 22, dtype=NP[dtype]).astype(bool)
    y = D.dropout_forward(upload(x_host), 0.5, 21, 22).cpu().numpy()
    for v in (1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, -3.0):
        sel = (x_host == v) & (np.signbit(x_host) == np.signbit(NP[dtype](v)))
        assert (sel & keep).any() and (sel & ~keep).any(), v                      # both cases are seen
        assert (y[sel & keep] == NP[dtype](v) * 2).all(), v
        if np.isinf(v):
            assert np.isnan(y[sel & ~keep]).all(), v
        else:
            assert (y[sel & ~keep] == 0).all() and (np.signbit(y[sel & ~keep]) == (v < 0 or np.signbit(v))).all(), v
    assert np.isnan(y[np.isnan(x_host)]).all()
    kept_nan = np.isnan(x_host) & keep                                            # NaN * 1 * scale: the input's word
    IT = np.int32 if dtype == torch.float32 else np.int64
    assert kept_nan.any() and (~keep & np.isnan(x_host)).any()
    assert (y[kept_nan].view(IT) == R.forward(x_host, 0.5, 21, 22)[kept_nan].view(IT)).all()
    assert (y[kept_nan].view(IT) == x_host[kept_nan].view(IT)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_in_place_and_test_phase(D, dtype):
    n = 1027
    x_host = values(n, NP[dtype])
    for a in (0, 1):                                                # the vector path and the ragged one
        x = torch.empty(n + 4, dtype=dtype, device="cuda")[a:a + n].copy_(upload(x_host))
        for fn in (D.dropout_forward, D.dropout_backward):
            apart = fn(x, 0.1, SEED, SEQUENCE, offset=8)
            assert same_words(x, upload(x_host))                    # the input of an out-of-place call is not written
            inplace = x.clone() if a == 0 else torch.empty(n + 4, dtype=dtype, device="cuda")[a:a + n].copy_(x)
            assert fn(inplace, 0.1, SEED, SEQUENCE, offset=8, out=inplace) is inplace
            assert same_words(inplace, apart)
            # TEST: a copy, whatever the seed; in place nothing at all
            buf, y = out_view(n, a, dtype)
            fn(x, 0.1, SEED, SEQUENCE, offset=8, train=False, out=y)
            assert same_words(y, x) and bool(guards_intact(buf, a, n))
            fn(x, 0.1, SEED, SEQUENCE, train=False, out=x)
            assert same_words(x, upload(x_host))


def test_counter_carry_and_the_other_words_of_the_key(D):
    """offset 2^34 - 2 with count 8: the group index crosses 2^32, so ctr[0] wraps and ctr[1] becomes 1.  And a mask
    depends on the seed and on the sequence, on the high half of each too."""
    offset = 2 ** 34 - 2
    x_host = np.arange(1, 9, dtype=np.float32)
    for o in (offset, offset + 1, 2 ** 63 + 5, 2 ** 64 - 9):
        for ratio in (0.1, 0.5):
            y = D.dropout_forward(upload(x_host), ratio, SEED, SEQUENCE, offset=o).cpu().numpy()
            assert (y.view(np.int32) == R.forward(x_host, ratio, SEED, SEQUENCE, offset=o).view(np.int32)).all(), (o, ratio)
            m = D.dropout_mask(8, ratio, SEED, SEQUENCE, offset=o).cpu().numpy()
            assert (m == R.mask(8, ratio, SEED, SEQUENCE, offset=o).astype(np.int32)).all(), (o, ratio)
    n = 4096
    base = D.dropout_mask(n, 0.5, SEED, SEQUENCE).cpu().numpy()
    for seed, sequence in ((SEED + 1, SEQUENCE), (SEED, SEQUENCE + 1), (SEED ^ (1 << 63), SEQUENCE),
                           (SEED, SEQUENCE ^ (1 << 63)), (SEQUENCE, SEED)):
        other = D.dropout_mask(n, 0.5, seed, sequence).cpu().numpy()
        assert (other == R.mask(n, 0.5, seed, sequence).astype(np.int32)).all(), (seed, sequence)
        assert 0.4 * n < (other != base).sum() < 0.6 * n, (seed, sequence)       # independent masks differ in half


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_sharding(D, dtype):
    """two calls on the two parts of a buffer, the second with offset = the first part's length, for a split point at
    every phase: the words of one call on the whole"""
    n = 2051
    x = upload(values(n, NP[dtype]))
    for base in (0, 7):                                             # the whole itself at a phase too
        whole = D.dropout_forward(x, 0.1, SEED, SEQUENCE, offset=base)
        whole_mask = D.dropout_mask(n, 0.1, SEED, SEQUENCE, offset=base, dtype=dtype)
        for split in (1024, 1025, 1026, 1027):
            y = torch.empty_like(x)
            D.dropout_forward(x[:split], 0.1, SEED, SEQUENCE, offset=base, out=y[:split])
            D.dropout_forward(x[split:], 0.1, SEED, SEQUENCE, offset=base + split, out=y[split:])
            assert same_words(y, whole), (base, split)
            m = torch.empty_like(whole_mask)
            D.dropout_mask(split, 0.1, SEED, SEQUENCE, offset=base, dtype=dtype, out=m[:split])
            D.dropout_mask(n - split, 0.1, SEED, SEQUENCE, offset=base + split, dtype=dtype, out=m[split:])
            assert torch.equal(m, whole_mask), (base, split)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_backward_regenerates_the_forwards_mask(D, dtype):
    n = 5003
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(n, dtype=dtype, device="cuda", generator=gen) + 0.5          # no zeros
    dy = torch.randn(n, dtype=dtype, device="cuda", generator=gen)
    for ratio in (0.1, 0.5):
        for offset in (0, 3):
            y = D.dropout_forward(x, ratio, SEED, SEQUENCE, offset=offset)
            mask = D.dropout_mask(n, ratio, SEED, SEQUENCE, offset=offset, dtype=dtype)
            assert torch.equal(mask != 0, y != 0)
            assert 0 < int(mask.sum()) < n
            _, scale = D.dropout_threshold(ratio, dtype)
            dx = D.dropout_backward(dy, ratio, SEED, SEQUENCE, offset=offset)
            assert same_words(dx, (dy * mask.to(dtype)) * torch.tensor(scale, dtype=dtype, device="cuda"))
            # another sequence is another mask: the host must pass the forward's
            assert not same_words(D.dropout_backward(dy, ratio, SEED, SEQUENCE + 1, offset=offset), dx)


def test_the_heads_mask_drawn_by_the_library(D):
    """mms_head_forward_f32 / _backward_f32 in TRAIN with the mask dropout_mask draws equal, word for word, the same
    calls given the model's mask uploaded from numpy"""
    from mms_answer_selection_amd import head
    N, F0, F1, H, C_ = 5, 7, 3, 32, 2
    r = np.random.default_rng(5)
    f = lambda *s: upload((r.standard_normal(s) * 0.5).astype(np.float32))
    x0, x1, w1, b1, w2, b2 = f(N, F0), f(N, F1), f(H, F0 + F1), f(H), f(C_, H), f(C_)
    label = upload(r.integers(0, C_, N).astype(np.float32))
    drawn = D.dropout_mask((N, H), 0.5, SEED, 77)
    model = upload(R.mask(N * H, 0.5, SEED, 77).astype(np.int32).reshape(N, H))
    assert torch.equal(drawn, model) and 0 < int(drawn.sum()) < N * H
    results = []
    for mask in (drawn, model):
        h, prob, loss = head.head_forward(x0, x1, w1, b1, mask, w2, b2, label)
        diffs = [torch.zeros_like(t) for t in (x0, x1, w1, b1, w2, b2)]
        head.head_backward(x0, x1, w1, w2, mask, h, prob, label, 1.0, *diffs)
        results.append([h, prob, loss] + diffs)
    for got, want in zip(*results):
        assert same_words(got, want)
    assert bool(torch.isfinite(results[0][2]).all())


def test_determinism(D):
    n = 100003
    x = upload(values(n, np.float32))
    first = D.dropout_forward(x, 0.1, SEED, SEQUENCE, offset=2)
    assert same_words(D.dropout_forward(x, 0.1, SEED, SEQUENCE, offset=2), first)
    assert torch.equal(D.dropout_mask(n, 0.1, SEED, SEQUENCE, offset=2), D.dropout_mask(n, 0.1, SEED, SEQUENCE, offset=2))
    assert same_words(D.dropout_backward(x, 0.1, SEED, SEQUENCE, offset=2), first)       # the same map


def test_binding_refusals_on_device_tensors(D):
    from mms_answer_selection_amd import capi
    x = torch.zeros(8, 8, device="cuda")
    with pytest.raises(capi.MMSError):
        D.dropout_forward(x.t(), 0.5, 1, 2)                                               # not contiguous
    with pytest.raises(capi.MMSError):
        D.dropout_forward(x, 0.5, 1, 2, out=torch.zeros(8, 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(capi.MMSError):
        D.dropout_forward(x, 1.0, 1, 2)                                                   # the library's refusal
    with pytest.raises(capi.MMSError):
        D.dropout_forward(x.reshape(-1)[:32], 0.5, 1, 2, out=x.reshape(-1)[1:33])         # partial overlap
    with pytest.raises(capi.MMSError):
        D.dropout_mask(4, 0.5, 1, 2, out=torch.zeros(4, device="cuda"))                   # not int32
    assert D.dropout_forward(torch.zeros(0, device="cuda"), 0.5, 1, 2).numel() == 0
