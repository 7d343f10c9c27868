"""The ordered scatter-add of the Embed backward at every segment length (mms_embed_backward_f32, _pair_f32,
_pair_indexed_f32, mms_embed_backward_f64): weight_diff against the oracle bit for bit, on inputs whose bits depend on
the order of the additions (tests/embed_segments.py; the conditions on them are asserted in
tests/test_embed_segments.py), bias_diff against an fp64 column sum and, on dyadic data, against the exact sum bit for
bit; then the edges of the call: ids that are clamped or truncated, the sort's bit counts, one row, one destination,
all-distinct ids."""
import numpy as np
import pytest
import torch

import embed_segments as es
from util import TOL, assert_bitexact, assert_close

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
VARIANTS = ["both", "weight_only", "bias_only"]


def dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()    # a copy: the cases are read-only


def offset_view(a):
    """A contiguous device copy of the float64 array `a` that starts 8 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 3, dtype=torch.float64, device="cuda")
    skip = 1 if buf.data_ptr() % 16 == 0 else 2
    v = buf[skip:skip + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(np.array(a, order="C")))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def words(x):
    x = np.ascontiguousarray(x)
    return x.view("u%d" % x.dtype.itemsize)


def same_words(got, ref, what):
    g, r = words(got).ravel(), words(ref).ravel()
    bad = np.flatnonzero(g != r)
    if bad.size:                                      # NaN must meet NaN; payloads may differ
        gn, rn = np.asarray(got).ravel()[bad], np.asarray(ref).ravel()[bad]
        still = ~(np.isnan(gn) & np.isnan(rn))
        assert not still.any(), "%s: %d of %d words differ, first at %d: %r vs %r" % (
            what, int(still.sum()), g.size, int(bad[still][0]), gn[still][0], rn[still][0])


def weight_diff_matches(got, ref, index, what):
    """Bit equality; a mismatch names the segment length and the 64-column slice of the first differing word, which
    say which branch of csrc/embed.hip produced it."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    bad = np.argwhere(words(got) != words(ref))
    if bad.size:
        seg = es.segment_lengths(index)
        rows = sorted({int(b[0]) for b in bad})
        print("%s: %d words differ in %d rows; first: id %d (segment of %d rows), column %d (slice %d); segment "
              "lengths of the differing rows: %s" % (what, len(bad), len(rows), bad[0][0], seg.get(int(bad[0][0]), 0),
                                                     bad[0][1], bad[0][1] // 64, sorted({seg.get(i, 0) for i in rows})))
    if got.dtype == F:
        assert_bitexact(got, ref, what)
    else:
        same_words(got, ref, what)


def bias_sum(top_diff, bd0):
    """bias_diff's reference: the fp64 column sum on top of the start value"""
    return bd0.astype(D) + top_diff.astype(D).sum(axis=0)


def bias_diff_matches(got, ref, what):
    err = np.abs(got.astype(D) - ref).max()
    if got.dtype == F:
        print("%s: max abs err %.3e (bound %.3e)" % (what, err, TOL * max(1.0, np.abs(ref).max())))
        assert_close(got, ref, TOL, what)
    else:
        print("%s: max abs err %.3e (bound %.3e)" % (what, err, 1e-12 * max(1.0, np.abs(ref).max())))
        assert err <= 1e-12 * max(1.0, np.abs(ref).max()), what


@pytest.fixture(scope="module")
def capi(hiplib):
    from mms_answer_selection_amd import capi
    return capi


def backward(capi, index, top_diff, wd0, bd0, which="both", cut=None, top_diff_dev=None):
    """One backward call of the library on fresh device copies -> (weight_diff, bias_diff) as numpy, None where the
    variant leaves it out.  `index` holds the ids as the call's element type; `cut`: the pair call, layers [0, cut) and
    [cut, M)."""
    dtype = top_diff.dtype
    wd = dev(wd0) if which != "bias_only" else None
    bd = dev(bd0) if which != "weight_only" else None
    dT = top_diff_dev if top_diff_dev is not None else dev(top_diff)
    if cut is not None:
        assert dtype == F
        capi.embed_backward_pair(dev(index[:cut]), dev(index[cut:]), dT[:cut], dT[cut:], wd, bias_diff=bd, shape=wd0.shape)
    elif dtype == F:
        capi.embed_backward(dev(index), dT, wd, bd, shape=wd0.shape)
    else:
        capi.embed_backward_f64(dev(index), dT, wd, bd, shape=wd0.shape)
    return (None if wd is None else wd.cpu().numpy()), (None if bd is None else bd.cpu().numpy())


# ------------------------------------------------------------------ planted segment lengths
@pytest.fixture(scope="module")
def reference(oracle):
    """name -> the case with the oracle's weight_diff ("wd": one layer; "wd_pair": layer 0's Backward, then layer
    1's) and the fp64 bias sum, computed once per case and left unchanged."""
    done = {}

    def get(name):
        if name not in done:
            c = dict(es.make_case(name))
            idx = c["index"].astype(c["dtype"])
            c["idx"] = idx
            c["wd"], _ = oracle.embed_backward(idx, c["top_diff"], c["wd0"], c["bd0"])
            if c["dtype"] == F:
                M0 = es.PAIR_CUT
                wd_a, _ = oracle.embed_backward(idx[:M0], c["top_diff"][:M0], c["wd0"])
                c["wd_pair"], _ = oracle.embed_backward(idx[M0:], c["top_diff"][M0:], wd_a)
            c["bd"] = bias_sum(c["top_diff"], c["bd0"])
            print("%s (CH = %d): segments per length class %s" % (
                name, es.seg_chunk(c["dtype"]), es.class_histogram(c["index"], es.seg_chunk(c["dtype"]))))
            done[name] = c
        return done[name]
    return get


def check_outputs(c, wd, bd, wd_ref, what):
    if wd is not None:
        weight_diff_matches(wd, wd_ref, c["index"], what + ": weight_diff (n-ascending sums)")
    if bd is not None:
        bias_diff_matches(bd, c["bd"], what + ": bias_diff")


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", es.FLOAT_CASES)
def test_backward_f32(reference, capi, name, which):
    c = reference(name)
    wd, bd = backward(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which)
    check_outputs(c, wd, bd, c["wd"], name)


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", es.FLOAT_CASES)
def test_backward_pair_f32(reference, capi, name, which):
    """Two layers over one table, cut at row 1777: layer 0's rows ascending, then layer 1's, into the same diffs."""
    c = reference(name)
    M0 = es.PAIR_CUT
    assert es.straddlers(c["index"], c["planted"], M0)               # a segment's chain crosses from layer 0 to layer 1
    wd, bd = backward(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which, cut=M0)
    check_outputs(c, wd, bd, c["wd_pair"], name + " pair")
    # ... and equals the two single-layer calls of this library
    wd2 = dev(c["wd0"]) if wd is not None else None
    bd2 = dev(c["bd0"]) if bd is not None else None
    dT = dev(c["top_diff"])
    capi.embed_backward(dev(c["idx"][:M0]), dT[:M0], wd2, bd2, shape=c["wd0"].shape)
    capi.embed_backward(dev(c["idx"][M0:]), dT[M0:], wd2, bd2, shape=c["wd0"].shape)
    if wd is not None:
        weight_diff_matches(wd, wd2.cpu().numpy(), c["index"], name + ": pair == two calls")
    if bd is not None:
        bias_diff_matches(bd2.cpu().numpy(), c["bd"], name + ": bias_diff of the two calls")


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", [n for n in es.FLOAT_CASES if es.CASES[n][1] <= es.PREP_MAX])
def test_backward_pair_indexed_f32(reference, capi, oracle, name, which):
    """The inverted index built beside the pair forward, used twice."""
    c = reference(name)
    M0, M, N = es.PAIR_CUT, c["M"], c["N"]
    r = np.random.default_rng(77)
    weight = r.uniform(-0.08, 0.08, (c["K"], N)).astype(F)
    i0, i1 = dev(c["idx"][:M0]), dev(c["idx"][M0:])
    t0 = torch.full((M0, N), float("nan"), device="cuda")
    t1 = torch.full((M - M0, N), float("nan"), device="cuda")
    index = capi.EmbedPairIndex()
    assert capi.embed_forward_pair(i0, i1, dev(weight), t0, t1, index=index)
    top = oracle.embed_forward(c["idx"], weight)
    assert_bitexact(t0.cpu().numpy(), top[:M0], "top0")
    assert_bitexact(t1.cpu().numpy(), top[M0:], "top1")
    dT = dev(c["top_diff"])
    for use in ("first", "second"):                                 # the index is read-only
        wd = dev(c["wd0"]) if which != "bias_only" else None
        bd = dev(c["bd0"]) if which != "weight_only" else None
        capi.embed_backward_pair_indexed(i0, i1, dT[:M0], dT[M0:], wd, index, bias_diff=bd, shape=c["wd0"].shape)
        check_outputs(c, None if wd is None else wd.cpu().numpy(), None if bd is None else bd.cpu().numpy(),
                      c["wd_pair"], "%s indexed, %s use" % (name, use))


def test_no_index_above_4096_rows(reference, capi):
    c = reference("f32-M4500-N300")
    M0, M, N = es.PAIR_CUT, c["M"], c["N"]
    weight = np.random.default_rng(78).uniform(-0.08, 0.08, (c["K"], N)).astype(F)
    t0, t1 = torch.empty((M0, N), device="cuda"), torch.empty((M - M0, N), device="cuda")
    index = capi.EmbedPairIndex()
    built = capi.embed_forward_pair(dev(c["idx"][:M0]), dev(c["idx"][M0:]), dev(weight), t0, t1, index=index)
    assert built is False
    assert_bitexact(torch.cat([t0, t1]).cpu().numpy(), weight[c["index"]], "the forward itself still runs")
    with pytest.raises(capi.MMSError):
        capi.embed_backward_pair_indexed(dev(c["idx"][:M0]), dev(c["idx"][M0:]), t0, t1, dev(c["wd0"]), index)


@pytest.mark.parametrize("which", VARIANTS + ["top_diff_offset"])
@pytest.mark.parametrize("name", es.DOUBLE_CASES)
def test_backward_f64(reference, capi, name, which):
    c = reference(name)
    off = offset_view(c["top_diff"]) if which == "top_diff_offset" else None    # rows 8 bytes off the 16-byte grid
    wd, bd = backward(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which, top_diff_dev=off)
    check_outputs(c, wd, bd, c["wd"], name)


# ------------------------------------------------------------------ bias_diff, exactly
@pytest.mark.parametrize("with_weight", [False, True], ids=["bias_only", "with_weight_diff"])
@pytest.mark.parametrize("dtype", [F, D], ids=["f32", "f64"])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 1024, 1025, 4096, 4097])
def test_bias_diff_of_dyadic_rows_is_exact(capi, M, dtype, with_weight):
    """top_diff and the start value are multiples of 2^-8 in [-4, 4]: every partial sum of up to 4500 of them is below
    2^15 with 8 fraction bits, 23 bits, exact in fp32 (and fp64) in ANY order.  So bias_diff has one right answer,
    whatever the launch shape (riders of the index build with 16 row lanes, the 4-lane kernel, the final sum as a rider
    or a launch of its own), the 128-row chunks and the eight-at-a-time fold of the partial sums -- no tolerance."""
    K = 600
    for N in (50, 64, 65):
        r = np.random.default_rng(1000 * N + M)
        q = r.integers(-1024, 1025, (M, N))
        b = r.integers(-1024, 1025, N)
        top_diff, bd0 = (q / 256.0).astype(dtype), (b / 256.0).astype(dtype)
        exact = ((b + q.sum(axis=0)) / 256.0).astype(dtype)
        assert np.abs(b + q.sum(axis=0)).max() < 2 ** 23
        index = r.integers(0, K, M).astype(dtype)
        wd0 = r.standard_normal((K, N)).astype(dtype)
        _, bd = backward(capi, index, top_diff, wd0, bd0, "both" if with_weight else "bias_only")
        bad = np.flatnonzero(words(bd) != words(exact))
        assert not bad.size, "M %d N %d: %d columns differ, first %d: %r vs %r" % (
            M, N, bad.size, bad[0], bd[bad[0]], exact[bad[0]])


# ------------------------------------------------------------------ edges of the call
def edge_inputs(index, N, K, dtype, seed):
    """telescoping top_diff and non-zero start values for an arbitrary id vector (ids in [0, K))"""
    top_diff, ids, y0 = es.telescoping_diff(index, N, dtype, seed)
    r = np.random.default_rng(seed + 1)
    wd0 = r.standard_normal((K, N), dtype=dtype)
    wd0[ids] = y0
    return top_diff, wd0, r.standard_normal(N).astype(dtype)


def check_edge(capi, oracle, raw, valid, N, K, dtype, seed, cut=None):
    """The library on the ids `raw` against the oracle on the in-range ids `valid`."""
    top_diff, wd0, bd0 = edge_inputs(valid, N, K, dtype, seed)
    wd_ref, _ = oracle.embed_backward(valid.astype(dtype), top_diff, wd0, bd0)
    wd, bd = backward(capi, raw.astype(dtype), top_diff, wd0, bd0, "both", cut=cut)
    weight_diff_matches(wd, wd_ref, valid, "weight_diff")
    bias_diff_matches(bd, bias_sum(top_diff, bd0), "bias_diff")
    return wd, wd0


def odd_ids(K, M, seed):
    """Ids the reference would DCHECK: the backward must clamp them to the table and truncate them toward zero exactly
    as the forward does (int(id), then [0, K - 1]).  -> (raw, in-range), shuffled among ordinary ids."""
    r = np.random.default_rng(seed)
    raw = np.r_[[-3.0, -0.5, 4.9, K - 0.5, K, K + 5.0, 1e9], r.integers(0, K, M - 7).astype(D)]
    raw = raw[r.permutation(M)]
    return raw, np.clip(np.trunc(raw), 0, K - 1).astype(np.int64)


@pytest.mark.parametrize("dtype,cut", [(F, None), (D, None), (F, 20)], ids=["f32", "f64", "f32-pair"])
def test_backward_clamps_and_truncates_ids_like_the_forward(capi, oracle, dtype, cut):
    K, M, N = 9, 45, 70
    raw, valid = odd_ids(K, M, 31)
    assert valid.min() == 0 and valid.max() == K - 1 and 4 in valid
    if cut is not None:                                            # odd ids in both layers
        assert (raw[:cut] != valid[:cut]).any() and (raw[cut:] != valid[cut:]).any()
    check_edge(capi, oracle, raw, valid, N, K, dtype, 32, cut=cut)


def test_forward_f32_clamps_and_truncates_ids(capi, oracle):
    K, M, N = 9, 45, 70
    raw, valid = odd_ids(K, M, 33)
    r = np.random.default_rng(34)
    weight, bias = r.standard_normal((K, N)).astype(F), r.standard_normal(N).astype(F)
    for b in (None, bias):
        ref = oracle.embed_forward(valid.astype(F), weight, b)
        top = torch.full((M, N), float("nan"), device="cuda")
        capi.embed_forward(dev(raw.astype(F)), dev(weight), top, bias=dev(b))
        assert_bitexact(top.cpu().numpy(), ref, "clamped rows")
        t0, t1 = torch.full((20, N), float("nan"), device="cuda"), torch.full((M - 20, N), float("nan"), device="cuda")
        capi.embed_forward_pair(dev(raw[:20].astype(F)), dev(raw[20:].astype(F)), dev(weight), t0, t1, bias=dev(b))
        assert_bitexact(torch.cat([t0, t1]).cpu().numpy(), ref, "clamped rows, pair forward")


@pytest.mark.parametrize("dtype,cut", [(F, None), (D, None), (F, 100)], ids=["f32", "f64", "f32-pair"])
@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 2 ** 20 + 1])
def test_first_and_last_table_row_at_every_bit_count(capi, oracle, K, dtype, cut):
    """The index sort looks at ceil(log2 K) bits of an id: every row of the batch on id 0 or id K - 1."""
    M, N = 300, 7
    r = np.random.default_rng(40 + K % 1000)
    valid = np.where(r.uniform(size=M) < 0.5, 0, K - 1).astype(np.int64)
    wd, wd0 = check_edge(capi, oracle, valid, valid, N, K, dtype, 41 + K % 1000, cut=cut)
    if K > 257:
        assert (words(wd[1:K - 1]) == words(wd0[1:K - 1])).all(), "a row other than 0 and K - 1 changed"
        assert (words(wd[[0, K - 1]]) != words(wd0[[0, K - 1]])).any(axis=1).all()


@pytest.mark.parametrize("dtype,cut", [(F, None), (D, None), (F, 1)], ids=["f32", "f64", "f32-pair"])
def test_one_row(capi, oracle, dtype, cut):
    M = 1 if cut is None else 2                                    # the pair call needs a row in each layer
    valid = np.full(M, 3, np.int64)
    check_edge(capi, oracle, valid, valid, 70, 5, dtype, 50, cut=cut)


@pytest.mark.parametrize("dtype,cut", [(F, None), (D, None), (F, 333)], ids=["f32", "f64", "f32-pair"])
def test_one_destination(capi, oracle, dtype, cut):
    """Every row on the same id: one segment of 700 rows (more than two chunks), 599 idle workgroups."""
    valid = np.full(700, 17, np.int64)
    check_edge(capi, oracle, valid, valid, 70, 600, dtype, 51, cut=cut)


@pytest.mark.parametrize("dtype,cut", [(F, None), (D, None), (F, 333)], ids=["f32", "f64", "f32-pair"])
def test_all_ids_distinct(capi, oracle, dtype, cut):
    """M = K segments of one row: every workgroup of the grid has one."""
    valid = np.random.default_rng(52).permutation(600).astype(np.int64)
    check_edge(capi, oracle, valid, valid, 70, 600, dtype, 53, cut=cut)
