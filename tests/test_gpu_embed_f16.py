"""The fp16-storage Embed calls (mms_embed_forward_f16, _forward_pair_f16, _backward_f16, _backward_pair_f16,
_backward_pair_indexed_f16).  Backward: weight_diff against the oracle on the widened top_diff bit for bit, on inputs whose
bits depend on the order of the additions (tests/embed_f16_model.py; the conditions on them are asserted in
tests/test_embed_f16_model.py), weight_diff and bias_diff against the _f32 twin on a widened copy bit for bit, bias_diff
against an fp64 column sum and, on dyadic data, against the exact sum.  Forward: the table's words, or the oracle's sum
rounded once.  Then misaligned operands, the edges of the call, the chain with the fp16-storage SimCross, and a graph."""
import numpy as np
import pytest
import torch

import embed_f16_model as em
import embed_segments as es
from util import TOL, assert_close

pytestmark = pytest.mark.gpu
F, D, H = np.float32, np.float64, np.float16
VARIANTS = ["both", "weight_only", "bias_only"]


def dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()    # a copy: the cases are read-only


def host(t):
    return None if t is None else t.cpu().numpy()


def words(x):
    x = np.ascontiguousarray(x)
    return x.view("u%d" % x.dtype.itemsize)


def same_words(got, ref, what, nan_meets_nan=False):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = words(got) != words(ref)
    if nan_meets_nan:                                  # an ADD may quieten a NaN or change its payload
        bad &= ~(np.isnan(got) & np.isnan(ref))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: %r vs %r" % (what, int(bad.sum()), bad.size, at,
                                                                                 got[at], ref[at]))


def weight_diff_matches(got, ref, index, what):
    """Bit equality; a mismatch names the segment length and the 64-column slice of the first differing word, which say
    which branch of csrc/embed.hip produced it."""
    bad = np.argwhere(words(got) != words(ref))
    if bad.size:
        seg = es.segment_lengths(index)
        rows = sorted({int(b[0]) for b in bad})
        print("%s: %d words differ in %d rows; first: id %d (segment of %d rows), column %d (slice %d); segment lengths "
              "of the differing rows: %s" % (what, len(bad), len(rows), bad[0][0], seg.get(int(bad[0][0]), 0), bad[0][1],
                                             bad[0][1] // 64, sorted({seg.get(i, 0) for i in rows})))
    same_words(got, ref, what)


def offset_half(a, past):
    """A contiguous device copy of the half array `a` that starts 2 bytes past a `past`-byte boundary (and, for past = 4,
    not 2 bytes past a 16-byte one): a view into a larger half buffer."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 16, dtype=torch.float16, device="cuda")
    want = 2 if past == 16 else 6
    skip = ((want - buf.data_ptr()) % 16) // 2
    v = buf[skip:skip + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == want and v.data_ptr() % past == 2 and v.is_contiguous()
    return v


def place(a, where):
    return dev(a) if where == "aligned" else offset_half(a, 4 if where == "4+2" else 16)


@pytest.fixture(scope="module")
def capi(hiplib):
    from mms_answer_selection_amd import capi
    return capi


def outputs(wd0, bd0, which):
    return (dev(wd0) if which != "bias_only" else None), (dev(bd0) if which != "weight_only" else None)


def backward16(capi, idx, top_diff, wd0, bd0, which="both", cut=None, dT=None):
    """One _f16 backward call on fresh device copies -> (weight_diff, bias_diff) as numpy, None where the variant leaves
    it out.  `cut`: the pair call, layers [0, cut) and [cut, M).  dT: top_diff already on the device."""
    wd, bd = outputs(wd0, bd0, which)
    dT = dev(top_diff) if dT is None else dT
    assert dT.dtype == torch.float16
    if cut is not None:
        capi.embed_backward_pair_f16(dev(idx[:cut]), dev(idx[cut:]), dT[:cut], dT[cut:], wd, bias_diff=bd, shape=wd0.shape)
    else:
        capi.embed_backward_f16(dev(idx), dT, wd, bd, shape=wd0.shape)
    return host(wd), host(bd)


def backward32(capi, idx, top_diff, wd0, bd0, which="both", cut=None):
    """The _f32 twin on a widened DEVICE copy of the half top_diff"""
    wd, bd = outputs(wd0, bd0, which)
    dT = dev(top_diff).float()
    if cut is not None:
        capi.embed_backward_pair(dev(idx[:cut]), dev(idx[cut:]), dT[:cut], dT[cut:], wd, bias_diff=bd, shape=wd0.shape)
    else:
        capi.embed_backward(dev(idx), dT, wd, bd, shape=wd0.shape)
    return host(wd), host(bd)


def bias_sum(top_diff, bd0):
    """bias_diff's reference: the fp64 column sum on top of the start value"""
    return bd0.astype(D) + top_diff.astype(D).sum(axis=0)


def bias_diff_close(got, ref, what):
    err = np.abs(got.astype(D) - ref).max()
    print("%s: max abs err %.3e (bound %.3e)" % (what, err, TOL * max(1.0, np.abs(ref).max())))
    assert_close(got, ref, TOL, what)


# ------------------------------------------------------------------ planted segment lengths
@pytest.fixture(scope="module")
def reference(oracle):
    """name -> the case with the oracle's weight_diff on the widened top_diff ("wd": one layer; "wd_pair": layer 0's
    Backward, then layer 1's) and the fp64 bias sum, computed once per case and left unchanged."""
    done = {}

    def get(name):
        if name not in done:
            c = dict(em.make_case(name))
            c["idx"] = c["index"].astype(F)
            wide = em.widen(c["top_diff"])
            c["wd"], _ = oracle.embed_backward(c["idx"], wide, c["wd0"], c["bd0"])
            M0 = es.PAIR_CUT
            wd_a, _ = oracle.embed_backward(c["idx"][:M0], wide[:M0], c["wd0"])
            c["wd_pair"], _ = oracle.embed_backward(c["idx"][M0:], wide[M0:], wd_a)
            c["bd"] = bias_sum(c["top_diff"], c["bd0"])
            done[name] = c
        return done[name]
    return get


def check_outputs(c, got, twin, wd_ref, what):
    (wd, bd), (wd32, bd32) = got, twin
    if wd is not None:
        weight_diff_matches(wd, wd_ref, c["index"], what + ": weight_diff against the oracle (n-ascending sums)")
        same_words(wd, wd32, what + ": weight_diff against the _f32 twin")
    if bd is not None:
        same_words(bd, bd32, what + ": bias_diff against the _f32 twin")
        bias_diff_close(bd, c["bd"], what + ": bias_diff")


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", list(em.CASES))
def test_backward_f16(reference, capi, name, which):
    c = reference(name)
    got = backward16(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which)
    twin = backward32(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which)
    check_outputs(c, got, twin, c["wd"], name)


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", list(em.CASES))
def test_backward_pair_f16(reference, capi, name, which):
    """Two layers over one table, cut at row 1777: layer 0's rows ascending, then layer 1's, into the same diffs."""
    c = reference(name)
    M0 = es.PAIR_CUT
    assert es.straddlers(c["index"], c["planted"], M0)               # a segment's chain crosses from layer 0 to layer 1
    got = backward16(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which, cut=M0)
    twin = backward32(capi, c["idx"], c["top_diff"], c["wd0"], c["bd0"], which, cut=M0)
    check_outputs(c, got, twin, c["wd_pair"], name + " pair")
    # ... and equals the two single-layer _f16 calls
    wd2, bd2 = outputs(c["wd0"], c["bd0"], which)
    dT = dev(c["top_diff"])
    capi.embed_backward_f16(dev(c["idx"][:M0]), dT[:M0], wd2, bd2, shape=c["wd0"].shape)
    capi.embed_backward_f16(dev(c["idx"][M0:]), dT[M0:], wd2, bd2, shape=c["wd0"].shape)
    if wd2 is not None:
        weight_diff_matches(got[0], host(wd2), c["index"], name + ": pair == two calls")
    if bd2 is not None:
        bias_diff_close(host(bd2), c["bd"], name + ": bias_diff of the two calls")


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("name", [n for n in em.CASES if em.CASES[n][0] <= es.PREP_MAX])
def test_backward_pair_indexed_f16(reference, capi, name, which):
    """The inverted index built beside the half pair forward, used twice; then an index from either forward under either
    indexed backward: the same words four times."""
    c = reference(name)
    M0, M, N = es.PAIR_CUT, c["M"], c["N"]
    r = np.random.default_rng(77)
    table = r.uniform(-0.08, 0.08, (c["K"], N)).astype(H)
    i0, i1 = dev(c["idx"][:M0]), dev(c["idx"][M0:])
    dT = dev(c["top_diff"])
    dT32 = dT.float()

    def forward(half):
        index = capi.EmbedPairIndex()                               # zeroed, so that the two buffers can be compared whole
        index.buf = torch.zeros(capi.lib().mms_embed_workspace_bytes(M, N), dtype=torch.uint8, device="cuda")
        if half:
            t0, t1 = torch.zeros((M0, N), dtype=torch.float16, device="cuda"), torch.zeros((M - M0, N), dtype=torch.float16, device="cuda")
            assert capi.embed_forward_pair_f16(i0, i1, dev(table), t0, t1, index=index)
            same_words(host(torch.cat([t0, t1])), table[c["index"]], "the forward beside the index build")
        else:
            t0, t1 = torch.zeros((M0, N), device="cuda"), torch.zeros((M - M0, N), device="cuda")
            assert capi.embed_forward_pair(i0, i1, dev(table.astype(F)), t0, t1, index=index)
        return index

    def indexed(index, half):
        wd, bd = outputs(c["wd0"], c["bd0"], which)
        if half:
            capi.embed_backward_pair_indexed_f16(i0, i1, dT[:M0], dT[M0:], wd, index, bias_diff=bd, shape=c["wd0"].shape)
        else:
            capi.embed_backward_pair_indexed(i0, i1, dT32[:M0], dT32[M0:], wd, index, bias_diff=bd, shape=c["wd0"].shape)
        return host(wd), host(bd)

    index16, index32 = forward(True), forward(False)
    assert index16.buf.any() and torch.equal(index16.buf, index32.buf), "the two forwards wrote different index workspaces"
    twin = indexed(index32, False)                                  # the _f32 twin: fp32 forward, fp32 indexed backward
    for use in ("first", "second"):                                 # the index is read-only
        check_outputs(c, indexed(index16, True), twin, c["wd_pair"], "%s indexed, %s use" % (name, use))
    for built, index in (("f16", index16), ("f32", index32)):
        for half in (True, False):
            check_outputs(c, indexed(index, half), twin, c["wd_pair"],
                          "%s: index of the %s forward, %s backward" % (name, built, "f16" if half else "f32"))


def test_no_index_above_4096_rows(reference, capi):
    c = reference("f16-M4500-N300")
    M0, M, N = es.PAIR_CUT, c["M"], c["N"]
    table = np.random.default_rng(78).uniform(-0.08, 0.08, (c["K"], N)).astype(H)
    t0 = torch.zeros((M0, N), dtype=torch.float16, device="cuda")
    t1 = torch.zeros((M - M0, N), dtype=torch.float16, device="cuda")
    index = capi.EmbedPairIndex()
    built = capi.embed_forward_pair_f16(dev(c["idx"][:M0]), dev(c["idx"][M0:]), dev(table), t0, t1, index=index)
    assert built is False
    same_words(host(torch.cat([t0, t1])), table[c["index"]], "the forward itself still runs")
    with pytest.raises(capi.MMSError):
        capi.embed_backward_pair_indexed_f16(dev(c["idx"][:M0]), dev(c["idx"][M0:]), t0, t1, dev(c["wd0"]), index)


def test_two_calls_give_the_same_words_and_a_graph_replays_them(reference, capi):
    """Deterministic; and one backward captured in a (single-branch) graph and replayed once is the eager call."""
    c = reference("f16-M4000-N300")
    idx, dT = dev(c["idx"]), dev(c["top_diff"])
    ws = capi.Workspace()
    runs = []
    for _ in range(2):
        wd, bd = dev(c["wd0"]), dev(c["bd0"])
        capi.embed_backward_f16(idx, dT, wd, bd, ws=ws)
        runs.append((host(wd), host(bd)))
    same_words(runs[0][0], runs[1][0], "weight_diff of two identical calls")
    same_words(runs[0][1], runs[1][1], "bias_diff of two identical calls")
    weight_diff_matches(runs[0][0], c["wd"], c["index"], "eager weight_diff")
    wd, bd = dev(c["wd0"]), dev(c["bd0"])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            capi.embed_backward_f16(idx, dT, wd, bd, ws=ws)
    torch.cuda.synchronize()
    same_words(host(wd), c["wd0"], "capture itself ran the kernels")
    graph.replay()
    torch.cuda.synchronize()
    same_words(host(wd), runs[0][0], "weight_diff of the replay against the eager call")
    same_words(host(bd), runs[0][1], "bias_diff of the replay against the eager call")


# ------------------------------------------------------------------ bias_diff, exactly
@pytest.mark.parametrize("with_weight", [False, True], ids=["bias_only", "with_weight_diff"])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 1025, 4096, 4097])
def test_bias_diff_of_dyadic_rows_is_exact(capi, M, with_weight):
    """top_diff holds multiples of 2^-8 in [-4, 4] (11 significant bits at most: halves), the start value likewise:
    every partial sum of up to 4500 of them is below 2^15 with 8 fraction bits, 23 bits, exact in fp32 in ANY order.  So
    bias_diff has one right answer whatever the launch shape and the fold of the partial sums -- no tolerance."""
    K = 600
    for N in (50, 64, 65):
        r = np.random.default_rng(1000 * N + M)
        q = r.integers(-1024, 1025, (M, N))
        b = r.integers(-1024, 1025, N)
        top_diff, bd0 = (q / 256.0).astype(H), (b / 256.0).astype(F)
        assert (top_diff.astype(D) * 256.0 == q).all()                # representable in half
        exact = ((b + q.sum(axis=0)) / 256.0).astype(F)
        assert np.abs(b + q.sum(axis=0)).max() < 2 ** 23
        index = r.integers(0, K, M).astype(F)
        wd0 = r.standard_normal((K, N)).astype(F)
        _, bd = backward16(capi, index, top_diff, wd0, bd0, "both" if with_weight else "bias_only")
        same_words(bd, exact, "M %d N %d" % (M, N))


# ------------------------------------------------------------------ misaligned operands
def small_case(N, seed):
    index, planted = es.planted_index((1, 2, 8, 9, 32, 33, 300), 500, 60, seed)
    top_diff, wd0, bd0 = em.large_accumulator_inputs(index, N, 60, seed + 1)
    return index.astype(F), top_diff, wd0, bd0


@pytest.mark.parametrize("where", ["4+2", "16+2"])
@pytest.mark.parametrize("N", [50, 51, 300])
def test_backward_of_a_misaligned_top_diff(capi, N, where):
    idx, top_diff, wd0, bd0 = small_case(N, 600 + N)
    ref = backward16(capi, idx, top_diff, wd0, bd0)
    got = backward16(capi, idx, top_diff, wd0, bd0, dT=place(top_diff, where))
    same_words(got[0], ref[0], "weight_diff")
    same_words(got[1], ref[1], "bias_diff")
    cut = 211
    dT = place(top_diff, where)                                       # layer 1 starts at row 211 of the same buffer
    pair = backward16(capi, idx, top_diff, wd0, bd0, cut=cut, dT=dT)
    same_words(pair[0], ref[0], "weight_diff of the pair call")


# ------------------------------------------------------------------ edges of the call
def check_edge(capi, oracle, raw, valid, N, K, seed, cut=None):
    """The library on the ids `raw` against the oracle on the in-range ids `valid`."""
    top_diff, wd0, bd0 = em.large_accumulator_inputs(valid, N, K, seed)
    wd_ref, _ = oracle.embed_backward(valid.astype(F), em.widen(top_diff), wd0, bd0)
    wd, bd = backward16(capi, raw.astype(F), top_diff, wd0, bd0, "both", cut=cut)
    weight_diff_matches(wd, wd_ref, valid, "weight_diff")
    bias_diff_close(bd, bias_sum(top_diff, bd0), "bias_diff")
    return wd, wd0


def odd_ids(K, M, seed):
    """Ids the reference would DCHECK: int(id), then [0, K - 1].  -> (raw, in-range), shuffled among ordinary ids."""
    r = np.random.default_rng(seed)
    raw = np.r_[[-3.0, -0.5, 4.9, K - 0.5, K, K + 5.0, 1e9], r.integers(0, K, M - 7).astype(D)]
    raw = raw[r.permutation(M)]
    return raw, np.clip(np.trunc(raw), 0, K - 1).astype(np.int64)


@pytest.mark.parametrize("cut", [None, 20], ids=["single", "pair"])
def test_backward_clamps_and_truncates_ids_like_the_forward(capi, oracle, cut):
    K, M, N = 9, 45, 70
    raw, valid = odd_ids(K, M, 31)
    assert valid.min() == 0 and valid.max() == K - 1 and 4 in valid
    if cut is not None:                                            # odd ids in both layers
        assert (raw[:cut] != valid[:cut]).any() and (raw[cut:] != valid[cut:]).any()
    check_edge(capi, oracle, raw, valid, N, K, 32, cut=cut)


@pytest.mark.parametrize("cut", [None, 100], ids=["single", "pair"])
@pytest.mark.parametrize("K", [1, 2, 257, 2 ** 20 + 1])
def test_first_and_last_table_row_at_every_bit_count(capi, oracle, K, cut):
    """The index sort looks at ceil(log2 K) bits of an id: every row of the batch on id 0 or id K - 1."""
    M, N = 300, 7
    r = np.random.default_rng(40 + K % 1000)
    valid = np.where(r.uniform(size=M) < 0.5, 0, K - 1).astype(np.int64)
    wd, wd0 = check_edge(capi, oracle, valid, valid, N, K, 41 + K % 1000, cut=cut)
    if K > 257:
        assert (words(wd[1:K - 1]) == words(wd0[1:K - 1])).all(), "a row other than 0 and K - 1 changed"
        assert (words(wd[[0, K - 1]]) != words(wd0[[0, K - 1]])).any(axis=1).all()


@pytest.mark.parametrize("cut", [None, 1], ids=["single", "pair"])
def test_one_row(capi, oracle, cut):
    M = 1 if cut is None else 2                                    # the pair call needs a row in each layer
    valid = np.full(M, 3, np.int64)
    check_edge(capi, oracle, valid, valid, 70, 5, 50, cut=cut)


@pytest.mark.parametrize("cut", [None, 333], ids=["single", "pair"])
def test_one_destination(capi, oracle, cut):
    """Every row on the same id: one segment of 700 rows (more than two chunks), 599 idle workgroups."""
    valid = np.full(700, 17, np.int64)
    check_edge(capi, oracle, valid, valid, 70, 600, 51, cut=cut)


@pytest.mark.parametrize("cut", [None, 333], ids=["single", "pair"])
def test_all_ids_distinct(capi, oracle, cut):
    """M = K segments of one row: every workgroup of the grid has one."""
    valid = np.random.default_rng(52).permutation(600).astype(np.int64)
    check_edge(capi, oracle, valid, valid, 70, 600, 53, cut=cut)


# ------------------------------------------------------------------ forward
SENTINEL = 0x7d55           # a NaN no table below holds and no sum produces (an add quietens: 0x7f55)
GUARD = 24                  # halves before and after a top buffer
SPECIAL = np.array([0x7e01, 0x7c01, 0xfe00, 0xfdff, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x0001, 0x83ff, 0x03ff, 0x7bff, 0xfbff,
                    0x3c00], np.uint16)   # NaNs with payloads (quiet and signalling), +-Inf, +-0, subnormals, max-finite


def special_table(K, N, seed):
    r = np.random.default_rng(seed)
    table = r.standard_normal((K, N)).astype(H)
    t = words(table)
    hit = r.uniform(size=(K, N)) < 0.2
    t[hit] = r.choice(SPECIAL, int(hit.sum()))
    t[:, 0] = np.resize(SPECIAL, K)                                  # every special in column 0, whatever the draw
    t[::2, N - 1] = 0x7bff                                          # max-finite down the last column: the overflow probe
    return table


class GuardedTop:
    """A half top (M, N) pre-filled with a sentinel inside a larger buffer whose guard halves must survive."""

    def __init__(self, M, N, where="aligned"):
        raw = np.full(M * N + 2 * GUARD, SENTINEL, np.uint16).view(H)
        self.buf = place(raw, where)
        self.t = self.buf[GUARD:GUARD + M * N].view(M, N)
        self.M, self.N = M, N

    def result(self, what):
        b = words(host(self.buf))
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.M * self.N:] == SENTINEL).all(), what + ": a guard half was written"
        got = b[GUARD:GUARD + self.M * self.N].reshape(self.M, self.N)
        assert (got != SENTINEL).all(), what + ": %d halves of top were not written" % int((got == SENTINEL).sum())
        return got.view(H)


def forward_reference(oracle, ids, table, bias):
    if bias is None:
        return table[ids]
    with np.errstate(over="ignore", invalid="ignore"):
        return oracle.embed_forward(ids.astype(F), em.widen(table), bias).astype(H)


@pytest.mark.parametrize("where", ["aligned", "4+2", "16+2"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("N", [50, 51, 64, 300])
def test_forward_f16(capi, oracle, N, with_bias, where):
    """Without a bias the table's words (every access width: N = 64 -> 8 halves, 300 -> 4, 50 -> 2, 51 -> 1, and one
    when a base is misaligned); with one, the oracle's sum on the widened table rounded once."""
    K, M = 97, 203
    r = np.random.default_rng(900 + N)
    table = special_table(K, N, 901 + N)
    raw, ids = odd_ids(K, M, 902 + N)
    bias = None
    if with_bias:
        bias = r.standard_normal(N).astype(F)
        bias[N - 1] = 64.0                                          # 65504 + 64 is past the last half before overflow
    ref = forward_reference(oracle, ids, table, bias)
    if with_bias:
        col = ref[:, N - 1]
        assert (words(table[ids])[:, N - 1] == 0x7bff).any() and np.isposinf(col[words(table[ids])[:, N - 1] == 0x7bff]).all()
    top = GuardedTop(M, N, where)
    capi.embed_forward_f16(dev(raw.astype(F)), place(table, where), top.t, bias=dev(bias))
    same_words(top.result("single"), ref, "top", nan_meets_nan=with_bias)
    # the pair forward is two single forwards
    cut = 77
    t0, t1 = GuardedTop(cut, N, where), GuardedTop(M - cut, N, "aligned")
    index = capi.EmbedPairIndex()
    assert capi.embed_forward_pair_f16(dev(raw[:cut].astype(F)), dev(raw[cut:].astype(F)), place(table, where), t0.t, t1.t,
                                       bias=dev(bias), index=index)
    same_words(np.concatenate([t0.result("pair, top0"), t1.result("pair, top1")]), ref, "pair forward", nan_meets_nan=with_bias)
    s0, s1 = GuardedTop(cut, N), GuardedTop(M - cut, N)
    capi.embed_forward_pair_f16(dev(raw[:cut].astype(F)), dev(raw[cut:].astype(F)), dev(table), s0.t, s1.t, bias=dev(bias))
    same_words(np.concatenate([s0.result("pair, no index"), s1.result("pair, no index")]), ref, "pair forward without an index",
               nan_meets_nan=with_bias)


# ------------------------------------------------------------------ the chain with the fp16-storage SimCross
@pytest.mark.parametrize("mode", [1, 0], ids=["euclid", "cosine"])
def test_chain_with_simcross_f16(capi, mode):
    N, W1, W2, Dm, K = 4, 5, 7, 50, 97
    r = np.random.default_rng(1200 + mode)
    table = dev((r.standard_normal((K, Dm)) * 0.4).astype(H))
    iq, ia = dev(r.integers(0, K, (N, W1)).astype(F)), dev(r.integers(0, K, (N, W2)).astype(F))

    def scores():
        return (torch.zeros((N, 1, W1, W2), device="cuda"),
                dict(norm0=torch.zeros((N, W1), device="cuda"), norm1=torch.zeros((N, W2), device="cuda")) if mode == 0 else {})

    # forward: Embed, then SimCross, against the fused call
    q, a = torch.zeros((N, W1, Dm), dtype=torch.float16, device="cuda"), torch.zeros((N, W2, Dm), dtype=torch.float16, device="cuda")
    capi.embed_forward_f16(iq, table, q.view(N * W1, Dm))
    capi.embed_forward_f16(ia, table, a.view(N * W2, Dm))
    top, norms = scores()
    capi.simcross_forward_f16(mode, q, a, top, **norms)
    ftop, fnorms = scores()
    capi.embed_simcross_forward_f16(mode, iq, ia, table, ftop, **fnorms)
    same_words(host(top), host(ftop), "top: Embed then SimCross against the fused call")
    for k in norms:
        same_words(host(norms[k]), host(fnorms[k]), k)
    # the training loop: pair forward (+ index) -> forward_backward -> indexed backward
    q2, a2 = torch.zeros_like(q), torch.zeros_like(a)
    index = capi.EmbedPairIndex()
    assert capi.embed_forward_pair_f16(iq, ia, table, q2.view(N * W1, Dm), a2.view(N * W2, Dm), index=index)
    same_words(host(q2), host(q), "q of the pair forward")
    same_words(host(a2), host(a), "a of the pair forward")
    top_diff = dev(r.standard_normal((N, 1, W1, W2)).astype(F))
    dq, da = torch.zeros_like(q), torch.zeros_like(a)
    top2, norms2 = scores()
    capi.simcross_forward_backward_f16(mode, q2, a2, top_diff, top2, dq, da, **norms2)
    assert np.isfinite(host(dq).astype(F)).all() and host(dq).any() and host(da).any()
    wd0 = (r.standard_normal((K, Dm)) * 0.01).astype(F)
    bd0 = r.standard_normal(Dm).astype(F)
    wd, bd = dev(wd0), dev(bd0)
    capi.embed_backward_pair_indexed_f16(iq, ia, dq.view(N * W1, Dm), da.view(N * W2, Dm), wd, index, bias_diff=bd)
    wd32, bd32 = dev(wd0), dev(bd0)
    capi.embed_backward_pair(iq, ia, dq.float().view(N * W1, Dm), da.float().view(N * W2, Dm), wd32, bias_diff=bd32)
    same_words(host(wd), host(wd32), "weight_diff of the half chain against embed_backward_pair on the widened dq / da")
    same_words(host(bd), host(bd32), "bias_diff of the half chain")
    assert (words(host(wd)) != words(wd0)).any()
