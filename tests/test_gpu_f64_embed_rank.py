"""GPU parity of the double twins of the Embed and ranking-metric calls (mms_embed_*_f64, mms_rank_*_f64) with the
oracle's double instantiation, on the 64-bit words unless a bound is stated.

AUC has no double oracle; it is checked against a restatement of auc_layer.cpp:42-136 written here.  That code sorts
its std::pair<Dtype, int> items with `mycompare_auc`, whose parameters are std::pair<float, int> (:42-44, :93-95):
std::sort converts each element for the call, so AUCLayer<double> ORDERS its items by the scores narrowed to float,
exactly like MAP / MRR, and only sums and divides in double.  The restatement narrows accordingly; scores that are
distinct as doubles and tied as floats are therefore ties, ordered by the tie mode (input order by default).  The test
data makes such pairs carry different labels in the order OPPOSITE to their double order, so that a sort on the full
double key gives another AUC (asserted on the data) and cannot pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D = np.float64


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def words(x):
    return np.ascontiguousarray(np.asarray(x, dtype=D)).view(np.uint64)


def same_words(got, ref, what):
    g, r = words(got).ravel(), words(ref).ravel()
    bad = np.flatnonzero(g != r)
    if bad.size:                                      # NaN must meet NaN; payloads may differ
        gn, rn = np.asarray(got, D).ravel()[bad], np.asarray(ref, D).ravel()[bad]
        still = ~(np.isnan(gn) & np.isnan(rn))
        assert not still.any(), "%s: %d of %d words differ, first at %d: %r vs %r" % (
            what, int(still.sum()), g.size, int(bad[still][0]), gn[still][0], rn[still][0])


@pytest.fixture(scope="module")
def capi(hiplib):
    from mms_answer_selection_amd import capi
    return capi


# ------------------------------------------------------------------ Embed
def offset_view(a):
    """A contiguous device copy of `a` that starts 8 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 3, dtype=torch.float64, device="cuda")
    skip = 1 if buf.data_ptr() % 16 == 0 else 2
    v = buf[skip:skip + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


EMBED_CASES = [(400, 50, 17, 0.0), (400, 3, 17, 0.0), (4096, 50, 300, 0.0), (4097, 50, 300, 0.0), (6000, 50, 300, 0.6)]


@pytest.fixture(scope="module", params=EMBED_CASES, ids=lambda c: "M%d-N%d-K%d" % c[:3])
def embed_case(request, oracle):
    M, N, K, zeros = request.param
    r = np.random.default_rng(9100 + M + N)
    index = r.integers(0, K, M)
    index[r.uniform(size=M) < zeros] = 0             # the zero-pad id: one long segment
    index = index.astype(D)
    c = {"M": M, "N": N, "K": K, "index": index, "weight": r.uniform(-0.08, 0.08, (K, N)),
         "bias": r.standard_normal(N), "dT": r.standard_normal((M, N)), "wd0": r.standard_normal((K, N)),
         "bd0": r.standard_normal(N)}
    c["top"] = {b: oracle.embed_forward(index, c["weight"], c["bias"] if b else None) for b in (False, True)}
    c["wd"], c["bd"] = oracle.embed_backward(index, c["dT"], c["wd0"], c["bd0"])
    return c


@pytest.mark.parametrize("use_bias", [False, True])
def test_embed_forward(embed_case, capi, use_bias):
    c = embed_case
    top = torch.full((c["M"], c["N"]), float("nan"), dtype=torch.float64, device="cuda")
    capi.embed_forward_f64(dev(c["index"]), dev(c["weight"]), top, bias=dev(c["bias"]) if use_bias else None)
    same_words(top.cpu().numpy(), c["top"][use_bias], "top")
    off = offset_view(np.full((c["M"], c["N"]), np.nan))                  # rows off the 16-byte grid: one column per lane
    capi.embed_forward_f64(dev(c["index"]), dev(c["weight"]), off, bias=dev(c["bias"]) if use_bias else None)
    same_words(off.cpu().numpy(), c["top"][use_bias], "top, 8 bytes off a 16-byte boundary")


def bias_close(got, ref):
    err = np.abs(got - ref).max()
    print("bias_diff max abs err %.3e (bound %.3e)" % (err, 1e-12 * max(1.0, np.abs(ref).max())))
    assert err <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("which", ["both", "weight_only", "bias_only", "top_diff_offset"])
def test_embed_backward(embed_case, capi, which):
    """weight_diff and bias_diff start from non-zero values: the layer accumulates (embed_layer.cpp:170, :177)."""
    c = embed_case
    wd = dev(c["wd0"]) if which != "bias_only" else None
    bd = dev(c["bd0"]) if which != "weight_only" else None
    dT = offset_view(c["dT"]) if which == "top_diff_offset" else dev(c["dT"])
    capi.embed_backward_f64(dev(c["index"]), dT, wd, bd, shape=(c["K"], c["N"]))
    if wd is not None:
        same_words(wd.cpu().numpy(), c["wd"], "weight_diff (n-ascending sums)")
    if bd is not None:
        bias_close(bd.cpu().numpy(), c["bd"])
    if which == "both":                               # no atomics: a second run gives the same words
        wd2 = dev(c["wd0"])
        capi.embed_backward_f64(dev(c["index"]), dev(c["dT"]), wd2, None)
        same_words(wd2.cpu().numpy(), c["wd"], "weight_diff, second run")


def test_embed_ids_are_clamped_like_the_float_call(capi, oracle):
    r = np.random.default_rng(9191)
    K, N = 5, 6
    index = np.array([-3.0, 0.0, 4.0, 7.0, 4.9, 1e9], D)
    weight = r.standard_normal((K, N))
    top = torch.empty((index.size, N), dtype=torch.float64, device="cuda")
    capi.embed_forward_f64(dev(index), dev(weight), top)
    same_words(top.cpu().numpy(), oracle.embed_forward(np.array([0.0, 0, 4, 4, 4, 4], D), weight), "clamped rows")


# ------------------------------------------------------------------ MAP / MRR
def rank_inputs(n, groups, fixed_axis, seed, tied=False):
    r = np.random.default_rng(seed)
    group = np.sort(r.integers(0, groups, n)).astype(D) if groups > 1 else np.zeros(n, D)
    group = group[r.permutation(n)] * 3 - 5           # unsorted, negative ids too (std::map<int, ...> order)
    label = (r.uniform(size=n) < 0.1).astype(D)
    if tied:   # float_value + k * 2^-40: distinct doubles, the same float (k * 2^-40 < half an ulp of 1/16)
        score = r.integers(1, 13, n) / 16.0 + r.permutation(np.arange(1, n + 1)) * 2.0 ** -40
        assert np.unique(score).size == n and np.unique(score.astype(np.float32)).size <= 12
    else:
        score = r.permutation(n) / float(n) + 0.25     # distinct as floats
        assert np.unique(score.astype(np.float32)).size == n
    prob = r.standard_normal((n, fixed_axis + 1))
    prob[:, fixed_axis] = score
    return prob, label, group


def check_map_mrr(capi, oracle, prob, label, group, fixed_axis):
    m_ref, e_ref = oracle.map_score(prob, label, group, fixed_axis)
    r_ref, _ = oracle.mrr_score(prob, label, group, fixed_axis)
    m, rr, eff = capi.rank_map_mrr_f64(dev(prob), dev(label), dev(group), fixed_axis)
    print("MAP %r / %r  MRR %r / %r  effective %d / %d" % (m, m_ref, rr, r_ref, eff, e_ref))
    assert eff == e_ref
    same_words(m, m_ref, "MAP")
    same_words(rr, r_ref, "MRR")


@pytest.mark.parametrize("fixed_axis", [1, 0])
@pytest.mark.parametrize("groups", [1, 7, 68])
@pytest.mark.parametrize("n", [50, 512, 513, 2048, 2049])
def test_map_mrr_distinct_scores(capi, oracle, n, groups, fixed_axis):
    check_map_mrr(capi, oracle, *rank_inputs(n, groups, fixed_axis, 7000 + n + groups), fixed_axis)


@pytest.mark.parametrize("n", [50, 513, 2049])
def test_map_mrr_doubles_that_tie_as_floats(capi, oracle, n):
    """The reference narrows every score to float before it sorts (std::pair<float, int>, map_layer.cpp:34-47): these
    scores are ties there, and in MMS_RANK_TIES_LIBSTDCXX mode their order is the one the oracle's std::sort leaves."""
    prob, label, group = rank_inputs(n, 7, 1, 7100 + n, tied=True)
    label[:] = np.random.default_rng(n).uniform(size=n) < 0.4            # ties across labels in every bucket
    capi.set_rank_tie_mode("libstdcxx")
    try:
        check_map_mrr(capi, oracle, prob, label, group, 1)
    finally:
        capi.set_rank_tie_mode("input")


@pytest.mark.parametrize("n", [50, 513, 2049])
def test_map_mrr_groups_without_a_positive_or_a_negative(capi, oracle, n):
    prob, label, group = rank_inputs(n, 7, 1, 7200 + n)
    ids = np.unique(group)
    label[group == ids[1]] = 0.0                      # no positive: counts for neither metric
    label[group == ids[2]] = 1.0                      # no negative: counts for neither metric
    check_map_mrr(capi, oracle, prob, label, group, 1)


@pytest.mark.parametrize("n", [50, 513, 2049])
def test_map_mrr_no_group_counts_gives_nan(capi, oracle, n):
    prob, label, group = rank_inputs(n, 7, 1, 7300 + n)
    label[:] = 0.0
    m, rr, eff = capi.rank_map_mrr_f64(dev(prob), dev(label), dev(group), 1)
    m_ref, e_ref = oracle.map_score(prob, label, group, 1)
    assert eff == e_ref == 0 and np.isnan(m_ref) and np.isnan(m) and np.isnan(rr)


# ------------------------------------------------------------------ AUC
def auc_restated(prob, label, fixed_axis, ignore_label=None, narrow=True):
    """auc_layer.cpp:47-136 for Dtype = double, prob (outer, channels, inner), label (outer, inner).  `narrow`: the
    comparator's std::pair<float, int> parameters (:42-44); ties in input order (a stable sort)."""
    items = []
    outer, _, inner = prob.shape
    for i in range(outer):
        for j in range(inner):
            lab = int(label[i, j])
            if ignore_label is not None and lab == ignore_label:
                continue
            items.append((prob[i, fixed_axis, j], lab))
    key = np.array([s for s, _ in items], D)
    key = key.astype(np.float32) if narrow else key
    order = np.argsort(-key, kind="stable")
    high, total = 0, 0
    for p in order:
        high += items[p][1]
        total += high * (1 - items[p][1])
    if high <= 0:
        return D(0.0)
    return D(total) / D(high) / D(len(items) - high)


def auc_inputs(outer, channels, inner, fixed_axis, seed, ignore=False):
    r = np.random.default_rng(seed)
    n = outer * inner
    label = (r.uniform(size=n) < 0.3).astype(D)
    base = ((r.permutation(n) // 2 + 1) / float(n)).astype(np.float32).astype(D)     # every float value twice ...
    score = base + 2.0 ** -40                          # ... told apart below float precision:
    first = np.zeros(n, bool)
    seen = set()
    for i in range(n):
        first[i] = base[i] not in seen
        seen.add(base[i])
    score[~first] += 2.0 ** -40                        # the LATER item of a pair is the larger double,
    label[~first & (r.uniform(size=n) < 0.8)] = 1.0    # and where the pair's labels differ ...
    for i in np.flatnonzero(~first):
        j = np.flatnonzero((base == base[i]) & first)[0]
        if label[i] == 1.0:
            label[j] = 0.0                             # ... the earlier one is the negative
    if ignore:
        label[r.uniform(size=n) < 0.15] = 2.0
    assert np.unique(score).size == n and np.unique(score.astype(np.float32)).size == (n + 1) // 2
    prob = r.standard_normal((outer, channels, inner))
    prob[:, fixed_axis, :] = score.reshape(outer, inner)
    return prob, label.reshape(outer, inner)


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("n", [50, 513, 2049])
def test_auc(capi, n, ignore):
    prob, label = auc_inputs(n, 2, 1, 1, 7400 + n, ignore)
    il = 2 if ignore else None
    ref, wide = auc_restated(prob, label, 1, il), auc_restated(prob, label, 1, il, narrow=False)
    assert words(ref) != words(wide)                  # the data tells a float-keyed sort from a double-keyed one
    got = capi.rank_auc_f64(dev(prob.reshape(n, 2)), dev(label.reshape(n)), 1, il)
    print("AUC %r / %r (double-keyed sort: %r)" % (got, ref, wide))
    same_words(got, ref, "AUC")
    got_nd = capi.rank_auc_nd_f64(dev(prob.reshape(n, 2)), dev(label.reshape(n)), 1, 1, il)
    same_words(got_nd, ref, "AUC through _nd")


def test_auc_nd_inner_axis(capi):
    for il in (None, 2):
        prob, label = auc_inputs(37, 2, 3, 1, 7500, ignore=il is not None)
        ref = auc_restated(prob, label, 1, il)
        got = capi.rank_auc_nd_f64(dev(prob), dev(label), 1, 1, il)
        same_words(got, ref, "AUC (37, 2, 3), ignore_label %r" % il)


@pytest.mark.parametrize("n", [50, 513, 2049])
def test_auc_without_a_positive_is_exactly_zero(capi, n):
    prob, _ = auc_inputs(n, 2, 1, 1, 7600 + n)
    got = capi.rank_auc_f64(dev(prob.reshape(n, 2)), dev(np.zeros(n, D)), 1)
    assert words(got) == words(0.0)


# ------------------------------------------------------------------ RankAccuracy
@pytest.mark.parametrize("count", [1, 63, 5000])
def test_rank_accuracy(capi, oracle, count):
    r = np.random.default_rng(7700 + count)
    a, b = r.standard_normal(count), r.standard_normal(count)
    same = r.uniform(size=count) < 0.2
    b[same] = a[same]                                 # a == b: never counted
    label = r.choice(np.array([-1.0, 0.0, 1.0]), count)
    ref = oracle.rank_accuracy(a, b, label)
    got = capi.rank_accuracy_f64(dev(a), dev(b), dev(label))
    same_words(got, ref, "accuracy")
