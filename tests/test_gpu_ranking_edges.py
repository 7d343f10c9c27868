"""Edge-case parity for the ranking metrics (csrc/ranking.hip, csrc/rank_onewg.hip, csrc/rank_common.h) on all three size
paths:

    n <= 512         rank_small_kernel   (LDS bitonic sort, one thread per position)
    513 <= n <= 2048 rank_mid_kernel     (register sort, buckets walked by 1,024 threads)
    n > 2048         rocPRIM radix sort + rank_bucket_kernel / rank_fold_kernel (also every n in libstdc++ tie mode)

Every case compares the C ABI with the oracle (std::map<int> + std::sort + the reference's float expressions,
oracle/mms_oracle_rank.cpp) bit for bit, and `effective` exactly: more buckets than threads, labels and group ids
that the reference converts with int(...), fixed_axis other than 1, AUC's general indexing at the larger sizes,
+0.0 / -0.0 scores (equal under the reference's `>`), and RankAccuracy where its reduction and the reference's
float accumulator reach their limits."""
import numpy as np
import pytest
import torch

from util import rng

pytestmark = pytest.mark.gpu

# one size on either side of every boundary: padded bitonic sizes, the small / mid / radix limits, 1,024 threads
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
PATH_SIZES = [300, 1500, 3000]          # one size per path: small, mid, radix


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_bits(x, y):
    return np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32) or (np.isnan(x) and np.isnan(y))


def distinct_scores(r, n):
    s = ((r.permutation(n) + 0.5) / n).astype(np.float32)
    assert np.unique(s).size == n
    return s


def nonzero_scores(r, n):
    """Distinct scores of either sign, none of them zero."""
    return (distinct_scores(r, n) * np.where(r.uniform(size=n) < 0.5, -1, 1)).astype(np.float32)


def make_prob(r, score, fixed_axis=1):
    """prob (n, fixed_axis + 1) whose column fixed_axis is `score` (map_layer.cpp:50); the other columns are noise."""
    if fixed_axis == 1:
        return np.stack([1 - score, score], 1).astype(np.float32)
    prob = r.uniform(-1, 1, (score.size, fixed_axis + 1)).astype(np.float32)
    prob[:, fixed_axis] = score
    return prob


def bucket_counts(label, group):
    """Per bucket in std::map order (ascending int(group)): does it count for MAP (a label 1 and a label != 1) and
    for MRR (a label 1 and a label 0)?  Labels and groups truncated like the reference's int(...)."""
    lab = np.trunc(label).astype(np.int64)
    _, inv = np.unique(np.trunc(group).astype(np.int64), return_inverse=True)
    inv = inv.reshape(-1)
    pos = np.bincount(inv, weights=lab == 1) > 0
    cmap = pos & (np.bincount(inv, weights=lab != 1) > 0)
    cmrr = pos & (np.bincount(inv, weights=lab == 0) > 0)
    return cmap, cmrr


def items_from_sizes(r, sizes, labels_of):
    """Buckets of the given sizes, bucket b with group id b - len(sizes) // 2 (negative ids sort first, like
    std::map<int>), so that the sorted bucket index of bucket b is b; labels from labels_of(size); then the items
    are permuted so that the buckets arrive interleaved."""
    sizes = np.asarray(sizes, np.int64)
    group = (np.repeat(np.arange(sizes.size), sizes) - sizes.size // 2).astype(np.float32)
    label = np.concatenate([labels_of(int(s)) for s in sizes]).astype(np.float32) if sizes.size else np.zeros(0, np.float32)
    perm = r.permutation(group.size)
    return group[perm], label[perm]


def one_pos_rest_neg(r):
    def f(s):
        lab = np.zeros(s, np.float32)
        if s > 1:
            lab[r.integers(s)] = 1
        else:
            lab[0] = r.integers(2)
        return lab
    return f


def layout(r, n, name):
    """-> (group, label) of n items in one of the layouts of the size matrix."""
    if name == "one":
        lab = (r.uniform(size=n) < 0.3).astype(np.float32)
        if n >= 2:
            lab[:2] = [1, 0]
        return items_from_sizes(r, [n], lambda s: lab)
    if name == "singletons":
        return items_from_sizes(r, [1] * n, lambda s: np.float32([r.integers(2)]))
    if name == "pairs":
        sizes = [2] * (n // 2) + [1] * (n % 2)
        return items_from_sizes(r, sizes, lambda s: r.permutation([1.0, 0.0]) if s == 2 else np.float32([1]))
    if name == "rand13":
        sizes = []
        while sum(sizes) < n:
            sizes.append(min(int(r.integers(1, 4)), n - sum(sizes)))
        return items_from_sizes(r, sizes, lambda s: (r.uniform(size=s) < 0.45).astype(np.float32))
    raise ValueError(name)


def sizes_for_buckets(n, B):
    """n items in exactly B buckets; the smaller buckets first, so the multi-item (counting) buckets take the
    highest sorted indices."""
    if 2 * B <= n:
        base, extra = divmod(n, B)
        return [base] * (B - extra) + [base + 1] * extra
    two = n - B
    return [1] * (B - two) + [2] * two


def check_map_mrr(oracle, prob, label, group, fixed_axis=1):
    """C ABI vs oracle, bit for bit and `effective` exactly; -> (effective MAP buckets, effective MRR buckets)."""
    from mms_answer_selection_amd import capi
    m_ref, eff_ref = oracle.map_score(prob, label, group, fixed_axis=fixed_axis)
    rr_ref, eff_mrr_ref = oracle.mrr_score(prob, label, group, fixed_axis=fixed_axis)
    m, rr, eff = capi.rank_map_mrr(dev(prob), dev(label), dev(group), fixed_axis=fixed_axis)
    assert eff == eff_ref, (eff, eff_ref)
    assert same_bits(m, m_ref), (m, m_ref)
    assert same_bits(rr, rr_ref), (rr, rr_ref)
    return eff_ref, eff_mrr_ref


# ---------------------------------------------------------------------------------------------------------------------
# size x group layout


@pytest.mark.parametrize("name", ["one", "singletons", "pairs", "rand13"])
@pytest.mark.parametrize("n", SIZES)
def test_size_by_layout(n, name, oracle, hiplib):
    r = rng(10 * n + len(name))
    group, label = layout(r, n, name)
    prob = make_prob(r, distinct_scores(r, n))
    cmap, cmrr = bucket_counts(label, group)
    eff, eff_mrr = check_map_mrr(oracle, prob, label, group)
    assert eff == int(cmap.sum()) and eff_mrr == int(cmrr.sum())
    if name == "singletons":
        assert eff == 0
    if name == "pairs" and n >= 2050:     # the radix path with counting buckets past sorted index 1023, for comparison
        assert cmap[1024:].any()
    if name == "one":
        from mms_answer_selection_amd import capi
        assert same_bits(capi.rank_auc(dev(prob), dev(label)), oracle.auc_score(prob, label))


@pytest.mark.parametrize("B", [1023, 1024, 1025, 1536, 2048])
def test_bucket_count_around_the_thread_count(B, oracle, hiplib):
    """n = 2048 (the mid path's largest input, 1,024 threads) in exactly B buckets; from B = 1025 on, buckets that
    count sit at sorted bucket index >= 1024, so a bucket left unwalked changes `effective` and both metrics.
    B = 2048 (all singletons) also fills the bucket-head array to its end."""
    n = 2048
    r = rng(B)
    sizes = sizes_for_buckets(n, B)
    assert len(sizes) == B and sum(sizes) == n
    group, label = items_from_sizes(r, sizes, one_pos_rest_neg(r))
    prob = make_prob(r, distinct_scores(r, n))
    cmap, cmrr = bucket_counts(label, group)
    assert cmap.size == B
    if B in (1025, 1536):
        assert cmap[1024:].sum() == B - 1024 and cmrr[1024:].sum() == B - 1024
    eff, eff_mrr = check_map_mrr(oracle, prob, label, group)
    assert eff == int(cmap.sum()) and eff_mrr == int(cmrr.sum())
    if B == 2048:
        from mms_answer_selection_amd import capi
        m, rr, e = capi.rank_map_mrr(dev(prob), dev(label), dev(group))
        assert e == 0 and np.isnan(m) and np.isnan(rr)


@pytest.mark.parametrize("n", [2000, 4099])
def test_counting_buckets_past_1024_on_mid_and_radix_paths(n, oracle, hiplib):
    """Groups of one to three candidates (per-pair evaluation, a WikiQA-style split): about n / 1.75 buckets with
    counting buckets spread over every sorted index, including the ones past 1023."""
    r = rng(n + 77)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(r.choice([1, 1, 2, 3])), n - sum(sizes)))
    group, label = items_from_sizes(r, sizes, one_pos_rest_neg(r))
    prob = make_prob(r, distinct_scores(r, n))
    cmap, cmrr = bucket_counts(label, group)
    assert cmap.size > 1024 and cmap[1024:].sum() > 20
    eff, eff_mrr = check_map_mrr(oracle, prob, label, group)
    assert eff == int(cmap.sum()) and eff_mrr == int(cmrr.sum())


# ---------------------------------------------------------------------------------------------------------------------
# labels and group ids as the reference converts them: int(x)


def random_groups(r, n, lo=1, hi=8):
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(r.integers(lo, hi)), n - sum(sizes)))
    return sizes


@pytest.mark.parametrize("n", PATH_SIZES)
def test_labels_converted_with_int(n, oracle, hiplib):
    """Labels outside {0, 1}: -1 and 2 are "not one" (MAP counts the bucket) but not "zero" (MRR does not);
    0.7 -> 0, 1.9 -> 1, -0.5 -> 0 (map_layer.cpp:50, mrr_layer.cpp:49 store them in an int)."""
    from mms_answer_selection_amd import capi
    r = rng(n + 5)
    values = np.float32([-1, 0, 1, 2, 0.7, 1.9, -0.5])
    group, _ = items_from_sizes(r, random_groups(r, n), lambda s: np.zeros(s, np.float32))
    label = values[r.choice(values.size, n, p=[0.15, 0.2, 0.2, 0.15, 0.1, 0.1, 0.1])]
    prob = make_prob(r, distinct_scores(r, n))
    cmap, cmrr = bucket_counts(label, group)
    eff, eff_mrr = check_map_mrr(oracle, prob, label, group)
    assert eff == int(cmap.sum()) and eff_mrr == int(cmrr.sum())
    assert eff > eff_mrr > 0            # the two flags really differ on this input
    # AUC over the same labels: high += int(label), auc += high * (1 - int(label)) (auc_layer.cpp:66-68, 119-123)
    assert same_bits(capi.rank_auc(dev(prob), dev(label)), oracle.auc_score(prob, label))
    # labels of 0.7 / 1.9 / -0.5 only: the same metrics as their truncations
    lab01 = np.float32([0.7, 1.9, -0.5, 0.0, 1.0])[r.integers(0, 5, n)]
    m, rr, e = capi.rank_map_mrr(dev(prob), dev(lab01), dev(group))
    m_t, rr_t, e_t = capi.rank_map_mrr(dev(prob), dev(np.trunc(lab01)), dev(group))
    assert e == e_t and same_bits(m, m_t) and same_bits(rr, rr_t)
    check_map_mrr(oracle, prob, lab01, group)


@pytest.mark.parametrize("n", PATH_SIZES)
def test_group_ids_converted_with_int(n, oracle, hiplib):
    """Group ids are bucketed by int(group): -0.5, -0.0, 0.0 and 0.5 share bucket 0, -1.9 and -1 share -1, 1.9 and 1
    share 1; ids of +-2^30 order like std::map<int> around the small ones."""
    from mms_answer_selection_amd import capi
    r = rng(n + 9)
    ids = np.array([-2 ** 30, -2 ** 30 + 128, -5, -1, 0, 1, 3, 2 ** 30 - 128, 2 ** 30], np.int64)
    gid = ids[r.integers(0, ids.size, n)]
    # each bucket through several float spellings of its id (all truncate to it)
    frac = r.uniform(0, 0.95, n).astype(np.float32)
    small = np.abs(gid) < 2 ** 20
    group = gid.astype(np.float32)
    group[small] += np.where(gid[small] > 0, 1, np.where(gid[small] < 0, -1, r.choice([-1, 1], n)[small])) * frac[small]
    zero = gid == 0
    group[zero & (r.uniform(size=n) < 0.2)] = -0.0
    assert (np.trunc(group).astype(np.int64) == gid).all()
    assert (group[zero] < 0).any() and (group[zero] > 0).any()
    label = (r.uniform(size=n) < 0.35).astype(np.float32)
    prob = make_prob(r, distinct_scores(r, n))
    cmap, cmrr = bucket_counts(label, group)
    assert cmap.size == ids.size
    eff, eff_mrr = check_map_mrr(oracle, prob, label, group)
    assert eff == int(cmap.sum()) == ids.size and eff_mrr == int(cmrr.sum())
    # the same metrics as the integer ids themselves
    m, rr, e = capi.rank_map_mrr(dev(prob), dev(label), dev(group))
    m_i, rr_i, e_i = capi.rank_map_mrr(dev(prob), dev(label), dev(gid.astype(np.float32)))
    assert e == e_i and same_bits(m, m_i) and same_bits(rr, rr_i)


@pytest.mark.parametrize("fixed_axis", [0, 2])
@pytest.mark.parametrize("n", PATH_SIZES)
def test_map_mrr_fixed_axis(n, fixed_axis, oracle, hiplib):
    """The score of item i is prob[i * (fixed_axis + 1) + fixed_axis] (map_layer.cpp:50, mrr_layer.cpp:49)."""
    r = rng(n + fixed_axis)
    group, label = items_from_sizes(r, random_groups(r, n, 1, 12), lambda s: (r.uniform(size=s) < 0.3).astype(np.float32))
    prob = make_prob(r, distinct_scores(r, n), fixed_axis)
    assert prob.shape == (n, fixed_axis + 1)
    eff, _ = check_map_mrr(oracle, prob, label, group, fixed_axis=fixed_axis)
    assert eff > 0


# ---------------------------------------------------------------------------------------------------------------------
# AUC's general layout at mid and radix sizes


@pytest.mark.parametrize("shape,axis", [((30, 2, 40), 1), ((1024, 2), 1), ((2, 1024), 0), ((5, 3, 700), 1),
                                        ((2049, 2), 1), ((3, 1100, 2), 2)])
def test_auc_general_layout_mid_and_large(shape, axis, oracle, hiplib):
    """rank_auc_nd with inner > 1, the label axis first / in the middle / last, both fixed_axis ends and ignore_label,
    at 1,024 - 3,500 items (mid and radix paths)."""
    from mms_answer_selection_amd import capi
    r = rng(sum(shape) + 3 * axis)
    total = int(np.prod(shape))
    prob = distinct_scores(r, total).reshape(shape)           # no two scores equal anywhere in the blob
    lshape = shape[:axis] + shape[axis + 1:]
    label = (r.uniform(size=lshape) < 0.4).astype(np.float32)
    C = shape[axis]
    assert 512 < label.size
    for fixed_axis in (0, C - 1):
        ref = oracle.auc_score_nd(prob, label, axis=axis, fixed_axis=fixed_axis)
        got = capi.rank_auc_nd(dev(prob), dev(label), axis=axis, fixed_axis=fixed_axis)
        assert same_bits(got, ref), (fixed_axis, got, ref)
    lab2 = label.copy()
    lab2.reshape(-1)[r.uniform(size=label.size) < 0.2] = 2
    for fixed_axis in (0, C - 1):
        ref = oracle.auc_score_nd(prob, lab2, axis=axis, fixed_axis=fixed_axis, ignore_label=2)
        got = capi.rank_auc_nd(dev(prob), dev(lab2), axis=axis, fixed_axis=fixed_axis, ignore_label=2)
        assert same_bits(got, ref), ("ignore", fixed_axis, got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# +0.0 and -0.0: equal scores under the reference's `lhs.first > rhs.first` (map_layer.cpp:33-38)


def signed_zero_groups(r, n, max_size=16):
    """Groups of 2..max_size items, each with several zero scores of both signs across both labels, the rest
    distinct non-zero scores.  The first groups are the two-item cases (-0 label 1, +0 label 0) and
    (+0 label 1, -0 label 0) and their mirror orders."""
    fixed = [([-0.0, 0.0], [1, 0]), ([0.0, -0.0], [0, 1]), ([0.0, -0.0], [1, 0]), ([-0.0, 0.0], [0, 1])]
    scores, labels, gids = [], [], []
    for g, (s, l) in enumerate(fixed):
        scores += s; labels += l; gids += [g, g]
    g = len(fixed)
    nonzero = iter(nonzero_scores(r, n))
    while len(scores) < n:
        m = min(int(r.integers(2, max_size + 1)), n - len(scores))
        z = min(m, int(r.integers(2, 7))) if m >= 2 else m
        s = [(-0.0 if r.integers(2) else 0.0) for _ in range(z)] + [float(next(nonzero)) for _ in range(m - z)]
        lab = list((r.uniform(size=m) < 0.5).astype(int))
        if m >= 2:
            lab[0], lab[1] = 1, 0                         # a cross-label tie among the zeros
            s[0], s[1] = (-0.0, 0.0) if r.integers(2) else (0.0, -0.0)
        order = r.permutation(m)
        scores += [s[i] for i in order]; labels += [lab[i] for i in order]; gids += [g] * m
        g += 1
    score = np.array(scores, np.float32)
    gid = np.array(gids, np.float32) - 3
    label = np.array(labels, np.float32)
    perm = r.permutation(score.size)                      # interleave the buckets; each keeps its items' order
    return score[perm], label[perm], gid[perm]


@pytest.mark.parametrize("n", PATH_SIZES)
def test_signed_zero_ties_in_small_buckets(n, oracle, hiplib):
    """Default tie mode, buckets of <= 16 items: libstdc++'s insertion sort keeps equal scores -- +0.0 and -0.0
    among them -- in input order, and so must every path."""
    r = rng(n + 21)
    score, label, group = signed_zero_groups(r, n)
    assert (np.signbit(score) & (score == 0)).any() and (~np.signbit(score) & (score == 0)).any()
    check_map_mrr(oracle, make_prob(r, score), label, group)


def test_signed_zero_two_item_group_exact_values(oracle, hiplib):
    """(-0.0, label 1) then (+0.0, label 0): the reference keeps the order, AP = 1 and RR = 1; the other order gives
    0.5 for both."""
    from mms_answer_selection_amd import capi
    for score, label, want in (([-0.0, 0.0], [1, 0], 1.0), ([0.0, -0.0], [1, 0], 1.0),
                               ([-0.0, 0.0], [0, 1], 0.5), ([0.0, -0.0], [0, 1], 0.5)):
        score, label = np.float32(score), np.float32(label)
        group = np.zeros(2, np.float32)
        prob = make_prob(None, score)
        m, rr, eff = capi.rank_map_mrr(dev(prob), dev(label), dev(group))
        assert eff == 1 and m == want and rr == want, (score, label, m, rr)
        assert oracle.map_score(prob, label, group)[0] == want


@pytest.mark.parametrize("n", range(2, 17))
def test_signed_zero_ties_auc_single_small_bucket(n, oracle, hiplib):
    """AUC's one bucket is the whole input: at n <= 16 its tie order is the input order too."""
    from mms_answer_selection_amd import capi
    r = rng(n + 300)
    score = np.where(r.uniform(size=n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    score[n // 2:] = np.where(r.uniform(size=n - n // 2) < 0.3, score[n // 2:],
                              r.uniform(-1, 1, n - n // 2).astype(np.float32))
    label = (r.uniform(size=n) < 0.5).astype(np.float32)
    label[:2] = [1, 0]
    score[:2] = [-0.0, 0.0]                 # -0.0 ahead of +0.0 in the input: the reference keeps that order
    prob = make_prob(r, score)
    assert same_bits(capi.rank_auc(dev(prob), dev(label)), oracle.auc_score(prob, label))
    lab_rev = label[::-1].copy()
    assert same_bits(capi.rank_auc(dev(prob), dev(lab_rev)), oracle.auc_score(prob, lab_rev))


@pytest.mark.parametrize("n", [120, 1500, 3000])
def test_signed_zero_ties_libstdcxx_mode(n, oracle, hiplib):
    """MMS_RANK_TIES_LIBSTDCXX: buckets of more than 16 items whose only cross-label ties are between +0.0 and -0.0
    (and other zeros) carry the bits of g++'s std::sort, MAP / MRR and AUC."""
    from mms_answer_selection_amd import capi
    r = rng(n + 31)
    sizes = random_groups(r, n, 17, 41)
    group, label = items_from_sizes(r, sizes, lambda s: (r.uniform(size=s) < 0.4).astype(np.float32))
    score = nonzero_scores(r, n)
    zero = r.uniform(size=n) < 0.4
    # a zero's sign follows its label (+0.0 for label 1 in even buckets, for label 0 in odd ones): zeros of one sign
    # share a label, so the only cross-label ties are between +0.0 and -0.0
    flip = np.trunc(group).astype(np.int64) % 2 == 1
    score[zero] = np.where((label[zero] == 1) != flip[zero], np.float32(0.0), np.float32(-0.0))
    prob = make_prob(r, score)
    # AUC's one bucket: +0.0 for every label-1 zero, -0.0 for every label-0 zero
    score_auc = score.copy()
    score_auc[zero] = np.where(label[zero] == 1, np.float32(0.0), np.float32(-0.0))
    prob_auc = make_prob(r, score_auc)
    m_ref, eff_ref = oracle.map_score(prob, label, group)
    rr_ref, _ = oracle.mrr_score(prob, label, group)
    auc_ref = oracle.auc_score(prob_auc, label)
    capi.set_rank_tie_mode("libstdcxx")
    try:
        m, rr, eff = capi.rank_map_mrr(dev(prob), dev(label), dev(group))
        auc = capi.rank_auc(dev(prob_auc), dev(label))
    finally:
        capi.set_rank_tie_mode("input")
    assert eff == eff_ref
    assert same_bits(m, m_ref), (m, m_ref)
    assert same_bits(rr, rr_ref), (rr, rr_ref)
    assert same_bits(auc, auc_ref), (auc, auc_ref)


# ---------------------------------------------------------------------------------------------------------------------
# every instantiation: the double twins at the ends of each size path, libstdc++ mode at its 16 / 17 threshold


def same_words(x, y):
    return np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64) or (np.isnan(x) and np.isnan(y))


def auc_f64(score, label):
    """auc_layer.cpp:119-134 for Dtype = double, distinct float scores, labels 0 / 1: every running sum is an integer
    below 2^53, so the double sum is the integer sum."""
    lab = label[np.argsort(-score.astype(np.float32), kind="stable")].astype(np.int64)
    high = np.cumsum(lab)
    total, H = int((high * (1 - lab)).sum()), int(high[-1])
    return np.float64(0) if H <= 0 else np.float64(total) / np.float64(H) / np.float64(lab.size - H)


@pytest.mark.parametrize("n,name", [(65, "rand13"), (512, "one"), (513, "rand13"), (2048, "one"), (2048, "singletons"),
                                    (2049, "rand13")])
def test_f64_at_the_ends_of_each_size_path(n, name, oracle, hiplib):
    """rank_small_kernel<0 / 1, double> at a padded size of 128 and at its largest input, rank_mid_kernel<0 / 1, double>
    at both ends (2,048 singleton groups fill the bucket-head array), the radix kernels in double at their smallest."""
    from mms_answer_selection_amd import capi
    r = rng(20 * n + len(name))
    group, label = layout(r, n, name)
    score = distinct_scores(r, n)
    prob, label, group = make_prob(r, score).astype(np.float64), label.astype(np.float64), group.astype(np.float64)
    m_ref, eff_ref = oracle.map_score(prob, label, group)
    rr_ref, _ = oracle.mrr_score(prob, label, group)
    m, rr, eff = capi.rank_map_mrr_f64(dev(prob), dev(label), dev(group))
    assert eff == eff_ref == int(bucket_counts(label, group)[0].sum())
    assert same_words(m, m_ref), (m, m_ref)
    assert same_words(rr, rr_ref), (rr, rr_ref)
    auc_ref = auc_f64(score, label)
    auc = capi.rank_auc_f64(dev(prob), dev(label))
    assert same_words(auc, auc_ref), (auc, auc_ref)
    if name == "rand13":       # the double front of libstdc++ mode, AUC's tail included: nothing ties, nothing changes
        capi.set_rank_tie_mode("libstdcxx")
        try:
            again = capi.rank_map_mrr_f64(dev(prob), dev(label), dev(group))
            auc_again = capi.rank_auc_f64(dev(prob), dev(label))
        finally:
            capi.set_rank_tie_mode("input")
        assert again[2] == eff and same_words(again[0], m) and same_words(again[1], rr) and same_words(auc_again, auc)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m", [16, 17])
def test_libstdcxx_mode_at_the_insertion_sort_threshold(m, dtype, oracle, hiplib):
    """Buckets of exactly m items, two score levels, labels mixed: at 16 std::sort is the stable insertion sort, at 17
    it is introsort, and a cross-label tie is re-sorted by rank_ties_emulate_kernel (the `m > 16` of the detect kernel)."""
    from mms_answer_selection_amd import capi
    r = rng(900 + m)
    group, label = items_from_sizes(r, [m] * 9, lambda s: r.permutation((np.arange(s) % 3 == 0).astype(np.float32)))
    score = r.choice(np.float32([0.25, 0.75]), group.size)
    prob, label, group = make_prob(r, score).astype(dtype), label.astype(dtype), group.astype(dtype)
    same = same_bits if dtype is np.float32 else same_words
    m_ref, eff_ref = oracle.map_score(prob, label, group)
    rr_ref, _ = oracle.mrr_score(prob, label, group)
    one = group == group[0]                                     # AUC's one bucket: the m items of one group
    p1, l1 = prob[one], label[one]
    auc_ref = oracle.auc_score(p1, l1)                          # (the oracle's AUC is float only)
    capi.set_rank_tie_mode("libstdcxx")
    try:
        got = (capi.rank_map_mrr if dtype is np.float32 else capi.rank_map_mrr_f64)(dev(prob), dev(label), dev(group))
        auc = (capi.rank_auc if dtype is np.float32 else capi.rank_auc_f64)(dev(p1), dev(l1))
    finally:
        capi.set_rank_tie_mode("input")
    assert got[2] == eff_ref == 9
    assert same(got[0], m_ref), (got[0], m_ref)
    assert same(got[1], rr_ref), (got[1], rr_ref)
    if dtype is np.float64:
        # auc = total / high / (count - high) with an integer total: the float oracle's value pins that integer (a
        # step of 1 in `total` moves the quotient by far more than a float ulp at m <= 17), and with it the double
        H, F = int(l1.sum()), np.float32
        totals = [t for t in range(H * (m - H) + 1) if same_bits(F(t) / F(H) / F(m - H), auc_ref)]
        assert len(totals) == 1
        auc_ref = np.float64(totals[0]) / np.float64(H) / np.float64(m - H)
    assert same(auc, auc_ref), (auc, auc_ref)


# ---------------------------------------------------------------------------------------------------------------------
# the Layer mirror and the device-result entry point on the mid path with more than 1,024 buckets


def test_layers_and_device_results_mid_path_many_buckets(oracle, hiplib):
    from mms_answer_selection_amd import capi
    from mms_answer_selection_amd import layers as L
    L.lib()
    L.set_mode_gpu()
    n = 2000
    r = rng(2000)
    sizes = [2] * 500 + [1] * 1000
    sizes = list(np.array(sizes)[r.permutation(len(sizes))])
    group, label = items_from_sizes(r, sizes, one_pos_rest_neg(r))
    prob = make_prob(r, distinct_scores(r, n))
    cmap, _ = bucket_counts(label, group)
    assert cmap.size == 1500 and cmap[1024:].sum() > 100
    m_ref, eff_ref = oracle.map_score(prob, label, group)
    rr_ref, _ = oracle.mrr_score(prob, label, group)
    assert eff_ref == 500
    out = torch.full((2,), -1.0, device="cuda")
    eff = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    capi.rank_map_mrr_device(dev(prob), dev(label), dev(group), out, eff)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert int(eff.item()) == eff_ref and same_bits(o[0], m_ref) and same_bits(o[1], rr_ref), (o, m_ref, rr_ref)
    bufs = []
    for x in (prob, label, group):
        b = L.Blob(x.shape)
        b.data[...] = x
        bufs.append(b)
    for make, ref in ((L.MAP, m_ref), (L.MRR, rr_ref)):
        lay, top = make(), L.Blob()
        lay.SetUp(bufs, [top])
        lay.Forward(bufs, [top])
        assert same_bits(top.data.reshape(-1)[0], ref), (make.__name__, top.data.reshape(-1)[0], ref)


# ---------------------------------------------------------------------------------------------------------------------
# RankAccuracy at the edges of its reduction


def _rank_accuracy_both(oracle, a, b, lab):
    from mms_answer_selection_amd import capi
    got = capi.rank_accuracy(dev(a), dev(b), dev(lab))
    ref = oracle.rank_accuracy(a, b, lab)
    assert same_bits(got, ref), (a.size, got, ref)
    return got


def test_rank_accuracy_grid_stride_and_zero_labels(oracle, hiplib):
    """More than 1,024 x 1,024 items: 1,024 blocks, each thread strides more than once; labels -1 / 0 / 1 (a label
    0 never counts, :45)."""
    r = rng(23)
    n = 1024 * 1024 + 4099
    a = r.uniform(size=n).astype(np.float32)
    b = r.uniform(size=n).astype(np.float32)
    lab = r.choice(np.float32([-1, 0, 1]), n)
    got = _rank_accuracy_both(oracle, a, b, lab)
    want = np.count_nonzero(lab * (a - b) > 0)
    assert same_bits(got, np.float32(want) / np.float32(n))
    # label 0 only: nothing counts
    assert _rank_accuracy_both(oracle, a[:5000], b[:5000], np.zeros(5000, np.float32)) == 0.0


def test_rank_accuracy_just_below_2_24(oracle, hiplib):
    """Below 2^24 the reference's float running count is exact."""
    r = rng(24)
    n = 2 ** 24 - 3
    a = r.uniform(size=n).astype(np.float32)
    b = r.uniform(size=n).astype(np.float32)
    lab = r.choice(np.float32([-1, 0, 1]), n)
    lab[:3] = 1
    a[:3], b[:3] = 1, 0
    got = _rank_accuracy_both(oracle, a, b, lab)
    assert same_bits(got, np.float32(np.count_nonzero(lab * (a - b) > 0)) / np.float32(n))
    ones = np.ones(n, np.float32)
    assert _rank_accuracy_both(oracle, ones, np.zeros(n, np.float32), ones) == 1.0


def test_rank_accuracy_count_sticks_at_2_24(oracle, hiplib):
    """2^24 + 2^20 items, every one correct: the reference's float accumulator stops at 2^24
    (rank_accuracy_layer.cpp:45, 2^24 + 1 rounds to 2^24), so the accuracy is 2^24 / n, not 1."""
    n = 2 ** 24 + 2 ** 20
    ones = np.ones(n, np.float32)
    got = _rank_accuracy_both(oracle, ones, np.zeros(n, np.float32), ones)
    assert same_bits(got, np.float32(2 ** 24) / np.float32(n)) and got < 1
