"""Conditions on the inputs of tests/test_gpu_embed_segments.py, checked with the reference chain only (no GPU): the
planted segment lengths are delivered exactly, every summation path of csrc/embed.hip is entered, and at N = 300 the
reference's bits tell a wrong order, a dropped row and a doubled row from the right result.  A seed that fails one of
these is replaced (tests/embed_segments.py CASES); the conditions stay."""
import numpy as np
import pytest

import embed_segments as es


@pytest.mark.parametrize("lengths,M,K", [((1, 2, 9, 40), 60, 20), ((5,), 5, 1), ((), 16, 2), (es.FLOAT_LENGTHS, 4500, 600),
                                         (es.DOUBLE_LENGTHS, 4200, 600)])
def test_planted_index_delivers_the_histogram(lengths, M, K):
    index, planted = es.planted_index(lengths, M, K, 7)
    assert index.shape == (M,) and index.min() >= 0 and index.max() < K
    assert planted.size == len(lengths) == np.unique(planted).size
    seg = es.segment_lengths(index)
    assert [seg[int(i)] for i in planted] == list(lengths)
    assert all(R <= 8 for i, R in seg.items() if i not in set(planted.tolist()))
    again, _ = es.planted_index(lengths, M, K, 7)
    assert (again == index).all()                                  # a function of the seed
    if len(lengths) and max(lengths) >= 40:                        # shuffled: the long segment is not one run of rows
        rows = np.flatnonzero(index == planted[int(np.argmax(lengths))])
        assert rows[-1] - rows[0] >= len(rows)


def test_telescoping_diff_keeps_every_running_sum_small():
    index, planted = es.planted_index((300, 2, 1), 400, 40, 3)
    for dtype in (np.float32, np.float64):
        top_diff, ids, y0 = es.telescoping_diff(index, 5, dtype, 4)
        assert top_diff.dtype == dtype and top_diff.shape == (400, 5) and (ids == np.unique(index)).all()
        X = top_diff[index == planted[0]]
        P = es.reference_prefix(X, y0[np.searchsorted(ids, planted[0])])
        assert np.abs(P).max() < 6.0                               # y ~ N(0, 1); a plain N(0, 1) walk reaches ~17 here
        assert np.abs(np.cumsum(X.astype(np.float64), 0)[-1]).max() < 12.0


def test_swapped_chains_is_the_chain_with_two_rows_exchanged():
    r = np.random.default_rng(5)
    X = r.standard_normal((11, 4)).astype(np.float32)
    a0 = r.standard_normal(4).astype(np.float32)
    P = es.reference_prefix(X, a0)
    A = es.swapped_chains(X, P, np.arange(10))
    for s in range(10):
        Y = X.copy()
        Y[[s, s + 1]] = Y[[s + 1, s]]
        assert (es.reference_prefix(Y, a0)[-1].view(np.uint32) == A[s].view(np.uint32)).all()
    few = es.swapped_chains(X, P, np.array([2, 9]))
    assert (few.view(np.uint32) == A[[2, 9]].view(np.uint32)).all()
    assert es.swaps_to_check(800, 256).size == 799
    far = es.swaps_to_check(2400, 256)
    assert far.size < 100 and {254, 255, 256, 2302, 2303, 2304, 2398} <= set(far.tolist())


@pytest.mark.parametrize("name", list(es.CASES))
def test_cases_enter_every_length_class(name):
    c = es.make_case(name)
    CH = es.seg_chunk(c["dtype"])
    seg = es.segment_lengths(c["index"])
    assert [seg[int(i)] for i in c["planted"]] == list(c["lengths"])
    assert max(R for i, R in seg.items() if i not in set(c["planted"].tolist())) <= 8
    hist = es.class_histogram(c["index"], CH)
    print("%s (CH = %d): segments per length class %s" % (name, CH, hist))
    assert all(hist[k] > 0 for k in es.CLASSES), hist
    have = set(c["lengths"])
    # both sides of every boundary between two paths; a last chunk of 8k, of 8k + 1 and of one row
    assert {1, 8, 9, 32, 33, CH - 1, CH, CH + 1, CH + 8, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH + 1} <= have
    assert (c["M"] <= es.PREP_MAX) == ("M4000" in name or "M2200" in name)
    if c["dtype"] == np.float32:                                   # the pair calls: segments that span both layers
        across = es.straddlers(c["index"], c["planted"], es.PAIR_CUT)
        assert len(across) >= 5 and int(c["planted"][-1]) in across
    assert c["wd0"].all() and c["bd0"].all()                       # the diffs accumulate: no zero start value


@pytest.mark.parametrize("name", es.WITNESS_CASES)
def test_the_reference_bits_see_order_loss_and_repetition(name):
    c = es.make_case(name)
    ws = es.order_witness(c["index"], c["top_diff"], c["wd0"], c["planted"])
    assert [w["R"] for w in ws] == list(c["lengths"])
    print("%s: smallest words changed of %d: swap %d, drop_last %d, add_twice %d" % (
        name, c["N"], min(w["swap"] for w in ws if w["R"] >= 2), min(w["drop_last"] for w in ws),
        min(w["add_twice"] for w in ws)))
    for w in ws:
        assert w["drop_last"] >= 1 and w["add_twice"] >= 1, w
        if w["R"] >= 2:
            assert w["swap"] >= 1, w
        else:
            assert w["swap"] is None
