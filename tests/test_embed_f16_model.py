"""Conditions on the inputs of tests/test_gpu_embed_f16.py, checked with the reference chain only (no GPU): those
tests/test_embed_segments.py puts on its own inputs, on the half-valued rows of tests/embed_f16_model.py.  A seed that
fails one of these is replaced (embed_f16_model.CASES); the conditions stay."""
import numpy as np
import pytest

import embed_f16_model as em
import embed_segments as es


def test_inputs_are_halves_on_a_large_accumulator():
    c = em.make_case("f16-M4000-N51")
    assert c["top_diff"].dtype == np.float16 and c["wd0"].dtype == np.float32 and c["bd0"].dtype == np.float32
    assert np.isfinite(c["top_diff"]).all()
    a = np.abs(c["wd0"])
    assert a.min() >= 8192.0 and a.max() < 12288.0 + 1.0 and (c["wd0"] < 0).any() and (c["wd0"] > 0).any()
    w = em.widen(c["top_diff"])
    assert w.dtype == np.float32 and (w.astype(np.float16).view(np.uint16) == c["top_diff"].view(np.uint16)).all()
    # the point of the large accumulator (ulp 2^-10): a half below 1 is a multiple of 2^-11 or finer and |N(0, 1)| < 1 for
    # 68 % of the draws -- half of those in [0.5, 1) round, three in four of those in [0.25, 0.5), ...: about 45 % of all
    rounds = (c["wd0"][:100].astype(np.float64) + w[:100].astype(np.float64)) != (c["wd0"][:100] + w[:100]).astype(np.float64)
    print("adds that round: %.1f %%" % (100.0 * rounds.mean()))
    assert rounds.mean() > 0.35


def test_half_rounded_telescoping_rows_would_not_pin_the_order():
    """Why es.telescoping_diff is not reused: on its half-rounded rows an adjacent swap can change no word at all."""
    index, planted = es.planted_index(em.LENGTHS, 4000, em.K, 5101)
    top_diff, ids, y0 = es.telescoping_diff(index, 300, np.float32, 5151)
    wd0 = np.zeros((em.K, 300), np.float32)
    wd0[ids] = y0.astype(np.float16).astype(np.float32)
    ws = es.order_witness(index, top_diff.astype(np.float16).astype(np.float32), wd0, planted)
    least = min(w["swap"] for w in ws if w["R"] >= 2)
    print("half-rounded telescoping rows: smallest swap witness %d words of 300" % least)
    assert least < 3


@pytest.mark.parametrize("name", list(em.CASES))
def test_cases_enter_every_length_class(name):
    c = em.make_case(name)
    CH = em.CH
    assert CH == es.seg_chunk(np.float32)                          # the half instantiation adds in fp32, 256-row chunks
    seg = es.segment_lengths(c["index"])
    assert [seg[int(i)] for i in c["planted"]] == list(c["lengths"])              # the histogram is exact
    assert max(R for i, R in seg.items() if i not in set(c["planted"].tolist())) <= 8
    hist = es.class_histogram(c["index"], CH)
    print("%s (CH = %d): segments per length class %s" % (name, CH, hist))
    assert all(hist[k] > 0 for k in es.CLASSES), hist
    have = set(c["lengths"])
    assert {1, 8, 9, 32, 33, CH - 1, CH, CH + 1, CH + 8, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH + 1} <= have
    assert (c["M"] <= es.PREP_MAX) == ("M4000" in name)
    across = es.straddlers(c["index"], c["planted"], es.PAIR_CUT)  # the pair calls: segments that span both layers
    assert len(across) >= 5 and int(c["planted"][-1]) in across
    assert c["wd0"].all() and c["bd0"].all()                       # the diffs accumulate: no zero start value


@pytest.mark.parametrize("name", em.WITNESS_CASES)
def test_the_reference_bits_see_order_loss_and_repetition(name):
    c = em.make_case(name)
    ws = es.order_witness(c["index"], em.widen(c["top_diff"]), c["wd0"], c["planted"])
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
