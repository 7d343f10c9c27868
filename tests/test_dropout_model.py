"""CPU suite: tests/dropout_reference.py, the numpy restatement of include/mms_dropout.h that the library is compared
with, is itself pinned -- by Random123's published Philox4x32-10 vectors, by the keep fraction its words give, and by
the properties the header states (a word depends on the global index alone)."""
import os
import re

import numpy as np
import pytest

import dropout_reference as R
from conftest import ROOT


@pytest.mark.parametrize("ctr,key,want", R.KNOWN_ANSWERS)
def test_known_answers(ctr, key, want):
    got = tuple(int(v) for v in R.philox4x32_10(ctr, key))
    assert got == want, " ".join("%08x" % v for v in got)


def test_known_answers_are_the_headers():
    """the three vectors of the model are those the header prints"""
    txt = open(os.path.join(ROOT, "include", "mms_dropout.h")).read()
    rows = re.findall(r"ctr ((?:[0-9a-f]{8} ){4}) *key ((?:[0-9a-f]{8} ?){2}) *-> *((?:[0-9a-f]{8} ?){4})", txt)
    parsed = [tuple(tuple(int(w, 16) for w in part.split()) for part in row) for row in rows]
    assert parsed == [(tuple(c), tuple(k), tuple(o)) for c, k, o in R.KNOWN_ANSWERS]
    assert (R.M0, R.M1, R.W0, R.W1) == tuple(int(v, 16) for v in ("D2511F53", "CD9E8D57", "9E3779B9", "BB67AE85"))
    for v in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert v in txt, v


def test_vector_form_equals_the_scalar_form():
    """arrays of counters give what one counter at a time gives; a word is words()[g - offset] for every offset"""
    ctrs = np.array([[0, 0, 0, 0], [0xffffffff] * 4, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344],
                     [1, 2, 3, 4]], dtype=np.uint64)
    key = (0xa4093822, 0x299f31d0)
    together = np.stack(R.philox4x32_10(tuple(ctrs[:, j] for j in range(4)), key), 1)
    for row, c in zip(together, ctrs):
        assert tuple(int(v) for v in row) == tuple(int(v) for v in R.philox4x32_10(tuple(int(v) for v in c), key))
    whole = R.words(7, 3, 0, 64)
    for offset in (0, 1, 2, 3, 4, 5, 17):
        assert (R.words(7, 3, offset, 40) == whole[offset:offset + 40]).all(), offset
        assert R.word(7, 3, offset) == int(whole[offset])


def test_the_counter_carries_into_its_second_word():
    """g >> 2 crossing 2^32: ctr[0] wraps to 0 and ctr[1] becomes 1"""
    offset = 2 ** 34 - 2
    got = R.words(5, 9, offset, 8)
    before = np.stack(R.philox4x32_10((0xffffffff, 0, 9, 0), (5, 0)), 0).astype(np.uint32)
    after = np.stack(R.philox4x32_10((0, 1, 9, 0), (5, 0)), 0).astype(np.uint32)
    assert (got == np.concatenate([before[2:], after, R.words(5, 9, 2 ** 34 + 4, 2)])).all()
    top = (1 << 64) - 8                            # the last two groups of the index space
    assert (R.words(1, 2, top, 8)[4:] == np.stack(R.philox4x32_10((0xffffffff, 0x3fffffff, 2, 0), (1, 0)), 0)).all()


@pytest.mark.parametrize("ratio", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", range(8))
def test_keep_fraction(ratio, seed):
    """2^20 elements, sequence 0, offset 0: the kept share is within 4 sigma of 1 - ratio, sigma^2 = p (1 - p) / n"""
    n = 1 << 20
    keep = R.mask(n, ratio, seed, 0).mean()
    p = 1.0 - ratio
    sigma = (p * (1.0 - p) / n) ** 0.5
    print("ratio %.1f seed %d: keep %.6f, %.2f sigma" % (ratio, seed, keep, abs(keep - p) / sigma))
    assert abs(keep - p) <= 4.0 * sigma


def test_threshold_and_scale_per_element_type():
    assert R.threshold(0.5, np.float32) == (1 << 31, np.float32(2.0))
    assert R.threshold(0.5, np.float64) == ((2 ** 32 - 1) // 2, 2.0)
    thr, scale = R.threshold(0.1, np.float32)
    assert thr == int(np.float32(0.1) * np.float32(2.0 ** 32)) == 429496736      # 2^32 * float(0.1), exact
    assert scale == np.float32(1.0 / (1.0 - float(np.float32(0.1)))) and scale.dtype == np.float32
    thr, scale = R.threshold(2.0 ** -24, np.float32)
    assert thr == 256 and scale == np.float32(1.0 / (1.0 - 2.0 ** -24))
    assert R.threshold(2.0 ** -24, np.float64)[0] == 255                          # (2^32 - 1) * 2^-24, truncated
    for bad in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert R.threshold(bad, np.float32) is None and R.threshold(bad, np.float64) is None, bad


def test_forward_is_the_references_arithmetic():
    x = np.array([1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 3.0] * 8, dtype=np.float32)
    m = R.mask(x.size, 0.5, 11, 4)
    assert 0 < m.sum() < x.size
    y = R.forward(x, 0.5, 11, 4)
    for xi, mi, yi in zip(x, m, y):
        want = np.float32(np.float32(xi * np.float32(mi)) * np.float32(2.0)) if np.isfinite(xi) or mi else np.float32("nan")
        assert (np.isnan(want) and np.isnan(yi)) or (want == yi and np.signbit(want) == np.signbit(yi)), (xi, mi, yi)
    assert (R.forward(x, 0.5, 11, 4, phase=R.TEST).view(np.uint32) == x.view(np.uint32)).all()
    assert R.forward(x.astype(np.float64), 0.5, 11, 4).dtype == np.float64
    # a shard at offset k computes what the whole computes there
    whole = R.forward(x, 0.1, 3, 8)
    for k in (1, 2, 3, 4, 13):
        assert (R.forward(x[k:], 0.1, 3, 8, offset=k).view(np.uint32) == whole[k:].view(np.uint32)).all(), k
