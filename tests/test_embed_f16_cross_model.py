"""tests/embed_f16_cross_model.py proved on the CPU: the case table reaches both forward kernels and the norm kernel in both modes, the
image predicate turns on the table's 4-byte alignment and on nothing finer, the refusals are the library's own answers, and the data has
what the GPU test relies on (repeated ids, a pair of equal rows, ids that clamp and truncate, an exact probe table)."""
import ctypes

import numpy as np
import pytest

import cosine_model as cm
import embed_f16_cross_model as em
import f16_cross_model as xm


def test_the_cases_take_the_routes_written_next_to_them():
    assert len(em.CASES) == len(em.EXPECTED_ROUTE)
    for c, want in zip(em.CASES, em.EXPECTED_ROUTE):
        assert em.route_of(c) == want, em.case_id(c)
    assert em.GRAPH_CASE in em.CASES


def test_both_forward_kernels_and_the_norm_kernel_in_both_modes():
    cells = {k for c in em.CASES for m in (0, 1) for k in em.launches(m, *c[0], table=2 * c[2])}
    for m in (0, 1):
        assert {k[0] for k in cells if k[-1] == m and len(k) == 4} == {"generic", "image"}, "mode %d" % m
        assert ("generic", 5, 5, m) in cells and ("generic", 1, 1, m) in cells and ("image", 5, 5, m) in cells
    assert ("norm",) in cells
    for c in em.CASES:
        assert len(em.launches(1, *c[0], table=2 * c[2])) == 1 and len(em.launches(0, *c[0], table=2 * c[2])) == 3
        assert em.launches(0, *c[0])[:2] == (("norm",), ("norm",))


def test_the_image_predicate_and_its_alignment():
    """The gathering image kernel loads half2: a 4-byte aligned table is all it asks (its rows are 100 bytes), where the grid call's asks 16."""
    s = (1024, 40, 40, 50)
    assert [em.fwd_image_ok(*s, table=t) for t in (0, 2, 4, 6, 8, 12, 16, 18)] == [True, False, True, False, True, True, True, False]
    assert xm.fwd_image_ok(*s, q=4, a=4) is False and em.fwd_image_ok(*s, table=4) is True
    for bad in ((1023, 40, 40, 50), (1024, 40, 40, 48), (1024, 40, 41, 50), (1024, 48, 40, 50), (1024, 40, 40, 52)):
        assert not em.fwd_image_ok(*bad), bad
    assert em.fwd_image_ok(1024, 8, 8, 50) and em.fwd_route(1024, 8, 16, 50, table=2) == ("generic", 1, 2)
    # the tile of the route that takes over is launch_cross_fwd<_Float16>'s, whatever the alignment
    assert em.fwd_route(4, 40, 40, 50) == ("generic", 1, 1) and em.fwd_route(1024, 40, 40, 48) == ("generic", 5, 5)


REFUSALS = [(0, 4, 5, 7, 50, 97), (1, 4, 5, 7, 50, 97), (1, 2, 1, 1, 1, 1), (2, 4, 5, 7, 50, 97), (3, 4, 5, 7, 50, 97), (-1, 4, 5, 7, 50, 97),
            (2, -1, 5, 7, 50, 97), (1, -1, 5, 7, 50, 97), (1, 4, 0, 7, 50, 97), (0, 4, 5, -7, 50, 97), (1, 4, 5, 7, 0, 97), (1, 4, 5, 7, 50, 0),
            (0, 4, 5, 7, 50, -1), (1, 4, 5, 7, 50, (1 << 31) // 50 + 1), (1, 4, 5, 7, 50, (1 << 31) // 50), (1, 1 << 20, 64, 7, 50, 97),
            (1, 1 << 20, 7, 64, 50, 97), (1, 1 << 16, 200, 200, 1, 97)]


@pytest.mark.parametrize("name", ["mms_embed_simcross_forward_f16", "mms_embed_simcross_forward_f32"])
def test_refusal_is_the_librarys(name, hiplib):
    """Host-side answers, no launch: with N > 0 and every pointer NULL an accepted size reaches the pointer check (INVALID_ARG)."""
    f = getattr(hiplib, name)
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.c_void_p] * 8
    for t in REFUSALS:
        want = em.refusal(*t)
        assert f(*t, *([None] * 8)) == (want if want != em.OK else em.INVALID_ARG), (name, t)
        if want == em.OK:
            assert f(t[0], 0, *t[2:], *([None] * 8)) == em.OK, (name, t, "N == 0")
    assert {em.refusal(*t) for t in REFUSALS} == {em.OK, em.INVALID_ARG, em.UNSUPPORTED}
    assert em.refusal(1, 2, 1, 1, 1, 1) == em.OK and xm.refusal(1, 2, 1, 1, 1) == em.UNSUPPORTED, "W1 == W2 == 1 is served here only"


@pytest.mark.parametrize("case", em.CASES, ids=em.case_id)
def test_ids_have_what_the_gpu_test_relies_on(case):
    shape, K, _ = case
    N, W1, W2, D = shape
    iq, ia = em.word_ids(shape, K)
    assert iq.shape == (N, W1) and ia.shape == (N, W2) and iq.dtype == ia.dtype == np.float32
    both = np.concatenate([iq.ravel(), ia.ravel()])
    for v in (-3.0, K + 5.0, 2.7):
        assert (both == np.float32(v)).any(), "%r does not appear" % v
    cq, ca = em.clamp_ids(iq, K), em.clamp_ids(ia, K)
    assert cq.min() >= 0 and ca.min() >= 0 and cq.max() <= K - 1 and ca.max() <= K - 1
    assert (cq[N - 1] == min(2, K - 1)).all() and (ca[N - 1] == min(2, K - 1)).all(), "the last pair's rows are all one table row"
    for n in range(N):                           # a pair of two rows repeats an id only by scoring a row against itself: the last pair does
        ids = np.concatenate([cq[n], ca[n]])
        assert len(set(ids.tolist())) < ids.size or (W1 + W2 == 2 and n < N - 1), "pair %d has no repeated id" % n


def test_clamp_ids_is_the_c_conversion():
    ids = np.array([-3.0, -0.5, 0.0, 0.99, 2.7, 96.0, 96.9, 97.0, 102.0, 1e9, -1e9], np.float32)
    assert em.clamp_ids(ids, 97).tolist() == [0, 0, 0, 0, 2, 96, 96, 96, 96, 96, 0]
    assert em.clamp_ids(ids, 1).tolist() == [0] * ids.size


@pytest.mark.parametrize("case", em.CASES, ids=em.case_id)
def test_probe_tables_sum_exactly(case):
    """bias + table are integers of magnitude <= 6 at one power of two: 36 D <= 2304 < 2^24, every partial sum of any order is exact."""
    shape, K, _ = case
    D = shape[3]
    i = em.inputs(shape, K, "probe")
    assert i["table"].dtype == np.float16 and i["table"].shape == (K, D) and i["bias"].shape == (D,)
    nz = i["table"][i["table"] != 0].astype(np.float64)
    e = int(np.log2(np.abs(nz).min()))
    for x, lim in ((i["table"].astype(np.float64), 4), (i["bias"].astype(np.float64), 2), (i["table"].astype(np.float64) + i["bias"], 6)):
        k = np.ldexp(x, -e)
        assert (k == np.rint(k)).all() and np.abs(k).max() <= lim
    q, a = em.gathered_rows(i["table"], i["bias"], i["iq"], i["ia"])
    assert (q.astype(np.float64) == i["table"].astype(np.float64)[em.clamp_ids(i["iq"], K)] + i["bias"]).all(), "the fp32 add is exact"
    assert 36 * D < 2 ** 24 and (q != 0).any() and (a != 0).any()


def test_gathered_rows_without_a_bias_are_the_widened_halves():
    shape, K, _ = em.CASES[0]
    i = em.inputs(shape, K, "dense")
    q, a = em.gathered_rows(i["table"], None, i["iq"], i["ia"])
    assert q.dtype == np.float32 and (q.astype(np.float16).astype(np.float32) == q).all()
    assert (q[0, 0] == i["table"][0].astype(np.float32)).all() and (a[0, 0] == i["table"][K - 1].astype(np.float32)).all(), "-3.0 -> 0, K + 5 -> K - 1"
    qb, _ = em.gathered_rows(i["table"], i["bias"], i["iq"], i["ia"])
    assert (qb != q).any()


def test_references_are_shared_and_frozen(oracle):
    """One reference per (shape, K, kind, bias, mode), whatever the table's placement; Euclid's equal-row pair scores 1."""
    (shape, K, _), same = em.CASES[6], em.CASES[8]
    assert same[0] == shape and same[1] == K
    c = em.reference(oracle, 1, shape, K, "dense", True)
    assert em.reference(oracle, 1, same[0], same[1], "dense", True) is c and not c["top"].flags.writeable
    assert (c["top"][shape[0] - 1] == 1.0).all()
    c0 = em.reference(oracle, 0, (3, 5, 7, 33), em.K_MAIN, "dense", False)
    assert set(c0["e_o"]) == {"top", "n0", "n1"} and all(np.isfinite(v) for v in c0["e_o"].values()) and c0["bias"] is None
    assert np.isfinite(c0["top"]).all() and cm.dense_bar(c0["e_o"]["top"]) >= cm.DENSE_FLOOR
