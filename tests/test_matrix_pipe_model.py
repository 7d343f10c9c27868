"""The accuracy helper checks itself, on the CPU: the generators give the planes they claim, the plane probes separate
a kernel that loses ONE kept plane product from a correct one at every output element, the suite's 1e-5 max-abs check does
not (the gap tests/test_gpu_matrix_pipe_accuracy.py closes), and power-of-two scaling commutes with the model."""
import numpy as np
import pytest

import matrix_pipe_model as mp
from util import TOL, assert_close, rng

# (N_out, K) of the probed products: every (K1, K2) of the GPU module's shapes, forward (K2, K1) and dq (K1, K2)
PROBE_NK = [(300, 300), (304, 52), (52, 304), (160, 64), (64, 160), (8, 24), (24, 8), (128, 96), (96, 128), (72, 200), (200, 72)]
PROBE_NK_HALF = [(304, 304), (160, 64), (64, 160), (8, 24), (24, 8), (128, 96), (96, 128), (72, 200), (200, 72)]


def test_bf16_rne_matches_definition():
    r = rng(1)
    x = (r.standard_normal(20000) * np.exp2(r.integers(-40, 40, 20000))).astype(np.float32)
    got = mp.bf16_rne(x).astype(np.float64)
    x64 = x.astype(np.float64)
    ulp = np.exp2(np.floor(np.log2(np.abs(x64))) - 7)
    lo = np.floor(x64 / ulp) * ulp
    hi = lo + ulp
    want = np.where(x64 - lo < hi - x64, lo, np.where(x64 - lo > hi - x64, hi, np.where(np.round(lo / ulp) % 2 == 0, lo, hi)))
    assert (got == want).all()
    # ties go to even
    assert mp.bf16_rne(np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]


def test_split_is_exact_on_random_data():
    r = rng(2)
    x = (r.standard_normal(50000) * 0.4).astype(np.float32)
    h, m, l = mp.split3(x)
    assert ((h.astype(np.float64) + m + l) == x).all()
    for p in (h, m, l):
        assert (mp.bf16_rne(p) == p).all()


@pytest.mark.parametrize("half", [False, True])
def test_probe_values_split_into_the_planes_they_were_built_from(half):
    x, H, M, L = mp.probe_values(rng(3), (4000,), half=half)
    h, m, l = mp.split3(x)
    assert (h == H).all() and (m == M).all() and (l == L).all()
    assert (H != 0).all() and (M != 0).all()
    if half:
        assert (l == 0).all(), "a half operand has a zero third plane"
        assert (x.astype(np.float16).astype(np.float32) == x).all()
    else:
        assert (L != 0).all()
    # the weights the derivation of the bar rests on
    ax = np.abs(x.astype(np.float64))
    assert (ax < 1.26).all() and (ax > 0.99).all()
    if not half:
        assert (np.abs(L) >= 1.5 * 2.0 ** -18).all() and (np.abs(M) >= 1.5 * 2.0 ** -9).all()
    else:
        assert (np.abs(M) == 3 * 2.0 ** -10).all()


def _probe(r, n_out, K, a_half):
    rows = 2 * K + 3
    vals = mp.probe_values(r, (rows,), half=a_half)[0]
    A = mp.one_per_row(vals, K)
    B = mp.probe_values(r, (K, n_out))[0]
    return A, B


@pytest.mark.parametrize("kstep", [16, 32])
@pytest.mark.parametrize("a_half", [False, True])
def test_probes_meet_the_bar_and_every_lost_term_misses_it_everywhere(a_half, kstep):
    r = rng(4)
    for n_out, K in (PROBE_NK_HALF if a_half else PROBE_NK):
        A, B = _probe(r, n_out, K, a_half)
        C64, D = mp.reference(A, B)
        assert (D > 0).all()
        e, _ = mp.componentwise_error(mp.model_product(A, B, a_half=a_half, kstep=kstep), C64, D)
        assert e <= mp.BAR, (n_out, K, e)
        for term in (mp.TERMS_HALF_A if a_half else mp.TERMS):
            C = mp.model_product(A, B, drop=term, a_half=a_half, kstep=kstep)
            rel = np.abs(C - C64) / D
            assert rel.min() >= 2 * mp.BAR, "lost %s at (N, K) = %s: smallest error %.3g" % (term, (n_out, K), rel.min())
            assert rel.min() >= mp.LOST_TERM_MIN - mp.BAR
            i = np.arange(A.shape[0])
            msg = mp.name_lost_term(A[i, i % K][:, None], B[i % K, :], C, a_half)
            assert "a.%s x b.%s" % term in msg and "1.0" in msg, "the message names the plane: " + msg


def test_half_by_half_probe_pins_its_terms():
    """The fp16-storage weight gradient: the A side (q) has two planes, the B side is dT * a -- three planes when dT is a
    probe value and a a power of two, two when both operands are halves and dT a power of two."""
    r = rng(5)
    K, n_out = 70, 40
    A = mp.one_per_row(mp.probe_values(r, (2 * K + 3,), half=True)[0], K)
    Bh = mp.probe_values(r, (K, n_out), half=True)[0]
    C64, D = mp.reference(A, Bh)
    assert mp.componentwise_error(mp.model_product(A, Bh, a_half=True, kstep=32), C64, D)[0] <= mp.BAR
    for term in (("m", "m"), ("m", "h"), ("h", "m"), ("h", "h")):
        rel = np.abs(mp.model_product(A, Bh, drop=term, a_half=True, kstep=32) - C64) / D
        assert rel.min() >= 2 * mp.BAR, term


def test_split_k_slabs_keep_the_probe_exact():
    r = rng(6)
    N, K1, K2 = 2049, 52, 40
    qcol = mp.one_per_column(mp.probe_values(r, (K1,))[0], N)
    rows = mp.tn_rows(N, K1)
    assert rows.min() >= 0 and rows[0] == N - 1 and len(set((rows % 32).tolist())) == 32
    a = mp.probe_values(r, (N, K2))[0]
    C64, D = mp.reference(qcol.T, a)
    for chunk in (64, 96, 2080):
        e, _ = mp.componentwise_error(mp.model_product(qcol.T, a, kstep=32, chunk=chunk), C64, D)
        assert e <= mp.BAR
        rel = np.abs(mp.model_product(qcol.T, a, drop=("l", "h"), kstep=32, chunk=chunk) - C64) / D
        assert rel.min() >= 2 * mp.BAR


def test_tn_rows_reach_every_chunk():
    for N, K1 in [(2049, 300), (2125, 52), (2049, 64), (2048, 24), (2125, 96), (2085, 200), (2304, 300), (2304, 64), (2125, 304)]:
        rows = mp.tn_rows(N, K1)
        assert len(set(rows.tolist())) == K1 and rows.min() >= 0 and rows[0] == N - 1
        if K1 >= 32:
            assert len(set((rows % 32).tolist())) == 32, "every position of a 32-pair step"
            assert len(set((rows // 64).tolist())) == (N + 63) // 64, "every 64-pair chunk, the ragged last one included"
            assert len(set(((rows // 32) % 2).tolist())) == 2, "both steps of a two-step chunk"


@pytest.mark.parametrize("drop", [None, ("l", "h"), ("m", "m"), "three"])
def test_the_suites_max_abs_check_does_not_see_a_lost_term(drop):
    """The gap, kept as a test: on the suite's standard data (256 x 300 x 300, outputs of order 0.3) a product with one --
    or all three -- of the 2^-16 .. 2^-18 terms missing passes util.assert_close at 1e-5, so the probes must not be
    folded back into that check."""
    q, _, W, _ = mp.dense_inputs(rng(7), 256, 300, 300)
    C64, D = mp.reference(q, W)
    if drop == "three":
        pa, pb = mp.planes(q), mp.planes(W)
        C = np.zeros((256, 300), dtype=np.float32)
        for k0 in range(0, 300, 16):
            ks = slice(k0, min(k0 + 16, 300))
            for ta, tb in (("m", "h"), ("h", "m"), ("h", "h")):
                C = (C.astype(np.float64) + pa[ta][:, ks].astype(np.float64) @ pb[tb][ks].astype(np.float64)).astype(np.float32)
    else:
        C = mp.model_product(q, W, drop=drop)
    assert_close(C, C64, TOL, "mutated model")           # passes: that is the gap
    e, _ = mp.componentwise_error(C, C64, D)
    if drop is None:
        assert e <= 4e-7                                   # the model of the correct kernel (issue: ~1.3e-7)
    # on RANDOM dense data the componentwise metric alone does not convict a lost term either (signs average out):
    # only the probes do.  Recorded, not asserted beyond sanity.
    assert e < 1e-4


def test_power_of_two_scaling_commutes_with_the_model():
    r = rng(8)
    N, K1, K2 = 200, 52, 72
    q, _, W, _ = mp.dense_inputs(r, N, K1, K2)
    ri, sk, cj = r.integers(-30, 31, N), r.integers(-30, 31, K1), r.integers(-30, 31, K2)
    qs = np.ldexp(q, (ri[:, None] + sk[None, :]).astype(np.int32)).astype(np.float32)
    Ws = np.ldexp(W, (-sk[:, None] + cj[None, :]).astype(np.int32)).astype(np.float32)
    assert mp.all_planes_normal(qs) and mp.all_planes_normal(Ws)
    for kstep in (16, 32):
        C, Cs = mp.model_product(q, W, kstep=kstep), mp.model_product(qs, Ws, kstep=kstep)
        want = np.ldexp(C, (ri[:, None] + cj[None, :]).astype(np.int32)).astype(np.float32)
        assert (Cs.view(np.uint32) == want.view(np.uint32)).all()


def test_metric_is_componentwise_and_strict_about_zeros():
    A = np.float32([[1.0, 0.0], [0.0, 2.0 ** -20]])
    B = np.float32([[1.0, 0.0], [0.0, 1.0]])
    C64, D = mp.reference(A, B)
    good = (A.astype(np.float64) @ B).astype(np.float32)
    assert mp.componentwise_error(good, C64, D)[0] == 0.0
    bad = good.copy(); bad[1, 1] *= np.float32(1.0 + 2.0 ** -10)      # a small element, wrong by 1e-3: invisible to max-abs
    assert_close(bad, C64, TOL, "max-abs")
    e, idx = mp.componentwise_error(bad, C64, D)
    assert idx == (1, 1) and abs(e - 2.0 ** -10) < 1e-9
    leak = good.copy(); leak[0, 1] = 1e-30
    with pytest.raises(AssertionError):
        mp.componentwise_error(leak, C64, D)
    assert mp.half_ulp_of_half(np.float64(1.5)) == 2.0 ** -11 and mp.half_ulp_of_half(np.float64(0.75)) == 2.0 ** -12
