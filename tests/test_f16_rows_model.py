"""tests/f16_rows_model.py proved on the CPU: the shape table reaches every reachable (family, bwd, NIT) cell of the fp16-storage
kernels and every boundary its comments name; the half bracket is the set of halves a value within the bar can round to, pins
at least 99 % of every dense case's gradient elements and admits the CPU oracle's own half-cast gradient; the adversarial rows
still defeat the 32-lane window after rounding to half.  A shape dropped from the table fails here."""
import numpy as np
import pytest

import cosine_model as cm
import f16_rows_model as fm

DENSE = [(f, s) for f in ("tree", "cosine") for s in fm.TABLE[f]]      # the families held to a bracket
dense_id = lambda c: "%s-%s" % (c[0], fm.shape_id(c[1]))


def test_routing_restated():
    assert fm.f16_rows_ok(8) and fm.f16_rows_ok(2048) and not fm.f16_rows_ok(12) and not fm.f16_rows_ok(2056) and not fm.f16_rows_ok(4)
    for which in ("q", "a"):
        assert not fm.f16_rows_ok(512, **{which: 8}) and not fm.f16_rows_ok(512, bwd=True, **{which: 8})
    for which in ("dq", "da"):
        assert fm.f16_rows_ok(512, **{which: 8}), "the forward-only call takes no " + which
        assert not fm.f16_rows_ok(512, bwd=True, **{which: 8})
    assert [fm.wave_pairs(D) for D in (8, 400, 408, 2048)] == [2, 2, 1, 1]
    assert [fm.family(D) for D in (8, 400, 408, 2048)] == ["wave2", "wave2", "lanechain", "lanechain"]
    assert fm.family(8, "tree") == fm.family(2048, "tree") == "tree"
    assert [fm.nit("wave2", D) for D in (8, 256, 264, 400)] == [1, 1, 2, 2]
    for fam in ("lanechain", "tree", "cosine"):
        assert [fm.nit(fam, D) for D in (8, 512, 520, 1024, 1032, 1536, 1544, 2048)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [fm.npad(D) for D in (8, 384, 304, 400, 1536, 1024, 2048)] == [1, 0, 2, 2, 0, 2, 1]
    assert fm.PAIRS_PER_WG == dict(tree=4, wave2=8, lanechain=8, cosine=4)


def test_table_reaches_every_reachable_cell():
    every = {(f, b, n) for f in fm.TABLE for b in (False, True) for n in (1, 2, 3, 4)}
    assert fm.REACHABLE | fm.UNREACHABLE == every and not fm.REACHABLE & fm.UNREACHABLE
    missing = sorted(fm.REACHABLE - fm.table_cells())
    assert not missing, "no shape of the table runs %s" % (missing,)
    assert not fm.table_cells() & fm.UNREACHABLE
    for fam, shapes in fm.TABLE.items():
        for (N, D) in shapes:
            assert N >= 1 and fm.f16_rows_ok(D) and (fam in ("tree", "cosine") or fm.family(D) == fam), (fam, N, D)
    assert all(fm.family(D) == "wave2" for D in fm.ADVERSARIAL_D)
    assert all(fam in ("tree", "cosine") or fm.family(D) == fam for fam, D in fm.EDGE_D.items())
    assert fm.nit("lanechain", fm.EDGE_D["lanechain"]) == 3 and fm.nit("cosine", fm.EDGE_D["cosine"]) == 3


def test_table_holds_every_boundary():
    D8s = {fam: {(2 if fam == "wave2" else 1) * (D // 8) for (_, D) in shapes} for fam, shapes in fm.TABLE.items()}
    # a full last trip against one lane (wave2: one lane per half-wave) in the next
    assert {64, 66} <= D8s["wave2"] and {64, 65, 128, 129, 192, 193, 256} <= D8s["lanechain"]
    assert {64, 65, 129, 192, 256} <= D8s["tree"] and {64, 65, 129, 192, 193, 256} <= D8s["cosine"]
    widths = {fam: {D for (_, D) in shapes} for fam, shapes in fm.TABLE.items()}
    assert 400 in widths["wave2"] and 408 in widths["lanechain"], "both sides of two pairs per wave | lane chain"
    assert any(fm.npad(D) == 0 for D in widths["wave2"]) and any(fm.npad(D) == 2 for D in widths["wave2"]) and any(fm.npad(D) == 1 for D in widths["wave2"])
    for fam, shapes in fm.TABLE.items():
        p = fm.PAIRS_PER_WG[fam]
        rem = {N % p for (N, _) in shapes}
        assert {0, 1, p - 1} <= rem, "%s: N %% %d misses one of 0, 1, %d" % (fam, p, p - 1)
        assert any(N > p for (N, _) in shapes), "%s: more than one workgroup" % fam
    assert (1, 304) in fm.WAVE2 and (1, 2048) in fm.LANECHAIN, "a lone pair: the mirrors"
    assert 2048 in widths["tree"] and 2048 in widths["cosine"] and 8 in widths["tree"] and 8 in widths["cosine"] and 8 in widths["wave2"]


def test_half_bracket_is_what_a_value_within_the_bar_rounds_to():
    f16 = lambda *v: np.array(v, np.float16)
    # a value next to a tie straddles, one away from it is pinned; rounding is monotone, so every v in between lands inside
    tie = 1.0 + 2.0 ** -11
    lo, hi = fm.half_bracket(np.array([tie, 1.0 + 2.0 ** -12, 70000.0, -70000.0, 65519.99, np.nan, 0.0, np.inf]), np.array([1.0, 1.0, 1.0, 1.0, 65519.0, 1.0, 0.0, 1.0]), 2.0 ** -20)
    assert list(lo[:2]) == [1.0, 1.0] and list(hi[:2]) == [np.float16(1.0 + 2.0 ** -10), 1.0]
    assert np.isposinf(lo[2]) and np.isposinf(hi[2]) and np.isneginf(lo[3]) and np.isneginf(hi[3])
    assert lo[4] == np.float16(65504) and np.isposinf(hi[4]), "65520 is where halves overflow"
    ok = fm.in_bracket(f16(1.0, 1.0, np.inf, -np.inf, np.inf, np.nan, -0.0, np.inf), lo, hi)
    assert ok.all()
    bad = fm.in_bracket(f16(1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, 65504.0, np.inf, np.nan, 0.0, 2.0 ** -24, 65504.0), lo, hi)
    assert not bad.any()
    assert fm.pinned_share(lo[:2], hi[:2]) == 0.5
    r = np.random.default_rng(9)
    ref = np.ldexp(r.standard_normal(20000), r.integers(-26, 14, 20000))
    b = 8 * cm.U24
    lo, hi = fm.half_bracket(ref, np.abs(ref), b)
    for t in (-1.0, -0.37, 0.0, 0.61, 1.0):
        assert fm.in_bracket((ref + t * b * np.abs(ref)).astype(np.float16), lo, hi).all()
    assert not fm.in_bracket((ref * (1 + 2.0 ** -9)).astype(np.float16), lo, hi)[np.abs(ref) > 2.0 ** -13].all()


@pytest.mark.parametrize("case", DENSE, ids=dense_id)
def test_dense_brackets_pin_and_admit_the_oracle(case, oracle):
    """Every dense case: the bar comes from the fp32 oracle's own error, the oracle's half-cast gradient is inside the bracket,
    and at least 99 % of the finite elements are pinned to ONE half."""
    fam, shape = case
    c = fm.dense_case(oracle, fam, shape)
    N, D = shape
    mags = np.abs(c["dT"]).ravel()
    if N >= 6:
        assert mags[mags > 0].max() / mags[mags > 0].min() >= 2.0 ** 12, "top_diff spans 2^-10 .. 2^10 across pairs"
    if fam != "cosine":
        assert N < 2 or (c["qh"][1] == c["ah"][1]).all()
        assert N < 3 or c["dT"][N - 1] == 0
        assert N < 2 or c["top"][1] == 1.0
    for k in ("dq", "da"):
        ref64, scale = c["ref"][k]
        assert np.isfinite(ref64).all() and np.isfinite(scale).all()
        bar = cm.dense_bar(c["e_o"][k])
        lo, hi = fm.check_bracket("oracle %s %s" % (k, case), c[k].astype(np.float16), ref64, scale, bar)
        share = fm.pinned_share(lo, hi)
        print("%s %s: e(oracle) = %.2f, bar %.2f (x 2^-24), pinned %.3f %%" % (k, dense_id(case), c["e_o"][k] / cm.U24, bar / cm.U24, 100 * share))
        assert share >= fm.PINNED_MIN
        assert bar < 2.0 ** -18, "the bar is a few fp32 roundings, far below a half's 2^-11"


@pytest.mark.parametrize("shape", fm.WAVE2 + fm.LANECHAIN, ids=fm.shape_id)
def test_ordered_dense_cases_exercise_the_contract(shape, oracle):
    """The ordered kernels are held to the oracle's bits; the data must make that mean something: gradients that are normal
    halves, subnormal halves and signed zeros all occur over the table, T == 1 on the a == q pair."""
    c = fm.dense_case(oracle, fm.family(shape[1]), shape)
    h = c["dq"].astype(np.float16)
    assert np.isfinite(h).all() and (h != 0).any()
    if shape[0] >= 3:
        assert not h[1].any() and not h[-1].any() and c["top"][1] == 1.0


@pytest.mark.parametrize("shape", fm.COSINE, ids=fm.shape_id)
def test_probes_are_exact_as_halves(shape, oracle):
    c = fm.probe_case(oracle, shape)
    assert (c["qh"].astype(np.float32) == c["q"]).all() and (c["ah"].astype(np.float32) == c["a"]).all()
    _, _, _, bound = cm.integer_sums(c["q"], c["a"], c["eq"], c["ea"])
    assert bound < 2 ** 24
    top, n0, n1 = cm.closed_form_forward(c["q"], c["a"], c["eq"], c["ea"])
    for got, want in ((c["top"], top), (c["n0"], n0), (c["n1"], n1)):
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    for k in ("dq", "da"):
        fm.check_bracket("oracle %s %s" % (k, shape), c[k].astype(np.float16), *c["ref"][k], cm.BAR_GRAD)
        assert np.isfinite(c[k].astype(np.float16)).all() and (c[k].astype(np.float16) != 0).mean() > 0.5


@pytest.mark.parametrize("D", fm.ADVERSARIAL_D)
def test_adversarial_rows_defeat_the_window(D):
    qh, ah = fm.adversarial_rows(D)
    assert qh.dtype == np.float16 and float(qh[0, 0, 1]) ** 2 < 2.0 ** -24 < float(qh[0, 0, 1]) ** 2 * 1.01
    for pair in (0, 1, 2, 3, 4):
        tree, seq = fm.first_segment_sums(qh, ah, pair)
        assert seq == 1.0, "the sequential sum swallows every small square"
        assert abs(int(tree.view(np.int32)) - int(seq.view(np.int32))) > fm.SPEC_WINDOW_32, (D, pair, tree, seq)


@pytest.mark.parametrize("fam", ["wave2", "lanechain", "tree", "cosine"])
def test_edge_rows_hold_the_edges(fam, oracle):
    c = fm.edge_case(oracle, fam)
    names, qh, ah, top = c["names"], c["qh"], c["ah"], c["top"].ravel()
    sub = np.abs(qh[3].astype(np.float64))
    assert ((sub >= 2.0 ** -24) & (sub < 2.0 ** -14)).all(), "subnormal halves only"
    assert np.isfinite(top[2]) and np.isfinite(top[3]) and np.isfinite(top[4]) and np.isfinite(top[6])
    assert np.isnan(top[1]) and np.isnan(top[5])
    over = np.abs(c["dq"][4].astype(np.float64)) >= 65520.0
    assert np.isfinite(c["dq"][4]).all() and over.any(), "top_diff 1e8: finite in fp32, some beyond half's range"
    with np.errstate(over="ignore"):
        assert np.isinf(c["dq"][4].astype(np.float16)[over]).all()
    if fam == "cosine":
        assert np.isnan(top[0]) and np.isnan(top[7]) and np.isnan(top[8]) and c["n0"][7] == 0 and c["n1"][8] == 0
        assert np.isnan(c["dq"][7]).all() and np.isnan(c["da"][8]).all()
    else:
        assert top[0] == 0.0 and top[7] == 1.0 and not c["dq"][8].any() and 0 < top[3] < 1
    assert names[9] == "clean" and np.isfinite(c["dq"][9]).all()
