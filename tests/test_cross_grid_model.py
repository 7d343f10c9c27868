"""tests/cross_grid_model.py proved on the CPU: its constants are the source's, its shape lists reach every instantiation of the fp32
word-grid kernels (25 + 25 forward tiles, seven lane widths in two arithmetics, the tiled kernel split and unsplit in both, the plain
kernel), every listed shape takes the route written next to it, and every routing threshold has a shape on either side."""
import re

import numpy as np

import cross_grid_model as gm


def test_constants_match_the_source():
    txt = {f: gm.source_text(f) for f in (gm.GRID, gm.LANE)}
    assert re.search(r"constexpr int kBwdDC = %d;" % gm.BWD_DC, txt[gm.GRID]) and gm.BWD_DC == 32
    # the named constants, each defined once, hold what the shape tables were chosen for
    assert dict(kBwdDC=gm.BWD_DC, kMaxTile=gm.MAX_TILE, kFill=gm.FILL, kImageD=gm.IMAGE_D, kLdsBytes=gm.LDS_BYTES) == gm.RESTATED
    for name in gm.RESTATED:
        assert len(re.findall(r"constexpr \w+ %s =" % name, txt[gm.GRID])) == 1, name
    # the lane kernel's source restates the chunk width its figures were taken at, and holds it to the definition
    assert re.findall(r"constexpr \w+ (k\w+) =", txt[gm.LANE]) == ["kBwdDC"]
    assert gm.IMAGE_MIN_N == 1024 and gm.gcd64(gm.IMAGE_D) <= 8, "rows 8 apart of the pair image fall in different banks"
    blanks = lambda s: " ".join(s.replace("\\\n", " ").split())          # runs of blanks and a macro's line continuations apart
    # the instantiation lists of the two forward kernels ("tile table row", "tile table": every <J, K> in 1..5, one helper used by both
    # tables) are among the lines
    for what, (source, pattern, want) in gm.source_lines().items():
        found = re.findall(pattern, txt[source])
        assert len(found) == 1, "%s: %d lines of %s match %r" % (what, len(found), source, pattern)
        assert blanks(found[0]) == blanks(want), "%s: %s now reads %r, the model restates %r" % (what, source, blanks(found[0]), want)
    assert txt[gm.GRID].count("#define MMS_TILES5X5(") == 1 and "MMS_TILES5" not in txt[gm.LANE]
    assert gm.bwd_lane_lds(True, 20, 40) == 16016 and gm.bwd_lane_lds(False, 138, 48) == 65296
    assert gm.bwd_tiled_lds(1, 40, 40) == 1600 * 20 + 80 * 33 * 4 + 16 and gm.bwd_tiled_lds(0, 40, 40) == 1600 * 16 + 80 * 33 * 4 + 16


def test_forward_lists_reach_every_tile():
    want = [(j, k) for j in range(1, 6) for k in range(1, 6)]
    assert [gm.fwd_route(*s) for s in gm.GENERIC_TILES] == [("fwd", j, k) for j, k in want]
    assert [gm.fwd_route(*s) for s in gm.IMAGE_TILES] == [("image", j, k) for j, k in want]
    assert [gm.fwd_route(*s, aligned=False) for s in gm.IMAGE_TILES] == [("fwd", j, k) for j, k in want]
    assert [gm.fwd_route(*s, aligned=False) for s in gm.GENERIC_TILES] == [gm.fwd_route(*s) for s in gm.GENERIC_TILES]
    for s, route in gm.FWD_EDGES.items():
        assert gm.fwd_route(*s) == route, s
    assert len(gm.FWD) == 53 == len(set(gm.FWD))
    # ragged remainders in both directions, every accumulator layout of CrossAcc, every chunk shape of the generic staging
    assert any(s[1] % 8 and s[2] % 8 for s in gm.GENERIC_TILES) and {s[3] for s in gm.GENERIC_TILES} == {3, 8, 33, 34}
    for (N, W1, W2, D), (rj, rk) in zip(gm.GENERIC_TILES, want):
        assert 8 * (rj - 1) < W1 <= 8 * rj and 8 * (rk - 1) < W2 <= 8 * rk and gm.fwd_tile(N, W1, W2)[2:] == (1, 1)
    assert any(s[0] % 2 for s in gm.IMAGE_TILES) and any(s[1] != s[2] for s in gm.IMAGE_TILES)


def test_backward_shapes_take_the_routes_written_next_to_them():
    for s, (reference, fp32) in gm.BWD.items():
        assert gm.bwd_route(*s, exact=True) == reference, (s, "reference", gm.bwd_route(*s, exact=True))
        assert gm.bwd_route(*s, exact=False) == fp32, (s, "fp32", gm.bwd_route(*s, exact=False))
    for small, large, axis in gm.EDGE_PAIRS:
        assert small in gm.BWD and large in gm.BWD
        d = [i for i in range(4) if small[i] != large[i]]
        assert d == [{"N": 0, "W1": 1, "D": 3}[axis]] and large[d[0]] == small[d[0]] + 1
    differ = [gm.BWD[s][0] != gm.BWD[l][0] for s, l, _ in gm.EDGE_PAIRS]
    assert differ == [True] * 6 + [False], "every pair but the last (138 / 139 rows: plain on both sides) changes kernel in reference mode"
    assert gm.BWD[gm.EDGE_PAIRS[-1][0]][1] != gm.BWD[gm.EDGE_PAIRS[-1][1]][1], "138 / 139 rows change kernel in fp32 mode"


def test_backward_union_covers_every_instantiation_and_threshold():
    for exact in (True, False):
        routes = {r[0 if exact else 1] for r in gm.BWD.values()}
        assert {r[1] for r in routes if r[0] == "lane"} == set(gm.LANE_WIDTHS), "lane widths, exact=%s" % exact
        assert {("tiled", exact, "split"), ("tiled", exact, "unsplit"), ("plain",)} <= routes
        assert gm.one_per_route(exact) and {gm.BWD[s][0 if exact else 1] for s in gm.one_per_route(exact)} == routes
    # either side of each LDS cap: one row more and the tables no longer fit
    for exact, cap, below, above in ((True, 16, (20, 40), (21, 40)), (True, 16, (17, 48), (18, 48)), (True, 16, (102, 8), (103, 8)),
                                     (False, 64, (138, 48), (139, 48))):
        assert gm.bwd_lane_lds(exact, *below) <= cap * 1024 < gm.bwd_lane_lds(exact, *above)
        lo, hi = [next(s for s in gm.BWD if s[1:3] == w) for w in (below, above)]
        assert gm.bwd_route(*lo, exact=exact)[0] == "lane" and gm.bwd_route(*hi, exact=exact)[0] != "lane"
    # N, D, the split edge, columns below the wave, widths that are not instantiated, a chunk of 4 after 28 whole ones
    assert gm.bwd_route(511, 8, 16, 50, True)[0] == "tiled" and gm.bwd_route(512, 8, 16, 50, True)[0] == "lane"
    assert gm.bwd_route(512, 8, 16, 64, True)[0] == "lane" and gm.bwd_route(512, 8, 16, 65, True)[0] == "tiled"
    assert {(511, 5, 7, 50), (512, 5, 7, 50), (520, 8, 16, 1), (520, 8, 16, 3), (512, 8, 12, 50), (40, 9, 7, 900)} <= set(gm.BWD)
    assert 511 * 2 == 1022 and 512 * 2 == 1024 and (900 + 31) // 32 == 29 and 900 % 32 == 4
    assert any(s[1] == 1 for s in gm.BWD) and any(s[2] == 1 for s in gm.BWD) and any(s[1] % 2 for s in gm.BWD if gm.BWD[s][1][0] == "lane")
    assert max(N * W1 * W2 * D for (N, W1, W2, D) in gm.BWD) < 28e6, "the oracle's largest case"


def test_inputs_hold_the_degenerate_pairs_and_extensions_share_their_rows():
    for shape in ((1024, 13, 22, 33), (512, 1, 16, 50), (512, 16, 1, 50)):
        q, a, dT = gm.inputs(shape)
        assert q.shape == (shape[0], shape[1], shape[3]) and a.shape == (shape[0], shape[2], shape[3]) and dT.shape == (shape[0], 1) + shape[1:3]
        eq = [n for n in range(shape[0]) if (a[n, -1] == q[n, -1]).all()]
        assert eq == [1, shape[0] - 1] == gm.degenerate_pairs(shape[0])
    for small, large, axis in gm.EDGE_PAIRS:
        q, a, dT = gm.inputs(small)
        Q, A, G = gm.extended(small, large, axis)
        N, W1, W2, D = small
        assert Q.shape == (large[0], large[1], large[3]) and A.shape == (large[0], large[2], large[3]) and G.shape == (large[0], 1) + large[1:3]
        assert (Q[:N, :W1, :D] == q).all() and (A[:N, :, :D] == a).all() and (G[:N, :, :W1] == dT).all()
        if axis == "W1":
            assert not G[:, :, W1:].any() and Q[:, W1:].any()
        if axis == "D":
            assert (Q[:, :, D:] == Q[:, :1, D:]).all() and (A[:, :, D:] == Q[:, :1, D:]).all() and Q[:, :, D:].any()


def test_term_budget_is_the_sum_of_the_terms_magnitudes(oracle):
    shape = (3, 5, 7, 9)
    c = gm.backward_case(oracle, shape)
    mag_q, mag_a = gm.term_budget(c["q"], c["a"], c["top"], c["dT"])
    T, g = c["top"].astype(np.float64)[:, 0], c["dT"].astype(np.float64)[:, 0]
    tt = (g * T ** 3 / (T - 1 + 1e-9))[..., None] * (c["q"].astype(np.float64)[:, :, None] - c["a"].astype(np.float64)[:, None])
    assert np.allclose(mag_q, np.abs(tt).sum(2), rtol=1e-12) and np.allclose(mag_a, np.abs(tt).sum(1), rtol=1e-12)
    assert c["top"][1, 0, -1, -1] == 1.0 and c["top"][2, 0, -1, -1] == 1.0 and np.isfinite(mag_q).all()
    # the oracle's own fp32 gradient sits inside the fp32 mode's bound around the fp64 sum, and the bound notices one wrong term
    gm.assert_fp32_mode(c["dq"], tt.sum(2), mag_q)
    gm.assert_fp32_mode(c["da"], -tt.sum(1), mag_a)
    wrong = c["dq"].copy()
    wrong[0, 2, 3] -= np.float32(tt[0, 2, 0, 3])
    try:
        gm.assert_fp32_mode(wrong, c["dq"], mag_q, north_star=False)
    except AssertionError:
        return
    raise AssertionError("a dropped term passed the bound")
