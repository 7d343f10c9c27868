"""tests/f16_cross_model.py proved on the CPU: the shape tables reach every kernel instantiation of the fp16-storage word-grid calls
and every routing boundary; the brackets admit the CPU oracle's own half-cast gradient (the oracle stands in for the kernel) and
pin at least 99 % of every case's elements; the parity bar's bracket cannot; the edge inputs hold the edges; and the three calls are
declared in include/mms.h and exported by the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import cosine_model as cm
import f16_cross_model as xm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mms_simcross_forward_f16", "mms_simcross_backward_f16", "mms_simcross_forward_backward_f16")


def test_symbols_declared_and_exported():
    from mms_answer_selection_amd import build, capi
    header = open(os.path.join(ROOT, "include", "mms.h")).read()
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(int dist_mode, int N, int W1, int W2, int D," % s, header), "%s is not declared in include/mms.h" % s
        assert hasattr(lib, s), "%s is not exported by libmms_hip.so" % s
        assert s in capi.EXPORTED_SYMBOLS
    assert re.search(r"#define MMS_VERSION 212\b", header)
    for w in ("simcross_forward_f16", "simcross_backward_f16", "simcross_forward_backward_f16"):
        assert callable(getattr(capi, w))


def test_routing_restated():
    assert xm.refusal(1, 4, 5, 7, 50) == xm.OK and xm.refusal(0, 0, 5, 7, 50) == xm.OK
    assert xm.refusal(2, 4, 5, 7, 50) == xm.UNSUPPORTED and xm.refusal(1, 4, 1, 1, 50) == xm.UNSUPPORTED and xm.refusal(0, 4, 1, 2, 50) == xm.OK
    for bad in ((3, 4, 5, 7, 50), (-1, 4, 5, 7, 50), (1, -1, 5, 7, 50), (1, 4, 0, 7, 50), (1, 4, 5, -2, 50), (1, 4, 5, 7, 0), (1, 1 << 20, 64, 64, 64)):
        assert xm.refusal(*bad) == xm.INVALID_ARG, bad
    assert xm.fwd_tile(3, 5, 7) == (1, 1, 1, 1) and xm.fwd_tile(2, 9, 17) == (1, 1, 2, 3)
    assert xm.fwd_tile(1024, 40, 40) == (5, 5, 1, 1) and xm.fwd_tile(1023, 40, 40) == (4, 4, 2, 2) and xm.fwd_tile(1024, 40, 24) == (5, 3, 1, 1)
    assert xm.fwd_image_ok(1024, 24, 40, 50) and not xm.fwd_image_ok(1023, 24, 40, 50) and not xm.fwd_image_ok(1024, 24, 40, 48)
    assert not xm.fwd_image_ok(1024, 24, 40, 50, q=2) and not xm.fwd_image_ok(1024, 24, 40, 50, a=8) and not xm.fwd_image_ok(1024, 23, 40, 50)
    assert not xm.fwd_image_ok(1024, 48, 8, 50), "six 8-row tiles"
    assert xm.fwd_route(*xm.MISALIGNED) == ("image", 3, 5) and xm.fwd_route(*xm.MISALIGNED, q=2) == ("generic", 3, 5)
    assert xm.bwd_tiled_lds(1, 40, 40) == 1600 * 20 + 80 * 33 * 4 + 16
    assert xm.bwd_route(1, False, 70, 40, 40, 50) == ("tiled", 1, False, 1) and xm.bwd_route(1, True, 512, 16, 24, 50) == ("tiled", 1, True, 0)
    assert xm.bwd_route(0, False, 511, 16, 24, 50) == ("tiled", 0, True, 1), "cosine has one arithmetic; 511 x 2 chunks split"
    assert xm.bwd_route(1, True, 2, 60, 60, 16) == ("plain", 1) and xm.bwd_route(0, True, 2, 60, 60, 16) == ("plain", 0)
    assert xm.bwd_route(1, True, 2, 56, 56, 16) == ("plain", 1) and xm.bwd_route(0, True, 2, 56, 56, 16) == ("tiled", 0, True, 1), \
        "Euclid's tables are 20 bytes per (j, k), cosine's 16"


def test_tables_reach_every_instantiation():
    assert not xm.UNREACHABLE
    missing = sorted(xm.FWD_REACHABLE - xm.fwd_cells())
    assert not missing, "no forward shape runs %s" % (missing,)
    assert xm.fwd_cells() <= xm.FWD_REACHABLE
    missing = sorted(xm.BWD_REACHABLE - xm.bwd_cells(), key=str)
    assert not missing, "no backward shape runs %s" % (missing,)
    assert xm.bwd_cells() <= xm.BWD_REACHABLE
    for s in xm.FWD + xm.BWD + [xm.EDGE, xm.MISALIGNED]:
        assert xm.refusal(1, *s) == xm.OK and xm.refusal(0, *s) == xm.OK
    assert len(xm.FWD) == len(set(xm.FWD)) and set(xm.NAMED_FWD) <= set(xm.FWD)
    for (N, W1, W2, D), rj, rk in zip(xm.GENERIC_TILES, [j for j in range(1, 6) for _ in range(5)], [k for _ in range(5) for k in range(1, 6)]):
        assert xm.fwd_route(N, W1, W2, D) == ("generic", rj, rk), (N, W1, W2, D)


def test_tables_hold_every_boundary():
    # forward: odd D, D % 32 == 1, ragged tiles, several tiles, a last image workgroup with one wave, both odd register tiles
    assert (2, 9, 17, 33) in xm.FWD and xm.fwd_tile(2, 9, 17)[2:] == (2, 3)
    assert any(D % 2 for (_, _, _, D) in xm.FWD) and any(W1 % 8 and W2 % 8 for (_, W1, W2, _) in xm.FWD)
    assert any(xm.fwd_route(*s)[0] == "image" and s[0] % 2 for s in xm.FWD)
    assert any(xm.fwd_route(*s) == ("generic", 5, 3) for s in xm.FWD)
    # backward: chunks of 32, of one d and ragged; split and not; rows whose byte length is 2, 4 and 8 (mod 8)
    chunks = {(D + 31) // 32 for (_, _, _, D) in xm.BWD}
    assert {1, 2, 3} <= chunks and any(D % 32 == 1 for (_, _, _, D) in xm.BWD)
    assert {2 * D % 8 for (_, _, _, D) in xm.BWD} >= {0, 2, 4}
    assert any(N * ((D + 31) // 32) == 1024 for (N, _, _, D) in xm.BWD), "the first unsplit batch"
    assert max(xm.bwd_tiled_lds(1, W1, W2) for (_, W1, W2, _) in xm.BWD if xm.bwd_route(1, True, 2, W1, W2, 16)[0] == "tiled") > 40000


@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_euclid_brackets_admit_the_oracle_and_pin(shape, oracle):
    """The default-mode case: (a) the parity bar's bracket holds the oracle's halves and cannot pin 99 %; (b) the per-element
    bracket holds them and pins at least 99 %.  The inputs' gradients are finite normal halves almost everywhere."""
    c = xm.backward_case(oracle, 1, shape, "aligned")
    assert np.isfinite(c["top"]).all() and (c["dT"] > 0).all()
    N = shape[0]
    if N >= 3:
        mags = np.abs(c["dT"]).reshape(N, -1).max(1)
        assert mags.max() / mags.min() >= 2.0 ** 19, "top_diff spans 2^-10 .. 2^10 across pairs"
    for k in ("dq", "da"):
        h = c[k].astype(np.float16)
        assert np.isfinite(h).all()
        ref, scale, b = xm.parity_bracket(c, k)
        lo, hi = xm.check_bracket("oracle %s, parity bar" % k, h, ref, scale, b)
        share_a = xm.pinned_share(lo, hi)
        assert share_a <= xm.parity_pinned_ceiling() < xm.PINNED_MIN, "the parity bar's bracket straddles a tie for at least 2 % of any array"
        ref64, scale = c["ref"][k]
        bar = xm.term_bar(c, k)
        lo, hi = xm.check_bracket("oracle %s %s" % (k, shape), h, ref64, scale, bar)
        share = xm.pinned_share(lo, hi)
        print("euclid %s %s: e(oracle) = %.2f, bar %.2f (x 2^-24), pinned %.3f %% (parity bar: %.2f %%)" % (
            k, xm.shape_id(shape), c["e_o"][k] / cm.U24, bar / cm.U24, 100 * share, 100 * share_a))
        assert share >= xm.PINNED_MIN
        assert bar < 2.0 ** -18, "the bar is a few fp32 roundings, far below a half's 2^-11"


@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_cosine_brackets_admit_the_oracle_and_pin(shape, oracle):
    c = xm.backward_case(oracle, 0, shape, "aligned")
    assert np.isfinite(c["top"]).all() and (c["n0"] > 0).all() and (c["n1"] > 0).all()
    for k in ("dq", "da"):
        ref64, scale = c["ref"][k]
        bar = cm.dense_bar(c["e_o"][k])
        lo, hi = xm.check_bracket("oracle %s %s" % (k, shape), c[k].astype(np.float16), ref64, scale, bar)
        share = xm.pinned_share(lo, hi)
        print("cosine %s %s: e(oracle) = %.2f, bar %.2f (x 2^-24), pinned %.3f %%" % (k, xm.shape_id(shape), c["e_o"][k] / cm.U24, bar / cm.U24, 100 * share))
        assert share >= xm.PINNED_MIN and bar < 2.0 ** -18
    for k in ("top", "n0", "n1"):
        assert cm.dense_bar(c["e_o"][k]) < 2.0 ** -18


@pytest.mark.parametrize("shape", xm.BWD, ids=xm.shape_id)
def test_reference_mode_cases_exercise_the_contract(shape, oracle):
    """The reference-rounding backward is held to the oracle's halves: they must be finite, mostly nonzero, and T == 1 must occur."""
    c = xm.backward_case(oracle, 1, shape, "dense")
    for k in ("dq", "da"):
        h = c[k].astype(np.float16)
        assert np.isfinite(h).all() and (h != 0).mean() > 0.9
    if shape[0] >= 2:
        assert c["top"][1, 0, 0, 0] == 1.0


@pytest.mark.parametrize("shape", xm.NAMED_FWD + xm.GENERIC_TILES[::6], ids=xm.shape_id)
def test_probes_are_exact_as_halves(shape, oracle):
    c = xm.forward_case(oracle, 0, shape)
    p = cm.probe_inputs(np.random.default_rng(1701 + cm.shape_seed(shape)), *shape)
    _, _, _, bound = cm.integer_sums(c["q"], c["a"], p["eq"], p["ea"])
    assert bound < 2 ** 24
    top, n0, n1 = cm.closed_form_forward(c["q"], c["a"], p["eq"], p["ea"])
    for got, want in ((c["top"], top), (c["n0"], n0), (c["n1"], n1)):
        assert (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_edge_inputs_hold_the_edges(mode, oracle):
    c = xm.edge_case(oracle, mode)
    qh, ah, top, names = c["qh"], c["ah"], c["top"][:, 0], c["names"]
    assert len(names) == xm.EDGE[0] and names[9] == "clean" and np.isfinite(c["dq"][9]).all() and np.isfinite(c["da"][9]).all()
    sub = np.abs(qh[3].astype(np.float64))
    assert ((sub >= 2.0 ** -24) & (sub < 2.0 ** -14)).all() and np.isfinite(top[3]).all()
    assert np.abs(qh[2].astype(np.float64)).min() == 65504.0 and np.isfinite(top[2]).all()
    mags = np.abs(c["dT"][[0, 9]]).reshape(2, -1).max(1)
    assert mags[1] / mags[0] >= 2.0 ** 19, "top_diff spans 2^-10 .. 2^10"
    over = lambda x: np.abs(x.astype(np.float64)) >= 65520.0
    with np.errstate(over="ignore"):
        if mode == 1:
            assert np.isnan(top[0, 1]).all() or (top[0, 1] == 0).all()
            assert (top[0, 1] == 0).all(), "an Inf coordinate: distance Inf, T = 0"
            assert np.isnan(top[1, :, 2]).all() and np.isnan(top[5, 2, 3])
            assert (np.diagonal(top[7]) == 1.0).all(), "q == a rows: T = 1, the divisor 1e-9"
            assert np.isfinite(c["dq"][2]).all() and over(c["dq"][2]).any() and np.isinf(c["dq"][2].astype(np.float16)[over(c["dq"][2])]).all()
            assert not c["dq"][4].any() and not c["da"][4].any(), "top_diff == 0"
            assert np.isfinite(top[6]).all() and np.isfinite(top[8]).all()
        else:
            assert np.isnan(top[0, 1]).all() and np.isnan(top[1, :, 2]).all() and np.isnan(top[5, 2, 3])
            assert c["n0"][6, 0] == 0 and np.isnan(top[6, 0]).all() and c["n1"][8, 4] == 0 and c["n0"][8, 3] == 0 and np.isnan(top[8, :, 4]).all()
            assert np.isfinite(c["dq"][4]).all() and over(c["dq"][4]).any() and np.isinf(c["dq"][4].astype(np.float16)[over(c["dq"][4])]).all()
