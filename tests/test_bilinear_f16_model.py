"""tests/bilinear_f16_model.py proved on the CPU: the routing restated there takes the decisions the issue's table names, the shape
table reaches every kernel instantiation of the fp16-storage bilinear calls (both forward kernels at both k depths, the backward at
both depths with direct and reduced gradient stores, the generic route in either direction, the three staging widths) and lists
nothing unreachable; the inputs are exact halves; and the in-order dbias reference is the oracle's."""
import numpy as np
import pytest

import bilinear_f16_model as bm
import bilinear_grid_model as gm


def test_refusals_restated():
    assert bm.refusal(4, 5, 7, 50, 2) == bm.OK and bm.refusal(0, 5, 7, 50, 2) == bm.OK and bm.refusal(4, 1, 2, 50, 1) == bm.OK
    assert bm.refusal(4, 1, 1, 50, 1) == bm.UNSUPPORTED and bm.refusal(4, 1, 1, 50, 3) == bm.UNSUPPORTED
    for bad in ((-1, 5, 7, 50, 2), (4, 0, 7, 50, 2), (4, 5, -7, 50, 2), (4, 5, 7, 0, 2), (4, 5, 7, 50, 0), (4, 5, 7, 50, -1),
                (1 << 20, 64, 64, 64, 1), (1 << 16, 48, 48, 8, 16)):
        assert bm.refusal(*bad) == bm.INVALID_ARG, bad
    assert bm.embed_refusal(512, 5, 7, 50, 2, 37) == bm.OK and bm.embed_refusal(3, 5, 7, 50, 4, 37) == bm.OK
    assert bm.embed_refusal(*bm.EMBED_UNSUPPORTED, 37) == bm.UNSUPPORTED and bm.embed_refusal(3, 5, 7, 65, 2, 37) == bm.UNSUPPORTED
    assert bm.embed_refusal(3, 5, 7, 50, 4, 0) == bm.INVALID_ARG and bm.embed_refusal(3, 5, 7, 64, 4, 1 << 26) == bm.INVALID_ARG
    assert bm.embed_refusal(0, 5, 7, 65, 2, 37) == bm.OK, "an empty batch is accepted before the geometry is looked at"


def test_routing_restated():
    assert bm.fwd_route(512, 5, 7, 50, 2) == ("eval", 13) and bm.fwd_route(512, 48, 48, 52, 2) == ("eval", 13)
    assert bm.fwd_route(512, 17, 33, 53, 1) == ("eval", 16) and bm.fwd_route(1 << 20, 48, 48, 64, 1)[0] == "eval"
    assert bm.fwd_route(511, 5, 7, 50, 2) == ("generic",) and bm.fwd_route(257, 5, 7, 50, 2) == ("generic",)
    assert bm.fwd_route(256, 5, 7, 50, 2) == ("train", 13) and bm.fwd_route(256, 5, 7, 53, 2) == ("train", 16)
    assert bm.fwd_route(256, 5, 7, 50, 256) == ("generic",), "N M > 65535"
    assert bm.fwd_route(3, 49, 7, 50, 2) == ("generic",) and bm.fwd_route(3, 5, 49, 50, 2) == ("generic",) and bm.fwd_route(3, 5, 7, 65, 2) == ("generic",)
    assert bm.bwd_route(50, 40, 40, 50, 4) == ("fused", (10, 13), "reduced") and bm.bwd_route(50, 40, 40, 52, 1) == ("fused", (10, 13), "direct")
    assert bm.bwd_route(50, 41, 40, 50, 4) == ("fused", (12, 16), "reduced") and bm.bwd_route(50, 40, 41, 50, 1) == ("fused", (12, 16), "direct")
    assert bm.bwd_route(50, 40, 40, 53, 1) == ("fused", (12, 16), "direct")
    assert bm.bwd_route(257, 5, 7, 50, 2) == ("generic",) and bm.bwd_route(512, 5, 7, 50, 2) == ("generic",) and bm.bwd_route(2, 5, 7, 65, 2) == ("generic",)
    assert not bm.scratch(50, 40, 40, 50, 4) and bm.scratch(512, 5, 7, 50, 2) and bm.scratch(300, 5, 7, 50, 2) and bm.scratch(3, 5, 7, 65, 2)
    # the driver's grid: 40 rows of 50 halves are 4000 contiguous bytes, a multiple of 16
    assert bm.stage_width(40, 40, 50) == 8 and bm.stage_width(40, 40, 50, q=2) == 1 and bm.stage_width(40, 40, 50, a=4) == 2
    assert bm.stage_width(5, 7, 50) == 2 and bm.stage_width(17, 33, 53) == 1 and bm.stage_width(48, 48, 64) == 8
    assert bm.stage_width(5, 7, 50, gather=True) == 2 and bm.stage_width(5, 7, 64, gather=True) == 8 and bm.stage_width(8, 8, 53, gather=True) == 1


def test_table_reaches_every_instantiation():
    assert not bm.UNREACHABLE
    assert bm.fwd_cells() == bm.FWD_REACHABLE, sorted(bm.FWD_REACHABLE ^ bm.fwd_cells(), key=str)
    assert bm.bwd_cells() == bm.BWD_REACHABLE, sorted(bm.BWD_REACHABLE ^ bm.bwd_cells(), key=str)
    assert bm.width_cells() == {8, 2, 1}
    assert {bm.stage_width(s[1], s[2], s[3], gather=True) for s in bm.EMBED} == {2}
    for s in bm.FWD + bm.BWD + bm.CANARY + bm.EMBED + [bm.OVERFLOW, bm.MISALIGNED_EVAL, bm.MISALIGNED_TRAIN]:
        assert bm.refusal(*s[:5]) == bm.OK, s
    # the rows of the issue's table, route by route
    assert [bm.fwd_route(*s[:5]) for s in bm.EVAL] == [("eval", 13), ("eval", 13), ("eval", 16), ("eval", 16)]
    assert [bm.fwd_route(*s[:5]) for s in bm.TRAIN] == [("train", 13)] * 4 + [("train", 16)] * 2, \
        "the table names the train rows by their backward: (2, 41, 9, 33) runs the <12, 16> backward behind the <13> forward"
    assert [bm.bwd_route(*s[:5])[1:] for s in bm.TRAIN] == [((10, 13), "reduced"), ((10, 13), "direct"), ((10, 13), "direct"),
                                                           ((12, 16), "reduced"), ((12, 16), "direct"), ((12, 16), "reduced")]
    assert all(bm.fwd_route(*s[:5]) == ("generic",) and bm.bwd_route(*s[:5]) == ("generic",) for s in bm.GENERIC)
    assert bm.fwd_route(*bm.BWD_ONLY_GENERIC[:5]) == ("eval", 13) and bm.bwd_route(*bm.BWD_ONLY_GENERIC[:5]) == ("generic",)
    assert {bm.fwd_route(*s[:5])[0] for s in bm.CANARY} == {"eval", "train", "generic"}
    assert {bm.fwd_route(*s[:5])[0] for s in bm.ORACLE} == {"eval", "train", "generic"} and \
        {bm.bwd_route(*s[:5])[:2] for s in bm.ORACLE[1:]} == {("fused", (10, 13)), ("fused", (12, 16)), ("generic",)}
    for s in bm.CANARY:
        N, W1, W2, D, M, _ = s
        assert (N * W1 * D) % 2 and (N * W2 * D) % 2 and (N * M * W1 * W2) % 2, "odd element counts: %s" % (s,)
    assert [bm.embed_refusal(*s[:5], bm.EMBED_K) for s in bm.EMBED] == [bm.OK, bm.OK]
    assert {bm.fwd_route(*s[:5])[0] for s in bm.EMBED} == {"eval", "train"}


def test_table_holds_every_boundary():
    shapes = bm.FWD + bm.BWD
    assert any(s[0] == 256 for s in bm.TRAIN) and any(s[0] == 512 for s in bm.EVAL) and any(256 < s[0] < 512 for s in bm.GENERIC)
    assert any(s[3] == 52 for s in shapes) and any(s[3] == 53 for s in shapes) and any(s[3] == 64 for s in shapes) and any(s[3] == 65 for s in shapes)
    assert any(s[1] == 48 and s[2] == 48 for s in shapes) and any(s[1] == 49 for s in shapes) and any(s[1] == 41 for s in bm.TRAIN)
    assert any(s[1] % 16 and s[2] % 16 and s[1] > 16 and s[2] > 16 for s in bm.EVAL), "several ragged tiles"
    assert any(s[3] % 2 for s in bm.EVAL) and any(s[3] % 2 for s in bm.TRAIN)
    assert any(s[5] for s in shapes) and any(not s[5] for s in shapes)
    assert (1, 1, 2, 1, 1, True) in bm.TRAIN


@pytest.mark.parametrize("shape", [bm.TRAIN[0], bm.GENERIC[1]], ids=bm.shape_id)
def test_inputs_are_exact_halves_and_shared(shape):
    c = bm.inputs(shape)
    assert c is bm.inputs(shape) and not c["q"].flags.writeable
    assert c["qh"].dtype == np.float16 and (c["q"] == c["qh"].astype(np.float32)).all() and np.isfinite(c["q"]).all()
    assert (c["bias"] is not None) == shape[5] and (c["dbias0"] is not None) == shape[5]
    N, W1, W2, D, M, _ = shape
    assert c["W"].shape == (M, D, D) and c["dT"].shape == (N, M, W1, W2)


def test_dbias_in_order_is_the_oracles(oracle):
    s = bm.TRAIN[0]
    c = bm.inputs(s)
    top, _, _ = oracle.simcross_forward(2, c["q"], c["a"], c["W"], c["bias"])
    _, _, _, db = oracle.simcross_backward(2, c["q"], c["a"], top, c["dT"], W=c["W"], bias_term=True, dbias_in=c["dbias0"])
    assert (gm.dbias_in_order(c["dT"], c["dbias0"]).view(np.uint32) == db.view(np.uint32)).all()


def test_embed_inputs_hold_out_of_range_ids():
    table, iq, ia, ebias = bm.embed_inputs(bm.EMBED[1])
    K = bm.EMBED_K
    assert table.dtype == np.float16 and table.shape == (K, 50) and ebias.shape == (50,)
    assert (iq < 0).any() and (iq >= K).any() and (ia < 0).any() and (ia >= K).any()
    assert bm.clamp_ids(iq, K).min() == 0 and bm.clamp_ids(iq, K).max() == K - 1
