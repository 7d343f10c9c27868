"""CPU suite: the shape lists of tests/layer_plans.py reach the launch-plan regimes they claim, by the restated plans
(fm_plan of csrc/fm.hip, bn_route of csrc/bn.hip, bp_route of csrc/bn_pool.hip); the restated BN / BN-pool routes agree
with the library's workspace queries, which are host code; and the new BN / BN-pool parity inputs are conditioned for
the 1e-5 bar of tests/test_gpu_layer_plans.py."""
import numpy as np
import pytest

import bn_pool_reference as BP
import bn_reference as BN
import layer_plans as L
from util import SEED, TOL

FM_PLANS = {shape: L.fm_plan(*shape) for shape, _, _ in L.FM_SHAPES}
ITEM = {np.float32: 4, np.float64: 8}


def test_the_constants_are_the_sources():
    """The model reads its constants from csrc/fm.hip and csrc/bn_common.h; the figures the issue and DESIGN.md quote
    (48 KB of LDS, room 92 / 188 / 380 / 764 floats, 4096 / 2048 groups, 64 chunks) follow from them today."""
    assert L.FM == {"kFmLdsBytes": 48 * 1024, "kFmThreads": 256}
    assert [L.fm_room(S) for S in (64, 32, 16, 8)] == [92, 188, 380, 764]
    assert L.BNC["kBnSmallGroups"] == L.BNC["kBnSmallThreads"] * L.BNC["kBnBatch"] == 4096
    assert L.BNC["kBnChunkGroups"] == 2048 and L.BNC["kBnMaxChunks"] == 64


@pytest.mark.parametrize("shape,S,what", L.FM_SHAPES, ids=[str(s[0]) for s in L.FM_SHAPES])
def test_fm_shape_takes_the_plan_it_is_listed_for(shape, S, what):
    plan = FM_PLANS[shape]
    assert (plan is None) == (S is None), (what, plan)
    if plan is None:
        return
    N, C, dim = shape
    got_S, P, st = plan
    assert got_S == S, (what, plan)
    # the image of a panel fits its stride, the stride fits the buffer, and the walkers' 16-byte reads stay aligned
    assert P >= 1 and P * (C + 1) <= st <= L.fm_room(S) and st % 4 == 0 and (st // 4) % 2 == 1
    assert 2 * S * st * 4 <= L.FM["kFmLdsBytes"]
    assert C <= st                                   # the linear column's image


def test_fm_every_S_and_both_sides_of_each_threshold():
    assert {p[0] for p in FM_PLANS.values() if p} == {8, 16, 32, 64}
    for S in (16, 32, 64):
        at = 511 * S + 1                             # the least N with ceil(N / S) >= 512
        assert (at + S - 1) // S == 512 and (at - 1 + S - 1) // S == 511
        assert FM_PLANS[(at - 1, 2, 9)][0] == S // 2 and FM_PLANS[(at, 2, 9)][0] == S
        assert at % S == 1                           # the upper shape's last workgroup has one sample
    assert 32831 % 64 == 63 and FM_PLANS[(32831, 3, 20)][0] == 64


def test_fm_hand_downs():
    """At N = 32705 the grid rule admits S = 64, so a smaller S is the LDS rules' doing: `room / C1 < min(cols, 8)`
    (panel width) or `C1 > room`."""
    N = 32705
    assert (N + 63) // 64 >= 512

    def refused(S, C, dim):
        C1, cols = C + 1, max(dim - 1, 1)
        room = L.fm_room(S)
        return C1 > room, room // C1 < min(cols, 8)

    for C, dim, S in ((11, 9, 32), (23, 9, 16), (47, 9, 8)):                 # by panel width alone, all 8 columns
        assert FM_PLANS[(N, C, dim)][0] == S
        for above in (64, 32, 16):
            if above > S:
                assert refused(above, C, dim) == (False, True)
        if S > 8:
            assert refused(S, C, dim) == (False, False)
        assert FM_PLANS[(N, C, dim)][1] == 8
    assert refused(64, 80, 3) == (False, True) and refused(32, 80, 3) == (False, False)
    assert FM_PLANS[(N, 80, 3)][:2] == (32, 2)                               # fewer than 8 columns: both in one panel
    assert refused(64, 100, 2)[0] and refused(32, 100, 2) == (False, False)  # C1 = 101 > 92
    assert FM_PLANS[(N, 100, 2)][:2] == (32, 1)


def test_fm_panels_and_the_last_lane_walk_shape():
    S, P, st = FM_PLANS[(32705, 2, 100)]
    assert S == 64 and L.fm_panels(100, P) == 4                              # both buffers, twice each
    S, P, st = FM_PLANS[(32705, 2, 1)]
    assert S == 64 and L.fm_panels(1, P) == 0                                # the linear column alone
    assert FM_PLANS[(3, 763, 2)] == (8, 1, 764) and L.fm_room(8) == 764      # C1 == room, one column per panel
    assert FM_PLANS[(5, 764, 3)] is None and FM_PLANS[(70, 800, 2)] is None
    assert L.fm_plan(5, 763, 3) is not None
    for N in (2048, 4096, 2049):                                             # the bias_diff chain's 2048-element step
        assert FM_PLANS[(N, 1, 2)] is not None
    assert L.FM_PLACEMENT_SHAPE in FM_PLANS


@pytest.mark.parametrize("case", L.BN_CASES, ids=L.case_id)
def test_bn_shape_is_past_64_minimum_chunks(case, hiplib):
    (N, C, S), dtype = case
    item = ITEM[dtype]
    small, chunks, gpc = L.bn_route(N, S, item)
    groups = (N * S + 16 // item - 1) // (16 // item)
    assert not small and chunks == L.BNC["kBnMaxChunks"] and gpc > L.BNC["kBnChunkGroups"]
    assert gpc == (groups + 63) // 64
    assert 0 < groups - 63 * gpc < gpc                                       # the last chunk is ragged
    query = hiplib.mms_bn_workspace_bytes if dtype == np.float32 else hiplib.mms_bn_workspace_bytes_f64
    assert query(N, C, S) == L.bn_workspace_bytes(N, C, S, item) == C * chunks * 4 * item
    if (N, S) == (4099, 129):
        assert S % 4 and (N * S) % 4                                         # one access per element, a partial group


@pytest.mark.parametrize("case", L.BP_CASES, ids=L.case_id)
def test_bn_pool_shape_is_past_64_minimum_chunks(case, hiplib):
    (N, C, H, W, kh, kw), dtype = case
    item = ITEM[dtype]
    small, chunks, wpc = L.bp_route(N, H, W, kh, kw, item)
    windows, least = N * H * W // (kh * kw), L.bp_least(kh, kw, item)
    assert not small and wpc > least and wpc == (windows + 63) // 64
    assert 0 < windows - (chunks - 1) * wpc < wpc                            # the last chunk is ragged
    query = (hiplib.mms_bn_pool_tanh_workspace_bytes if dtype == np.float32
             else hiplib.mms_bn_pool_tanh_workspace_bytes_f64)
    want = C * min(64, (windows + least - 1) // least) * 4 * item
    assert query(N, C, H, W, kh, kw) == L.bp_workspace_bytes(N, C, H, W, kh, kw, item) == want == C * 64 * 4 * item
    if case[0] == L.BP_63_CHUNKS:
        assert (kh * kw, least, wpc, chunks) == (144, 57, 58, 63)            # 63 chunks; the query answers for 64
    else:
        assert chunks == 64


@pytest.mark.parametrize("N", [1, 13, 20, 129, 405, 1517, 3652, 4099, 20000])
def test_the_restated_routes_are_the_workspace_queries(N, hiplib):
    """Beyond the listed shapes: both restatements against the library's queries over the geometries the suites use,
    on either route."""
    for S in (25, 129, 144, 1296):
        assert hiplib.mms_bn_workspace_bytes(N, 3, S) == L.bn_workspace_bytes(N, 3, S, 4)
        assert hiplib.mms_bn_workspace_bytes_f64(N, 3, S) == L.bn_workspace_bytes(N, 3, S, 8)
    for geom in ((36, 36, 4, 4), (5, 5, 5, 5), (12, 12, 12, 12), (9, 37, 3, 37), (25, 41, 5, 1)):
        assert hiplib.mms_bn_pool_tanh_workspace_bytes(N, 3, *geom) == L.bp_workspace_bytes(N, 3, *geom, 4)
        assert hiplib.mms_bn_pool_tanh_workspace_bytes_f64(N, 3, *geom) == L.bp_workspace_bytes(N, 3, *geom, 8)


def test_probe_sums_are_exact_by_the_shape():
    for shape, dtype in L.BN_CASES + L.BP_CASES:
        x = L.probe_x(shape, dtype, SEED)                                    # asserts N*S*16 < 2^24 itself
        assert np.abs(x).max() == L.PROBE_MAX and (x == np.rint(x)).all()
        axes = tuple(a for a in range(x.ndim) if a != 1)
        assert (x.astype(np.int64) ** 2).sum(axis=axes).max() < 2 ** 24


@pytest.mark.parametrize("case", [c for c in L.BN_CASES if c[1] == np.float32], ids=L.case_id)
def test_bn_parity_inputs_are_well_conditioned(case):
    """On the float32 inputs of the GPU test, BN's algebra in float32 with every channel sum taken as the large route
    documents it -- 64 chunk sums, each numpy's own float32 `sum`, folded in ascending order -- stays within TOL / 2 of
    the float64 model on every output, in assert_close's metric: the device, whose chunk sums are trees over a few
    groups per thread, has the other half of the bar.  bn_reference.conditioned_inputs serve as they are: the worst
    ratio to TOL / 2 is 0.045 at (405, 2, 1296) and 0.032 at (4099, 1, 129).

    ONE running float32 sum over a channel's half a million elements is not the form to use and nothing here sums that
    way: its error grows with the length of the chain, and already bn_reference's own float32 model, whose running
    sums are only S and then N long, reaches 0.13 and 0.48 of TOL / 2 at these two shapes."""
    shape = case[0]
    i = BN.conditioned_inputs(shape, np.float32, SEED)
    got, want = L.bn_chunked_outputs(i), BN.model_outputs(i, np.float64)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float32 and want[k].dtype == np.float64 and got[k].shape == want[k].shape, k
    worst = L.worst_ratio(got, want, TOL / 2)
    print("%s: worst ratio to TOL / 2 = %.3f" % (shape, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("case", [c for c in L.BP_CASES if c[1] == np.float32], ids=L.case_id)
def test_bn_pool_parity_inputs_are_well_conditioned(case):
    """The same for the fused algebra of mms_bn_pool_tanh_*: sum x and sum x*x over each chunk's windows, sum gp and
    sum gp*save_pool over each chunk's pooled elements, 64 (63) chunk sums by numpy's float32 `sum` folded in ascending
    order, against the three layers in sequence in float64.  Worst ratio to TOL / 2 with conditioned_inputs as they
    are: 0.061 at (405, 2, 36, 36, 4, 4), 0.053 at (3652, 1, 12, 12, 12, 12).  A plainly sequential float32 sum is not
    the form to use (bn_pool_reference's docstring has the figures at 21645 elements; its fused_outputs, with running
    sums over a map and then over N, is at 0.12 and 0.67 here)."""
    shape = case[0]
    i = BP.conditioned_inputs(shape, np.float32, SEED)
    got, want = L.bp_chunked_outputs(i, shape[4:]), BP.model_outputs(i, shape[4:], np.float64)
    assert sorted(got) == sorted(want) and len(want) == 2 * len(BP.OUTPUTS)
    for k in want:
        assert got[k].dtype == np.float32 and want[k].dtype == np.float64 and got[k].shape == want[k].shape, k
    worst = L.worst_ratio(got, want, TOL / 2)
    print("%s: worst ratio to TOL / 2 = %.3f" % (shape, worst))
    assert worst <= 1.0
