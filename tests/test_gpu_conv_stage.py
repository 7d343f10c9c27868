"""GPU suite: the TEST-phase Convolution -> BN -> AvePool -> TanH stage (include/mms_conv_stage.h,
csrc/conv_stage.hip) against tests/conv_stage_reference.py.  The fused launch (mms_conv_stage_forward_fused_f32, at
every shape it reaches, whichever route the main call's measured rules pick there) is held to the sequence route -- the
two public calls -- by EQUALITY on integer probes, whatever order a kernel sums the products in, and at network_v4's
two stages and at one shape per instantiation of the pooling epilogue on conditioned inputs too; the order of the window
sum by an order probe whose sums round; the main call to the route mms_conv_stage_route names; every shape to the
float64 model at the project's 1e-5 (float32) and 1e-12 (float64) in assert_close's metric; the fixed order and the workspace's irrelevance by equality of words between two runs.
The bodies that do not depend on the pooling method are tests/pooled_stage_suite.py's, bound here to this stage."""
import numpy as np
import pytest

import conv_stage_reference as R
from pooled_stage_suite import ConvStage
from test_gpu_conv import assert_words_equal
from util import TOL, assert_close

pytestmark = pytest.mark.gpu

S = ConvStage("conv_stage", R, assert_words_equal)
FUSED_IDS = [R.stage_id(st) for st in R.FUSED_STAGES]
ALL_IDS = [R.stage_id(st) for st in R.GPU_STAGES]


@pytest.mark.parametrize("st", R.FUSED_STAGES, ids=FUSED_IDS)
def test_integer_probe_fused_equals_sequence(st, hiplib):
    """The map is exact whatever order its products are summed in, so both routes pool the same numbers: top and
    save_pool equal word for word, and save_pool equals the float32 restatement of the finish."""
    S.check_integer_probe_fused_equals_sequence(st)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("st", R.GPU_STAGES, ids=ALL_IDS)
def test_parity_and_determinism(st, dtype, hiplib):
    """ConvStage.check_parity_and_determinism; network_v4's stages and one shape per instantiation of the epilogue (both
    routes have the same chunks of input channels there): fused and sequence, the same words."""
    S.check_parity_and_determinism(st, dtype, R.V4_STAGES + R.INSTANTIATION_STAGES)


@pytest.mark.parametrize("st", R.ORDER_STAGES, ids=[R.stage_id(st) for st in R.ORDER_STAGES])
def test_order_probe_window_sum_is_the_chain_in_hw_order(st, hiplib):
    """R.order_probe: every element of y is one exact product, the window sums round.  save_pool of the fused launch
    is the float32 restatement on the exact map -- the window added as one chain in (h, w) order from 0 -- word for
    word, at every instantiation AVE reaches (compiled and run-time windows, every MT); a column-major, a reversed or a
    pairwise sum differs from it in at least a tenth of the windows (asserted here on the draw, printed).  The sequence
    and the main call give the same words: their map is exact too."""
    ost = R.order_stage(st)
    inp = R.order_probe(ost, R.ORDER_SEED)
    y = R.order_probe_map(ost, inp)
    shares = R.order_shares(y, ost.pool)
    print("windows that differ from the (h, w) chain: " + ", ".join("%s %.0f %%" % (k, 100 * v) for k, v in sorted(shares.items())))
    assert min(shares.values()) >= R.ORDER_MIN_SHARE
    want_top, want_sp = R.finish(y, ost.pool, inp["mean"], inp["var"], inp["scale"], inp["shift"])
    fused, seq, auto = S.run(ost, inp, route="fused"), S.run(ost, inp, route="sequence"), S.run(ost, inp)
    assert_words_equal(fused["save_pool"], want_sp, "order probe, save_pool against the float32 restatement")
    assert_close(fused["top"], want_top, TOL, "order probe, top")
    for k in ("top", "save_pool"):
        assert_words_equal(seq[k], fused[k], "order probe, sequence against fused, " + k)
        assert_words_equal(auto[k], fused[k], "order probe, the main call against fused, " + k)


def test_the_main_call_reaches_both_routes_on_the_fused_list(hiplib):
    m = S.mod()
    assert [S.route_of(st) for st in R.V4_STAGES] == [m.ROUTE_FUSED, m.ROUTE_SEQUENCE, m.ROUTE_FUSED]


@pytest.mark.parametrize("st", [R.FUSED_STAGES[0], R.FUSED_STAGES[4], R.SEQUENCE_STAGES[0]],
                         ids=[ALL_IDS[0], ALL_IDS[4], R.stage_id(R.SEQUENCE_STAGES[0])])
def test_save_pool_is_optional(st, hiplib):
    S.check_save_pool_is_optional(st)


@pytest.mark.parametrize("st", R.SEQUENCE_STAGES, ids=[R.stage_id(st) for st in R.SEQUENCE_STAGES])
def test_sequence_route_is_the_two_public_calls(st, hiplib):
    """The main call on a shape it routes to the sequence, against mms_conv_forward_f32 and
    mms_bn_pool_tanh_forward_f32 (TEST) issued here."""
    from mms_answer_selection_amd import capi
    S.check_sequence_route_is_the_two_public_calls(st, capi.bn_pool_tanh_forward)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_empty_batch_writes_nothing(dtype, hiplib):
    S.check_empty_batch_writes_nothing(dtype)
