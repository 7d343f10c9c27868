"""The TEST-phase stage Convolution -> BN -> MaxPool -> TanH (include/mms_conv_maxpool_stage.h) as numpy: the layers of
tests/conv_reference.py and tests/bn_maxpool_reference.py (phase TEST) in sequence, generic over the dtype, plus the
float32 restatement of the finish that the library's save_pool is held to word for word where the convolution's map is
exact.

    x (N, C, H, W)   weight (K, C/group, kh, kw)   bias, mean, var, scale, shift (K)   top, save_pool (N, K, OH/ph, OW/pw)
"""
import numpy as np

import bn_maxpool_reference as BM
import conv_reference as CR
import conv_stage_reference as A
from conv_stage_reference import ST, pooled_shape, stage_id                    # noqa: F401 (the callers' names)

# network_v3's and network_v5's five stages in miniature: the fused launch reaches each
NET_STAGES = [
    ST(3, 1, 40, 40, 64, 5, 5, (4, 4)),                 # v3's first stage: one input channel, nine bands of 4 rows
    ST(23, 64, 9, 9, 64, 5, 5, (5, 5)),                 # its second: 64 input channels; ten images per workgroup, the
                                                        # last workgroup ragged (three images)
    ST(3, 2, 40, 40, 32, 3, 3, (2, 2)),                 # v5's first stage: a 38 x 38 map, bands of 6 rows, the last of 2
    ST(5, 32, 19, 19, 32, 4, 4, (2, 2)),                # its second: a 256-pixel map, one image per workgroup
    ST(15, 32, 8, 8, 32, 3, 3, (6, 6)),                 # its third: seven 6 x 6 images per workgroup, the last workgroup
                                                        # holding one
]
# conv_stage_reference's lists by import: the ragged K, no-bias, bands 8/8/4, N = 1, wide-window cases the fused launch
# reaches; stride / pad / group, > 64 channels and "two rows fit, not three", which it does not
# the fewest workgroups at which the main call takes the fused launch (mms_conv_maxpool_stage_route), of each kind
MAIN_FUSED_STAGES = [
    ST(8, 2, 40, 40, 32, 3, 3, (2, 2)),                 # 56 workgroups of a band of rows (54 would do: 7 per image)
    ST(414, 32, 8, 8, 32, 3, 3, (6, 6)),                # 60 workgroups of seven whole images, the last holding one
]
FUSED_STAGES = NET_STAGES + MAIN_FUSED_STAGES + A.FUSED_STAGES
SEQUENCE_STAGES = A.SEQUENCE_STAGES
GPU_STAGES = FUSED_STAGES + SEQUENCE_STAGES
# the stages whose two routes cut the input channels into the same chunks (one chunk): fused and sequence, the same words
SAME_CHUNK_STAGES = [NET_STAGES[0], NET_STAGES[2]]
# ... and conv_stage_reference's INSTANTIATION_STAGES, one per instantiation of the pooling epilogue: both plans have the
# same CC at each (several chunks at two of them), which tests/test_conv_stage_plans.py reads from the C++
SAME_WORDS_STAGES = SAME_CHUNK_STAGES + A.INSTANTIATION_STAGES
NAN_STAGES = SAME_CHUNK_STAGES + [A.INSTANTIATION["a"], A.INSTANTIATION["g"]]     # test_a_window_holding_one_nan's

ZERO_CHANNEL, NEGATIVE_CHANNEL = 0, 1                   # scale exactly 0.0 / negative at every stage (K >= 3 everywhere)


def forward(st, x, weight, bias, mean, var, scale, shift):
    """-> top, save_pool in x's dtype: conv_reference.conv_forward, then bn_maxpool_reference.forward in TEST phase."""
    y = CR.conv_forward(st.conv, x, weight, bias)
    out = BM.forward(y, st.pool, scale, shift, mean, var, phase=BM.TEST)
    return out[0], out[1]


def finish(y, pool, mean, var, scale, shift):
    """-> top, save_pool from the convolution's map y, in y's dtype, by the formulas of include/mms_bn_maxpool.h: the
    window scanned in (h, w) order from its first element (the larger kept for scale > 0, the smaller for scale < 0, the
    first for scale == 0), (e + (-mean)) / sqrt(var + 1e-9), tanh(sp*scale + shift).  Every step is one correctly
    rounded operation but the tanh, so save_pool is the library's word for word."""
    out = BM.fused_forward(y, pool, scale, shift, mean, var, phase=BM.TEST)
    return out[0], out[1]


SIGN_SEED_OFFSET = 57            # the signs come from their own generator: seed + this


def _with_signs(inp, seed, dtype):
    """inp with scale given random signs, channel ZERO_CHANNEL's exactly 0.0, channel NEGATIVE_CHANNEL's negative and
    channel 2's positive: all three scan directions run at every shape."""
    scale = np.array(inp["scale"], dtype=np.float64)
    assert scale.size >= 3
    scale *= np.random.default_rng(seed + SIGN_SEED_OFFSET).choice([-1.0, 1.0], scale.size)
    scale[ZERO_CHANNEL], scale[NEGATIVE_CHANNEL], scale[2] = 0.0, -abs(scale[NEGATIVE_CHANNEL]), abs(scale[2])
    return dict(inp, scale=np.ascontiguousarray(scale.astype(dtype)))


def conditioned_inputs(st, dtype, seed):
    """conv_stage_reference.conditioned_inputs (the map is O(1); mean 0.5 N(0, 1), var and |scale| from [0.5, 1.5],
    shift 0.5 N(0, 1)) with _with_signs' signs on scale.  Read-only arrays."""
    out = _with_signs(A.conditioned_inputs(st, dtype, seed), seed, dtype)
    out["scale"].setflags(write=False)
    return out


def integer_probe(st, seed):
    """x, weight, bias as int64 in [-4, 4] (conv_reference.integer_probe): every element of the map is an integer below
    probe_bound, and its windows are full of ties.  mean, var, scale, shift generic, in float32, scale with _with_signs'
    signs."""
    return _with_signs(A.integer_probe(st, seed), seed, np.float32)


def probe_bound(st):
    """The largest |partial sum| of an element of the map on integer_probe inputs, in any order; a scan adds nothing."""
    s = st.conv
    return 16 * (s.C // s.group) * s.kh * s.kw + 4


def probe_outputs(st, inp):
    """The integer probe's exact map (int64, as float32) finished in float32 -> top, save_pool."""
    y = CR.conv_forward(st.conv, inp["x"], inp["weight"], inp["bias"]).astype(np.float32)
    return finish(y, st.pool, inp["mean"], inp["var"], inp["scale"], inp["shift"])


def model_outputs(st, inp, dtype):
    """{"top", "save_pool"} at `dtype` on inp (cast to it)."""
    c = {k: (None if v is None else v.astype(dtype)) for k, v in inp.items()}
    top, sp = forward(st, c["x"], c["weight"], c["bias"], c["mean"], c["var"], c["scale"], c["shift"])
    return dict(top=top, save_pool=sp)
