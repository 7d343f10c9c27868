"""The TEST-phase stage Convolution -> BN -> AvePool -> TanH (include/mms_conv_stage.h) as numpy: the layers of
tests/conv_reference.py and tests/bn_pool_reference.py (phase TEST) in sequence, generic over the dtype, plus the
float32 restatement of the finish that the library's save_pool is held to word for word where the convolution's map is
exact.

    x (N, C, H, W)   weight (K, C/group, kh, kw)   bias, mean, var, scale, shift (K)   top, save_pool (N, K, OH/ph, OW/pw)
"""
import collections

import numpy as np

import bn_pool_reference as BP
import conv_reference as CR

Stage = collections.namedtuple("Stage", "conv pool")         # conv: a conv_reference.Shape; pool: (ph, pw)


def ST(N, C, H, W, K, kh, kw, pool, **kw_):
    return Stage(CR.S(N, C, H, W, K, kh, kw, **kw_), (int(pool[0]), int(pool[1])))


# The shapes of tests/test_gpu_conv_stage.py, the smallest at which each thing can go wrong.  Those the fused launch
# reaches (mms_conv_stage_forward_fused_f32; the main call takes it at the first and the third, mms_conv_stage_route):
V4_STAGES = [
    ST(3, 4, 40, 40, 32, 5, 5, (4, 4)),                 # network_v4's first stage in miniature: nine bands of 4 rows
    ST(23, 32, 9, 9, 64, 5, 5, (5, 5)),                 # its second: ten images per workgroup, three workgroups, the
                                                        # last with three images; the input channels in six chunks
    ST(93, 32, 9, 9, 64, 5, 5, (5, 5)),                 # the same on ten workgroups, the fewest the main call fuses
]
FUSED_STAGES = V4_STAGES + [
    ST(2, 3, 12, 14, 20, 3, 3, (2, 3), bias=False),     # K = 20: a ragged second channel tile; no bias
    ST(5, 2, 8, 8, 5, 3, 3, (3, 2), bias=False),        # K = 5; five 6 x 6 images where seven would fit
    ST(2, 3, 22, 32, 7, 3, 3, (2, 5)),                  # OH = 20, ph = 2: bands of 8, 8 and 4 rows
    ST(2, 2, 17, 52, 6, 3, 3, (3, 5)),                  # OW = 50: five rows fit a workgroup, ph = 3 leaves it three
    ST(1, 5, 11, 13, 7, 3, 3, (3, 11)),                 # N = 1; a window as wide as the map
]
# Those it does not reach: the sequence route of every call:
SEQUENCE_STAGES = [
    ST(2, 3, 10, 10, 4, 3, 3, (5, 1), stride=2, pad=1),
    ST(2, 4, 7, 7, 6, 3, 3, (1, 5), group=2, bias=False),
    ST(2, 65, 6, 6, 4, 3, 3, (2, 2)),                   # more than 64 input channels
    ST(1, 2, 5, 102, 3, 3, 3, (3, 4)),                  # the convolution is fast, but two rows of 100 fit, not three
]
GPU_STAGES = FUSED_STAGES + SEQUENCE_STAGES


def stage_id(st):
    return "-".join(str(v) for v in st.conv) + "-pool%dx%d" % st.pool


def pooled_shape(st):
    OH, OW = CR.output_dims(st.conv)
    return (st.conv.N, st.conv.K, OH // st.pool[0], OW // st.pool[1])


def forward(st, x, weight, bias, mean, var, scale, shift):
    """-> top, save_pool in x's dtype: conv_reference.conv_forward, then bn_pool_reference.forward in TEST phase."""
    y = CR.conv_forward(st.conv, x, weight, bias)
    out = BP.forward(y, st.pool, scale, shift, mean, var, phase=BP.TEST)
    return out[0], out[1]


def finish(y, pool, mean, var, scale, shift):
    """-> top, save_pool from the convolution's map y, in y's dtype, by the formulas of include/mms_conv_stage.h: the
    window added in (h, w) order from 0, one division by ph*pw, (m + (-mean)) / sqrt(var + 1e-9), tanh(sp*scale + shift).
    Every step is one correctly rounded operation but the tanh, so save_pool is the library's word for word."""
    out = BP.fused_forward(y, pool, scale, shift, mean, var, phase=BP.TEST)
    return out[0], out[1]


def _bn_arrays(K, r):
    return dict(mean=0.5 * r.standard_normal(K), var=r.uniform(0.5, 1.5, K), scale=r.uniform(0.5, 1.5, K),
                shift=0.5 * r.standard_normal(K))


BN_SEED_OFFSET = 31              # BN's four arrays come from their own generator: seed + this


def conditioned_inputs(st, dtype, seed):
    """conv_reference.conditioned_inputs (the map is O(1)) and BN blobs as bn_reference conditions them: mean
    0.5 N(0, 1), var from [0.5, 1.5], scale from [0.5, 1.5], shift 0.5 N(0, 1).  Read-only arrays."""
    c = CR.conditioned_inputs(st.conv, dtype, seed)
    out = {k: c[k] for k in ("x", "weight", "bias")}
    for k, v in _bn_arrays(st.conv.K, np.random.default_rng(seed + BN_SEED_OFFSET)).items():
        out[k] = np.ascontiguousarray(v.astype(dtype))
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def integer_probe(st, seed):
    """x, weight, bias as int64 in [-4, 4] (conv_reference.integer_probe): the map and every partial sum of a window are
    integers below probe_bound.  mean, var, scale, shift generic, in float32."""
    p = CR.integer_probe(st.conv, seed)
    out = {k: p[k] for k in ("x", "weight", "bias")}
    for k, v in _bn_arrays(st.conv.K, np.random.default_rng(seed + BN_SEED_OFFSET)).items():
        out[k] = np.ascontiguousarray(v.astype(np.float32))
    return out


def probe_bound(st):
    """The largest |partial sum| on integer_probe inputs in any order: of an element of the map, then of a window."""
    s = st.conv
    return st.pool[0] * st.pool[1] * (16 * (s.C // s.group) * s.kh * s.kw + 4)


def probe_outputs(st, inp):
    """The integer probe's exact map (int64, as float32) finished in float32 -> top, save_pool."""
    y = CR.conv_forward(st.conv, inp["x"], inp["weight"], inp["bias"]).astype(np.float32)
    return finish(y, st.pool, inp["mean"], inp["var"], inp["scale"], inp["shift"])


def model_outputs(st, inp, dtype):
    """{"top", "save_pool"} at `dtype` on inp (cast to it)."""
    c = {k: (None if v is None else v.astype(dtype)) for k, v in inp.items()}
    top, sp = forward(st, c["x"], c["weight"], c["bias"], c["mean"], c["var"], c["scale"], c["shift"])
    return dict(top=top, save_pool=sp)
