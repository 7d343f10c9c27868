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
# One shape per instantiation of the pooling epilogue that the lists above (and the MaxPool and TRAIN suites' own) leave
# out: conv_stage_kernel<MT, MAX, PH, PW> and train_product_kernel<MT, MAX, PH, PW> are MT in {1, 2, 4} x AVE / MAX x the
# window forms of stage_pool_dispatch (AVE: 4 x 4, 5 x 5, run-time; MAX: 4 x 4, 2 x 2, run-time).  Each is the smallest
# that reaches what its comment names.  INSTANTIATION_PLANS has the plan each one claims as fields of what
# tests/native/conv_stage_plans_host.cpp prints from the C++ (tests/test_conv_stage_plans.py holds them to it, and
# computes from that output which kernels, kinds of workgroup, ragged channel tiles and tile rows the lists reach).  The
# convolution's own plan (rq = 1) has the same CC at every one, so fused and sequence cut the input channels alike.
INSTANTIATION = collections.OrderedDict([
    ("a", ST(2, 2, 34, 34, 64, 3, 3, (4, 4))),          # (MT 4, 4 x 4) on four bands of 8 rows; 64 x 256 words: the tile
                                                        # fills the LDS, its row is P (stage_tile_row's fallback)
    ("b", ST(9, 8, 10, 10, 64, 3, 3, (4, 4))),          # (4, 4 x 4) on four whole images, the fallback again; three
                                                        # workgroups, the last with one image
    ("c", ST(3, 3, 10, 10, 5, 3, 3, (4, 4))),           # (1, 4 x 4); three images where four fit
    ("d", ST(3, 3, 12, 12, 7, 3, 3, (5, 5))),           # AVE (1, 5 x 5); MAX (1, run-time)
    ("e", ST(2, 3, 22, 17, 20, 3, 3, (5, 5))),          # AVE (2, 5 x 5) on two bands of 10 rows; K = 20, a ragged second
                                                        # tile (TRAIN has no other); MAX (2, run-time)
    ("f", ST(2, 3, 14, 14, 33, 3, 3, (3, 2))),          # (4, run-time); K = 33: one channel in the third tile, the fourth
                                                        # empty; one whole image
    ("g", ST(3, 4, 18, 18, 47, 3, 3, (2, 2))),          # MAX (4, 2 x 2); AVE (4, run-time); K = 47; a 256-pixel image
    ("h", ST(5, 3, 8, 8, 9, 3, 3, (2, 2))),             # MAX (1, 2 x 2) on whole images, five where seven fit
    ("k", ST(2, 4, 17, 17, 40, 3, 3, (5, 5))),          # AVE 5 x 5 on one whole image; K = 40
    ("l", ST(2, 3, 14, 14, 17, 3, 3, (4, 4))),          # 4 x 4 on one whole image; K = 17, one past a tile
    ("m", ST(3, 20, 12, 12, 35, 3, 3, (5, 5))),         # a ragged MT = 4 (K = 35) across two chunks of channels (18 + 2)
    ("s", ST(2, 4, 23, 23, 64, 8, 8, (4, 4))),          # the LDS loop halves the band 16 -> 8 -> 4 rows in units of ph;
                                                        # chunks of 3 + 1; the convolution's own band is one row
])
# a and b without a bias: conv_tile_word's other branch in the tile's store, with the tile over the whole LDS
NO_BIAS = [ST(2, 2, 34, 34, 64, 3, 3, (4, 4), bias=False), ST(9, 8, 10, 10, 64, 3, 3, (4, 4), bias=False)]
INSTANTIATION_STAGES = list(INSTANTIATION.values()) + NO_BIAS
# kind: 0 several whole images per workgroup, 1 a band of rows, 2 one whole image; chunks of input channels, the last of
# last_chunk; fallback: the tile's row is P where the padded row does not fit
INSTANTIATION_PLANS = {
    "a": dict(kind=1, G=1, R=8, bands=4, MT=4, CC=2, chunks=1, P=256, PS=256, fallback=1),
    "b": dict(kind=0, G=4, R=8, bands=1, MT=4, CC=8, chunks=1, P=256, PS=256, fallback=1, groups=3, last_images=1),
    "c": dict(kind=0, G=4, R=8, bands=1, MT=1, CC=3, chunks=1, PS=260, fallback=0, last_images=3),
    "d": dict(kind=0, G=2, R=10, bands=1, MT=1, CC=3, chunks=1, fallback=0),
    "e": dict(kind=1, G=1, R=10, bands=2, MT=2, CC=3, chunks=1, fallback=0),
    "f": dict(kind=2, G=1, R=12, bands=1, MT=4, CC=3, chunks=1, fallback=0),
    "g": dict(kind=2, G=1, R=16, bands=1, MT=4, CC=4, chunks=1, P=256, PS=260, fallback=0),
    "h": dict(kind=0, G=7, R=6, bands=1, MT=1, CC=3, chunks=1, fallback=0, last_images=5),
    "k": dict(kind=2, G=1, R=15, bands=1, MT=4, CC=4, chunks=1, fallback=0),
    "l": dict(kind=2, G=1, R=12, bands=1, MT=2, CC=3, chunks=1, fallback=0),
    "m": dict(kind=0, G=2, R=10, bands=1, MT=4, CC=18, chunks=2, last_chunk=2, fallback=0),
    "s": dict(kind=1, G=1, R=4, bands=4, MT=4, CC=3, chunks=2, last_chunk=1, geo_R=16, own_R=1, fallback=0),
}
FUSED_STAGES = FUSED_STAGES + INSTANTIATION_STAGES
# Those the fused launch does not reach: the sequence route of every call:
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


# ---- the order probe: AVE's window sum is one chain in (h, w) order from 0 ----------------------------------------
ORDER_SEED = 20261023            # the draw meets ORDER_MIN_SHARE at every shape of ORDER_STAGES (tests/test_conv_stage_plans.py)
ORDER_MIN_SHARE = 0.1            # of a shape's windows, at least, differ in float32 under each of OTHER_ORDERS
ORDER_STAGES = list(INSTANTIATION.values()) + [V4_STAGES[0]]


def order_stage(st):
    """st without a bias: the order probe's map is one product per element."""
    return Stage(st.conv._replace(bias=False), st.pool)


def order_probe(st, seed):
    """Inputs on which every element of y is ONE exact product, whatever the chunking, and the window sums round, so
    the order of a window's additions shows in save_pool's words.  weight: one nonzero tap per output channel, +-2^j
    with j in -2 .. 2; input channel, tap and sign vary with k.  x = m 2^e with integer |m| <= 4096 and e in -8 .. 8.  No
    bias (st is an order_stage).  mean, var, scale, shift as conditioned_inputs', in float32."""
    s = st.conv
    assert not s.bias and s.group == 1
    r = np.random.default_rng(seed)
    m = r.integers(-4096, 4097, (s.N, s.C, s.H, s.W))
    # e uniform in -8 .. 8 tells the orders apart in 29 to 56 % of 4 x 4 and 5 x 5 windows, but in 0.5 to 7.4 % of 2 x 2 and
    # 3 x 2 ones (20 000 drawn per window): a window of fewer than 16 elements draws e from the two ends of the range,
    # which gives 12 to 43 %
    e = r.integers(-8, 9, m.shape) if st.pool[0] * st.pool[1] >= 16 else r.choice([-8, 8], m.shape)
    x = np.ldexp(m.astype(np.float64), e).astype(np.float32)
    weight = np.zeros((s.K, s.C, s.kh, s.kw), np.float32)
    for k in range(s.K):
        weight[k, k % s.C, (3 * k + 1) % s.kh, (5 * k + 2) % s.kw] = (-1.0 if k % 3 == 1 else 1.0) * 2.0 ** (k % 5 - 2)
    out = dict(x=x, weight=weight, bias=None)
    for k, v in _bn_arrays(s.K, np.random.default_rng(seed + BN_SEED_OFFSET)).items():
        out[k] = np.ascontiguousarray(v.astype(np.float32))
    return out


def order_probe_map(st, inp):
    """The order probe's map, exact in float32: each element is one tap's weight, a power of two, times one x."""
    y = CR.conv_forward(st.conv, inp["x"].astype(np.float64), inp["weight"].astype(np.float64), None)
    y32 = y.astype(np.float32)
    assert (y32.astype(np.float64) == y).all()
    return y32


def _window_elements(y, pool):
    """-> the ph * pw elements of every window as a list of (N, K, POH, POW) arrays, in (h, w) order"""
    ph, pw = pool
    return [y[:, :, i::ph, j::pw] for i in range(ph) for j in range(pw)]


def _chain(v):
    acc = np.zeros_like(v[0])
    for a in v:
        acc = acc + a
    return acc


def _pairwise(v):
    v = list(v)
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def order_shares(y, pool):
    """{order: the share of y's windows whose float32 sum under that order differs from the chain in (h, w) order from
    0}, for the orders a kernel could take by mistake: column-major, reversed, pairwise."""
    assert y.dtype == np.float32
    ph, pw = pool
    v = _window_elements(y, pool)
    hw = _chain(v)
    other = dict(column_major=_chain([v[i * pw + j] for j in range(pw) for i in range(ph)]), reversed=_chain(v[::-1]),
                 pairwise=_pairwise(v))
    return {k: float((o != hw).mean()) for k, o in other.items()}


def model_outputs(st, inp, dtype):
    """{"top", "save_pool"} at `dtype` on inp (cast to it)."""
    c = {k: (None if v is None else v.astype(dtype)) for k, v in inp.items()}
    top, sp = forward(st, c["x"], c["weight"], c["bias"], c["mean"], c["var"], c["scale"], c["shift"])
    return dict(top=top, save_pool=sp)
