"""The TRAIN-phase stage Convolution -> BN -> AvePool / MaxPool -> TanH (include/mms_conv_stage_train.h) as numpy, both
passes: the layers of tests/conv_reference.py and tests/bn_pool_reference.py / tests/bn_maxpool_reference.py (phase
TRAIN) in sequence, generic over the dtype; the conditioned inputs of the GPU parity tests with their conditions
checked here; the large shapes with the plans they claim, their forward-only conditioning and the fused route's order of
sums in float32 numpy; and the exact probe, whose statistics are restated in float32 from int64 sums.

    x (N, C, H, W)   weight (K, C/group, kh, kw)   bias, scale, shift, running_mean, running_var (K)
    y (N, K, OH, OW)   top, save_pool, top_diff (N, K, OH/ph, OW/pw)
"""
import numpy as np

import bn_maxpool_reference as BM
import bn_pool_reference as BP
import conv_reference as CR
import conv_stage_reference as SR
from conv_stage_reference import ST, pooled_shape, stage_id                    # noqa: F401 (the callers' names)

AVE, MAX = "ave", "max"
METHODS = (AVE, MAX)
BN_MEMORY, VAR_EPS = BP.BN_MEMORY, BP.VAR_EPS

# The shapes of tests/test_gpu_conv_stage_train.py: the smallest that reach each launch geometry of the fused route.
A = ST(3, 4, 28, 28, 32, 5, 5, (4, 4))          # 24 x 24: three bands of 8 rows per image, one input-channel chunk
B = ST(23, 32, 9, 9, 64, 5, 5, (5, 5))          # 5 x 5: ten whole images per workgroup, the last group of three;
                                                # several input-channel chunks; K x 256 fills the LDS tile
C = ST(1, 3, 12, 12, 5, 3, 3, (2, 2))           # 10 x 10: one workgroup, K = 5 no multiple of the MFMA tile
D = ST(3, 4, 28, 28, 32, 5, 5, (4, 4), group=2)  # A off the fast route: the SEQUENCE route in float
E = ST(4, 3, 12, 12, 8, 5, 5, (4, 4))           # 8 x 8, N * OH * OW = 256: the exact probe's mean is exact
F = ST(2, 3, 22, 22, 7, 3, 3, (4, 4))           # 20 x 20: the window makes the band higher (12 rows) than the
                                                # convolution's own (10); bands of 12 and 8 rows
G = ST(2, 32, 24, 24, 32, 5, 5, (4, 4))         # 20 x 20 again, 32 channels: a band of 12 rows holds 13 input channels
                                                # where the convolution's own 10 rows hold 14, so the fused plan
                                                # halves its band to 8 rows to keep the convolution's chunk
# conv_stage_reference's shapes, one per instantiation of the pooling epilogue (train_product_kernel<MT, MAX, PH, PW>:
# the same window forms, and TK = 256 / (16 MT) lanes folding a channel's sums), the two without a bias included.  What
# each reaches is there; tests/test_conv_stage_plans.py holds it to the C++, train_plan's figures among them.
I = SR.INSTANTIATION
Ia, Ib, Ic, Id, Ie, If, Ig, Ih, Ik, Il, Im, Is = (I[k] for k in "abcdefghklms")
INSTANTIATION_STAGES = SR.INSTANTIATION_STAGES
# The exact probe's mean is exact where N * OH * OW is a power of two (Ia's 2048 and Is's 512 are): where the batch alone
# keeps a shape above from it, the nearest batch that gives one; Il on a 16 x 16 map.  (Id, Ie, If, Ih, Ik and Im have maps of
# 100, 300, 144, 36, 225 and 100 pixels: no batch does.)
Ib8 = ST(8, 8, 10, 10, 64, 3, 3, (4, 4))        # 512: two full workgroups of four images
Ic4 = ST(4, 3, 10, 10, 5, 3, 3, (4, 4))         # 256: the four images that fit
Ig4 = ST(4, 4, 18, 18, 47, 3, 3, (2, 2))        # 1024
Il4 = ST(4, 3, 18, 18, 17, 3, 3, (4, 4))        # 1024: 4 x 4 on one whole 16 x 16 image, K = 17
EXACT_MEAN_STAGES = [Ib8, Ic4, Ig4, Il4]
# TRAIN alone: none of the shapes above has MT = 2 under a 2 x 2 window, which the TEST-phase lists have of their own.
# K = 20 on two whole 10 x 10 images per workgroup, the last workgroup with one: AVE (2, run-time), MAX (2, 2 x 2)
It = ST(3, 3, 12, 12, 20, 3, 3, (2, 2))
TRAIN_ONLY_STAGES = [It]
FUSED_STAGES = [A, B, C, E, F, G] + INSTANTIATION_STAGES + EXACT_MEAN_STAGES + TRAIN_ONLY_STAGES
SEQUENCE_STAGES = [D]
GPU_STAGES = FUSED_STAGES + SEQUENCE_STAGES
PARITY_STAGES = [A, B, C, D]

# The shapes at which the fused forward's two launches take the sizes the main call routes to them (kTrainSpans), each
# with the claim it is there for.  LARGE_PLANS has the claims as fields of what tests/native/
# conv_stage_train_plans_host.cpp prints from the C++ (tests/test_conv_stage_train_plans.py holds them to it): launch 1's
# plan, launch 2's grid and the route of the main call per method.
P = ST(41, 3, 12, 12, 5, 3, 3, (2, 2))          # 2 images per workgroup, 21 workgroups, the last with one image; 1025
                                                # pooled elements per channel: 2 chunks in launch 2, the second holds one
Q = ST(513, 3, 12, 12, 5, 3, 3, (2, 2))         # 257 workgroups: thread 0 of launch 2 adds two partials, the last image
                                                # group is ragged; 12825 pooled elements: 13 chunks, the last of 537
R = ST(225, 3, 22, 22, 7, 3, 3, (4, 4))         # F at the batch where its bands of 12 and 8 rows are 450 workgroups: the
                                                # main call FUSES, AVE and MAX; 5625 pooled elements: 6 chunks
R_MINUS = ST(224, 3, 22, 22, 7, 3, 3, (4, 4))   # 448 workgroups: one step below both spans
R_PLUS = ST(226, 3, 22, 22, 7, 3, 3, (4, 4))    # 452 workgroups: past AVE's span, inside MAX's
W = ST(657, 2, 22, 22, 4, 3, 3, (2, 2))         # two bands of 10 rows, 1314 workgroups (blockIdx.x up to 656); 65700
                                                # pooled elements: past the cap of 64 chunks, 1027 each, the last of 999
LARGE_STAGES = [P, Q, R, R_MINUS, R_PLUS, W]
SEQ, FUSED = "sequence", "fused"
LARGE_PLANS = {
    P: dict(plan=dict(kind=0, G=2, R=10, bands=1, groups=21, last_images=1, CC=3, MT=1),
            finish=dict(windows=1025, wpc=1024, chunks=2, last=1), route={AVE: SEQ, MAX: SEQ}),
    Q: dict(plan=dict(kind=0, G=2, R=10, bands=1, groups=257, last_images=1, CC=3, MT=1),
            finish=dict(windows=12825, wpc=1024, chunks=13, last=537), route={AVE: SEQ, MAX: SEQ}),
    R: dict(plan=dict(kind=1, G=1, R=12, bands=2, last_rows=8, groups=450, CC=3, MT=1),
            finish=dict(windows=5625, wpc=1024, chunks=6, last=505), route={AVE: FUSED, MAX: FUSED}),
    R_MINUS: dict(plan=dict(kind=1, G=1, R=12, bands=2, last_rows=8, groups=448, CC=3, MT=1),
                  finish=dict(windows=5600, wpc=1024, chunks=6, last=480), route={AVE: SEQ, MAX: SEQ}),
    R_PLUS: dict(plan=dict(kind=1, G=1, R=12, bands=2, last_rows=8, groups=452, CC=3, MT=1),
                 finish=dict(windows=5650, wpc=1024, chunks=6, last=530), route={AVE: SEQ, MAX: FUSED}),
    W: dict(plan=dict(kind=1, G=1, R=10, bands=2, last_rows=10, groups=1314, CC=2, MT=1),
            finish=dict(windows=65700, wpc=1027, chunks=64, last=999), route={AVE: SEQ, MAX: FUSED}),
}
FOLD_THREADS, WAVE = 256, 64     # launch 2: kBnThreads threads fold the partials, csrc/bn_common.h; a wave's lanes

GAP = BM.GAP                     # the least top-two gap of a window's BN outputs, relative to max(1, |y|)
MIN_VAR, MIN_SCALE = 1e-2, 0.5
BN_SEED_OFFSET, RETRY_STEP = 41, 7919
# top_diff ~ 0.1 N(0, 1), conv_reference's own scale.  bias_diff is the sum of dy over a channel, which BN's backward makes
# the difference of two sums of size |scale * shift_diff| that cancel exactly in the model: in float that difference
# carries about 1e-7 of their size, so the size is held below MAX_CANCELLING (tests/test_conv_stage_train_reference.py).
TOP_DIFF_SCALE, MAX_CANCELLING = 0.1, 8.0
OUTPUTS = ("y", "top", "save_pool", "save_mean", "save_std", "running_mean", "running_var", "bottom_diff",
           "weight_diff", "bias_diff", "scale_diff", "shift_diff")
FORWARD_OUTPUTS = OUTPUTS[:7]


def _bn(method):
    return BP if method == AVE else BM


def forward(st, method, x, weight, bias, scale, shift, running_mean, running_var, bn_memory=BN_MEMORY):
    """-> y, top, save_pool, save_mean, save_std, running_mean, running_var: the convolution, then the three layers."""
    y = CR.conv_forward(st.conv, x, weight, bias)
    return (y,) + tuple(_bn(method).forward(y, st.pool, scale, shift, running_mean, running_var, bn_memory, BP.TRAIN))


def backward(st, method, x, weight, y, top, top_diff, scale, shift, save_mean, save_std, weight_diff0, bias_diff0):
    """-> bottom_diff, weight_diff, bias_diff (the diffs passed plus this batch's, None without a bias), scale_diff,
    shift_diff."""
    if method == AVE:
        dy, dscale, dshift = BP.backward(y, st.pool, top, top_diff, scale, save_mean, save_std)
    else:
        dy, dscale, dshift = BM.backward(y, st.pool, top, top_diff, scale, shift, save_mean, save_std)
    dx, dw, db = CR.conv_backward(st.conv, x, weight, dy, weight_diff0, bias_diff0)
    return dx, dw, db, dscale, dshift


def model_outputs(st, method, inp, dtype):
    """Every output of both passes at `dtype` on inp (cast to it); bias_diff is absent without a bias."""
    c = {k: (None if v is None else np.asarray(v).astype(dtype)) for k, v in inp.items()}
    f = forward(st, method, c["x"], c["weight"], c["bias"], c["scale"], c["shift"], c["running_mean"], c["running_var"])
    y, top, _, mean, std = f[:5]
    b = backward(st, method, c["x"], c["weight"], y, top, c["top_diff"], c["scale"], c["shift"], mean, std,
                 c["weight_diff0"], c["bias_diff0"])
    out = dict(zip(OUTPUTS, f + b))
    if out["bias_diff"] is None:
        del out["bias_diff"]
    return out


def _draw(st, dtype, seed):
    c = CR.conditioned_inputs(st.conv, dtype, seed)
    out = {k: c[k] for k in ("x", "weight", "bias", "weight_diff0", "bias_diff0")}
    r, K = np.random.default_rng(seed + BN_SEED_OFFSET), st.conv.K
    bn = dict(scale=r.uniform(MIN_SCALE, 1.5, K) * r.choice([-1.0, 1.0], K), shift=0.5 * r.standard_normal(K),
              running_mean=0.5 * r.standard_normal(K), running_var=r.uniform(0.5, 1.5, K),
              top_diff=TOP_DIFF_SCALE * r.standard_normal(pooled_shape(st)))
    if K >= 2:
        bn["scale"][0], bn["scale"][1] = abs(bn["scale"][0]), -abs(bn["scale"][1])
    for k, v in bn.items():
        out[k] = np.ascontiguousarray(v.astype(dtype))
    return out


def conditions(st, inp):
    """-> (least variance of a channel of y, least |scale|, least top-two gap of a window's BN outputs) of the float64
    model on inp."""
    c = {k: (None if v is None else v.astype(np.float64)) for k, v in inp.items()}
    y = CR.conv_forward(st.conv, c["x"], c["weight"], c["bias"])
    mean, var = y.mean(axis=(0, 2, 3)), y.var(axis=(0, 2, 3))
    bn = (y - mean[None, :, None, None]) / np.sqrt(var + VAR_EPS)[None, :, None, None] \
        * c["scale"][None, :, None, None] + c["shift"][None, :, None, None]
    return float(var.min()), float(np.abs(c["scale"]).min()), float(BM.top_two_gap(bn, *st.pool).min())


def conditioned(st, inp):
    var, scale, gap = conditions(st, inp)
    return var >= MIN_VAR and scale >= MIN_SCALE and gap >= GAP


def conditioned_inputs(st, dtype, seed):
    """conv_reference.conditioned_inputs (y is O(1)) with |scale| from [0.5, 1.5] of either sign (channel 0 positive,
    channel 1 negative), shift and running_mean 0.5 N(0, 1), running_var from [0.5, 1.5], top_diff 0.1 N(0, 1); drawn again
    from seed + RETRY_STEP, ... until `conditioned` holds: every window's maximum of BN's output is GAP away from the
    runner-up, so the float mask is the model's, every channel's variance is far above 1e-9 and |scale| >= 0.5.
    The same inputs serve AVE and MAX.  Read-only arrays."""
    for attempt in range(200):
        out = _draw(st, dtype, seed + RETRY_STEP * attempt)
        if conditioned(st, out):
            for v in out.values():
                if v is not None:
                    v.setflags(write=False)
            return out
    raise AssertionError("no conditioned inputs for %s" % (st,))


def forward_conditioned(st, inp):
    var, scale, _ = conditions(st, inp)
    return var >= MIN_VAR and scale >= MIN_SCALE


def forward_conditioned_inputs(st, dtype, seed):
    """conditioned_inputs' draws with the variance and the scale condition only.  The top-two gap protects the backward's
    mask; it cannot hold over the 10^4 to 10^5 windows of LARGE_STAGES, whose parity is forward-only -- the forward's
    extremum is continuous in y, whichever element attains it.  Read-only arrays."""
    for attempt in range(200):
        out = _draw(st, dtype, seed + RETRY_STEP * attempt)
        if forward_conditioned(st, out):
            for v in out.values():
                if v is not None:
                    v.setflags(write=False)
            return out
    raise AssertionError("no forward-conditioned inputs for %s" % (st,))


def model_forward(st, method, inp):
    """The seven forward outputs of the float64 model on inp (cast to float64), under FORWARD_OUTPUTS' names."""
    c = {k: (None if v is None else np.asarray(v).astype(np.float64)) for k, v in inp.items()}
    return dict(zip(FORWARD_OUTPUTS, forward(st, method, c["x"], c["weight"], c["bias"], c["scale"], c["shift"],
                                             c["running_mean"], c["running_var"])))


# ---- the fused route's statistics in float32 ---------------------------------------------------------------------
def _tree_sum(v):
    """(..., 2^k) -> (...): adjacent pairs, then pairs of pairs, ...: the shape of wave_sum's butterfly (csrc/mms_common.h)."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def fused_partials(y, G, R, bands):
    """Launch 1 as the fused route documents it: (K, groups, 2) float32, sum y and sum y*y of the real pixels of
    workgroup wg = image group * bands + band -- G images, rows [band R, band R + R) of each, the last group and the last
    band what is left -- each one numpy sum in float32."""
    f = np.float32
    assert y.dtype == f
    N, K = y.shape[:2]
    gx = (N + G - 1) // G
    part = np.zeros((K, gx * bands, 2), f)
    for bx in range(gx):
        for by in range(bands):
            blk = y[bx * G:(bx + 1) * G, :, by * R:(by + 1) * R]
            assert blk.size
            part[:, bx * bands + by, 0] = blk.sum(axis=(0, 2, 3), dtype=f)
            part[:, bx * bands + by, 1] = (blk * blk).sum(axis=(0, 2, 3), dtype=f)
    return part


def fold_partials(part):
    """Launch 2's prologue: thread t of FOLD_THREADS adds the partials of workgroups t, t + 256, ... ascending from 0,
    then bn_block_sum -- a butterfly inside each wave, the waves ascending.  (K, groups, 2) -> (K, 2), float32."""
    f = np.float32
    K, groups = part.shape[:2]
    rounds = (groups + FOLD_THREADS - 1) // FOLD_THREADS
    padded = np.zeros((K, rounds * FOLD_THREADS, 2), f)
    padded[:, :groups] = part
    tot = np.zeros((K, FOLD_THREADS, 2), f)
    for r in range(rounds):
        tot = tot + padded[:, r * FOLD_THREADS:(r + 1) * FOLD_THREADS]
    waves = _tree_sum(tot.reshape(K, FOLD_THREADS // WAVE, WAVE, 2).transpose(0, 1, 3, 2))      # (K, waves, 2)
    out = waves[:, 0]
    for w in range(1, FOLD_THREADS // WAVE):
        out = out + waves[:, w]
    assert out.dtype == f
    return out


def statistics_f32(st, inp, s0, s1, memory, N=None):
    """bn_statistics (csrc/bn_common.h) in float32 from the two channel sums, every step one rounded operation.
    -> save_mean, save_std, running_mean, running_var."""
    f = np.float32
    OH, OW = CR.output_dims(st.conv)
    inv_S, inv_N = f(1.0 / (OH * OW)), f(1.0 / (st.conv.N if N is None else N))
    mean = inv_N * (inv_S * s0.astype(f))
    var = inv_N * (inv_S * s1.astype(f)) - mean * mean
    std = np.sqrt(var + f(VAR_EPS))
    keep, take = f(memory), f(1) - f(memory)
    return mean, std, take * mean + keep * inp["running_mean"].astype(f), take * var + keep * inp["running_var"].astype(f)


def fused_statistics_f32(st, inp, G, R, bands, memory=BN_MEMORY):
    """save_mean, save_std, running_mean, running_var as float32 arithmetic alone gives them on the fused route's order of
    sums: y is the float64 model's map rounded to float32, summed by fused_partials and fold_partials."""
    c = {k: inp[k].astype(np.float64) for k in ("x", "weight")}
    bias = None if inp["bias"] is None else inp["bias"].astype(np.float64)
    y = CR.conv_forward(st.conv, c["x"], c["weight"], bias).astype(np.float32)
    tot = fold_partials(fused_partials(y, G, R, bands))
    return dict(zip(FORWARD_OUTPUTS[3:], statistics_f32(st, inp, tot[:, 0], tot[:, 1], memory)))


# ---- the order probe (AVE) ----------------------------------------------------------------------------------------
ORDER_STAGES = SR.ORDER_STAGES


def order_probe(st, seed):
    """conv_stage_reference.order_probe's x and weight (st an order_stage: no bias; every element of y one exact
    product, window sums that round) with _draw's scale, shift and running blobs; top_diff is not used."""
    p = SR.order_probe(st, seed)
    d = _draw(st, np.float32, seed)
    return dict(x=p["x"], weight=p["weight"], bias=None, weight_diff0=None, bias_diff0=None, top_diff=d["top_diff"],
                **{k: d[k] for k in ("scale", "shift", "running_mean", "running_var")})


def order_probe_forward(st, inp, y):
    """The fused TRAIN forward of bn_pool_reference in float32 on the exact map y: the window added in (h, w) order from
    0, the statistics by plainly sequential sums.  -> {top, save_pool, save_mean, save_std, running_mean, running_var}"""
    assert y.dtype == np.float32
    out = BP.fused_forward(y, st.pool, inp["scale"], inp["shift"], inp["running_mean"], inp["running_var"], BN_MEMORY, BP.TRAIN)
    return dict(zip(FORWARD_OUTPUTS[1:], out))


# ---- the exact probe ---------------------------------------------------------------------------------------------
PROBE_MEMORY = 0.5               # bn_memory of the probe: 1 - 0.5 is exact
ZERO_CHANNEL, NEGATIVE_CHANNEL, POSITIVE_CHANNEL = 0, 1, 2


def integer_probe(st, seed):
    """x and weight int64 in {-1, 0, 1}, bias int64 in [-2, 2]: y is a small integer, its windows are full of ties
    (channels 0, 1 and 2 read one tap of x: every window of theirs has them), and sum y and sum y*y over a channel are
    integers below 2^24 (probe_sums asserts it).  scale has an exact 0, a negative and a positive channel; shift, the
    running blobs and top_diff are dyadic."""
    r, s = np.random.default_rng(seed), st.conv
    out = dict(x=r.integers(-1, 2, (s.N, s.C, s.H, s.W), dtype=np.int64),
               weight=r.integers(-1, 2, (s.K, s.C // s.group, s.kh, s.kw), dtype=np.int64),
               bias=r.integers(-2, 3, (s.K,), dtype=np.int64) if s.bias else None)
    K = s.K
    for k in (ZERO_CHANNEL, NEGATIVE_CHANNEL, POSITIVE_CHANNEL):       # planted ties: these channels' y is one tap of x
        out["weight"][k] = 0
        out["weight"][k, 0, k % s.kh, k % s.kw] = 1
    scale = r.integers(1, 5, K).astype(np.float32) / 4 * r.choice([-1.0, 1.0], K).astype(np.float32)
    scale[ZERO_CHANNEL], scale[NEGATIVE_CHANNEL] = 0.0, -abs(scale[NEGATIVE_CHANNEL])
    scale[POSITIVE_CHANNEL] = abs(scale[POSITIVE_CHANNEL])
    out.update(scale=scale, shift=r.integers(-4, 5, K).astype(np.float32) / 8,
               running_mean=r.integers(-8, 9, K).astype(np.float32) / 4,
               running_var=r.integers(1, 9, K).astype(np.float32) / 4,
               top_diff=r.integers(-4, 5, pooled_shape(st)).astype(np.float32) / 4,
               weight_diff0=r.integers(-4, 5, out["weight"].shape).astype(np.float32),
               bias_diff0=r.integers(-4, 5, (K,)).astype(np.float32) if s.bias else None)
    return out


def probe_sums(st, inp, images=None):
    """-> y (int64), sum y, sum y*y per channel (int64) over `images` (a slice; default all).  Every partial sum of
    either, in any order, is bounded by sum |y| and sum y*y: both asserted below 2^24, so float32 holds them exactly."""
    y = CR.conv_forward(st.conv, inp["x"], inp["weight"], inp["bias"])
    part = y if images is None else y[images]
    s0, s1 = part.sum(axis=(0, 2, 3)), (part * part).sum(axis=(0, 2, 3))
    assert np.abs(part).sum(axis=(0, 2, 3)).max() < 2 ** 24 and s1.max() < 2 ** 24
    return y, s0, s1


def probe_statistics(st, inp, s0, s1, N=None):
    """bn_statistics (csrc/bn_common.h) in float32 from the exact sums: every step one correctly rounded operation, so
    these are the library's words.  -> save_mean, save_std, running_mean, running_var."""
    return statistics_f32(st, inp, s0, s1, PROBE_MEMORY, N)
