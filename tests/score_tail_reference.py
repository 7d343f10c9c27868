"""A float64 model of the scoring tail (include/mms_score_tail.h), composed of the models its two calls already have,
imported as they are: conv_stage_reference (AVE) or conv_maxpool_stage_reference (MAX) for Convolution -> BN -> pooling
-> TanH, then head_reference in TEST phase on [Flatten(top) | overlap].  Also here, for the three score-tail suites: the
shape lists and the input generator.
"""
import collections

import numpy as np

import conv_maxpool_stage_reference as M
import conv_stage_reference as A
import head_reference as HR

AVE, MAX = 0, 1
POOLS = (AVE, MAX)
POOL_NAME = {AVE: "ave", MAX: "max"}

# stage: a conv_stage_reference.Stage; F1, H, C: the head's widths
Tail = collections.namedtuple("Tail", "stage F1 H C")


def T(N, C_, H_, W_, K, kh, kw, pool, F1, H, C, **kw_):
    return Tail(A.ST(N, C_, H_, W_, K, kh, kw, pool, **kw_), F1, H, C)


def v4(N):
    """network_v4's tail: 32 x 9 x 9 -> 64 x 5 x 5, a 5 x 5 window, two overlap features, 32 hidden units, 2 classes."""
    return T(N, 32, 9, 9, 64, 5, 5, (5, 5), 2, 32, 2)


def v5(N):
    """network_v5's last stage, 32 x 8 x 8 -> 32 x 6 x 6 under a 6 x 6 window, with network_v4_2's head behind it."""
    return T(N, 32, 8, 8, 32, 3, 3, (6, 6), 2, 64, 2)


# The smallest shapes at which each thing can go wrong.  The fused launch reaches all of these:
MINIMAL = [T(N, 2, 3, 3, 3, 2, 2, (2, 2), F1, 3, 2) for F1 in (0, 2) for N in (1, 3)]
# the fused launch takes three images per workgroup (csrc/score_tail.hip: kTailImages): 21 is seven full workgroups, 23
# leaves the last two images, 7 leaves it one
NETS = [v4(21), v4(23), v5(7)]
# just inside each of the head's fast limits, K + F1 = 128, H = 64, C = 16, at the fewest workgroups the main call
# fuses (17 of three images) ...
INSIDE = [T(50, 2, 3, 3, 64, 2, 2, (2, 2), 64, 3, 2), T(50, 2, 3, 3, 3, 2, 2, (2, 2), 2, 64, 2),
          T(50, 2, 3, 3, 3, 2, 2, (2, 2), 2, 3, 16)]
# ... and just past it: the sequence
PAST = [T(50, 2, 3, 3, 64, 2, 2, (2, 2), 65, 3, 2), T(50, 2, 3, 3, 3, 2, 2, (2, 2), 2, 65, 2),
        T(50, 2, 3, 3, 3, 2, 2, (2, 2), 2, 3, 17)]
# where mms_score_tail_route says FUSED: 17 to 506 workgroups; the driver's training batch is the fewest
MAIN_FUSED = INSIDE + [v4(50)]
# where the fused launch reaches but the route does not send the shape: fewer than 17 workgroups
FORCED_ONLY = MINIMAL + NETS
FUSED_TAILS = FORCED_ONLY + MAIN_FUSED
# a pooled map larger than 1 x 1 (2 x 2: F0 = 4 K); a strided convolution
SEQUENCE_TAILS = PAST + [T(3, 2, 6, 6, 3, 3, 3, (2, 2), 2, 5, 2), T(2, 3, 10, 10, 4, 3, 3, (5, 5), 1, 4, 3, stride=2, pad=1)]
GPU_TAILS = FUSED_TAILS + SEQUENCE_TAILS


def tail_id(t):
    return A.stage_id(t.stage) + "-F1_%d-H%d-C%d" % (t.F1, t.H, t.C)


def F0(t):
    _, K, POH, POW = A.pooled_shape(t.stage)
    return K * POH * POW


def head_shape(t):
    return HR.S(t.stage.conv.N, F0(t), t.F1, t.H, t.C)


def cfg(norm=HR.VALID, ignore_label=None):
    return HR.Cfg(HR.TEST, 0.5, norm, ignore_label)


OVERLAP_SEED_OFFSET = 211        # the head's arrays come from their own generator: seed + this


def conditioned_inputs(t, pool, dtype, seed, config=None, ignored=False, out_of_range=False):
    """The stage's conditioned inputs (MAX: with every scan direction among the channels) and head_reference's for the
    head behind it: overlap in [0, 1], Xavier-sized weights, labels as asked.  Read-only arrays."""
    config = config or cfg()
    stage = (M if pool == MAX else A).conditioned_inputs(t.stage, dtype, seed)
    hd = HR.conditioned_inputs(head_shape(t), dtype, seed + OVERLAP_SEED_OFFSET, config, ignored, out_of_range)
    out = dict(stage, overlap=hd["x1"], w1=hd["w1"], b1=hd["b1"], w2=hd["w2"], b2=hd["b2"], label=hd["label"])
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def forward(t, pool, inp, config=None, dtype=np.float64, with_label=True):
    """-> {"flt", "h", "prob"[, "loss"]} in `dtype`: the stage's model, Flatten, the head's model in TEST phase."""
    config = config or cfg()
    ty = np.dtype(dtype).type
    stage = M if pool == MAX else A
    top, _ = stage.forward(t.stage, *(None if inp[k] is None else inp[k].astype(ty)
                                      for k in ("x", "weight", "bias", "mean", "var", "scale", "shift")))
    flt = np.ascontiguousarray(top.reshape(top.shape[0], -1))
    hin = dict(x0=flt, x1=inp["overlap"], w1=inp["w1"], b1=inp["b1"], w2=inp["w2"], b2=inp["b2"], mask=None,
               label=inp["label"] if with_label else None)
    out = HR.forward(head_shape(t), config, hin, dtype)
    out["flt"] = flt
    return out
