"""A float64 model of the TRAIN-phase tail (include/mms_train_tail.h), both passes, composed of the models its two calls
already have, imported as they are: conv_stage_train_reference for Convolution -> BN (batch statistics) -> pooling ->
TanH, head_reference in TRAIN phase on [Flatten(top) | overlap]; the backward runs them the other way round, the head's
x0_diff being the stage's top_diff.  Also here, for the three train-tail suites: the shape lists, the input generator and
the exact probe.
"""
import numpy as np

import conv_stage_train_reference as S
import head_reference as HR
from layer_plans import constants
from score_tail_reference import F0, T, Tail, head_shape, tail_id                  # noqa: F401 (the callers' names)

AVE, MAX = 0, 1                                  # MMS_STAGE_POOL_*
POOLS = (AVE, MAX)
METHOD = {AVE: S.AVE, MAX: S.MAX}                # conv_stage_train_reference's names
POOL_NAME = dict(METHOD)
IMAGES = constants("train_tail.hip", ["kTrainTailImages"])["kTrainTailImages"]
FINISH = HR.TILE                                 # samples of a workgroup of the fused route's second launch
BN_MEMORY = S.BN_MEMORY

FORWARD_OUTPUTS = ("y", "flt", "save_pool", "save_mean", "save_std", "running_mean", "running_var", "h", "prob", "loss")
BACKWARD_OUTPUTS = ("bottom_diff", "weight_diff", "bias_diff", "scale_diff", "shift_diff", "overlap_diff", "w1_diff",
                    "b1_diff", "w2_diff", "b2_diff")
ACCUMULATED = ("weight_diff", "bias_diff", "w1_diff", "b1_diff", "w2_diff", "b2_diff")


def small(N):
    """3 -> 5 channels, 3 x 3 on 6 x 6 under a 4 x 4 window; three overlap features, five hidden units: ragged MFMA rows
    and columns everywhere."""
    return T(N, 3, 6, 6, 5, 3, 3, (4, 4), 3, 5, 2)


def v4(N):
    """network_v4's tail: 32 x 9 x 9 -> 64 x 5 x 5 under a 5 x 5 window, four overlap features, 32 hidden units."""
    return T(N, 32, 9, 9, 64, 5, 5, (5, 5), 4, 32, 2)


def v5(N):
    """network_v5's last stage, 32 x 8 x 8 -> 32 x 6 x 6 under a 6 x 6 window, 32 hidden units."""
    return T(N, 32, 8, 8, 32, 3, 3, (6, 6), 2, 32, 2)


# one image; a full launch-1 workgroup and one image more; one and two workgroups of the second launch (the loss inside
# it and by the one-thread launch); more launch-1 workgroups than one fold step of 256 holds
SMALL_N = sorted({1, IMAGES, IMAGES + 1, FINISH, FINISH + 1, 257})
NET_N = (1, 50, FINISH + 1)
FUSED_TAILS = [small(N) for N in SMALL_N] + [v4(N) for N in NET_N] + [v5(N) for N in NET_N]
PAST_H = T(5, 3, 6, 6, 5, 3, 3, (4, 4), 3, HR.MAX_H + 1, 2)       # the head's fast limit: the plan refuses
STRIDED = T(2, 3, 10, 10, 4, 3, 3, (5, 5), 1, 4, 3, stride=2, pad=1)         # off the convolution's fast route
SEQUENCE_TAILS = [PAST_H, STRIDED]
GPU_TAILS = FUSED_TAILS + SEQUENCE_TAILS
NOT_WHOLE_MAP = T(3, 2, 6, 6, 3, 3, 3, (2, 2), 2, 5, 2)           # a 2 x 2 pooled map: refused


def cfg(norm=HR.VALID, ignore_label=None, ratio=0.5):
    return HR.Cfg(HR.TRAIN, ratio, norm, ignore_label)


HEAD_SEED_OFFSET = 223           # the head's arrays come from their own generator: seed + this


def conditioned_inputs(t, dtype, seed, config=None, ignored=False, out_of_range=False):
    """conv_stage_train_reference's conditioned inputs (the same for AVE and MAX; its top_diff is not used) and
    head_reference's for the head behind the stage.  Read-only arrays."""
    config = config or cfg()
    stage = S.conditioned_inputs(t.stage, dtype, seed)
    hd = HR.conditioned_inputs(head_shape(t), dtype, seed + HEAD_SEED_OFFSET, config, ignored, out_of_range)
    out = {k: stage[k] for k in ("x", "weight", "bias", "scale", "shift", "running_mean", "running_var", "weight_diff0",
                                 "bias_diff0")}
    out.update(overlap=hd["x1"], **{k: hd[k] for k in ("w1", "b1", "w2", "b2", "mask", "label", "loss_weight", "w1_diff0",
                                                       "b1_diff0", "w2_diff0", "b2_diff0")})
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _head_inputs(inp, flt, ty, with_label=True):
    c = lambda k: None if inp.get(k) is None else np.asarray(inp[k]).astype(ty)     # noqa: E731
    return dict(x0=flt, x1=c("overlap"), w1=c("w1"), b1=c("b1"), w2=c("w2"), b2=c("b2"), mask=inp["mask"],
                label=inp["label"] if with_label else None, loss_weight=inp.get("loss_weight", 1.0),
                w1_diff0=c("w1_diff0"), b1_diff0=c("b1_diff0"), w2_diff0=c("w2_diff0"), b2_diff0=c("b2_diff0"))


def forward(t, pool, inp, config=None, dtype=np.float64, with_label=True, bn_memory=BN_MEMORY):
    """-> {y, flt, save_pool, save_mean, save_std, running_mean, running_var, h, prob[, loss]} in `dtype`."""
    config = config or cfg()
    ty = np.dtype(dtype).type
    c = lambda k: None if inp[k] is None else np.asarray(inp[k]).astype(ty)         # noqa: E731
    y, top, sp, mean, std, rm, rv = S.forward(t.stage, METHOD[pool], c("x"), c("weight"), c("bias"), c("scale"),
                                              c("shift"), c("running_mean"), c("running_var"), ty(bn_memory))
    N = t.stage.conv.N
    flt = np.ascontiguousarray(top.reshape(N, -1))
    out = HR.forward(head_shape(t), config, _head_inputs(inp, flt, ty, with_label), dtype)
    out.update(y=y, flt=flt, save_pool=np.ascontiguousarray(sp.reshape(N, -1)), save_mean=mean, save_std=std,
               running_mean=rm, running_var=rv)
    return out


def backward(t, pool, inp, fwd, config=None, dtype=np.float64):
    """The ten diffs from what the forward left: head_reference.backward, then conv_stage_train_reference.backward with
    the head's x0_diff as top_diff.  bias_diff is absent without a bias, overlap_diff without overlap."""
    config = config or cfg()
    ty = np.dtype(dtype).type
    c = lambda k: None if inp[k] is None else np.asarray(inp[k]).astype(ty)         # noqa: E731
    hb = HR.backward(head_shape(t), config, _head_inputs(inp, fwd["flt"].astype(ty), ty), fwd["h"], fwd["prob"], dtype)
    pooled = S.pooled_shape(t.stage)
    dx, dw, db, dsc, dsh = S.backward(t.stage, METHOD[pool], c("x"), c("weight"), fwd["y"].astype(ty),
                                      fwd["flt"].astype(ty).reshape(pooled), hb["x0_diff"].reshape(pooled), c("scale"),
                                      c("shift"), fwd["save_mean"].astype(ty), fwd["save_std"].astype(ty),
                                      c("weight_diff0"), c("bias_diff0"))
    out = dict(bottom_diff=dx, weight_diff=dw, scale_diff=dsc, shift_diff=dsh,
               **{k: hb[k] for k in ("w1_diff", "b1_diff", "w2_diff", "b2_diff")})
    if db is not None:
        out["bias_diff"] = db
    if t.F1:
        out["overlap_diff"] = hb["x1_diff"]
    return out


def model_outputs(t, pool, inp, config=None, dtype=np.float64):
    """Forward, then backward from the forward's own outputs."""
    out = forward(t, pool, inp, config, dtype)
    out.update(backward(t, pool, inp, out, config, dtype))
    return out


# ---- the exact probe ---------------------------------------------------------------------------------------------
PROBE_MEMORY = S.PROBE_MEMORY


def integer_probe(t, seed):
    """conv_stage_train_reference.integer_probe for the stage -- y a small integer, every partial sum of y and y*y in
    any order exact in float32 (probe_sums asserts it) -- with real head weights behind it and every label but the first
    out of range: the loss is one term and zeros, the same word in any order.  Float32 arrays (x, weight, bias: integers
    as floats)."""
    st = S.integer_probe(t.stage, seed)
    S.probe_sums(t.stage, st)
    hd = HR.conditioned_inputs(head_shape(t), np.float32, seed + HEAD_SEED_OFFSET, cfg())
    label = np.full(t.stage.conv.N, -1.0, dtype=np.float32)
    label[0] = 1.0
    out = {k: (None if st[k] is None else st[k].astype(np.float32)) for k in
           ("x", "weight", "bias", "scale", "shift", "running_mean", "running_var", "weight_diff0", "bias_diff0")}
    out.update(overlap=hd["x1"], **{k: hd[k] for k in ("w1", "b1", "w2", "b2", "mask", "loss_weight", "w1_diff0",
                                                       "b1_diff0", "w2_diff0", "b2_diff0")}, label=label)
    return out
