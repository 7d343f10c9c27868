"""The three host-side launch plans of FM, BN and BN -> AvePool -> TanH restated in plain Python, and the shapes the plan
tests run (tests/test_layer_plans.py on the CPU, tests/test_gpu_layer_plans.py on the GPU).

fm_plan, bn_route and bp_route are line-for-line restatements of the C++ functions of those names; the named constants
they use are read from the two sources (csrc/fm.hip, csrc/bn_common.h) by regular expression, so a change to a constant
moves the model with it.  bn_route and bp_route are observable through the workspace queries and are held to them; FM's
plan is not observable: the model only proves that the FM list reaches each regime, and FM's results do not depend on
the plan -- which is what the GPU test checks.

The second half is the conditioning evidence for the new BN / BN-pool parity shapes: the layers' algebra in the inputs'
own dtype with every channel sum taken as the large route documents it -- one sum per chunk (numpy's own `sum` over the
chunk's elements), the chunk sums folded in ascending chunk order."""
import os
import re

import numpy as np

import bn_pool_reference as BP
import bn_reference as BN

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mms_answer_selection_amd", "csrc")


def constants(source, names):
    """{name: value} of `constexpr int|unsigned name = <product of integers and earlier constants>;` in csrc/<source>."""
    txt = open(os.path.join(CSRC, source)).read()
    found = dict(re.findall(r"constexpr\s+(?:int|unsigned)\s+(k\w+)\s*=\s*([^;]+);", txt))

    def value(name):
        assert name in found, "%s: no constexpr %s" % (source, name)
        out = 1
        for factor in found[name].split("*"):
            factor = factor.strip()
            assert re.fullmatch(r"\d+|k\w+", factor), "%s: %s = %s is not a product" % (source, name, found[name])
            out *= int(factor) if factor.isdigit() else value(factor)
        return out

    return {n: value(n) for n in names}


FM = constants("fm.hip", ["kFmLdsBytes", "kFmThreads"])
BNC = constants("bn_common.h", ["kBnSmallThreads", "kBnBatch", "kBnSmallGroups", "kBnChunkGroups", "kBnMaxChunks"])
SLOTS = 4                        # workspace words per (channel, chunk), include/mms.h


def fm_room(S):
    """Floats per sample and buffer of the lane-walk kernel's LDS image at S samples per workgroup (fm.hip, fm_plan):
    the largest stride that is a multiple of 4 with an odd quarter."""
    room = FM["kFmLdsBytes"] // 4 // (2 * S)
    room &= ~3
    if ((room >> 2) & 1) == 0:
        room -= 4
    return room


def fm_plan(N, C, dim):
    """csrc/fm.hip, fm_plan: (S, P, st) -- samples per workgroup, columns per panel, floats per sample image -- or None
    where the float calls take fm_forward_thread_kernel."""
    C1 = C + 1
    S = 64
    while S >= 8:
        if (N + S - 1) // S < 512 and S > 8:
            S //= 2
            continue
        room = fm_room(S)
        cols = dim - 1 if dim > 1 else 1
        if C1 > room or (S > 8 and room // C1 < (cols if cols < 8 else 8)):
            S //= 2
            continue
        P = room // C1
        if P > cols:
            P = cols
        np_ = (cols + P - 1) // P
        P = (cols + np_ - 1) // np_
        st = (P * C1 + 3) & ~3
        if ((st >> 2) & 1) == 0:
            st += 4
        return S, P, st
    return None


def fm_panels(dim, P):
    """Latent panels of the lane-walk kernel (its `np`): 0 when there is no latent column."""
    return (dim - 1 + P - 1) // P


def bn_route(N, S, itemsize):
    """csrc/bn.hip, bn_route<T>: (small, chunks, groups_per_chunk)."""
    V = 16 // itemsize
    total = N * S
    groups = (total + V - 1) // V
    if groups <= BNC["kBnSmallGroups"]:
        return True, 1, groups
    gpc = (groups + BNC["kBnMaxChunks"] - 1) // BNC["kBnMaxChunks"]
    if gpc < BNC["kBnChunkGroups"]:
        gpc = BNC["kBnChunkGroups"]
    return False, (groups + gpc - 1) // gpc, gpc


def bn_workspace_bytes(N, C, S, itemsize):
    """csrc/bn.hip, bn_workspace_bytes<T>, for a shape it accepts."""
    small, chunks, _ = bn_route(N, S, itemsize)
    return 0 if small else C * chunks * SLOTS * itemsize


def bp_least(kh, kw, itemsize):
    """Windows that hold kBnChunkGroups groups of x (csrc/bn_pool.hip, `least` of bp_route and bp_workspace_bytes)."""
    V = 16 // itemsize
    ke = kh * kw
    return (BNC["kBnChunkGroups"] * V + ke - 1) // ke


def bp_route(N, H, W, kh, kw, itemsize):
    """csrc/bn_pool.hip, bp_route<T>: (small, chunks, windows_per_chunk)."""
    V = 16 // itemsize
    ke = kh * kw
    total = N * H * W
    windows = total // ke
    if (total + V - 1) // V <= BNC["kBnSmallGroups"]:
        return True, 1, windows
    least = bp_least(kh, kw, itemsize)
    wpc = (windows + BNC["kBnMaxChunks"] - 1) // BNC["kBnMaxChunks"]
    if wpc < least:
        wpc = least
    return False, (windows + wpc - 1) // wpc, wpc


def bp_workspace_bytes(N, C, H, W, kh, kw, itemsize):
    """csrc/bn_pool.hip, bp_workspace_bytes<T>, for a shape it accepts: an upper bound on the chunks, not their count."""
    if bp_route(N, H, W, kh, kw, itemsize)[0]:
        return 0
    least = bp_least(kh, kw, itemsize)
    windows = N * H * W // (kh * kw)
    bound = min((windows + least - 1) // least, BNC["kBnMaxChunks"])
    return C * bound * SLOTS * itemsize


def chunk_bounds(count, per_chunk, chunks):
    """[(first, end)] of each chunk's groups or windows (bn_chunk / bp_chunk): whole chunks, the last one ragged."""
    out = [(k * per_chunk, min((k + 1) * per_chunk, count)) for k in range(chunks)]
    assert out[-1][1] == count and all(lo < hi for lo, hi in out)
    return out


# ---- the shapes --------------------------------------------------------------------------------------------------
# FM (N, C, dim) -> the S the model must give (None: no lane-walk plan), and what the shape is there for
FM_SHAPES = [
    ((8176, 2, 9), 8, "below the S = 16 threshold"),
    ((8177, 2, 9), 16, "at it: 512 workgroups, the last with one sample"),
    ((16352, 2, 9), 16, "below the S = 32 threshold"),
    ((16353, 2, 9), 32, "at it"),
    ((32704, 2, 9), 32, "below the S = 64 threshold"),
    ((32705, 2, 9), 64, "at it"),
    ((32705, 2, 100), 64, "four panels through both buffers"),
    ((32705, 2, 1), 64, "no latent panel"),
    ((32831, 3, 20), 64, "a last workgroup of 63 samples"),
    ((32705, 11, 9), 32, "64 -> 32 by panel width"),
    ((32705, 23, 9), 16, "32 -> 16 by panel width"),
    ((32705, 47, 9), 8, "16 -> 8 by panel width"),
    ((32705, 80, 3), 32, "64 -> 32 with two columns"),
    ((32705, 100, 2), 32, "64 -> 32 by C1 > room, one column"),
    ((3, 763, 2), 8, "the last lane-walk shape: C1 == room"),
    ((5, 764, 3), None, "the one-thread float route"),
    ((70, 800, 2), None, "the one-thread float route, two workgroups' worth of channels"),
    ((2048, 1, 2), 8, "bias_diff chain: one full step"),
    ((4096, 1, 2), 8, "bias_diff chain: two full steps"),
    ((2049, 1, 2), 8, "bias_diff chain: one step and one element"),
]
FM_PLACEMENT_SHAPE = (16353, 2, 9)

# BN (N, C, S) and BN-pool (N, C, H, W, kh, kw) with their element types: every one is past 64 chunks of the minimum
# size, so the chunk size is ceil(groups / 64) (ceil(windows / 64)) and the last chunk is ragged
BN_CASES = [
    ((405, 2, 1296), np.float32),        # 131,220 vectorised groups per channel
    ((4099, 1, 129), np.float32),        # odd runs: one access per element, the last group partial
    ((203, 2, 1296), np.float64),
]
BP_CASES = [
    ((405, 2, 36, 36, 4, 4), np.float32),        # network_v4's first window
    ((3652, 1, 12, 12, 12, 12), np.float32),     # 144-element windows: 63 chunks under a 64-chunk workspace
    ((203, 2, 36, 36, 4, 4), np.float64),
]
BP_63_CHUNKS = (3652, 1, 12, 12, 12, 12)
PROBE_MAX = 4                    # the integer probes: |x| <= 4


def case_id(case):
    return "%s-%s" % ("x".join(str(d) for d in case[0]), np.dtype(case[1]).name)


def probe_x(shape, dtype, seed):
    """Integer-valued x, |x| <= PROBE_MAX, of a BN (N, C, S) or BN-pool (N, C, H, W, ...) shape: every sum of x and of
    x*x over any part of a channel is an integer below 2^24, asserted from the shape, hence exact in any order."""
    dims = shape[:3] if len(shape) == 3 else shape[:4]
    per_channel = int(np.prod(dims)) // dims[1]
    assert per_channel * PROBE_MAX * PROBE_MAX < 2 ** 24
    return np.random.default_rng(seed).integers(-PROBE_MAX, PROBE_MAX + 1, size=dims).astype(dtype)


# ---- the layers' algebra with the large route's chunked sums -----------------------------------------------------
def _fold(rows, bounds):
    """(C, count) -> (C,): numpy's sum of each chunk [lo, hi) in rows' dtype, the chunk sums added in ascending order."""
    tot = None
    for lo, hi in bounds:
        s = rows[:, lo:hi].sum(axis=1, dtype=rows.dtype)
        tot = s if tot is None else tot + s
    assert tot.dtype == rows.dtype
    return tot


def bn_chunked_outputs(inp):
    """bn_reference.model_outputs' keys in the inputs' dtype, by the formulas of include/mms.h (mms_bn_*), the six
    channel sums chunked as bn_route cuts the channel's (n, s)-ordered elements."""
    x, dy, scale, shift = inp["x"], inp["dy"], inp["scale"], inp["shift"]
    N, C, S = x.shape
    t = x.dtype.type
    V = 16 // x.dtype.itemsize
    small, chunks, gpc = bn_route(N, S, x.dtype.itemsize)
    assert not small
    groups = (N * S + V - 1) // V
    bounds = [(lo * V, min(hi * V, N * S)) for lo, hi in chunk_bounds(groups, gpc, chunks)]
    c = (None, slice(None), None)

    def total(v):
        return _fold(np.ascontiguousarray(v.transpose(1, 0, 2)).reshape(C, N * S), bounds)

    out = {}
    for name, phase in (("train", BN.TRAIN), ("test", BN.TEST)):
        if phase == BN.TRAIN:
            mean = t(1.0 / N) * (t(1.0 / S) * total(x))
            var = t(1.0 / N) * (t(1.0 / S) * total(x * x)) - mean * mean
            keep, take = t(BN.BN_MEMORY), t(1) - t(BN.BN_MEMORY)
            rm, rv = take * mean + keep * inp["running_mean"], take * var + keep * inp["running_var"]
        else:
            mean, var, rm, rv = (inp[k].copy() for k in ("running_mean", "running_var", "running_mean", "running_var"))
        std = np.sqrt(var + t(BN.VAR_EPS))
        xn = (x + (-mean)[c]) / std[c]
        g = dy * scale[c]
        a, b = total(xn * g), total(g)
        dx = (g + t(-1.0 / (N * S)) * (xn * a[c] + b[c])) / std[c]
        out.update({name + "_top": xn * scale[c] + shift[c], name + "_save_mean": mean, name + "_save_std": std,
                    name + "_running_mean": rm, name + "_running_var": rv, name + "_bottom_diff": dx,
                    name + "_scale_diff": total(xn * dy), name + "_shift_diff": total(dy)})
    return out


def bp_chunked_outputs(inp, kernel):
    """bn_pool_reference.model_outputs' keys in the inputs' dtype, by the fused algebra of include/mms.h
    (mms_bn_pool_tanh_*): sum x and sum x*x over the elements of each chunk's windows, sum gp and sum gp*save_pool over
    each chunk's pooled elements, chunked as bp_route cuts the channel's (n, ph, pw)-ordered windows."""
    x, top_diff, scale, shift = inp["x"], inp["top_diff"], inp["scale"], inp["shift"]
    N, C, H, W = x.shape
    kh, kw = kernel
    t = x.dtype.type
    small, chunks, wpc = bp_route(N, H, W, kh, kw, x.dtype.itemsize)
    assert not small
    windows = N * (H // kh) * (W // kw)
    per_window = chunk_bounds(windows, wpc, chunks)
    per_element = [(lo * kh * kw, hi * kh * kw) for lo, hi in per_window]
    c = (None, slice(None), None, None)

    def total_x(v):                  # (N, C, H, W): window-major, a window's elements in (h, w) order
        w = v.reshape(N, C, H // kh, kh, W // kw, kw).transpose(1, 0, 2, 4, 3, 5)
        return _fold(np.ascontiguousarray(w).reshape(C, N * H * W), per_element)

    def total_pooled(v):             # (N, C, PH, PW)
        return _fold(np.ascontiguousarray(v.transpose(1, 0, 2, 3)).reshape(C, windows), per_window)

    out = {}
    for name, phase in (("train", BP.TRAIN), ("test", BP.TEST)):
        if phase == BP.TRAIN:
            mean = t(1.0 / N) * (t(1.0 / (H * W)) * total_x(x))
            var = t(1.0 / N) * (t(1.0 / (H * W)) * total_x(x * x)) - mean * mean
            keep, take = t(BP.BN_MEMORY), t(1) - t(BP.BN_MEMORY)
            rm, rv = take * mean + keep * inp["running_mean"], take * var + keep * inp["running_var"]
        else:
            mean, var, rm, rv = (inp[k].copy() for k in ("running_mean", "running_var", "running_mean", "running_var"))
        std = np.sqrt(var + t(BP.VAR_EPS))
        save_pool = (BP.ave_pool(x, kh, kw) + (-mean)[c]) / std[c]
        top = np.tanh(save_pool * scale[c] + shift[c])
        gp = top_diff * (1 - top * top)
        shift_diff, scale_diff = total_pooled(gp), total_pooled(gp * save_pool)
        a, b = scale * scale_diff, scale * shift_diff
        xn = (x + (-mean)[c]) / std[c]
        g = np.repeat(np.repeat(gp / t(kh * kw) * scale[c], kh, axis=2), kw, axis=3)
        dx = (g + t(-1.0 / (N * H * W)) * (xn * a[c] + b[c])) / std[c]
        for k, v in zip(BP.OUTPUTS, (top, save_pool, mean, std, rm, rv, dx, scale_diff, shift_diff)):
            out[name + "_" + k] = v
    return out


def worst_ratio(got, want, bar):
    """max over the outputs of (max |got - want|) / (bar * max(1, max |want|)): assert_close passes iff <= 1."""
    worst = 0.0
    for k in sorted(want):
        scale = max(1.0, float(np.max(np.abs(want[k]))))
        err = float(np.max(np.abs(got[k].astype(np.float64) - want[k])))
        print("%-22s %.3e" % (k, err / scale))
        worst = max(worst, err / (bar * scale))
    return worst
