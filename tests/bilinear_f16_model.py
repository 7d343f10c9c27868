"""The fp16-storage bilinear word-grid family (csrc/bilinear_f16.hip behind mms_simcross_bilinear_forward_f16, _backward_f16,
_forward_backward_f16 and mms_embed_simcross_bilinear_forward_f16): the host routing restated in Python, the shape table that reaches
every kernel instantiation, and the inputs.  q (N, W1, D), a (N, W2, D), dq, da and the embedding table halves; W (M, D, D), bias, dbias
(M, W1, W2), top, top_diff (N, M, W1, W2), dW fp32.

Routing, one function per host decision (csrc/bilinear_pair.h, csrc/bilinear_f16.hip, csrc/mms_abi.hip):
  refusal         bilinear_f16_refusal: dims_ok(2, ...) else INVALID_ARG; W1 == W2 == 1 UNSUPPORTED
  pair_bwd_ok     pair_bwd_eligible: W1, W2 <= 48, D <= 64, W1 W2 > 1, N <= 256, N M <= 65535
  fwd_route       pair_fwd_route + pair_fwd_launch: ("eval", 13 | 16) for N >= 512 on grids that fit, ("train", 13 | 16) when
                  pair_bwd_ok, else ("generic",); KS = 13 for D <= 52
  bwd_route       pair_bwd_launch: ("fused", (10, 13) | (12, 16), "direct" | "reduced") when pair_bwd_ok -- (10, 13) for W1, W2 <= 40 and
                  D <= 52; "direct": M == 1, the kernel stores the dq / da halves; "reduced": M > 1, the grouped half reduction -- else
                  ("generic",): widen, the fp32 layer, narrow
  stage_width     half_stage_width: halves per staging load of a fused kernel, 8, 2 or 1, the widest that q's and a's addresses and the
                  lengths W1 D, W2 D (with the Embed gather: the table's address and D) allow
  embed_refusal   mms_embed_simcross_bilinear_forward_f16: dims_ok, K > 0, K D <= 2^31 - 1; UNSUPPORTED where fwd_route is generic
  scratch         bilinear_f16_ws: the four fp32 arrays of the generic route exist unless both directions are fused

What the kernels are held to (tests/test_gpu_bilinear_f16.py): top, dW, dbias the 32-bit words of the fp32 entry point on the widened
inputs; dq, da that call's gradients rounded once to half, 16-bit word for word; the CPU oracle at the suite's bars.

CPU only; tests/test_bilinear_f16_model.py proves this module.
"""
import numpy as np

import bilinear_grid_model as gm

OK, INVALID_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3          # include/mms.h
FB_W, FB_D = 48, 64


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def refusal(N, W1, W2, D, M):
    lim = 0x7fffffff
    if N < 0 or W1 <= 0 or W2 <= 0 or D <= 0 or M <= 0:
        return INVALID_ARG
    if N * W1 * D > lim or N * W2 * D > lim or N * M * W1 * W2 > lim:
        return INVALID_ARG
    if W1 == 1 and W2 == 1:
        return UNSUPPORTED
    return OK


def pair_bwd_ok(N, W1, W2, D, M):
    return W1 <= FB_W and W2 <= FB_W and D <= FB_D and W1 * W2 > 1 and N <= 256 and N * M <= 65535


def fwd_route(N, W1, W2, D, M):
    ks = 13 if D <= 52 else 16
    if W1 <= FB_W and W2 <= FB_W and D <= FB_D and W1 * W2 > 1 and N >= 512:
        return ("eval", ks)
    if pair_bwd_ok(N, W1, W2, D, M):
        return ("train", ks)
    return ("generic",)


def bwd_route(N, W1, W2, D, M):
    if not pair_bwd_ok(N, W1, W2, D, M):
        return ("generic",)
    return ("fused", (10, 13) if W1 <= 40 and W2 <= 40 and D <= 52 else (12, 16), "direct" if M == 1 else "reduced")


def stage_width(W1, W2, D, q=0, a=0, gather=False):
    """q, a: addresses of the pair's first elements (the table's, twice, with the gather)."""
    addr = q | a
    length = D if gather else (W1 * D) | (W2 * D)
    if addr % 16 == 0 and length % 8 == 0:
        return 8
    if addr % 4 == 0 and length % 2 == 0:
        return 2
    return 1


def embed_refusal(N, W1, W2, D, M, K):
    if refusal(N, W1, W2, D, M) == INVALID_ARG or K <= 0 or K * D > 0x7fffffff:
        return INVALID_ARG
    if N == 0:
        return OK
    return UNSUPPORTED if fwd_route(N, W1, W2, D, M) == ("generic",) else OK


def scratch(N, W1, W2, D, M):
    return fwd_route(N, W1, W2, D, M) == ("generic",) or bwd_route(N, W1, W2, D, M) == ("generic",)


FWD_REACHABLE = {("eval", 13), ("eval", 16), ("train", 13), ("train", 16), ("generic",)}
BWD_REACHABLE = {("fused", k, s) for k in ((10, 13), (12, 16)) for s in ("direct", "reduced")} | {("generic",)}
UNREACHABLE = set()

# ----------------------------------------------------------------------------------------------------------------------
# the shape table (N, W1, W2, D, M, bias): the smallest shapes at which each kernel can still go wrong
# ----------------------------------------------------------------------------------------------------------------------
EVAL = [(512, 5, 7, 50, 2, True),         # <13>: ragged single tile, 100-byte rows
        (513, 40, 40, 52, 4, True),       # <13>: the full driver grid, last D of KS = 13
        (512, 17, 33, 53, 1, False),      # <16>: odd D, rows only 2-byte aligned, several ragged tiles
        (512, 48, 48, 64, 2, True)]       # <16>: the limits
TRAIN = [(3, 5, 7, 50, 4, True),          # <10, 13>
         (2, 40, 40, 52, 1, False),       # <10, 13>: M == 1, direct half stores
         (1, 1, 2, 1, 1, True),           # <10, 13>: the smallest grid
         (2, 41, 9, 33, 2, True),         # <12, 16>: W > 40, odd D
         (2, 48, 48, 64, 1, False),       # <12, 16>
         (256, 3, 2, 64, 2, True)]        # <12, 16>: N at the limit
GENERIC = [(3, 5, 7, 65, 2, True),        # D > 64
           (2, 49, 3, 8, 1, False),       # W > 48
           (300, 5, 7, 50, 2, True)]      # 256 < N < 512, both directions
BWD_ONLY_GENERIC = (512, 5, 7, 50, 2, True)     # forward fused (eval), backward generic: N > 256
FWD = EVAL + TRAIN + GENERIC
BWD = TRAIN + GENERIC + [BWD_ONLY_GENERIC]
MISALIGNED_EVAL, MISALIGNED_TRAIN = (513, 40, 40, 52, 4, True), (2, 40, 40, 52, 1, False)      # q (and dq) one half past 16 bytes
ORACLE = [EVAL[0], TRAIN[0], TRAIN[3], GENERIC[0]]          # one case per route against the CPU oracle
CANARY = [(513, 5, 7, 53, 1, True), (3, 5, 7, 53, 3, True), (3, 5, 7, 65, 1, False)]    # odd element counts: eval, train, generic
EMBED = [(512, 5, 7, 50, 2, True), (3, 5, 7, 50, 4, True)]
EMBED_K = 37
EMBED_UNSUPPORTED = (300, 5, 7, 50, 2)
OVERFLOW = (3, 5, 7, 50, 4, True)


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def fwd_cells():
    return {fwd_route(*s[:5]) for s in FWD}


def bwd_cells():
    return {bwd_route(*s[:5]) for s in BWD}


def width_cells():
    """The staging widths the table's fused shapes run, aligned and with q one half off."""
    c = {stage_width(s[1], s[2], s[3]) for s in EVAL + TRAIN}
    return c | {stage_width(s[1], s[2], s[3], q=2) for s in (MISALIGNED_EVAL, MISALIGNED_TRAIN)}


# ----------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------
def seed(shape):
    return 4201 + sum(int(v) * p for v, p in zip(shape, (1, 7, 61, 523, 4099, 32771)))


_inputs = {}


def inputs(shape):
    """bilinear_grid_model.dense_inputs with q, a rounded to half first; bias, dbias0 ~ N(0, 1) or None.  Shared, read-only."""
    if shape not in _inputs:
        N, W1, W2, D, M, bias_term = shape
        r = np.random.default_rng(seed(shape))
        q, a, W, dT = gm.dense_inputs(r, N, W1, W2, D, M)
        c = dict(qh=q.astype(np.float16), ah=a.astype(np.float16), W=W, dT=dT, bias=None, dbias0=None)
        if bias_term:
            c["bias"] = r.standard_normal((M, W1, W2)).astype(np.float32)
            c["dbias0"] = r.standard_normal((M, W1, W2)).astype(np.float32)
        c["q"], c["a"] = c["qh"].astype(np.float32), c["ah"].astype(np.float32)
        for v in c.values():
            if v is not None:
                v.setflags(write=False)
        _inputs[shape] = c
    return _inputs[shape]


def embed_inputs(shape, K=EMBED_K):
    """A half table (K, D), ids for q and a that include -3, K and K + 5 (clamped by the layer), an Embed bias."""
    N, W1, W2, D, M, _ = shape
    r = np.random.default_rng(seed(shape) + 1)
    table = (r.standard_normal((K, D)) * 0.4).astype(np.float16)
    iq = r.integers(0, K, (N, W1)).astype(np.float32)
    ia = r.integers(0, K, (N, W2)).astype(np.float32)
    iq[0, 0], iq[-1, -1], ia[0, 1], ia[-1, 0] = -3.0, K + 5.0, float(K), -1.0
    ebias = r.standard_normal(D).astype(np.float32)
    return table, iq, ia, ebias


def clamp_ids(ix, K):
    return np.clip(ix.astype(np.int64), 0, K - 1)
