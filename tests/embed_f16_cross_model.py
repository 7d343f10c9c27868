"""mms_embed_simcross_forward_f16 (csrc/simcross_cross_f16.hip: the GATHER instantiations of csrc/cross_grid.h, with the Embed gather of csrc/cross_gather.h): the host routing restated in
Python, the table of cases the GPU test runs, their data and their references.  index_q (N, W1), index_a (N, W2) word ids as floats, table
(K, D) halves, embed_bias (D) fp32 or None; top (N, 1, W1, W2), norm0 (N, W1), norm1 (N, W2) fp32.

Routing, one function per host decision:
  refusal        mms_abi.hip: embed_simcross_refusal -- a dist_mode other than 0 / 1 UNSUPPORTED (before the sizes, as the _f32 twin); bad sizes,
                 K <= 0, K D > 2^31 - 1 INVALID_ARG.  W1 == W2 == 1 is served.
  fwd_tile       cross_fwd_tile: the function mms_simcross_forward_f16 goes through -- cross_grid_model.fwd_tile, not restated twice
  fwd_image_ok   cross_fwd_image_ok<_Float16, GATHER = true> (cross_grid_model.fwd_image_ok): whole 8-row tiles of at most 5, N >= 1024, D == 50,
                 two images in 64 KB and the table 4-byte aligned (GridStorage<_Float16>::kGatherAlign) -- the image kernel gathers in half2, and a
                 row of 50 halves = 100 bytes keeps 4-byte alignment and no more
  fwd_route      the image kernel <W1 / 8, W2 / 8> if fwd_image_ok, else the generic kernel <rj, rk>
  launches       cross_forward: dist_mode 1 the forward alone; dist_mode 0 row_norm_kernel<_Float16> twice, then the forward

What the call is held to (tests/test_gpu_embed_simcross_f16.py):
  Euclid: top is the CPU oracle's on the fp32 rows bias + widen(table)[clamped ids], bit for bit.
  both modes: top (cosine: and the norms) are mms_embed_simcross_forward_f32's on the widened table bit for bit, and without a bias
      mms_simcross_forward_f16's on the gathered half rows.
  cosine, exact-sum probe table (cosine_model.probe_inputs: small integers at one power of two, exact as halves; the bias small integers at
      the same power): every sum is exact in any order, so top and the norms are the oracle's bits.
  cosine, dense: top and the norms within f16_cross_model's existing fp64 bar dense_bar(e_o), e_o the oracle's own error on the same rows.

CPU only; tests/test_embed_f16_cross_model.py proves this module.
"""
import numpy as np

import cosine_model as cm
import cross_grid_model as gm
import f16_cross_model as xm
from cross_grid_model import fwd_tile            # noqa: F401 (the same host function: cross_fwd_tile)

OK, INVALID_ARG, UNSUPPORTED = xm.OK, xm.INVALID_ARG, xm.UNSUPPORTED
IMAGE_D = xm.IMAGE_D
LDS_BYTES = xm.LDS_BYTES


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def refusal(mode, N, W1, W2, D, K):
    """mms_abi.hip: embed_simcross_refusal, up to the pointer checks."""
    lim = 0x7fffffff
    if mode not in (0, 1):
        return UNSUPPORTED
    if N < 0 or W1 <= 0 or W2 <= 0 or D <= 0:
        return INVALID_ARG
    if N * W1 * D > lim or N * W2 * D > lim or N * W1 * W2 > lim:
        return INVALID_ARG
    if K <= 0 or K * D > lim:
        return INVALID_ARG
    return OK


def fwd_image_ok(N, W1, W2, D, table=0):
    """cross_fwd_image_ok<_Float16, GATHER = true>: q == a == the table; table is the table's address."""
    return gm.fwd_image_ok(N, W1, W2, D, table, table, need=gm.GATHER_ALIGN["_Float16"])


def fwd_route(N, W1, W2, D, table=0):
    if fwd_image_ok(N, W1, W2, D, table):
        return ("image", W1 // 8, W2 // 8)
    return ("generic",) + fwd_tile(N, W1, W2)[:2]


def launches(mode, N, W1, W2, D, table=0):
    """The kernels of one accepted call, in order."""
    fwd = fwd_route(N, W1, W2, D, table) + (mode,)
    return (("norm",), ("norm",), fwd) if mode == 0 else (fwd,)


# ----------------------------------------------------------------------------------------------------------------------
# the cases: (N, W1, W2, D), K, off = halves between a 16-byte boundary and the table
# ----------------------------------------------------------------------------------------------------------------------
K_MAIN = 97
CASES = [((3, 5, 7, 33), K_MAIN, 0),          # generic <1, 1>: ragged tile, ragged 32-wide chunk (32 + 1)
         ((3, 5, 7, 33), 1, 0),               # K = 1: every id clamps to row 0
         ((2, 1, 1, 1), K_MAIN, 0),           # W1 == W2 == 1 on the word-grid kernels, D = 1
         ((2, 1, 9, 64), K_MAIN, 0),          # generic <1, 1>, two k tiles (one ragged), two full chunks
         ((4, 40, 40, 50), K_MAIN, 0),        # small N: the register tile shrinks to <1, 1>, 5 x 5 tiles per pair
         ((1024, 40, 40, 48), K_MAIN, 0),     # generic <5, 5>: D != 50 keeps it off the image
         ((1024, 8, 16, 50), K_MAIN, 0),      # image <1, 2>, table 16-byte aligned
         ((1024, 40, 40, 50), K_MAIN, 0),     # image <5, 5>, table 16-byte aligned
         ((1024, 8, 16, 50), K_MAIN, 1),      # the same two one half further: rows only 2-byte aligned, generic <1, 2> ...
         ((1024, 40, 40, 50), K_MAIN, 1),     # ... and generic <5, 5>, the image kernel's bits
         ((1024, 8, 16, 50), K_MAIN, 2)]      # 4-byte but not 16-byte aligned: exactly the image kernel's precondition
EXPECTED_ROUTE = [("generic", 1, 1), ("generic", 1, 1), ("generic", 1, 1), ("generic", 1, 1), ("generic", 1, 1), ("generic", 5, 5),
                  ("image", 1, 2), ("image", 5, 5), ("generic", 1, 2), ("generic", 5, 5), ("image", 1, 2)]
GRAPH_CASE = ((1024, 8, 16, 50), K_MAIN, 0)
REFUSED_SHAPE, REFUSED_K = (4, 5, 7, 50), K_MAIN


def case_id(c):
    shape, K, off = c
    return "%s-K%d-off%d" % (xm.shape_id(shape), K, off)


def route_of(c):
    shape, K, off = c
    return fwd_route(*shape, table=2 * off)


# ----------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------
def clamp_ids(ids, K):
    """gather_id (cross_gather.h): (int) truncates toward zero, then the clamp to [0, K - 1]."""
    return np.clip(np.trunc(ids.astype(np.float64)).astype(np.int64), 0, K - 1)


def word_ids(shape, K):
    """(index_q (N, W1), index_a (N, W2)) float32.  Pair 0 holds -3.0 and K + 5.0 in its first rows and 2.7 in its last ones, pair 1 the
    same on the other side where there is a middle pair; then ids repeat within every pair of more than two rows (q row 1 is q row 0, a row 1
    is a row 0, where the side has two rows); every row of the LAST pair is table row min(2, K - 1), named 2.7 on the q side and 2.0 on the a
    side -- for W1 == W2 == 1 that is the pair whose two ids repeat."""
    N, W1, W2, D = shape
    r = np.random.default_rng(3301 + cm.shape_seed(shape) + K)
    iq, ia = r.integers(0, K, (N, W1)).astype(np.float32), r.integers(0, K, (N, W2)).astype(np.float32)
    iq[0, W1 - 1], ia[0, W2 - 1] = 2.7, 2.7
    iq[0, 0], ia[0, 0] = -3.0, K + 5.0
    if N > 2:
        iq[1, 0], ia[1, 0] = K + 5.0, -3.0
    if W1 > 1:
        iq[:, 1] = iq[:, 0]
    if W2 > 1:
        ia[:, 1] = ia[:, 0]
    iq[N - 1], ia[N - 1] = 2.7, 2.0
    return iq, ia


def dense_table(shape, K):
    """GloVe-like rows N(0, 0.4^2) as halves, the bias N(0, 0.1^2) fp32."""
    D = shape[3]
    r = np.random.default_rng(4401 + cm.shape_seed(shape) + K)
    return (r.standard_normal((K, D)) * 0.4).astype(np.float16), (r.standard_normal(D) * 0.1).astype(np.float32)


def probe_table(shape, K):
    """cosine_model.probe_inputs' exact-sum rows as a (K, D) table, rounded to half (exactly: integers of magnitude <= 4 at one power of two), and a bias
    of integers in [-2, 2] at the same power: bias + table stays an integer of magnitude <= 6 there, every product and every sum over
    D <= 64 of them exact in fp32."""
    D = shape[3]
    r = np.random.default_rng(5501 + cm.shape_seed(shape) + K)
    p = cm.probe_inputs(r, 1, K, 1, D)
    t32 = p["q"][0]
    th = t32.astype(np.float16)
    assert (th.astype(np.float32) == t32).all(), "the probe table is not exact in half"
    bias = np.ldexp(r.integers(-2, 3, D).astype(np.float64), p["eq"]).astype(np.float32)
    return th, bias


def gathered_rows(table_h, bias, iq, ia):
    """The fp32 rows the call scores: bias[d] + widen(table[id][d]), one fp32 add, or the widened half alone."""
    K = table_h.shape[0]
    t32 = table_h.astype(np.float32)
    q, a = t32[clamp_ids(iq, K)], t32[clamp_ids(ia, K)]
    if bias is not None:
        q, a = (bias[None, None, :] + q).astype(np.float32), (bias[None, None, :] + a).astype(np.float32)
    return q, a


# ----------------------------------------------------------------------------------------------------------------------
# references: computed once per (shape, K, kind, bias, mode) -- the placement of the table does not enter -- and shared read-only
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def inputs(shape, K, kind):
    """kind "dense" or "probe": dict(table (K, D) half, bias (D) fp32, iq, ia)."""
    key = ("in", kind, K) + tuple(shape)
    if key not in _cases:
        th, bias = (dense_table if kind == "dense" else probe_table)(shape, K)
        iq, ia = word_ids(shape, K)
        _cases[key] = cm._freeze(dict(table=th, bias=bias, iq=iq, ia=ia))
    return _cases[key]


def reference(oracle, mode, shape, K, kind, with_bias):
    """f16_cross_model.forward_reference on the gathered fp32 rows: the oracle's top (cosine: n0, n1, the fp64 values with their scales and the
    oracle's own errors e_o), with the inputs of the case alongside."""
    key = ("ref", mode, kind, K, bool(with_bias)) + tuple(shape)
    if key not in _cases:
        i = inputs(shape, K, kind)
        q, a = gathered_rows(i["table"], i["bias"] if with_bias else None, i["iq"], i["ia"])
        c = xm.forward_reference(oracle, mode, q, a)
        c.update(table=i["table"], bias=i["bias"] if with_bias else None, iq=i["iq"], ia=i["ia"])
        _cases[key] = cm._freeze(c)
    return _cases[key]
