"""The word-grid SimCross (dist_mode 0 and 1; csrc/cross_grid.h -- one kernel set and one launch plan for float and half storage --
csrc/simcross_cross.hip with the fp32-only lane kernel, csrc/cross_acc.h): the host routing restated in Python, the shapes that reach every
fp32 kernel instantiation and straddle every routing threshold, the inputs and the references.

Routing, one function per host decision, each a line-for-line restatement:
  fwd_tile       cross_fwd_tile: the register tile (rj, rk) = ceil(W / 8) capped at 5, 4, .. 1 until N tilesJ tilesK >= 1024
  fwd_image_ok   cross_fwd_image_ok: whole 8-row tiles of at most 5, N >= 1024, D == 50, q and a aligned to `need` bytes (16; gathered from a
                 table GridStorage::kGatherAlign: 16 for floats, 4 for halves), two pairs' fp32 images in 64 KB; rows 8 apart fall in different banks
                 at that D (a static_assert there)
  fwd_route      launch_cross_fwd: ("image", W1 / 8, W2 / 8) if fwd_image_ok, else ("fwd", rj, rk).  MODE 0 and 1 alike.
  bwd_lane_lds   cross_bwd_lane_lds        bwd_tiled_lds  cross_bwd_tiled_lds        bwd_lane_ok  cross_bwd_lane_ok
  bwd_tiled      cross_backward: the tiled kernel ("split" | "unsplit") while its tables fit 64 KB, else None (the plain kernel)
  bwd_route      cross_backward<float>, Euclid: ("lane", W2, exact), ("tiled", exact, "split" | "unsplit") or ("plain",)
tests/f16_cross_model.py and tests/embed_f16_cross_model.py import fwd_tile, fwd_image_ok, bwd_tiled_lds and bwd_tiled from here: the half calls
go through the same host functions.  The named constants are read from the source; the lane kernel's are literals there, and source_lines()
names the lines that hold every decision so that tests/test_cross_grid_model.py can assert they still read as restated here: a retune breaks
the model instead of passing it by.

CPU only; tests/test_cross_grid_model.py proves this module, tests/test_gpu_cross_grid.py uses it.
"""
import os

import numpy as np

from layer_plans import CSRC, constants
from util import TOL, qa

GRID = "cross_grid.h"                           # the kernels and the launch plan of both storages
LANE = "simcross_cross.hip"                     # the fp32-only lane kernel and its route
_K = constants(GRID, ["kBwdDC", "kMaxTile", "kFill", "kImageD", "kLdsBytes"])
BWD_DC = _K["kBwdDC"]
LANE_WIDTHS = (8, 16, 20, 24, 32, 40, 48)       # cross_bwd_lane_ok, MMS_LANE
LANE_MIN_N, LANE_MAX_D = 512, 64                # cross_bwd_lane_ok
LANE_LDS_KB = {True: 16, False: 64}             # cross_bwd_lane_ok: reference rounding, fp32 arithmetic
LDS_BYTES = _K["kLdsBytes"]                     # cross_backward (tiled), cross_fwd_image_ok (two images)
FILL = _K["kFill"]                              # cross_fwd_tile: N tiles >= 1024; cross_fwd_image_ok: N >= 1024; cross_backward: split while N nchunks < 1024
IMAGE_D, IMAGE_MIN_N, MAX_TILE = _K["kImageD"], FILL, _K["kMaxTile"]
RESTATED = dict(kBwdDC=32, kMaxTile=5, kFill=1024, kImageD=50, kLdsBytes=64 * 1024)      # what the shape tables below were chosen for
GATHER_ALIGN = {"float": 16, "_Float16": 4}     # GridStorage<S>::kGatherAlign


def source_lines():
    """{what: (file, regular expression, the text its group must hold, runs of blanks apart)}: the lines of the sources with the decisions
    and literals restated above."""
    return {
        "lane widths": (LANE, r"const bool width = ([^;]+);", " || ".join("W2 == %d" % w for w in LANE_WIDTHS)),
        "lane widths instantiated": (LANE, r"switch \(W2\) \{ ([^}]+) \}", " ".join("MMS_LANE(%d)" % w for w in LANE_WIDTHS)),
        "lane conditions": (LANE, r"return width && ([^;]+);",
                            "D <= %d && N >= %d && cross_bwd_lane_lds(exact, W1, W2) <= (exact ? %d : %d) * 1024"
                            % (LANE_MAX_D, LANE_MIN_N, LANE_LDS_KB[True], LANE_LDS_KB[False])),
        "lane table bytes": (LANE, r"return (\(size_t\)W1 \* W2 \* \(exact [^;]+);",
                             "(size_t)W1 * W2 * (exact ? 8 + 8 + 4 : 8) + (exact ? 0 : (size_t)W2 * 64 * sizeof(float)) + 16"),
        "lane first": (GRID, r"if \((mode == 1 && launch_cross_bwd_lane<S>\([^;]+)\) return;",
                       "mode == 1 && launch_cross_bwd_lane<S>(N, W1, W2, D, q, a, top, top_diff, dq, da, exact, s)"),
        "lane route": (LANE, r"if \((!cross_bwd_lane_ok\([^;]+)\) return false;", "!cross_bwd_lane_ok(exact, N, W1, W2, D)"),
        "lane figures' chunk": (LANE, r"namespace lane_figures \{\s*(constexpr int kBwdDC = \d+;\s*static_assert\([^,]+),",
                                "constexpr int kBwdDC = %d; static_assert(kBwdDC == ::mms::kBwdDC" % BWD_DC),
        "tiled table bytes": (GRID, r"const size_t tables = ([^;]+);", "mode == 1 ? JK * (8 + 8 + 4) : JK * 16"),
        "tiled staging bytes": (GRID, r"return tables \+ ([^;]+);", "(size_t)(W1 + W2) * (kBwdDC + 1) * sizeof(float) + 16"),
        "tiled bytes": (GRID, r"const size_t lds = ([^;]+);", "cross_bwd_tiled_lds(mode, W1, W2)"),
        "tiled condition": (GRID, r"\n  if \((lds <= [^{]+)\) \{", "lds <= kLdsBytes && 2LL * N * nchunks <= 0x7fffffffLL"),
        "split": (GRID, r"const int split = ([^;]+);", "((long long)N * nchunks < kFill) ? 1 : 0"),
        "chunks": (GRID, r"const int nchunks = ([^;]+);", "(D + kBwdDC - 1) / kBwdDC"),
        "tile cap": (GRID, r"for \(int cap = (\w+); cap >= 1; --cap\)", "kMaxTile"),
        "tile fill": (GRID, r"if \(\(long long\)N \* t\.tilesJ \* t\.tilesK >= (\w+)\) break;", "kFill"),
        "image conditions": (GRID, r"return (W1 % 8 == 0 [^;]+);",
                             "W1 % 8 == 0 && W2 % 8 == 0 && W1 / 8 <= kMaxTile && W2 / 8 <= kMaxTile && N >= kFill && D == kImageD && "
                             "(reinterpret_cast<uintptr_t>(q) & need) == 0 && (reinterpret_cast<uintptr_t>(a) & need) == 0 && 2 * img <= kLdsBytes"),
        "image bytes": (GRID, r"inline bool cross_fwd_image_ok\([^{]+\{[^}]*?const size_t img = ([^;]+);", "(size_t)(W1 + W2) * D * sizeof(float)"),
        "image alignment": (GRID, r"const uintptr_t need = ([^;]+);", "(GATHER ? GridStorage<S>::kGatherAlign : 16) - 1"),
        "image banks": (GRID, r"static_assert\((kImageD[^,]+),", "kImageD % 2 == 0 && kImageD % 16 != 0"),
        "gather alignment, floats": (GRID, r"struct GridStorage<float> \{[^}]*?kGatherAlign = (\d+),", "%d" % GATHER_ALIGN["float"]),
        "gather alignment, halves": (GRID, r"struct GridStorage<_Float16> \{[^}]*?kGatherAlign = (\d+),", "%d" % GATHER_ALIGN["_Float16"]),
        "tile table row": (GRID, r"#define MMS_TILES5\(K, S, J, \.\.\.\) \\\n\s*\{([^}]+)\}", ", ".join("K<S, J, %d, __VA_ARGS__>" % k for k in range(1, MAX_TILE + 1))),
        "tile table": (GRID, r"#define MMS_TILES5X5\(K, S, \.\.\.\)[ \\\n]*\{([^}]+)\}",
                       ", ".join("MMS_TILES5(K, S, %d, __VA_ARGS__)" % j for j in range(1, MAX_TILE + 1))),
        "image kernels": (GRID, r"image\[kMaxTile\]\[kMaxTile\] =\s*(MMS_TILES5X5\([^;]+);", "MMS_TILES5X5(cross_fwd_image_kernel, S, MODE, kImageD, GATHER)"),
        "generic kernels": (GRID, r"generic\[kMaxTile\]\[kMaxTile\] =\s*(MMS_TILES5X5\([^;]+);", "MMS_TILES5X5(cross_fwd_kernel, S, MODE, GATHER)"),
        "image kernel chosen": (GRID, r"hipLaunchKernelGGL\((image\[[^,]+),", "image[W1 / 8 - 1][W2 / 8 - 1]"),
        "generic kernel chosen": (GRID, r"hipLaunchKernelGGL\((generic\[[^,]+),", "generic[t.rj - 1][t.rk - 1]"),
    }


def source_text(source=GRID):
    return open(os.path.join(CSRC, source)).read()


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def fwd_tile(N, W1, W2):
    """cross_fwd_tile: (rj, rk, tilesJ, tilesK)."""
    for cap in range(MAX_TILE, 0, -1):
        rj, rk = min((W1 + 7) // 8, cap), min((W2 + 7) // 8, cap)
        tj, tk = (W1 + 8 * rj - 1) // (8 * rj), (W2 + 8 * rk - 1) // (8 * rk)
        if N * tj * tk >= FILL:
            break
    return rj, rk, tj, tk


def gcd64(d):
    g = 64
    while d % g:
        g >>= 1
    return g


def fwd_image_ok(N, W1, W2, D, q=0, a=0, need=16):
    """cross_fwd_image_ok; q, a are addresses, need the alignment asked of them: 16, or gathered GATHER_ALIGN of the storage."""
    img = (W1 + W2) * D * 4
    return (W1 % 8 == 0 and W2 % 8 == 0 and W1 // 8 <= MAX_TILE and W2 // 8 <= MAX_TILE and N >= IMAGE_MIN_N and D == IMAGE_D
            and q % need == 0 and a % need == 0 and 2 * img <= LDS_BYTES)


def fwd_route(N, W1, W2, D, aligned=True):
    """launch_cross_fwd<float>: ("image", J, K) or ("fwd", rj, rk); aligned: q and a both on a 16-byte boundary."""
    if fwd_image_ok(N, W1, W2, D, q=0 if aligned else 4):
        return ("image", W1 // 8, W2 // 8)
    return ("fwd",) + fwd_tile(N, W1, W2)[:2]


def bwd_lane_lds(exact, W1, W2):
    return W1 * W2 * (8 + 8 + 4 if exact else 8) + (0 if exact else W2 * 64 * 4) + 16


def bwd_tiled_lds(mode, W1, W2):
    JK = W1 * W2
    return (JK * (8 + 8 + 4) if mode == 1 else JK * 16) + (W1 + W2) * (BWD_DC + 1) * 4 + 16


def bwd_lane_ok(exact, N, W1, W2, D):
    return W2 in LANE_WIDTHS and D <= LANE_MAX_D and N >= LANE_MIN_N and bwd_lane_lds(exact, W1, W2) <= LANE_LDS_KB[bool(exact)] * 1024


def bwd_tiled(mode, N, W1, W2, D):
    """cross_backward behind the lane kernel: "split" or "unsplit" for the tiled kernel, None for the plain one."""
    nchunks = (D + BWD_DC - 1) // BWD_DC
    if bwd_tiled_lds(mode, W1, W2) <= LDS_BYTES and 2 * N * nchunks <= 0x7fffffff:
        return "split" if N * nchunks < FILL else "unsplit"
    return None


def bwd_route(N, W1, W2, D, exact):
    """cross_backward<float>, mode 1."""
    if bwd_lane_ok(exact, N, W1, W2, D):
        return ("lane", W2, bool(exact))
    tiled = bwd_tiled(1, N, W1, W2, D)
    return ("tiled", bool(exact), tiled) if tiled else ("plain",)


# ----------------------------------------------------------------------------------------------------------------------
# the shapes (N, W1, W2, D)
# ----------------------------------------------------------------------------------------------------------------------
TILES = [(j, k) for j in range(1, MAX_TILE + 1) for k in range(1, MAX_TILE + 1)]
# every fwd<rj, rk>: N = 1024 keeps cap 5; ragged widths inside (8 (r - 1), 8 r]; D away from 50: a chunk of 3, of 8, 32 + 1 and 32 + 2
GENERIC_TILES = [(1024, 8 * rj - (rj + rk) % 4, 8 * rk - (2 * rj + rk) % 5, (3, 8, 33, 34)[(rj + 2 * rk) % 4]) for rj, rk in TILES]
# every image<j, k>; odd N: the last workgroup's second wave has no pair.  With q and a off a 16-byte boundary: fwd<j, k>
IMAGE_TILES = [(1024 + ((j + k) & 1), 8 * j, 8 * k, IMAGE_D) for j, k in TILES]
FWD_EDGES = {(1023, 16, 24, 50): ("fwd", 2, 2),       # N one below the image: the tile shrinks until N tiles >= 1024
             (1024, 16, 24, 52): ("fwd", 2, 3),       # D next to the image's
             (1024, 48, 8, 50): ("fwd", 5, 1)}        # six 8-row tiles decline the image
FWD = list(dict.fromkeys(GENERIC_TILES + IMAGE_TILES + list(FWD_EDGES)))

L, T, P = "lane", "tiled", ("plain",)
_lane = lambda w: ((L, w, True), (L, w, False))
_tiled = lambda s: ((T, True, s), (T, False, s))
# shape -> (route with reference rounding, route with fp32 arithmetic)
BWD = {
    (512, 3, 16, 50): _lane(16), (513, 9, 16, 7): _lane(16), (512, 25, 16, 64): _lane(16), (512, 1, 16, 50): _lane(16),
    (512, 2, 32, 50): _lane(32), (515, 25, 32, 33): _lane(32),
    (512, 7, 20, 50): _lane(20), (514, 11, 24, 34): _lane(24),
    (512, 20, 40, 50): _lane(40),                                         # 16016 bytes of reference-rounding tables: the last that fit 16 KB
    (512, 21, 40, 50): ((T, True, "unsplit"), (L, 40, False)),
    (512, 17, 48, 50): _lane(48),
    (512, 18, 48, 50): ((T, True, "unsplit"), (L, 48, False)),
    (512, 102, 8, 8): _lane(8),
    (512, 103, 8, 8): ((T, True, "split"), (L, 8, False)),
    (512, 138, 48, 8): (P, (L, 48, False)),                               # 65296 bytes of fp32 tables: the last that fit 64 KB
    (512, 139, 48, 8): (P, P),
    (511, 8, 16, 50): _tiled("split"),                                    # N one below the lane kernel's 512
    (512, 8, 16, 50): _lane(16),
    (512, 8, 16, 64): _lane(16),
    (512, 8, 16, 65): _tiled("unsplit"),                                  # D one above the lane kernel's 64
    (520, 8, 16, 1): _lane(16), (520, 8, 16, 3): _lane(16),               # fewer columns than lanes
    (512, 8, 12, 50): _tiled("unsplit"),                                  # a width that is not instantiated
    (1024, 5, 7, 20): _tiled("unsplit"),
    (40, 9, 7, 900): _tiled("unsplit"),                                   # 29 chunks, the last of 4
    (512, 5, 7, 50): _tiled("unsplit"),                                   # N nchunks == 1024: the first unsplit size
    (511, 5, 7, 50): _tiled("split"),                                     # 1022: the last split size
    (512, 16, 1, 50): _tiled("unsplit"),
}
# (smaller, larger, axis): the larger case is the smaller one extended along `axis`; in reference mode the two sides take different
# kernels and what they share must carry identical words
EDGE_PAIRS = [((511, 5, 7, 50), (512, 5, 7, 50), "N"),          # tiled split | tiled unsplit
              ((511, 8, 16, 50), (512, 8, 16, 50), "N"),        # tiled split | lane
              ((512, 8, 16, 64), (512, 8, 16, 65), "D"),        # lane | tiled unsplit
              ((512, 102, 8, 8), (512, 103, 8, 8), "W1"),       # lane | tiled split
              ((512, 20, 40, 50), (512, 21, 40, 50), "W1"),     # lane | tiled unsplit
              ((512, 17, 48, 50), (512, 18, 48, 50), "W1"),     # lane | tiled unsplit
              ((512, 138, 48, 8), (512, 139, 48, 8), "W1")]     # plain | plain in reference mode; lane | plain in fp32 mode


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def shape_seed(s):
    return sum((i + 1) * int(v) for i, v in enumerate(s))


def one_per_route(exact):
    """The first (hence a small) shape of BWD on each backward route of one arithmetic mode."""
    seen = {}
    for s, routes in BWD.items():
        seen.setdefault(routes[0 if exact else 1], s)
    return sorted(seen.values())


# ----------------------------------------------------------------------------------------------------------------------
# inputs and references: computed once per case, shared read-only
# ----------------------------------------------------------------------------------------------------------------------
def degenerate_pairs(N):
    return sorted({min(1, N - 1), N - 1})


def inputs(shape):
    """GloVe-like rows (util.qa) and top_diff ~ N(0, 1); the last row of a equals the last row of q in pair 1 and in the last pair:
    T = 1 and the divisor 1e-9 in the last output of the last tile."""
    N, W1, W2, D = shape
    r = np.random.default_rng(1701 + shape_seed(shape))
    q, a = qa(r, N, W1, W2, D)
    for n in degenerate_pairs(N):
        a[n, W2 - 1] = q[n, W1 - 1]
    dT = r.standard_normal((N, 1, W1, W2)).astype(np.float32)
    return q, a, dT


def extended(small, large, axis):
    """inputs(small) extended to `large`: more pairs, one more row of q (with top_diff 0: da keeps its terms), or one more column in
    which every row of q and of a holds the same value (q - a = 0 there: top keeps its bits and the other columns their terms)."""
    q, a, dT = inputs(small)
    r = np.random.default_rng(2701 + shape_seed(large))
    N, W1, W2, D = large
    if axis == "N":
        q2, a2 = qa(r, N - small[0], W1, W2, D)
        return np.concatenate([q, q2]), np.concatenate([a, a2]), np.concatenate([dT, r.standard_normal((N - small[0], 1, W1, W2)).astype(np.float32)])
    if axis == "W1":
        q2, _ = qa(r, N, W1 - small[1], W2, D)
        return np.concatenate([q, q2], 1), a, np.concatenate([dT, np.zeros((N, 1, W1 - small[1], W2), np.float32)], 2)
    assert axis == "D" and D == small[3] + 1
    c = (r.standard_normal((N, 1, 1)) * 0.4).astype(np.float32)
    return np.concatenate([q, np.broadcast_to(c, (N, W1, 1))], 2), np.concatenate([a, np.broadcast_to(c, (N, W2, 1))], 2), dT


_cases = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def forward_case(oracle, mode, shape):
    """q, a; top (and n0, n1) of the fp32 oracle; cosine: the fp64 values with their scales and the oracle's own scaled errors."""
    import cosine_model as cm
    key = ("fwd", mode) + tuple(shape)
    if key not in _cases:
        q, a, _ = inputs(shape)
        c = dict(q=q, a=a)
        c["top"], c["n0"], c["n1"] = oracle.simcross_forward(mode, q, a)
        if mode == 0:
            f64 = lambda x: x.astype(np.float64)
            top64, n064, n164 = oracle.simcross_forward(0, f64(q), f64(a))
            _, mt = cm.top_ref(q, a)
            c["ref"] = dict(top=(top64, mt), n0=(n064, n064), n1=(n164, n164))
            c["e_o"] = {k: cm.scaled_error(c[k], *c["ref"][k])[0] for k in ("top", "n0", "n1")}
        _cases[key] = _freeze(c)
    return _cases[key]


def embed_case(oracle, shape, bias):
    """A table of K rows, ids (as floats) with different rows for q and a, the gathered blobs (the oracle's Embed forward) and the
    oracle's Euclid top on them.  The degenerate pairs gather one table row for the last word of both sentences."""
    key = ("embed", bool(bias)) + tuple(shape)
    if key not in _cases:
        N, W1, W2, D = shape
        K = 301
        r = np.random.default_rng(3701 + shape_seed(shape) + int(bias))
        table = (r.standard_normal((K, D)) * 0.4).astype(np.float32)
        b = (r.standard_normal(D) * 0.1).astype(np.float32) if bias else None
        iq = r.integers(0, K, (N, W1)).astype(np.float32)
        ia = r.integers(0, K, (N, W2)).astype(np.float32)
        for n in degenerate_pairs(N):
            ia[n, W2 - 1] = iq[n, W1 - 1]
        c = dict(table=table, bias=b, iq=iq, ia=ia, q=oracle.embed_forward(iq, table, b), a=oracle.embed_forward(ia, table, b))
        c["top"], _, _ = oracle.simcross_forward(1, c["q"], c["a"])
        _cases[key] = _freeze(c)
    return _cases[key]


def term_budget(q, a, top, dT):
    """(mag_q, mag_a): the sum over an element's walk of |tt| = |dT T^3 (q - a) / (T - 1 + 1e-9)| in fp64 -- the scale of the fp32
    arithmetic mode's contract (include/mms.h: every term within 2 ulp of the reference's)."""
    T = np.asarray(top, np.float64)[:, 0]
    N, W1, D = q.shape
    coef = np.abs(np.asarray(dT, np.float64)[:, 0] * T ** 3 / (T - 1 + 1e-9))          # (N, W1, W2)
    mag_q, mag_a = np.empty(q.shape), np.empty(a.shape)
    step = max(1, (1 << 22) // (W1 * a.shape[1] * D))
    for n0 in range(0, N, step):
        s = slice(n0, n0 + step)
        t = coef[s, :, :, None] * np.abs(q[s].astype(np.float64)[:, :, None, :] - a[s].astype(np.float64)[:, None, :, :])
        mag_q[s], mag_a[s] = t.sum(axis=2), t.sum(axis=1)
    return mag_q, mag_a


def assert_fp32_mode(got, ref, mag, north_star=True):
    """The fp32 arithmetic mode's bound on a gradient array: each of an element's terms is within 2 ulp of the reference's, so the
    element is within 4 eps of the sum of the terms' magnitudes, and within the 1e-5 bar against the largest magnitude."""
    eps = np.finfo(np.float32).eps
    assert (np.abs(got - ref) <= 4 * eps * mag + 1e-30).all()
    if north_star:
        np.testing.assert_allclose(got, ref, rtol=0, atol=TOL * max(1.0, np.abs(ref).max()))


def backward_case(oracle, shape, extend=None):
    """inputs(shape), or with extend = (smaller shape, axis) that smaller case extended to `shape`; the oracle's top and its gradients."""
    key = ("bwd",) + tuple(shape) + (extend or ())
    if key not in _cases:
        q, a, dT = inputs(shape) if extend is None else extended(extend[0], shape, extend[1])
        c = dict(q=q, a=a, dT=dT)
        c["top"], _, _ = oracle.simcross_forward(1, q, a)
        c["dq"], c["da"], _, _ = oracle.simcross_backward(1, q, a, c["top"], dT)
        _cases[key] = _freeze(c)
    return _cases[key]
