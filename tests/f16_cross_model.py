"""The fp16-storage word-grid family (the _Float16 instantiations of csrc/cross_grid.h, entered through csrc/simcross_cross_f16.hip behind
mms_simcross_forward_f16, mms_simcross_backward_f16 and mms_simcross_forward_backward_f16): the host routing, the shapes that reach every
kernel instantiation, the references and the bars.  q (N, W1, D), a (N, W2, D), dq, da halves; top, top_diff (N, 1, W1, W2), norm0 (N, W1),
norm1 (N, W2) fp32.

Routing, one function per host decision; the launch plan is the fp32 call's (one template for both storages), so its restatement is
tests/cross_grid_model.py's, held to the source's literals by tests/test_cross_grid_model.py, and imported here:
  refusal        mms_abi.hip: grid_f16_refusal -- bad sizes INVALID_ARG, dist_mode 2 and W1 == W2 == 1 UNSUPPORTED
  fwd_tile       cross_grid_model.fwd_tile (cross_fwd_tile)
  fwd_image_ok   cross_grid_model.fwd_image_ok (cross_fwd_image_ok) with q and a 16-byte aligned
  fwd_route      the image kernel <W1 / 8, W2 / 8> if fwd_image_ok, else the generic kernel <rj, rk>; either for MODE 0 and 1
  bwd_tiled_lds  cross_grid_model.bwd_tiled_lds (cross_bwd_tiled_lds): bytes of the coefficient tables and the staged chunk
  bwd_route      cross_backward<_Float16> -- no lane kernel for halves: tiled <MODE, EXACT> while cross_grid_model.bwd_tiled says so, split
                 when N nchunks < 1024; else plain <MODE>
Every instantiation is reachable: FWD_REACHABLE is 25 generic and 25 image tiles for each mode, BWD_REACHABLE the tiled kernel's three
arithmetics (cosine, Euclid reference rounding, Euclid fp32) split and unsplit and the two plain kernels.  UNREACHABLE is empty
(cross_bwd_tiled_kernel<_Float16, 0, false> is never instantiated: cosine has one arithmetic).

What the kernels are held to:
  Euclid forward: top is the fp32 oracle's on the widened inputs bit for bit, and the fp32 call's.
  Euclid backward, MMS_EUCLID_BWD_REFERENCE: dq / da are oracle_grad.astype(float16) as uint16.
  Euclid backward, default mode (fp32 term arithmetic), two brackets, both asserted:
    (a) the bar tests/test_gpu_parity.py holds the fp32 word-grid backward to in that mode, _assert_grad -> util.assert_close:
        |got - oracle| <= TOL max(1, max |oracle|), TOL = 1e-5, per array.  As a half bracket: centre the oracle's fp32 gradient,
        scale PARITY_SCALE = max(1, max |oracle gradient|) for every element, b = TOL.
        This bracket CANNOT pin 99 % of any array: an element v in [2^e, 2^(e+1)) has halves 2^(e-10) apart and the bracket is
        2 TOL S >= 2e-5 2^e wide (S >= |v|), so a tie falls inside it with probability >= 2e-5 x 2^10 = 2 %; parity_pinned_ceiling
        is that arithmetic and tests/test_f16_cross_model.py measures 7-45 % on the table's cases (top_diff spans 2^20).  The pinned condition is
        therefore carried by
    (b) the half bracket around the fp64 gradient from the stored fp32 top (euclid_grad_ref), scale sum |tt| over the element's walk,
        b = dense_bar(e_o) + FP32_TERM_BAR: e_o the fp32 oracle's own error in that scale (it covers the roundings of c, q - a, the
        division and the ordered sum, which the kernel shares), FP32_TERM_BAR = 4 x 2^-24 the mode's contract (include/mms.h: each
        term at most 2 ulp = 2 x 2^-23 of its value from the reference's).  At least PINNED_MIN of every case's finite elements.
  cosine, exact-sum probes (cosine_model.probe_inputs): top, norm0, norm1 the oracle's bits and the fp32 call's.
  cosine, dense: top and the norms within dense_bar(e_o) of fp64; gradients in the half bracket around cosine_grad_ref from the stored
      top and norms, b = dense_bar(e_o), scale the sum of |t1| + |t2| over the walk; at least PINNED_MIN pinned.
The bracket cases use `aligned_inputs`: the rows of a pair's q scatter a little around one vector and those of a around another, and
top_diff is positive, so the W terms of a gradient element mostly share a sign -- sum |terms| stays near |sum| and b sum |terms| far
below a half's spacing; GloVe-like rows with a signed top_diff cancel by sqrt(W) and pin only 93-97 %.

CPU only; tests/test_f16_cross_model.py proves this module, tests/test_gpu_f16_cross.py uses it.
"""
import numpy as np

import cosine_model as cm
import cross_grid_model as gm
from cross_grid_model import bwd_tiled_lds, fwd_image_ok, fwd_tile            # noqa: F401 (the same host functions: cross_grid.h)
from f16_rows_model import PINNED_MIN, check_bracket, half_bracket, in_bracket, pinned_share, finite_error  # noqa: F401 (re-exported)
from util import TOL

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2          # include/mms.h
FP32_TERM_BAR = 4.0 * cm.U24                    # 2 ulp of a term = 2 x 2^-23 of its value
IMAGE_D, LDS_BYTES, BWD_DC = gm.IMAGE_D, gm.LDS_BYTES, gm.BWD_DC


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def refusal(mode, N, W1, W2, D):
    """mms_abi.hip: dims_ok, then grid_f16_refusal."""
    lim = 0x7fffffff
    if mode < 0 or mode > 2 or N < 0 or W1 <= 0 or W2 <= 0 or D <= 0:
        return INVALID_ARG
    if N * W1 * D > lim or N * W2 * D > lim or N * W1 * W2 > lim:
        return INVALID_ARG
    if mode == 2 or (W1 == 1 and W2 == 1):
        return UNSUPPORTED
    return OK


def fwd_route(N, W1, W2, D, q=0, a=0):
    if fwd_image_ok(N, W1, W2, D, q, a):
        return ("image", W1 // 8, W2 // 8)
    return ("generic",) + fwd_tile(N, W1, W2)[:2]


def bwd_route(mode, exact, N, W1, W2, D):
    """cross_backward<_Float16>: ("tiled", mode, exact, split) or ("plain", mode); cosine's tiled instance is <0, true>."""
    tiled = gm.bwd_tiled(mode, N, W1, W2, D)
    if tiled:
        return ("tiled", mode, True if mode == 0 else bool(exact), 1 if tiled == "split" else 0)
    return ("plain", mode)


FWD_REACHABLE = {(kind, j, k, m) for kind in ("generic", "image") for j in range(1, 6) for k in range(1, 6) for m in (0, 1)}
BWD_REACHABLE = ({("tiled", m, e, s) for (m, e) in ((0, True), (1, True), (1, False)) for s in (0, 1)} | {("plain", 0), ("plain", 1)})
UNREACHABLE = set()

# ----------------------------------------------------------------------------------------------------------------------
# the shapes (N, W1, W2, D)
# ----------------------------------------------------------------------------------------------------------------------
NAMED_FWD = [(3, 5, 7, 50),         # ragged single tile, RJ = RK = 1, 100-byte rows
             (2, 9, 17, 33),        # several ragged tiles, odd D, chunk boundary at 32 + 1, rows only 2-byte aligned
             (1024, 40, 40, 8),     # RJ = RK = 5 on the generic staging
             (1024, 40, 24, 34),    # RJ = 5, RK = 3: both odd, the accq and accs paths of CrossAcc
             (1024, 24, 40, 50),    # the pair-image kernel
             (1025, 8, 8, 50)]      # the pair-image kernel, last workgroup with one valid wave
MISALIGNED = (1024, 24, 40, 50)     # q one half past a 16-byte boundary: generic <3, 5>, the image kernel's bits
# every generic <rj, rk>: N = 1024 so that cap 5 holds; ragged widths inside (8 (r - 1), 8 r]; D away from 50, odd and even
GENERIC_TILES = [(1024, 8 * rj - (rj + rk) % 4, 8 * rk - (2 * rj + rk) % 5, (3, 8, 33, 34)[(rj + 2 * rk) % 4]) for rj in range(1, 6) for rk in range(1, 6)]
IMAGE_TILES = [(1024, 8 * j, 8 * k, IMAGE_D) for j in range(1, 6) for k in range(1, 6)]
FWD = list(dict.fromkeys(NAMED_FWD + GENERIC_TILES + IMAGE_TILES))

BWD = [(3, 5, 7, 50),               # tiled, split; one d chunk of 32 and one of 18; 100-byte rows: 4- and 8-byte aligned stores alternate
       (2, 9, 17, 33),              # tiled, split; a chunk of ONE d; rows only 2-byte aligned: every packed store falls back on odd rows
       (70, 40, 40, 50),            # tiled, split (70 x 2 chunks < 1024): the 40 x 40 tables of network_v4
       (512, 16, 24, 50),           # tiled, NOT split: N nchunks == 1024
       (2, 12, 20, 70),             # tiled, split, three chunks, ragged last one (6)
       (2, 60, 60, 16)]             # plain: 60 x 60 tables exceed 64 KB in both modes
EDGE = (10, 5, 7, 50)


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def fwd_cells():
    c = {fwd_route(*s) + (m,) for s in FWD for m in (0, 1)}
    return c | {fwd_route(*MISALIGNED, q=2) + (m,) for m in (0, 1)}


def bwd_cells():
    return {bwd_route(m, e, *s) for s in BWD for (m, e) in ((0, True), (1, True), (1, False))}


def parity_pinned_ceiling():
    """The largest share bracket (a) can pin: a tie every 2^(e-10), a bracket at least 2 TOL 2^e wide."""
    return 1.0 - 2 * TOL * 2.0 ** 10


# ----------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------
def pair_exponents(N):
    return np.rint(np.linspace(-10, 10, N)).astype(np.int32) if N > 1 else np.zeros(1, np.int32)


def dense_inputs(shape):
    """GloVe-like rows rounded to half; top_diff ~ N(0, 1) 2^s_n, s_n spread over -10 .. 10 across the pairs.  N >= 2: row 0 of a of
    pair 1 is row 0 of q (Euclid: T = 1, the divisor 1e-9)."""
    from util import qa
    N, W1, W2, D = shape
    r = np.random.default_rng(1701 + cm.shape_seed(shape))
    q, a = qa(r, N, W1, W2, D)
    qh, ah = q.astype(np.float16), a.astype(np.float16)
    if N >= 2:
        ah[1, 0] = qh[1, 0]
    dT = np.ldexp(r.standard_normal((N, 1, W1, W2)), pair_exponents(N).reshape(N, 1, 1, 1)).astype(np.float32)
    return qh, ah, dT


def aligned_inputs(shape):
    """The bracket cases: q rows of pair n = c_n + 0.05 noise, a rows = c'_n + 0.05 noise (c, c' GloVe-like, c' made orthogonal to c), as halves;
    top_diff = (0.5 + U(0, 1)) 2^s_n > 0 with s_n spread over -10 .. 10 across the pairs."""
    N, W1, W2, D = shape
    r = np.random.default_rng(2701 + cm.shape_seed(shape))
    c, c2 = r.standard_normal((2, N, 1, D)) * 0.4
    if D > 1:
        c2 = c2 - c * ((c2 * c).sum(-1, keepdims=True) / (c * c).sum(-1, keepdims=True))      # c' orthogonal to c: the cosine's T term stays small
    qh = (c + 0.05 * r.standard_normal((N, W1, D))).astype(np.float16)
    ah = (c2 + 0.05 * r.standard_normal((N, W2, D))).astype(np.float16)
    dT = np.ldexp(0.5 + r.uniform(size=(N, 1, W1, W2)), pair_exponents(N).reshape(N, 1, 1, 1)).astype(np.float32)
    return qh, ah, dT


def edge_inputs(cosine):
    """(qh, ah, dT, names) at EDGE: one edge per pair; top_diff = +-{1, 1.25, 1.5} 2^s_n, s_n spread over -10 .. 10."""
    N, W1, W2, D = EDGE
    qh, ah, _ = dense_inputs(EDGE)
    qh, ah = qh.copy(), ah.copy()
    ah[1, 0] = np.random.default_rng(5).standard_normal(D).astype(np.float16)        # undo dense_inputs' equal rows: pair 7 has them
    r = np.random.default_rng(1701 + int(cosine))
    dT = np.ldexp(r.choice(np.array([1.0, -1.5, 1.25]), (N, 1, W1, W2)), pair_exponents(N).reshape(N, 1, 1, 1)).astype(np.float32)
    names = ["clean"] * N
    qh[0, 1, 5] = np.inf
    names[0] = "q row 1 holds Inf"
    ah[1, 2, D - 1] = np.nan
    names[1] = "a row 2 holds NaN"
    qh[2, :, 0::2], qh[2, :, 1::2] = 65504.0, -65504.0
    ah[2] = qh[2, 0]
    ah[2, :, 3] = -65472.0                    # one half above -65504: distance 32 from every q row
    dT[2] = 1e8 if not cosine else dT[2]
    names[2] = "65504-magnitude rows" + ("" if cosine else ", a short distance and top_diff 1e8: the gradient overflows half")
    sub = lambda W: (np.ldexp(r.integers(1, 1024, (W, D)).astype(np.float64), -24) * r.choice(np.array([-1.0, 1.0]), (W, D))).astype(np.float16)
    qh[3], ah[3] = sub(W1), sub(W2)
    names[3] = "subnormal halves"
    if cosine:
        ah[4] = 65504.0 * r.choice(np.array([-1.0, 1.0]), (W2, D))
        qh[4] = sub(W1)
        dT[4] = np.abs(dT[4]) * 2.0 ** 12
        names[4] = "65504-magnitude a rows against subnormal q rows: dq overflows half"
    else:
        dT[4] = 0.0
        names[4] = "top_diff == 0"
    qh[5, 2, D // 2], ah[5, 3, D // 2] = np.inf, np.inf
    names[5] = "Inf in both operands at one coordinate"
    qh[6, 0] = 0
    names[6] = "zero q row"
    ah[7, :min(W1, W2)] = qh[7, :min(W1, W2)]
    names[7] = "a rows == q rows: T = 1 on the diagonal"
    ah[8, 4] = 0
    qh[8, 3] = 0
    names[8] = "zero a row and zero q row"
    return qh, ah, dT, names


# ----------------------------------------------------------------------------------------------------------------------
# references: computed once per case, shared read-only
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def euclid_grad_ref(c, top32):
    """((dq64, scale), (da64, scale)) in fp64 from the widened inputs and the fp32 scores the backward is given: tt = g T^3 (q - a) /
    (T - 1 + 1e-9) term by term (no rearrangement: the T = 1 terms are 1e9 times the others), scale = sum |tt| over the walk."""
    q, a = c["qh"].astype(np.float64), c["ah"].astype(np.float64)
    T, g = np.asarray(top32, np.float64)[:, 0], np.asarray(c["dT"], np.float64)[:, 0]
    N, W1, D = q.shape
    W2 = a.shape[1]
    dq, mq, da, ma = np.zeros((N, W1, D)), np.zeros((N, W1, D)), np.zeros((N, W2, D)), np.zeros((N, W2, D))
    step = max(1, (1 << 22) // (W1 * W2 * D))
    with np.errstate(all="ignore"):
        coef = g * T * T * T / (T - 1.0 + 1e-9)
        for n0 in range(0, N, step):
            s = slice(n0, n0 + step)
            tt = coef[s, :, :, None] * (q[s, :, None, :] - a[s, None, :, :])
            dq[s], mq[s], da[s], ma[s] = tt.sum(2), np.abs(tt).sum(2), -tt.sum(1), np.abs(tt).sum(1)
    return (dq, mq), (da, ma)


def cosine_grad_ref(c, top32, n032, n132):
    """cosine_model.grad_ref on the widened inputs from the fp32 forward."""
    with np.errstate(all="ignore"):
        return cm.grad_ref(c["qh"].astype(np.float32), c["ah"].astype(np.float32), top32, n032, n132, c["dT"])


def forward_reference(oracle, mode, qh, ah):
    """The fp32 oracle's forward on the widened inputs; cosine: fp64 values, scales and the oracle's own errors e_o."""
    q32, a32 = qh.astype(np.float32), ah.astype(np.float32)
    c = dict(qh=qh, ah=ah, q=q32, a=a32)
    with np.errstate(all="ignore"):
        c["top"], c["n0"], c["n1"] = oracle.simcross_forward(mode, q32, a32)
        if mode == 0:
            top64, n064, n164 = oracle.simcross_forward(0, q32.astype(np.float64), a32.astype(np.float64))
            _, mt = cm.top_ref(q32, a32)
            c["ref"] = dict(top=(top64, mt), n0=(n064, n064), n1=(n164, n164))
            c["e_o"] = {k: finite_error(c[k], *c["ref"][k]) for k in ("top", "n0", "n1")}
    return c


def backward_reference(oracle, mode, c, dT):
    """Adds to forward_reference: the fp32 oracle's backward from its own forward, the fp64 gradient from that same forward with its
    scales, and e_o of the gradients."""
    f64 = lambda x: np.asarray(x).astype(np.float64)
    c = dict(c, dT=dT)
    kw = dict(norm0=c["n0"], norm1=c["n1"]) if mode == 0 else {}
    with np.errstate(all="ignore"):
        c["dq"], c["da"], _, _ = oracle.simcross_backward(mode, c["q"], c["a"], c["top"], dT, **kw)
        kw64 = {k: f64(v) for k, v in kw.items()}
        dq64, da64, _, _ = oracle.simcross_backward(mode, f64(c["q"]), f64(c["a"]), f64(c["top"]), f64(dT), **kw64)
    rq, ra = euclid_grad_ref(c, c["top"]) if mode == 1 else cosine_grad_ref(c, c["top"], c["n0"], c["n1"])
    for x, y, m in ((rq[0], dq64, rq[1]), (ra[0], da64, ra[1])):          # the vectorised fp64 agrees with the fp64 oracle
        assert finite_error(x, y, m) < 2.0 ** -40
    c["ref"] = dict(c.get("ref", {}), dq=rq, da=ra)
    c["e_o"] = dict(c.get("e_o", {}), dq=finite_error(c["dq"], *rq), da=finite_error(c["da"], *ra))
    return c


def forward_case(oracle, mode, shape):
    """Euclid: dense_inputs; cosine: the exact-sum probe as halves."""
    key = ("fwd", mode) + tuple(shape)
    if key not in _cases:
        if mode == 1:
            qh, ah, _ = dense_inputs(shape)
        else:
            p = cm.probe_inputs(np.random.default_rng(1701 + cm.shape_seed(shape)), *shape)
            qh, ah = p["q"].astype(np.float16), p["a"].astype(np.float16)
            assert (qh.astype(np.float32) == p["q"]).all() and (ah.astype(np.float32) == p["a"]).all()
        _cases[key] = cm._freeze(forward_reference(oracle, mode, qh, ah))
    return _cases[key]


def backward_case(oracle, mode, shape, kind):
    """kind "dense" (dense_inputs: the bit-for-bit Euclid cases) or "aligned" (aligned_inputs: the bracket cases)."""
    key = ("bwd", mode, kind) + tuple(shape)
    if key not in _cases:
        qh, ah, dT = (dense_inputs if kind == "dense" else aligned_inputs)(shape)
        _cases[key] = cm._freeze(backward_reference(oracle, mode, forward_reference(oracle, mode, qh, ah), dT))
    return _cases[key]


def edge_case(oracle, mode):
    key = ("edge", mode)
    if key not in _cases:
        qh, ah, dT, names = edge_inputs(mode == 0)
        c = backward_reference(oracle, mode, forward_reference(oracle, mode, qh, ah), dT)
        c["names"] = names
        _cases[key] = cm._freeze(c)
    return _cases[key]


def parity_bracket(c, k):
    """Bracket (a) of the default Euclid backward mode: (ref64, scale, b)."""
    ref = c[k].astype(np.float64)
    fin = np.isfinite(ref)
    s = max(1.0, float(np.abs(ref[fin]).max())) if fin.any() else 1.0
    return ref, np.full(ref.shape, s), TOL


def term_bar(c, k):
    """b of bracket (b)."""
    return cm.dense_bar(c["e_o"][k]) + FP32_TERM_BAR
