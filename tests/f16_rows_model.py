"""The fp16-storage sentence-vector family (csrc/simcross_rows_f16.hip: euclid_rows_wave_f16_kernel, euclid_rows_lanechain_f16_kernel,
cosine_rows_wave_f16_kernel behind mms_simcross_{euclid,cosine}_forward[_backward]_f16): the host routing restated in Python, the
shapes that reach every kernel instantiation, the references and the bars.  q, a, dq, da (N, 1, D) halves; top, norms, top_diff fp32.

Routing, one function per host decision (simcross_euclid_rows_f16 / simcross_cosine_rows_f16):
  f16_rows_ok    D % 8 == 0, D <= 2048, q and a 16-byte aligned, dq and da too in the fused call, else MMS_ERR_UNSUPPORTED
  family         Euclid: distance mode tree -> `tree` (euclid_rows_wave_f16_kernel<NIT, 1, B, true>); ordered and D <= 400 (wave_pairs
                 == 2) -> `wave2` (euclid_rows_wave_f16_kernel<NIT, 2, B>); ordered beyond -> `lanechain`; cosine has one family
  nit            half8 loads per operand per lane: ceil(RW D8 / 64), D8 = D / 8, RW = 2 for wave2 and 1 otherwise; the kernel is
                 kernels[bwd][nit - 1] of an MMS_NIT4 table
  PAIRS_PER_WG   pairs per workgroup: the grid is ceil(N / that)
  npad           zero float4 behind a pair's image of squares (wave2 only): 3 ceil(D4 / 3) - D4, D4 = D / 4
wave2 cannot reach NIT 3 or 4 (RW D8 <= 100): UNREACHABLE lists those cells, nothing pretends to test them.

What the kernels are held to:
  Euclid, ordered (wave2, lanechain): the header's contract, no tolerance -- top is the fp32 oracle's on the widened inputs bit for
      bit, dq / da are oracle_grad.astype(float16) as uint16.
  Euclid, tree: top within cosine_model.dense_bar(e_o) of the fp64 oracle, relative (every term of the distance is positive); e_o =
      the ORDERED fp32 oracle's own error against the fp64 oracle on the same widened inputs.  Gradients: the half bracket (below)
      around the fp64 oracle's gradient, scale |ref64| (one product chain, no cancellation), b = dense_bar(e_o of the fp32
      oracle's gradient), both backwards from the same fp32 top.
  cosine, exact-sum probes (cosine_model.probe_inputs: small integers times a power of two, exact as halves): top, norm0, norm1
      the oracle's bits and the fp32 kernel's; a gradient element is ONE (j, k) contribution held to the half bracket with b =
      BAR_GRAD of |t1| + |t2|.  The f16 kernel's roundings: c1 = g / n0 / n1: 2, x other: 1 -> 3 u |t1|; g T: 1, n n: 1, the
      division: 1, x self: 1 -> 4 u |t2|; the subtraction: 1 -> u |t1 - t2|: at most 4 u |t1| + 5 u |t2| <= 5 u (|t1| + |t2|).
  cosine, dense: top and the norms within dense_bar(e_o) of fp64; gradients in the half bracket, b = dense_bar(e_o), scale the
      sum of |t1| + |t2| (cosine_model.grad_ref).
The f16 calls have no backward of their own: a gradient comes from the forward of the same launch.  T (and the norms) are stored
exactly as the backward uses them, so the gradient's fp64 reference is taken from the backward's OWN fp32 inputs, as
cosine_model.grad_ref does: the stored top, norm0, norm1 cast to fp64 (euclid_grad_ref, cosine_grad_ref) -- the forward is held to
fp64 separately.  e_o is the fp32 oracle's backward from ITS fp32 forward against the fp64 backward from that same forward.  (End
to end against an fp64 forward the oracle's sequential sums cost it 20 - 50 x 2^-24 at these widths and the bar pins under 99 %.)
On the CPU the oracle's forward stands in for the kernel's; the GPU tests rebuild the bracket from the forward the launch stored.

The half bracket.  A kernel that rounds (RNE) a value v with |v - ref64| <= b s to half can store exactly the halves in
[RNE16(ref64 - b s), RNE16(ref64 + b s)]: rounding is monotone, and numpy's float64 -> float16 cast is one RNE rounding.  Compared
as values; +-Inf where the bracket overflows; NaN where both ends are NaN.  An element is PINNED when both ends are the same
half.  b is around 2^-21 and a half's spacing 2^-11 of its value, so about 2 b / 2^-11 = 0.1-0.2 % of the elements straddle a tie;
every dense case must pin at least PINNED_MIN = 99 % of its finite gradient elements, or the bracket hides failures.

CPU only; tests/test_f16_rows_model.py proves this module, tests/test_gpu_f16_rows_accuracy.py uses it.
"""
import numpy as np

import cosine_model as cm

MAX_D = 2048
PINNED_MIN = 0.99
SPEC_WINDOW_32 = 12          # euclid_math.h: SpecPlan<32>::H1, ulps either side of the predicted end of segment 0


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def f16_rows_ok(D, q=0, a=0, dq=0, da=0, bwd=False):
    """simcross_rows_f16.hip: f16_rows_ok; q, a, dq, da are addresses."""
    return D % 8 == 0 and D <= MAX_D and q % 16 == 0 and a % 16 == 0 and (not bwd or (dq % 16 == 0 and da % 16 == 0))


def wave_pairs(D):
    """euclid_math.h: wave_pairs."""
    return 2 if D <= 400 else 1


def family(D, mode="ordered"):
    """simcross_euclid_rows_f16: `tree` first, then rw == 2, else the lane chain."""
    if mode == "tree":
        return "tree"
    return "wave2" if wave_pairs(D) == 2 else "lanechain"


def nit(fam, D):
    """simcross_euclid_rows_f16: nit = (rw * D8 + 63) / 64 with rw = tree ? 1 : wave_pairs(D); simcross_cosine_rows_f16: (D8 + 63) / 64."""
    rw = 2 if fam == "wave2" else 1
    return (rw * (D // 8) + 63) // 64


PAIRS_PER_WG = dict(tree=4, wave2=8, lanechain=8, cosine=4)      # the grids: (N + 3) / 4, (N + 4 rw - 1) / (4 rw), (N + wpb - 1) / wpb, (N + 3) / 4


def npad(D):
    """euclid_rows_wave_f16_kernel: npad = st4 - D4, st4 = 3 spec_h4(D4)."""
    D4 = D // 4
    return 3 * ((D4 + 2) // 3) - D4


def cell(fam, D, bwd):
    return (fam, bool(bwd), nit(fam, D))


def families_of(D):
    """The families a width can be sent to."""
    return ("tree", family(D), "cosine")


REACHABLE = {cell(f, D, b) for D in range(8, MAX_D + 1, 8) for f in families_of(D) for b in (False, True)}
UNREACHABLE = {("wave2", b, n) for b in (False, True) for n in (3, 4)}       # 2 D8 <= 100 < 129

# ----------------------------------------------------------------------------------------------------------------------
# the shapes (N, D); every one is run forward-only and fused
# ----------------------------------------------------------------------------------------------------------------------
WAVE2 = [(5, 8),        # NIT 1: two lanes of the wave hold data; N % 8 == 5: the third wave has one pair, the second half-wave mirrors
         (9, 256),      # 2 D8 == 64: exactly one full trip; N % 8 == 1
         (6, 264),      # 2 D8 == 66: two lanes in trip 2
         (4, 384),      # D4 == 96: npad == 0, no zero float4 behind the image
         (7, 400),      # the last width of two pairs per wave; N % 8 == 7
         (1, 304),      # one pair: the second half-wave mirrors it
         (16, 304)]     # N % 8 == 0: exactly two full workgroups
LANECHAIN = [(3, 408),  # the first width of the lane chain: D8 == 51
             (9, 512),  # D8 == 64: one full trip; N % 8 == 1
             (8, 520),  # D8 == 65: one lane in trip 2; N % 8 == 0
             (5, 1024),  # D8 == 128: NIT 2 full
             (7, 1032),  # D8 == 129: NIT 3, one lane in trip 3; N % 8 == 7
             (2, 1536),  # D8 == 192: NIT 3 full
             (3, 1544),  # D8 == 193: NIT 4, one lane in trip 4
             (1, 2048)]  # D8 == 256: NIT 4 full; seven waves mirror row 0
TREE = [(5, 8),         # N % 4 == 1
        (6, 384),       # D8 == 48: one trip, partly filled
        (9, 512),       # D8 == 64: one full trip
        (4, 520),       # D8 == 65: NIT 2, one lane in trip 2; N % 4 == 0
        (7, 1032),      # NIT 3, one lane in trip 3; N % 4 == 3
        (2, 1536),      # NIT 3 full
        (3, 2048)]      # NIT 4 full
COSINE = [(5, 8),       # N % 4 == 1
          (9, 512),     # D8 == 64: one full trip
          (6, 520),     # D8 == 65: NIT 2, one lane in trip 2
          (7, 1032),    # NIT 3, one lane in trip 3; N % 4 == 3
          (2, 1536),    # NIT 3 full
          (3, 1544),    # NIT 4, one lane in trip 4
          (1, 2048),    # NIT 4 full; three waves return early
          (8, 304)]     # N % 4 == 0; D8 == 38
TABLE = dict(wave2=WAVE2, lanechain=LANECHAIN, tree=TREE, cosine=COSINE)
ADVERSARIAL_D = (200, 304)       # wave2: the 32-lane windows
EDGE_D = dict(wave2=304, lanechain=1032, tree=520, cosine=1032)


def shape_id(s):
    return "x".join(str(int(v)) for v in s)


def table_cells():
    return {cell(f, D, b) for f, shapes in TABLE.items() for (_, D) in shapes for b in (False, True)}


# ----------------------------------------------------------------------------------------------------------------------
# the half bracket
# ----------------------------------------------------------------------------------------------------------------------
def half_bracket(ref64, scale, b):
    """(lo, hi) float16: the RNE halves of ref64 -+ b scale."""
    ref64, scale = np.asarray(ref64, np.float64), np.asarray(scale, np.float64)
    with np.errstate(all="ignore"):
        w = b * scale
        return (ref64 - w).astype(np.float16), (ref64 + w).astype(np.float16)


def in_bracket(got16, lo, hi):
    """Per element: lo <= got <= hi as values (so -0 == +0 and +-Inf compare); where both ends are NaN, got is NaN."""
    assert got16.dtype == np.float16 and lo.dtype == np.float16 and hi.dtype == np.float16 and got16.shape == lo.shape == hi.shape
    g, l, h = (x.astype(np.float64) for x in (got16, lo, hi))
    both_nan = np.isnan(l) & np.isnan(h)
    with np.errstate(invalid="ignore"):
        return np.where(both_nan, np.isnan(g), (l <= g) & (g <= h))


def pinned_share(lo, hi):
    """The share of the elements with finite ends whose two ends are the same half."""
    fin = np.isfinite(lo) & np.isfinite(hi)
    return float((lo[fin] == hi[fin]).mean()) if fin.any() else 1.0


def check_bracket(what, got16, ref64, scale, b):
    lo, hi = half_bracket(ref64, scale, b)
    ok = in_bracket(got16, lo, hi)
    if not ok.all():
        i = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d halves outside [RNE16(ref - b s), RNE16(ref + b s)], b = %.2f x 2^-24; first at %s: got %r, "
                             "bracket [%r, %r], fp64 %r" % (what, int((~ok).sum()), ok.size, b / cm.U24, i, got16[i], lo[i], hi[i],
                                                            np.asarray(ref64)[i]))
    return lo, hi


# ----------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------
def top_diff_spanning(r, N):
    """N(0, 1) 2^s_n with s_n spread evenly over -10 .. 10 across the pairs (N == 1: s = 0), never zero."""
    s = np.rint(np.linspace(-10, 10, N)) if N > 1 else np.zeros(1)
    g = r.standard_normal(N)
    g = np.where(np.abs(g) < 2.0 ** -6, 1.0, g)
    return np.ldexp(g, s.astype(np.int32)).astype(np.float32).reshape(N, 1, 1, 1)


def dense_inputs(shape, euclid):
    """GloVe-like rows rounded to half and top_diff spanning 2^-10 .. 2^10 across pairs.  Euclid: pair 1 has a == q (N >= 2:
    distance 0, T = 1, the divisor 1e-9) and the last pair top_diff == 0 (N >= 3)."""
    from util import qa
    N, D = shape
    r = np.random.default_rng(1701 + 13 * N + D + (0 if euclid else 5))
    q, a = qa(r, N, 1, 1, D)
    qh, ah = q.astype(np.float16), a.astype(np.float16)
    dT = top_diff_spanning(r, N)
    if euclid:
        if N >= 2:
            ah[1] = qh[1]
        if N >= 3:
            dT[N - 1] = 0.0
    return qh, ah, dT


def adversarial_rows(D):
    """tests/test_gpu_parity.py: test_euclid_speculation_miss_falls_back_exactly, in halves: one coordinate 1.0, then coordinates
    whose squares (the half just below 2^-12, squared: below 2^-24) are under half an ulp of the running sum.  (qh, ah) of 6 pairs."""
    N = 6
    q = np.zeros((N, 1, D), np.float16)
    a = np.zeros((N, 1, D), np.float16)
    tiny = np.nextafter(np.float16(2.0 ** -12), np.float16(0))
    q[:, 0, 0] = 1.0
    q[0:2, 0, 1:] = tiny                    # small terms in every segment
    q[2:4, 0, 1:D // 2] = tiny              # in segment 0 and part of segment 1
    q[4, 0, 1:] = -tiny
    a[5, 0, :] = (np.random.default_rng(3).standard_normal(D) * 0.4).astype(np.float16)   # an ordinary row alongside
    return q, a


def first_segment_sums(qh, ah, pair):
    """(tree, seq) fp32 sums of the squares of segment 0 (spec_h4 float4) of one pair: what centres the window, what it must hit."""
    D = qh.shape[-1]
    n = ((D // 4 + 2) // 3) * 4
    d = qh[pair, 0, :n].astype(np.float32) - ah[pair, 0, :n].astype(np.float32)
    sq = (d * d).astype(np.float32)
    seq = np.float32(0)
    for v in sq:
        seq = np.float32(seq + v)
    return np.float32(sq.astype(np.float64).sum()), seq


def edge_rows(D, cosine):
    """(qh, ah, dT, names) of 10 pairs of GloVe-like halves, one edge per pair; names[i] says what pair i holds."""
    from util import qa
    N = 10
    r = np.random.default_rng(1701 + 3 * D + int(cosine))
    q, a = qa(r, N, 1, 1, D)
    qh, ah = q.astype(np.float16), a.astype(np.float16)
    dT = np.ldexp(r.choice(np.array([1.0, -1.5, 1.25]), N), r.integers(-3, 4, N)).astype(np.float32).reshape(N, 1, 1, 1)
    names = ["clean"] * N
    qh[0, 0, 5 % D] = np.inf
    names[0] = "q holds Inf"
    ah[1, 0, D - 1] = np.nan
    names[1] = "a holds NaN"
    qh[2, 0, :], ah[2, 0, :] = 65504.0, -65504.0
    qh[2, 0, 1::2], ah[2, 0, 1::2] = -65504.0, 65504.0
    names[2] = "+-65504 against -+65504 in every coordinate"
    sub = lambda: np.ldexp(r.integers(1, 1024, D).astype(np.float64), -24).astype(np.float16) * r.choice(np.array([-1, 1], np.float16), D)
    qh[3, 0], ah[3, 0] = sub(), sub()
    names[3] = "subnormal halves"
    dT[4] = 1e8
    if not cosine:
        ah[4, 0, 64:] = qh[4, 0, 64:]           # a short distance: T large enough for 1e8 T^3 |q - a| / (1 - T) to pass 65504
    names[4] = "top_diff 1e8: half gradients overflow"
    qh[5, 0, D // 2], ah[5, 0, D // 2] = np.inf, np.inf
    names[5] = "Inf in both operands at one coordinate"
    qh[6, 0, D - 1], ah[6, 0, D - 1] = -65504.0, 65504.0
    names[6] = "one coordinate -65504 against 65504"
    if cosine:
        qh[7, 0] = 0
        names[7] = "zero q row"
        ah[8, 0] = 0
        names[8] = "zero a row"
    else:
        ah[7] = qh[7]
        names[7] = "a == q"
        dT[8] = 0.0
        names[8] = "top_diff == 0"
    return qh, ah, dT, names


# ----------------------------------------------------------------------------------------------------------------------
# references: computed once per case, shared read-only
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def finite_error(got, ref64, scale):
    """cosine_model.scaled_error over the elements whose reference and scale are finite (0.0 if there are none)."""
    ref64, scale = np.asarray(ref64, np.float64), np.asarray(scale, np.float64)
    fin = np.isfinite(ref64) & np.isfinite(scale)
    if not fin.any():
        return 0.0
    return cm.scaled_error(np.asarray(got)[fin], ref64[fin], scale[fin])[0]


def euclid_grad_ref(oracle, c, top32):
    """((dq64, scale), (da64, scale)): the fp64 oracle's backward on the widened inputs from the fp32 scores `top32` -- the
    backward's own inputs, as in cosine_model.grad_ref; scale |ref64| (one product chain per element, no cancellation)."""
    f64 = lambda x: np.asarray(x).astype(np.float64)
    with np.errstate(all="ignore"):
        dq64, da64, _, _ = oracle.simcross_backward(1, f64(c["qh"]), f64(c["ah"]), f64(top32), f64(c["dT"]))
    return (dq64, np.abs(dq64)), (da64, np.abs(da64))


def cosine_grad_ref(c, top32, n032, n132):
    """cosine_model.grad_ref on the widened inputs from the fp32 forward (top32, n032, n132): fp64 values and the scales |t1| + |t2|."""
    with np.errstate(all="ignore"):
        return cm.grad_ref(c["qh"].astype(np.float32), c["ah"].astype(np.float32), top32, n032, n132, c["dT"])


def euclid_reference(oracle, qh, ah, dT):
    """The widened inputs through the fp32 oracle (forward, then backward from its top); top against the fp64 oracle, relative;
    the gradients against the fp64 backward from the SAME fp32 top (euclid_grad_ref); e_o = the fp32 oracle's scaled errors
    over the finite elements."""
    q32, a32 = qh.astype(np.float32), ah.astype(np.float32)
    f64 = lambda x: x.astype(np.float64)
    c = dict(qh=qh, ah=ah, dT=dT)
    with np.errstate(all="ignore"):
        c["top"], _, _ = oracle.simcross_forward(1, q32, a32)
        c["dq"], c["da"], _, _ = oracle.simcross_backward(1, q32, a32, c["top"], dT)
        top64, _, _ = oracle.simcross_forward(1, f64(q32), f64(a32))
    rq, ra = euclid_grad_ref(oracle, c, c["top"])
    c["ref"] = dict(top=(top64, np.abs(top64)), dq=rq, da=ra)
    c["e_o"] = {k: finite_error(c[k], *c["ref"][k]) for k in ("top", "dq", "da")}
    return cm._freeze(c)


def cosine_reference(oracle, qh, ah, dT):
    """As euclid_reference for dist_mode 0: top (scale sum |q_i a_i| / (n0 n1)) and the norms against fp64; the gradients against
    cosine_grad_ref from the fp32 oracle's own forward."""
    q32, a32 = qh.astype(np.float32), ah.astype(np.float32)
    f64 = lambda x: x.astype(np.float64)
    c = dict(qh=qh, ah=ah, dT=dT)
    with np.errstate(all="ignore"):
        c["top"], c["n0"], c["n1"] = oracle.simcross_forward(0, q32, a32)
        c["dq"], c["da"], _, _ = oracle.simcross_backward(0, q32, a32, c["top"], dT, norm0=c["n0"], norm1=c["n1"])
        top64, n064, n164 = oracle.simcross_forward(0, f64(q32), f64(a32))
        dq64, da64, _, _ = oracle.simcross_backward(0, f64(q32), f64(a32), f64(c["top"]), f64(dT), norm0=f64(c["n0"]), norm1=f64(c["n1"]))
        top_np, mt = cm.top_ref(q32, a32)
    rq, ra = cosine_grad_ref(c, c["top"], c["n0"], c["n1"])
    # the vectorised fp64 expressions that give the scales agree with the fp64 oracle
    for x, y, m in ((top_np, top64, mt), (rq[0], dq64, rq[1]), (ra[0], da64, ra[1])):
        assert finite_error(x, y, m) < 2.0 ** -40
    c["ref"] = dict(top=(top64, mt), n0=(n064, n064), n1=(n164, n164), dq=rq, da=ra)
    c["e_o"] = {k: finite_error(c[k], *c["ref"][k]) for k in ("top", "n0", "n1", "dq", "da")}
    return cm._freeze(c)


def dense_case(oracle, fam, shape):
    key = ("dense", fam == "cosine") + tuple(shape)
    if key not in _cases:
        qh, ah, dT = dense_inputs(shape, euclid=fam != "cosine")
        _cases[key] = (cosine_reference if fam == "cosine" else euclid_reference)(oracle, qh, ah, dT)
    return _cases[key]


def edge_case(oracle, fam):
    key = ("edge", fam == "cosine", EDGE_D[fam])
    if key not in _cases:
        qh, ah, dT, names = edge_rows(EDGE_D[fam], fam == "cosine")
        c = dict((cosine_reference if fam == "cosine" else euclid_reference)(oracle, qh, ah, dT))
        c["names"] = names
        _cases[key] = c
    return _cases[key]


def probe_case(oracle, shape):
    """cosine_model.probe_inputs at (N, 1, 1, D), as halves: the oracle's forward and, for the ONE contribution of each gradient
    element, its fp64 value and scale from that forward."""
    key = ("probe",) + tuple(shape)
    if key not in _cases:
        N, D = shape
        p = cm.probe_inputs(np.random.default_rng(1701 + 31 * N + D), N, 1, 1, D)
        c = dict(q=p["q"], a=p["a"], qh=p["q"].astype(np.float16), ah=p["a"].astype(np.float16), dT=p["dT_rows"], eq=p["eq"], ea=p["ea"])
        c["top"], c["n0"], c["n1"] = oracle.simcross_forward(0, c["q"], c["a"])
        (dq64, mq), (da64, ma) = cm.grad_ref(c["q"], c["a"], c["top"], c["n0"], c["n1"], c["dT"])
        c["ref"] = dict(dq=(dq64, mq), da=(da64, ma))
        c["dq"], c["da"], _, _ = oracle.simcross_backward(0, c["q"], c["a"], c["top"], c["dT"], norm0=c["n0"], norm1=c["n1"])
        _cases[key] = cm._freeze(c)
    return _cases[key]
