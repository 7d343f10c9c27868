// csrc/euclid_math.h -- the Euclidean SimCross backward term, bit-exact with
// the reference CPU expression (src/caffe/layers/sim_cross_layer.cpp:216-217)
//
//   Dtype tt = top_diff*top*top*top*(q - a) / (top - 1 + 1e-9);
//
// For Dtype = float the numerator is a float product evaluated left to right,
// `top - 1` is a float, `+ 1e-9` promotes to double, the quotient is a double
// division, and the assignment rounds it to float.
#ifndef MMS_EUCLID_MATH_H_
#define MMS_EUCLID_MATH_H_

#include <hip/hip_runtime.h>

#include "mms_common.h"

namespace mms {

// Per-(pair,j,k) coefficients.  c = ((g*T)*T)*T ; den = (double)(T-1) + 1e-9 ;
// rcp ~ 1/den (about 1 ulp), used only by the self-checking fast path below.
struct EuclidCoef {
  float c;
  double den;
  double rcp;
};

// 1/den to ~1 ulp without the ~35-instruction IEEE division: hardware
// reciprocal seed + two Newton steps (each squares the relative error; the
// seed is good to > 20 bits, so two steps leave only the final roundings).
// Only euclid_tt's fast path consumes it, and that path re-checks itself.
__device__ __forceinline__ double rcp_newton(double den) {
  double r = __builtin_amdgcn_rcp(den);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
  return r;
}

__device__ __forceinline__ EuclidCoef euclid_coef(float T, float g) {
  EuclidCoef k;
  k.c = g * T * T * T;
  k.den = (double)(T - 1.0f) + 1e-9;
  k.rcp = rcp_newton(k.den);
  return k;
}

// Lane `src`'s den or rcp in every lane; `src` is a compile-time lane once the caller's loop is unrolled: two v_readlane.
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)b, src);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The reference expression, literally.
__device__ __forceinline__ float euclid_tt_exact(float c, double den, float diff) {
  return (float)((double)(c * diff) / den);
}

// Same bits, ~4x fewer instructions: one fp64 multiply by the per-pair
// reciprocal instead of an fp64 division per element.
//   Q = num/den (real).  The reference returns fl32(fl64(Q)).
//   p = fl64(num * rcp), rcp = 1/den to ~1 ulp, is within a few double-ulps
//   of fl64(Q) (rcp error <= ~2 ulp, product rounding 0.5 ulp, each up to 2x
//   when expressed in ulps of p).  fl32(p) can differ from fl32(fl64(Q)) only
//   if a float rounding boundary lies between them.  Below float precision a
//   double carries 29 mantissa bits; the boundary (midpoint of two floats) is
//   the pattern 1000...0 = 2^28 in those bits.  If p's low 29 bits are
//   farther than 64 from 2^28 there is no boundary within reach and the cheap
//   result is the reference's result; otherwise (probability ~2.4e-7) the lane
//   redoes the division exactly.  Results in the float-subnormal range round
//   at a different bit and also take the exact path.
__device__ __forceinline__ float euclid_tt(const EuclidCoef& k, float diff) {
  const float num = k.c * diff;
  const double p = (double)num * k.rcp;
  float res = (float)p;
  const unsigned lo = (unsigned)__double_as_longlong(p) & 0x1fffffffu;
  const bool near_boundary = (lo - 0x0fffffc0u) <= 128u;
  const bool tiny = (fabsf(res) <= 1.17549435e-38f) && (num != 0.0f);
  if (near_boundary || tiny) res = (float)((double)num / k.den);
  return res;
}

// The term in the fp32 arithmetic of MMS_EUCLID_BWD_FP32 (include/mms.h): r = fl32(1/den), at most 2 ulp from
// euclid_tt's value.
__device__ __forceinline__ float euclid_tt_f32(float c, float r, float diff) { return (c * diff) * r; }

// Four elements that share one coefficient set (a float4 of one pair's row):
// same arithmetic as euclid_tt, with the rare-case tests made cheaper and
// RETURNED instead of branched on, so that a caller can run several float4s
// as one straight-line block (independent instruction chains interleave) and
// take a single wave-level branch for all of them:
//   * "result could be float-subnormal" needs |num * rcp| < 2^-126; when
//     |rcp| >= 1 (always true for T in (0,1]: |den| <= 1) that requires num
//     itself to be subnormal -- one v_cmp_class per element; a pair whose
//     |rcp| < 1 (only possible for caller-supplied T outside (0,1]) takes the
//     exact path wholesale.
__device__ __forceinline__ float4 euclid_tt4_fast(const EuclidCoef& k, const float4& d, bool& risky) {
  const float n0 = k.c * d.x, n1 = k.c * d.y, n2 = k.c * d.z, n3 = k.c * d.w;
  const double p0 = (double)n0 * k.rcp, p1 = (double)n1 * k.rcp;
  const double p2 = (double)n2 * k.rcp, p3 = (double)n3 * k.rcp;
  float4 r;
  r.x = (float)p0; r.y = (float)p1; r.z = (float)p2; r.w = (float)p3;
  auto near = [](double p) {
    const unsigned lo = (unsigned)__double_as_longlong(p) & 0x1fffffffu;
    return (lo - 0x0fffffc0u) <= 128u;
  };
  auto subn = [](float x) -> bool { return __builtin_isfpclass(x, 0x0090 /* +-subnormal */); };
  risky = near(p0) || near(p1) || near(p2) || near(p3) || subn(n0) || subn(n1) || subn(n2) ||
          subn(n3) || !(fabs(k.rcp) >= 1.0);
  return r;
}
__device__ __forceinline__ float4 euclid_tt4_exact(const EuclidCoef& k, const float4& d) {
  float4 r;
  r.x = euclid_tt_exact(k.c, k.den, d.x); r.y = euclid_tt_exact(k.c, k.den, d.y);
  r.z = euclid_tt_exact(k.c, k.den, d.z); r.w = euclid_tt_exact(k.c, k.den, d.w);
  return r;
}
__device__ __forceinline__ float4 euclid_tt4(const EuclidCoef& k, const float4& d) {
  bool risky;
  float4 r = euclid_tt4_fast(k, d, risky);
  if (risky) r = euclid_tt4_exact(k, d);
  return r;
}

// s = init; for i in [0, n4): s += r4[i].x, .y, .z, .w  (fp32, adds only, in
// that order) -- the reference's accumulation order for `dist += diff*diff`
// (sim_cross_layer.cpp:100-105) once the squares are formed.  `r4` points at
// float4 squares in LDS.  The chain is bound by VALU issue (~4.5 cycles per
// wave-instruction whatever the number of active lanes) as much as by add
// latency, so the loop carries NOTHING but the adds: LDS reads run one
// 8 x 16 B batch ahead with immediate offsets, and no per-element predicate.
__device__ __forceinline__ float chain_sum_lds(const float4* r4, int n4, float init) {
  float s = init;
  const int nb = n4 >> 3;
  float4 va[8], vb[8];
  if (nb > 0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) va[u] = r4[u];
  }
  int b = 0;
  for (; b + 2 <= nb; b += 2) {
#pragma unroll
    for (int u = 0; u < 8; ++u) vb[u] = r4[(b + 1) * 8 + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s += va[u].x; s += va[u].y; s += va[u].z; s += va[u].w;
    }
    if (b + 2 < nb) {
#pragma unroll
      for (int u = 0; u < 8; ++u) va[u] = r4[(b + 2) * 8 + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s += vb[u].x; s += vb[u].y; s += vb[u].z; s += vb[u].w;
    }
  }
  if (b < nb) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s += va[u].x; s += va[u].y; s += va[u].z; s += va[u].w;
    }
  }
  for (int d = nb * 8; d < n4; ++d) {
    const float4 v = r4[d];
    s += v.x; s += v.y; s += v.z; s += v.w;
  }
  return s;
}

// Packed variant: one v_pk_add_f32 advances TWO running sums (the two halves of
// `s`) by the same addend.  op_sel picks which dword of the 64-bit source pair
// feeds both halves, so no broadcast moves are needed (plain vector code: hipcc
// emits the op_sel forms itself and keeps its counted LDS waits).  Measured
// (profiles/r01_chainbench…): ~10.5 ticks per dependent packed add however many
// waves share the SIMD, against ~14 for a plain add at two waves per SIMD.
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2v chain_sum_lds_pk(const float4* r4, int n4, float2v init) {
  float2v s = init;
  auto step = [&](const float4& v) {
    // hipcc lowers each line to one v_pk_add_f32 with op_sel broadcasting the addend
    s = s + (float2v){v.x, v.x};
    s = s + (float2v){v.y, v.y};
    s = s + (float2v){v.z, v.z};
    s = s + (float2v){v.w, v.w};
  };
  const int nb = n4 >> 3;
  float4 va[8], vb[8];
  if (nb > 0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) va[u] = r4[u];
  }
  int b = 0;
  for (; b + 2 <= nb; b += 2) {
#pragma unroll
    for (int u = 0; u < 8; ++u) vb[u] = r4[(b + 1) * 8 + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) step(va[u]);
    if (b + 2 < nb) {
#pragma unroll
      for (int u = 0; u < 8; ++u) va[u] = r4[(b + 2) * 8 + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) step(vb[u]);
  }
  if (b < nb) {
#pragma unroll
    for (int u = 0; u < 8; ++u) step(va[u]);
  }
  for (int d = nb * 8; d < n4; ++d) step(r4[d]);
  return s;
}

// ---------------------------------------------------------------------------
// Speculative three-segment evaluation of the d-ascending chain, bit-exact.
//
// A dependent fp32 add costs ~6.6 cycles of latency and ~4.5 issue cycles of
// its SIMD no matter how few lanes are active (profiles/r01_chainbench_*), so
// a D-long chain per pair is the critical path of the forward pass.  The chain
// cannot be re-associated (it must round like the reference), but a later
// segment can be started before the earlier ones have finished if the value
// they will end on is GUESSED: the sequential fp32 partial sum differs from a
// tree sum of the same terms by a few ulps only (random-walk rounding error,
// sigma ~ 0.22*sqrt(n) ulp: 1.8 ulp at n = 100, 2.5 at n = 200, measured).
// Each pair gets LPR = 64/RW lanes and, thanks to packed adds, 2*LPR running
// sums ("slots"):
//   lane 0                 walks segment 0 from 0                       (exact prefix)
//   lanes 1 .. L1          walk segment 1 from pred1 + k ulps, |k| <= H1
//   lanes L1+1 .. LPR-1    walk segment 2 from pred2 + k ulps, |k| <= H2
// (LPR = 32: H1 = 12, H2 = 15; LPR = 64: H1 = 25, H2 = 36), where pred1/pred2
// are tree sums of segment 0 / segments 0-1.  When the walks finish, the exact
// end of segment 0 selects the segment-1 slot whose start value IS that end --
// that slot has computed exactly the reference's continuation -- and its end
// selects the segment-2 slot the same way.  A miss (the true value outside the
// window; < 1e-6 per pair on embedding-like data, forced in the tests) re-walks
// that segment from the exact value.  The result is the reference's sum bit for
// bit in every case; only the time varies.
//
// LDS image of one pair: its D4 float4 squares followed by all-zero float4 up
// to 3*h4, h4 = ceil(D4/3); segment g is [g*h4, (g+1)*h4).  Adding +0 to the
// non-negative running sum is exact, so every lane runs the same h4 steps.
__host__ __device__ __forceinline__ int spec_h4(int D4) { return (D4 + 2) / 3; }
__host__ __device__ __forceinline__ int spec_stride4(int D4) { return 3 * spec_h4(D4); }
// What float4 `i4` (tree sum `s4`) of a pair's image adds to (pred1, pred2) of its pair; `r1`: the wave's second pair.
template <int RW>
__device__ __forceinline__ void spec_pred_add(float2v (&pred)[RW], bool r1, int i4, int h4, float s4) {
  const float2v c = {(i4 < h4) ? s4 : 0.f, (i4 < 2 * h4) ? s4 : 0.f}, z2 = {0.f, 0.f};
  pred[0] += r1 ? z2 : c;
  if (RW == 2) pred[RW - 1] += r1 ? c : z2;
}

// Host-side facts about the kernels built on this scheme (the three simcross_rows*.hip and the fused triplet steps
// of triplet_steps.hip route on them; each is written here and nowhere else).
// Dynamic LDS of a workgroup of `waves` waves that each hold `pairs_per_wave` images of D4 float4.
inline size_t spec_image_lds(int waves, int pairs_per_wave, int D4) {
  return (size_t)waves * pairs_per_wave * spec_stride4(D4) * sizeof(float4);
}
// Widths with a kernel specialised at compile time: 100-d, 200-d and 300-d GloVe (D4 = 25, 50, 75).
inline bool glove_width(int D) { return D == 300 || D == 200 || D == 100; }
// f(std::integral_constant<int, D4>{}) for such a width, so that D4 can be a template argument:
// with_glove_d4(D, [&](auto W) { launch K<decltype(W)::value, ...> }).  Calls nothing for any other D.
template <class F>
inline void with_glove_d4(int D, F&& f) {
  switch (D) {
    case 100: f(std::integral_constant<int, 25>{}); break;
    case 200: f(std::integral_constant<int, 50>{}); break;
    case 300: f(std::integral_constant<int, 75>{}); break;
  }
}
// A wave kernel keeps a pair in registers, at most four 16-byte loads per operand per lane of a whole wave.
inline bool wave_width_ok(int D) { return D <= 1024; }
// Two pairs per wave (32 candidate lanes each) only while the narrower windows hold: at D = 1024 the ordered
// fp32 sum of a 344-term segment strays sigma ~ 6 ulp from its tree-sum prediction, the +-12 / +-15 windows
// of 32 lanes missed on 3.4 % of pairs and the exact re-walks ate the gain at cfg 5's shard
// size (19.5 vs 18.6 us; 125 vs 149 us at 65536 pairs).  One pair per wave beyond.
inline int wave_pairs(int D) { return D <= 400 ? 2 : 1; }

template <int LPR> struct SpecPlan;
template <> struct SpecPlan<32> { static constexpr int H1 = 12, L1 = 13, H2 = 15; };
template <> struct SpecPlan<64> { static constexpr int H1 = 25, L1 = 26, H2 = 36; };

// `img4`   this pair's image in LDS (pad entries already zero)
// `pred1`, `pred2`  tree sums of segment 0 and of segments 0-1 (they only centre the windows)
// `j`      this lane's index within the pair's lane group; `lead` = lane id of j = 0
// returns  the full sum, valid in EVERY lane of the group.
template <int LPR>
__device__ __forceinline__ float chain_sum_speculative(const float4* img4, int D4, float pred1,
                                                       float pred2, int j, int lead) {
  typedef SpecPlan<LPR> P;
  const int h4 = spec_h4(D4);
  const int seg = (j == 0) ? 0 : (j <= P::L1 ? 1 : 2);
  const int c0 = (seg == 1) ? 2 * (j - 1) - P::H1 : 2 * (j - 1 - P::L1) - P::H2;   // ulp offset of slot 0
  const int pbits = __float_as_int(seg == 1 ? pred1 : pred2);
  float2v start;
  start.x = (seg == 0) ? 0.0f : __int_as_float(pbits + c0);
  start.y = (seg == 0) ? 0.0f : __int_as_float(pbits + c0 + 1);
  __builtin_amdgcn_s_setprio(3);
  const float2v end = chain_sum_lds_pk(img4 + seg * h4, h4, start);
  // segment 0 -> 1
  const float s1 = __shfl(end.x, lead, 64);
  const int k1 = __float_as_int(s1) - __float_as_int(pred1) + P::H1;     // slot index in segment 1
  const bool hit1 = (k1 >= 0) && (k1 <= 2 * P::H1);
  const int l1 = lead + 1 + ((hit1 ? k1 : 0) >> 1);
  const float e1x = __shfl(end.x, l1, 64), e1y = __shfl(end.y, l1, 64);
  float s2 = (k1 & 1) ? e1y : e1x;
  if (!hit1) s2 = chain_sum_lds(img4 + h4, h4, s1);   // re-walk, exact
  // segment 1 -> 2
  const int k2 = __float_as_int(s2) - __float_as_int(pred2) + P::H2;
  const bool hit2 = (k2 >= 0) && (k2 <= 2 * P::H2);
  const int l2 = lead + 1 + P::L1 + ((hit2 ? k2 : 0) >> 1);
  const float e2x = __shfl(end.x, l2, 64), e2y = __shfl(end.y, l2, 64);
  float s3 = (k2 & 1) ? e2y : e2x;
  if (!hit2) s3 = chain_sum_lds(img4 + 2 * h4, h4, s2);
  __builtin_amdgcn_s_setprio(0);
  return s3;
}

// Compile-time-length variants for the widths the wave-pair kernel is specialised
// for (simcross_rows.hip: euclid_pair32_kernel).  H4 (float4s per segment)
// is a constant, so
//  * the segment's LDS reads are all issued up front into registers (two waves
//    per SIMD leave 256 VGPRs per lane) -- and BEFORE the window centres are
//    reduced, so that LDS latency hides behind the DPP sums;
//  * the chain is H4*4 straight-line packed adds: no loop control, no register
//    rotation, and op_sel broadcasts each addend lane-locally;
//  * the two look-ups that stitch the segments together run on the SCALAR unit
//    (v_readlane with a computed lane, s_sub/s_cmp) instead of three dependent
//    ds_bpermute round trips;
//  * a miss anywhere (never observed on real data; forced by the adversarial
//    tests) sends the whole wave to ONE exact re-walk of the full image.
// Byte address of `p` within the workgroup's LDS, and the 16-byte read of float4 `u` behind such an address (one
// ds_read_b128 with an immediate offset, issued where it is written).
typedef __attribute__((address_space(3))) const mms_v4f lds_v4f;
__device__ __forceinline__ unsigned lds_address(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p;
}
__device__ __forceinline__ float4 lds_read4(unsigned addr, int u) {
  const mms_v4f t = ((lds_v4f*)(size_t)addr)[u];
  return make_float4(t.x, t.y, t.z, t.w);
}

template <int H4>
struct SpecSegment {
  float4 v[H4];
  __device__ __forceinline__ void load(const float4* r4) {
#pragma unroll
    for (int u = 0; u < H4; ++u) v[u] = r4[u];
  }
  __device__ __forceinline__ float2v chain(float2v s) const {
#pragma unroll
    for (int u = 0; u < H4; ++u) {
      const float2v lo = {v[u].x, v[u].y}, hi = {v[u].z, v[u].w};
      s = s + __builtin_shufflevector(lo, lo, 0, 0);
      s = s + __builtin_shufflevector(lo, lo, 1, 1);
      s = s + __builtin_shufflevector(hi, hi, 0, 0);
      s = s + __builtin_shufflevector(hi, hi, 1, 1);
    }
    return s;
  }

  // The same reads and the same adds with the chain started on its FIRST read.  lgkmcnt counts to 15: behind all H4
  // reads of load() the wait in front of step 0 can only say "at most 14 outstanding", i.e. H4 - 14 reads back,
  // while step 0 needs read 0.  So load_first() issues AHEAD <= 15 reads, and chain_streamed() issues read u + AHEAD
  // right after the four adds of step u, as counter room appears: every wait in the chain is then the exact count
  // of the read it needs (AHEAD - 1 outstanding behind it).  Whatever the caller puts between the two calls runs
  // while read 0 is on its way.  `seg` is the segment's LDS byte address (lds_address below), which the caller can
  // form and pin long before the reads.  The empty asm makes the address of read u + AHEAD depend on the sum after
  // step u -- no instruction, but the read cannot be hoisted back to the front -- and one scheduling fence per step
  // keeps it from drifting behind the next step.
  static constexpr int AHEAD = H4 < 15 ? H4 : 15;
  __device__ __forceinline__ void load_first(unsigned seg) {
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) v[u] = lds_read4(seg, u);
  }
  __device__ __forceinline__ float2v chain_streamed(unsigned seg, float2v s) {
#pragma unroll
    for (int u = 0; u < H4; ++u) {
      const float2v lo = {v[u].x, v[u].y}, hi = {v[u].z, v[u].w};
      s = __builtin_shufflevector(lo, lo, 0, 0) + s;
      s = __builtin_shufflevector(lo, lo, 1, 1) + s;
      s = __builtin_shufflevector(hi, hi, 0, 0) + s;
      s = __builtin_shufflevector(hi, hi, 1, 1) + s;
      if (u + AHEAD < H4) {
        asm volatile("" : "+v"(seg) : "v"(s));
        v[u + AHEAD] = lds_read4(seg, u + AHEAD);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    return s;
  }
};

// segment of lane j of a 32-lane group: j = 0 walks segment 0 from 0.0f exactly
__device__ __forceinline__ int spec_seg32(int j) { return (j == 0) ? 0 : (j <= SpecPlan<32>::L1 ? 1 : 2); }

__device__ __forceinline__ float2v spec_start32(float pred1, float pred2, int j) {
  typedef SpecPlan<32> P;
  const int seg = spec_seg32(j);
  const int c0 = (seg == 1) ? 2 * (j - 1) - P::H1 : 2 * (j - 1 - P::L1) - P::H2;   // ulp offset of slot 0
  const int pbits = __float_as_int(seg == 1 ? pred1 : pred2);
  float2v start;
  start.x = (seg == 0) ? 0.0f : __int_as_float(pbits + c0);
  start.y = (seg == 0) ? 0.0f : __int_as_float(pbits + c0 + 1);
  return start;
}

// Stitch the three segments of BOTH pairs of a wave at once (lanes 0-31 / 32-63), on the
// VALU: the lane whose start value equals the running total contributes its end value, and
// an OR-reduction over the half (DPP, no LDS) hands it to every lane.  Sums of squares are
// never negative, so bit 31 is free to carry "some lane matched".  Three reductions of six
// dependent DPP steps replace three ds_bpermute round trips (or ~40 dependent scalar ops).
// Returns the pair's total in every lane of its half; `hit` is false on a window miss.
__device__ __forceinline__ float spec_resolve_halves(float2v start, float2v end, int j, bool* hit) {
  constexpr unsigned F = 0x80000000u;
  const int seg = spec_seg32(j);
  const unsigned sx = __float_as_uint(start.x), sy = __float_as_uint(start.y);
  const unsigned ex = __float_as_uint(end.x) | F, ey = __float_as_uint(end.y) | F;
  const unsigned s1 = half_wave_or(j == 0 ? ex : 0u) & ~F;                 // segment 0 ends here
  const unsigned m1 = (seg == 1) ? (sx == s1 ? ex : (sy == s1 ? ey : 0u)) : 0u;
  const unsigned s2f = half_wave_or(m1);
  const unsigned s2 = s2f & ~F;
  const unsigned m2 = (seg == 2) ? (sx == s2 ? ex : (sy == s2 ? ey : 0u)) : 0u;
  const unsigned s3f = half_wave_or(m2);
  *hit = ((s2f & s3f) & F) != 0;
  return __uint_as_float(s3f & ~F);
}

// Compiler-level ordering between LDS writes of some lanes and LDS reads of
// other lanes of the SAME wave (the hardware executes a wave's LDS
// instructions in order; no workgroup barrier is needed or wanted).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace mms
#endif  // MMS_EUCLID_MATH_H_
