// csrc/simcross_rows.hip -- SimCross dist_mode 1 (Euclidean) for W1 == W2 == 1 (sentence-vector pairs; BASELINE
// cfg 2), fp32, for gfx950: the kernels, their routing and the per-thread backward mode.  HBM-bound: no MFMA here.
// The word-grid kernels and the three fp32 entry points, which try this side first, are in simcross_cross.hip; the
// rows kernels of dist_mode 0 and of half storage in the two other simcross_rows_*.hip.
//
// Reference semantics (all file:line in src/caffe/layers/sim_cross_layer.cpp):
//   Euclid fwd  :96-111   T = 1/(1+sqrt(sum_d (q-a)^2)), d ascending, fp32.
//   Euclid bwd  :208-225  tt = dT*T*T*T*(q-a)/(T-1+1e-9) (double divide); dq[d] = tt, da[d] = -tt.
//
// A workgroup owns ROWS consecutive pairs, streams them with 16-byte loads into LDS, and ONE lane per pair walks d
// ascending so the sum has the reference's order bit for bit.  The forward+backward fusion keeps q-a in LDS (or in
// registers) so q and a are read from HBM once.
//
// Compiled with -ffp-contract=off: the reference CPU build has no FMA
// contraction, so mul and add must round separately to match it bitwise.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "euclid_math.h"
#include "mms_internal.h"

namespace mms {

// ---- wave-centric kernel (the fast path) ------------------------------------
// A wave owns RW (1 or 2) consecutive pairs (RW*D/4 float4 per operand); the
// four waves of a workgroup are independent (no workgroup barrier).  Timeline
// of one wave:
//   1. ALL its 16-byte loads of q and a are issued back to back (NIT per
//      operand per lane, predicated) -- nothing waits inside a loop;
//   2. diff = q-a stays in registers; diff^2 goes to the wave's LDS slice;
//   3. the d-ascending sum of each pair's squares -- the reference's summation
//      order -- is evaluated by the pair's 64/RW lanes with the speculative
//      two-segment scheme of euclid_math.h (bit-exact, half the chain length);
//   4. every lane derives T and the backward coefficients of its pair
//      (wave-uniform per lane group; no LDS round trip);
//   5. every lane turns its register-resident diffs into dq / da and stores
//      16 bytes per lane.
// FWD only stops after 3; BWD only skips 2-3 and reads T from memory.
template <int NIT, int RW, bool FWD, bool BWD>
__global__ __launch_bounds__(256) void euclid_rows_wave_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_in, const float* __restrict__ top_diff,
    float* __restrict__ top_out, float* __restrict__ dq, float* __restrict__ da, int N,
    int D4) {
  constexpr int LPR = 64 / RW;                   // lanes per pair
  extern __shared__ float4 lds4[];               // [4 waves][RW split images] (euclid_math.h)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + wave) * RW;
  if (row0 >= N) return;                         // whole wave leaves; no block barrier below
  const int rows = min(RW, N - row0);
  const int n4 = rows * D4;
  const size_t base4 = (size_t)row0 * D4;
  const float4* q4 = reinterpret_cast<const float4*>(q) + base4;
  const float4* a4 = reinterpret_cast<const float4*>(a) + base4;
  const int st4 = spec_stride4(D4);
  float4* sq4 = lds4 + (size_t)wave * RW * st4;

  float4 x[NIT], y[NIT], df[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const int ii = i < n4 ? i : 0;               // clamp: keep the load unconditional
    x[it] = q4[ii];
    y[it] = a4[ii];
  }
  // this lane's pair for the chain / coefficient work
  const int grp = lane / LPR, j = lane % LPR;
  const int grow = min(grp, rows - 1);           // a missing 2nd pair mirrors the 1st (results unused)
  float T = 0.f;
  if (!FWD) T = top_in[row0 + grow];
  float g = 0.f;
  if (BWD) g = top_diff[row0 + grow];

  float2v pred[RW];                              // per pair: (pred1, pred2) partial sums
#pragma unroll
  for (int r = 0; r < RW; ++r) pred[r] = (float2v){0.f, 0.f};
  const int h4 = spec_h4(D4);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    df[it].x = x[it].x - y[it].x; df[it].y = x[it].y - y[it].y;
    df[it].z = x[it].z - y[it].z; df[it].w = x[it].w - y[it].w;
    if (FWD) {
      const int i = lane + 64 * it;
      float4 s;
      s.x = df[it].x * df[it].x; s.y = df[it].y * df[it].y;
      s.z = df[it].z * df[it].z; s.w = df[it].w * df[it].w;
      // image slot of this float4 (pair r's image starts at r*st4) and its tree-sum
      // contribution to the two predictions of the pair it belongs to
      const bool r1 = (RW == 2) && (i >= D4);
      const int ir = r1 ? i - D4 : i;
      if (i < n4) sq4[r1 ? i + (st4 - D4) : i] = s;
      const float s4 = (i < n4) ? (s.x + s.y) + (s.z + s.w) : 0.f;
      spec_pred_add<RW>(pred, r1, ir, h4, s4);
    }
  }
  if (FWD) {
    // zero pad at the end of each image (0..2 entries)
    const int npad = st4 - D4;
    if (lane < RW * npad) sq4[(lane / npad) * st4 + D4 + (lane % npad)] = make_float4(0.f, 0.f, 0.f, 0.f);
    float my1 = 0.f, my2 = 0.f;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float p1 = wave_sum(pred[r].x), p2 = wave_sum(pred[r].y);
      if (r == grow) { my1 = p1; my2 = p2; }
    }
    wave_lds_sync();
    const float dist = chain_sum_speculative<LPR>(sq4 + grow * st4, D4, my1, my2, j, grp * LPR);
    T = 1.0f / (1.0f + sqrtf(dist));            // :106-107
    if (BWD) asm volatile("" : "+v"(g));        // in a register before the store of T (see euclid_pair32_kernel)
    if (j == 0 && grp < rows) top_out[row0 + grp] = T;
  }
  if (!BWD) return;

  // coefficients of this lane group's pair, then of the pairs this lane's elements belong to
  const EuclidCoef mine = euclid_coef(T, g);
  EuclidCoef kr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r)                   // lane r*LPR leads pair r's lane group
    kr[r] = EuclidCoef{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.c), r * LPR)),
                       readlane_f64(mine.den, r * LPR), readlane_f64(mine.rcp, r * LPR)};
  float4* dq4 = reinterpret_cast<float4*>(dq) + base4;
  float4* da4 = reinterpret_cast<float4*>(da) + base4;
  // all NIT float4s as ONE straight-line block (their instruction chains interleave),
  // then a single wave-level branch for the rare exact re-computation
  float4 t[NIT];
  bool any_risky = false;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const EuclidCoef& k = (RW == 2 && i >= D4) ? kr[RW - 1] : kr[0];
    bool risky;
    t[it] = euclid_tt4_fast(k, df[it], risky);
    any_risky |= risky && (i < n4);
  }
  if (any_risky) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = lane + 64 * it;
      const EuclidCoef& k = (RW == 2 && i >= D4) ? kr[RW - 1] : kr[0];
      t[it] = euclid_tt4_exact(k, df[it]);
    }
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i >= n4) break;
    // dq = 0 + tt ; da = 0 + (-tt)   (:176-177 zero, :219-220 accumulate once)
    float4 o0, o1;
    o0.x = 0.f + t[it].x; o0.y = 0.f + t[it].y; o0.z = 0.f + t[it].z; o0.w = 0.f + t[it].w;
    o1.x = 0.f + (-t[it].x); o1.y = 0.f + (-t[it].y); o1.z = 0.f + (-t[it].z); o1.w = 0.f + (-t[it].w);
    stream_store(dq4 + i, o0);
    stream_store(da4 + i, o1);
  }
}

// p[i] as ONE 16-byte vector load that stays where it is written.  (A float4 is a struct: copying one out of a
// __restrict__ const array is a memcpy that the optimiser forwards to the first use of each member, i.e. the load is
// emitted THERE -- behind whatever was meant to run while it is in flight.)
template <typename I>
__device__ __forceinline__ float4 load4(const float4* p, I i) {
  const mms_v4f v = reinterpret_cast<const mms_v4f*>(p)[i];
  return make_float4(v.x, v.y, v.z, v.w);
}

// ---- the forward-only launch of euclid_pair32_kernel (below; its comment describes the algorithm) ----------
// One pass at two waves per SIMD with every wave in the same phase: whatever a wave executes between "its last byte
// has landed" and "T is stored" is exposed once per launch.  Same algorithm, same LDS image, same windows, same
// expressions on the same values as the kernel's shared body, so T keeps its bits; what differs is the order of
// issue, the waits and the predicates:
//  * all 2 * NIT operand loads leave first, in row order (slot 0 first), as unconditional vector loads of a clamped
//    column: a lane without a column in a slot reads column 0 of its row and neither writes nor sums the result
//    (left to the compiler, slot 0's loads sank into the lane-masked block of its LDS write, behind the other
//    slots' loads, with a wait for ALL loads inside the mask);
//  * slot `it` is subtracted, squared, written to the image and added to the window centres under a counted wait
//    that leaves the later slots in flight (vmcnt(4), (2), (0) at NIT = 3).  The squares are pinned in registers
//    ahead of the lane mask of the LDS write: the masked block then holds a DS write and no wait;
//  * a window centre is reduced across the half-wave as soon as the last slot that contributes to it is in
//    (D = 300: p1 after slot 0, p2 and with it the chain's start value after slot 1), under the loads still in
//    flight, instead of after the image is complete;
//  * the zero pad of the image is written while the loads are in flight, and the priority is raised before the
//    chain's reads, not after them;
//  * the chain starts on its first LDS read (SpecSegment::load_first / chain_streamed in euclid_math.h);
//  * FULL: every pair of the launch lies inside the batch and q and a span less than 4 GiB each (the host knows).
//    No clamp of the row, no `have` on the store of T, one 32-bit byte offset per slot off the two kernel
//    arguments (which arrive in SGPRs) instead of a 64-bit row pointer per operand.
template <int D4C, int WPB, bool SHIFT, bool FULL>
__device__ __forceinline__ void euclid_pair32_forward(int N, const float* __restrict__ q, const float* __restrict__ a,
                                                      float* __restrict__ top_out, float4* lds4) {
  constexpr int NIT = (D4C + 31) / 32;
  constexpr int H4 = (D4C + 2) / 3, ST4 = 3 * H4;
  constexpr int MAXU = SHIFT ? 7 : 0;            // largest peel at the start of a row
  // slot `it` holds columns [32*it - MAXU, 32*it + 31]: the last slot with a column of segment 0 / of segments 0-1
  constexpr int P1_LAST = (H4 + MAXU - 1) / 32 < NIT - 1 ? (H4 + MAXU - 1) / 32 : NIT - 1;
  constexpr int P2_LAST = (2 * H4 + MAXU - 1) / 32 < NIT - 1 ? (2 * H4 + MAXU - 1) / 32 : NIT - 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane >> 5, j = lane & 31;
  const int want = (blockIdx.x * WPB + wave) * 2 + grp;
  const bool have = FULL || want < N;            // (a wave past the end works on the last pair and stores nothing)
  const int row = have ? want : N - 1;
  const unsigned r0 = (unsigned)row * D4C;       // FULL: the row's first float4, as a 32-bit index
  const float4* q4 = reinterpret_cast<const float4*>(q) + (FULL ? 0 : (size_t)row * D4C);
  const float4* a4 = reinterpret_cast<const float4*>(a) + (FULL ? 0 : (size_t)row * D4C);
  const int u = !SHIFT ? 0
                : FULL ? (int)(((unsigned)(reinterpret_cast<size_t>(q) >> 4) + r0) & 7)
                       : (int)((reinterpret_cast<size_t>(q4) >> 4) & 7);
  const int j0 = j - u;
  const bool first_ok = !SHIFT || j0 >= 0;
  const bool last_ok = j0 + 32 * (NIT - 1) < D4C;
  auto valid_slot = [&](int it) { return (it > 0 || first_ok) && (it < NIT - 1 || last_ok); };

  float4 x[NIT], y[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = valid_slot(it) ? j0 + 32 * it : 0;   // clamp: the load is unconditional
    if constexpr (FULL) {
      const unsigned off = (r0 + (unsigned)i) * 16u;
      const char* qb = reinterpret_cast<const char*>(q4) + off;
      const char* ab = reinterpret_cast<const char*>(a4) + off;
      x[it] = load4(reinterpret_cast<const float4*>(qb), 0);
      y[it] = load4(reinterpret_cast<const float4*>(ab), 0);
    } else {
      x[it] = load4(q4, i);
      y[it] = load4(a4, i);
    }
    __builtin_amdgcn_sched_barrier(0);           // in row order, and every request before anything else
  }

  float4* img = lds4 + (wave * 2 + grp) * ST4;
  unsigned seg = lds_address(img + spec_seg32(j) * H4);   // this lane's segment of the chain,
  asm volatile("" : "+v"(seg));                            // addressed before the first wait
  if (ST4 > D4C && j < ST4 - D4C) img[D4C + j] = make_float4(0.f, 0.f, 0.f, 0.f);
  float p1 = 0.f, p2 = 0.f;
  float2v start = {0.f, 0.f};
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const bool valid = valid_slot(it);
    float4 s;
    s.x = x[it].x - y[it].x; s.y = x[it].y - y[it].y;
    s.z = x[it].z - y[it].z; s.w = x[it].w - y[it].w;
    s.x = s.x * s.x; s.y = s.y * s.y; s.z = s.z * s.z; s.w = s.w * s.w;
    asm volatile("" : "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w));   // in registers before the lane mask
    const int i = j0 + 32 * it;
    if (valid) img[i] = s;
    const float s4 = valid ? (s.x + s.y) + (s.z + s.w) : 0.f;
    // tree-sum contributions to the two window centres, as in the shared body
    if (32 * it + 31 < H4) p1 += s4;
    else if (32 * it - MAXU < H4) p1 += (i < H4) ? s4 : 0.f;
    if (32 * it + 31 < 2 * H4) p2 += s4;
    else if (32 * it - MAXU < 2 * H4) p2 += (i < 2 * H4) ? s4 : 0.f;
    if (it < NIT - 1) {                          // a centre that is complete is reduced under the loads in flight
      if (it == P1_LAST) p1 = half_wave_sum(p1);
      if (it == P2_LAST) {
        p2 = half_wave_sum(p2);
        start = spec_start32(p1, p2, j);
        asm volatile("" : "+v"(start));
      }
    }
    __builtin_amdgcn_sched_barrier(0);           // slot `it` is done before slot it + 1 is waited for
  }
  wave_lds_sync();
  __builtin_amdgcn_s_setprio(3);
  SpecSegment<H4> sg;
  sg.load_first(seg);                            // in flight while whatever is left of the centres is reduced
  if (P1_LAST == NIT - 1) p1 = half_wave_sum(p1);
  if (P2_LAST == NIT - 1) {
    p2 = half_wave_sum(p2);
    start = spec_start32(p1, p2, j);
  }
  const float2v end = sg.chain_streamed(seg, start);
  bool hit;
  float dist = spec_resolve_halves(start, end, j, &hit);
  if (!hit) {                                    // uniform per half; exact re-walk of this lane's pair
    dist = chain_sum_lds(img, ST4, 0.0f);
  }
  __builtin_amdgcn_s_setprio(0);
  const float T = 1.0f / (1.0f + sqrtf(dist));   // :106-107
  if (j == 0 && have) top_out[row] = T;
}

// ---- width-specialised wave-pair kernel (the headline configuration) ----------
// Same algorithm as euclid_rows_wave_kernel<.., RW = 2, ..> for D/4 = D4C known at
// compile time, with the layout made ROW-ALIGNED: lanes 0-31 own pair 2w, lanes
// 32-63 pair 2w+1, lane j holds float4s j, j+32, j+64 of its pair.  A lane then
// belongs to ONE pair for everything it does (loads, squares, speculation lane,
// coefficients, stores): no per-slot pair masks, no cross-lane broadcast of the
// coefficients, half-wave DPP sums, and every loop bound is a constant, so the
// chain is straight-line code.  About 40 % fewer wave-instructions than the
// generic kernel, which is what bounds this kernel.
//
// EXACT selects the arithmetic of the backward term tt = dT*T^3*(q-a)/(T-1+1e-9):
//   true : the reference's bits (fp32 product, DOUBLE divisor, one rounding to
//          float) through the checked reciprocal fast path of euclid_math.h;
//   false: fp32 throughout, tt = (c*(q-a)) * fl32(1/den): at most 2 ulp from the
//          reference's value (1.2e-7 relative against the 1e-5 bar), a third of
//          the instructions.  The FORWARD value T is bit-exact in both.
//
// SHIFT selects the LINE-ALIGNED lane map.  A row is D4C*16 bytes, no multiple of a 128-byte line at any of the
// three widths (1200 = 9*128 + 48), so a row starts u = (address >> 4) & 7 float4s into a line and each 16-lane
// quarter of a half-wave's 512-byte piece straddles three lines where two would do.  With SHIFT lane j, slot `it`
// holds float4 i = j + 32*it - u of its row: every quarter starts on a line.  A lane whose i falls outside
// [0, D4C) is idle (clamped load, no square, no store); 32*NIT - 7 >= D4C keeps the row covered.  Only the
// assignment of columns to lanes changes: the LDS image, the chain and its windows are indexed by i as before,
// and the tree sums p1 / p2 merely centre the windows, so T has the same bits.  The lane must hold the same
// column of every array it touches, so the host asks for SHIFT only when they are congruent mod 128
// (same_line_phase below); u is taken from q.
//
// The forward-only launch (FWD && !BWD) runs euclid_pair32_forward above; FULL is its whole-batch form.  The FWD
// parts of the body below serve the fused launch.
template <int D4C, bool FWD, bool BWD, bool EXACT, int WPB, bool SHIFT = false, bool FULL = false>
__global__ __launch_bounds__(64 * WPB) void euclid_pair32_kernel(
    int N, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_in, const float* __restrict__ top_diff,
    float* __restrict__ top_out, float* __restrict__ dq, float* __restrict__ da) {
  // N first: with -amdgpu-kernarg-preload-count the leading arguments arrive in SGPRs at wave
  // start, so the loads below do not wait on a scalar fetch of the argument block
  constexpr int NIT = (D4C + 31) / 32;
  constexpr int H4 = (D4C + 2) / 3, ST4 = 3 * H4;
  constexpr int MAXU = SHIFT ? 7 : 0;            // largest peel at the start of a row
  static_assert(32 * NIT - MAXU >= D4C, "the shifted slots must still cover the row");
  __shared__ float4 lds4[FWD ? WPB * 2 * ST4 : 1];
  static_assert(!FULL || (FWD && !BWD), "the whole-batch instantiation exists for the forward-only launch");
  if constexpr (FWD && !BWD) {
    euclid_pair32_forward<D4C, WPB, SHIFT, FULL>(N, q, a, top_out, lds4);
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = lane >> 5, j = lane & 31;
  // No early exit: a wave past the end works on the last pair and stores nothing, so that no
  // branch (and no wait on the kernel arguments) stands between wave start and the loads.
  const int want = (blockIdx.x * WPB + wave) * 2 + grp;
  const bool have = want < N;
  const int row = have ? want : N - 1;
  const float4* q4 = reinterpret_cast<const float4*>(q) + (size_t)row * D4C;
  const float4* a4 = reinterpret_cast<const float4*>(a) + (size_t)row * D4C;
  // column of slot `it`, and whether this lane has one there: only the first slot can start before the row
  // (SHIFT) and only the last can run past its end
  const int j0 = SHIFT ? j - (int)((reinterpret_cast<size_t>(q4) >> 4) & 7) : j;
  const bool first_ok = !SHIFT || j0 >= 0;
  const bool last_ok = j0 + 32 * (NIT - 1) < D4C;
  auto valid_slot = [&](int it) { return (it > 0 || first_ok) && (it < NIT - 1 || last_ok); };

  float T = 0.f;
  if (!FWD) T = top_in[row];
  float g = 0.f;
  if (BWD) g = top_diff[row];
  float4 x[NIT], y[NIT], df[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = valid_slot(it) ? j0 + 32 * it : 0;   // clamp: keep the load unconditional
    x[it] = q4[i];
    y[it] = a4[i];
  }

  float p1 = 0.f, p2 = 0.f;
  float4* img = lds4 + (wave * 2 + grp) * ST4;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    df[it].x = x[it].x - y[it].x; df[it].y = x[it].y - y[it].y;
    df[it].z = x[it].z - y[it].z; df[it].w = x[it].w - y[it].w;
    if (FWD) {
      const bool valid = valid_slot(it);
      float4 s;
      s.x = df[it].x * df[it].x; s.y = df[it].y * df[it].y;
      s.z = df[it].z * df[it].z; s.w = df[it].w * df[it].w;
      const int i = j0 + 32 * it;
      if (valid) img[i] = s;
      const float s4 = valid ? (s.x + s.y) + (s.z + s.w) : 0.f;
      // tree-sum contributions to the two window centres (segment 0; segments 0-1); the slot's columns
      // lie in [32*it - MAXU, 32*it + 31]
      if (32 * it + 31 < H4) p1 += s4;
      else if (32 * it - MAXU < H4) p1 += (i < H4) ? s4 : 0.f;
      if (32 * it + 31 < 2 * H4) p2 += s4;
      else if (32 * it - MAXU < 2 * H4) p2 += (i < 2 * H4) ? s4 : 0.f;
    }
  }
  if (FWD) {
    if (ST4 > D4C && j < ST4 - D4C) img[D4C + j] = make_float4(0.f, 0.f, 0.f, 0.f);
    wave_lds_sync();
    SpecSegment<H4> sg;
    sg.load(img + spec_seg32(j) * H4);          // in flight while the window centres are reduced
    p1 = half_wave_sum(p1);
    p2 = half_wave_sum(p2);
    __builtin_amdgcn_s_setprio(3);
    const float2v start = spec_start32(p1, p2, j);
    const float2v end = sg.chain(start);
    bool hit;
    float dist = spec_resolve_halves(start, end, j, &hit);
    if (!hit) {                                 // uniform per half; exact re-walk of this lane's pair
      dist = chain_sum_lds(img, ST4, 0.0f);
    }
    __builtin_amdgcn_s_setprio(0);
    T = 1.0f / (1.0f + sqrtf(dist));            // :106-107
    // g is pinned as "in a register" HERE, before the store of T: left to the compiler, its first use came
    // after that store (issued under a lane mask, so the wait could not be counted) and every wave sat in
    // s_waitcnt vmcnt(0) until the store was acknowledged
    if (BWD) asm volatile("" : "+v"(g));
    if (j == 0 && have) top_out[row] = T;
  }
  if (!BWD) return;

  float4* dq4 = reinterpret_cast<float4*>(dq) + (size_t)row * D4C;
  float4* da4 = reinterpret_cast<float4*>(da) + (size_t)row * D4C;
  if (!FWD) {                                   // all requests landed before the first store (see euclid_block_kernel)
    asm volatile("" : "+v"(T), "+v"(g));
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      asm volatile("" : "+v"(df[it].x), "+v"(df[it].y), "+v"(df[it].z), "+v"(df[it].w));
  }
  float4 t[NIT];
  if (EXACT) {
    const EuclidCoef k = euclid_coef(T, g);
    bool any_risky = false;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      bool risky;
      t[it] = euclid_tt4_fast(k, df[it], risky);
      any_risky |= risky && valid_slot(it);
    }
    if (any_risky) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) t[it] = euclid_tt4_exact(k, df[it]);
    }
  } else {
    const float c = g * T * T * T;
    const float r = (float)rcp_newton((double)(T - 1.0f) + 1e-9);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      t[it].x = (c * df[it].x) * r; t[it].y = (c * df[it].y) * r;
      t[it].z = (c * df[it].z) * r; t[it].w = (c * df[it].w) * r;
    }
  }
  if (have) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (!valid_slot(it)) continue;
    // dq = 0 + tt ; da = 0 + (-tt)   (:176-177 zero, :219-220 accumulate once)
    float4 o0, o1;
    o0.x = 0.f + t[it].x; o0.y = 0.f + t[it].y; o0.z = 0.f + t[it].z; o0.w = 0.f + t[it].w;
    o1.x = 0.f + (-t[it].x); o1.y = 0.f + (-t[it].y); o1.z = 0.f + (-t[it].z); o1.w = 0.f + (-t[it].w);
    stream_store(dq4 + j0 + 32 * it, o0);
    stream_store(da4 + j0 + 32 * it, o1);
  }
  }
}

// What a backward-only launch of euclid_block_kernel keeps per slot once T and dT of the slot's pair have landed:
// c = dT*T*T*T and r = fl32(1/den) in the fp32 arithmetic, the reference mode's coefficient set otherwise.
template <bool EXACT> struct SlotCoef { float c, r; };
template <> struct SlotCoef<true> { EuclidCoef k; };

// ---- the same algorithm with the global-memory side laid out by WORKGROUP, not by pair ----------
// Measured (tools/launchbench.hip, profiles/r02_launchbench.txt): HBM-cold, a launch whose waves each read
// two 512-byte pieces 1200 bytes apart per load instruction (the row-aligned layout above) takes 4.4 us for
// q and a of cfg 2, a launch whose workgroup reads its rows as ONE dense run (instruction `it` of all its
// waves covers a contiguous span) takes 3.6 us -- the speed of a flat one-float4-per-thread read; the
// write side behaves the same (6.5 vs 5.5 us for a backward-shaped launch).  What costs is the order in
// which a CU's requests reach a DRAM page: three visits at different times against one.
// So: a workgroup of WPB waves owns R = 2*WPB consecutive pairs = C = R*D4C consecutive float4 of q and of
// a; thread t loads float4s t, t+T, t+2T ... of that run (and stores dq / da the same way).  The squares
// go to LDS at (pair, column) -- the image layout the chain wants -- and after ONE workgroup barrier each
// half-wave walks its pair's chain exactly as in euclid_pair32_kernel (same predictions, same windows,
// same bits).  A thread's float4s belong to whatever pairs they fall in, so the backward reads T (and the
// per-pair coefficients) by pair index: from LDS when this launch computed T, from top_in otherwise -- a
// backward-only launch has no LDS traffic and no barrier at all.
// SPAN = waves that share one dense run: WPB (the whole workgroup, one barrier) or 1 (each wave reads its own two
// rows as a dense run and synchronises with nobody: the chain phases of a CU's waves then start as their own data
// arrives instead of all at once).
//
// The BACKWARD-ONLY launch (!FWD && BWD) is one pass at two waves per SIMD with every wave in the same phase, so
// whatever a wave executes between "its last byte has landed" and "its last store is issued" is exposed once per
// launch.  Two things keep that stretch short:
//  * T and dT of a thread's slots are requested BEFORE the operands (vmcnt retires in order: they are usable while
//    the six 16-byte loads are still in flight) and everything that depends on them alone -- c = dT*T*T*T and the
//    fp64 reciprocal chain of the divisor, or the reference mode's EuclidCoef -- is formed and pinned in registers
//    under a counted wait that leaves the operand loads outstanding.  Same expressions on the same values: the
//    gradients keep their bits.
//  * FULL: every run of the launch lies inside the batch (the host knows: N a multiple of the pairs per workgroup).
//    No end-of-batch clamp on any address, no lane mask on any store but the compile-time i < C of the last slot,
//    32-bit index math off one 64-bit base per run.  With the stores unmasked the compiler counts vmcnt per slot:
//    slot `it`'s two stores leave as soon as its own operands are in.
template <int D4C, bool FWD, bool BWD, bool EXACT, int WPB, int SPAN = WPB, bool FULL = false>
__global__ __launch_bounds__(64 * WPB) void euclid_block_kernel(
    int N, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_in, const float* __restrict__ top_diff,
    float* __restrict__ top_out, float* __restrict__ dq, float* __restrict__ da) {
  static_assert(SPAN == WPB || SPAN == 1, "a dense run belongs to the workgroup or to one wave");
  constexpr bool BONLY = !FWD && BWD;                        // the backward-only launch
  static_assert(!FULL || BONLY, "the whole-batch instantiation exists for the backward-only launch");
  constexpr int T = 64 * SPAN, R = 2 * SPAN, C = R * D4C;
  constexpr int NSPAN = WPB / SPAN;                          // runs per workgroup
  constexpr int NIT = (C + T - 1) / T;                       // float4s per operand per thread
  constexpr int PNIT = (D4C + 31) / 32, LASTN = D4C - 32 * (PNIT - 1);
  constexpr int H4 = (D4C + 2) / 3, ST4 = 3 * H4;
  __shared__ float4 lds4_all[FWD ? NSPAN * R * ST4 : 1];
  __shared__ float Tl_all[(FWD && BWD) ? NSPAN * R : 1];
  const int span = (SPAN == WPB) ? 0 : (int)(threadIdx.x >> 6);
  const int tid = (SPAN == WPB) ? (int)threadIdx.x : (int)(threadIdx.x & 63);
  float4* lds4 = lds4_all + (FWD ? span * R * ST4 : 0);
  float* Tl = Tl_all + ((FWD && BWD) ? span * R : 0);
  const long long run = (long long)blockIdx.x * NSPAN + span;   // index of this dense run
  const long long total4 = (long long)N * D4C;
  const long long b = run * C;
  const float4* q4 = reinterpret_cast<const float4*>(q);
  const float4* a4 = reinterpret_cast<const float4*>(a);

  // slot `it` holds float4 i of the run: only the last slot can fall past its end (T * (NIT - 1) < C), so in the
  // backward-only launch the test folds away for every other slot once the loops are unrolled (the forward
  // instantiations keep the test they had, and with it their code)
  auto in_run = [](int it, int i) { return NIT * T == C || (BONLY && it < NIT - 1) || i < C; };
  // per-float4 pair values (dT; T too in a backward-only launch, which requests them ahead of the operands)
  float Tg[NIT], gg[NIT];
  auto request_pair_values = [&] {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + T * it;
      const int pr = (in_run(it, i) ? i : 0) / D4C;             // pair within the run
      if constexpr (FULL) {
        gg[it] = (top_diff + run * R)[pr];
        Tg[it] = (top_in + run * R)[pr];
      } else {
        long long row = run * R + pr;
        row = row < N ? row : N - 1;
        gg[it] = top_diff[row];
        if (!FWD) Tg[it] = top_in[row];
      }
    }
  };
  if constexpr (BONLY) request_pair_values();
  float4 x[NIT], y[NIT], df[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + T * it;
    const int ci = in_run(it, i) ? i : 0;                     // clamp: keep the load unconditional
    if constexpr (FULL) {
      x[it] = load4(q4 + b, ci);
      y[it] = load4(a4 + b, ci);
    } else {
      long long gi = b + ci;
      gi = gi < total4 ? gi : total4 - 1;                     // a run past the end reads the last float4
      // (load4 only where something is meant to run under the loads: the forward instantiations keep their code)
      x[it] = BONLY ? load4(q4, gi) : q4[gi];
      y[it] = BONLY ? load4(a4, gi) : a4[gi];
    }
  }
  if constexpr (BWD && !BONLY) request_pair_values();
  if constexpr (BONLY) __builtin_amdgcn_sched_barrier(0);    // every request is issued before the first wait
  // backward-only launch: the per-slot coefficients, formed while the operands are in flight and pinned so that
  // they cannot sink behind the operand wait
  SlotCoef<EXACT> coef[BONLY ? NIT : 1];                     // (no other launch has any)
  if constexpr (BONLY) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if constexpr (EXACT) {
        coef[it].k = euclid_coef(Tg[it], gg[it]);
        asm volatile("" : "+v"(coef[it].k.c), "+v"(coef[it].k.den), "+v"(coef[it].k.rcp));
      } else {
        coef[it].c = gg[it] * Tg[it] * Tg[it] * Tg[it];
        coef[it].r = (float)rcp_newton((double)(Tg[it] - 1.0f) + 1e-9);
        asm volatile("" : "+v"(coef[it].c), "+v"(coef[it].r));
      }
    }
    __builtin_amdgcn_sched_barrier(0);                       // ... and no operand's first use is hoisted into them
  }
  auto subtract = [&](int it) {
    df[it].x = x[it].x - y[it].x; df[it].y = x[it].y - y[it].y;
    df[it].z = x[it].z - y[it].z; df[it].w = x[it].w - y[it].w;
  };
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if constexpr (!FULL) subtract(it);                      // FULL: slot by slot, next to the slot's stores
    if (FWD) {
      const int i = tid + T * it;
      float4 s;
      s.x = df[it].x * df[it].x; s.y = df[it].y * df[it].y;
      s.z = df[it].z * df[it].z; s.w = df[it].w * df[it].w;
      if (in_run(it, i)) lds4[(ST4 == D4C) ? i : (i / D4C) * ST4 + (i % D4C)] = s;
    }
  }
  if (FWD) {
    if constexpr (ST4 > D4C) {                              // zero tail of each image
      if (tid < R * (ST4 - D4C))
        lds4[(tid / (ST4 - D4C)) * ST4 + D4C + tid % (ST4 - D4C)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (SPAN == WPB) __syncthreads(); else wave_lds_sync();
    const int wave = tid >> 6, lane = tid & 63;
    const int grp = lane >> 5, j = lane & 31;
    const int lp = wave * 2 + grp;
    const long long row = run * R + lp;
    const bool have = row < N;
    const float4* img = lds4 + lp * ST4;
    SpecSegment<H4> sg;
    sg.load(img + spec_seg32(j) * H4);          // in flight while the window centres are formed
    // tree-sum contributions to the two window centres (segment 0; segments 0-1): the same per-lane
    // terms and the same reduction as euclid_pair32_kernel, read back from the image
    const bool last_ok = (LASTN >= 32) || (j < LASTN);
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int it = 0; it < PNIT; ++it) {
      const bool valid = (it < PNIT - 1) || last_ok;
      const float4 s = img[valid ? j + 32 * it : 0];
      const float s4 = valid ? (s.x + s.y) + (s.z + s.w) : 0.f;
      const int i = j + 32 * it;
      if (32 * it + 31 < H4) p1 += s4;
      else if (32 * it < H4) p1 += (i < H4) ? s4 : 0.f;
      if (32 * it + 31 < 2 * H4) p2 += s4;
      else if (32 * it < 2 * H4) p2 += (i < 2 * H4) ? s4 : 0.f;
    }
    p1 = half_wave_sum(p1);
    p2 = half_wave_sum(p2);
    __builtin_amdgcn_s_setprio(3);
    const float2v start = spec_start32(p1, p2, j);
    const float2v end = sg.chain(start);
    bool hit;
    float dist = spec_resolve_halves(start, end, j, &hit);
    if (!hit) {                                 // uniform per half; exact re-walk of this lane's pair
      dist = chain_sum_lds(img, ST4, 0.0f);
    }
    __builtin_amdgcn_s_setprio(0);
    const float Tp = 1.0f / (1.0f + sqrtf(dist));            // :106-107
    if (BWD) {                                  // in registers before the store of T (see euclid_pair32_kernel)
#pragma unroll
      for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(gg[it]));
    }
    if (j == 0) {
      if (have) top_out[row] = Tp;
      if (BWD) Tl[lp] = Tp;
    }
    if (BWD) { if (SPAN == WPB) __syncthreads(); else wave_lds_sync(); }
  }
  if (!BWD) return;

  float4* dq4 = reinterpret_cast<float4*>(dq);
  float4* da4 = reinterpret_cast<float4*>(da);
  if constexpr (BONLY && !FULL) {
    // Everything this thread requested is in registers before its first store.  The stores sit under lane masks
    // (the end of the batch), so the compiler cannot count them: a load consumed after a store became
    // s_waitcnt vmcnt(0), i.e. a wait for the ACKNOWLEDGEMENT of the stores already issued -- in the middle of
    // the store phase of the launch that bounds the headline.  (The pair values were consumed above; FULL has no
    // masked store before its last slot and needs none of this.)
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      asm volatile("" : "+v"(df[it].x), "+v"(df[it].y), "+v"(df[it].z), "+v"(df[it].w));
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + T * it;
    const bool live = in_run(it, i) && (FULL || b + i < total4);
    if constexpr (FULL) subtract(it);
    if constexpr (FULL && NIT * T != C) {
      // the last slot's stores are masked: its operands are waited for (counted: only stores are younger) out here,
      // so that neither the wait nor the loads can move into the masked block
      if (it == NIT - 1) asm volatile("" : "+v"(df[it].x), "+v"(df[it].y), "+v"(df[it].z), "+v"(df[it].w));
    }
    float4 t;
    if constexpr (BONLY) {
      if constexpr (EXACT) {
        t = euclid_tt4(coef[it].k, df[it]);
      } else {
        const float c = coef[it].c, r = coef[it].r;
        t.x = (c * df[it].x) * r; t.y = (c * df[it].y) * r;
        t.z = (c * df[it].z) * r; t.w = (c * df[it].w) * r;
      }
    } else {
      const float Tp = Tl[(in_run(it, i) ? i : 0) / D4C];
      if (EXACT) {
        const EuclidCoef k = euclid_coef(Tp, gg[it]);
        t = euclid_tt4(k, df[it]);
      } else {
        const float c = gg[it] * Tp * Tp * Tp;
        const float r = (float)rcp_newton((double)(Tp - 1.0f) + 1e-9);
        t.x = (c * df[it].x) * r; t.y = (c * df[it].y) * r;
        t.z = (c * df[it].z) * r; t.w = (c * df[it].w) * r;
      }
    }
    if (live) {
      // dq = 0 + tt ; da = 0 + (-tt)   (:176-177 zero, :219-220 accumulate once)
      float4 o0, o1;
      o0.x = 0.f + t.x; o0.y = 0.f + t.y; o0.z = 0.f + t.z; o0.w = 0.f + t.w;
      o1.x = 0.f + (-t.x); o1.y = 0.f + (-t.y); o1.z = 0.f + (-t.z); o1.w = 0.f + (-t.w);
      stream_store(dq4 + b + i, o0);
      stream_store(da4 + b + i, o1);
    }
    if constexpr (FULL) __builtin_amdgcn_sched_barrier(0);   // slot `it` is stored before slot it + 1 is waited for
  }
}

// ---- generic fallback (any D, any alignment): workgroup of ROWS pairs --------
// Forward (BWD=false) or forward+backward (BWD=true) for W1=W2=1, Euclidean.
// LDS: diff[ROWS*D] floats (dynamic) + per-row coefficient slots.
template <int ROWS, int THREADS, bool BWD>
__global__ __launch_bounds__(THREADS) void euclid_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_diff, float* __restrict__ top,
    float* __restrict__ dq, float* __restrict__ da, int N, int D) {
  extern __shared__ float4 lds_raw[];
  float* diff = reinterpret_cast<float*>(lds_raw);
  __shared__ float cs[ROWS];
  __shared__ double dens[ROWS];

  const int row0 = blockIdx.x * ROWS;
  const int rows = min(ROWS, N - row0);
  const size_t base = (size_t)row0 * D;
  const int total = rows * D;

  for (int i = threadIdx.x; i < total; i += THREADS) diff[i] = q[base + i] - a[base + i];
  __syncthreads();

  // One lane per pair: the reference's d-ascending fp32 chain (:100-106).
  if (threadIdx.x < rows) {
    const float* r = diff + threadIdx.x * D;
    float dist = 0.f;
    for (int d = 0; d < D; ++d) dist += r[d] * r[d];
    dist = sqrtf(dist);
    const float T = 1.0f / (1.0f + dist);
    top[row0 + threadIdx.x] = T;
    if (BWD) {
      const EuclidCoef k = euclid_coef(T, top_diff[row0 + threadIdx.x]);
      cs[threadIdx.x] = k.c;
      dens[threadIdx.x] = k.den;
    }
  }
  if (!BWD) return;
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int r = i / D;
    const float t = euclid_tt_exact(cs[r], dens[r], diff[i]);
    dq[base + i] = 0.f + t;
    da[base + i] = 0.f + (-t);
  }
}

// Backward alone, generic fallback: pure streaming.
__global__ __launch_bounds__(256) void euclid_rows_bwd_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top, const float* __restrict__ top_diff,
    float* __restrict__ dq, float* __restrict__ da, int total, int D) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int r = i / D;
    const EuclidCoef k = euclid_coef(top[r], top_diff[r]);
    const float t = euclid_tt_exact(k.c, k.den, q[i] - a[i]);
    dq[i] = 0.f + t;
    da[i] = 0.f + (-t);
  }
}

// ================================= dispatch =================================
// DESIGN.md 4.4b is the table this section is read against.

// Backward arithmetic of the Euclidean term (include/mms.h: mms_set_euclid_backward_mode).  The mode
// belongs to the calling thread (Caffe drives each GPU from its own thread); a thread that never set it
// takes the process default from the environment.
static std::atomic<int> g_euclid_bwd_default{-1};
static thread_local int t_euclid_bwd_mode = -1;
int euclid_backward_mode() {
  if (t_euclid_bwd_mode >= 0) return t_euclid_bwd_mode;
  int m = g_euclid_bwd_default.load(std::memory_order_relaxed);
  if (m < 0) {
    const char* e = std::getenv("MMS_EUCLID_BWD");
    m = (e && (!std::strcmp(e, "reference") || !std::strcmp(e, "exact") || !std::strcmp(e, "1")))
            ? MMS_EUCLID_BWD_REFERENCE : MMS_EUCLID_BWD_FP32;
    g_euclid_bwd_default.store(m, std::memory_order_relaxed);
  }
  return m;
}
void set_euclid_backward_mode(int m) { t_euclid_bwd_mode = m; }

constexpr int kRows = 8;       // pairs per workgroup in the generic rows kernels
constexpr int kRowsThreads = 256;

// The line-aligned lane map of euclid_pair32_kernel (SHIFT) gives a lane the column that sits at the same place
// of a 128-byte line in every array, so it serves a launch only when all the arrays it touches (as in vec4_ok)
// start at the same offset within a line.  Allocator-aligned blobs do; views carved at unrelated offsets get
// the unshifted map.
static bool same_line_phase(const void* p0, const void* p1, const void* p2, const void* p3) {
  const auto ph = [](const void* p) { return reinterpret_cast<uintptr_t>(p) & 127; };
  return ph(p1) == ph(p0) && (!p2 || ph(p2) == ph(p0)) && (!p3 || ph(p3) == ph(p0));
}

// generic rows kernels: LDS needed; the forward falls back to the cross kernels above ~64 KB.
static size_t rows_lds_bytes(int D) { return (size_t)kRows * D * sizeof(float); }
static bool rows_fit(int D) { return rows_lds_bytes(D) <= 64 * 1024; }

// Which kernel family serves a launch, from D and the arrays it touches (dq, da null in a forward).
enum class EuclidRows { kPair32, kWave, kGeneric, kNone };
static EuclidRows euclid_rows_route(int D, const void* q, const void* a, const void* dq, const void* da) {
  if (vec4_ok(D, q, a, dq, da) && wave_width_ok(D)) return glove_width(D) ? EuclidRows::kPair32 : EuclidRows::kWave;
  return rows_fit(D) ? EuclidRows::kGeneric : EuclidRows::kNone;
}

// Eight waves (16 pairs) per workgroup: N = 4096 is then 256 workgroups, one per CU, two waves
// per SIMD -- measured 3 % faster HBM-cold than 512 workgroups of four waves (dispatch ramp).
template <bool FWD, bool BWD>
static void launch_pair32(const float* q, const float* a, const float* top_in, const float* top_diff,
                          float* top_out, float* dq, float* da, int N, int D, bool exact, hipStream_t s) {
  constexpr int WPB = 8;
  const unsigned grid = (unsigned)((N + 2 * WPB - 1) / (2 * WPB));
  // Which global-memory layout (same results bit for bit; tests/test_gpu_parity.py runs both for every kind
  // of launch).  Measured at cfg 2, HBM-cold, graph-replayed (tools/layoutab.sh, profiles/r02_layout_ab.txt):
  //   backward-only launch      row-aligned 6.27 us, workgroup-dense 4.87 us  -> dense
  //   forward-only launch       4.87 vs 4.92 us: the chain's tail, not the read pattern, bounds it -> row-aligned
  //   fused forward+backward    5.65 vs 6.0 us: waves free of workgroup barriers spread the store phase -> row-aligned
  //   Forward launch then Backward launch (what a Net issues): 8.80 us both row-aligned -> 7.97 us forward
  //   row-aligned + backward dense.  Both must map workgroup b to the SAME pairs (same waves per workgroup):
  //   the backward then finds q and a in the L2 of the XCD that read them in the forward; mismatched maps cost
  //   0.6 us.
  // The row-aligned kernel's lane map is LINE-ALIGNED when the launch's arrays are congruent mod 128
  // (same_line_phase; euclid_pair32_kernel's SHIFT).  Probe (tools/launchbench.hip,
  // profiles/launchbench_lane_map.txt): the bare read of q and a in the row-aligned map 4.43 us, line-aligned
  // 4.13 us, dense 3.59-3.68 us, at the same bytes and the same L1-to-L2 read requests (one per line either
  // way) but 24 % fewer L1 line accesses: a 16-lane quarter that starts mid-line looks up three lines, one
  // that starts on a line two.  The figures above predate the map; with it the Forward launch + dense Backward
  // launch of bench.py went 7.50 -> 7.22 us per step, and with the dense Backward's coefficients formed ahead of
  // its operands and its whole-batch instantiation (euclid_block_kernel's FULL, selected below) 7.28 -> 7.03
  // (profiles/bwd_coef_first_*); with the forward-only launch's own body (euclid_pair32_forward: loads first in row
  // order, counted waits per slot, window centres reduced under the loads, the chain started on its first LDS read,
  // whole-batch instantiation) 7.06 / 7.01 -> 6.94 (profiles/fwd_tail_*).
  // Dev switch for A/B timing: MMS_EUCLID_LAYOUT_{FWD,BWD,FUSED} = pair | block | wave (dense run per wave).
  static const int layout = [] {
    const char* e = std::getenv(FWD && BWD ? "MMS_EUCLID_LAYOUT_FUSED" : FWD ? "MMS_EUCLID_LAYOUT_FWD" : "MMS_EUCLID_LAYOUT_BWD");
    if (e) return !std::strcmp(e, "pair") ? 0 : (!std::strcmp(e, "wave") ? 2 : 1);
    return FWD ? 0 : 1;
  }();
  const bool shift = same_line_phase(q, a, BWD ? dq : nullptr, BWD ? da : nullptr);
  // Every workgroup's pairs lie inside the batch: the backward-only dense kernel then runs without end-of-batch
  // clamps and store masks (euclid_block_kernel's FULL; a workgroup owns 2 * WPB pairs whatever its SPAN).
  constexpr bool BONLY = !FWD && BWD;
  const bool full = BONLY && N % (2 * WPB) == 0;
  // The same promise to the forward-only row-aligned kernel (euclid_pair32_forward's FULL), which also forms its
  // addresses from 32-bit byte offsets: q and a span less than 4 GiB each.
  constexpr bool FONLY = FWD && !BWD;
  const bool full_fwd = FONLY && N % (2 * WPB) == 0 && (unsigned long long)N * D * sizeof(float) <= 0xffffffffull;
  with_glove_d4(D, [&](auto W) {
    constexpr int D4C = decltype(W)::value;
    with_bool(BWD && exact, [&](auto E) {   // a forward has no backward term: its EXACT is false
      constexpr bool EXACT = decltype(E)::value;
      hipLaunchKernelGGL((layout == 0   ? (full_fwd ? (shift ? euclid_pair32_kernel<D4C, FWD, BWD, EXACT, WPB, true, FONLY>
                                                             : euclid_pair32_kernel<D4C, FWD, BWD, EXACT, WPB, false, FONLY>)
                                                    : (shift ? euclid_pair32_kernel<D4C, FWD, BWD, EXACT, WPB, true>
                                                             : euclid_pair32_kernel<D4C, FWD, BWD, EXACT, WPB>))
                          : layout == 1 ? (full ? euclid_block_kernel<D4C, FWD, BWD, EXACT, WPB, WPB, BONLY>
                                                : euclid_block_kernel<D4C, FWD, BWD, EXACT, WPB>)
                                        : (full ? euclid_block_kernel<D4C, FWD, BWD, EXACT, WPB, 1, BONLY>
                                                : euclid_block_kernel<D4C, FWD, BWD, EXACT, WPB, 1>)),
                         dim3(grid), dim3(64 * WPB), 0, s, N, q, a, top_in, top_diff, top_out, dq, da);
    });
  });
}

// wave kernel: RW = wave_pairs(D) pairs per wave, NIT = ceil(RW*D/4 / 64) 16-byte loads per operand per lane
// (1..4 for every D that euclid_rows_route sends here).
template <bool FWD, bool BWD>
static void launch_rows_wave(const float* q, const float* a, const float* top_in,
                             const float* top_diff, float* top_out, float* dq, float* da, int N,
                             int D, hipStream_t s) {
  const int D4 = D / 4;
  const int rw = wave_pairs(D), nit = (rw * D4 + 63) / 64;
  const unsigned grid = (unsigned)((N + 4 * rw - 1) / (4 * rw));
  const size_t lds = FWD ? spec_image_lds(4, rw, D4) : 0;
  static constexpr decltype(&euclid_rows_wave_kernel<1, 1, FWD, BWD>) kernels[2][4] = {
      MMS_NIT4(euclid_rows_wave_kernel, 1, FWD, BWD), MMS_NIT4(euclid_rows_wave_kernel, 2, FWD, BWD)};
  hipLaunchKernelGGL(kernels[rw - 1][nit - 1], dim3(grid), dim3(256), lds, s, q, a, top_in, top_diff, top_out,
                     dq, da, N, D4);
}

// Euclid, W1 = W2 = 1.  false: no rows kernel serves this forward (or fused) launch and the caller's word-grid
// kernels take it; a backward alone is always served (euclid_rows_bwd_kernel streams at any D).
template <bool FWD, bool BWD>
bool launch_euclid_rows(int N, int D, const float* q, const float* a, const float* top_in, const float* top_diff,
                        float* top_out, float* dq, float* da, bool exact, hipStream_t s) {
  const EuclidRows route = euclid_rows_route(D, q, a, dq, da);
  if (route == EuclidRows::kPair32) {
    launch_pair32<FWD, BWD>(q, a, top_in, top_diff, top_out, dq, da, N, D, exact, s);
  } else if (route == EuclidRows::kWave) {
    launch_rows_wave<FWD, BWD>(q, a, top_in, top_diff, top_out, dq, da, N, D, s);
  } else if (!FWD) {
    const int total = N * D;
    int blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(euclid_rows_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q, a, top_in, top_diff,
                       dq, da, total, D);
  } else if (route == EuclidRows::kGeneric) {
    hipLaunchKernelGGL((euclid_rows_kernel<kRows, kRowsThreads, BWD>), dim3((unsigned)((N + kRows - 1) / kRows)),
                       dim3(kRowsThreads), rows_lds_bytes(D), s, q, a, top_diff, top_out, dq, da, N, D);
  } else {
    return false;
  }
  return true;
}

#define MMS_ROWS_INSTANCE(F, B)                                                                                   \
  template bool launch_euclid_rows<F, B>(int, int, const float*, const float*, const float*, const float*, float*, \
                                         float*, float*, bool, hipStream_t);
MMS_ROWS_INSTANCE(true, false) MMS_ROWS_INSTANCE(false, true) MMS_ROWS_INSTANCE(true, true)
#undef MMS_ROWS_INSTANCE

}  // namespace mms
