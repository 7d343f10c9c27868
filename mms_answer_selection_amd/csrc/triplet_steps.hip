// csrc/triplet_steps.hip -- the fused (q, a+, a-) training steps, Euclid and cosine, for gfx950: two SimCross,
// PairRankLoss on the two score columns and the whole backward in one launch, the loss scalar reduced inside that
// launch where the width-specialised kernels serve (LossArrival), by triplet_loss_from_terms (pairrank.hip) otherwise.
#include <cmath>
#include <cstdint>

#include "cosine_math.h"
#include "euclid_math.h"
#include "pairrank_math.h"
#include "mms_internal.h"

namespace mms {

constexpr int kTicketTop = 1024;      // words 0..1023 of a ticket slot: one per group of kTicketGroup workgroups; then the top word
constexpr int kTicketStride = kTicketTop + 32;
constexpr int kTicketGroup = 16;
// An arrival word carries the arrivals AND what arrived, so that ONE atomic both hands over a partial loss
// and tells its issuer whether it was the last: [63] poison, [52..62] arrivals, [0..51] sum of the terms in
// units of 2^-S (S chosen by the host from N so that the field cannot overflow while every term < 2^kFxTermBits).
constexpr int kFxSumBits = 52;
constexpr int kFxTermBits = 10;
constexpr unsigned long long kFxPoison = 1ull << 63;
constexpr unsigned long long kFxOne = 1ull << kFxSumBits;
constexpr unsigned long long kFxSumMask = kFxOne - 1;

static thread_local int t_triplet_finish = MMS_TRIPLET_FINISH_INLAUNCH;
int triplet_finish_mode() { return t_triplet_finish; }
void set_triplet_finish_mode(int m) { t_triplet_finish = m; }

// ======================= fused (q, a+, a-) training step =====================
// In-launch loss sum of the width-specialised fused steps (Euclid and cosine): see "loss scalar" in
// triplet32x2_kernel for the scheme and its measurements.  A wave's terms are added to (fx_sum, fx_bad) by every
// lane alike; lane 0 then calls arrive() ONCE per wave, every wave of the launch, and finish() after its stores.
struct LossArrival {
  unsigned long long fx_sum = 0, fx_bad = 0;
  bool top_wait = false;
  unsigned long long top_old = 0, top_pay = 0;
  __device__ __forceinline__ void add(float tm, double fx_scale) {
    const bool ok = tm >= 0.f && tm < (float)(1 << kFxTermBits);
    fx_sum += ok ? (unsigned long long)((double)tm * fx_scale) : 0ull;
    fx_bad += ok ? 0ull : 1ull;
  }
  template <int WPB>
  __device__ __forceinline__ void arrive(unsigned long long* wg_arrivals, unsigned long long* __restrict__ ticket) {
    const unsigned long long pay = (1ull << 60) | (fx_bad ? kFxOne : 0ull) | fx_sum;
    const unsigned long long old = __hip_atomic_fetch_add(wg_arrivals, pay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if ((old >> 60) == (unsigned long long)(WPB - 1)) {
      const unsigned long long wg = old + pay;
      const unsigned grp = blockIdx.x / kTicketGroup;
      const unsigned gsize = min((unsigned)kTicketGroup, gridDim.x - (unsigned)kTicketGroup * grp);
      const unsigned long long gpay = kFxOne | (wg & kFxSumMask);
      if ((wg >> kFxSumBits) & 0xffull)
        __hip_atomic_fetch_or(ticket + grp, kFxPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long gold = __hip_atomic_fetch_add(ticket + grp, gpay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (((gold >> kFxSumBits) & 0x7ffull) == (unsigned long long)(gsize - 1)) {
        const unsigned long long g = gold + gpay;
        __hip_atomic_store(ticket + grp, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        top_pay = kFxOne | (g & kFxSumMask);
        if (g & kFxPoison) __hip_atomic_fetch_or(ticket + kTicketTop, kFxPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        top_old = __hip_atomic_fetch_add(ticket + kTicketTop, top_pay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        top_wait = true;
      }
    }
  }
  __device__ __forceinline__ void finish(unsigned long long* __restrict__ ticket, float* __restrict__ loss, double fx_scale,
                                         int N) const {
    if (top_wait) {
      const unsigned ngrp = (gridDim.x + kTicketGroup - 1) / kTicketGroup;
      if (((top_old >> kFxSumBits) & 0x7ffull) == (unsigned long long)(ngrp - 1)) {
        const unsigned long long all = top_old + top_pay;
        __hip_atomic_store(ticket + kTicketTop, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float sum = (float)((double)(all & kFxSumMask) / fx_scale);
        *loss = (all & kFxPoison) ? __builtin_nanf("") : sum / (float)N;                       // pair_rank_loss_layer.cpp:49
      }
    }
  }
};

// Euclidean SimCross on (q,a+) and (q,a-), PairRankLoss on the two score
// columns, and the whole backward, in one launch (+ a one-block loss finish).
// Same wave-centric structure as euclid_rows_wave_kernel: a wave owns ONE
// triplet, issues all its 16-byte loads of q, a+, a- up front, keeps q-a+ and
// q-a- in registers; lanes 0-31 evaluate the positive branch's d-ascending sum
// and lanes 32-63 the negative branch's (speculative two-segment scheme of
// euclid_math.h when SPEC, plain walk by lanes 0 / 32 otherwise; both are the
// reference order, sim_cross_layer.cpp:100-106).  Each input is read once and
// each gradient written once.
template <int NIT, bool SPEC>
__global__ __launch_bounds__(256) void triplet_wave_kernel(
    int N, int D4, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge) {
  extern __shared__ float4 lds4[];               // [4 waves][2 branches] split images (euclid_math.h)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= N) return;
  const size_t base4 = (size_t)row * D4;
  const float4* q4 = reinterpret_cast<const float4*>(q) + base4;
  const float4* p4 = reinterpret_cast<const float4*>(ap) + base4;
  const float4* m4 = reinterpret_cast<const float4*>(an) + base4;
  const int st4 = spec_stride4(D4);
  float4* sqp = lds4 + (size_t)wave * 2 * st4;
  float4* sqn = sqp + st4;

  float4 x[NIT], u[NIT], v[NIT], dp[NIT], dn[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const int ii = i < D4 ? i : 0;
    x[it] = q4[ii]; u[it] = p4[ii]; v[it] = m4[ii];
  }
  float yy = y[row];
  float predp1 = 0.f, predp2 = 0.f, predn1 = 0.f, predn2 = 0.f;
  const int h4 = spec_h4(D4);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    dp[it].x = x[it].x - u[it].x; dp[it].y = x[it].y - u[it].y;
    dp[it].z = x[it].z - u[it].z; dp[it].w = x[it].w - u[it].w;
    dn[it].x = x[it].x - v[it].x; dn[it].y = x[it].y - v[it].y;
    dn[it].z = x[it].z - v[it].z; dn[it].w = x[it].w - v[it].w;
    float4 a, b;
    a.x = dp[it].x * dp[it].x; a.y = dp[it].y * dp[it].y;
    a.z = dp[it].z * dp[it].z; a.w = dp[it].w * dp[it].w;
    b.x = dn[it].x * dn[it].x; b.y = dn[it].y * dn[it].y;
    b.z = dn[it].z * dn[it].z; b.w = dn[it].w * dn[it].w;
    if (i < D4) { sqp[i] = a; sqn[i] = b; }
    const float a4 = (i < D4) ? (a.x + a.y) + (a.z + a.w) : 0.f;
    const float b4 = (i < D4) ? (b.x + b.y) + (b.z + b.w) : 0.f;
    predp1 += (i < h4) ? a4 : 0.f; predp2 += (i < 2 * h4) ? a4 : 0.f;
    predn1 += (i < h4) ? b4 : 0.f; predn2 += (i < 2 * h4) ? b4 : 0.f;
  }
  {
    const int npad = st4 - D4;                      // zero pad at the end of both images
    if (lane < 2 * npad) sqp[(lane / npad) * st4 + D4 + (lane % npad)] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int br = lane >> 5, j = lane & 31;       // branch handled by this half-wave
  float dist;
  if (SPEC) {
    predp1 = wave_sum(predp1); predp2 = wave_sum(predp2);
    predn1 = wave_sum(predn1); predn2 = wave_sum(predn2);
    wave_lds_sync();
    dist = chain_sum_speculative<32>(br ? sqn : sqp, D4, br ? predn1 : predp1, br ? predn2 : predp2,
                                     j, br * 32);
  } else {
    wave_lds_sync();
    dist = 0.f;
    if (j == 0) {   // plain walk over the whole image (the pad adds +0: exact)
      dist = chain_sum_lds(br ? sqn : sqp, st4, 0.f);
    }
    dist = __shfl(dist, br * 32, 64);
  }
  const float Tmine = 1.0f / (1.0f + sqrtf(dist));
  const float Tp = __shfl(Tmine, 0, 64), Tn = __shfl(Tmine, 32, 64);
  asm volatile("" : "+v"(yy));   // in a register before the stores below, or its wait becomes vmcnt(0) behind them (see euclid_pair32_kernel)
  if (lane == 0) { s_pos[row] = Tp; s_neg[row] = Tn; }

  // PairRankLoss on (Tp, Tn, y): every lane computes the same scalars
  const PairTerm pt = pair_term(Tp, Tn, yy, margin);
  float ga, gb;
  pair_grad(yy, pt.ordered, pt.similar, s0, s1, ga, gb, hinge_ge != 0);
  if (lane == 0) partials[row] = pt.term;
  const EuclidCoef k0 = euclid_coef(Tp, ga), k1 = euclid_coef(Tn, gb);

  // Layer-by-layer semantics: each SimCross backward produces dq_branch = 0 + tt and
  // da = 0 + (-tt); Caffe's Split layer then adds the two dq_branch blobs.
  float4* dq4 = reinterpret_cast<float4*>(dq) + base4;
  float4* dp4 = reinterpret_cast<float4*>(dap) + base4;
  float4* dn4 = reinterpret_cast<float4*>(dan) + base4;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i >= D4) break;
    const float4 tp = euclid_tt4(k0, dp[it]), tn = euclid_tt4(k1, dn[it]);
    float4 oq, op, on;
    oq.x = (0.f + tp.x) + (0.f + tn.x); oq.y = (0.f + tp.y) + (0.f + tn.y);
    oq.z = (0.f + tp.z) + (0.f + tn.z); oq.w = (0.f + tp.w) + (0.f + tn.w);
    op.x = 0.f + (-tp.x); op.y = 0.f + (-tp.y); op.z = 0.f + (-tp.z); op.w = 0.f + (-tp.w);
    on.x = 0.f + (-tn.x); on.y = 0.f + (-tn.y); on.z = 0.f + (-tn.z); on.w = 0.f + (-tn.w);
    stream_store(dq4 + i, oq);
    stream_store(dp4 + i, op);
    stream_store(dn4 + i, on);
  }
}

// Width-specialised step (D = 100 / 200 / 300), the triplet counterpart of euclid_pair32_kernel
// (simcross_rows.hip): D4C known at compile time, eight waves per workgroup, no early exit, N first
// for the kernarg preload, streaming stores.  EXACT as in euclid_pair32_kernel (include/mms.h:
// mms_set_euclid_backward_mode).
// A wave owns triplets 2w and 2w+1: their rows of q, a+ and a- are ONE dense run of 2*D4C float4 per array
// (lane l holds float4s l, l+64, l+128 of the run, whatever triplet they fall in), all requested up front.
// The two triplets then go through the chain phase one after the other -- pass 0, pass 1.  In a pass lanes
// 0-31 walk the image of the positive branch in LDS and lanes 32-63 that of the negative branch: the window
// centres by a half-wave DPP sum, the chain straight-line packed adds fed by LDS reads issued before the
// reductions, the stitch the DPP OR-reduction.  A pass stores its own triplet's gradients as
// soon as its scores are known: pass 1's LDS round trip and packed-add chains run while pass 0's stores drain,
// instead of every wave of the launch chaining and then every wave storing.  Half as many waves to dispatch,
// and a CU has half as many chains in its LDS return path at a time than with one triplet per wave (10.0
// against 10.4 us per step at 4096x300).  Same arithmetic, same bits.
template <int D4C, bool EXACT, int WPB, bool INL>
__global__ __launch_bounds__(64 * WPB) void triplet32x2_kernel(
    int N, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge,
    unsigned long long* __restrict__ ticket, float* __restrict__ loss, double fx_scale) {
  constexpr int C = 2 * D4C;                       // float4 per array per wave
  constexpr int NIT = (C + 63) / 64;
  constexpr int PNIT = (D4C + 31) / 32, LASTN = D4C - 32 * (PNIT - 1);
  constexpr int H4 = (D4C + 2) / 3, ST4 = 3 * H4;
  __shared__ float4 lds4[WPB * 4 * ST4];           // per wave: (triplet 0, +), (0, -), (1, +), (1, -)
  __shared__ unsigned long long wg_arrivals;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (INL) {
    if (threadIdx.x == 0) wg_arrivals = 0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  const long long r0 = ((long long)blockIdx.x * WPB + wave) * 2;
  const long long total4 = (long long)N * D4C;
  const long long b4 = r0 * D4C;
  const float4* q4 = reinterpret_cast<const float4*>(q);
  const float4* p4 = reinterpret_cast<const float4*>(ap);
  const float4* m4 = reinterpret_cast<const float4*>(an);
  float yy[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) yy[t] = y[min(r0 + t, (long long)N - 1)];
  float4 dp[NIT], dn[NIT];
  {
    float4 x[NIT], u[NIT], v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = lane + 64 * it;
      long long gi = b4 + ((NIT * 64 == C || i < C) ? i : 0);          // clamp: keep the load unconditional
      gi = gi < total4 ? gi : total4 - 1;                              // a run past the end reads the last float4
      x[it] = q4[gi]; u[it] = p4[gi]; v[it] = m4[gi];
    }
    float4* img = lds4 + (size_t)wave * 4 * ST4;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = lane + 64 * it;
      dp[it].x = x[it].x - u[it].x; dp[it].y = x[it].y - u[it].y;
      dp[it].z = x[it].z - u[it].z; dp[it].w = x[it].w - u[it].w;
      dn[it].x = x[it].x - v[it].x; dn[it].y = x[it].y - v[it].y;
      dn[it].z = x[it].z - v[it].z; dn[it].w = x[it].w - v[it].w;
      float4 a, b;
      a.x = dp[it].x * dp[it].x; a.y = dp[it].y * dp[it].y;
      a.z = dp[it].z * dp[it].z; a.w = dp[it].w * dp[it].w;
      b.x = dn[it].x * dn[it].x; b.y = dn[it].y * dn[it].y;
      b.z = dn[it].z * dn[it].z; b.w = dn[it].w * dn[it].w;
      if (NIT * 64 == C || i < C) {
        const int t = i >= D4C ? 1 : 0, c = i - t * D4C;
        img[(2 * t) * ST4 + c] = a;
        img[(2 * t + 1) * ST4 + c] = b;
      }
    }
    if constexpr (ST4 > D4C) {                                         // zero tail of each of the four images
      if (lane < 4 * (ST4 - D4C))
        img[(lane / (ST4 - D4C)) * ST4 + D4C + lane % (ST4 - D4C)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  asm volatile("" : "+v"(yy[0]), "+v"(yy[1]));    // in registers before any store (see euclid_pair32_kernel)
  wave_lds_sync();

  const int br = lane >> 5, j = lane & 31;         // branch walked by this half-wave
  float4* dq4 = reinterpret_cast<float4*>(dq);
  float4* dp4 = reinterpret_cast<float4*>(dap);
  float4* dn4 = reinterpret_cast<float4*>(dan);
  // ---- loss scalar ------------------------------------------------------------------------------------------
  // INL: ONE launch.  The terms are added as integers (units of 2^-S), so the sum does not depend on the order
  // of arrival, and the arrival count travels in the same 64-bit word as the sum: an atomic's return value
  // tells its issuer both that it was the last and what the others brought, with no store whose visibility
  // would have to be waited for first.  Three hops: waves -> workgroup word in LDS -> one word per
  // kTicketGroup workgroups -> top word; the wave that completes the top word writes the loss.  All of it is
  // issued BEFORE this wave's gradient stores (one wave per workgroup waits one round trip for its group word,
  // one per group issues the top atomic and reads its return after its stores), so the round trips run under
  // the launch's store drain instead of behind it (the first in-launch form -- write-through term stores,
  // arrival tickets, then a 16 KB read of the terms by the last workgroup -- had four dependent round trips
  // behind the terms and measured 12.6 us against 11.3 for a second launch).
  // A term outside [0, 2^kFxTermBits) (labels or a margin in the hundreds, a NaN input) poisons the words it
  // passes through and the loss comes out NaN; the two-launch mode has no such limit (include/mms.h).
  // In-launch loss: both passes first, then the arrival atomics, then ALL gradient stores, so that the atomics
  // enter the memory queues ahead of the wave's 7 KB of stores.  Measured (rocprofv3): the launch takes 9.6 us
  // with the in-launch sum against 7.6 us without, wherever the atomics are issued -- two DEPENDENT device-scope
  // atomic round trips (group word, then top word; they execute at the memory side of the fabric, not in an
  // XCD's L2) cost ~1.9 us, about what the second launch costs (1.9-2.3 us): 10.0 vs 10.2 us per step.
  // With the second launch a pass stores as soon as its scores are known.
  constexpr bool LATE = INL;
  LossArrival arr;
  EuclidCoef k0[2], k1[2];
  float c0[2] = {0.f, 0.f}, c1[2] = {0.f, 0.f}, rr0[2] = {0.f, 0.f}, rr1[2] = {0.f, 0.f};
  auto store_pass = [&](int t) {                   // gradients of triplet t's float4s (a slot can hold both triplets': masked)
    const bool have = r0 + t < N;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (64 * it >= (t + 1) * D4C || 64 * it + 63 < t * D4C) continue;   // no float4 of triplet t in this slot
      const int i = lane + 64 * it;
      const bool mine = have && i >= t * D4C && i < (t + 1) * D4C;
      float4 tp, tn;
      if (EXACT) { tp = euclid_tt4(k0[t], dp[it]); tn = euclid_tt4(k1[t], dn[it]); }
      else {
        tp.x = (c0[t] * dp[it].x) * rr0[t]; tp.y = (c0[t] * dp[it].y) * rr0[t];
        tp.z = (c0[t] * dp[it].z) * rr0[t]; tp.w = (c0[t] * dp[it].w) * rr0[t];
        tn.x = (c1[t] * dn[it].x) * rr1[t]; tn.y = (c1[t] * dn[it].y) * rr1[t];
        tn.z = (c1[t] * dn[it].z) * rr1[t]; tn.w = (c1[t] * dn[it].w) * rr1[t];
      }
      if (mine) {
        float4 oq, op, on;
        oq.x = (0.f + tp.x) + (0.f + tn.x); oq.y = (0.f + tp.y) + (0.f + tn.y);
        oq.z = (0.f + tp.z) + (0.f + tn.z); oq.w = (0.f + tp.w) + (0.f + tn.w);
        op.x = 0.f + (-tp.x); op.y = 0.f + (-tp.y); op.z = 0.f + (-tp.z); op.w = 0.f + (-tp.w);
        on.x = 0.f + (-tn.x); on.y = 0.f + (-tn.y); on.z = 0.f + (-tn.z); on.w = 0.f + (-tn.w);
        stream_store(dq4 + b4 + i, oq);
        stream_store(dp4 + b4 + i, op);
        stream_store(dn4 + b4 + i, on);
      }
    }
  };
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bool have = r0 + t < N;
    const long long row = have ? r0 + t : (long long)N - 1;
    const float4* im = lds4 + ((size_t)wave * 4 + 2 * t + br) * ST4;
    SpecSegment<H4> sg;
    sg.load(im + spec_seg32(j) * H4);
    // window centres: tree sums of segment 0 / segments 0-1, read back from the image (as euclid_block_kernel)
    const bool last_ok = (LASTN >= 32) || (j < LASTN);
    float p1 = 0.f, p2 = 0.f;
#pragma unroll
    for (int it = 0; it < PNIT; ++it) {
      const bool valid = (it < PNIT - 1) || last_ok;
      const float4 sq = im[valid ? j + 32 * it : 0];
      const float s4 = valid ? (sq.x + sq.y) + (sq.z + sq.w) : 0.f;
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
    if (!hit) {
      dist = chain_sum_lds(im, ST4, 0.0f);
    }
    __builtin_amdgcn_s_setprio(0);
    const float Tmine = 1.0f / (1.0f + sqrtf(dist));
    const float Tp = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Tmine), 0));
    const float Tn = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Tmine), 32));
    const PairTerm pt = pair_term(Tp, Tn, yy[t], margin);
    float ga, gb;
    pair_grad(yy[t], pt.ordered, pt.similar, s0, s1, ga, gb, hinge_ge != 0);
    if (EXACT) { k0[t] = euclid_coef(Tp, ga); k1[t] = euclid_coef(Tn, gb); }
    else {
      c0[t] = ga * Tp * Tp * Tp; c1[t] = gb * Tn * Tn * Tn;
      rr0[t] = (float)rcp_newton((double)(Tp - 1.0f) + 1e-9);
      rr1[t] = (float)rcp_newton((double)(Tn - 1.0f) + 1e-9);
    }
    if (INL) {
      arr.add(have ? pt.term : 0.f, fx_scale);
      if (t == 1 && lane == 0) arr.template arrive<WPB>(&wg_arrivals, ticket);   // the wave's two terms arrive together ("loss scalar" above)
    } else {
      if (lane == 0 && have) partials[row] = pt.term;
    }
    if (lane == 0 && have) { s_pos[row] = Tp; s_neg[row] = Tn; }
    if (!LATE) store_pass(t);
  }
  if (LATE) { store_pass(0); store_pass(1); }
  if (!INL) return;
  arr.finish(ticket, loss, fx_scale, N);
}

// Generic fallback (any D / alignment): a workgroup owns ROWS triplets.
template <int ROWS, int THREADS>
__global__ __launch_bounds__(THREADS) void triplet_generic_kernel(
    int N, int D, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge) {
  extern __shared__ float4 lds_raw[];
  float* dpos = reinterpret_cast<float*>(lds_raw);   // [ROWS*D]
  float* dneg = dpos + (size_t)ROWS * D;             // [ROWS*D]
  __shared__ float Ts[2][ROWS];
  __shared__ float cs[2][ROWS];
  __shared__ double dens[2][ROWS];
  __shared__ float terms[ROWS];

  const int row0 = blockIdx.x * ROWS;
  const int rows = min(ROWS, N - row0);
  if (rows <= 0) return;                             // uniform per workgroup: no barrier is skipped by part of one
  const size_t base = (size_t)row0 * D;
  const int total = rows * D;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const float x = q[base + i];
    dpos[i] = x - ap[base + i];
    dneg[i] = x - an[base + i];
  }
  __syncthreads();
  if (threadIdx.x < 2 * ROWS) {
    const int br = threadIdx.x / ROWS, r = threadIdx.x % ROWS;
    if (r < rows) {
      const float* src = (br ? dneg : dpos) + r * D;
      float dist = 0.f;
      for (int d = 0; d < D; ++d) dist += src[d] * src[d];
      const float T = 1.0f / (1.0f + sqrtf(dist));
      Ts[br][r] = T;
      (br ? s_neg : s_pos)[row0 + r] = T;
    }
  }
  __syncthreads();
  if (threadIdx.x < ROWS) {
    const int r = threadIdx.x;
    float t = 0.f;
    if (r < rows) {
      const float yy = y[row0 + r];
      const PairTerm p = pair_term(Ts[0][r], Ts[1][r], yy, margin);
      float ga, gb;
      pair_grad(yy, p.ordered, p.similar, s0, s1, ga, gb, hinge_ge != 0);
      const EuclidCoef k0 = euclid_coef(Ts[0][r], ga), k1 = euclid_coef(Ts[1][r], gb);
      cs[0][r] = k0.c; dens[0][r] = k0.den;
      cs[1][r] = k1.c; dens[1][r] = k1.den;
      t = p.term;
    }
    terms[r] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < rows) partials[row0 + threadIdx.x] = terms[threadIdx.x];   // one term per triplet, like the wave kernels
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int r = i / D;
    const float tp = euclid_tt_exact(cs[0][r], dens[0][r], dpos[i]);
    const float tn = euclid_tt_exact(cs[1][r], dens[1][r], dneg[i]);
    dq[base + i] = (0.f + tp) + (0.f + tn);
    dap[base + i] = 0.f + (-tp);
    dan[base + i] = 0.f + (-tn);
  }
}

constexpr int kTripRows = 8;
constexpr int kTripThreads = 256;

// Arrival words of the in-launch loss reduction live at the HEAD of the caller's triplet workspace (kTicketStride
// 64-bit words, then one float per triplet).  They are zero whenever no launch is using the workspace:
// mms_triplet_workspace_init zeroes them once (and again after a launch that died mid-way), and the wave that
// completes a word resets it.  A launch -- eager or as a node of a captured graph -- therefore owns the words of the
// workspace it was given: the ABI's "one workspace per call in flight" rule covers them, and nothing about them is
// chosen at call time by host state.
constexpr size_t kTicketBytes = (size_t)kTicketStride * sizeof(unsigned long long);

size_t triplet_workspace_bytes(int N) { return kTicketBytes + (size_t)N * sizeof(float); }

int triplet_workspace_init(void* ws, size_t ws_bytes, hipStream_t s) {
  if (ws == nullptr || ws_bytes < kTicketBytes || (reinterpret_cast<uintptr_t>(ws) & 7u)) return MMS_ERR_WORKSPACE;
  return hipMemsetAsync(ws, 0, kTicketBytes, s) == hipSuccess ? MMS_OK : MMS_ERR_LAUNCH;
}

// What both steps derive from (N, loss_weight, workspace) before they pick a kernel.
struct TripletPlan {
  float s0, s1;                  // the two bottoms' signs times loss_weight / count (pair_rank_loss_layer.cpp:64, count = N*1)
  int hge;                       // hinge gate `>=` (pairrank.hip: t_hinge_mode)
  unsigned long long* tickets;   // head of the workspace: the arrival words
  float* partials;               // then one term per triplet
};
static int triplet_plan(int N, float loss_weight, void* ws, size_t ws_bytes, TripletPlan* p) {
  if (ws == nullptr || ws_bytes < triplet_workspace_bytes(N) || (reinterpret_cast<uintptr_t>(ws) & 7u))
    return MMS_ERR_WORKSPACE;
  const float scale = loss_weight / (float)N;
  *p = {-1.0f * scale, 1.0f * scale, pairrank_hinge_mode() == MMS_PAIRRANK_HINGE_GPU ? 1 : 0,
        static_cast<unsigned long long*>(ws), reinterpret_cast<float*>(static_cast<char*>(ws) + kTicketBytes)};
  return MMS_OK;
}

// Is the loss of a width-specialised launch of `grid` workgroups summed inside it, and at what fixed-point scale?
// MMS_TRIPLET_FINISH_INLAUNCH: yes (integer terms, arrival words that carry the sum: see triplet32x2_kernel);
// otherwise, and for batches beyond what a ticket slot covers, `tickets` is null, the kernel stores the per-triplet
// terms and a second, one-workgroup launch sums them.
struct InLaunchLoss { unsigned long long* tickets; double fx_scale; };
static InLaunchLoss in_launch_loss(const TripletPlan& p, unsigned grid, int N, const float* loss) {
  const unsigned ngrp = (grid + kTicketGroup - 1) / kTicketGroup;
  const bool inl = triplet_finish_mode() == MMS_TRIPLET_FINISH_INLAUNCH && ngrp <= (unsigned)kTicketTop &&
                   loss_sum_mode() != MMS_LOSS_SUM_REFERENCE && loss != nullptr;
  int lg = 0;
  while (((long long)1 << lg) < (long long)N) ++lg;
  return {inl ? p.tickets : nullptr, std::ldexp(1.0, kFxSumBits - kFxTermBits - lg)};
}

int triplet_euclid_step(int N, int D, float margin, float loss_weight, const float* q,
                        const float* ap, const float* an, const float* y, float* s_pos,
                        float* s_neg, float* loss, float* dq, float* dap, float* dan, void* ws,
                        size_t ws_bytes, hipStream_t s) {
  if (N == 0) return MMS_OK;
  TripletPlan p;
  if (const int rc = triplet_plan(N, loss_weight, ws, ws_bytes, &p)) return rc;
  const bool v = (D % 4 == 0) && aligned16(q) && aligned16(ap) && aligned16(an) &&
                 aligned16(dq) && aligned16(dap) && aligned16(dan);
  if (v && glove_width(D)) {
    constexpr int WPB = 8;
    const unsigned grid = (unsigned)((N + WPB * 2 - 1) / (WPB * 2));   // two triplets per wave
    const InLaunchLoss il = in_launch_loss(p, grid, N, loss);
    with_glove_d4(D, [&](auto W) {
      with_bool(euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE, [&](auto EXACT) {
        with_bool(il.tickets != nullptr, [&](auto INL) {
          hipLaunchKernelGGL((triplet32x2_kernel<decltype(W)::value, decltype(EXACT)::value, WPB, decltype(INL)::value>),
                             dim3(grid), dim3(64 * WPB), 0, s, N, margin, p.s0, p.s1, q, ap, an, y, s_pos, s_neg,
                             p.partials, dq, dap, dan, p.hge, il.tickets, loss, il.fx_scale);
        });
      });
    });
    if (il.tickets) return launch_status();        // the loss was reduced inside the launch
  } else if (v && wave_width_ok(D)) {
    const int D4 = D / 4;
    const int nit = (D4 + 63) / 64;
    const unsigned grid = (unsigned)((N + 3) / 4);
    const size_t lds = spec_image_lds(4, 2, D4);   // one triplet per wave: the images of its two pairs
    const bool spec = wave_pairs(D) == 2;          // the +-15 ulp window of 32 lanes holds: see euclid_math.h
    static constexpr decltype(&triplet_wave_kernel<1, true>) kernels[2][4] = {MMS_NIT4(triplet_wave_kernel, false),
                                                                              MMS_NIT4(triplet_wave_kernel, true)};
    hipLaunchKernelGGL(kernels[spec][nit - 1], dim3(grid), dim3(256), lds, s, N, D4, margin, p.s0, p.s1, q, ap, an, y,
                       s_pos, s_neg, p.partials, dq, dap, dan, p.hge);
  } else {
    const size_t lds = 2 * (size_t)kTripRows * D * sizeof(float);
    if (lds > 96 * 1024) return MMS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((triplet_generic_kernel<kTripRows, kTripThreads>), dim3((unsigned)((N + kTripRows - 1) / kTripRows)),
                       dim3(kTripThreads), lds, s, N, D, margin, p.s0, p.s1, q, ap, an, y, s_pos,
                       s_neg, p.partials, dq, dap, dan, p.hge);   // one term per triplet, like the wave kernels
  }
  if (loss == nullptr) return launch_status();     // the caller does not want the scalar: no reduction at all
  return triplet_loss_from_terms(p.partials, N, loss, s);
}

// ======================= fused cosine (q, a+, a-) training step =====================
// SimCross dist_mode 0 on (q,a+) and (q,a-), PairRankLoss on the two score columns and the whole backward in one
// launch (include/mms.h: mms_triplet_cosine_step_f32).  No ordered chain: five dot products per triplet (qq, pp, nn,
// qp, qn -- qq ONCE for both branches, where the two layers would each compute it), accumulated per lane and reduced
// exactly as the unfused kernel that serves the width does (cosine_math.h), so that scores, norms and gradients
// carry that kernel's bits.
//
// Width-specialised (D = 100 / 200 / 300, inputs 16-byte aligned): the data movement of cosine_pair32_kernel -- 32
// lanes per triplet, two triplets per wave, every float4 of q, a+ and a- requested up front (9 per lane at D = 300)
// and kept for the backward, half-wave DPP sums, streaming stores.  Every lane of a half holds its triplet's scalars
// (T+, T-, the hinge term, g+, g-), so nothing is broadcast.  The loss goes through the arrival words of the Euclid
// step (LossArrival), the atomics issued before the gradient stores.  VOUT = false (a gradient array that is not
// 16-byte aligned): the unfused backward takes cosine_rows_kernel's scalar path there, so its expression and scalar
// stores are used.
template <int D4C, int WPB, bool INL, bool VOUT>
__global__ __launch_bounds__(64 * WPB) void triplet_cosine32_kernel(
    int N, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ norm_q,
    float* __restrict__ norm_pos, float* __restrict__ norm_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge,
    unsigned long long* __restrict__ ticket, float* __restrict__ loss, double fx_scale) {
  constexpr int NIT = (D4C + 31) / 32;
  __shared__ unsigned long long wg_arrivals;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 5, j = lane & 31;
  if (INL) {
    if (threadIdx.x == 0) wg_arrivals = 0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  const long long want = ((long long)blockIdx.x * WPB + wave) * 2 + grp;
  const bool have = want < N;
  const long long row = have ? want : (long long)N - 1;
  const float4* q4 = reinterpret_cast<const float4*>(q) + row * D4C;
  const float4* p4 = reinterpret_cast<const float4*>(ap) + row * D4C;
  const float4* m4 = reinterpret_cast<const float4*>(an) + row * D4C;
  float4 x[NIT], u[NIT], v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = j + 32 * it;
    const int ii = i < D4C ? i : 0;              // clamp: keep the load unconditional
    x[it] = q4[ii]; u[it] = p4[ii]; v[it] = m4[ii];
  }
  float yy = y[row];
  float sqq = 0.f, spp = 0.f, snn = 0.f, sqp = 0.f, sqn = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (j + 32 * it < D4C) {
      cosine_acc4(sqq, x[it], x[it]); cosine_acc4(spp, u[it], u[it]); cosine_acc4(snn, v[it], v[it]);
      cosine_acc4(sqp, x[it], u[it]); cosine_acc4(sqn, x[it], v[it]);
    }
  }
  sqq = half_wave_sum(sqq); spp = half_wave_sum(spp); snn = half_wave_sum(snn);
  sqp = half_wave_sum(sqp); sqn = half_wave_sum(sqn);
  const CosineScore cp = cosine_score(sqq, spp, sqp), cn = cosine_score(sqq, snn, sqn);   // cp.n0 == cn.n0
  asm volatile("" : "+v"(yy));   // in a register before any store, or its wait becomes vmcnt(0) behind them (see euclid_pair32_kernel)
  const PairTerm pt = pair_term(cp.T, cn.T, yy, margin);
  float ga, gb;
  pair_grad(yy, pt.ordered, pt.similar, s0, s1, ga, gb, hinge_ge != 0);
  LossArrival arr;
  if (INL) {
    const float tm = have ? pt.term : 0.f;
    arr.add(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(tm), 0)), fx_scale);
    arr.add(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(tm), 32)), fx_scale);
    if (lane == 0) arr.template arrive<WPB>(&wg_arrivals, ticket);   // the wave's two terms arrive together
  } else {
    if (j == 0 && have) partials[row] = pt.term;
  }
  if (j == 0 && have) {
    s_pos[row] = cp.T; s_neg[row] = cn.T;
    if (norm_q) norm_q[row] = cp.n0;
    if (norm_pos) norm_pos[row] = cp.n1;
    if (norm_neg) norm_neg[row] = cn.n1;
  }
  // Layer by layer: each SimCross backward writes dq_branch = 0 + g*(...), Net::Init's Split layer adds the two.
  if (VOUT) {
    const CosineFactors fp = cosine_factors(cp.T, cp.n0, cp.n1), fn = cosine_factors(cn.T, cn.n0, cn.n1);
    float4* dq4 = reinterpret_cast<float4*>(dq) + row * D4C;
    float4* dp4 = reinterpret_cast<float4*>(dap) + row * D4C;
    float4* dn4 = reinterpret_cast<float4*>(dan) + row * D4C;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = j + 32 * it;
      if (i < D4C && have) {
        const float4 qp = cosine_grad4_fac(ga, fp.inv01, fp.cq, u[it], x[it]);
        const float4 qn = cosine_grad4_fac(gb, fn.inv01, fn.cq, v[it], x[it]);
        float4 oq;
        oq.x = qp.x + qn.x; oq.y = qp.y + qn.y; oq.z = qp.z + qn.z; oq.w = qp.w + qn.w;
        stream_store(dq4 + i, oq);
        stream_store(dp4 + i, cosine_grad4_fac(ga, fp.inv01, fp.ca, x[it], u[it]));
        stream_store(dn4 + i, cosine_grad4_fac(gb, fn.inv01, fn.ca, x[it], v[it]));
      }
    }
  } else {
    const float n00 = cp.n0 * cp.n0, npp = cp.n1 * cp.n1, nnn = cn.n1 * cn.n1;
    float* dqr = dq + row * (4 * D4C);
    float* dpr = dap + row * (4 * D4C);
    float* dnr = dan + row * (4 * D4C);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = j + 32 * it;
      if (i < D4C && have) {
        const float4 qp = cosine_grad4_div(ga, cp.n0, cp.n1, cp.T, n00, u[it], x[it]);
        const float4 qn = cosine_grad4_div(gb, cn.n0, cn.n1, cn.T, n00, v[it], x[it]);
        const float4 op = cosine_grad4_div(ga, cp.n0, cp.n1, cp.T, npp, x[it], u[it]);
        const float4 on = cosine_grad4_div(gb, cn.n0, cn.n1, cn.T, nnn, x[it], v[it]);
        dqr[4 * i] = qp.x + qn.x; dqr[4 * i + 1] = qp.y + qn.y; dqr[4 * i + 2] = qp.z + qn.z; dqr[4 * i + 3] = qp.w + qn.w;
        dpr[4 * i] = op.x; dpr[4 * i + 1] = op.y; dpr[4 * i + 2] = op.z; dpr[4 * i + 3] = op.w;
        dnr[4 * i] = on.x; dnr[4 * i + 1] = on.y; dnr[4 * i + 2] = on.z; dnr[4 * i + 3] = on.w;
      }
    }
  }
  if (INL) arr.finish(ticket, loss, fx_scale, N);
}

// Any other width that is a multiple of 4 up to 1024, all six arrays 16-byte aligned: a wave owns ONE triplet (the
// shape of triplet_wave_kernel), its float4s of q, a+ and a- requested up front and kept for the backward.  Sum
// order and backward expression are cosine_rows_kernel<VEC4>'s, the kernel the unfused calls use for these widths.
template <int NIT>
__global__ __launch_bounds__(256) void triplet_cosine_wave_kernel(
    int N, int D4, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ norm_q,
    float* __restrict__ norm_pos, float* __restrict__ norm_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= N) return;
  const size_t base4 = (size_t)row * D4;
  const float4* q4 = reinterpret_cast<const float4*>(q) + base4;
  const float4* p4 = reinterpret_cast<const float4*>(ap) + base4;
  const float4* m4 = reinterpret_cast<const float4*>(an) + base4;
  float4 x[NIT], u[NIT], v[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const int ii = i < D4 ? i : 0;
    x[it] = q4[ii]; u[it] = p4[ii]; v[it] = m4[ii];
  }
  float yy = y[row];
  float sqq = 0.f, spp = 0.f, snn = 0.f, sqp = 0.f, sqn = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (lane + 64 * it < D4) {
      cosine_acc4(sqq, x[it], x[it]); cosine_acc4(spp, u[it], u[it]); cosine_acc4(snn, v[it], v[it]);
      cosine_acc4(sqp, x[it], u[it]); cosine_acc4(sqn, x[it], v[it]);
    }
  }
  sqq = wave_sum(sqq); spp = wave_sum(spp); snn = wave_sum(snn); sqp = wave_sum(sqp); sqn = wave_sum(sqn);
  const CosineScore cp = cosine_score(sqq, spp, sqp), cn = cosine_score(sqq, snn, sqn);
  asm volatile("" : "+v"(yy));
  const PairTerm pt = pair_term(cp.T, cn.T, yy, margin);
  float ga, gb;
  pair_grad(yy, pt.ordered, pt.similar, s0, s1, ga, gb, hinge_ge != 0);
  if (lane == 0) {
    s_pos[row] = cp.T; s_neg[row] = cn.T; partials[row] = pt.term;
    if (norm_q) norm_q[row] = cp.n0;
    if (norm_pos) norm_pos[row] = cp.n1;
    if (norm_neg) norm_neg[row] = cn.n1;
  }
  const float n00 = cp.n0 * cp.n0, npp = cp.n1 * cp.n1, nnn = cn.n1 * cn.n1;
  float4* dq4 = reinterpret_cast<float4*>(dq) + base4;
  float4* dp4 = reinterpret_cast<float4*>(dap) + base4;
  float4* dn4 = reinterpret_cast<float4*>(dan) + base4;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i >= D4) break;
    const float4 qp = cosine_grad4_div(ga, cp.n0, cp.n1, cp.T, n00, u[it], x[it]);
    const float4 qn = cosine_grad4_div(gb, cn.n0, cn.n1, cn.T, n00, v[it], x[it]);
    float4 oq;
    oq.x = qp.x + qn.x; oq.y = qp.y + qn.y; oq.z = qp.z + qn.z; oq.w = qp.w + qn.w;
    stream_store(dq4 + i, oq);
    stream_store(dp4 + i, cosine_grad4_div(ga, cp.n0, cp.n1, cp.T, npp, x[it], u[it]));
    stream_store(dn4 + i, cosine_grad4_div(gb, cn.n0, cn.n1, cn.T, nnn, x[it], v[it]));
  }
}

// Generic tail (any D, any alignment, widths beyond 1024): a wave per triplet, the two loops of cosine_rows_kernel.
// VIN: D % 4 == 0 and q, a+, a- 16-byte aligned -- the unfused FORWARD then sums float4-wise, so this one does; the
// backward re-reads the row (it was just read: L2) and stores element by element, whatever the gradients' alignment.
template <bool VIN>
__global__ __launch_bounds__(256) void triplet_cosine_rows_kernel(
    int N, int D, float margin, float s0, float s1, const float* __restrict__ q,
    const float* __restrict__ ap, const float* __restrict__ an, const float* __restrict__ y,
    float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ norm_q,
    float* __restrict__ norm_pos, float* __restrict__ norm_neg, float* __restrict__ partials,
    float* __restrict__ dq, float* __restrict__ dap, float* __restrict__ dan, int hinge_ge) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const size_t base = (size_t)row * D;
  const float* qr = q + base;
  const float* pr = ap + base;
  const float* mr = an + base;
  float yy = y[row];
  float sqq = 0.f, spp = 0.f, snn = 0.f, sqp = 0.f, sqn = 0.f;
  if (VIN) {
    const float4* q4 = reinterpret_cast<const float4*>(qr);
    const float4* p4 = reinterpret_cast<const float4*>(pr);
    const float4* m4 = reinterpret_cast<const float4*>(mr);
    for (int i = lane; i < (D >> 2); i += 64) {
      const float4 x = q4[i], u = p4[i], v = m4[i];
      cosine_acc4(sqq, x, x); cosine_acc4(spp, u, u); cosine_acc4(snn, v, v);
      cosine_acc4(sqp, x, u); cosine_acc4(sqn, x, v);
    }
  } else {
    for (int i = lane; i < D; i += 64) {
      const float x = qr[i], u = pr[i], v = mr[i];
      cosine_acc1(sqq, x, x); cosine_acc1(spp, u, u); cosine_acc1(snn, v, v);
      cosine_acc1(sqp, x, u); cosine_acc1(sqn, x, v);
    }
  }
  sqq = wave_sum(sqq); spp = wave_sum(spp); snn = wave_sum(snn); sqp = wave_sum(sqp); sqn = wave_sum(sqn);
  const CosineScore cp = cosine_score(sqq, spp, sqp), cn = cosine_score(sqq, snn, sqn);
  asm volatile("" : "+v"(yy));
  const PairTerm pt = pair_term(cp.T, cn.T, yy, margin);
  float ga, gb;
  pair_grad(yy, pt.ordered, pt.similar, s0, s1, ga, gb, hinge_ge != 0);
  if (lane == 0) {
    s_pos[row] = cp.T; s_neg[row] = cn.T; partials[row] = pt.term;
    if (norm_q) norm_q[row] = cp.n0;
    if (norm_pos) norm_pos[row] = cp.n1;
    if (norm_neg) norm_neg[row] = cn.n1;
  }
  const float n00 = cp.n0 * cp.n0, npp = cp.n1 * cp.n1, nnn = cn.n1 * cn.n1;
  for (int i = lane; i < D; i += 64) {
    const float x = qr[i], u = pr[i], v = mr[i];
    dq[base + i] = cosine_grad_div(ga, cp.n0, cp.n1, cp.T, n00, u, x) + cosine_grad_div(gb, cn.n0, cn.n1, cn.T, n00, v, x);
    dap[base + i] = cosine_grad_div(ga, cp.n0, cp.n1, cp.T, npp, x, u);
    dan[base + i] = cosine_grad_div(gb, cn.n0, cn.n1, cn.T, nnn, x, v);
  }
}

int triplet_cosine_step(int N, int D, float margin, float loss_weight, const float* q, const float* ap,
                        const float* an, const float* y, float* s_pos, float* s_neg, float* norm_q,
                        float* norm_pos, float* norm_neg, float* loss, float* dq, float* dap, float* dan,
                        void* ws, size_t ws_bytes, hipStream_t s) {
  if (N == 0) return MMS_OK;
  TripletPlan p;
  if (const int rc = triplet_plan(N, loss_weight, ws, ws_bytes, &p)) return rc;
  // The unfused forward picks its kernel -- and with it the sum order -- from D and the alignment of its INPUTS; the
  // unfused backward picks its expression from the alignment of the gradients as well.
  const bool vin = (D % 4 == 0) && aligned16(q) && aligned16(ap) && aligned16(an);
  const bool vout = aligned16(dq) && aligned16(dap) && aligned16(dan);
  if (vin && glove_width(D)) {
    constexpr int WPB = 8;
    const unsigned grid = (unsigned)((N + WPB * 2 - 1) / (WPB * 2));   // two triplets per wave
    const InLaunchLoss il = in_launch_loss(p, grid, N, loss);
    with_glove_d4(D, [&](auto W) {
      with_bool(il.tickets != nullptr, [&](auto INL) {
        with_bool(vout, [&](auto VOUT) {
          hipLaunchKernelGGL((triplet_cosine32_kernel<decltype(W)::value, WPB, decltype(INL)::value, decltype(VOUT)::value>),
                             dim3(grid), dim3(64 * WPB), 0, s, N, margin, p.s0, p.s1, q, ap, an, y, s_pos, s_neg, norm_q,
                             norm_pos, norm_neg, p.partials, dq, dap, dan, p.hge, il.tickets, loss, il.fx_scale);
        });
      });
    });
    if (il.tickets) return launch_status();        // the loss was reduced inside the launch
  } else if (vin && vout && wave_width_ok(D)) {
    const int D4 = D / 4;
    static constexpr decltype(&triplet_cosine_wave_kernel<1>) kernels[4] = {
        triplet_cosine_wave_kernel<1>, triplet_cosine_wave_kernel<2>, triplet_cosine_wave_kernel<3>,
        triplet_cosine_wave_kernel<4>};
    hipLaunchKernelGGL(kernels[(D4 + 63) / 64 - 1], dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, N, D4, margin, p.s0,
                       p.s1, q, ap, an, y, s_pos, s_neg, norm_q, norm_pos, norm_neg, p.partials, dq, dap, dan, p.hge);
  } else {
    hipLaunchKernelGGL((vin ? triplet_cosine_rows_kernel<true> : triplet_cosine_rows_kernel<false>),
                       dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, N, D, margin, p.s0, p.s1, q, ap, an, y, s_pos,
                       s_neg, norm_q, norm_pos, norm_neg, p.partials, dq, dap, dan, p.hge);
  }
  if (loss == nullptr) return launch_status();     // the caller does not want the scalar: no reduction at all
  return triplet_loss_from_terms(p.partials, N, loss, s);
}

}  // namespace mms
