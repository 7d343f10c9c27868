// csrc/cross_grid.h -- SimCross dist_mode 0 (cosine) and 1 (Euclidean) on general W1 x W2 word grids (TREC-QA 40x40)
// for gfx950: the kernels and their launch plan, ONE definition each, templated on the storage type S of q, a, dq, da
// in HBM -- float (simcross_cross.hip) or IEEE half (simcross_cross_f16.hip); top, top_diff and the norms are fp32.
// HBM-bound: no MFMA here.
//
// Reference semantics (all file:line in src/caffe/layers/sim_cross_layer.cpp):
//   Euclid fwd  :96-111   T = 1/(1+sqrt(sum_d (q-a)^2)), d ascending, fp32.
//   Euclid bwd  :208-225  tt = dT*T*T*T*(q-a)/(T-1+1e-9) (double divide);
//                         dq[j,d] = sum_k tt (k ascending from 0),
//                         da[k,d] = sum_j -tt (j ascending from 0).
//   Cosine fwd  :112-139  n0,n1 = sqrt(dot) cached; T = dot/n0/n1.
//   Cosine bwd  :226-250.
//
// The arithmetic is fp32 on the exactly-widened inputs whatever S is: an element becomes a float when it is written to
// LDS (forward, tiled backward) or right after its load (plain backward, norms) -- the identity for S = float -- every
// sum runs in the reference's order, and a gradient element is rounded ONCE when it is stored (halves: RNE,
// v_cvt_f16_f32, overflow gives +-Inf).  So a half call carries the bits of the fp32 call on the widened inputs.
// The forward's register tile and T are CrossAcc (cross_acc.h), the backward terms euclid_math.h / cosine_math.h: no
// arithmetic is defined here.  The cosine terms are cosine_math.h's BARE ones (no leading `0.f +`): every one of them
// is added to an accumulator that starts at +0.f, and there the two forms give the same bits -- `0.f +` changes only a
// term of -0 into +0, and acc + (-0) = acc + (+0) for every acc an accumulation from +0 can hold (never -0).
//
// Alignment: elements are loaded and stored one by one unless a wider access has tested its own preconditions -- the
// pair image copies 16 bytes per lane (cross_fwd_image_ok) or, gathered from a table, two elements; the half backward
// packs 2 or 4 neighbouring d of a row into one store where the address allows (store_halves).  Any D >= 1 and any
// element-aligned operand is served.
//
// The Embed gather (cross_gather.h) is the template option GATHER of the two forward kernels and a run-time one of the
// norm kernel: q and a are then both the table, row j of pair n is table row gather_id(iq[n*W1 + j]), and a row value
// is bias[d] + widen(table[id][d]) -- one fp32 add after the widening -- or the widened element alone without a bias.
//
// Compiled with -ffp-contract=off: the reference CPU build has no FMA contraction, so mul and add must round
// separately to match it bitwise.  DESIGN.md 4.4b is the table the launch plan at the end is read against;
// tests/cross_grid_model.py restates every decision of it, one function each.
#ifndef MMS_CROSS_GRID_H_
#define MMS_CROSS_GRID_H_

#include "cosine_math.h"
#include "cross_acc.h"
#include "cross_gather.h"
#include "euclid_math.h"
#include "mms_internal.h"

namespace mms {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// n <= NT fp32 values to consecutive halves at p, each rounded once (RNE); one NT-wide store when all NT are valid
// and p is aligned to it.
template <int NT>
__device__ __forceinline__ void store_halves(_Float16* p, const float* v, int n) {
  static_assert(NT == 2 || NT == 4, "half2 or half4 stores");
  if (n == NT && (reinterpret_cast<uintptr_t>(p) & (2 * NT - 1)) == 0) {
    if constexpr (NT == 2) {
      *reinterpret_cast<half2v*>(p) = (half2v){(_Float16)v[0], (_Float16)v[1]};
    } else {
      *reinterpret_cast<half4v*>(p) = (half4v){(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < NT; ++u)
    if (u < n) p[u] = (_Float16)v[u];
}

// What differs between the two storages, and nothing else:
//   Vec16, widen16   the 16-byte vector of the pair-image copy and its widening into the fp32 LDS image
//   Vec2, widen2     the two-element vector of the gathered image copy and its widening
//   kGatherAlign     bytes of alignment the gathered image route asks of the table (ungathered: 16 for both)
//   kNT, store       neighbouring elements of a gradient row per thread, and the store of 1 <= n <= NT finished ones
template <class S> struct GridStorage;
template <> struct GridStorage<float> {
  typedef float4 Vec16;
  typedef float2 Vec2;
  static constexpr int kGatherAlign = 16, kNT = 1;
  static __device__ __forceinline__ void widen16(float4* dst, const float4& v) { dst[0] = v; }
  static __device__ __forceinline__ float2 widen2(const float2& v) { return v; }
  template <int NT>
  static __device__ __forceinline__ void store(float* p, const float* v, int n) {
#pragma unroll
    for (int u = 0; u < NT; ++u)
      if (u == 0 || u < n) p[u] = v[u];
  }
};
template <> struct GridStorage<_Float16> {
  typedef half8 Vec16;
  typedef half2v Vec2;
  // a table row is D halves = 100 bytes at the image's D: a 4-byte aligned table promises 4-byte aligned rows, no more
  static constexpr int kGatherAlign = 4, kNT = 2;
  static __device__ __forceinline__ void widen16(float4* dst, const half8& h) {
    dst[0] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
    dst[1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
  }
  static __device__ __forceinline__ float2 widen2(const half2v& h) { return make_float2((float)h[0], (float)h[1]); }
  template <int NT>
  static __device__ __forceinline__ void store(_Float16* p, const float* v, int n) { store_halves<NT>(p, v, n); }
};

// L2 norms of `rows` rows of length D: one wave per row (cosine).
// index != nullptr: row `row` is table row index[row] of x (K rows) -- the Embed gather fused in -- and ebias (or
// nullptr) is added before squaring.
template <class S>
__global__ __launch_bounds__(256) void row_norm_kernel(const S* __restrict__ x, float* __restrict__ nrm, long long rows,
                                                       int D, const float* __restrict__ index, int K,
                                                       const float* __restrict__ ebias) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const S* r = x + (index ? (long long)gather_id(index[row], K) : row) * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) { const float v = ebias ? ebias[i] + (float)r[i] : (float)r[i]; s += v * v; }
  s = wave_sum(s);
  if (lane == 0) nrm[row] = sqrtf(s);
}

// Forward, generic staging, MODE 0 (cosine; norms precomputed) or 1.  One wave per (pair, j-tile, k-tile); tile =
// (8*RJ) x (8*RK) outputs, lane (lj = lane>>3, lk = lane&7) owns outputs j = j0+lj+8*rj, k = k0+lk+8*rk: CrossAcc
// (cross_acc.h).  q / a are staged DC values of d at a time in LDS, as floats, with stride DC+1 (bank = (row + d) mod
// 32: conflict-free across rows, broadcast within a row).
// Staging: every load of a chunk is issued (clamped, hence unconditional, addresses) before the first LDS write;
// out-of-range elements are zeroed when written.  Written as `ok ? load : 0` the compiler emitted load / wait / write
// per row: 40 serialized round trips per chunk (18 of 38 us at 1517 x 40 x 40 x 50).  The NEXT chunk's loads are issued
// right after the LDS writes of the current one, so they are in flight behind its arithmetic.
// GATHER: the word ids of the tile's rows (gather_id clamps them) become table offsets once per wave, in LDS; the bias
// of a chunk's column is loaded with the chunk and added when the element is widened into LDS.
template <class S, int RJ, int RK, int MODE, bool GATHER>
__global__ __launch_bounds__(256) void cross_fwd_kernel(
    const S* __restrict__ q, const S* __restrict__ a, const float* __restrict__ norm0,
    const float* __restrict__ norm1, float* __restrict__ top, int N, int W1, int W2, int D, int tilesJ, int tilesK,
    CrossGather gt) {
  constexpr int TJ = 8 * RJ, TK = 8 * RK, DC = 32, LS = DC + 1;
  __shared__ float qs[4][TJ * LS];
  __shared__ float as[4][TK * LS];
  __shared__ int rowoff[4][GATHER ? TJ + TK : 1];   // gather: element offset of each tile row in the table
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long work = (long long)blockIdx.x * 4 + wave;
  const long long total = (long long)N * tilesJ * tilesK;
  const bool valid = work < total;
  const long long w = valid ? work : 0;
  const int n = (int)(w / (tilesJ * tilesK));
  const int rem = (int)(w % (tilesJ * tilesK));
  const int j0 = (rem / tilesK) * TJ, k0 = (rem % tilesK) * TK;
  const int lj = lane >> 3, lk = lane & 7;
  const S* qn = q + (size_t)n * W1 * D;
  const S* an = a + (size_t)n * W2 * D;

  CrossAcc<RJ, RK, MODE> acc;
  acc.clear();

  const int lrow = lane >> 5, lcol = lane & 31;
  S rq[TJ / 2], ra[TK / 2];
  float bv = 0.f;                                  // gather with a bias: the bias of this lane's column of the chunk
  const bool biased = GATHER && gt.bias != nullptr;
  if constexpr (GATHER) {                          // word ids of this tile's rows -> table offsets, once
    for (int r = lane; r < TJ + TK; r += 64) {
      const bool isq = r < TJ;
      const int rr = isq ? min(j0 + r, W1 - 1) : min(k0 + r - TJ, W2 - 1);
      const float id = isq ? gt.iq[(size_t)n * W1 + rr] : gt.ia[(size_t)n * W2 + rr];
      rowoff[wave][r] = gather_id(id, gt.K) * D;
    }
    wave_lds_sync();
  }
  auto fetch = [&](int d0) {
    const int col = min(d0 + lcol, D - 1);
    if constexpr (GATHER) {
#pragma unroll
      for (int r = 0; r < TJ; r += 2) rq[r / 2] = q[(size_t)rowoff[wave][r + lrow] + col];
#pragma unroll
      for (int r = 0; r < TK; r += 2) ra[r / 2] = a[(size_t)rowoff[wave][TJ + r + lrow] + col];
      if (biased) bv = gt.bias[col];
    } else {
#pragma unroll
      for (int r = 0; r < TJ; r += 2) rq[r / 2] = qn[(size_t)min(j0 + r + lrow, W1 - 1) * D + col];
#pragma unroll
      for (int r = 0; r < TK; r += 2) ra[r / 2] = an[(size_t)min(k0 + r + lrow, W2 - 1) * D + col];
    }
  };
  // a staged value: the widened element, plus the bias where there is one (never 0 + x: -0 keeps its sign without a bias)
  auto value = [&](S x) { return biased ? bv + (float)x : (float)x; };
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += DC) {
    const int dn = min(DC, D - d0);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TJ; r += 2)
      qs[wave][(r + lrow) * LS + lcol] = (valid && j0 + r + lrow < W1 && lcol < dn) ? value(rq[r / 2]) : 0.f;
#pragma unroll
    for (int r = 0; r < TK; r += 2)
      as[wave][(r + lrow) * LS + lcol] = (valid && k0 + r + lrow < W2 && lcol < dn) ? value(ra[r / 2]) : 0.f;
    __syncthreads();
    if (d0 + DC < D) fetch(d0 + DC);
    acc.accumulate(&qs[wave][lj * LS], &as[wave][lk * LS], LS, dn);
  }
  if (!valid) return;
  acc.finish(top, norm0, norm1, n, j0, k0, lj, lk, W1, W2);
}

// Forward, "pair image" staging for small D (the driver's default 50-d vectors): a wave owns one whole pair, W1 = 8*RJ
// and W2 = 8*RK exactly, and the (W1 x D) and (W2 x D) blocks of q and a -- contiguous in memory, a multiple of 16
// bytes (W % 8 == 0) -- are COPIED as they are, 16 bytes per lane per load, and widened into an fp32 image in LDS with
// row stride D (no padding, no chunking over d, no index arithmetic) that accumulate() reads.  Rows 8 apart must fall
// into different banks for its broadcast reads: gcd(D, 64) <= 8 (kImageD).  Against the generic staging at
// 1517 x 40 x 40 x 50 this replaces 80 4-byte load instructions and 80 predicated LDS writes per wave by 16 + 16.
// All loads of a batch are issued before its first LDS write.  Waves are independent: 2 per workgroup, 32 KB of LDS
// each.  D is a template parameter: with a run-time row stride the ten row addresses of accumulate() are recomputed per
// d step (VALU-bound loop: +15 % time); compiled in, they are immediate offsets.
// GATHER: image row r is table row id[r], assembled row by row, two elements per load (GridStorage::kGatherAlign),
// D / 2 per row.  Per batch: the ids of 8 + 8 vectors, then their 16 loads (and the bias pairs: floats of their own
// alignment, two 4-byte loads per pair), then the writes.
template <class S, int RJ, int RK, int MODE, int D, bool GATHER>
__global__ __launch_bounds__(128) void cross_fwd_image_kernel(
    const S* __restrict__ q, const S* __restrict__ a, const float* __restrict__ norm0,
    const float* __restrict__ norm1, float* __restrict__ top, int N, CrossGather gt) {
  typedef GridStorage<S> GS;
  constexpr int W1 = 8 * RJ, W2 = 8 * RK;
  constexpr int E = 16 / sizeof(S), F4 = E / 4;       // elements and image float4 per 16-byte vector
  constexpr int nq = W1 * D / E, na = W2 * D / E;     // exact: W1, W2 multiples of 8
  extern __shared__ float4 img4[];                    // [2 waves][(W1 + W2) * D / 4]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int work = blockIdx.x * 2 + wave;
  const bool valid = work < N;
  const int n = valid ? work : N - 1;
  float4* qs4 = img4 + (size_t)wave * F4 * (nq + na);
  float4* as4 = qs4 + F4 * nq;
  if constexpr (GATHER) {
    static_assert(D % 2 == 0, "the gather copies two elements per load");
    constexpr int R2 = D / 2;                      // vectors per row
    constexpr int NQ2 = W1 * R2, NA2 = W2 * R2, NMAX = NQ2 > NA2 ? NQ2 : NA2;
    float2* qs2 = reinterpret_cast<float2*>(qs4);
    float2* as2 = reinterpret_cast<float2*>(as4);
    const typename GS::Vec2* t2 = reinterpret_cast<const typename GS::Vec2*>(q);
    const float* iq = gt.iq + (size_t)n * W1;
    const float* ia = gt.ia + (size_t)n * W2;
    const bool biased = gt.bias != nullptr;
    for (int e0 = 0; e0 < NMAX; e0 += 512) {
      float idq[8], ida[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        idq[u] = iq[min(e, NQ2 - 1) / R2];
        ida[u] = ia[min(e, NA2 - 1) / R2];
      }
      typename GS::Vec2 rq[8], ra[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        rq[u] = t2[(size_t)gather_id(idq[u], gt.K) * R2 + min(e, NQ2 - 1) % R2];
        ra[u] = t2[(size_t)gather_id(ida[u], gt.K) * R2 + min(e, NA2 - 1) % R2];
      }
      float2 vq[8], va[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        vq[u] = GS::widen2(rq[u]);
        va[u] = GS::widen2(ra[u]);
      }
      if (biased) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = e0 + 64 * u + lane;
          const int cq = 2 * (min(e, NQ2 - 1) % R2), ca = 2 * (min(e, NA2 - 1) % R2);
          vq[u].x = gt.bias[cq] + vq[u].x; vq[u].y = gt.bias[cq + 1] + vq[u].y;
          va[u].x = gt.bias[ca] + va[u].x; va[u].y = gt.bias[ca + 1] + va[u].y;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        if (e < NQ2) qs2[e] = vq[u];
        if (e < NA2) as2[e] = va[u];
      }
    }
  } else {
    const typename GS::Vec16* qv = reinterpret_cast<const typename GS::Vec16*>(q + (size_t)n * W1 * D);
    const typename GS::Vec16* av = reinterpret_cast<const typename GS::Vec16*>(a + (size_t)n * W2 * D);
    // copy in batches of 4 + 4 loads
    for (int i0 = 0; i0 < (nq > na ? nq : na); i0 += 256) {
      typename GS::Vec16 rq[4], ra[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 64 * u + lane;
        rq[u] = qv[min(i, nq - 1)];
        ra[u] = av[min(i, na - 1)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 64 * u + lane;
        if (i < nq) GS::widen16(qs4 + F4 * i, rq[u]);
        if (i < na) GS::widen16(as4 + F4 * i, ra[u]);
      }
    }
  }
  wave_lds_sync();
  const int lj = lane >> 3, lk = lane & 7;
  CrossAcc<RJ, RK, MODE> acc;
  acc.clear();
  acc.accumulate(reinterpret_cast<const float*>(qs4) + lj * D, reinterpret_cast<const float*>(as4) + lk * D, D, D);
  if (!valid) return;
  acc.finish(top, norm0, norm1, n, 0, 0, lj, lk, W1, W2);
}

// Backward, plain: one workgroup per pair, for grids whose coefficient tables do not fit LDS.  A thread owns kNT
// neighbouring elements of the pair's dq block (two halves may lie in two rows), walks k ascending from 0 for each, and
// stores them together where the address allows; then the same for da, j ascending -- the reference's accumulation
// order (:209-223), so Euclidean is bit-exact: the reference's expression in either backward mode.  q/a/top rows of
// one n stay L1/L2-resident across the walk.
template <class S, int MODE>
__global__ __launch_bounds__(256) void cross_bwd_plain_kernel(
    const S* __restrict__ q, const S* __restrict__ a, const float* __restrict__ top,
    const float* __restrict__ top_diff, const float* __restrict__ norm0, const float* __restrict__ norm1,
    S* __restrict__ dq, S* __restrict__ da, int W1, int W2, int D) {
  typedef GridStorage<S> GS;
  constexpr int NT = GS::kNT;
  const int n = blockIdx.x;
  const S* qn = q + (size_t)n * W1 * D;
  const S* an = a + (size_t)n * W2 * D;
  const float* Tn = top + (size_t)n * W1 * W2;
  const float* gn = top_diff + (size_t)n * W1 * W2;
  S* dqn = dq + (size_t)n * W1 * D;
  S* dan = da + (size_t)n * W2 * D;
  const float* n0n = MODE == 0 ? norm0 + (size_t)n * W1 : nullptr;
  const float* n1n = MODE == 0 ? norm1 + (size_t)n * W2 : nullptr;

  for (int e0 = NT * threadIdx.x; e0 < W1 * D; e0 += NT * 256) {
    float out[NT] = {};
    const int cnt = NT == 1 ? 1 : min(NT, W1 * D - e0);
    for (int u = 0; u < cnt; ++u) {
      const int e = e0 + u, j = e / D, d = e - j * D;
      const float qv = (float)qn[e];
      float acc = 0.f;
      if (MODE == 1) {
        for (int k = 0; k < W2; ++k) {
          const EuclidCoef kc = euclid_coef(Tn[j * W2 + k], gn[j * W2 + k]);
          acc += euclid_tt_exact(kc.c, kc.den, qv - (float)an[(size_t)k * D + d]);
        }
      } else {
        const float nrm0 = n0n[j];
        for (int k = 0; k < W2; ++k)
          acc += cosine_term_div(gn[j * W2 + k], nrm0, n1n[k], Tn[j * W2 + k], nrm0 * nrm0, (float)an[(size_t)k * D + d], qv);
      }
      out[u] = acc;
    }
    GS::template store<NT>(dqn + e0, out, cnt);
  }
  for (int e0 = NT * threadIdx.x; e0 < W2 * D; e0 += NT * 256) {
    float out[NT] = {};
    const int cnt = NT == 1 ? 1 : min(NT, W2 * D - e0);
    for (int u = 0; u < cnt; ++u) {
      const int e = e0 + u, k = e / D, d = e - k * D;
      const float av = (float)an[e];
      float acc = 0.f;
      if (MODE == 1) {
        for (int j = 0; j < W1; ++j) {
          const EuclidCoef kc = euclid_coef(Tn[j * W2 + k], gn[j * W2 + k]);
          acc += -euclid_tt_exact(kc.c, kc.den, (float)qn[(size_t)j * D + d] - av);
        }
      } else {
        const float nrm1 = n1n[k];
        for (int j = 0; j < W1; ++j)
          acc += cosine_term_div(gn[j * W2 + k], n0n[j], nrm1, Tn[j * W2 + k], nrm1 * nrm1, (float)qn[(size_t)j * D + d], av);
      }
      out[u] = acc;
    }
    GS::template store<NT>(dan + e0, out, cnt);
  }
}

// Backward, tiled (the fast path when the per-pair tables fit LDS): one workgroup per (pair, kBwdDC-wide d chunk), or
// two with `split` -- blockIdx.x = (n * nchunks + chunk) * 2 + pass, the dq pass and the da pass apart (twice the
// parallelism; small batches); otherwise one workgroup does both and the tables are built once (large batches).
//   * the per-(j, k) coefficient tables are built ONCE per workgroup in LDS -- Euclid: c, den, 1/den (reference
//     rounding) or c, fl32(1/den) (fp32 arithmetic, include/mms.h); cosine: g and cosine_factors;
//   * the q / a chunk is staged in LDS as floats (stride 33: conflict-free): eight unconditional (clamped) loads per
//     thread in flight before the first LDS write -- a rolled `ok ? load : 0` loop paid one memory round trip per
//     iteration;
//   * a thread owns NT neighbouring d of one row j of dq and walks k ascending from 0, then NT d of one row k of da,
//     j ascending from 0 (:209-223): the coefficients of a (j, k) are read once per NT terms, and the NT elements
//     leave together where the storage packs them.  NT = 4 in the fp32 arithmetic (6 LDS reads per 4 terms instead
//     of 12: that loop is LDS-bandwidth-bound), GridStorage::kNT otherwise.  The walk reads the row's NT operands
//     first and names the coefficient reads inside the loop over the NT terms (the compiler merges them into one read
//     per (j, k)): hoisted in front of that loop, den is live on every path, and at NT = 1 the compiler then turns
//     euclid_tt's rare exact division from a branch into a select -- a double division per term, 183 -> 281 us at
//     1517 x 40 x 40 x 50 with reference rounding.
// Euclid with EXACT stays bit-exact (euclid_tt's self-checking reciprocal path).  Cosine multiplies by precomputed
// reciprocals instead of dividing per term: it is held to 1e-5 like everything that is BLAS-ordered in the reference.
constexpr int kBwdDC = 32;

template <class S, int MODE, bool EXACT>
__global__ __launch_bounds__(256) void cross_bwd_tiled_kernel(
    const S* __restrict__ q, const S* __restrict__ a, const float* __restrict__ top,
    const float* __restrict__ top_diff, const float* __restrict__ norm0, const float* __restrict__ norm1,
    S* __restrict__ dq, S* __restrict__ da, int W1, int W2, int D, int nchunks, int split) {
  typedef GridStorage<S> GS;
  extern __shared__ double lds_d[];
  constexpr int DC = kBwdDC, LS = DC + 1;
  constexpr int NT = (MODE == 1 && !EXACT) ? 4 : GS::kNT, PER = DC / NT;
  const int bid = split ? (blockIdx.x >> 1) : blockIdx.x;
  const bool do_dq = !split || (blockIdx.x & 1) == 0, do_da = !split || (blockIdx.x & 1) == 1;
  const int n = bid / nchunks, chunk = bid % nchunks;
  const int d0 = chunk * DC, dn = min(DC, D - d0);
  const int JK = W1 * W2;
  // carve (cross_bwd_tiled_lds): doubles first (8-byte aligned), then floats
  double* t_den = lds_d;                                // Euclid, reference rounding: [JK]
  double* t_rcp = lds_d + (MODE == 1 ? JK : 0);         // Euclid, reference rounding: [JK]
  float* fbase = reinterpret_cast<float*>(lds_d + (MODE == 1 ? 2 * JK : 0));
  float* t_c = fbase;                                   // Euclid: c       cosine: g
  float* t_i01 = fbase + JK;                            // cosine: 1/n0/n1
  float* t_b1 = fbase + 2 * JK;                         // cosine: T/n0^2
  float* t_b2 = fbase + 3 * JK;                         // cosine: T/n1^2
  float* qs = fbase + (MODE == 1 ? JK : 4 * JK);
  float* as = qs + W1 * LS;
  float* t_r = reinterpret_cast<float*>(lds_d);         // Euclid, fp32 arithmetic: fl32(1/den) in place of the doubles

  const S* qn = q + (size_t)n * W1 * D;
  const S* an = a + (size_t)n * W2 * D;
  const float* Tn = top + (size_t)n * JK;
  const float* gn = top_diff + (size_t)n * JK;

  for (int e0 = threadIdx.x; MODE == 1 && e0 < JK; e0 += 256 * 8) {
    float tv[8], gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int e = min(e0 + 256 * u, JK - 1); tv[u] = Tn[e]; gv[u] = gn[e]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 256 * u;
      if (e >= JK) break;
      const EuclidCoef k = euclid_coef(tv[u], gv[u]);
      t_c[e] = k.c;
      if (EXACT) { t_den[e] = k.den; t_rcp[e] = k.rcp; } else { t_r[e] = (float)k.rcp; }
    }
  }
  for (int e = threadIdx.x; MODE == 0 && e < JK; e += 256) {
    const int j = e / W2, kk = e - j * W2;
    const CosineFactors f = cosine_factors(Tn[e], norm0[(size_t)n * W1 + j], norm1[(size_t)n * W2 + kk]);
    t_c[e] = gn[e];
    t_i01[e] = f.inv01;
    t_b1[e] = f.cq;
    t_b2[e] = f.ca;
  }
  auto stage = [&](const S* src, float* dst, int W) {
    for (int base = 0; base < W * DC; base += 256 * 8) {
      S v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + threadIdx.x + 256 * u;
        v[u] = src[(size_t)min(e >> 5, W - 1) * D + min(d0 + (e & 31), D - 1)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + threadIdx.x + 256 * u;
        if (e < W * DC) dst[(e >> 5) * LS + (e & 31)] = (e & 31) < dn ? (float)v[u] : 0.f;
      }
    }
  };
  static_assert(DC == 32, "stage() splits an element index into row e >> 5 and column e & 31");
  stage(qn, qs, W1);
  stage(an, as, W2);
  __syncthreads();

  S* dqn = dq + (size_t)n * W1 * D;
  S* dan = da + (size_t)n * W2 * D;
  for (int e = threadIdx.x; do_dq && e < W1 * PER; e += 256) {
    const int j = e / PER, dd0 = (e % PER) * NT;
    if (dd0 >= dn) continue;
    float qv[NT], acc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) { qv[u] = qs[j * LS + dd0 + u]; acc[u] = 0.f; }
    for (int k = 0; k < W2; ++k) {
      const int t = j * W2 + k;
      float ar[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) ar[u] = as[k * LS + dd0 + u];
      if (MODE == 1 && EXACT) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          EuclidCoef kc;
          kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
          acc[u] += euclid_tt(kc, qv[u] - ar[u]);
        }
      } else if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += euclid_tt_f32(t_c[t], t_r[t], qv[u] - ar[u]);
      } else {
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += cosine_term_fac(t_c[t], t_i01[t], t_b1[t], ar[u], qv[u]);
      }
    }
    GS::template store<NT>(dqn + (size_t)j * D + d0 + dd0, acc, min(NT, dn - dd0));
  }
  for (int e = threadIdx.x; do_da && e < W2 * PER; e += 256) {
    const int k = e / PER, dd0 = (e % PER) * NT;
    if (dd0 >= dn) continue;
    float av[NT], acc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) { av[u] = as[k * LS + dd0 + u]; acc[u] = 0.f; }
    for (int j = 0; j < W1; ++j) {
      const int t = j * W2 + k;
      float qr[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) qr[u] = qs[j * LS + dd0 + u];
      if (MODE == 1 && EXACT) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          EuclidCoef kc;
          kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
          acc[u] += -euclid_tt(kc, qr[u] - av[u]);
        }
      } else if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += -euclid_tt_f32(t_c[t], t_r[t], qr[u] - av[u]);
      } else {
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += cosine_term_fac(t_c[t], t_i01[t], t_b2[t], qr[u], av[u]);
      }
    }
    GS::template store<NT>(dan + (size_t)k * D + d0 + dd0, acc, min(NT, dn - dd0));
  }
}

// ================================ launch plan ================================
// Host side.  Each decision and each of its literals is written once, here; the storage enters through GridStorage.

constexpr int kMaxTile = 5;               // largest register tile per lane: 8 * 5 = 40 rows of q or of a
constexpr int kFill = 1024;               // waves (forward) or workgroups (tiled backward) that occupy the chip
constexpr int kImageD = 50;               // the driver's default embedding width (do_trec_qa_clean.py -d 50)
constexpr unsigned kLdsBytes = 64 * 1024; // dynamic LDS a launch may ask for

// The 25 instances K<S, RJ, RK, ...> of a forward kernel as a table indexed [rj - 1][rk - 1] (the idiom of MMS_NIT4):
//   static constexpr decltype(&K<S, 1, 1, ...>) kernels[kMaxTile][kMaxTile] = MMS_TILES5X5(K, S, ...);
#define MMS_TILES5(K, S, J, ...) \
  {K<S, J, 1, __VA_ARGS__>, K<S, J, 2, __VA_ARGS__>, K<S, J, 3, __VA_ARGS__>, K<S, J, 4, __VA_ARGS__>, K<S, J, 5, __VA_ARGS__>}
#define MMS_TILES5X5(K, S, ...)                                                                         \
  {MMS_TILES5(K, S, 1, __VA_ARGS__), MMS_TILES5(K, S, 2, __VA_ARGS__), MMS_TILES5(K, S, 3, __VA_ARGS__), \
   MMS_TILES5(K, S, 4, __VA_ARGS__), MMS_TILES5(K, S, 5, __VA_ARGS__)}
static_assert(kMaxTile == 5, "MMS_TILES5X5 lists the tiles 1 .. 5");

// Register tile per lane: as large as possible (fewer LDS reads per flop) while the launch still has enough waves to
// occupy the chip (small N: smaller tiles, more waves).
struct CrossTile {
  int rj, rk, tilesJ, tilesK;
};
inline CrossTile cross_fwd_tile(int N, int W1, int W2) {
  auto r_cap = [](int w, int cap) { int r = (w + 7) / 8; return r > cap ? cap : r; };
  CrossTile t{1, 1, 1, 1};
  for (int cap = kMaxTile; cap >= 1; --cap) {
    t.rj = r_cap(W1, cap); t.rk = r_cap(W2, cap);
    t.tilesJ = (W1 + 8 * t.rj - 1) / (8 * t.rj); t.tilesK = (W2 + 8 * t.rk - 1) / (8 * t.rk);
    if ((long long)N * t.tilesJ * t.tilesK >= kFill) break;
  }
  return t;
}

// The pair image (cross_fwd_image_kernel) needs whole 8-row tiles, a wave per SIMD's worth of pairs, the width it is
// compiled for, two images in LDS and the alignment of its loads: 16 bytes from both operands, or, gathered (q == a ==
// the table), GridStorage::kGatherAlign.
template <class S, bool GATHER>
inline bool cross_fwd_image_ok(int N, int W1, int W2, int D, const S* q, const S* a) {
  static_assert(kImageD % 2 == 0 && kImageD % 16 != 0, "rows 8 apart in different banks: gcd(D, 64) <= 8");
  const size_t img = (size_t)(W1 + W2) * D * sizeof(float);
  const uintptr_t need = (GATHER ? GridStorage<S>::kGatherAlign : 16) - 1;
  return W1 % 8 == 0 && W2 % 8 == 0 && W1 / 8 <= kMaxTile && W2 / 8 <= kMaxTile && N >= kFill && D == kImageD &&
         (reinterpret_cast<uintptr_t>(q) & need) == 0 && (reinterpret_cast<uintptr_t>(a) & need) == 0 && 2 * img <= kLdsBytes;
}

// GATHER: q == a == the table and gt names the ids
template <class S, int MODE, bool GATHER>
inline void launch_cross_fwd(const S* q, const S* a, const float* n0, const float* n1, float* top, int N, int W1, int W2,
                             int D, hipStream_t s, CrossGather gt) {
  if (cross_fwd_image_ok<S, GATHER>(N, W1, W2, D, q, a)) {
    static constexpr decltype(&cross_fwd_image_kernel<S, 1, 1, MODE, kImageD, GATHER>) image[kMaxTile][kMaxTile] =
        MMS_TILES5X5(cross_fwd_image_kernel, S, MODE, kImageD, GATHER);
    const size_t img = (size_t)(W1 + W2) * D * sizeof(float);
    hipLaunchKernelGGL(image[W1 / 8 - 1][W2 / 8 - 1], dim3((unsigned)((N + 1) / 2)), dim3(128), 2 * img, s, q, a, n0, n1,
                       top, N, gt);
    return;
  }
  static constexpr decltype(&cross_fwd_kernel<S, 1, 1, MODE, GATHER>) generic[kMaxTile][kMaxTile] =
      MMS_TILES5X5(cross_fwd_kernel, S, MODE, GATHER);
  const CrossTile t = cross_fwd_tile(N, W1, W2);
  const long long work = (long long)N * t.tilesJ * t.tilesK;
  hipLaunchKernelGGL(generic[t.rj - 1][t.rk - 1], dim3((unsigned)((work + 3) / 4)), dim3(256), 0, s, q, a, n0, n1, top, N,
                     W1, W2, D, t.tilesJ, t.tilesK, gt);
}

// The word-grid forward: cosine computes the norms of q's rows and of a's first.  GATHER: q and a are the embedding
// table and the Embed gather is fused in.
template <class S, bool GATHER>
inline void cross_forward(int mode, int N, int W1, int W2, int D, const S* q, const S* a, float* top, float* norm0,
                          float* norm1, hipStream_t s, CrossGather gt) {
  if (mode == 1) {
    launch_cross_fwd<S, 1, GATHER>(q, a, nullptr, nullptr, top, N, W1, W2, D, s, gt);
    return;
  }
  const long long r0 = (long long)N * W1, r1 = (long long)N * W2;
  hipLaunchKernelGGL(row_norm_kernel<S>, dim3((unsigned)((r0 + 3) / 4)), dim3(256), 0, s, q, norm0, r0, D, gt.iq, gt.K, gt.bias);
  hipLaunchKernelGGL(row_norm_kernel<S>, dim3((unsigned)((r1 + 3) / 4)), dim3(256), 0, s, a, norm1, r1, D, gt.ia, gt.K, gt.bias);
  launch_cross_fwd<S, 0, GATHER>(q, a, norm0, norm1, top, N, W1, W2, D, s, gt);
}
constexpr CrossGather kNoGather{nullptr, nullptr, 0, nullptr};

// dynamic LDS of cross_bwd_tiled_kernel: the tables, then the staged q / a chunk
inline size_t cross_bwd_tiled_lds(int mode, int W1, int W2) {
  const size_t JK = (size_t)W1 * W2;
  const size_t tables = mode == 1 ? JK * (8 + 8 + 4) : JK * 16;
  return tables + (size_t)(W1 + W2) * (kBwdDC + 1) * sizeof(float) + 16;
}

// The lane kernel (Euclid, many pairs of narrow grids) exists for fp32 storage alone: simcross_cross.hip specialises
// this for float.  Returns whether it served the call.
template <class S>
inline bool launch_cross_bwd_lane(int N, int W1, int W2, int D, const S* q, const S* a, const float* top,
                                  const float* top_diff, S* dq, S* da, bool exact, hipStream_t s) {
  return false;
}

// The word-grid backward: lane kernel, else tiled while the tables fit LDS, else plain.  `exact`:
// euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE, read once by the entry point.
template <class S>
inline void cross_backward(int mode, int N, int W1, int W2, int D, const S* q, const S* a, const float* top,
                           const float* top_diff, const float* norm0, const float* norm1, S* dq, S* da, bool exact,
                           hipStream_t s) {
  const int nchunks = (D + kBwdDC - 1) / kBwdDC;
  const size_t lds = cross_bwd_tiled_lds(mode, W1, W2);
  if (mode == 1) norm0 = norm1 = nullptr;                          // Euclid caches no norms
  if (mode == 1 && launch_cross_bwd_lane<S>(N, W1, W2, D, q, a, top, top_diff, dq, da, exact, s)) return;
  if (lds <= kLdsBytes && 2LL * N * nchunks <= 0x7fffffffLL) {
    const int split = ((long long)N * nchunks < kFill) ? 1 : 0;    // fill the chip when the batch is small
    const unsigned grid = (unsigned)((split ? 2LL : 1LL) * N * nchunks);
    // cosine has one arithmetic: its instance is <0, true>
    const auto k = mode == 0 ? cross_bwd_tiled_kernel<S, 0, true>
                   : exact   ? cross_bwd_tiled_kernel<S, 1, true> : cross_bwd_tiled_kernel<S, 1, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, q, a, top, top_diff, norm0, norm1, dq, da, W1, W2, D, nchunks,
                       split);
  } else {
    hipLaunchKernelGGL((mode == 1 ? cross_bwd_plain_kernel<S, 1> : cross_bwd_plain_kernel<S, 0>), dim3(N), dim3(256), 0,
                       s, q, a, top, top_diff, norm0, norm1, dq, da, W1, W2, D);
  }
}

#undef MMS_TILES5X5
#undef MMS_TILES5

}  // namespace mms
#endif  // MMS_CROSS_GRID_H_
