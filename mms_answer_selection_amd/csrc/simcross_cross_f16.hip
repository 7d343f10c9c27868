// csrc/simcross_cross_f16.hip -- fp16-STORAGE SimCross dist_mode 0 (cosine) and 1 (Euclidean) on W1 x W2 word grids
// (mms_simcross_forward_f16 / _backward_f16 / _forward_backward_f16, and mms_embed_simcross_forward_f16, the forward
// straight from word ids and a half embedding table): q, a, dq, da are IEEE halves in HBM; top, top_diff and the norms fp32.  The arithmetic is that of simcross_cross.hip on the exactly-widened inputs: a half
// becomes a float when it is written to LDS (forward, tiled backward) or right after its load (plain backward, norms),
// every sum is fp32 in the reference's order (sim_cross_layer.cpp:96-139, 208-250), and a gradient element is rounded
// ONCE, RNE, when it is stored (v_cvt_f16_f32: overflow gives +-Inf).  The forward's register tile and T are CrossAcc
// (cross_acc.h), the backward terms euclid_math.h / cosine_math.h: no arithmetic is defined here.
//
// Alignment: halves are loaded and stored one by one unless a wider access has tested its own preconditions -- the
// pair image copies 16 bytes per lane (cross_fwd_image_ok_f16: aligned16 of both bases, D = 50) or, gathered from a
// table, 4 bytes (a 4-byte aligned table: its 100-byte rows promise no more), the backward packs 2 or 4 neighbouring d
// of a row into one store where the address allows (store_halves).  Any D >= 1 and any 2-byte aligned operand is served.
//
// The Embed gather (cross_gather.h) is the template option GATHER of the two forward kernels and a run-time one of the
// norm kernel: q and a are then both the table, row j of pair n is table row gather_id(iq[n*W1 + j]), and a row value
// is bias[d] + widen(table[id][d]) -- one fp32 add after the widening -- or the widened half alone without a bias.
//
// Compiled with -ffp-contract=off like every source of the library.
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

// L2 norms of `rows` half rows of length D: one wave per row, the lane order and the wave sum of row_norm_kernel
// (simcross_cross.hip), so the norms carry the bits of the fp32 call on the widened rows.
// index != nullptr: row `row` is table row index[row] of x (K rows), and ebias (or nullptr) is added before squaring.
__global__ __launch_bounds__(256) void row_norm_f16_kernel(const _Float16* __restrict__ x, float* __restrict__ nrm,
                                                           long long rows, int D, const float* __restrict__ index, int K,
                                                           const float* __restrict__ ebias) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const _Float16* r = x + (index ? (long long)gather_id(index[row], K) : row) * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) { const float v = ebias ? ebias[i] + (float)r[i] : (float)r[i]; s += v * v; }
  s = wave_sum(s);
  if (lane == 0) nrm[row] = sqrtf(s);
}

// Forward, generic staging: cross_fwd_kernel (simcross_cross.hip) with halves in the staging registers.  One wave per
// (pair, j-tile, k-tile); q / a are staged DC values of d at a time in LDS, as floats, stride DC + 1.  Every load of a
// chunk is issued (clamped, hence unconditional, addresses) before the first LDS write, and the next chunk's loads
// right after the writes of the current one -- `ok ? load : 0` costs one memory round trip per row.
// GATHER: the word ids of the tile's rows become table offsets once per wave, in LDS, as in cross_fwd_kernel; the bias
// of a chunk's column is loaded with the chunk and added when the half is widened.
template <int RJ, int RK, int MODE, bool GATHER>
__global__ __launch_bounds__(256) void cross_fwd_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ norm0,
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
  const _Float16* qn = q + (size_t)n * W1 * D;
  const _Float16* an = a + (size_t)n * W2 * D;

  CrossAcc<RJ, RK, MODE> acc;
  acc.clear();

  const int lrow = lane >> 5, lcol = lane & 31;
  _Float16 rq[TJ / 2], ra[TK / 2];
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
  // a staged value: the widened half, plus the bias where there is one (never 0 + x: -0 keeps its sign without a bias)
  auto value = [&](_Float16 h) { return biased ? bv + (float)h : (float)h; };
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

// Forward, pair image (cross_fwd_image_kernel): a wave owns one whole pair, W1 = 8*RJ and W2 = 8*RK exactly.  The
// W1*D and W2*D halves of the pair are contiguous and a multiple of 16 bytes (W % 8 == 0), so with 16-byte aligned
// bases they are copied 8 halves per lane per load and widened into the fp32 image (row stride D floats) that
// accumulate() reads.  All loads of a batch are issued before its first LDS write.  2 waves per workgroup.
// GATHER: image row r is table row id[r], assembled row by row.  A table row is D halves = 100 bytes, so a 4-byte
// aligned table promises 4-byte aligned rows and no more: the copy runs in half2, D / 2 per row, widened to the float2
// of the same image.  Per batch: the ids of 8 + 8 elements, then their 16 loads (and the bias pairs), then the writes.
template <int RJ, int RK, int MODE, int D, bool GATHER>
__global__ __launch_bounds__(128) void cross_fwd_image_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ norm0,
    const float* __restrict__ norm1, float* __restrict__ top, int N, CrossGather gt) {
  constexpr int W1 = 8 * RJ, W2 = 8 * RK;
  constexpr int nq8 = W1 * D / 8, na8 = W2 * D / 8;   // exact: W1, W2 multiples of 8
  extern __shared__ float4 img4_f16[];                // [2 waves][(W1 + W2) * D / 4]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int work = blockIdx.x * 2 + wave;
  const bool valid = work < N;
  const int n = valid ? work : N - 1;
  float4* qs4 = img4_f16 + (size_t)wave * 2 * (nq8 + na8);
  float4* as4 = qs4 + 2 * nq8;
  if constexpr (GATHER) {
    static_assert(D % 2 == 0, "the gather copies half2");
    constexpr int R2 = D / 2;                      // half2 per row
    constexpr int NQ2 = W1 * R2, NA2 = W2 * R2, NMAX = NQ2 > NA2 ? NQ2 : NA2;
    float2* qs2 = reinterpret_cast<float2*>(qs4);
    float2* as2 = reinterpret_cast<float2*>(as4);
    const half2v* t2 = reinterpret_cast<const half2v*>(q);
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
      half2v rq[8], ra[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        rq[u] = t2[(size_t)gather_id(idq[u], gt.K) * R2 + min(e, NQ2 - 1) % R2];
        ra[u] = t2[(size_t)gather_id(ida[u], gt.K) * R2 + min(e, NA2 - 1) % R2];
      }
      float2 vq[8], va[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        vq[u] = make_float2((float)rq[u][0], (float)rq[u][1]);
        va[u] = make_float2((float)ra[u][0], (float)ra[u][1]);
      }
      if (biased) {                                // the bias is floats of its own alignment: two 4-byte loads per pair
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
    const half8* q8 = reinterpret_cast<const half8*>(q + (size_t)n * W1 * D);
    const half8* a8 = reinterpret_cast<const half8*>(a + (size_t)n * W2 * D);
    auto widen = [](float4* dst, const half8& h) {
      dst[0] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
      dst[1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
    };
    for (int i0 = 0; i0 < (nq8 > na8 ? nq8 : na8); i0 += 256) {
      half8 rq[4], ra[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 64 * u + lane;
        rq[u] = q8[min(i, nq8 - 1)];
        ra[u] = a8[min(i, na8 - 1)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 64 * u + lane;
        if (i < nq8) widen(qs4 + 2 * i, rq[u]);
        if (i < na8) widen(as4 + 2 * i, ra[u]);
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

// Backward, plain: one workgroup per pair, for grids whose coefficient tables do not fit LDS.  A thread owns two
// neighbouring elements of the pair's dq block (they may lie in two rows), walks k ascending from 0 for each
// (:209-223), and stores them as one half2 where the address allows; then the same for da, j ascending.  Euclid is
// the reference's expression in either backward mode, as in cross_bwd_kernel.
template <int MODE>
__global__ __launch_bounds__(256) void cross_bwd_plain_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ top,
    const float* __restrict__ top_diff, const float* __restrict__ norm0, const float* __restrict__ norm1,
    _Float16* __restrict__ dq, _Float16* __restrict__ da, int W1, int W2, int D) {
  const int n = blockIdx.x;
  const _Float16* qn = q + (size_t)n * W1 * D;
  const _Float16* an = a + (size_t)n * W2 * D;
  const float* Tn = top + (size_t)n * W1 * W2;
  const float* gn = top_diff + (size_t)n * W1 * W2;
  _Float16* dqn = dq + (size_t)n * W1 * D;
  _Float16* dan = da + (size_t)n * W2 * D;
  const float* n0n = MODE == 0 ? norm0 + (size_t)n * W1 : nullptr;
  const float* n1n = MODE == 0 ? norm1 + (size_t)n * W2 : nullptr;

  for (int e0 = 2 * threadIdx.x; e0 < W1 * D; e0 += 512) {
    float out[2] = {0.f, 0.f};
    const int cnt = min(2, W1 * D - e0);
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
          acc += cosine_grad_div(gn[j * W2 + k], nrm0, n1n[k], Tn[j * W2 + k], nrm0 * nrm0, (float)an[(size_t)k * D + d], qv);
      }
      out[u] = acc;
    }
    store_halves<2>(dqn + e0, out, cnt);
  }
  for (int e0 = 2 * threadIdx.x; e0 < W2 * D; e0 += 512) {
    float out[2] = {0.f, 0.f};
    const int cnt = min(2, W2 * D - e0);
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
          acc += cosine_grad_div(gn[j * W2 + k], n0n[j], nrm1, Tn[j * W2 + k], nrm1 * nrm1, (float)qn[(size_t)j * D + d], av);
      }
      out[u] = acc;
    }
    store_halves<2>(dan + e0, out, cnt);
  }
}

// Backward, tiled (cross_bwd_tiled_kernel): one workgroup per (pair, 32-wide d chunk), or two with `split` (the dq pass
// and the da pass apart: small batches).
//   * the per-(j, k) coefficient tables are built once per workgroup in LDS -- Euclid: c, den, 1/den (reference
//     rounding) or c, fl32(1/den) (fp32 arithmetic); cosine: g and cosine_factors;
//   * the q / a chunk is staged in LDS as floats, stride 33, all loads of a batch before its first LDS write;
//   * a thread owns NT neighbouring d of one row j of dq and walks k ascending from 0, then NT d of one row k of da,
//     j ascending from 0 (:209-223): the coefficients of a (j, k) are read once per NT terms, and the NT halves
//     leave as one store where the address allows.  NT = 4 in the fp32 arithmetic (LDS-bandwidth-bound loop),
//     2 otherwise.
constexpr int kBwdDC16 = 32;

template <int MODE, bool EXACT>
__global__ __launch_bounds__(256) void cross_bwd_tiled_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ top,
    const float* __restrict__ top_diff, const float* __restrict__ norm0, const float* __restrict__ norm1,
    _Float16* __restrict__ dq, _Float16* __restrict__ da, int W1, int W2, int D, int nchunks, int split) {
  extern __shared__ double lds_d16[];
  constexpr int DC = kBwdDC16, LS = DC + 1;
  constexpr int NT = (MODE == 1 && !EXACT) ? 4 : 2, PER = DC / NT;
  const int bid = split ? (blockIdx.x >> 1) : blockIdx.x;
  const bool do_dq = !split || (blockIdx.x & 1) == 0, do_da = !split || (blockIdx.x & 1) == 1;
  const int n = bid / nchunks, chunk = bid % nchunks;
  const int d0 = chunk * DC, dn = min(DC, D - d0);
  const int JK = W1 * W2;
  // carve (cross_bwd_tiled_lds_f16): doubles first, then floats
  double* t_den = lds_d16;                              // Euclid, reference rounding: [JK]
  double* t_rcp = lds_d16 + (MODE == 1 ? JK : 0);       // Euclid, reference rounding: [JK]
  float* fbase = reinterpret_cast<float*>(lds_d16 + (MODE == 1 ? 2 * JK : 0));
  float* t_c = fbase;                                   // Euclid: c       cosine: g
  float* t_i01 = fbase + JK;                            // cosine: 1/n0/n1
  float* t_b1 = fbase + 2 * JK;                         // cosine: T/n0^2
  float* t_b2 = fbase + 3 * JK;                         // cosine: T/n1^2
  float* qs = fbase + (MODE == 1 ? JK : 4 * JK);
  float* as = qs + W1 * LS;
  float* t_r = reinterpret_cast<float*>(lds_d16);       // Euclid, fp32 arithmetic: fl32(1/den) in place of the doubles

  const _Float16* qn = q + (size_t)n * W1 * D;
  const _Float16* an = a + (size_t)n * W2 * D;
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
  auto stage = [&](const _Float16* src, float* dst, int W) {
    for (int base = 0; base < W * DC; base += 256 * 8) {
      _Float16 v[8];
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
  stage(qn, qs, W1);
  stage(an, as, W2);
  __syncthreads();

  _Float16* dqn = dq + (size_t)n * W1 * D;
  _Float16* dan = da + (size_t)n * W2 * D;
  for (int e = threadIdx.x; do_dq && e < W1 * PER; e += 256) {
    const int j = e / PER, dd0 = (e % PER) * NT;
    if (dd0 >= dn) continue;
    float qv[NT], acc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) { qv[u] = qs[j * LS + dd0 + u]; acc[u] = 0.f; }
    for (int k = 0; k < W2; ++k) {
      const int t = j * W2 + k;
      const float* ar = as + k * LS + dd0;
      if (MODE == 1 && EXACT) {
        EuclidCoef kc;
        kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += euclid_tt(kc, qv[u] - ar[u]);
      } else if (MODE == 1) {
        const float c = t_c[t], r = t_r[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += euclid_tt_f32(c, r, qv[u] - ar[u]);
      } else {
        const float g = t_c[t], i01 = t_i01[t], b = t_b1[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += cosine_grad_fac(g, i01, b, ar[u], qv[u]);
      }
    }
    store_halves<NT>(dqn + (size_t)j * D + d0 + dd0, acc, min(NT, dn - dd0));
  }
  for (int e = threadIdx.x; do_da && e < W2 * PER; e += 256) {
    const int k = e / PER, dd0 = (e % PER) * NT;
    if (dd0 >= dn) continue;
    float av[NT], acc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) { av[u] = as[k * LS + dd0 + u]; acc[u] = 0.f; }
    for (int j = 0; j < W1; ++j) {
      const int t = j * W2 + k;
      const float* qr = qs + j * LS + dd0;
      if (MODE == 1 && EXACT) {
        EuclidCoef kc;
        kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += -euclid_tt(kc, qr[u] - av[u]);
      } else if (MODE == 1) {
        const float c = t_c[t], r = t_r[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += -euclid_tt_f32(c, r, qr[u] - av[u]);
      } else {
        const float g = t_c[t], i01 = t_i01[t], b = t_b2[t];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] += cosine_grad_fac(g, i01, b, qr[u], av[u]);
      }
    }
    store_halves<NT>(dan + (size_t)k * D + d0 + dd0, acc, min(NT, dn - dd0));
  }
}

// dynamic LDS of cross_bwd_tiled_f16_kernel: the tables, then the staged q / a chunk
static size_t cross_bwd_tiled_lds_f16(int mode, int W1, int W2) {
  const size_t JK = (size_t)W1 * W2;
  const size_t tables = mode == 1 ? JK * (8 + 8 + 4) : JK * 16;
  return tables + (size_t)(W1 + W2) * (kBwdDC16 + 1) * sizeof(float) + 16;
}

// ================================ dispatch ==================================
// tests/f16_cross_model.py restates every decision below, one function each.

constexpr int kImageD16 = 50;   // the driver's default embedding width (do_trec_qa_clean.py -d 50)

// the pair image needs whole 8-row tiles, two images in 64 KB and the alignment of its loads: 16 bytes from both
// operands, or, gathered (q == a == the table), the 4 bytes that a 4-byte aligned table's 100-byte rows keep
static bool cross_fwd_image_ok_f16(int N, int W1, int W2, int D, const void* q, const void* a, bool gather) {
  const size_t img = (size_t)(W1 + W2) * D * sizeof(float);
  const uintptr_t need = gather ? 3u : 15u;
  return W1 % 8 == 0 && W2 % 8 == 0 && W1 / 8 <= 5 && W2 / 8 <= 5 && N >= 1024 && D == kImageD16 &&
         (reinterpret_cast<uintptr_t>(q) & need) == 0 && (reinterpret_cast<uintptr_t>(a) & need) == 0 && 2 * img <= 64 * 1024;
}

// GATHER: q == a == the table and gt names the ids (embed_simcross_forward_f16)
template <int MODE, bool GATHER>
static void launch_cross_fwd_f16(const _Float16* q, const _Float16* a, const float* n0, const float* n1, float* top,
                                 int N, int W1, int W2, int D, hipStream_t s, CrossGather gt) {
  // register tile per lane as in launch_cross_fwd: as large as possible while the launch has 1024 waves
  auto r_cap = [](int w, int cap) { int r = (w + 7) / 8; return r > cap ? cap : r; };
  int rj = 1, rk = 1, tilesJ = 1, tilesK = 1;
  for (int cap = 5; cap >= 1; --cap) {
    rj = r_cap(W1, cap); rk = r_cap(W2, cap);
    tilesJ = (W1 + 8 * rj - 1) / (8 * rj); tilesK = (W2 + 8 * rk - 1) / (8 * rk);
    if ((long long)N * tilesJ * tilesK >= 1024) break;
  }
  if (cross_fwd_image_ok_f16(N, W1, W2, D, q, a, GATHER)) {
    static_assert(kImageD16 % 2 == 0 && (kImageD16 % 16) != 0, "rows 8 apart in different banks: gcd(D, 64) <= 8");
    const size_t img = (size_t)(W1 + W2) * D * sizeof(float);
    const unsigned g2 = (unsigned)((N + 1) / 2);
#define MMS_IMG_CASE(J, K)                                                                                    \
  if (W1 == 8 * J && W2 == 8 * K) {                                                                           \
    hipLaunchKernelGGL((cross_fwd_image_f16_kernel<J, K, MODE, kImageD16, GATHER>), dim3(g2), dim3(128),      \
                       2 * img, s, q, a, n0, n1, top, N, gt);                                                 \
    return;                                                                                                   \
  }
#define MMS_IMG_ROW(J) MMS_IMG_CASE(J, 1) MMS_IMG_CASE(J, 2) MMS_IMG_CASE(J, 3) MMS_IMG_CASE(J, 4) MMS_IMG_CASE(J, 5)
    MMS_IMG_ROW(1) MMS_IMG_ROW(2) MMS_IMG_ROW(3) MMS_IMG_ROW(4) MMS_IMG_ROW(5)
#undef MMS_IMG_ROW
#undef MMS_IMG_CASE
  }
  const long long work = (long long)N * tilesJ * tilesK;
  const unsigned grid = (unsigned)((work + 3) / 4);
#define MMS_CROSS_CASE(J, K)                                                                    \
  if (rj == J && rk == K) {                                                                     \
    hipLaunchKernelGGL((cross_fwd_f16_kernel<J, K, MODE, GATHER>), dim3(grid), dim3(256), 0, s, \
                       q, a, n0, n1, top, N, W1, W2, D, tilesJ, tilesK, gt);                    \
    return;                                                                                     \
  }
#define MMS_CROSS_ROW(J) MMS_CROSS_CASE(J, 1) MMS_CROSS_CASE(J, 2) MMS_CROSS_CASE(J, 3) \
                         MMS_CROSS_CASE(J, 4) MMS_CROSS_CASE(J, 5)
  MMS_CROSS_ROW(1) MMS_CROSS_ROW(2) MMS_CROSS_ROW(3) MMS_CROSS_ROW(4) MMS_CROSS_ROW(5)
#undef MMS_CROSS_ROW
#undef MMS_CROSS_CASE
}

// The word-grid forward; GATHER: q and a are the embedding table and the Embed gather is fused in.
template <bool GATHER>
static void cross_forward_f16(int mode, int N, int W1, int W2, int D, const _Float16* q, const _Float16* a, float* top,
                              float* norm0, float* norm1, hipStream_t s, CrossGather gt) {
  if (mode == 1) {
    launch_cross_fwd_f16<1, GATHER>(q, a, nullptr, nullptr, top, N, W1, W2, D, s, gt);
    return;
  }
  const long long r0 = (long long)N * W1, r1 = (long long)N * W2;
  hipLaunchKernelGGL(row_norm_f16_kernel, dim3((unsigned)((r0 + 3) / 4)), dim3(256), 0, s, q, norm0, r0, D, gt.iq, gt.K, gt.bias);
  hipLaunchKernelGGL(row_norm_f16_kernel, dim3((unsigned)((r1 + 3) / 4)), dim3(256), 0, s, a, norm1, r1, D, gt.ia, gt.K, gt.bias);
  launch_cross_fwd_f16<0, GATHER>(q, a, norm0, norm1, top, N, W1, W2, D, s, gt);
}

// tiled while the tables fit 64 KB of LDS, else plain; `exact`: the Euclid backward mode, read once by the entry point
static void cross_backward_f16(int mode, int N, int W1, int W2, int D, const _Float16* q, const _Float16* a,
                               const float* top, const float* top_diff, const float* norm0, const float* norm1,
                               _Float16* dq, _Float16* da, bool exact, hipStream_t s) {
  const int nchunks = (D + kBwdDC16 - 1) / kBwdDC16;
  if (mode == 1) norm0 = norm1 = nullptr;
  const size_t lds = cross_bwd_tiled_lds_f16(mode, W1, W2);
  if (lds <= 64 * 1024 && 2LL * N * nchunks <= 0x7fffffffLL) {
    const int split = ((long long)N * nchunks < 1024) ? 1 : 0;
    const unsigned grid = (unsigned)((split ? 2LL : 1LL) * N * nchunks);
    // cosine has one arithmetic: its instance is <0, true>
    const auto k = mode == 0 ? cross_bwd_tiled_f16_kernel<0, true>
                   : exact   ? cross_bwd_tiled_f16_kernel<1, true> : cross_bwd_tiled_f16_kernel<1, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, q, a, top, top_diff, norm0, norm1, dq, da, W1, W2, D, nchunks,
                       split);
  } else {
    hipLaunchKernelGGL((mode == 1 ? cross_bwd_plain_f16_kernel<1> : cross_bwd_plain_f16_kernel<0>), dim3(N), dim3(256),
                       0, s, q, a, top, top_diff, norm0, norm1, dq, da, W1, W2, D);
  }
}

// =============================== entry points ===============================
// mms_abi.hip has checked the arguments: mode 0 or 1, not W1 == W2 == 1 (the gathered forward serves that too), N >= 1.

constexpr CrossGather kNoGather{nullptr, nullptr, 0, nullptr};

int simcross_grid_forward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, float* top,
                              float* norm0, float* norm1, hipStream_t s) {
  cross_forward_f16<false>(mode, N, W1, W2, D, static_cast<const _Float16*>(q), static_cast<const _Float16*>(a), top,
                           norm0, norm1, s, kNoGather);
  return launch_status();
}

// top = SimCross(Embed(index_q), Embed(index_a)) for dist_mode 0 / 1 from a half table (K, D): embed_simcross_forward
// (simcross_cross.hip) with the table's halves widened by the gathering loads.  No workspace, one launch for Euclid and
// three for cosine.
int embed_simcross_forward_f16(int mode, int N, int W1, int W2, int D, int K, const float* index_q, const float* index_a,
                               const void* table, const float* embed_bias, float* top, float* norm0, float* norm1,
                               hipStream_t s) {
  const _Float16* t = static_cast<const _Float16*>(table);
  cross_forward_f16<true>(mode, N, W1, W2, D, t, t, top, norm0, norm1, s, CrossGather{index_q, index_a, K, embed_bias});
  return launch_status();
}

int simcross_grid_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, const float* top,
                               const float* top_diff, const float* norm0, const float* norm1, void* dq, void* da,
                               hipStream_t s) {
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  cross_backward_f16(mode, N, W1, W2, D, static_cast<const _Float16*>(q), static_cast<const _Float16*>(a), top,
                     top_diff, norm0, norm1, static_cast<_Float16*>(dq), static_cast<_Float16*>(da), exact, s);
  return launch_status();
}

int simcross_grid_forward_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a,
                                       const float* top_diff, float* top, float* norm0, float* norm1, void* dq,
                                       void* da, hipStream_t s) {
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  const _Float16* qh = static_cast<const _Float16*>(q);
  const _Float16* ah = static_cast<const _Float16*>(a);
  cross_forward_f16<false>(mode, N, W1, W2, D, qh, ah, top, norm0, norm1, s, kNoGather);
  cross_backward_f16(mode, N, W1, W2, D, qh, ah, top, top_diff, norm0, norm1, static_cast<_Float16*>(dq),
                     static_cast<_Float16*>(da), exact, s);
  return launch_status();
}

}  // namespace mms
