// csrc/conv_wdiff_tile.h -- the fast route's PARAMETER-DIFF tile and the reduce behind it, shared by csrc/conv.hip (whose
// top_diff lies in memory) and csrc/train_tail_backward.hip (which forms it from y and per-channel coefficients while
// staging).  ONE definition of the walk over a slab's units, the staging and the MFMA loop, parameterised by where an
// element of top_diff comes from; csrc/conv.hip's header comment describes the launch, csrc/conv_plans.h has its plan.
#ifndef MMS_CONV_WDIFF_TILE_H_
#define MMS_CONV_WDIFF_TILE_H_

#include "conv_plans.h"

namespace mms {

// top_diff as it lies in memory: element (n, m, oy, ox) of a.dy
struct ConvLoadTopDiff {
  __device__ __forceinline__ float operator()(const ConvWdiffArgs& a, int n, int m, int oy, int ox) const {
    return a.dy[((size_t)n * a.K + m) * ((size_t)a.OH * a.OW) + (size_t)oy * a.OW + ox];
  }
};

// Workgroup (blockIdx.x: four column tiles of 16 (c, i, j); blockIdx.y: slab) of kConvThreads threads, lds: a.lds_bytes
// at least.  dy(a, n, m, oy, ox) is element (n, m, oy, ox) of top_diff.
template <int MT, class Dy>
__device__ __forceinline__ void conv_wdiff_tile(const ConvWdiffArgs& a, float* lds, Dy dy) {
  constexpr int Mpad = 16 * MT;
  float* band = lds;                                    // [G][C][BR][W]
  float* tds = band + a.G * a.C * a.plane;              // [Mpad][PP]: top_diff, channel x pixel of the unit
  int* pixoff = reinterpret_cast<int*>(tds + Mpad * a.PP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
  const int khkw = a.kh * a.kw, ncols = a.C * khkw, nW = a.K * ncols;
  const int ct = blockIdx.x * 4 + wave;
  const bool tile_on = a.want_w && ct * 16 < ncols;     // wave-uniform
  const int ncol = ct * 16 + l16;
  int ncoff = 0;
  if (ncol < ncols) {
    const int c = ncol / khkw, t = ncol - c * khkw, i = t / a.kw, j = t - i * a.kw;
    ncoff = c * a.plane + i * a.W + j;
  }
  const bool bias_on = a.want_b && blockIdx.x == 0 && tid < a.K;
  float bsum = 0.f;
  conv_v4f acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (conv_v4f){0.f, 0.f, 0.f, 0.f};

  const int u0 = blockIdx.y * a.ups, u1 = min(a.units, u0 + a.ups);
  for (int u = u0; u < u1; ++u) {
    const int ig = u / a.bands, bnd = u - ig * a.bands;
    const int n0 = ig * a.G, gc = min(a.G, a.N - n0);
    const int oy0 = bnd * a.R, rb = min(a.R, a.OH - oy0);
    const int per = rb * a.OW, P = gc * per, steps = (P + 3) >> 2, p4 = steps * 4, bru = rb + a.kh - 1;
    __syncthreads();                                    // the previous unit has been consumed
    if (a.want_w) {                                     // every wave stages, with or without a tile of its own
      for (int e = tid; e < gc * a.C * bru * a.W; e += kConvThreads) {
        const int bc = e % a.W;
        int t = e / a.W;
        const int br = t % bru;
        t /= bru;                                       // t = img * C + c
        band[t * a.plane + br * a.W + bc] = a.x[((size_t)(n0 * a.C + t) * a.H + oy0 + br) * a.W + bc];
      }
    }
    for (int e = tid; e < Mpad * p4; e += kConvThreads) {
      const int m = e / p4, p = e - m * p4;
      float v = 0.f;
      if (m < a.K && p < P) {
        const int img = p / per, q = p - img * per, r = q / a.OW, c = q - r * a.OW;
        v = dy(a, n0 + img, m, oy0 + r, c);
      }
      tds[m * a.PP + p] = v;
    }
    for (int p = tid; p < p4; p += kConvThreads) {
      int o = -1;
      if (p < P) {
        const int img = p / per, q = p - img * per, r = q / a.OW, c = q - r * a.OW;
        o = img * a.C * a.plane + r * a.W + c;
      }
      pixoff[p] = o;
    }
    __syncthreads();
    if (bias_on)
      for (int p = 0; p < P; ++p) bsum += tds[tid * a.PP + p];
    if (tile_on) {
      for (int s = 0; s < steps; ++s) {
        const int p = 4 * s + grp;
        const int po = pixoff[p];
        const float t = band[ncoff + (po < 0 ? 0 : po)];
        const float bv = po < 0 ? 0.f : t;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(tds[(16 * mt + l16) * a.PP + p], bv, acc[mt], 0, 0, 0);
      }
    }
  }
  float* slab = a.part + (size_t)blockIdx.y * (nW + a.K);
  if (tile_on && ncol < ncols) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * grp + r;
        if (m < a.K) slab[(size_t)m * ncols + ncol] = acc[mt][r];
      }
  }
  if (bias_on) slab[nW + tid] = bsum;
}

// diff[e] = diff[e] + (part[0][e] + part[1][e] + ... ), slabs ascending, for the thread's element e of the nW weights
// and K biases behind them; a NULL diff is skipped.
template <typename T>
__device__ __forceinline__ void conv_reduce_element(const T* __restrict__ part, int slabs, int nW, int K,
                                                    T* __restrict__ weight_diff, T* __restrict__ bias_diff) {
  const int e = blockIdx.x * kConvThreads + threadIdx.x;
  if (e >= nW + K) return;
  T* out = e < nW ? (weight_diff ? weight_diff + e : nullptr) : (bias_diff ? bias_diff + (e - nW) : nullptr);
  if (!out) return;
  const size_t stride = (size_t)nW + K;
  T s = part[e];
  for (int k = 1; k < slabs; ++k) s += part[k * stride + e];
  *out = *out + s;
}

}  // namespace mms
#endif  // MMS_CONV_WDIFF_TILE_H_
