// csrc/conv_tile.h -- the fast route's PRODUCT tile, shared by four sources: csrc/conv.hip (forward and bottom_diff,
// whose epilogue stores the map) and csrc/conv_stage.hip, csrc/conv_stage_train.hip and csrc/score_tail.hip (whose
// epilogues pool it: csrc/conv_pool_tile.h has what those three share).  Here: the shape check, the geometry of a
// workgroup, the plan of the product and ONE definition of the staging + MFMA loop, parameterised by what is done with
// the accumulators.  csrc/conv.hip's header comment describes the product; the order of a sum is fixed here: channels
// ascending in chunks, (c, i, j) ascending inside a chunk in steps of four, the four of a step as the MFMA adds them.
#ifndef MMS_CONV_TILE_H_
#define MMS_CONV_TILE_H_

#include <limits.h>

#include <type_traits>

#include "mms_common.h"
#include "mms_conv.h"

namespace mms {

typedef float conv_v4f __attribute__((ext_vector_type(4)));

constexpr int kConvThreads = 256;
constexpr int kConvTilePixels = 256;       // output pixels of a fast workgroup: 16 tiles of 16
constexpr int kConvNT = 4;                 // pixel tiles of a wave: w, w + 4, w + 8, w + 12
constexpr int kConvLdsFloats = 16384;      // 64 KB: the dynamic LDS a launch gets without asking for more
constexpr int kConvMaxChannels = 64;       // fast route: MT <= 4 channel tiles of 16

struct ConvDims {
  int N, C, H, W, K, kh, kw, sh, sw, ph, pw, G, OH, OW, Cg, Kg;
};

// the shape's refusal, else MMS_OK and *d
inline int conv_check(const mms_conv_shape* s, ConvDims* d) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->N < 0 || s->C <= 0 || s->H <= 0 || s->W <= 0 || s->K <= 0 || s->kh <= 0 || s->kw <= 0 || s->stride_h <= 0 ||
      s->stride_w <= 0 || s->pad_h < 0 || s->pad_w < 0 || s->dilation_h <= 0 || s->dilation_w <= 0 || s->group <= 0)
    return MMS_ERR_INVALID_ARG;
  if (s->C % s->group || s->K % s->group) return MMS_ERR_INVALID_ARG;
  if (s->dilation_h != 1 || s->dilation_w != 1) return MMS_ERR_UNSUPPORTED;
  const long long eh = (long long)s->H + 2LL * s->pad_h - s->kh, ew = (long long)s->W + 2LL * s->pad_w - s->kw;
  if (eh < 0 || ew < 0) return MMS_ERR_INVALID_ARG;
  const long long OH = eh / s->stride_h + 1, OW = ew / s->stride_w + 1;
  const long long nx = (long long)s->N * s->C, nt = (long long)s->N * s->K;
  const long long nw = (long long)s->K * (s->C / s->group);
  if (OH > INT_MAX || OW > INT_MAX || (long long)s->H * s->W > INT_MAX || OH * OW > INT_MAX ||
      (long long)s->kh * s->kw > INT_MAX)
    return MMS_ERR_INVALID_ARG;
  if (nx > INT_MAX || nt > INT_MAX || nw > INT_MAX || nx * ((long long)s->H * s->W) > INT_MAX ||
      nt * (OH * OW) > INT_MAX || nw * ((long long)s->kh * s->kw) > INT_MAX)
    return MMS_ERR_INVALID_ARG;
  *d = {s->N,     s->C,     s->H,     s->W,    s->K,    s->kh,           s->kw,          s->stride_h, s->stride_w,
        s->pad_h, s->pad_w, s->group, (int)OH, (int)OW, s->C / s->group, s->K / s->group};
  return MMS_OK;
}

inline int conv_round4(int v) { return (v + 3) & ~3; }

// The pixels of a workgroup: `G` whole images where an image has at most kConvTilePixels / 2 pixels, else `R` whole
// rows of one image, `bands` bands per image.  rq: R is a multiple of it (OHt is; 1 for the plain product, the pooling
// window's height where the epilogue pools).  false: not even rq rows fit the tile.
inline bool conv_tile_geometry(int OHt, int OWt, int rq, int* G, int* R, int* bands) {
  if (OWt > kConvTilePixels) return false;
  const int PI = OHt * OWt;
  if (PI <= kConvTilePixels / 2) {
    *G = kConvTilePixels / PI;
    *R = OHt;
    *bands = 1;
  } else {
    const int upb = kConvTilePixels / OWt / rq;           // units of rq rows a band holds at most
    if (upb < 1) return false;
    const int units = OHt / rq, nb = (units + upb - 1) / upb;
    *G = 1;
    *R = (units + nb - 1) / nb * rq;
    *bands = (OHt + *R - 1) / *R;
  }
  return true;
}

struct ConvProdArgs {
  const float* in;       // (N, Cin, IH, IW)
  const float* w;        // W'(m, ci, t) = w[m * w_ms + ci * w_cs + (flip ? kh kw - 1 - t : t)]
  const float* bias;     // per output channel, or NULL
  float* out;            // (N, Cout, OHt, OWt)
  int N, Cin, Cout, IH, IW, OHt, OWt, kh, kw;
  int vph, vpw;          // rows / columns of zeros before the input (bottom_diff: kh - 1, kw - 1)
  int G, R, bands;       // conv_tile_geometry
  int BW, plane;         // band: row length IW + 2 vpw, BR * BW elements per channel with BR = R + kh - 1
  int CC, Kpad;          // input channels per chunk; conv_round4(CC * kh * kw)
  int MT;                // channel tiles of 16
  int w_ms, w_cs, flip;
  bool ok;
  size_t lds_bytes;
};

// pass 0: forward.  pass 1: bottom_diff, the forward product on top_diff with C and K swapped and the taps flipped.
// rq: conv_tile_geometry's, kept while the band shrinks to the LDS.
inline ConvProdArgs conv_prod_plan(const ConvDims& d, int pass, int rq) {
  ConvProdArgs a = {};
  if (d.sh != 1 || d.sw != 1 || d.ph != 0 || d.pw != 0 || d.G != 1 || d.C > kConvMaxChannels || d.K > kConvMaxChannels)
    return a;
  const int khkw = d.kh * d.kw;
  a.N = d.N; a.kh = d.kh; a.kw = d.kw;
  if (pass == 0) {
    a.Cin = d.C; a.Cout = d.K; a.IH = d.H; a.IW = d.W; a.OHt = d.OH; a.OWt = d.OW;
    a.vph = a.vpw = 0;
    a.w_ms = d.C * khkw; a.w_cs = khkw; a.flip = 0;
  } else {
    a.Cin = d.K; a.Cout = d.C; a.IH = d.OH; a.IW = d.OW; a.OHt = d.H; a.OWt = d.W;
    a.vph = d.kh - 1; a.vpw = d.kw - 1;
    a.w_ms = khkw; a.w_cs = d.C * khkw; a.flip = 1;
  }
  if (!conv_tile_geometry(a.OHt, a.OWt, rq, &a.G, &a.R, &a.bands)) return a;
  a.BW = a.IW + 2 * a.vpw;
  a.MT = a.Cout <= 16 ? 1 : a.Cout <= 32 ? 2 : 4;
  const int Mpad = 16 * a.MT;
  for (;;) {
    a.plane = (a.R + d.kh - 1) * a.BW;
    a.CC = 0;
    for (int cc = a.Cin; cc >= 1; --cc) {
      const long long kp = conv_round4(cc * khkw);
      if ((long long)a.G * cc * a.plane + (long long)Mpad * kp + kp <= kConvLdsFloats) { a.CC = cc; break; }
    }
    if (a.CC >= (a.Cin < 4 ? a.Cin : 4)) break;
    if (a.G > 1) { a.G = (a.G + 1) / 2; continue; }       // fewer images, then fewer rows, per workgroup
    if (a.R > rq) { a.R = (a.R / rq + 1) / 2 * rq; a.bands = (a.OHt + a.R - 1) / a.R; continue; }
    if (a.CC >= 1) break;
    return a;
  }
  a.Kpad = conv_round4(a.CC * khkw);
  a.lds_bytes = ((size_t)a.G * a.CC * a.plane + (size_t)Mpad * a.Kpad + a.Kpad) * sizeof(float);
  a.ok = true;
  return a;
}

// What the workgroup (blockIdx.x, blockIdx.y) of a product launch owns: images [n0, n0 + gc), rows [oy0, oy0 + rb) of
// each, `per` pixels per image and P in all; pixel p is (image p / per, row (p % per) / OWt, column p % OWt).
struct ConvTile {
  int n0, gc, oy0, rb, per, P;
};

// The product's own read of its input: element (n, c, iy, ix) of a.in.  A caller that forms the operand on the fly
// (csrc/train_tail_backward.hip: top_diff from y and per-channel coefficients) passes another.
struct ConvLoadInput {
  __device__ __forceinline__ float operator()(const ConvProdArgs& a, int n, int c, int iy, int ix) const {
    return a.in[(((size_t)n * a.Cin + c) * a.IH + iy) * a.IW + ix];
  }
};

// The product of one workgroup (kConvThreads threads, lds: a.lds_bytes at least).  Wave w owns pixel tiles w + 4 nt;
// its lane (l16, grp) ends with acc[mt][nt][r] = pixel (w + 4 nt) * 16 + l16, output channel 16 mt + 4 grp + r, WITHOUT
// the bias.  epi.pixel(a, t, nt, img, r, c) is told each of the lane's pixels before the loop (pixel 0's coordinates
// where valid[nt] is false); epi.finish(a, t, acc, valid) gets the sums.  No barrier follows the last chunk: a finish
// that writes LDS places one first.  load(a, n, c, iy, ix) is element (n, c, iy, ix) of the (N, Cin, IH, IW) operand.
template <int MT, class Epi, class Load = ConvLoadInput>
__device__ __forceinline__ void conv_tile_product(const ConvProdArgs& a, float* lds, Epi& epi, Load load = Load()) {
  constexpr int NT = kConvNT, Mpad = 16 * MT;
  float* band = lds;                                    // [G][CC][BR][BW]
  float* wsm = band + a.G * a.CC * a.plane;             // [Kpad][Mpad]
  int* koff = reinterpret_cast<int*>(wsm + a.Kpad * Mpad);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
  const int khkw = a.kh * a.kw;
  ConvTile t;
  t.n0 = blockIdx.x * a.G;
  t.gc = min(a.G, a.N - t.n0);
  t.oy0 = blockIdx.y * a.R;
  t.rb = min(a.R, a.OHt - t.oy0);
  t.per = t.rb * a.OWt;
  t.P = t.gc * t.per;
  const int n0 = t.n0, gc = t.gc, oy0 = t.oy0, per = t.per, P = t.P, bru = t.rb + a.kh - 1;

  for (int k = tid; k < a.Kpad; k += kConvThreads) {
    const int cl = k / khkw, tt = k - cl * khkw, i = tt / a.kw, j = tt - i * a.kw;
    koff[k] = cl * a.plane + i * a.BW + j;
  }
  int pix[NT];
  bool pvalid[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int p = (wave + 4 * nt) * 16 + l16;
    pvalid[nt] = p < P;
    const int pp = pvalid[nt] ? p : 0;
    const int img = pp / per, q = pp - img * per, r = q / a.OWt, c = q - r * a.OWt;
    pix[nt] = img * a.CC * a.plane + r * a.BW + c;
    epi.pixel(a, t, nt, img, r, c);
  }
  conv_v4f acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (conv_v4f){0.f, 0.f, 0.f, 0.f};

  for (int ci0 = 0; ci0 < a.Cin; ci0 += a.CC) {
    const int cc = min(a.CC, a.Cin - ci0), klen = cc * khkw, ksteps = (klen + 3) >> 2, k4 = ksteps * 4;
    __syncthreads();                                    // the previous chunk has been consumed
    for (int e = tid; e < Mpad * k4; e += kConvThreads) {
      const int m = e / k4, kk = e - m * k4;
      float v = 0.f;
      if (m < a.Cout && kk < klen) {
        const int cl = kk / khkw, tt = kk - cl * khkw;
        v = a.w[(size_t)m * a.w_ms + (size_t)(ci0 + cl) * a.w_cs + (a.flip ? khkw - 1 - tt : tt)];
      }
      wsm[kk * Mpad + m] = v;
    }
    for (int e = tid; e < gc * cc * bru * a.BW; e += kConvThreads) {
      const int bc = e % a.BW;
      int tt = e / a.BW;
      const int br = tt % bru;
      tt /= bru;
      const int cl = tt % cc, img = tt / cc;
      const int iy = oy0 + br - a.vph, ix = bc - a.vpw;
      float v = 0.f;
      if (iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW) v = load(a, n0 + img, ci0 + cl, iy, ix);
      band[(img * a.CC + cl) * a.plane + br * a.BW + bc] = v;
    }
    __syncthreads();
    for (int s = 0; s < ksteps; ++s) {
      const int k = 4 * s + grp;
      const bool kvalid = k < klen;                     // the weights of k >= klen are zeros; the band's are not staged
      const int off = kvalid ? koff[k] : 0;
      float av[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[mt] = wsm[k * Mpad + 16 * mt + l16];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if ((wave + 4 * nt) * 16 >= P) continue;        // wave-uniform: the tile holds no pixel
        const float tv = band[off + pix[nt]];
        const float bv = kvalid ? tv : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv, acc[mt][nt], 0, 0, 0);
      }
    }
  }
  epi.finish(a, t, acc, pvalid);
}

// The word of the map from an accumulator element of output channel m: b = conv_tile_bias(a, m), loaded once per
// channel, is added where there is a bias.
__device__ __forceinline__ float conv_tile_bias(const ConvProdArgs& a, int m) { return a.bias ? a.bias[m] : 0.f; }
__device__ __forceinline__ float conv_tile_word(const ConvProdArgs& a, float acc, float b) {
  return a.bias ? acc + b : acc;
}

// The epilogue that stores the map: csrc/conv.hip's forward and bottom_diff, csrc/train_tail_backward.hip's bottom_diff.
struct ConvStoreEpilogue {
  size_t outoff[kConvNT];
  size_t PI;
  __device__ __forceinline__ void pixel(const ConvProdArgs& a, const ConvTile& t, int nt, int img, int r, int c) {
    outoff[nt] = (size_t)(t.n0 + img) * a.Cout * PI + (size_t)(t.oy0 + r) * a.OWt + c;
  }
  // lane: pixel column l16, output channels 16 mt + 4 grp + r
  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile&, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int grp = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * grp + r;
        if (m >= a.Cout) continue;
        const float b = conv_tile_bias(a, m);
#pragma unroll
        for (int nt = 0; nt < kConvNT; ++nt)
          if (pvalid[nt]) a.out[outoff[nt] + (size_t)m * PI] = conv_tile_word(a, acc[mt][nt][r], b);
      }
  }
};

template <class F>
inline void conv_with_mt(int MT, F&& f) {
  if (MT == 1) f(std::integral_constant<int, 1>{});
  else if (MT == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace mms
#endif  // MMS_CONV_TILE_H_
