// csrc/head_tile.h -- the tile steps of the head's fast forward, shared by csrc/head.hip (whose kernel walks a slab's
// tiles of samples read from memory), csrc/score_tail.hip (whose epilogue runs them on the rows a convolution stage
// left in LDS) and csrc/train_tail.hip (whose second launch runs them in TRAIN phase): the shape check, the fast plan, the LDS layout of a tile and ONE definition of each step -- staging the
// weights, fc1 on the matrix pipe with tanh, fc2, softmax with the loss term.  csrc/head.hip's header comment describes
// the route; the order of every sum is fixed here and depends neither on the row a sample has in its tile nor on which
// wave or lane takes it: fc1's features ascending four per MFMA step from 0, then the bias; fc2's hidden units ascending
// from 0, then the bias; the softmax's classes ascending.
#ifndef MMS_HEAD_TILE_H_
#define MMS_HEAD_TILE_H_

#include <float.h>
#include <limits.h>

#include "mms_common.h"
#include "mms_head.h"

namespace mms {

typedef float head_v4f __attribute__((ext_vector_type(4)));

constexpr int kHeadThreads = 256;
constexpr int kHeadFastSamples = 64;       // samples of a tile: 16 per wave
constexpr int kHeadFastFeatures = 128;      // fast route: F0 + F1, eight column tiles of 16
constexpr int kHeadFastHidden = 64;         // fast route: H, four tiles of 16
constexpr int kHeadFastClasses = 16;        // fast route: C; C H <= 4 elements of w2_diff per thread
constexpr int kHeadMaxLdsBytes = 131072;   // the fast kernels' dynamic LDS, at most (the CU has 160 KB)

struct HeadDims {
  int N, F0, F1, F, H, C, train, norm, has_ign, ign;
};

// the shape's refusal, else MMS_OK and *d
inline int head_check(const mms_head_shape* s, HeadDims* d) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->N < 0 || s->F0 <= 0 || s->F1 < 0 || s->H <= 0 || s->C <= 0) return MMS_ERR_INVALID_ARG;
  if (!(s->dropout_ratio > 0.f && s->dropout_ratio < 1.f)) return MMS_ERR_INVALID_ARG;
  if (s->phase != MMS_HEAD_TRAIN && s->phase != MMS_HEAD_TEST) return MMS_ERR_INVALID_ARG;
  if (s->normalization < MMS_HEAD_NORM_FULL || s->normalization > MMS_HEAD_NORM_NONE) return MMS_ERR_INVALID_ARG;
  const long long F = (long long)s->F0 + s->F1, N = s->N;
  if (F > INT_MAX || N * s->F0 > INT_MAX || N * s->F1 > INT_MAX || N * s->H > INT_MAX || N * s->C > INT_MAX ||
      F * s->H > INT_MAX || (long long)s->C * s->H > INT_MAX)
    return MMS_ERR_INVALID_ARG;
  if (F * s->H + s->H + (long long)s->C * s->H + s->C > INT_MAX) return MMS_ERR_INVALID_ARG;
  *d = {s->N, s->F0, s->F1, (int)F, s->H, s->C, s->phase == MMS_HEAD_TRAIN, s->normalization, s->has_ignore_label != 0,
        s->ignore_label};
  return MMS_OK;
}

// the class of a label, or -1: ignored (the ignore label, or outside [0, C))
template <typename T>
__device__ inline int head_class(const HeadDims& d, T label) {
  const int lv = static_cast<int>(label);
  if ((d.has_ign && lv == d.ign) || lv < 0 || lv >= d.C) return -1;
  return lv;
}

template <typename T>
__device__ inline T head_normalizer(const HeadDims& d, int count) {
  T v;
  switch (d.norm) {
    case MMS_HEAD_NORM_VALID: v = T(count); break;
    case MMS_HEAD_NORM_NONE: v = T(1); break;
    default: v = T(d.N); break;       // FULL: outer_num * inner_num; BATCH_SIZE: outer_num
  }
  return v > T(1) ? v : T(1);
}

template <typename T>
__device__ inline T head_loss_term(T p) {
  return -log(p > T(FLT_MIN) ? p : T(FLT_MIN));
}

struct HeadFastPlan {
  int HT, FT;        // tiles of 16 hidden units / features
  int Fp;            // forward: F rounded up to the K step of 4
  int Fa, Ha;        // strides of [row][k] operands: 2 mod 4
  int Fk, Hk;        // strides of [k][column] operands: 16 mod 32
  size_t fwd_lds, bwd_lds;
  bool ok;
};

inline int head_stride16(int tiles) { return 16 * tiles + ((tiles & 1) ? 0 : 16); }

// floats of the forward's LDS for tiles of `rows` samples (p.HT, p.Fa and p.Ha set)
inline size_t head_fwd_lds_floats(const HeadDims& d, const HeadFastPlan& p, int rows) {
  return (size_t)16 * p.HT * p.Fa + rows * p.Fa + rows * p.Ha + d.C * (d.H + 1) + rows * (d.C + 1) + 16 * p.HT + d.C +
         2 * rows;
}

inline HeadFastPlan head_fast_plan(const HeadDims& d) {
  HeadFastPlan p = {};
  if (d.F > kHeadFastFeatures || d.H > kHeadFastHidden || d.C > kHeadFastClasses) return p;
  p.HT = (d.H + 15) / 16;
  p.FT = (d.F + 15) / 16;
  p.Fp = (d.F + 3) & ~3;
  p.Fa = p.Fp + 2;
  p.Ha = 16 * p.HT + 2;
  p.Fk = head_stride16(p.FT);
  p.Hk = head_stride16(p.HT);
  const int T = kHeadFastSamples;
  p.fwd_lds = sizeof(float) * head_fwd_lds_floats(d, p, T);
  p.bwd_lds = sizeof(float) * ((size_t)16 * p.HT * p.Fk + T * p.Fk + T * p.Ha + T * p.Hk + d.C * (d.H + 1) +
                               T * (d.C + 1) + 4);
  p.ok = p.fwd_lds <= (size_t)kHeadMaxLdsBytes && p.bwd_lds <= (size_t)kHeadMaxLdsBytes;
  return p;
}

// The forward's LDS, head_fwd_lds_floats(d, p, rows) floats from `lds`.
struct HeadFwdLds {
  float* w1s;        // [16 HT][Fa]: w1, rows past H and columns F .. Fp zero
  float* feats;      // [rows][Fa]: the tile's [x0 | x1], rows past the tile and columns F .. Fp zero
  float* dbuf;       // [rows][Ha]: d
  float* w2s;        // [C][H + 1]
  float* z2s;        // [rows][C + 1]
  float* b1s;        // [16 HT]
  float* b2s;        // [C]
  float* terms;      // [rows]
  int* valid;        // [rows]
};

__device__ inline HeadFwdLds head_fwd_carve(float* lds, const HeadDims& d, const HeadFastPlan& p, int rows) {
  HeadFwdLds L;
  const int Hw = 16 * p.HT;
  L.w1s = lds;
  L.feats = L.w1s + Hw * p.Fa;
  L.dbuf = L.feats + rows * p.Fa;
  L.w2s = L.dbuf + rows * p.Ha;
  L.z2s = L.w2s + d.C * (d.H + 1);
  L.b1s = L.z2s + rows * (d.C + 1);
  L.b2s = L.b1s + Hw;
  L.terms = L.b2s + d.C;
  L.valid = reinterpret_cast<int*>(L.terms + rows);
  return L;
}

// w1, w2 and the biases to LDS, by the whole workgroup.  A barrier follows before they are read.
__device__ inline void head_stage_weights(const HeadFwdLds& L, const HeadDims& d, const HeadFastPlan& p, const float* w1,
                                          const float* b1, const float* w2, const float* b2) {
  const int tid = threadIdx.x, Hw = 16 * p.HT, W2 = d.H + 1;
  for (int e = tid; e < Hw * p.Fp; e += kHeadThreads) {
    const int j = e / p.Fp, f = e - j * p.Fp;
    L.w1s[j * p.Fa + f] = (j < d.H && f < d.F) ? w1[(size_t)j * d.F + f] : 0.f;
  }
  for (int e = tid; e < d.C * d.H; e += kHeadThreads) {
    const int c = e / d.H, j = e - c * d.H;
    L.w2s[c * W2 + j] = w2[e];
  }
  for (int j = tid; j < Hw; j += kHeadThreads) L.b1s[j] = (b1 && j < d.H) ? b1[j] : 0.f;
  for (int c = tid; c < d.C; c += kHeadThreads) L.b2s[c] = b2 ? b2[c] : 0.f;
}

// Dropout of one element of h in TRAIN phase, from its word of the caller's mask: (h * Dtype(mask)) * scale.  The `drop`
// of head_fc1_block in csrc/head.hip (TRAIN) and in csrc/train_tail.hip.
__device__ __forceinline__ float head_dropout(float hv, unsigned m, float scale) { return (hv * float(m)) * scale; }

// fc1 and tanh of one block, by one wave: rows 16 rt .. 16 rt + 15 of the tile (sample n0 + row, below n1) by hidden
// units 16 ht .. 16 ht + 15, K = the features in steps of 4.  h goes to memory where `h` is not NULL and
// d = drop(h, n, j) to L.dbuf, zeros for a row past the tile or a unit past H.
template <class Drop>
__device__ inline void head_fc1_block(const HeadFwdLds& L, const HeadDims& d, const HeadFastPlan& p, int rt, int ht,
                                      bool has_b1, int n0, int n1, float* h, Drop drop) {
  const int lane = threadIdx.x & 63, l16 = lane & 15, grp = lane >> 4;
  head_v4f acc = {0.f, 0.f, 0.f, 0.f};
  const float* ap = L.feats + (16 * rt + l16) * p.Fa + grp;
  const float* bp = L.w1s + (16 * ht + l16) * p.Fa + grp;
  for (int s = 0; s < p.Fp; s += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s], bp[s], acc, 0, 0, 0);
  const int j = 16 * ht + l16;              // lane: hidden unit j, rows 16 rt + 4 grp + r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * rt + 4 * grp + r, n = n0 + row;
    float dv = 0.f;
    if (n < n1 && j < d.H) {
      const float hv = tanhf(has_b1 ? acc[r] + L.b1s[j] : acc[r]);
      if (h) h[(size_t)n * d.H + j] = hv;
      dv = drop(hv, n, j);
    }
    L.dbuf[row * p.Ha + j] = dv;
  }
}

// fc2: z2 of (row, class c) from the row's d
__device__ inline void head_fc2_one(const HeadFwdLds& L, const HeadDims& d, const HeadFastPlan& p, int row, int c,
                                    bool has_b2) {
  const float* dr = L.dbuf + row * p.Ha;
  const float* wc = L.w2s + c * (d.H + 1);
  float z = 0.f;
  for (int j = 0; j < d.H; ++j) z += dr[j] * wc[j];
  L.z2s[row * (d.C + 1) + c] = has_b2 ? z + L.b2s[c] : z;
}

// softmax of one row, by one lane: prob_row (C) is written; lv is the row's class (head_class) or -1.  Returns the loss
// term of the row, 0 without a class, and *ok = whether it has one.
__device__ inline float head_softmax_row(const HeadFwdLds& L, const HeadDims& d, int row, float* prob_row, int lv,
                                         int* ok) {
  float* zr = L.z2s + row * (d.C + 1);
  float mx = zr[0];
  for (int c = 1; c < d.C; ++c) mx = zr[c] > mx ? zr[c] : mx;
  float sum = 0.f;
  for (int c = 0; c < d.C; ++c) {
    const float e = expf(zr[c] - mx);
    zr[c] = e;
    sum += e;
  }
  float term = 0.f;
  *ok = 0;
  for (int c = 0; c < d.C; ++c) {
    const float pv = zr[c] / sum;
    prob_row[c] = pv;
    if (c == lv) {
      term = head_loss_term(pv);
      *ok = 1;
    }
  }
  return term;
}

}  // namespace mms
#endif  // MMS_HEAD_TILE_H_
