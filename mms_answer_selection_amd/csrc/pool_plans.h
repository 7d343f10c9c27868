// csrc/pool_plans.h -- what the host decides for a Pooling call (include/mms_pool.h) before it launches: the shape's
// judgement with the reference's output size, and the forward's launch plan.  Inline host text with no HIP call, so that
// tests/native/pool_plans_host.cpp sweeps it where there is no GPU; the few functions the kernels repeat on the device
// (a band's rows) are marked for both sides.
#ifndef MMS_POOL_PLANS_H_
#define MMS_POOL_PLANS_H_

#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "mms_pool.h"

#if defined(__HIPCC__)
#define MMS_POOL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MMS_POOL_HD inline
#endif

namespace mms {

constexpr int kPoolThreads = 256;
// LDS a forward workgroup stages its rows in (plus 16 bytes: the image keeps the source's offset from a 16-byte
// boundary).  Eight workgroups of 256 fill a CU's wave slots; eight times this is 128 of its 160 KB.
constexpr int kPoolLdsBytes = 16 * 1024;
// One resident round of the chip: 8 workgroups on each of 256 CUs.  A larger call strides over its items.
constexpr int kPoolMaxBlocks = 2048;

struct PoolGeom {
  int N, C, H, W, kh, kw, sh, sw, pad_h, pad_w, PH, PW, method;
  int planes;                               // N * C; set once the counts are known to fit
};

// pooling_layer.cpp:90-105 for one axis; `any_pad`: pad_h or pad_w is not 0.  The quotient and the ceil are float's, as
// the reference's are.
inline long long pool_out_dim(int in, int k, int s, int p, bool any_pad) {
  const long long span = (long long)in + 2LL * p - k;
  long long o = (long long)ceilf((float)span / (float)s) + 1;
  if (any_pad)
    while (o > 1 && (o - 1) * s >= (long long)in + p) --o;
  return o;
}

// The shape's judgement (the refusal table of include/mms_pool.h up to the counts): *g is set on MMS_OK, planes
// excepted.
inline int pool_geometry(const mms_pool_shape* s, PoolGeom* g) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->N < 0 || s->C < 1 || s->H < 1 || s->W < 1 || s->kernel_h < 1 || s->kernel_w < 1 || s->stride_h < 1 ||
      s->stride_w < 1 || s->pad_h < 0 || s->pad_w < 0 || s->pad_h >= s->kernel_h || s->pad_w >= s->kernel_w)
    return MMS_ERR_INVALID_ARG;
  if (s->method == MMS_POOL_STOCHASTIC) return MMS_ERR_UNSUPPORTED;
  if (s->method != MMS_POOL_AVE && s->method != MMS_POOL_MAX) return MMS_ERR_INVALID_ARG;
  const bool any_pad = s->pad_h != 0 || s->pad_w != 0;
  const long long PH = pool_out_dim(s->H, s->kernel_h, s->stride_h, s->pad_h, any_pad);
  const long long PW = pool_out_dim(s->W, s->kernel_w, s->stride_w, s->pad_w, any_pad);
  if (PH < 1 || PW < 1 || PH > INT_MAX || PW > INT_MAX) return MMS_ERR_INVALID_ARG;
  if ((PH - 1) * s->stride_h >= (long long)s->H + s->pad_h || (PW - 1) * s->stride_w >= (long long)s->W + s->pad_w)
    return MMS_ERR_UNSUPPORTED;
  const PoolGeom out = {s->N,        s->C,     s->H,     s->W,    s->kernel_h, s->kernel_w, s->stride_h,
                        s->stride_w, s->pad_h, s->pad_w, (int)PH, (int)PW,     s->method,   0};
  *g = out;
  return MMS_OK;
}

// Element counts of bottom and top; false where one is above INT_MAX (Caffe's count()).  Sets g->planes.
inline bool pool_counts(PoolGeom* g, long long* bottom, long long* top) {
  const long long planes = (long long)g->N * g->C, hw = (long long)g->H * g->W, phw = (long long)g->PH * g->PW;
  if (planes > INT_MAX || hw > INT_MAX || phw > INT_MAX) return false;
  if (planes > 0 && (hw > INT_MAX / planes || phw > INT_MAX / planes)) return false;
  g->planes = (int)planes;
  *bottom = planes * hw;
  *top = planes * phw;
  return true;
}

// The rows [lo, hi) of a plane that the output rows [ph0, ph1) read.
MMS_POOL_HD int pool_band_lo(const PoolGeom& g, int ph0) {
  const int hs = ph0 * g.sh - g.pad_h;
  return hs > 0 ? hs : 0;
}
MMS_POOL_HD int pool_band_hi(const PoolGeom& g, int ph1) {
  const long long he = (long long)(ph1 - 1) * g.sh - g.pad_h + g.kh;
  return he < g.H ? (int)he : g.H;
}

// The forward's plan.  An ITEM is what a workgroup stages in LDS and pools from there, so that a row is read from memory
// once however many windows share it:
//   kPoolStaged   P whole planes (H * W elements each fit the LDS).  P grows with the call, so that up to one resident
//                 round of workgroups covers it, and stops at what the LDS holds.  A window that is the whole map makes
//                 one output per plane: lane p of the workgroup walks plane p's chain from LDS while the other
//                 workgroups of the CU load theirs.
//   kPoolBanded   one band of R output rows of one plane, whose (R - 1) * stride_h + kernel_h input rows fit the LDS.
//   kPoolDirect   not even one output row's input rows fit: a thread per output reads its window from memory (the
//                 caches serve what windows share).  An item is kPoolThreads outputs.
// `blocks` workgroups stride over `items`.
enum PoolRoute { kPoolStaged = 0, kPoolBanded = 1, kPoolDirect = 2 };
struct PoolPlan {
  int route, P, R, bands, blocks;
  long long items;
  size_t lds_bytes;
};

inline PoolPlan pool_forward_plan(const PoolGeom& g, int elem_bytes) {
  const long long cap = kPoolLdsBytes / elem_bytes, hw = (long long)g.H * g.W;
  PoolPlan p = {};
  p.lds_bytes = (size_t)kPoolLdsBytes + 16;
  if (hw <= cap) {
    p.route = kPoolStaged;
    const long long fit = cap / hw, want = ((long long)g.planes + kPoolMaxBlocks - 1) / kPoolMaxBlocks;
    p.P = (int)(want < 1 ? 1 : want > fit ? fit : want);
    p.R = g.PH;
    p.bands = 1;
    p.items = ((long long)g.planes + p.P - 1) / p.P;
  } else if ((long long)g.kh * g.W <= cap) {
    p.route = kPoolBanded;
    p.P = 1;
    const long long rows = cap / g.W, R = (rows - g.kh) / g.sh + 1;
    p.R = (int)(R < g.PH ? R : g.PH);
    p.bands = (g.PH + p.R - 1) / p.R;
    p.items = (long long)g.planes * p.bands;
  } else {
    p.route = kPoolDirect;
    p.P = 1;
    p.R = g.PH;
    p.bands = 1;
    p.items = ((long long)g.planes * g.PH * g.PW + kPoolThreads - 1) / kPoolThreads;
    p.lds_bytes = 0;
  }
  p.blocks = (int)(p.items < kPoolMaxBlocks ? p.items : kPoolMaxBlocks);
  return p;
}

// Workgroups of an elementwise sweep over `groups` units of work, one per thread and trip.
inline int pool_sweep_blocks(long long groups) {
  const long long b = (groups + kPoolThreads - 1) / kPoolThreads;
  return (int)(b < kPoolMaxBlocks ? b : kPoolMaxBlocks);
}

}  // namespace mms
#endif  // MMS_POOL_PLANS_H_
