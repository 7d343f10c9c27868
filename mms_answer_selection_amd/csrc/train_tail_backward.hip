// csrc/train_tail_backward.hip -- the fused backward of the TRAIN-phase tail Convolution -> BN -> Pool -> TanH -> head
// (include/mms_train_tail_backward.h: mms_train_tail_backward_*) and its extern "C" entry points.  The window is the
// whole map (S = OH OW pixels, M = N S), so BN -> Pool -> TanH's backward collapses: with g = x0_diff (1 - flt^2) and
// p^ = save_pool, per channel k
//
//   shift_diff = sum_n g          scale_diff = sum_n g p^          cs = scale / std
//   dy[n,k,oy,ox] = A0[k] + B[k] y[n,k,oy,ox] + (AVE: cg[n,k] at every pixel; MAX: cg[n,k] at the mask's pixel alone)
//   B  = -((cs scale_diff) / M) / std        A0 = -((cs shift_diff) / M) - B mean
//   cg = ((g / S) scale) / std  (AVE)        ((g scale) / std)  (MAX)
//
// which is csrc/bn_pool.hip's dx = (gs + (-1/M) (xn a + b)) / std with xn = (y - mean) / std spelt out in y.  No
// (N, K, OH, OW) dy is written or read: both convolution launches form it in their loaders (TrainTailDy).
//
// Launches of the FUSED route, ordered by the stream:
//   1. mms_head_backward_f32 on its fast route (one launch; a second, its ordered reduce, with more than 64 samples and
//      a parameter diff): the five head outputs are that call's words, x0_diff goes to the workspace.
//   2. train_tail_backward_coef_kernel.  Workgroup 0: thread k < K adds g and g p^ of channel k over n = 0, 1, ... in
//      ONE ascending chain each, writes scale_diff / shift_diff (the one designated workgroup) and A0, B to the
//      workspace.  Workgroups 1 ..: one thread per (n, k) writes cg and, MAX, the mask's pixel: csrc/bn_pool.hip's rule,
//      bp_keep's extremum of the window, then the first pixel whose BN output (bp_normalised, bp_bn_out) is the
//      extremum's.
//   3. train_tail_backward_bottom_kernel: conv_tile_product on the bottom_diff plan with at most
//      kTrainTailBackwardImages whole images per workgroup and TrainTailDy as its loader; ConvStoreEpilogue stores dx.
//   4. train_tail_backward_wdiff_kernel: conv_wdiff_tile with the same cut of images and the same loader; per-slab
//      partial sums to the workspace; bias_diff from the same sweep (the staged dy tile added pixel by pixel), not from
//      the coefficients.
//   5. train_tail_backward_reduce_kernel: conv_reduce_element, slabs ascending, ACCUMULATED into weight_diff / bias_diff.
// Launches whose outputs are all NULL are not issued.  No floating-point atomics, no arrival counters; every workspace
// word that is read has been written by this call.
#include "conv_wdiff_tile.h"
#include "mms_internal.h"
#include "mms_train_tail.h"
#include "mms_train_tail_backward.h"
#include "train_tail_backward_plans.h"

namespace mms {
namespace {

// Images of a workgroup of launches 3 and 4, at most: the tail's own constant, not the convolution's 256 pixels' worth
// (three 9 x 9 images in bottom_diff, ten 5 x 5 maps in the parameter diffs).  Measured
// (profiles/train_tail_backward_bench.txt, builds that differ in this constant only; forced FUSED, us per call, at
// N = 50 / 100 / 256): network_v4's tail 240.9 / 302.6 / 445.7 with one image, 270.0 / 336.5 / 475.4 with two,
// 321.6 / 364.4 / 520.3 with three; network_v3's 393.0 / 459.8 / 657.6, 425.0 / 529.7 / 749.4 and 476.5 / 583.4 / 804.5;
// network_v5's 98.2 / 133.0 / 240.0, 108.1 / 144.0 / 247.1 and 122.4 / 155.8 / 260.6.  One image is the fastest at every
// net and every N: with N <= 256 there are never more workgroups than two per CU, so fewer, longer workgroups only
// lengthen the chain of channel chunks each walks.
constexpr int kTrainTailBackwardImages = 1;

// The measured rule (tools/bench_train_tail_backward.py, profiles/train_tail_backward_bench.txt: forced FUSED against
// mms_train_tail_backward_f32, medians of seven alternating passes, us per call): FUSED on the span of launch-3 workgroup
// counts -- one per image -- at which the ratio sequence / fused is above 1 and the two rows' ranges are apart at every
// stage of the class; every other count, unmeasured ones included, is the SEQUENCE, and so is every image of more than
// 128 pixels (train_tail_backward_small_images), which no net of the driver has.
//   AVE (network_v4's tail): 1.23 x at 50 workgroups (240.9 against 296.6 us), 1.10 x at 100 (302.6 against 332.8), both
//     apart; 1.00 x at 256 with the ranges overlapping.  FUSED on 50 .. 100.
//   MAX (network_v3's tail, network_v5's last stage): v3's 1.11, 1.17 and 1.06 x at 50, 100 and 256, apart; v5's 1.31 x
//     at 50, apart, 0.86 x at 256; at 100 v5 has 1.12 x, apart, in the committed table and 1.11 x with the ranges
//     overlapping (one fused pass of seven at 174.5 us) in an earlier run of the same build: the runs disagree, so 100
//     is not taken.  FUSED at 50, the one count at which both stages' ranges are apart in every run.
// [MAX]: workgroups of launch 3.  {0, -1}: no count.
constexpr StageSpan kTrainTailBackwardGroups[2] = {{50, 100}, {50, 50}};

struct TrainTailDy {
  const float* y;            // (N, K, OH, OW)
  const float* A0;           // (K)
  const float* B;            // (K)
  const float* cg;           // (N, K)
  const int* pos;            // (N, K): MAX, the mask's pixel oy OW + ox
  int K, OW;
  size_t PI;
};

template <bool MAX>
__device__ __forceinline__ float train_tail_dy(const TrainTailDy& c, int n, int k, int oy, int ox) {
  const size_t nk = (size_t)n * c.K + k;
  const int q = oy * c.OW + ox;
  const float t = c.B[k] * c.y[nk * c.PI + q] + c.A0[k];
  if constexpr (MAX) return q == c.pos[nk] ? t + c.cg[nk] : t;
  else return t + c.cg[nk];
}

template <bool MAX>
struct TrainTailDyProd {     // conv_tile_product's loader: the operand is (N, K, OH, OW)
  TrainTailDy c;
  __device__ __forceinline__ float operator()(const ConvProdArgs&, int n, int k, int iy, int ix) const {
    return train_tail_dy<MAX>(c, n, k, iy, ix);
  }
};

template <bool MAX>
struct TrainTailDyWdiff {    // conv_wdiff_tile's
  TrainTailDy c;
  __device__ __forceinline__ float operator()(const ConvWdiffArgs&, int n, int m, int oy, int ox) const {
    return train_tail_dy<MAX>(c, n, m, oy, ox);
  }
};

struct TrainTailCoefArgs {
  const float *x0d, *flt, *save_pool, *scale, *shift, *save_mean, *save_std, *y;
  float *scale_diff, *shift_diff;       // or NULL
  float *A0, *B, *cg;
  int* pos;
  int N, K, S;
  float inv_M, ke;
};

template <bool MAX>
__global__ __launch_bounds__(kConvThreads) void train_tail_backward_coef_kernel(TrainTailCoefArgs a) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    for (int k = tid; k < a.K; k += kConvThreads) {
      float shd = 0.f, sd = 0.f;
      for (int n = 0; n < a.N; ++n) {
        const size_t o = (size_t)n * a.K + k;
        const float t = a.flt[o];
        const float g = a.x0d[o] * (1.f - t * t);
        shd += g;
        sd += g * a.save_pool[o];
      }
      if (a.shift_diff) a.shift_diff[k] = shd;
      if (a.scale_diff) a.scale_diff[k] = sd;
      const float std = a.save_std[k], cs = a.scale[k] / std;
      const float B = -(((cs * sd) * a.inv_M) / std);
      a.B[k] = B;
      a.A0[k] = -((cs * shd) * a.inv_M) - B * a.save_mean[k];
    }
    return;
  }
  const int e = (blockIdx.x - 1) * kConvThreads + tid;
  if (e >= a.N * a.K) return;
  const int k = e % a.K;
  const float t = a.flt[e], sc = a.scale[k], std = a.save_std[k];
  const float g = a.x0d[e] * (1.f - t * t);
  if constexpr (MAX) {
    a.cg[e] = (g * sc) / std;
    // the mask: csrc/bn_pool.hip's bp_backward_sweep, the window's extremum, then the first pixel with its BN output
    const float nmean = -a.save_mean[k], sh = a.shift[k];
    const int dir = bp_dir(sc);
    const float* w = a.y + (size_t)e * a.S;
    float ext = 0.f;
    for (int i = 0; i < a.S; ++i) bp_keep(i == 0, w[i], dir, &ext);
    const float ymax = bp_bn_out(bp_normalised(ext, nmean, std), sc, sh);
    // A thread walks its window's S consecutive words of y twice, windows S words apart across the lanes: not
    // coalesced, and cheap while S is a tail's 25 or 36 words (the second walk is served by the cache).
    int at = -1;                                        // -1: no pixel has ymax (a NaN window): no delta, as the sweep
    for (int i = a.S - 1; i >= 0; --i)
      if (bp_bn_out(bp_normalised(w[i], nmean, std), sc, sh) == ymax) at = i;
    a.pos[e] = at;
  } else {
    a.cg[e] = ((g / a.ke) * sc) / std;
  }
}

template <int MT, bool MAX>
__global__ __launch_bounds__(kConvThreads) void train_tail_backward_bottom_kernel(ConvProdArgs a, TrainTailDy c) {
  extern __shared__ float conv_lds[];
  ConvStoreEpilogue epi;
  epi.PI = (size_t)a.OHt * a.OWt;
  conv_tile_product<MT>(a, conv_lds, epi, TrainTailDyProd<MAX>{c});
}

template <int MT, bool MAX>
__global__ __launch_bounds__(kConvThreads) void train_tail_backward_wdiff_kernel(ConvWdiffArgs a, TrainTailDy c) {
  extern __shared__ float conv_lds[];
  conv_wdiff_tile<MT>(a, conv_lds, TrainTailDyWdiff<MAX>{c});
}

__global__ __launch_bounds__(kConvThreads) void train_tail_backward_reduce_kernel(const float* __restrict__ part,
                                                                                  int slabs, int nW, int K,
                                                                                  float* __restrict__ weight_diff,
                                                                                  float* __restrict__ bias_diff) {
  conv_reduce_element(part, slabs, nW, K, weight_diff, bias_diff);
}

// ---- host -----------------------------------------------------------------------------------------------------------
TrainTailBackwardPlan plan_of(const TrainTailDims& g) {
  return train_tail_backward_plan(g, kTrainTailBackwardImages, mms_head_workspace_bytes(&g.hs));
}

int route_of(const TrainTailDims& g) {
  return train_tail_backward_fused(g, kTrainTailBackwardImages, kTrainTailBackwardGroups) ? MMS_TRAIN_TAIL_ROUTE_FUSED
                                                                                         : MMS_TRAIN_TAIL_ROUTE_SEQUENCE;
}

enum { kAuto = -1, kFused = MMS_TRAIN_TAIL_ROUTE_FUSED };

int train_tail_backward_go(const mms_score_tail_shape* shape, int phase, float dropout_ratio, float loss_weight,
                           const float* x, const float* w, const float* y, const float* flt, const float* save_pool,
                           const float* scale, const float* shift, const float* save_mean, const float* save_std,
                           const float* overlap, const float* w1, const float* w2, const unsigned* mask, const float* h,
                           const float* prob, const float* label, float* dx, float* dw, float* db, float* dscale,
                           float* dshift, float* doverlap, float* w1d, float* b1d, float* w2d, float* b2d,
                           void* workspace, size_t workspace_bytes, int force, void* stream) {
  TrainTailDims g;
  int rc = train_tail_check(shape, phase, dropout_ratio, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  bool stage;
  float* dov = doverlap;
  rc = train_tail_backward_args(g, x, w, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2, mask, h,
                                prob, label, dx, dw, db, dscale, dshift, &dov, w1d, b1d, w2d, b2d, workspace, &stage);
  if (rc != MMS_OK) return rc;
  const TrainTailBackwardPlan p = plan_of(g);
  if (force == kFused && !p.ok) return MMS_ERR_UNSUPPORTED;
  if (force == kAuto && route_of(g) != MMS_TRAIN_TAIL_ROUTE_FUSED)
    return mms_train_tail_backward_f32(shape, phase, dropout_ratio, loss_weight, x, w, y, flt, save_pool, scale, shift,
                                       save_mean, save_std, overlap, w1, w2, mask, h, prob, label, dx, dw, db, dscale,
                                       dshift, doverlap, w1d, b1d, w2d, b2d, workspace, workspace_bytes, stream);
  // the routed call asks for its own query, which covers the forward too; the forced call for the fused layout alone
  const size_t need = force == kAuto ? mms_train_tail_backward_workspace_bytes(shape) : p.bytes;
  if (!workspace || workspace_bytes < need) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  float* x0d = stage ? reinterpret_cast<float*>(base + p.off_x0d) : nullptr;
  // launch 1: its own refusals have been answered above
  rc = mms_head_backward_f32(&g.hs, flt, overlap, w1, w2, mask, h, prob, label, loss_weight, x0d, dov, w1d, b1d, w2d, b2d,
                             base + p.off_head, p.off_coef - p.off_head, stream);
  if (rc != MMS_OK || !stage) return rc;
  const ConvDims& d = g.d;
  const int NK = d.N * d.K, S = d.OH * d.OW;
  float* coef = reinterpret_cast<float*>(base + p.off_coef);
  TrainTailCoefArgs c = {};
  c.x0d = x0d; c.flt = flt; c.save_pool = save_pool; c.scale = scale; c.shift = shift; c.save_mean = save_mean;
  c.save_std = save_std; c.y = y; c.scale_diff = dscale; c.shift_diff = dshift;
  c.A0 = coef; c.B = coef + d.K; c.cg = coef + 2 * d.K; c.pos = reinterpret_cast<int*>(coef + p.coef_floats);
  c.N = d.N; c.K = d.K; c.S = S;
  c.inv_M = (float)(1. / ((double)d.N * S));
  c.ke = (float)S;
  const bool maps = dx || dw || db;
  const unsigned coef_groups = maps ? 1u + (unsigned)((NK + kConvThreads - 1) / kConvThreads) : 1u;
  with_bool(g.max, [&](auto MAX) {
    hipLaunchKernelGGL((train_tail_backward_coef_kernel<decltype(MAX)::value>), dim3(coef_groups), dim3(kConvThreads), 0,
                       as_stream(stream), c);
  });
  if ((rc = launch_status()) != MMS_OK || !maps) return rc;
  const TrainTailDy dy = {y, c.A0, c.B, c.cg, c.pos, d.K, d.OW, (size_t)S};
  if (dx) {
    ConvProdArgs a = p.bottom;
    a.in = nullptr; a.w = w; a.bias = nullptr; a.out = dx;
    const dim3 grid((unsigned)((a.N + a.G - 1) / a.G), (unsigned)a.bands);
    conv_with_mt(a.MT, [&](auto M) {
      with_bool(g.max, [&](auto MAX) {
        hipLaunchKernelGGL((train_tail_backward_bottom_kernel<decltype(M)::value, decltype(MAX)::value>), grid,
                           dim3(kConvThreads), a.lds_bytes, as_stream(stream), a, dy);
      });
    });
    if ((rc = launch_status()) != MMS_OK) return rc;
  }
  if (!dw && !db) return MMS_OK;
  ConvWdiffArgs a = p.wdiff;
  a.x = x; a.dy = nullptr; a.part = reinterpret_cast<float*>(base + p.off_part);
  a.want_w = dw != nullptr; a.want_b = db != nullptr;
  const int nW = d.K * d.C * d.kh * d.kw;
  const int groups = dw ? (d.C * d.kh * d.kw + 63) / 64 : 1;         // four column tiles of 16 per workgroup
  conv_with_mt(a.MT, [&](auto M) {
    with_bool(g.max, [&](auto MAX) {
      hipLaunchKernelGGL((train_tail_backward_wdiff_kernel<decltype(M)::value, decltype(MAX)::value>),
                         dim3((unsigned)groups, (unsigned)a.slabs), dim3(kConvThreads), a.lds_bytes, as_stream(stream), a,
                         dy);
    });
  });
  if ((rc = launch_status()) != MMS_OK) return rc;
  hipLaunchKernelGGL(train_tail_backward_reduce_kernel, dim3((nW + d.K + kConvThreads - 1) / kConvThreads),
                     dim3(kConvThreads), 0, as_stream(stream), (const float*)a.part, a.slabs, nW, d.K, dw, db);
  return launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_train_tail_backward_route(const mms_score_tail_shape* shape) {
  TrainTailDims g;
  if (train_tail_check(shape, MMS_HEAD_TRAIN, 0.5f, &g) != MMS_OK) return MMS_TRAIN_TAIL_ROUTE_NONE;
  return route_of(g);
}

size_t mms_train_tail_backward_fused_workspace_bytes(const mms_score_tail_shape* shape) {
  TrainTailDims g;
  if (train_tail_check(shape, MMS_HEAD_TRAIN, 0.5f, &g) != MMS_OK || g.d.N == 0) return 0;
  const TrainTailBackwardPlan p = plan_of(g);
  return p.ok ? p.bytes : 0;
}

size_t mms_train_tail_backward_workspace_bytes(const mms_score_tail_shape* shape) {
  const size_t step = mms_train_tail_workspace_bytes(shape), fused = mms_train_tail_backward_fused_workspace_bytes(shape);
  if (mms_train_tail_backward_route(shape) != MMS_TRAIN_TAIL_ROUTE_FUSED) return step;
  return fused > step ? fused : step;
}

#define MMS_TRAIN_TAIL_BACKWARD_ARGS                                                                                    \
  const float *x, const float *weight, const float *y, const float *flt, const float *save_pool, const float *scale,   \
      const float *shift, const float *save_mean, const float *save_std, const float *overlap, const float *w1,        \
      const float *w2, const unsigned int *mask, const float *h, const float *prob, const float *label,                \
      float *bottom_diff, float *weight_diff, float *bias_diff, float *scale_diff, float *shift_diff,                  \
      float *overlap_diff, float *w1_diff, float *b1_diff, float *w2_diff, float *b2_diff, void *workspace,            \
      size_t workspace_bytes, void *stream
#define MMS_TRAIN_TAIL_BACKWARD_PASS                                                                                   \
  x, weight, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2, mask, h, prob, label, bottom_diff, \
      weight_diff, bias_diff, scale_diff, shift_diff, overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, workspace,    \
      workspace_bytes

int mms_train_tail_backward_routed_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio,
                                       float loss_weight, MMS_TRAIN_TAIL_BACKWARD_ARGS) {
  return train_tail_backward_go(shape, phase, dropout_ratio, loss_weight, MMS_TRAIN_TAIL_BACKWARD_PASS, kAuto, stream);
}

int mms_train_tail_backward_fused_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio,
                                      float loss_weight, MMS_TRAIN_TAIL_BACKWARD_ARGS) {
  return train_tail_backward_go(shape, phase, dropout_ratio, loss_weight, MMS_TRAIN_TAIL_BACKWARD_PASS, kFused, stream);
}

}  // extern "C"
