// csrc/conv_stage.hip -- the TEST-phase stage Convolution -> BN -> AvePool -> TanH as one call, and its extern "C" entry
// points (include/mms_conv_stage.h: mms_conv_stage_*).  With y = conv(x, w) (+ bias), per output channel k and pooling
// window (ph x pw, the windows tile y's (OH, OW)):
//
//   m = the window's y added in (h, w) order, starting from 0, / (ph pw)
//   save_pool = (m + (-mean[k])) / sqrt(var[k] + 1e-9)          top = tanh(save_pool * scale[k] + shift[k])
//
// Two routes (conv_stage_route, the one place that decides):
//
//   sequence  mms_conv_forward_* into the workspace, then mms_bn_pool_tanh_forward_* in TEST phase from it: the two
//             public calls, nothing of their own here.  All of double; float where the fused route does not reach.
//             Workspace: [y: N K OH OW][save_mean: K][save_std: K][save_pool: N K OH/ph OW/pw], the last used when the
//             caller passes no save_pool.
//   fused     float, where the convolution's forward is on its fast route (csrc/conv_tile.h) with a band whose height
//             is a multiple of ph: conv_prod_plan with rq = ph.  A workgroup's pixels -- whole rows of one image, or
//             several whole small images -- are then whole windows.  The product is conv_tile_product, the one
//             csrc/conv.hip runs; the epilogue puts accumulator + bias in LDS as tile[k][pixel], over the band and the
//             weights the last chunk has finished with (K <= 64 channels x 256 pixels is the 64 KB those had at most),
//             and after a barrier thread e takes (image, channel, window) e, e + 256, ...: it adds its window from the
//             tile in (h, w) order as one chain from 0 and finishes with bn_pool_test_finish, csrc/bn_pool.hip's own.
//             Only pooled-size arrays are stored; y is never in device memory.
//
// A shape the fused route reaches but does not pay at goes to the sequence: conv_stage_route has the rule.
// An element of y is the same chain of MFMA steps on both routes wherever both cut the input channels into the same
// chunks (CC of conv_prod_plan: the band's height enters it), and then the two routes give the same words.
#include "bn_common.h"
#include "conv_tile.h"
#include "mms_conv_stage.h"
#include "mms_internal.h"

namespace mms {
namespace {

static_assert(kConvMaxChannels * kConvTilePixels <= kConvLdsFloats, "the accumulator tile of any fast plan fits the LDS");

struct StageDims {
  ConvDims d;
  int ph, pw, POH, POW;
};

// the refusal of the shape and the window, else MMS_OK and *g
int stage_check(const mms_conv_shape* shape, int ph, int pw, StageDims* g) {
  const int rc = conv_check(shape, &g->d);
  if (rc != MMS_OK) return rc;
  if (ph < 1 || pw < 1 || g->d.OH % ph || g->d.OW % pw) return MMS_ERR_INVALID_ARG;
  g->ph = ph;
  g->pw = pw;
  g->POH = g->d.OH / ph;
  g->POW = g->d.OW / pw;
  return MMS_OK;
}

struct StageArgs {
  ConvProdArgs p;        // conv_prod_plan(d, forward, ph); p.out is not used
  const float *mean, *var, *scale, *shift;
  float* top;            // (N, K, POH, POW)
  float* save_pool;      // the same, or NULL
  int ph, pw, POH, POW;
  int PS;                // row length of the accumulator tile [Cout][PS]
  size_t lds_bytes;
};

// p.ok false: the sequence route.
StageArgs stage_plan(const StageDims& g) {
  StageArgs a = {};
  a.p = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, g.ph);
  if (!a.p.ok) return a;
  a.ph = g.ph; a.pw = g.pw; a.POH = g.POH; a.POW = g.POW;
  const int P = a.p.G * a.p.R * a.p.OWt;
  // Lane groups of an accumulator are four channels apart: a row length of 4 or 12 mod 16 puts their 16 pixels in
  // separate banks.  Taken where it still fits.
  a.PS = P;
  while (a.PS % 16 != 4 && a.PS % 16 != 12) ++a.PS;
  if (a.p.Cout * a.PS > kConvLdsFloats) a.PS = P;
  const size_t tile = (size_t)a.p.Cout * a.PS * sizeof(float);
  a.lds_bytes = tile > a.p.lds_bytes ? tile : a.p.lds_bytes;
  return a;
}

// The measured rules (tools/bench_conv_stage.py, profiles/conv_stage_bench.txt: fused against sequence at network_v4's
// two stages over a range of N; `groups` is the launch's workgroups).
//   Whole images per workgroup (conv1, ten each): slower at 5 workgroups (189.7 against 180.7 us), faster at 10, 20, 40,
//   80 and 152 (1.03 to 1.09 x).  Few workgroups are latency-bound and the epilogue is on each one's critical path.
//   Fused from the smallest count measured to win.
constexpr long long kStageMinImageGroups = 10;
//   A band the pooling window made lower than the convolution's own (conv0: 4 rows for 6): faster at 450 and 1800
//   workgroups (1.42 x, 1.05 x), level at 4095 (0.98 x, ranges overlapping), slower at 6300, 9000 and 13653 (0.96 to
//   0.97 x).  Why is not measured: supposedly the nine pixel tiles over four waves (3, 2, 2, 2) and 8 staged rows per 4
//   computed against 10 per 6.  Fused up to a count between the last win and the tie.
constexpr long long kStageMaxShrunkBandGroups = 2048;

int conv_stage_route(const StageDims& g) {
  const StageArgs a = stage_plan(g);
  if (!a.p.ok) return MMS_CONV_STAGE_ROUTE_SEQUENCE;
  const long long groups = (long long)((a.p.N + a.p.G - 1) / a.p.G) * a.p.bands;
  if (a.p.G > 1) return groups >= kStageMinImageGroups ? MMS_CONV_STAGE_ROUTE_FUSED : MMS_CONV_STAGE_ROUTE_SEQUENCE;
  if (a.p.R < conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1).R && groups > kStageMaxShrunkBandGroups)
    return MMS_CONV_STAGE_ROUTE_SEQUENCE;
  return MMS_CONV_STAGE_ROUTE_FUSED;
}

// PH, PW > 0: the window's size at compile time (== s.ph, s.pw); 0: any window.
template <int PH, int PW>
struct StagePoolEpilogue {
  const StageArgs& s;
  float* tile;
  int kc;                // the channel whose values follow: that of the thread's first (image, channel, window)
  float nmean, std, sc, sh;
  __device__ __forceinline__ void channel(int k) {
    kc = k;
    nmean = -s.mean[k];
    std = bn_sqrt(s.var[k] + 1e-9f);
    sc = s.scale[k];
    sh = s.shift[k];
  }
  // Before the product: the loads are long back when the epilogue, on the workgroup's critical path, needs them.
  __device__ __forceinline__ void pixel(const ConvProdArgs& a, const ConvTile& t, int nt, int, int, int) {
    if (nt == 0) channel((int)threadIdx.x / (t.rb / s.ph * s.POW) % a.Cout);
  }

  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile& t, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
    const int PS = s.PS;
    __syncthreads();                                    // every wave has finished with the band and the weights
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * grp + r;
        if (m >= a.Cout) continue;
        const float b = a.bias ? a.bias[m] : 0.f;
#pragma unroll
        for (int nt = 0; nt < kConvNT; ++nt)
          if (pvalid[nt]) tile[m * PS + (wave + 4 * nt) * 16 + l16] = a.bias ? acc[mt][nt][r] + b : acc[mt][nt][r];
      }
    __syncthreads();
    const int ph = PH > 0 ? PH : s.ph, pw = PW > 0 ? PW : s.pw;
    const int wrows = t.rb / ph, wper = wrows * s.POW;  // windows of the band: per image
    const int PP = s.POH * s.POW, q0 = t.oy0 / ph * s.POW;
    const float ke = (float)(ph * pw);
    for (int e = tid; e < t.gc * a.Cout * wper; e += kConvThreads) {
      const int q = e % wper;
      int u = e / wper;
      const int k = u % a.Cout, img = u / a.Cout;
      const int wr = q / s.POW, wc = q - wr * s.POW;
      const float* src = tile + k * PS + img * t.per + wr * ph * a.OWt + wc * pw;
      float sum = 0.f;
      if constexpr (PH > 0) {
        float v[PH][PW];
#pragma unroll
        for (int i = 0; i < PH; ++i)
#pragma unroll
          for (int j = 0; j < PW; ++j) v[i][j] = src[i * a.OWt + j];
#pragma unroll
        for (int i = 0; i < PH; ++i)
#pragma unroll
          for (int j = 0; j < PW; ++j) sum += v[i][j];
      } else {
        for (int i = 0; i < ph; ++i)
          for (int j = 0; j < pw; ++j) sum += src[i * a.OWt + j];
      }
      const size_t o = ((size_t)(t.n0 + img) * a.Cout + k) * PP + q0 + q;
      if (k != kc) channel(k);
      float sp;
      const float tv = bn_pool_test_finish(sum, ke, nmean, std, sc, sh, &sp);
      if (s.save_pool) s.save_pool[o] = sp;
      s.top[o] = tv;
    }
  }
};

template <int MT, int PH, int PW>
__global__ __launch_bounds__(kConvThreads) void conv_stage_kernel(StageArgs s) {
  extern __shared__ float conv_lds[];
  StagePoolEpilogue<PH, PW> epi{s, conv_lds};
  conv_tile_product<MT>(s.p, conv_lds, epi);
}

template <int K>
using stage_int = std::integral_constant<int, K>;

// f(PH, PW) as types: network_v4's two windows at compile time, any other at run time.
template <class F>
void stage_dispatch(int ph, int pw, F&& f) {
  if (ph == 4 && pw == 4) f(stage_int<4>{}, stage_int<4>{});
  else if (ph == 5 && pw == 5) f(stage_int<5>{}, stage_int<5>{});
  else f(stage_int<0>{}, stage_int<0>{});
}

template <typename T>
size_t stage_sequence_bytes(const StageDims& g) {
  const size_t map = (size_t)g.d.N * g.d.K * g.d.OH * g.d.OW, pooled = (size_t)g.d.N * g.d.K * g.POH * g.POW;
  return (map + 2 * (size_t)g.d.K + pooled) * sizeof(T);
}

template <typename T>
size_t stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, bool sequence) {  // sequence: whatever the route
  StageDims g;
  if (stage_check(shape, ph, pw, &g) != MMS_OK || g.d.N == 0) return 0;
  if (std::is_same<T, float>::value && !sequence && conv_stage_route(g) == MMS_CONV_STAGE_ROUTE_FUSED) return 0;
  return stage_sequence_bytes<T>(g);
}

inline int conv_public(const mms_conv_shape* s, const float* x, const float* w, const float* b, float* y, void* st) {
  return mms_conv_forward_f32(s, x, w, b, y, nullptr, 0, st);
}
inline int conv_public(const mms_conv_shape* s, const double* x, const double* w, const double* b, double* y, void* st) {
  return mms_conv_forward_f64(s, x, w, b, y, nullptr, 0, st);
}
// TEST phase reads running_mean / running_var and writes neither; it needs no workspace.
inline int bn_pool_public(const StageDims& g, const float* y, const float* scale, const float* shift, const float* mean,
                          const float* var, float* top, float* sp, float* sm, float* ss, void* st) {
  return mms_bn_pool_tanh_forward_f32(1, g.d.N, g.d.K, g.d.OH, g.d.OW, g.ph, g.pw, 0.f, y, scale, shift,
                                      const_cast<float*>(mean), const_cast<float*>(var), top, sp, sm, ss, nullptr, 0, st);
}
inline int bn_pool_public(const StageDims& g, const double* y, const double* scale, const double* shift,
                          const double* mean, const double* var, double* top, double* sp, double* sm, double* ss,
                          void* st) {
  return mms_bn_pool_tanh_forward_f64(1, g.d.N, g.d.K, g.d.OH, g.d.OW, g.ph, g.pw, 0., y, scale, shift,
                                      const_cast<double*>(mean), const_cast<double*>(var), top, sp, sm, ss, nullptr, 0,
                                      st);
}

// force: MMS_CONV_STAGE_ROUTE_NONE (conv_stage_route decides), _SEQUENCE or _FUSED (float; MMS_ERR_UNSUPPORTED where the
// fused plan does not reach).
template <typename T>
int stage_forward(const mms_conv_shape* shape, int ph, int pw, const T* x, const T* w, const T* bias, const T* mean,
                  const T* var, const T* scale, const T* shift, T* top, T* save_pool, void* workspace,
                  size_t workspace_bytes, int force, void* stream) {
  StageDims g;
  const int rc = stage_check(shape, ph, pw, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !top || !mean || !var || !scale || !shift) return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, w, bias, mean, var, scale, shift};
  for (const void* in : inputs) {
    if (in && (top == in || save_pool == in)) return MMS_ERR_INVALID_ARG;
  }
  if (top == save_pool) return MMS_ERR_INVALID_ARG;
  if constexpr (std::is_same<T, float>::value) {
    if (force == MMS_CONV_STAGE_ROUTE_FUSED && !stage_plan(g).p.ok) return MMS_ERR_UNSUPPORTED;
    if (force == MMS_CONV_STAGE_ROUTE_FUSED ||
        (force == MMS_CONV_STAGE_ROUTE_NONE && conv_stage_route(g) == MMS_CONV_STAGE_ROUTE_FUSED)) {
      StageArgs a = stage_plan(g);
      a.p.in = x; a.p.w = w; a.p.bias = bias; a.p.out = nullptr;
      a.mean = mean; a.var = var; a.scale = scale; a.shift = shift; a.top = top; a.save_pool = save_pool;
      const dim3 grid((unsigned)((a.p.N + a.p.G - 1) / a.p.G), (unsigned)a.p.bands);
      conv_with_mt(a.p.MT, [&](auto M) {
        stage_dispatch(ph, pw, [&](auto PH, auto PW) {
          hipLaunchKernelGGL((conv_stage_kernel<decltype(M)::value, decltype(PH)::value, decltype(PW)::value>), grid,
                             dim3(kConvThreads), a.lds_bytes, as_stream(stream), a);
        });
      });
      return launch_status();
    }
  }
  if (!workspace || workspace_bytes < stage_sequence_bytes<T>(g)) return MMS_ERR_WORKSPACE;
  const size_t map = (size_t)g.d.N * g.d.K * g.d.OH * g.d.OW;
  T* y = static_cast<T*>(workspace);
  T* save_mean = y + map;
  T* save_std = save_mean + g.d.K;
  T* sp = save_pool ? save_pool : save_std + g.d.K;
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  const int rc1 = conv_public(shape, x, w, bias, y, stream);
  if (rc1 != MMS_OK) return rc1;
  return bn_pool_public(g, y, scale, shift, mean, var, top, sp, save_mean, save_std, stream);
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_conv_stage_route(const mms_conv_shape* shape, int ph, int pw) {
  StageDims g;
  if (stage_check(shape, ph, pw, &g) != MMS_OK) return MMS_CONV_STAGE_ROUTE_NONE;
  return conv_stage_route(g);
}

size_t mms_conv_stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float>(shape, ph, pw, false);
}
size_t mms_conv_stage_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<double>(shape, ph, pw, false);
}
size_t mms_conv_stage_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float>(shape, ph, pw, true);
}

int mms_conv_stage_forward_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                               const float* bias, const float* mean, const float* var, const float* scale,
                               const float* shift, float* top, float* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return stage_forward<float>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                              workspace_bytes, MMS_CONV_STAGE_ROUTE_NONE, stream);
}

int mms_conv_stage_forward_f64(const mms_conv_shape* shape, int ph, int pw, const double* x, const double* weight,
                               const double* bias, const double* mean, const double* var, const double* scale,
                               const double* shift, double* top, double* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return stage_forward<double>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                               workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_stage_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, const float* x,
                                        const float* weight, const float* bias, const float* mean, const float* var,
                                        const float* scale, const float* shift, float* top, float* save_pool,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  return stage_forward<float>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                              workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_stage_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                                     const float* bias, const float* mean, const float* var, const float* scale,
                                     const float* shift, float* top, float* save_pool, void* stream) {
  return stage_forward<float>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, nullptr, 0,
                              MMS_CONV_STAGE_ROUTE_FUSED, stream);
}

}  // extern "C"
