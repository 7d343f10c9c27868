// csrc/conv_stage.hip -- the TEST-phase stages Convolution -> BN -> AvePool -> TanH (include/mms_conv_stage.h:
// mms_conv_stage_*) and Convolution -> BN -> MaxPool -> TanH (include/mms_conv_maxpool_stage.h:
// mms_conv_maxpool_stage_*), each as one call, and their extern "C" entry points.  The two families are one set of
// templates with a `MAX` parameter: the checks, the plan, the accumulator tile, the workspace and the launchers are
// stated once; what differs is what a thread keeps of its window, the finish (csrc/bn_common.h has both), the second
// call of the sequence and the measured routing rule.  With y = conv(x, w) (+ bias), per output channel k and pooling
// window (ph x pw, the windows tile y's (OH, OW)):
//
//   AVE  m = the window's y added in (h, w) order, starting from 0, / (ph pw)
//   MAX  m = the window's y scanned in (h, w) order from its first element: the larger kept for scale[k] > 0, the
//        smaller for scale[k] < 0, the first for scale[k] == 0; a NaN never wins (bp_keep)
//   save_pool = (m + (-mean[k])) / sqrt(var[k] + 1e-9)          top = tanh(save_pool * scale[k] + shift[k])
//
// Two routes (stage_route<MAX>, the one place that decides for a family):
//
//   sequence  mms_conv_forward_* into the workspace, then mms_bn_pool_tanh_forward_* (MAX:
//             mms_bn_maxpool_tanh_forward_*) in TEST phase from it: the two public calls, nothing of their own here.
//             All of double; float where the fused route does not reach.
//             Workspace: [y: N K OH OW][save_mean: K][save_std: K][save_pool: N K OH/ph OW/pw], the last used when the
//             caller passes no save_pool.
//   fused     float, where the convolution's forward is on its fast route (csrc/conv_tile.h) with a band whose height
//             is a multiple of ph: conv_prod_plan with rq = ph.  A workgroup's pixels -- whole rows of one image, or
//             several whole small images -- are then whole windows.  The product is conv_tile_product, the one
//             csrc/conv.hip runs; the epilogue's steps are listed in csrc/conv_pool_tile.h, which has the tile.  Thread e
//             takes (image, channel, window) e, e + 256, ... and finishes its window's sum with bn_pool_test_finish
//             (MAX: its extremum with bn_maxpool_test_finish), both csrc/bn_pool.hip's own.
//             Only pooled-size arrays are stored; y is never in device memory.
//
// A shape the fused route reaches but does not pay at goes to the sequence: stage_route<MAX> has each family's rule.
// An element of y is the same chain of MFMA steps on both routes wherever both cut the input channels into the same
// chunks (CC of conv_prod_plan: the band's height enters it), and then the two routes give the same words.
// The host side of the fused launch -- StageArgs, stage_plan, stage_band_shrunk, stage_route<MAX> with its measured
// thresholds -- is csrc/conv_stage_plans.h, where tests/native/conv_stage_plans_host.cpp reads it.
#include "conv_stage_plans.h"
#include "mms_internal.h"

namespace mms {
namespace {

// the refusal of the shape and the window, else MMS_OK and *g
template <bool MAX>
int stage_check(const mms_conv_shape* shape, int ph, int pw, StageDims* g) {
  g->max = MAX;
  return stage_window_check(shape, ph, pw, g);
}

// PH, PW > 0: the window's size at compile time (== s.ph, s.pw); 0: any window.  MAX: the window's extremum where AVE
// has its sum.
template <bool MAX, int PH, int PW>
struct StagePoolEpilogue {
  const StageArgs& s;
  float* tile;
  StageChannel<MAX> ch;  // of the channel whose values follow: that of the thread's first (image, channel, window)
  // Before the product: the loads are long back when the epilogue, on the workgroup's critical path, needs them.
  __device__ __forceinline__ void pixel(const ConvProdArgs& a, const ConvTile& t, int nt, int, int, int) {
    if (nt == 0) ch.load(s, (int)threadIdx.x / (t.rb / s.ph * s.POW) % a.Cout);
  }

  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile& t, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int tid = threadIdx.x, PS = s.PS;
    stage_tile_store(a, tile, PS, acc, pvalid);
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
      if (MAX && k != ch.kc) ch.load(s, k);                // the scan needs the channel's direction
      float sum = 0.f;                                  // AVE: the window's sum; MAX: its extremum
      const auto keep = [&](bool first, float v) {      // one element of the window, in (h, w) order
        if constexpr (MAX) bp_keep(first, v, ch.dir, &sum);
        else sum += v;
      };
      if constexpr (PH > 0) {
        float v[PH][PW];
#pragma unroll
        for (int i = 0; i < PH; ++i)
#pragma unroll
          for (int j = 0; j < PW; ++j) v[i][j] = src[i * a.OWt + j];
#pragma unroll
        for (int i = 0; i < PH; ++i)
#pragma unroll
          for (int j = 0; j < PW; ++j) keep(i == 0 && j == 0, v[i][j]);
      } else {
        for (int i = 0; i < ph; ++i)
          for (int j = 0; j < pw; ++j) keep(i == 0 && j == 0, src[i * a.OWt + j]);
      }
      const size_t o = ((size_t)(t.n0 + img) * a.Cout + k) * PP + q0 + q;
      if (!MAX && k != ch.kc) ch.load(s, k);
      float sp;
      const float tv = MAX ? bn_maxpool_test_finish(sum, ch.nmean, ch.std, ch.sc, ch.sh, &sp)
                           : bn_pool_test_finish(sum, ke, ch.nmean, ch.std, ch.sc, ch.sh, &sp);
      if (s.save_pool) s.save_pool[o] = sp;
      s.top[o] = tv;
    }
  }
};

template <int MT, bool MAX, int PH, int PW>
__global__ __launch_bounds__(kConvThreads) void conv_stage_kernel(StageArgs s) {
  extern __shared__ float conv_lds[];
  StagePoolEpilogue<MAX, PH, PW> epi{s, conv_lds};
  conv_tile_product<MT>(s.p, conv_lds, epi);
}

template <typename T>
size_t stage_sequence_bytes(const StageDims& g) {
  const size_t map = (size_t)g.d.N * g.d.K * g.d.OH * g.d.OW, pooled = (size_t)g.d.N * g.d.K * g.POH * g.POW;
  return (map + 2 * (size_t)g.d.K + pooled) * sizeof(T);
}

template <typename T, bool MAX>
size_t stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, bool sequence) {  // sequence: whatever the route
  StageDims g;
  if (stage_check<MAX>(shape, ph, pw, &g) != MMS_OK || g.d.N == 0) return 0;
  if (std::is_same<T, float>::value && !sequence && stage_route<MAX>(g) == MMS_CONV_STAGE_ROUTE_FUSED) return 0;
  return stage_sequence_bytes<T>(g);
}

// force: MMS_CONV_STAGE_ROUTE_NONE (stage_route<MAX> decides), _SEQUENCE or _FUSED (float; MMS_ERR_UNSUPPORTED where the
// fused plan does not reach).
template <typename T, bool MAX>
int stage_forward(const mms_conv_shape* shape, int ph, int pw, const T* x, const T* w, const T* bias, const T* mean,
                  const T* var, const T* scale, const T* shift, T* top, T* save_pool, void* workspace,
                  size_t workspace_bytes, int force, void* stream) {
  StageDims g;
  const int rc = stage_check<MAX>(shape, ph, pw, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !top || !mean || !var || !scale || !shift) return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, w, bias, mean, var, scale, shift};
  const void* const outputs[] = {top, save_pool};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  if constexpr (std::is_same<T, float>::value) {
    if (force == MMS_CONV_STAGE_ROUTE_FUSED && !stage_plan(g).p.ok) return MMS_ERR_UNSUPPORTED;
    if (force == MMS_CONV_STAGE_ROUTE_FUSED ||
        (force == MMS_CONV_STAGE_ROUTE_NONE && stage_route<MAX>(g) == MMS_CONV_STAGE_ROUTE_FUSED)) {
      StageArgs a = stage_plan(g);
      a.p.in = x; a.p.w = w; a.p.bias = bias; a.p.out = nullptr;
      a.mean = mean; a.var = var; a.scale = scale; a.shift = shift; a.top = top; a.save_pool = save_pool;
      const dim3 grid((unsigned)((a.p.N + a.p.G - 1) / a.p.G), (unsigned)a.p.bands);
      conv_with_mt(a.p.MT, [&](auto M) {
        stage_pool_dispatch<MAX>(ph, pw, [&](auto PH, auto PW) {
          hipLaunchKernelGGL((conv_stage_kernel<decltype(M)::value, MAX, decltype(PH)::value, decltype(PW)::value>),
                             grid, dim3(kConvThreads), a.lds_bytes, as_stream(stream), a);
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
  const int rc1 = Abi<T>::conv_forward(shape, x, w, bias, y, nullptr, 0, stream);
  if (rc1 != MMS_OK) return rc1;
  // phase 1 (TEST) reads running_mean / running_var, writes neither and needs no workspace
  const auto bn_pool_tanh = g.max ? Abi<T>::bn_maxpool_tanh_forward : Abi<T>::bn_pool_tanh_forward;
  return bn_pool_tanh(1, g.d.N, g.d.K, g.d.OH, g.d.OW, g.ph, g.pw, T(0), y, scale, shift, const_cast<T*>(mean),
                      const_cast<T*>(var), top, sp, save_mean, save_std, nullptr, 0, stream);
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_conv_stage_route(const mms_conv_shape* shape, int ph, int pw) {
  StageDims g;
  if (stage_check<false>(shape, ph, pw, &g) != MMS_OK) return MMS_CONV_STAGE_ROUTE_NONE;
  return stage_route<false>(g);
}

size_t mms_conv_stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float, false>(shape, ph, pw, false);
}
size_t mms_conv_stage_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<double, false>(shape, ph, pw, false);
}
size_t mms_conv_stage_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float, false>(shape, ph, pw, true);
}

int mms_conv_stage_forward_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                               const float* bias, const float* mean, const float* var, const float* scale,
                               const float* shift, float* top, float* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return stage_forward<float, false>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                                     workspace_bytes, MMS_CONV_STAGE_ROUTE_NONE, stream);
}

int mms_conv_stage_forward_f64(const mms_conv_shape* shape, int ph, int pw, const double* x, const double* weight,
                               const double* bias, const double* mean, const double* var, const double* scale,
                               const double* shift, double* top, double* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return stage_forward<double, false>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool,
                                      workspace, workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_stage_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, const float* x,
                                        const float* weight, const float* bias, const float* mean, const float* var,
                                        const float* scale, const float* shift, float* top, float* save_pool,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  return stage_forward<float, false>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                                     workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_stage_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                                     const float* bias, const float* mean, const float* var, const float* scale,
                                     const float* shift, float* top, float* save_pool, void* stream) {
  return stage_forward<float, false>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, nullptr,
                                     0, MMS_CONV_STAGE_ROUTE_FUSED, stream);
}

// include/mms_conv_maxpool_stage.h: the MAX form, the same arguments.
int mms_conv_maxpool_stage_route(const mms_conv_shape* shape, int ph, int pw) {
  StageDims g;
  if (stage_check<true>(shape, ph, pw, &g) != MMS_OK) return MMS_CONV_STAGE_ROUTE_NONE;
  return stage_route<true>(g);
}

size_t mms_conv_maxpool_stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float, true>(shape, ph, pw, false);
}
size_t mms_conv_maxpool_stage_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<double, true>(shape, ph, pw, false);
}
size_t mms_conv_maxpool_stage_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw) {
  return stage_workspace_bytes<float, true>(shape, ph, pw, true);
}

int mms_conv_maxpool_stage_forward_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                                       const float* bias, const float* mean, const float* var, const float* scale,
                                       const float* shift, float* top, float* save_pool, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return stage_forward<float, true>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                                    workspace_bytes, MMS_CONV_STAGE_ROUTE_NONE, stream);
}

int mms_conv_maxpool_stage_forward_f64(const mms_conv_shape* shape, int ph, int pw, const double* x,
                                       const double* weight, const double* bias, const double* mean, const double* var,
                                       const double* scale, const double* shift, double* top, double* save_pool,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return stage_forward<double, true>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                                     workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_maxpool_stage_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, const float* x,
                                                const float* weight, const float* bias, const float* mean,
                                                const float* var, const float* scale, const float* shift, float* top,
                                                float* save_pool, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  return stage_forward<float, true>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, workspace,
                                    workspace_bytes, MMS_CONV_STAGE_ROUTE_SEQUENCE, stream);
}

int mms_conv_maxpool_stage_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, const float* x,
                                             const float* weight, const float* bias, const float* mean,
                                             const float* var, const float* scale, const float* shift, float* top,
                                             float* save_pool, void* stream) {
  return stage_forward<float, true>(shape, ph, pw, x, weight, bias, mean, var, scale, shift, top, save_pool, nullptr, 0,
                                    MMS_CONV_STAGE_ROUTE_FUSED, stream);
}

}  // extern "C"
