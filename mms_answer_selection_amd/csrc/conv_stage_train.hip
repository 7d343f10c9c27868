// csrc/conv_stage_train.hip -- the TRAIN-phase stage Convolution -> BN -> AvePool / MaxPool -> TanH, forward and
// backward each as one call (include/mms_conv_stage_train.h: mms_conv_stage_train_*), and their extern "C" entry
// points.  The formulas are those of csrc/conv.hip and csrc/bn_pool.hip; what is new here is the forward's FUSED route.
//
//   sequence  forward: mms_conv_forward_* into the caller's y, then mms_bn_pool_tanh_forward_* /
//             mms_bn_maxpool_tanh_forward_* with phase 0 on it -- three launches at the training batch (the
//             convolution, BN's sweep of the whole map, the pooled-size finish).  backward: the BN -> pool -> TanH
//             backward leaves dy in the workspace, mms_conv_backward_* runs on it.  Nothing of their own here.
//   fused     forward, float: two launches.
//             Launch 1 (train_product_kernel) is csrc/conv_tile.h's product with a band whose height is a multiple of
//             ph (conv_prod_plan with rq = ph, as csrc/conv_stage.hip) AND the chunk of input channels of the
//             convolution's own plan (rq = 1), so an element of y is the convolution's own chain of MFMA steps.  The
//             epilogue's steps are listed in csrc/conv_pool_tile.h, which has the tile; each word of the tile is
//             stored to y as well.  The 256 / (16 MT) adjacent lanes that serve channel k walk the workgroup's windows of k: lane j
//             takes windows j, j + T, ... in (image, window row, window column) order, stores the window's mean
//             (MAX: extremum) to save_pool, and adds the window's values in the same order into one sum of y and one
//             of y*y.  Only real pixels are windows: a band's tail and a ragged last image group add nothing.  The T
//             lanes' sums are combined by xor-shuffles 1, 2 (, 4, 8) apart -- registers and lanes, no LDS beside the
//             full tile -- and lane 0 writes them to the workspace slot of (channel, workgroup).
//             Launch 2 (train_finish_kernel) is pooled-size: grid (K, chunks); every workgroup adds its channel's
//             partials (thread t those of workgroups t, t + 256, ..., then bn_block_sum), forms the statistics with
//             bn_statistics -- chunk 0's first thread updates the running blobs and writes save_mean / save_std --
//             and finishes its chunk of the channel's pooled elements in place with bn_pool_train_finish,
//             csrc/bn_pool.hip's own.
// train_route is the one place that decides; its thresholds are lines of profiles/conv_stage_train_bench.txt.  The host
// side of the two launches -- TrainArgs, train_plan, train_route, fused_bytes, train_finish_grid -- is
// csrc/conv_stage_train_plans.h, where tests/native/conv_stage_train_plans_host.cpp reads it.
#include "conv_stage_train_plans.h"
#include "mms_internal.h"

namespace mms {
namespace {

// the refusal of the shape, the window and the pool, else MMS_OK and *g.  A shape's own refusal comes first; the
// window's and the pool's are the same code.
int train_check(const mms_conv_shape* shape, int ph, int pw, int pool, StageDims* g) {
  const int rc = stage_window_check(shape, ph, pw, g);
  if (rc != MMS_OK) return rc;
  if (pool != MMS_STAGE_POOL_AVE && pool != MMS_STAGE_POOL_MAX) return MMS_ERR_INVALID_ARG;
  g->max = pool == MMS_STAGE_POOL_MAX;
  return MMS_OK;
}

// PH, PW > 0: the window's size at compile time (== s.ph, s.pw); 0: any window.
template <bool MAX, int PH, int PW>
struct TrainEpilogue {
  const TrainArgs& s;
  float* tile;
  // Nothing is kept across the product loop: its register budget is csrc/conv.hip's less the store offsets.
  __device__ __forceinline__ void pixel(const ConvProdArgs&, const ConvTile&, int, int, int, int) {}

  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile& t, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, PS = s.PS;
    const size_t PI = (size_t)a.OHt * a.OWt;
    // pixel p = (image p / per, row, column) of the band: rows are whole, so its place in the map is oy0 OWt + p % per
    size_t yoff[kConvNT];
#pragma unroll
    for (int nt = 0; nt < kConvNT; ++nt) {
      const int p = pvalid[nt] ? (wave + 4 * nt) * 16 + l16 : 0, img = p / t.per;
      yoff[nt] = (size_t)(t.n0 + img) * a.Cout * PI + (size_t)t.oy0 * a.OWt + (p - img * t.per);
    }
    stage_tile_store(a, tile, PS, acc, pvalid, [y = a.out, &yoff, PI](int nt, int m, float v) { y[yoff[nt] + (size_t)m * PI] = v; });
    constexpr int TK = kConvThreads / (16 * MT);        // adjacent lanes per channel: 16, 8, 4
    const int k = tid / TK, j = tid - k * TK;
    const int ph = PH > 0 ? PH : s.ph, pw = PW > 0 ? PW : s.pw;
    float s0 = 0.f, s1 = 0.f;
    if (k < a.Cout) {
      const int wper = t.rb / ph * s.POW;               // windows of the band: per image
      const int PP = s.POH * s.POW, q0 = t.oy0 / ph * s.POW;
      const float ke = (float)(ph * pw);
      int dir = 0;
      if constexpr (MAX) dir = bp_dir(s.scale[k]);
      const auto element = [&](bool first, float v, float* m) {
        if constexpr (MAX) bp_keep(first, v, dir, m);
        else *m += v;
        s0 += v;
        s1 += v * v;
      };
      for (int e = j; e < t.gc * wper; e += TK) {
        const int img = e / wper, q = e - img * wper, wr = q / s.POW, wc = q - wr * s.POW;
        const float* src = tile + k * PS + img * t.per + wr * ph * a.OWt + wc * pw;
        float m = 0.f;                                  // AVE: the window's sum; MAX: its extremum
        if constexpr (PH > 0) {
          float v[PH][PW];
#pragma unroll
          for (int i = 0; i < PH; ++i)
#pragma unroll
            for (int c = 0; c < PW; ++c) v[i][c] = src[i * a.OWt + c];
#pragma unroll
          for (int i = 0; i < PH; ++i)
#pragma unroll
            for (int c = 0; c < PW; ++c) element(i == 0 && c == 0, v[i][c], &m);
        } else {
          for (int i = 0; i < ph; ++i)
            for (int c = 0; c < pw; ++c) element(i == 0 && c == 0, src[i * a.OWt + c], &m);
        }
        s.save_pool[((size_t)(t.n0 + img) * a.Cout + k) * PP + q0 + q] = MAX ? m : m / ke;
      }
    }
    // every lane takes part: the TK lanes of a channel are an aligned run of one wave
#pragma unroll
    for (int d = 1; d < TK; d <<= 1) {
      s0 += __shfl_xor(s0, d);
      s1 += __shfl_xor(s1, d);
    }
    if (k < a.Cout && j == 0) {
      const size_t wg = (size_t)blockIdx.x * gridDim.y + blockIdx.y;
      float* o = s.part + ((size_t)k * s.groups + wg) * 2;
      o[0] = s0;
      o[1] = s1;
    }
  }
};

template <int MT, bool MAX, int PH, int PW>
__global__ __launch_bounds__(kConvThreads) void train_product_kernel(TrainArgs s) {
  extern __shared__ float conv_lds[];
  TrainEpilogue<MAX, PH, PW> epi{s, conv_lds};
  conv_tile_product<MT>(s.p, conv_lds, epi);
}

// Launch 2: grid (K, chunks), kBnThreads threads.  Windows [y wpc, (y + 1) wpc) of the channel's N * PP.
__global__ __launch_bounds__(kBnThreads) void train_finish_kernel(
    const float* __restrict__ part, int groups, const float* __restrict__ scale, const float* __restrict__ shift,
    float* running_mean, float* running_var, float* __restrict__ top, float* save_pool, float* save_mean,
    float* save_std, unsigned K, unsigned PP, unsigned windows, unsigned wpc, float bn_memory, float inv_S,
    float inv_N) {
  __shared__ float red[2 * kBnThreads / kWave];
  const unsigned c = blockIdx.x;
  const float* p = part + (size_t)c * groups * 2;
  float tot[2] = {0.f, 0.f};
  for (int g = threadIdx.x; g < groups; g += kBnThreads) {
    tot[0] += p[2 * g];
    tot[1] += p[2 * g + 1];
  }
  bn_block_sum<kBnThreads, 2>(tot, red);
  float nmean, std;
  bn_statistics(tot, (int)c, blockIdx.y == 0 && threadIdx.x == 0, bn_memory, inv_S, inv_N, running_mean, running_var,
                save_mean, save_std, &nmean, &std);
  const float sc = scale[c], sh = shift[c];
  const unsigned w0 = blockIdx.y * wpc, w1 = windows - w0 < wpc ? windows : w0 + wpc;
  for (unsigned w = w0 + threadIdx.x; w < w1; w += kBnThreads) {
    const unsigned n = w / PP, r = w - n * PP;
    const size_t o = ((size_t)n * K + c) * PP + r;
    float sp;
    const float t = bn_pool_train_finish(save_pool[o], nmean, std, sc, sh, &sp);
    save_pool[o] = sp;
    top[o] = t;
  }
}

template <typename T>
size_t bn_bytes(const StageDims& g) {
  return Abi<T>::bn_pool_tanh_workspace_bytes(g.d.N, g.d.K, g.d.OH, g.d.OW, g.ph, g.pw);
}

// The backward's workspace with every output: [dy][the BN call's][the convolution's], the first two rounded to 16 bytes.
template <typename T>
struct BackwardCarve {
  size_t dy, bn, conv;
  size_t all() const { return dy + bn + conv; }
};
template <typename T>
BackwardCarve<T> backward_carve(const mms_conv_shape* shape, const StageDims& g) {
  const size_t map = (size_t)g.d.N * g.d.K * g.d.OH * g.d.OW;
  return {round_up(map * sizeof(T), 16), round_up(bn_bytes<T>(g), 16), Abi<T>::conv_workspace_bytes(shape)};
}

enum { kAuto = -1, kSequence = MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE, kFused = MMS_CONV_STAGE_TRAIN_ROUTE_FUSED };

// What the forward needs on `force` (kAuto: train_route decides; kFused where it does not reach: 0).
template <typename T>
size_t forward_bytes(const StageDims& g, int force) {
  if (std::is_same<T, float>::value && force != kSequence) {
    const TrainArgs a = train_plan(g);
    if (force == kFused) return a.p.ok ? fused_bytes(a) : 0;
    if (train_route(g) == MMS_CONV_STAGE_TRAIN_ROUTE_FUSED) return fused_bytes(a);
  }
  return bn_bytes<T>(g);
}

template <typename T>
size_t train_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool, int force) {
  StageDims g;
  if (train_check(shape, ph, pw, pool, &g) != MMS_OK || g.d.N == 0) return 0;
  if (force == kFused && !train_plan(g).p.ok) return 0;
  const size_t f = forward_bytes<T>(g, force), b = backward_carve<T>(shape, g).all();
  return f > b ? f : b;
}

// the BN -> pool -> TanH backward of g's method; shift is an input of the MAX form only
template <typename T>
int bn_bwd(const StageDims& g, const T* y, const T* top, const T* td, const T* sp, const T* sc, const T* sh, const T* sm,
           const T* ss, T* dy, T* dsc, T* dsh, void* ws, size_t wsb, void* st) {
  const int N = g.d.N, K = g.d.K, OH = g.d.OH, OW = g.d.OW;
  return g.max ? Abi<T>::bn_maxpool_tanh_backward(N, K, OH, OW, g.ph, g.pw, y, top, td, sp, sc, sh, sm, ss, dy, dsc, dsh,
                                                  ws, wsb, st)
               : Abi<T>::bn_pool_tanh_backward(N, K, OH, OW, g.ph, g.pw, y, top, td, sp, sc, sm, ss, dy, dsc, dsh, ws,
                                               wsb, st);
}

template <typename T>
int train_forward(const mms_conv_shape* shape, int ph, int pw, int pool, T bn_memory, const T* x, const T* w,
                  const T* bias, const T* scale, const T* shift, T* running_mean, T* running_var, T* y, T* top,
                  T* save_pool, T* save_mean, T* save_std, void* workspace, size_t workspace_bytes, int force,
                  void* stream) {
  StageDims g;
  const int rc = train_check(shape, ph, pw, pool, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !scale || !shift || !running_mean || !running_var || !y || !top || !save_pool || !save_mean ||
      !save_std)
    return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, w, bias, scale, shift};
  const void* const outputs[] = {y, top, save_pool, save_mean, save_std, running_mean, running_var};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  if constexpr (std::is_same<T, float>::value) {
    if (force == kFused && !train_plan(g).p.ok) return MMS_ERR_UNSUPPORTED;
    if (force == kFused || (force == kAuto && train_route(g) == MMS_CONV_STAGE_TRAIN_ROUTE_FUSED)) {
      TrainArgs a = train_plan(g);
      if (!workspace || workspace_bytes < fused_bytes(a)) return MMS_ERR_WORKSPACE;
      a.p.in = x; a.p.w = w; a.p.bias = bias; a.p.out = y;
      a.scale = scale; a.save_pool = save_pool; a.part = static_cast<float*>(workspace);
      const dim3 grid((unsigned)((a.p.N + a.p.G - 1) / a.p.G), (unsigned)a.p.bands);
      conv_with_mt(a.p.MT, [&](auto M) {
        with_bool(g.max, [&](auto MAX) {
          stage_pool_dispatch<decltype(MAX)::value>(ph, pw, [&](auto PH, auto PW) {
            hipLaunchKernelGGL(
                (train_product_kernel<decltype(M)::value, decltype(MAX)::value, decltype(PH)::value, decltype(PW)::value>),
                grid, dim3(kConvThreads), a.lds_bytes, as_stream(stream), a);
          });
        });
      });
      const int rc1 = launch_status();
      if (rc1 != MMS_OK) return rc1;
      const unsigned PP = (unsigned)(g.POH * g.POW);
      const TrainFinishGrid f = train_finish_grid(g.d.N, PP);
      const dim3 grid2((unsigned)g.d.K, f.chunks);
      hipLaunchKernelGGL(train_finish_kernel, grid2, dim3(kBnThreads), 0, as_stream(stream), (const float*)a.part,
                         a.groups, scale, shift, running_mean, running_var, top, save_pool, save_mean, save_std,
                         (unsigned)g.d.K, PP, f.windows, f.wpc, bn_memory, (float)(1. / ((double)g.d.OH * g.d.OW)),
                         (float)(1. / g.d.N));
      return launch_status();
    }
  }
  const size_t need = bn_bytes<T>(g);
  if (need && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  const int rc1 = Abi<T>::conv_forward(shape, x, w, bias, y, nullptr, 0, stream);
  if (rc1 != MMS_OK) return rc1;
  const auto bn_pool_tanh = g.max ? Abi<T>::bn_maxpool_tanh_forward : Abi<T>::bn_pool_tanh_forward;
  return bn_pool_tanh(0, g.d.N, g.d.K, g.d.OH, g.d.OW, g.ph, g.pw, bn_memory, y, scale, shift, running_mean, running_var,
                      top, save_pool, save_mean, save_std, workspace, workspace_bytes, stream);
}

template <typename T>
int train_backward(const mms_conv_shape* shape, int ph, int pw, int pool, const T* x, const T* w, const T* y,
                   const T* top, const T* top_diff, const T* save_pool, const T* scale, const T* shift,
                   const T* save_mean, const T* save_std, T* dx, T* dw, T* db, T* dscale, T* dshift, void* workspace,
                   size_t workspace_bytes, void* stream) {
  StageDims g;
  const int rc = train_check(shape, ph, pw, pool, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !y || !top || !top_diff || !save_pool || !scale || (g.max && !shift) || !save_mean || !save_std ||
      (!dx && !dw && !db && !dscale && !dshift))
    return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, w, y, top, top_diff, save_pool, scale, shift, save_mean, save_std};
  const void* const outputs[] = {dx, dw, db, dscale, dshift};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  const bool conv = dx || dw || db;
  const BackwardCarve<T> carve = backward_carve<T>(shape, g);
  const size_t need = conv ? carve.all() : bn_bytes<T>(g);
  if (need && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  T* dy = conv ? reinterpret_cast<T*>(base) : nullptr;
  void* bn_ws = conv ? base + carve.dy : base;
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  const int rc1 = bn_bwd(g, y, top, top_diff, save_pool, scale, shift, save_mean, save_std, dy, dscale, dshift, bn_ws,
                         bn_bytes<T>(g), stream);
  if (rc1 != MMS_OK || !conv) return rc1;
  return Abi<T>::conv_backward(shape, x, w, dy, dx, dw, db, base + carve.dy + carve.bn, carve.conv, stream);
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_conv_stage_train_route(const mms_conv_shape* shape, int ph, int pw, int pool) {
  StageDims g;
  if (train_check(shape, ph, pw, pool, &g) != MMS_OK) return MMS_CONV_STAGE_TRAIN_ROUTE_NONE;
  return train_route(g);
}

size_t mms_conv_stage_train_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool) {
  return train_workspace_bytes<float>(shape, ph, pw, pool, kAuto);
}
size_t mms_conv_stage_train_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw, int pool) {
  return train_workspace_bytes<double>(shape, ph, pw, pool, kSequence);
}
size_t mms_conv_stage_train_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool) {
  return train_workspace_bytes<float>(shape, ph, pw, pool, kSequence);
}
size_t mms_conv_stage_train_fused_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool) {
  return train_workspace_bytes<float>(shape, ph, pw, pool, kFused);
}

int mms_conv_stage_train_forward_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                     const float* x, const float* weight, const float* bias, const float* scale,
                                     const float* shift, float* running_mean, float* running_var, float* y, float* top,
                                     float* save_pool, float* save_mean, float* save_std, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return train_forward<float>(shape, ph, pw, pool, bn_memory, x, weight, bias, scale, shift, running_mean, running_var,
                              y, top, save_pool, save_mean, save_std, workspace, workspace_bytes, kAuto, stream);
}

int mms_conv_stage_train_forward_f64(const mms_conv_shape* shape, int ph, int pw, int pool, double bn_memory,
                                     const double* x, const double* weight, const double* bias, const double* scale,
                                     const double* shift, double* running_mean, double* running_var, double* y,
                                     double* top, double* save_pool, double* save_mean, double* save_std,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return train_forward<double>(shape, ph, pw, pool, bn_memory, x, weight, bias, scale, shift, running_mean, running_var,
                               y, top, save_pool, save_mean, save_std, workspace, workspace_bytes, kSequence, stream);
}

int mms_conv_stage_train_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                              const float* x, const float* weight, const float* bias,
                                              const float* scale, const float* shift, float* running_mean,
                                              float* running_var, float* y, float* top, float* save_pool,
                                              float* save_mean, float* save_std, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return train_forward<float>(shape, ph, pw, pool, bn_memory, x, weight, bias, scale, shift, running_mean, running_var,
                              y, top, save_pool, save_mean, save_std, workspace, workspace_bytes, kSequence, stream);
}

int mms_conv_stage_train_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                           const float* x, const float* weight, const float* bias, const float* scale,
                                           const float* shift, float* running_mean, float* running_var, float* y,
                                           float* top, float* save_pool, float* save_mean, float* save_std,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return train_forward<float>(shape, ph, pw, pool, bn_memory, x, weight, bias, scale, shift, running_mean, running_var,
                              y, top, save_pool, save_mean, save_std, workspace, workspace_bytes, kFused, stream);
}

int mms_conv_stage_train_backward_f32(const mms_conv_shape* shape, int ph, int pw, int pool, const float* x,
                                      const float* weight, const float* y, const float* top, const float* top_diff,
                                      const float* save_pool, const float* scale, const float* shift,
                                      const float* save_mean, const float* save_std, float* bottom_diff,
                                      float* weight_diff, float* bias_diff, float* scale_diff, float* shift_diff,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return train_backward<float>(shape, ph, pw, pool, x, weight, y, top, top_diff, save_pool, scale, shift, save_mean,
                               save_std, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, workspace,
                               workspace_bytes, stream);
}

int mms_conv_stage_train_backward_f64(const mms_conv_shape* shape, int ph, int pw, int pool, const double* x,
                                      const double* weight, const double* y, const double* top, const double* top_diff,
                                      const double* save_pool, const double* scale, const double* shift,
                                      const double* save_mean, const double* save_std, double* bottom_diff,
                                      double* weight_diff, double* bias_diff, double* scale_diff, double* shift_diff,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return train_backward<double>(shape, ph, pw, pool, x, weight, y, top, top_diff, save_pool, scale, shift, save_mean,
                                save_std, bottom_diff, weight_diff, bias_diff, scale_diff, shift_diff, workspace,
                                workspace_bytes, stream);
}

}  // extern "C"
