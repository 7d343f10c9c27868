// csrc/score_tail.hip -- the scoring tail Convolution -> BN -> Pool -> TanH -> head -> prob as one call
// (include/mms_score_tail.h: mms_score_tail_*) and its extern "C" entry points.  With flt = Flatten of the stage's top:
//
//   flt[n, k]   = tanh(BN(pool_window(conv(x, w) + bias)))          csrc/conv_stage.hip, AVE or MAX
//   h[n, :]     = tanh([flt[n] | overlap[n]] . w1^T + b1)           csrc/head.hip, TEST phase
//   prob[n, :]  = softmax(h[n] . w2^T + b2)        loss = -sum_n log(max(prob[n, label_n], FLT_MIN)) / normalizer
//
// Two routes (tail_route, the one place that decides):
//
//   sequence  mms_conv_stage_forward_* (MAX: mms_conv_maxpool_stage_forward_*) into flt, then mms_head_forward_* from
//             it: the two public calls on the routes they choose, nothing of their own here.  All of double; float where
//             the fused route does not reach or does not pay.
//             Workspace: [the stage call's][flt: N F0][h: N H][the head call's], each rounded up to 16 bytes; flt and
//             h there are used when the caller passes none.
//   fused     float, where tail_plan says ok.  The product is conv_tile_product with conv_prod_plan's chunks (CC) and
//             whole images per workgroup: kTailImages of them at most, the tail's own choice (below), not the stage's.  Before the
//             product the workgroup stages w1, w2, the biases and its images' overlap rows into a region of LDS behind
//             the convolution's.  The epilogue's steps are those csrc/conv_pool_tile.h lists, the window being the
//             image's whole map; thread e takes (image, channel) e, e + 256, ... and finishes with
//             bn_pool_test_finish / bn_maxpool_test_finish; the value goes to the image's feat row in LDS (and to
//             flt where asked).  Then csrc/head_tile.h's steps on those rows: fc1
//             blocks of 16 samples x 16 hidden units dealt to the four waves, fc2 one thread per (sample, class),
//             softmax one thread per sample.  With a loss each sample's term and whether it counts go to the workspace
//             and head_loss_from_terms (csrc/head.hip), one thread, adds them in ascending n: a second launch.
//
// A value of flt, h or prob is the same chain of operations on both routes: the convolution's chunks are the
// convolution's own (tail_plan refuses a plan that would cut them differently) and every later step is per sample.
#include "conv_pool_tile.h"
#include "head_tile.h"
#include "mms_conv_maxpool_stage.h"
#include "mms_conv_stage.h"
#include "mms_internal.h"
#include "mms_score_tail.h"

namespace mms {
namespace {

constexpr int kTailMaxLdsBytes = 163840;   // the fused kernel's dynamic LDS, at most: the CU's 160 KB
// Images of a workgroup, at most: the tail's own choice, not the stage's 256 pixels' worth (ten 5 x 5 maps, seven 6 x 6).
// Measured (profiles/score_tail_bench.txt, builds that differ in this constant only): network_v4's tail takes 144 / 199 /
// 193 / 207 us at N = 50 / 100 / 400 / 1517 with the stage's ten, 146 / 149 / 179 us at N = 100 / 400 / 1517 with five and
// 133 / 134 / 139 / 162 us with three; network_v5's last stage 65 / 78 us at N = 50 / 1517 with seven, 56 / 76 with five,
// 47 / 62 with three.  A workgroup's time is its chain of channel chunks, each staged behind a barrier, and the product of
// up to sixteen pixel tiles: fewer images make each chunk's staging and product shorter and put more workgroups on the
// 256 CUs, which sit idle at these batch sizes.  Three is the fewest measured; one and two are not.
constexpr int kTailImages = 3;

struct TailDims : StageDims {
  mms_head_shape hs;         // the head call's shape
  HeadDims hd;
};

// the refusal of the shape, else MMS_OK and *g
int tail_check(const mms_score_tail_shape* s, TailDims* g) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->pool != MMS_STAGE_POOL_AVE && s->pool != MMS_STAGE_POOL_MAX) return MMS_ERR_INVALID_ARG;
  const int rc = stage_window_check(&s->conv, s->ph, s->pw, g);
  if (rc != MMS_OK) return rc;
  g->max = s->pool == MMS_STAGE_POOL_MAX;
  const long long F0 = (long long)g->d.K * g->POH * g->POW;       // at most K OH OW, which conv_check bounds
  g->hs = {g->d.N, (int)F0, s->F1, s->H, s->C, MMS_HEAD_TEST, 0.5f, s->normalization, s->has_ignore_label,
           s->ignore_label};
  return head_check(&g->hs, &g->hd);
}

struct TailArgs {
  ConvProdArgs p;            // conv_prod_plan(d, forward, ph) with G cut to the tail's; p.out is not used
  const float *mean, *var, *scale, *shift;
  const float *overlap, *w1, *b1, *w2, *b2, *label;
  float *flt, *h, *prob;     // flt, h: or NULL
  float* terms;              // (N) in the workspace, or NULL: no loss
  int* valid;                // (N)
  HeadDims hd;
  HeadFastPlan hp;
  int PS;                    // row length of the accumulator tile [Cout][PS]
  int rows;                  // rows of the head's tile: G rounded up to 16
  int head_off;              // floats from the start of the LDS to the head's region
  size_t lds_bytes;
  bool ok;
};

// ok false: the fused launch does not reach this shape.
TailArgs tail_plan(const TailDims& g, int images) {
  TailArgs a = {};
  if (g.d.OH != g.ph || g.d.OW != g.pw) return a;
  a.p = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, g.ph);
  if (!a.p.ok || a.p.bands != 1) return a;
  // the same chunks of input channels as the convolution's own launch, so the same words as the sequence
  const ConvProdArgs own = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1);
  if (!own.ok || own.CC != a.p.CC) return a;
  a.hp = head_fast_plan(g.hd);
  if (!a.hp.ok) return a;
  if (a.p.G > images) a.p.G = images;
  const int Mpad = 16 * a.p.MT;
  a.p.lds_bytes = ((size_t)a.p.G * a.p.CC * a.p.plane + (size_t)Mpad * a.p.Kpad + a.p.Kpad) * sizeof(float);
  const int P = a.p.G * a.p.OHt * a.p.OWt;
  a.PS = stage_tile_row(a.p.Cout, P);
  const size_t conv_bytes = stage_lds_bytes(a.p.Cout, P, a.p.lds_bytes);
  a.head_off = (int)((conv_bytes + sizeof(float) - 1) / sizeof(float));
  a.rows = (a.p.G + 15) / 16 * 16;
  a.hd = g.hd;
  a.lds_bytes = ((size_t)a.head_off + head_fwd_lds_floats(g.hd, a.hp, a.rows)) * sizeof(float);
  a.ok = a.lds_bytes <= (size_t)kTailMaxLdsBytes;
  return a;
}

// The one routing decision, for a shape tail_check accepts.  The measured rule (tools/bench_score_tail.py,
// profiles/score_tail_bench.txt: fused against sequence, median of seven alternating passes, the two ranges apart at
// every point).  Measured: workgroups of several whole small images -- network_v4's tail (AVE 5 x 5) at N = 50, 100, 400
// and 1517, which is 17, 34, 134 and 506 workgroups of three: 1.53, 1.60, 1.50 and 1.31 x; network_v5's last stage
// (MAX 6 x 6) at N = 50 and 1517, 17 and 506 workgroups: 1.64 and 1.41 x.  FUSED on the workgroup counts between the
// fewest and the most measured; fewer than 17 and more than 506 are not measured and go to the sequence, as does a
// workgroup of one image of 129 to 256 pixels, which no net of the driver has.
constexpr StageSpan kTailGroups = {17, 506};   // N = 50, N = 1517

int tail_route(const TailDims& g) {
  const TailArgs a = tail_plan(g, kTailImages);
  if (!a.ok) return MMS_SCORE_TAIL_ROUTE_SEQUENCE;
  const bool small_images = a.p.OHt * a.p.OWt <= kConvTilePixels / 2;      // conv_tile_geometry: G > 1
  return small_images && kTailGroups.holds(stage_groups(a.p)) ? MMS_SCORE_TAIL_ROUTE_FUSED
                                                              : MMS_SCORE_TAIL_ROUTE_SEQUENCE;
}

template <bool MAX>
struct TailEpilogue {
  const TailArgs& s;
  float* tile;
  HeadFwdLds L;
  StageChannel<MAX> ch;      // of the channel whose values follow: that of the thread's first (image, channel)
  // Before the product: the loads are long back when the epilogue, on the workgroup's critical path, needs them.
  __device__ __forceinline__ void pixel(const ConvProdArgs& a, const ConvTile&, int nt, int, int, int) {
    if (nt == 0) ch.load(s, (int)threadIdx.x % a.Cout);
  }

  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile& t, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
    const int PS = s.PS;
    const HeadDims& hd = s.hd;
    const HeadFastPlan& hp = s.hp;
    // stage_tile_store's body, written out: called from here it changed this kernel's register allocation
    __syncthreads();                                    // every wave has finished with the band and the weights
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * grp + r;
        if (m >= a.Cout) continue;
        const float b = conv_tile_bias(a, m);
#pragma unroll
        for (int nt = 0; nt < kConvNT; ++nt)
          if (pvalid[nt]) tile[m * PS + (wave + 4 * nt) * 16 + l16] = conv_tile_word(a, acc[mt][nt][r], b);
      }
    __syncthreads();
    // pool and finish: the window is the image's whole map, one row of t.per = ph pw values in (h, w) order
    const float ke = (float)t.per;
    for (int e = tid; e < t.gc * a.Cout; e += kConvThreads) {
      const int k = e % a.Cout, img = e / a.Cout;
      if (k != ch.kc) ch.load(s, k);
      const float* src = tile + k * PS + img * t.per;
      float sum = 0.f;                                  // AVE: the window's sum; MAX: its extremum
      for (int i = 0; i < t.per; ++i) {
        if constexpr (MAX) bp_keep(i == 0, src[i], ch.dir, &sum);
        else sum += src[i];
      }
      float sp;
      const float tv = MAX ? bn_maxpool_test_finish(sum, ch.nmean, ch.std, ch.sc, ch.sh, &sp)
                           : bn_pool_test_finish(sum, ke, ch.nmean, ch.std, ch.sc, ch.sh, &sp);
      if (s.flt) s.flt[(size_t)(t.n0 + img) * a.Cout + k] = tv;
      L.feats[img * hp.Fa + k] = tv;
    }
    __syncthreads();
    // the head on rows 0 .. gc of the tile: sample t.n0 + row
    const int n0 = t.n0, n1 = t.n0 + t.gc, blocks = s.rows / 16 * hp.HT;
    for (int b = wave; b < blocks; b += kConvThreads / 64)
      head_fc1_block(L, hd, hp, b / hp.HT, b % hp.HT, s.b1 != nullptr, n0, n1, s.h,
                     [](float hv, int, int) { return hv; });         // TEST: Dropout is the identity
    __syncthreads();
    for (int e = tid; e < t.gc * hd.C; e += kConvThreads) head_fc2_one(L, hd, hp, e / hd.C, e % hd.C, s.b2 != nullptr);
    __syncthreads();
    if (tid < t.gc) {
      const int n = n0 + tid;
      int ok;
      const float term =
          head_softmax_row(L, hd, tid, s.prob + (size_t)n * hd.C, s.label ? head_class(hd, s.label[n]) : -1, &ok);
      if (s.terms) {
        s.terms[n] = term;
        s.valid[n] = ok;
      }
    }
  }
};

static_assert(kConvThreads == kHeadThreads, "head_stage_weights strides by the workgroup's threads");

template <int MT, bool MAX>
__global__ __launch_bounds__(kConvThreads) void score_tail_kernel(TailArgs s) {
  extern __shared__ float conv_lds[];
  TailEpilogue<MAX> epi{s, conv_lds, head_fwd_carve(conv_lds + s.head_off, s.hd, s.hp, s.rows)};
  const HeadDims& hd = s.hd;
  const HeadFastPlan& hp = s.hp;
  // The head's region is nobody else's: staged before the product, whose barriers come before its first reader.
  head_stage_weights(epi.L, hd, hp, s.w1, s.b1, s.w2, s.b2);
  const int n0 = blockIdx.x * s.p.G, gc = min(s.p.G, s.p.N - n0);
  for (int e = threadIdx.x; e < s.rows * hp.Fp; e += kConvThreads) {
    const int r = e / hp.Fp, f = e - r * hp.Fp;
    // columns below F0 are the epilogue's; overlap behind them; zeros in the padding and in the rows past the images
    epi.L.feats[r * hp.Fa + f] =
        (r < gc && f >= hd.F0 && f < hd.F) ? s.overlap[(size_t)(n0 + r) * hd.F1 + (f - hd.F0)] : 0.f;
  }
  conv_tile_product<MT>(s.p, conv_lds, epi);
}

struct TailSequenceWorkspace {
  size_t stage, flt, h, head, total;       // bytes of each part; flt and h start at offsets rounded up to 16
};

template <typename T>
TailSequenceWorkspace tail_sequence_workspace(const mms_score_tail_shape* s, const TailDims& g) {
  TailSequenceWorkspace w;
  const auto stage_bytes = g.max ? Abi<T>::conv_maxpool_stage_workspace_bytes : Abi<T>::conv_stage_workspace_bytes;
  w.stage = stage_bytes(&s->conv, g.ph, g.pw);
  w.head = Abi<T>::head_workspace_bytes(&g.hs);
  w.flt = (size_t)g.hd.N * g.hd.F0 * sizeof(T);
  w.h = (size_t)g.hd.N * g.hd.H * sizeof(T);
  w.total = round_up(w.stage, 16) + round_up(w.flt, 16) + round_up(w.h, 16) + round_up(w.head, 16);
  return w;
}

inline size_t tail_fused_bytes(const TailDims& g) { return (size_t)g.hd.N * (sizeof(float) + sizeof(int)); }

template <typename T>
size_t tail_workspace_bytes(const mms_score_tail_shape* shape, bool sequence) {       // sequence: whatever the route
  TailDims g;
  if (tail_check(shape, &g) != MMS_OK || g.d.N == 0) return 0;
  if (std::is_same<T, float>::value && !sequence && tail_route(g) == MMS_SCORE_TAIL_ROUTE_FUSED)
    return tail_fused_bytes(g);
  return tail_sequence_workspace<T>(shape, g).total;
}

template <int MT, bool MAX>
int tail_launch(const TailArgs& a, void* stream) {
  static const hipError_t once = allow_dynamic_lds(&score_tail_kernel<MT, MAX>, kTailMaxLdsBytes);
  if (once != hipSuccess) return MMS_ERR_LAUNCH;
  hipLaunchKernelGGL((score_tail_kernel<MT, MAX>), dim3((unsigned)stage_groups(a.p)), dim3(kConvThreads), a.lds_bytes,
                     as_stream(stream), a);
  return launch_status();
}

// force: MMS_SCORE_TAIL_ROUTE_NONE (tail_route decides), _SEQUENCE or _FUSED (float; MMS_ERR_UNSUPPORTED where the fused
// plan does not reach).
template <typename T>
int tail_forward(const mms_score_tail_shape* shape, const T* x, const T* w, const T* bias, const T* mean, const T* var,
                 const T* scale, const T* shift, const T* overlap, const T* w1, const T* b1, const T* w2, const T* b2,
                 const T* label, T* flt, T* h, T* prob, T* loss, void* workspace, size_t workspace_bytes, int force,
                 void* stream) {
  TailDims g;
  int rc = tail_check(shape, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !mean || !var || !scale || !shift) return MMS_ERR_INVALID_ARG;
  if (!w1 || !w2 || !prob || (g.hd.F1 > 0 && !overlap) || (loss && !label)) return MMS_ERR_INVALID_ARG;
  const void* const outs[] = {flt, h, prob, loss};
  const void* const ins[] = {x, w, bias, mean, var, scale, shift, overlap, w1, b1, w2, b2, label};
  if (outputs_alias(outs, ins)) return MMS_ERR_INVALID_ARG;
  if constexpr (std::is_same<T, float>::value) {
    if (force == MMS_SCORE_TAIL_ROUTE_FUSED && !tail_plan(g, kTailImages).ok) return MMS_ERR_UNSUPPORTED;
    if (force == MMS_SCORE_TAIL_ROUTE_FUSED ||
        (force == MMS_SCORE_TAIL_ROUTE_NONE && tail_route(g) == MMS_SCORE_TAIL_ROUTE_FUSED)) {
      if (loss && (!workspace || workspace_bytes < tail_fused_bytes(g))) return MMS_ERR_WORKSPACE;
      TailArgs a = tail_plan(g, kTailImages);
      a.p.in = x; a.p.w = w; a.p.bias = bias; a.p.out = nullptr;
      a.mean = mean; a.var = var; a.scale = scale; a.shift = shift;
      a.overlap = overlap; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.label = label;
      a.flt = flt; a.h = h; a.prob = prob;
      if (loss) {
        a.terms = static_cast<float*>(workspace);
        a.valid = reinterpret_cast<int*>(a.terms + g.hd.N);
      }
      conv_with_mt(a.p.MT, [&](auto M) {
        rc = g.max ? tail_launch<decltype(M)::value, true>(a, stream) : tail_launch<decltype(M)::value, false>(a, stream);
      });
      if (rc != MMS_OK || !loss) return rc;
      return head_loss_from_terms(a.terms, a.valid, g.hd, loss, as_stream(stream));
    }
  }
  const TailSequenceWorkspace ws = tail_sequence_workspace<T>(shape, g);
  if (!workspace || workspace_bytes < ws.total) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  void* stage_ws = base;
  T* flt_ws = reinterpret_cast<T*>(base + round_up(ws.stage, 16));
  T* h_ws = reinterpret_cast<T*>(base + round_up(ws.stage, 16) + round_up(ws.flt, 16));
  void* head_ws = base + round_up(ws.stage, 16) + round_up(ws.flt, 16) + round_up(ws.h, 16);
  T* f = flt ? flt : flt_ws;
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  const auto stage_forward = g.max ? Abi<T>::conv_maxpool_stage_forward : Abi<T>::conv_stage_forward;
  rc = stage_forward(&shape->conv, g.ph, g.pw, x, w, bias, mean, var, scale, shift, f, nullptr, stage_ws, ws.stage, stream);
  if (rc != MMS_OK) return rc;
  return Abi<T>::head_forward(&g.hs, f, overlap, w1, b1, nullptr, w2, b2, label, h ? h : h_ws, prob, loss, head_ws,
                              ws.head, stream);
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_score_tail_route(const mms_score_tail_shape* shape) {
  TailDims g;
  if (tail_check(shape, &g) != MMS_OK) return MMS_SCORE_TAIL_ROUTE_NONE;
  return tail_route(g);
}

size_t mms_score_tail_workspace_bytes(const mms_score_tail_shape* shape) {
  return tail_workspace_bytes<float>(shape, false);
}
size_t mms_score_tail_workspace_bytes_f64(const mms_score_tail_shape* shape) {
  return tail_workspace_bytes<double>(shape, false);
}
size_t mms_score_tail_sequence_workspace_bytes(const mms_score_tail_shape* shape) {
  return tail_workspace_bytes<float>(shape, true);
}

int mms_score_tail_forward_f32(const mms_score_tail_shape* shape, const float* x, const float* weight, const float* bias,
                               const float* mean, const float* var, const float* scale, const float* shift,
                               const float* overlap, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* label, float* flt, float* h, float* prob, float* loss, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return tail_forward<float>(shape, x, weight, bias, mean, var, scale, shift, overlap, w1, b1, w2, b2, label, flt, h,
                             prob, loss, workspace, workspace_bytes, MMS_SCORE_TAIL_ROUTE_NONE, stream);
}

int mms_score_tail_forward_f64(const mms_score_tail_shape* shape, const double* x, const double* weight,
                               const double* bias, const double* mean, const double* var, const double* scale,
                               const double* shift, const double* overlap, const double* w1, const double* b1,
                               const double* w2, const double* b2, const double* label, double* flt, double* h,
                               double* prob, double* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return tail_forward<double>(shape, x, weight, bias, mean, var, scale, shift, overlap, w1, b1, w2, b2, label, flt, h,
                              prob, loss, workspace, workspace_bytes, MMS_SCORE_TAIL_ROUTE_SEQUENCE, stream);
}

int mms_score_tail_forward_sequence_f32(const mms_score_tail_shape* shape, const float* x, const float* weight,
                                        const float* bias, const float* mean, const float* var, const float* scale,
                                        const float* shift, const float* overlap, const float* w1, const float* b1,
                                        const float* w2, const float* b2, const float* label, float* flt, float* h,
                                        float* prob, float* loss, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return tail_forward<float>(shape, x, weight, bias, mean, var, scale, shift, overlap, w1, b1, w2, b2, label, flt, h,
                             prob, loss, workspace, workspace_bytes, MMS_SCORE_TAIL_ROUTE_SEQUENCE, stream);
}

int mms_score_tail_forward_fused_f32(const mms_score_tail_shape* shape, const float* x, const float* weight,
                                     const float* bias, const float* mean, const float* var, const float* scale,
                                     const float* shift, const float* overlap, const float* w1, const float* b1,
                                     const float* w2, const float* b2, const float* label, float* flt, float* h,
                                     float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return tail_forward<float>(shape, x, weight, bias, mean, var, scale, shift, overlap, w1, b1, w2, b2, label, flt, h,
                             prob, loss, workspace, workspace_bytes, MMS_SCORE_TAIL_ROUTE_FUSED, stream);
}

}  // extern "C"
