// csrc/train_tail.hip -- the TRAIN-phase tail Convolution -> BN -> Pool -> TanH -> head as one forward and one backward
// call (include/mms_train_tail.h: mms_train_tail_*) and its extern "C" entry points.  With flt = Flatten of the stage's
// top, the window being the whole map:
//
//   y           = conv(x, w) + bias                                  csrc/conv.hip
//   flt[n, k]   = tanh(BN_batch(pool_window(y[n, k])))               csrc/bn_pool.hip, TRAIN phase: batch statistics
//   h[n, :]     = tanh([flt[n] | overlap[n]] . w1^T + b1)            csrc/head.hip, TRAIN phase
//   prob[n, :]  = softmax(Dropout(h[n]) . w2^T + b2)   loss = -sum_n log(max(prob[n, label_n], FLT_MIN)) / normalizer
//
// Two routes of the forward (train_tail_route, the one place that decides); the backward has the sequence only:
//
//   sequence  mms_conv_stage_train_forward_* into y, flt, save_*, then mms_head_forward_* from flt; backward
//             mms_head_backward_* with x0_diff in the workspace, then mms_conv_stage_train_backward_* with it as
//             top_diff.  The public calls on the routes they choose, nothing of their own here.
//             Workspace: [the stage call's][x0_diff: N K][the head call's], each rounded up to 16 bytes.
//   fused     float, where train_tail_plan says ok: two launches.
//             Launch 1 (train_tail_product_kernel) is conv_tile_product with conv_prod_plan's chunks (CC) and whole
//             images per workgroup, kTrainTailImages at most.  The epilogue's steps are those csrc/conv_pool_tile.h
//             lists; each word of the tile goes to y as well.  The 256 / (16 MT) adjacent lanes that serve channel k
//             take the workgroup's images j, j + T, ...: a lane walks its image's map in (h, w) order, leaves the mean
//             (MAX: the extremum) in save_pool and adds the same values into one sum of y and one of y*y.  The lanes'
//             sums are combined by xor-shuffles -- registers and lanes, no LDS beside the tile -- and lane 0 writes
//             them to the workspace slot of (channel, workgroup).
//             Launch 2 (train_tail_finish_kernel) has one workgroup per kHeadFastSamples samples.  Each stages the
//             head's weights, adds every channel's partials in train_finish_kernel's order (csrc/conv_stage_train.hip:
//             thread t those of workgroups t, t + 256, ..., then bn_block_sum; here kTrainTailFold channels per
//             bn_block_sum), forms the statistics with bn_statistics -- workgroup 0's first thread updates the running
//             blobs and writes save_mean / save_std --, finishes its samples' pooled elements with
//             bn_pool_train_finish into save_pool, flt and the samples' feat rows in LDS, next to their overlap rows,
//             and runs csrc/head_tile.h's steps on those rows.  The loss: one workgroup adds its terms itself, thread 0
//             in ascending n; several leave each sample's term and whether it counts in the workspace for
//             head_loss_from_terms (csrc/head.hip), one thread, the same chain.
#include "conv_pool_tile.h"
#include "head_tile.h"
#include "mms_conv_stage_train.h"
#include "mms_internal.h"
#include "mms_train_tail.h"
#include "train_tail_check.h"

namespace mms {
namespace {

constexpr int kTrainTailMaxLdsBytes = 163840;   // a launch's LDS, at most: the CU's 160 KB
// Images of a workgroup of launch 1, at most: the tail's own choice, not the stage's 256 pixels' worth (ten 5 x 5 maps).
// Measured (profiles/train_tail_bench.txt, builds that differ in this constant only; the forward FUSED, us per call, at
// N = 50 / 100 / 400 / 1517): network_v4's tail 193 / 204 / 231 / 326 with three images, 177 / 180 / 211 / 339 with two,
// 169 / 177 / 237 / 512 with one; network_v3's 321 / 330 / 361 / 495, 275 / 284 / 319 / 511 and 264 / 279 / 355 / 788;
// network_v5's 83 / 90 / 112 / 194, 82 / 86 / 111 / 203 and 72 / 80 / 115 / 252.  One image wins at the training batch
// of 50 at every net, which is what the constant is chosen by: a workgroup's time is its chain of channel chunks, and 50
// workgroups of one image leave the other 206 CUs no worse off than 17 of three.  It loses from N = 400 on, where the
// second launch's workgroups each add N partials per channel; those counts go to the sequence (kTrainTailGroups).
constexpr int kTrainTailImages = 1;
constexpr int kTrainTailFold = 8;               // channels of one bn_block_sum in launch 2

struct TrainTailArgs {
  ConvProdArgs p;            // conv_prod_plan(d, forward, ph) with G cut to the tail's; p.out is y
  const float* scale;        // MAX: the direction of a channel's scan
  float* save_pool;          // (N, K): launch 1 leaves the windows' means / extrema here
  float* part;               // [K][groups][2]: sum y, sum y*y of a workgroup's images
  int PS;                    // row length of the accumulator tile [Cout][PS]
  int groups;                // workgroups of launch 1
  HeadFastPlan hp;
  size_t lds_bytes;          // launch 1
  size_t finish_lds_bytes;   // launch 2, dynamic
  bool ok;
};

constexpr size_t kTrainTailFinishStatic =
    sizeof(float) * (2 * kConvMaxChannels + 2 * kConvMaxChannels * kHeadThreads / kWave);

// ok false: the fused launches do not reach this shape.
TrainTailArgs train_tail_plan(const TrainTailDims& g, int images) {
  TrainTailArgs a = {};
  a.p = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, g.ph);
  if (!a.p.ok || a.p.bands != 1) return a;
  // the same chunks of input channels as the convolution's own launch, so y is the convolution's words
  const ConvProdArgs own = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1);
  if (!own.ok || own.CC != a.p.CC) return a;
  a.hp = head_fast_plan(g.hd);
  if (!a.hp.ok) return a;
  if (a.p.G > images) a.p.G = images;
  const int Mpad = 16 * a.p.MT;
  a.p.lds_bytes = ((size_t)a.p.G * a.p.CC * a.p.plane + (size_t)Mpad * a.p.Kpad + a.p.Kpad) * sizeof(float);
  const int P = a.p.G * a.p.OHt * a.p.OWt;
  a.PS = stage_tile_row(a.p.Cout, P);
  a.lds_bytes = stage_lds_bytes(a.p.Cout, P, a.p.lds_bytes);
  a.groups = (int)stage_groups(a.p);
  a.finish_lds_bytes = a.hp.fwd_lds;
  a.ok = a.lds_bytes <= (size_t)kTrainTailMaxLdsBytes &&
         a.finish_lds_bytes + kTrainTailFinishStatic <= (size_t)kTrainTailMaxLdsBytes;
  return a;
}

// The one routing decision, for a shape train_tail_check accepts.  The measured rule (tools/bench_train_tail.py,
// profiles/train_tail_bench.txt: forced FUSED against the forced sequence, medians of seven alternating passes): FUSED
// on the span of launch-1 workgroup counts -- one per image -- at which the ratio sequence / fused is above 1 and the two
// rows' ranges are apart at every stage of the class; every other count, unmeasured ones included, is the SEQUENCE.
//   AVE (network_v4's tail): 1.27 x at 50 workgroups (168.9 against 213.8 us), 1.29 x at 100; 0.94 x at 400, 0.49 x at
//     1517.  FUSED on 50 .. 100.
//   MAX (network_v3's tail, network_v5's last stage): v3's 1.53, 1.51 and 1.15 x at 50, 100 and 400, 0.59 x at 1517;
//     v5's 1.16 and 1.17 x at 50 and 100, 0.82 x at 400.  FUSED on 50 .. 100, the counts inside both stages' spans.
//   An image of 129 to 256 pixels, which no net of the driver has, is not measured: the sequence.
// [MAX]: workgroups of launch 1
constexpr StageSpan kTrainTailGroups[2] = {{50, 100}, {50, 100}};

int train_tail_route(const TrainTailDims& g) {
  const TrainTailArgs a = train_tail_plan(g, kTrainTailImages);
  if (!a.ok) return MMS_TRAIN_TAIL_ROUTE_SEQUENCE;
  const bool small_images = a.p.OHt * a.p.OWt <= kConvTilePixels / 2;      // the measured class
  return small_images && kTrainTailGroups[g.max].holds(a.groups) ? MMS_TRAIN_TAIL_ROUTE_FUSED
                                                                 : MMS_TRAIN_TAIL_ROUTE_SEQUENCE;
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------
template <bool MAX>
struct TrainTailEpilogue {
  const TrainTailArgs& s;
  float* tile;
  // Nothing is kept across the product loop: its register budget is csrc/conv.hip's less the store offsets.
  __device__ __forceinline__ void pixel(const ConvProdArgs&, const ConvTile&, int, int, int, int) {}

  template <int MT>
  __device__ __forceinline__ void finish(const ConvProdArgs& a, const ConvTile& t, const conv_v4f (&acc)[MT][kConvNT],
                                         const bool (&pvalid)[kConvNT]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, PS = s.PS;
    const size_t PI = (size_t)t.per;                    // whole images: a workgroup's image is its map
    size_t yoff[kConvNT];
#pragma unroll
    for (int nt = 0; nt < kConvNT; ++nt) {
      const int p = pvalid[nt] ? (wave + 4 * nt) * 16 + l16 : 0, img = p / t.per;
      yoff[nt] = (size_t)(t.n0 + img) * a.Cout * PI + (p - img * t.per);
    }
    stage_tile_store(a, tile, PS, acc, pvalid, [y = a.out, &yoff, PI](int nt, int m, float v) { y[yoff[nt] + (size_t)m * PI] = v; });
    constexpr int TK = kConvThreads / (16 * MT);        // adjacent lanes per channel: 16, 8, 4
    const int k = tid / TK, j = tid - k * TK;
    float s0 = 0.f, s1 = 0.f;
    if (k < a.Cout) {
      const float ke = (float)t.per;
      int dir = 0;
      if constexpr (MAX) dir = bp_dir(s.scale[k]);
      // Lanes j of a channel read rows `per` floats apart and channels PS apart (4 or 12 mod 16): the walk's reads of
      // a wave spread over the banks as the tile's stores did.
      for (int img = j; img < t.gc; img += TK) {
        const float* src = tile + k * PS + img * t.per;
        float m = 0.f;                                  // AVE: the window's sum; MAX: its extremum
        for (int i = 0; i < t.per; ++i) {
          const float v = src[i];
          if constexpr (MAX) bp_keep(i == 0, v, dir, &m);
          else m += v;
          s0 += v;
          s1 += v * v;
        }
        s.save_pool[(size_t)(t.n0 + img) * a.Cout + k] = MAX ? m : m / ke;
      }
    }
    // every lane takes part: the TK lanes of a channel are an aligned run of one wave
#pragma unroll
    for (int d = 1; d < TK; d <<= 1) {
      s0 += __shfl_xor(s0, d);
      s1 += __shfl_xor(s1, d);
    }
    if (k < a.Cout && j == 0) {
      float* o = s.part + ((size_t)k * s.groups + blockIdx.x) * 2;
      o[0] = s0;
      o[1] = s1;
    }
  }
};

template <int MT, bool MAX>
__global__ __launch_bounds__(kConvThreads) void train_tail_product_kernel(TrainTailArgs s) {
  extern __shared__ float conv_lds[];
  TrainTailEpilogue<MAX> epi{s, conv_lds};
  conv_tile_product<MT>(s.p, conv_lds, epi);
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------
struct TrainTailFinishArgs {
  HeadDims hd;
  HeadFastPlan hp;
  const float* part;         // [K][groups][2]
  int groups;
  const float *scale, *shift, *overlap, *w1, *b1, *w2, *b2, *label;
  const unsigned* mask;
  float *running_mean, *running_var, *save_pool, *save_mean, *save_std, *flt, *h, *prob;
  float* loss;               // or NULL
  float* terms;              // (N) in the workspace: several workgroups and a loss; else NULL
  int* valid;                // (N)
  float bn_memory, inv_S, inv_N, drop_scale;
};

static_assert(kConvThreads == kHeadThreads, "head_stage_weights strides by the workgroup's threads");
static_assert(kConvMaxChannels % kTrainTailFold == 0, "whole folds of channels");

__global__ __launch_bounds__(kHeadThreads) void train_tail_finish_kernel(TrainTailFinishArgs s) {
  constexpr int TS = kHeadFastSamples, FOLD = kTrainTailFold, W = kHeadThreads / kWave;
  extern __shared__ float head_lds[];
  __shared__ float red[kConvMaxChannels / FOLD][2 * FOLD * W];     // a fold's own words: no barrier between folds
  __shared__ float stat[2][kConvMaxChannels];                      // -mean, std of every channel
  const HeadDims& d = s.hd;
  const HeadFastPlan& p = s.hp;
  const HeadFwdLds L = head_fwd_carve(head_lds, d, p, TS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
  const int K = d.F0;

  head_stage_weights(L, d, p, s.w1, s.b1, s.w2, s.b2);

  // every channel's statistics, in every workgroup, in one order: a function of the counts alone
  for (int c0 = 0; c0 < K; c0 += FOLD) {
    float tot[2 * FOLD];
#pragma unroll
    for (int q = 0; q < FOLD; ++q) {
      tot[2 * q] = tot[2 * q + 1] = 0.f;
      if (c0 + q < K) {
        const float* pc = s.part + (size_t)(c0 + q) * s.groups * 2;
        for (int g = tid; g < s.groups; g += kHeadThreads) {
          tot[2 * q] += pc[2 * g];
          tot[2 * q + 1] += pc[2 * g + 1];
        }
      }
    }
    bn_block_sum<kHeadThreads, 2 * FOLD>(tot, red[c0 / FOLD]);
#pragma unroll
    for (int q = 0; q < FOLD; ++q) {
      if (c0 + q < K) {
        const float tq[2] = {tot[2 * q], tot[2 * q + 1]};
        float nmean, std;
        bn_statistics(tq, c0 + q, blockIdx.x == 0 && tid == 0, s.bn_memory, s.inv_S, s.inv_N, s.running_mean,
                      s.running_var, s.save_mean, s.save_std, &nmean, &std);
        if (tid == 0) {
          stat[0][c0 + q] = nmean;
          stat[1][c0 + q] = std;
        }
      }
    }
  }
  __syncthreads();

  // the workgroup's samples: pooled elements finished into save_pool, flt and the feat rows; overlap behind them; zeros
  // in the padding and in the rows past the samples
  const int n0 = blockIdx.x * TS, n1 = min(d.N, n0 + TS);
  for (int e = tid; e < TS * p.Fp; e += kHeadThreads) {
    const int r = e / p.Fp, f = e - r * p.Fp, n = n0 + r;
    float v = 0.f;
    if (n < n1) {
      if (f < K) {
        const size_t o = (size_t)n * K + f;
        float sp;
        v = bn_pool_train_finish(s.save_pool[o], stat[0][f], stat[1][f], s.scale[f], s.shift[f], &sp);
        s.save_pool[o] = sp;
        s.flt[o] = v;
      } else if (f < d.F) {
        v = s.overlap[(size_t)n * d.F1 + (f - K)];
      }
    }
    L.feats[r * p.Fa + f] = v;
  }
  __syncthreads();
  // fc1: rows = this wave's 16 samples, columns = 16 hidden units; tanh and Dropout on the accumulators
  for (int ht = 0; ht < p.HT; ++ht)
    head_fc1_block(L, d, p, wave, ht, s.b1 != nullptr, n0, n1, s.h, [&](float hv, int n, int j) {
      return head_dropout(hv, s.mask[(size_t)n * d.H + j], s.drop_scale);
    });
  __syncthreads();
  // fc2: lane (sample l16 of the wave, classes grp, grp + 4, ...)
  for (int c = grp; c < d.C; c += 4) head_fc2_one(L, d, p, 16 * wave + l16, c, s.b2 != nullptr);
  __syncthreads();
  if (grp == 0) {                            // softmax and the loss term: one lane per sample
    const int row = 16 * wave + l16, n = n0 + row;
    float term = 0.f;
    int ok = 0;
    if (n < n1) {
      term = head_softmax_row(L, d, row, s.prob + (size_t)n * d.C, s.label ? head_class(d, s.label[n]) : -1, &ok);
      if (s.terms) {
        s.terms[n] = term;
        s.valid[n] = ok;
      }
    }
    L.terms[row] = term;
    L.valid[row] = ok;
  }
  if (s.loss && !s.terms) {                  // uniform: the one workgroup holds every sample
    __syncthreads();
    if (tid == 0) {
      float sum = L.terms[0];
      int c = L.valid[0];
      for (int n = 1; n < d.N; ++n) {
        sum += L.terms[n];
        c += L.valid[n];
      }
      *s.loss = sum / head_normalizer<float>(d, c);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct TrainTailCarve {
  size_t stage, x0d, head;   // bytes of each part of the sequence layout, before rounding
  size_t total() const { return round_up(stage, 16) + round_up(x0d, 16) + round_up(head, 16); }
};

template <typename T>
TrainTailCarve train_tail_carve(const mms_score_tail_shape* s, const TrainTailDims& g) {
  TrainTailCarve w;
  w.stage = Abi<T>::conv_stage_train_workspace_bytes(&s->conv, g.ph, g.pw, g.pool);
  w.head = Abi<T>::head_workspace_bytes(&g.hs);
  w.x0d = (size_t)g.hd.N * g.hd.F0 * sizeof(T);
  return w;
}

inline size_t train_tail_part_bytes(const TrainTailArgs& a) { return (size_t)2 * a.p.Cout * a.groups * sizeof(float); }
inline size_t train_tail_fused_bytes(const TrainTailArgs& a, const TrainTailDims& g) {
  return round_up(train_tail_part_bytes(a), 16) + round_up((size_t)g.hd.N * (sizeof(float) + sizeof(int)), 16);
}

enum { kAuto = -1, kSequence = MMS_TRAIN_TAIL_ROUTE_SEQUENCE, kFused = MMS_TRAIN_TAIL_ROUTE_FUSED };

// both passes of a step with the forward on `force` (kFused where it does not reach: 0), for a checked shape, N > 0
template <typename T>
size_t train_tail_bytes(const mms_score_tail_shape* shape, const TrainTailDims& g, int force) {
  const size_t seq = train_tail_carve<T>(shape, g).total();
  if (!std::is_same<T, float>::value || force == kSequence) return seq;
  const TrainTailArgs a = train_tail_plan(g, kTrainTailImages);
  if (force == kFused && !a.ok) return 0;
  if (force == kAuto && train_tail_route(g) != MMS_TRAIN_TAIL_ROUTE_FUSED) return seq;
  const size_t fused = train_tail_fused_bytes(a, g);
  return fused > seq ? fused : seq;
}

template <typename T>
size_t train_tail_workspace_bytes(const mms_score_tail_shape* shape, int force) {
  TrainTailDims g;
  if (train_tail_check(shape, MMS_HEAD_TRAIN, 0.5f, &g) != MMS_OK || g.d.N == 0) return 0;
  return train_tail_bytes<T>(shape, g, force);
}

// force: kAuto (train_tail_route decides), kSequence or kFused (float; MMS_ERR_UNSUPPORTED where the plan refuses)
template <typename T>
int train_tail_forward(const mms_score_tail_shape* shape, int phase, T bn_memory, float dropout_ratio, const T* x,
                       const T* w, const T* bias, const T* scale, const T* shift, T* running_mean, T* running_var,
                       const T* overlap, const T* w1, const T* b1, const unsigned* mask, const T* w2, const T* b2,
                       const T* label, T* y, T* flt, T* save_pool, T* save_mean, T* save_std, T* h, T* prob, T* loss,
                       void* workspace, size_t workspace_bytes, int force, void* stream) {
  TrainTailDims g;
  int rc = train_tail_check(shape, phase, dropout_ratio, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  if (!x || !w || !scale || !shift || !running_mean || !running_var || !w1 || !mask || !w2 || !y || !flt || !save_pool ||
      !save_mean || !save_std || !h || !prob || (g.hd.F1 > 0 && !overlap) || (loss && !label))
    return MMS_ERR_INVALID_ARG;
  const void* const arrays[] = {x,  w,  bias,  scale, shift, running_mean, running_var, overlap,  w1, b1,   mask,
                                w2, b2, label, y,     flt,   save_pool,    save_mean,   save_std, h,  prob, loss};
  const void* const ws_only[] = {workspace};
  if (outputs_alias(arrays, ws_only)) return MMS_ERR_INVALID_ARG;     // any two arrays, the workspace included
  const TrainTailCarve carve = train_tail_carve<T>(shape, g);
  char* base = static_cast<char*>(workspace);
  if constexpr (std::is_same<T, float>::value) {
    if (force == kFused && !train_tail_plan(g, kTrainTailImages).ok) return MMS_ERR_UNSUPPORTED;
    if (force == kFused || (force == kAuto && train_tail_route(g) == MMS_TRAIN_TAIL_ROUTE_FUSED)) {
      if (!workspace || workspace_bytes < train_tail_bytes<float>(shape, g, kFused)) return MMS_ERR_WORKSPACE;
      TrainTailArgs a = train_tail_plan(g, kTrainTailImages);
      a.p.in = x; a.p.w = w; a.p.bias = bias; a.p.out = y;
      a.scale = scale; a.save_pool = save_pool; a.part = reinterpret_cast<float*>(base);
      static const hipError_t once =
          allow_dynamic_lds(&train_tail_finish_kernel, kTrainTailMaxLdsBytes - (int)kTrainTailFinishStatic);
      if (once != hipSuccess) return MMS_ERR_LAUNCH;
      conv_with_mt(a.p.MT, [&](auto M) {
        with_bool(g.max, [&](auto MAX) {
          hipLaunchKernelGGL((train_tail_product_kernel<decltype(M)::value, decltype(MAX)::value>),
                             dim3((unsigned)a.groups), dim3(kConvThreads), a.lds_bytes, as_stream(stream), a);
        });
      });
      if ((rc = launch_status()) != MMS_OK) return rc;
      TrainTailFinishArgs f = {};
      f.hd = g.hd; f.hp = a.hp; f.part = a.part; f.groups = a.groups;
      f.scale = scale; f.shift = shift; f.overlap = overlap; f.w1 = w1; f.b1 = b1; f.w2 = w2; f.b2 = b2; f.label = label;
      f.mask = mask;
      f.running_mean = running_mean; f.running_var = running_var; f.save_pool = save_pool; f.save_mean = save_mean;
      f.save_std = save_std; f.flt = flt; f.h = h; f.prob = prob; f.loss = loss;
      const unsigned finish_groups = (unsigned)((g.hd.N + kHeadFastSamples - 1) / kHeadFastSamples);
      if (loss && finish_groups > 1) {
        f.terms = reinterpret_cast<float*>(base + round_up(train_tail_part_bytes(a), 16));
        f.valid = reinterpret_cast<int*>(f.terms + g.hd.N);
      }
      f.bn_memory = bn_memory;
      f.inv_S = (float)(1. / ((double)g.d.OH * g.d.OW));
      f.inv_N = (float)(1. / g.d.N);
      f.drop_scale = float(1. / (1. - dropout_ratio));          // csrc/head.hip: head_scale
      hipLaunchKernelGGL(train_tail_finish_kernel, dim3(finish_groups), dim3(kHeadThreads), a.finish_lds_bytes,
                         as_stream(stream), f);
      if ((rc = launch_status()) != MMS_OK || !f.terms) return rc;
      return head_loss_from_terms(f.terms, f.valid, g.hd, loss, as_stream(stream));
    }
  }
  if (!workspace || workspace_bytes < carve.total()) return MMS_ERR_WORKSPACE;
  void* head_ws = base + round_up(carve.stage, 16) + round_up(carve.x0d, 16);
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  rc = Abi<T>::conv_stage_train_forward(&shape->conv, g.ph, g.pw, g.pool, bn_memory, x, w, bias, scale, shift,
                                        running_mean, running_var, y, flt, save_pool, save_mean, save_std, base,
                                        carve.stage, stream);
  if (rc != MMS_OK) return rc;
  return Abi<T>::head_forward(&g.hs, flt, overlap, w1, b1, mask, w2, b2, label, h, prob, loss, head_ws, carve.head,
                              stream);
}

template <typename T>
int train_tail_backward(const mms_score_tail_shape* shape, int phase, float dropout_ratio, T loss_weight, const T* x,
                        const T* w, const T* y, const T* flt, const T* save_pool, const T* scale, const T* shift,
                        const T* save_mean, const T* save_std, const T* overlap, const T* w1, const T* w2,
                        const unsigned* mask, const T* h, const T* prob, const T* label, T* dx, T* dw, T* db, T* dscale,
                        T* dshift, T* doverlap, T* w1d, T* b1d, T* w2d, T* b2d, void* workspace, size_t workspace_bytes,
                        void* stream) {
  TrainTailDims g;
  int rc = train_tail_check(shape, phase, dropout_ratio, &g);
  if (rc != MMS_OK) return rc;
  if (g.d.N == 0) return MMS_OK;
  bool stage;
  rc = train_tail_backward_args(g, x, w, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2, mask, h,
                                prob, label, dx, dw, db, dscale, dshift, &doverlap, w1d, b1d, w2d, b2d, workspace, &stage);
  if (rc != MMS_OK) return rc;
  const TrainTailCarve carve = train_tail_carve<T>(shape, g);
  if (!workspace || workspace_bytes < carve.total()) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  T* x0d = stage ? reinterpret_cast<T*>(base + round_up(carve.stage, 16)) : nullptr;
  void* head_ws = base + round_up(carve.stage, 16) + round_up(carve.x0d, 16);
  // Both calls' own refusals have been answered above: neither can refuse after the other has enqueued.
  rc = Abi<T>::head_backward(&g.hs, flt, overlap, w1, w2, mask, h, prob, label, loss_weight, x0d, doverlap, w1d, b1d, w2d,
                             b2d, head_ws, carve.head, stream);
  if (rc != MMS_OK || !stage) return rc;
  return Abi<T>::conv_stage_train_backward(&shape->conv, g.ph, g.pw, g.pool, x, w, y, flt, x0d, save_pool, scale, shift,
                                           save_mean, save_std, dx, dw, db, dscale, dshift, base, carve.stage, stream);
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_train_tail_route(const mms_score_tail_shape* shape) {
  TrainTailDims g;
  if (train_tail_check(shape, MMS_HEAD_TRAIN, 0.5f, &g) != MMS_OK) return MMS_TRAIN_TAIL_ROUTE_NONE;
  return train_tail_route(g);
}

size_t mms_train_tail_workspace_bytes(const mms_score_tail_shape* shape) {
  return train_tail_workspace_bytes<float>(shape, kAuto);
}
size_t mms_train_tail_workspace_bytes_f64(const mms_score_tail_shape* shape) {
  return train_tail_workspace_bytes<double>(shape, kSequence);
}
size_t mms_train_tail_sequence_workspace_bytes(const mms_score_tail_shape* shape) {
  return train_tail_workspace_bytes<float>(shape, kSequence);
}
size_t mms_train_tail_fused_workspace_bytes(const mms_score_tail_shape* shape) {
  return train_tail_workspace_bytes<float>(shape, kFused);
}

#define MMS_TRAIN_TAIL_FORWARD_ARGS(T)                                                                                 \
  const T *x, const T *weight, const T *bias, const T *scale, const T *shift, T *running_mean, T *running_var,        \
      const T *overlap, const T *w1, const T *b1, const unsigned int *mask, const T *w2, const T *b2, const T *label, \
      T *y, T *flt, T *save_pool, T *save_mean, T *save_std, T *h, T *prob, T *loss, void *workspace,                 \
      size_t workspace_bytes, void *stream
#define MMS_TRAIN_TAIL_FORWARD_PASS                                                                                    \
  x, weight, bias, scale, shift, running_mean, running_var, overlap, w1, b1, mask, w2, b2, label, y, flt, save_pool,  \
      save_mean, save_std, h, prob, loss, workspace, workspace_bytes

int mms_train_tail_forward_f32(const mms_score_tail_shape* shape, int phase, float bn_memory, float dropout_ratio,
                               MMS_TRAIN_TAIL_FORWARD_ARGS(float)) {
  return train_tail_forward<float>(shape, phase, bn_memory, dropout_ratio, MMS_TRAIN_TAIL_FORWARD_PASS, kAuto, stream);
}
int mms_train_tail_forward_f64(const mms_score_tail_shape* shape, int phase, double bn_memory, float dropout_ratio,
                               MMS_TRAIN_TAIL_FORWARD_ARGS(double)) {
  return train_tail_forward<double>(shape, phase, bn_memory, dropout_ratio, MMS_TRAIN_TAIL_FORWARD_PASS, kSequence,
                                    stream);
}
int mms_train_tail_forward_sequence_f32(const mms_score_tail_shape* shape, int phase, float bn_memory,
                                        float dropout_ratio, MMS_TRAIN_TAIL_FORWARD_ARGS(float)) {
  return train_tail_forward<float>(shape, phase, bn_memory, dropout_ratio, MMS_TRAIN_TAIL_FORWARD_PASS, kSequence,
                                   stream);
}
int mms_train_tail_forward_fused_f32(const mms_score_tail_shape* shape, int phase, float bn_memory, float dropout_ratio,
                                     MMS_TRAIN_TAIL_FORWARD_ARGS(float)) {
  return train_tail_forward<float>(shape, phase, bn_memory, dropout_ratio, MMS_TRAIN_TAIL_FORWARD_PASS, kFused, stream);
}

#define MMS_TRAIN_TAIL_BACKWARD_ARGS(T)                                                                                \
  const T *x, const T *weight, const T *y, const T *flt, const T *save_pool, const T *scale, const T *shift,          \
      const T *save_mean, const T *save_std, const T *overlap, const T *w1, const T *w2, const unsigned int *mask,    \
      const T *h, const T *prob, const T *label, T *bottom_diff, T *weight_diff, T *bias_diff, T *scale_diff,         \
      T *shift_diff, T *overlap_diff, T *w1_diff, T *b1_diff, T *w2_diff, T *b2_diff, void *workspace,                \
      size_t workspace_bytes, void *stream
#define MMS_TRAIN_TAIL_BACKWARD_PASS                                                                                   \
  x, weight, y, flt, save_pool, scale, shift, save_mean, save_std, overlap, w1, w2, mask, h, prob, label, bottom_diff, \
      weight_diff, bias_diff, scale_diff, shift_diff, overlap_diff, w1_diff, b1_diff, w2_diff, b2_diff, workspace,    \
      workspace_bytes, stream

int mms_train_tail_backward_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio, float loss_weight,
                                MMS_TRAIN_TAIL_BACKWARD_ARGS(float)) {
  return train_tail_backward<float>(shape, phase, dropout_ratio, loss_weight, MMS_TRAIN_TAIL_BACKWARD_PASS);
}
int mms_train_tail_backward_f64(const mms_score_tail_shape* shape, int phase, float dropout_ratio, double loss_weight,
                                MMS_TRAIN_TAIL_BACKWARD_ARGS(double)) {
  return train_tail_backward<double>(shape, phase, dropout_ratio, loss_weight, MMS_TRAIN_TAIL_BACKWARD_PASS);
}

}  // extern "C"
