// csrc/conv_pool_tile.h -- what the pooled stages behind csrc/conv_tile.h's product share: csrc/conv_stage.hip (TEST
// phase), csrc/conv_stage_train.hip (TRAIN phase) and csrc/score_tail.hip (the scoring tail).  Each runs
// conv_tile_product with an epilogue that
//
//   1. puts accumulator + bias (conv_tile_word) in LDS as tile[k][pixel], over the band and the weights the last chunk
//      has finished with, between two barriers (stage_tile_store): K <= 64 channels x 256 pixels is the 64 KB those
//      had at most; a row is PS floats (stage_tile_row);
//   2. has a thread walk whole pooling windows of the tile in (h, w) order: AVE adds the window as one chain from 0, MAX
//      scans it with bp_keep from its first element.  The walk is written in each source: a shared form of it changed
//      the kernels' instructions (register allocation, operand order of the packed adds), and the same holds for
//      csrc/score_tail.hip's step 1, which is its own copy;
//   3. finishes the pooled value its own way (a thread's BN constants in TEST phase: StageChannel).
//
// The host side is here once as well: the window's refusal (stage_window_check), the tile's row length and the
// launch's LDS bytes, the windows compiled in (stage_pool_dispatch), what a workgroup holds and a span of workgroup
// counts for the measured routing rules (stage_plan_kind, StageSpan).  The routing thresholds are each source's own; the
// sequence routes call the public entry points through csrc/typed_abi.h and refuse an output that is another array of
// the call with csrc/host_args.h's outputs_alias.
#ifndef MMS_CONV_POOL_TILE_H_
#define MMS_CONV_POOL_TILE_H_

#include "bn_common.h"
#include "conv_tile.h"
#include "host_args.h"
#include "typed_abi.h"

namespace mms {

static_assert(kConvMaxChannels * kConvTilePixels <= kConvLdsFloats, "the accumulator tile of any fast plan fits the LDS");

// ---- host ---------------------------------------------------------------------------------------------------------
struct StageDims {
  ConvDims d;
  int ph, pw, POH, POW;
  bool max;              // the caller's: MaxPool where AvePool has its sum
};

// the refusal of the shape and the window (the windows tile the map), else MMS_OK and *g but g->max
inline int stage_window_check(const mms_conv_shape* shape, int ph, int pw, StageDims* g) {
  const int rc = conv_check(shape, &g->d);
  if (rc != MMS_OK) return rc;
  if (ph < 1 || pw < 1 || g->d.OH % ph || g->d.OW % pw) return MMS_ERR_INVALID_ARG;
  g->ph = ph;
  g->pw = pw;
  g->POH = g->d.OH / ph;
  g->POW = g->d.OW / pw;
  return MMS_OK;
}

// Row length of the accumulator tile [Cout][PS] of a workgroup of P pixels.  Lane groups of an accumulator are four
// channels apart: a row length of 4 or 12 mod 16 puts their 16 pixels in separate banks.  Taken where it still fits.
inline int stage_tile_row(int Cout, int P) {
  int PS = P;
  while (PS % 16 != 4 && PS % 16 != 12) ++PS;
  return Cout * PS > kConvLdsFloats ? P : PS;
}

// The launch's LDS: the tile lies over the product's band and weights.
inline size_t stage_lds_bytes(int Cout, int P, size_t product_bytes) {
  const size_t tile = (size_t)Cout * stage_tile_row(Cout, P) * sizeof(float);
  return tile > product_bytes ? tile : product_bytes;
}

// The product launch's grid is (image groups, bands): its workgroups.
inline long long stage_groups(const ConvProdArgs& p) { return (long long)((p.N + p.G - 1) / p.G) * p.bands; }

// What a workgroup of the plan holds: the measured routing rules are told apart by it.
enum StagePlanKind { kStageImages = 0, kStageRowBand = 1, kStageOneImage = 2 };   // several whole images / rows of one / one
inline StagePlanKind stage_plan_kind(const ConvProdArgs& p) {
  return p.G > 1 ? kStageImages : p.bands > 1 ? kStageRowBand : kStageOneImage;
}

struct StageSpan {
  long long least, most;       // workgroups; {0, -1}: no count
  constexpr bool holds(long long groups) const { return groups >= least && groups <= most; }
};

template <int K>
using stage_int = std::integral_constant<int, K>;

// f(PH, PW) as types.  AVE: network_v4's two windows at compile time, any other at run time.  MAX: 4 x 4 and 2 x 2 at
// compile time, any other -- the nets' 5 x 5 and 6 x 6 included -- at run time.  Against a build with the run-time scan
// only, process by process in turn, the fused launch with the 4 x 4 is 6 to 8 % faster at v3's first stage and with the
// 2 x 2 6 to 7 % (N = 50) and 4 to 5 % (N = 1517) at v5's first and 0.8 to 1.4 % at v5's second, ranges apart in both
// rounds (profiles/conv_maxpool_stage_bench.txt, second section).  A 5 x 5 and a 6 x 6 instantiation gained under 1 %
// where the main call fuses, inside the spread, and are not kept.
template <bool MAX, class F>
void stage_pool_dispatch(int ph, int pw, F&& f) {
  if (ph == 4 && pw == 4) f(stage_int<4>{}, stage_int<4>{});
  else if (!MAX && ph == 5 && pw == 5) f(stage_int<5>{}, stage_int<5>{});
  else if (MAX && ph == 2 && pw == 2) f(stage_int<2>{}, stage_int<2>{});
  else f(stage_int<0>{}, stage_int<0>{});
}

// ---- device -------------------------------------------------------------------------------------------------------
struct StageNothing {
  template <class... A>
  __device__ __forceinline__ void operator()(A...) const {}
};

// Step 1.  The first barrier: every wave has finished with the band and the weights.  also(nt, m, v) is called behind
// each word's store.
template <int MT, class Also = StageNothing>
__device__ __forceinline__ void stage_tile_store(const ConvProdArgs& a, float* tile, int PS,
                                                 const conv_v4f (&acc)[MT][kConvNT], const bool (&pvalid)[kConvNT],
                                                 Also also = Also{}) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * mt + 4 * grp + r;
      if (m >= a.Cout) continue;
      const float b = conv_tile_bias(a, m);
#pragma unroll
      for (int nt = 0; nt < kConvNT; ++nt)
        if (pvalid[nt]) {
          const float v = conv_tile_word(a, acc[mt][nt][r], b);
          tile[m * PS + (wave + 4 * nt) * 16 + l16] = v;
          also(nt, m, v);
        }
    }
  __syncthreads();
}

// A thread's TEST-phase BN constants of channel kc; MAX: with the direction of the channel's scan.
template <bool MAX>
struct StageChannel {
  int kc;
  float nmean, std, sc, sh;
  int dir;               // MAX: bp_dir(sc)
  // s: the kernel's arguments, with mean, var, scale and shift
  template <class Args>
  __device__ __forceinline__ void load(const Args& s, int k) {
    kc = k;
    nmean = -s.mean[k];
    std = bn_sqrt(s.var[k] + 1e-9f);
    sc = s.scale[k];
    sh = s.shift[k];
    if constexpr (MAX) dir = bp_dir(sc);
  }
};

}  // namespace mms
#endif  // MMS_CONV_POOL_TILE_H_
