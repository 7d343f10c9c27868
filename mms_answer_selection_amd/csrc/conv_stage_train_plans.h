// csrc/conv_stage_train_plans.h -- the host-side plans of csrc/conv_stage_train.hip's FUSED forward, in a header so that
// a host program can read them (tests/native/conv_stage_train_plans_host.cpp prints every plan and asserts what the two
// launches rely on): launch 1's arguments and plan (TrainArgs, train_plan), the measured routing rule (kTrainSpans,
// train_route), the partial sums' workspace (fused_bytes) and launch 2's grid (train_finish_grid).  Host text only; the
// kernels are csrc/conv_stage_train.hip's.
#ifndef MMS_CONV_STAGE_TRAIN_PLANS_H_
#define MMS_CONV_STAGE_TRAIN_PLANS_H_

#include "conv_pool_tile.h"
#include "mms_conv_stage_train.h"

namespace mms {

struct TrainArgs {
  ConvProdArgs p;        // the product; p.out is y
  const float* scale;    // MAX: the direction of a channel's scan
  float* save_pool;      // (N, K, POH, POW): launch 1 leaves the windows' means / extrema here
  float* part;           // [K][groups][2]: sum y, sum y*y of a workgroup's real pixels
  int ph, pw, POH, POW;
  int PS;                // row length of the accumulator tile [Cout][PS]
  int groups;            // workgroups of launch 1
  size_t lds_bytes;
};

// p.ok false: the fused launches do not reach.
inline TrainArgs train_plan(const StageDims& g) {
  TrainArgs a = {};
  ConvProdArgs p = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, g.ph);
  if (!p.ok) return a;
  // The chunk of the convolution's own plan: the two plans walk the same states until one image is left per workgroup
  // (so G is the same), then the own plan may halve its band below ph rows.  A band no higher than the own one holds
  // the own chunk as it is; a higher one is halved, in units of ph rows, until it does.
  const int CC = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1).CC;
  const int khkw = p.kh * p.kw, Mpad = 16 * p.MT;
  const long long kp = conv_round4(CC * khkw);
  const auto fits = [&] {
    return (long long)p.G * CC * ((p.R + p.kh - 1) * p.BW) + (long long)Mpad * kp + kp <= kConvLdsFloats;
  };
  while (!fits() && p.G == 1 && p.R > g.ph) {
    p.R = (p.R / g.ph + 1) / 2 * g.ph;
    p.bands = (p.OHt + p.R - 1) / p.R;
  }
  if (!fits()) return a;
  p.CC = CC;
  p.plane = (p.R + p.kh - 1) * p.BW;
  p.Kpad = (int)kp;
  p.lds_bytes = ((size_t)p.G * p.CC * p.plane + (size_t)Mpad * p.Kpad + p.Kpad) * sizeof(float);
  a.p = p;
  a.ph = g.ph; a.pw = g.pw; a.POH = g.POH; a.POW = g.POW;
  const int P = p.G * p.R * p.OWt;
  a.PS = stage_tile_row(p.Cout, P);
  a.lds_bytes = stage_lds_bytes(p.Cout, P, p.lds_bytes);
  a.groups = (int)stage_groups(p);
  return a;
}

// The measured rule (tools/bench_conv_stage_train.py, profiles/conv_stage_train_bench.txt: forced FUSED against the two
// public calls in one process, medians of seven alternating passes; "faster": the median ratio is above 1 and the two
// ranges are apart).  A class of shapes -- pooling method x what a workgroup of launch 1 holds -- is FUSED on the span
// of workgroup counts from the first to the last measured count at which every stage of the class is faster or level
// with a faster count on either side; every other count, unmeasured ones included, is the SEQUENCE.  {0, -1}: no count.
//   AVE, a band of rows (network_v4's conv0, 9 bands of 4 rows): faster at 450 workgroups (N = 50: 28.8 against 32.8 us,
//     1.14 x), level at 1800 (0.98 x), slower at 3600, 7200 and 13653 (0.94 to 0.88 x).  FUSED at 450 only: nothing
//     was measured between 450 and 1800.
//   AVE, several whole images (conv1, ten each): slower at 5, 20 and 80 workgroups (0.97 x), faster at 152 (1.02 x),
//     level at 300.  One winning count between a loss and a tie: not taken.
//   MAX, a band of rows (network_v3's first stage, network_v5's first): v3's faster at 450 (1.13 x) and 13653 (1.06 x),
//     level at 3600 (1.04 x); v5's faster at 350, 2800 and 10619 (1.20, 1.11, 1.08 x).  FUSED on 450 .. 10619, the
//     counts inside both stages' spans.
//   MAX, one whole image (v5's second stage): slower at 50, level at 400 and 1517.  Not taken.
//   MAX, several whole images (v3's second stage, v5's third): slower or level at every count measured.  Not taken.
//   AVE, one whole image: not measured.
// [MAX][stage_plan_kind]: workgroups of launch 1
constexpr StageSpan kTrainSpans[2][3] = {
    {{0, -1}, {450, 450}, {0, -1}},
    {{0, -1}, {450, 10619}, {0, -1}},
};

inline int train_route(const StageDims& g) {
  const TrainArgs a = train_plan(g);
  if (!a.p.ok) return MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE;
  return kTrainSpans[g.max][stage_plan_kind(a.p)].holds(a.groups) ? MMS_CONV_STAGE_TRAIN_ROUTE_FUSED
                                                                  : MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE;
}

// The fused forward's workspace: launch 1's partial sums.
inline size_t fused_bytes(const TrainArgs& a) { return (size_t)2 * a.p.Cout * a.groups * sizeof(float); }

constexpr unsigned kTrainFinishWindows = 1024;     // pooled elements of a launch-2 workgroup, at least: four per thread
constexpr unsigned kTrainFinishChunks = 64;        // ... unless that takes more workgroups per channel than this

// Launch 2's grid is (K, chunks): workgroup y of a channel finishes pooled elements [y wpc, (y + 1) wpc) of the
// channel's `windows` = N * PP, the last chunk what is left.
struct TrainFinishGrid {
  unsigned windows, wpc, chunks;
};
inline TrainFinishGrid train_finish_grid(int N, unsigned PP) {
  const unsigned windows = (unsigned)N * PP;
  unsigned wpc = (windows + kTrainFinishChunks - 1) / kTrainFinishChunks;
  if (wpc < kTrainFinishWindows) wpc = kTrainFinishWindows;
  return {windows, wpc, (windows + wpc - 1) / wpc};
}

}  // namespace mms
#endif  // MMS_CONV_STAGE_TRAIN_PLANS_H_
