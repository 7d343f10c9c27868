// csrc/train_tail_backward_plans.h -- the host-side plan of the TRAIN-phase tail's fused backward
// (include/mms_train_tail_backward.h, csrc/train_tail_backward.hip), in a header so that a host program can read it
// (tests/native/train_tail_backward_plans_host.cpp sweeps it and asserts what the kernels rely on): whether the fused
// launches reach a shape, the two convolution plans cut to the tail's images per workgroup, every launch's LDS and the
// parts of the workspace.  Host text only; it needs no device code.
#ifndef MMS_TRAIN_TAIL_BACKWARD_PLANS_H_
#define MMS_TRAIN_TAIL_BACKWARD_PLANS_H_

#include "conv_plans.h"
#include "train_tail_check.h"

namespace mms {

constexpr int kTrainTailBackwardMaxLdsBytes = 163840;   // a launch's LDS, at most: the CU's 160 KB
constexpr int kTrainTailBackwardMaxN = 256;             // the coefficients' chain over n, at most

struct TrainTailBackwardPlan {
  ConvProdArgs bottom;       // conv_prod_plan(d, bottom_diff, 1) with G cut to the tail's images
  ConvWdiffArgs wdiff;       // conv_wdiff_plan(d) with G cut likewise; units, ups and slabs follow
  HeadFastPlan hp;
  int N, K;
  // The workspace, bytes from its start; every part starts at a multiple of 16:
  //   [x0_diff] N K floats: the head's gradient w.r.t. flt
  //   [head]    the head call's own workspace
  //   [coef]    A0 (K), B (K), cg (N K) floats, then pos (N K) ints
  //   [part]    slabs x (K C kh kw + K) floats: the parameter diffs' partial sums
  size_t off_x0d, off_head, off_coef, off_part, bytes;
  size_t coef_floats;        // 2 K + N K: pos starts behind them
  size_t bottom_lds, wdiff_lds, head_lds;
  bool ok;                   // false: the fused launches do not reach this shape
};

// head_bytes: mms_head_workspace_bytes of the tail's head.
inline TrainTailBackwardPlan train_tail_backward_plan(const TrainTailDims& g, int images, size_t head_bytes) {
  TrainTailBackwardPlan p = {};
  const ConvDims& d = g.d;
  p.N = d.N;
  p.K = d.K;
  if (d.N < 1 || d.N > kTrainTailBackwardMaxN || images < 1) return p;
  p.hp = head_fast_plan(g.hd);
  if (!p.hp.ok) return p;
  p.bottom = conv_prod_plan(d, MMS_CONV_PASS_BOTTOM_DIFF, 1);
  p.wdiff = conv_wdiff_plan(d);
  // workgroups hold whole images: neither launch cuts an image into bands of rows
  if (!p.bottom.ok || !p.wdiff.ok || p.bottom.bands != 1 || p.wdiff.bands != 1) return p;
  ConvProdArgs& b = p.bottom;
  if (b.G > images) b.G = images;
  b.lds_bytes = ((size_t)b.G * b.CC * b.plane + (size_t)16 * b.MT * b.Kpad + b.Kpad) * sizeof(float);
  ConvWdiffArgs& w = p.wdiff;
  if (w.G > images) w.G = images;
  w.PP = conv_round4(w.G * w.R * d.OW) + 1;
  w.lds_bytes = ((size_t)w.G * d.C * w.plane + (size_t)16 * w.MT * w.PP + w.PP) * sizeof(float);
  w.units = (d.N + w.G - 1) / w.G;
  const int want = w.units < kConvMaxSlabs ? w.units : kConvMaxSlabs;
  w.ups = (w.units + want - 1) / want;
  w.slabs = (w.units + w.ups - 1) / w.ups;
  p.bottom_lds = b.lds_bytes;
  p.wdiff_lds = w.lds_bytes;
  p.head_lds = p.hp.bwd_lds;
  const size_t NK = (size_t)d.N * d.K, nW = (size_t)d.K * d.C * d.kh * d.kw;
  p.coef_floats = 2 * (size_t)d.K + NK;
  p.off_x0d = 0;
  p.off_head = p.off_x0d + round_up(NK * sizeof(float), 16);
  p.off_coef = p.off_head + round_up(head_bytes, 16);
  p.off_part = p.off_coef + round_up(p.coef_floats * sizeof(float) + NK * sizeof(int), 16);
  p.bytes = p.off_part + round_up((size_t)w.slabs * (nW + d.K) * sizeof(float), 16);
  p.ok = p.bottom_lds <= (size_t)kTrainTailBackwardMaxLdsBytes && p.wdiff_lds <= (size_t)kTrainTailBackwardMaxLdsBytes &&
         p.head_lds <= (size_t)kTrainTailBackwardMaxLdsBytes;
  return p;
}

// workgroups of the bottom_diff launch: what the measured routing rule is stated in
inline int train_tail_backward_groups(const TrainTailBackwardPlan& p) { return (p.N + p.bottom.G - 1) / p.bottom.G; }

// The measured class: an image of at most kConvTilePixels / 2 pixels in both convolution launches (the input map in
// bottom_diff, the output map in the parameter diffs), as every tail of the driver has.  The plan also reaches images
// of 129 to 256 pixels whose rows fit one workgroup; no measurement covers them.
inline bool train_tail_backward_small_images(const ConvDims& d) {
  return d.H * d.W <= kConvTilePixels / 2 && d.OH * d.OW <= kConvTilePixels / 2;
}

// The one routing decision, for a shape train_tail_check accepts: FUSED where the plan reaches the shape, its images
// are in the measured class (train_tail_backward_small_images) and the bottom_diff launch's workgroup count lies in the
// measured span of the pooling method (spans[MAX]; csrc/train_tail_backward.hip holds the table and names each
// threshold); every other count, unmeasured ones included, and every larger image is the SEQUENCE.  Returns 1 for
// FUSED, 0 else.
inline int train_tail_backward_fused(const TrainTailDims& g, int images, const StageSpan (&spans)[2]) {
  const TrainTailBackwardPlan p = train_tail_backward_plan(g, images, 0);
  if (!p.ok || !train_tail_backward_small_images(g.d)) return 0;
  return spans[g.max].holds(train_tail_backward_groups(p)) ? 1 : 0;
}

}  // namespace mms
#endif  // MMS_TRAIN_TAIL_BACKWARD_PLANS_H_
