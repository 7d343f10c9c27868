// csrc/conv_stage_plans.h -- the host-side plans of csrc/conv_stage.hip's FUSED launch, in a header so that a host
// program can read them (tests/native/conv_stage_plans_host.cpp prints every plan and asserts what the pooling epilogue
// relies on): the launch's arguments and plan (StageArgs, stage_plan), whether the window made the band lower
// (stage_band_shrunk) and the two families' measured routing rules (stage_route<MAX> and their constants).  Host text
// only; the kernels are csrc/conv_stage.hip's.
#ifndef MMS_CONV_STAGE_PLANS_H_
#define MMS_CONV_STAGE_PLANS_H_

#include "conv_pool_tile.h"
#include "mms_conv_maxpool_stage.h"
#include "mms_conv_stage.h"

namespace mms {

// One set of route values for both families: the code below names MMS_CONV_STAGE_ROUTE_* only.
static_assert(MMS_CONV_MAXPOOL_STAGE_ROUTE_NONE == MMS_CONV_STAGE_ROUTE_NONE &&
                  MMS_CONV_MAXPOOL_STAGE_ROUTE_SEQUENCE == MMS_CONV_STAGE_ROUTE_SEQUENCE &&
                  MMS_CONV_MAXPOOL_STAGE_ROUTE_FUSED == MMS_CONV_STAGE_ROUTE_FUSED,
              "the MAX stage's routes carry the AVE stage's values");

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
inline StageArgs stage_plan(const StageDims& g) {
  StageArgs a = {};
  a.p = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, g.ph);
  if (!a.p.ok) return a;
  a.ph = g.ph; a.pw = g.pw; a.POH = g.POH; a.POW = g.POW;
  const int P = a.p.G * a.p.R * a.p.OWt;
  a.PS = stage_tile_row(a.p.Cout, P);
  a.lds_bytes = stage_lds_bytes(a.p.Cout, P, a.p.lds_bytes);
  return a;
}

// whether the window made the band lower than the convolution's own
inline bool stage_band_shrunk(const StageDims& g, const StageArgs& a) {
  return a.p.R < conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1).R;
}

// The one routing decision of a family, for a shape and window stage_check accepts.
template <bool MAX>
int stage_route(const StageDims& g);

// AVE.  The measured rules (tools/bench_conv_stage.py, profiles/conv_stage_bench.txt: fused against sequence at
// network_v4's two stages over a range of N; `groups` is the launch's workgroups).
//   Whole images per workgroup (conv1, ten each): slower at 5 workgroups (189.7 against 180.7 us), faster at 10, 20, 40,
//   80 and 152 (1.03 to 1.09 x).  Few workgroups are latency-bound and the epilogue is on each one's critical path.
//   Fused from the smallest count measured to win.
constexpr long long kStageMinImageGroups = 10;
//   A band the pooling window made lower than the convolution's own (conv0: 4 rows for 6): faster at 450 and 1800
//   workgroups (1.42 x, 1.05 x), level at 4095 (0.98 x, ranges overlapping), slower at 6300, 9000 and 13653 (0.96 to
//   0.97 x).  Why is not measured: supposedly the nine pixel tiles over four waves (3, 2, 2, 2) and 8 staged rows per 4
//   computed against 10 per 6.  Fused up to a count between the last win and the tie.
constexpr long long kStageMaxShrunkBandGroups = 2048;

template <>
inline int stage_route<false>(const StageDims& g) {
  const StageArgs a = stage_plan(g);
  if (!a.p.ok) return MMS_CONV_STAGE_ROUTE_SEQUENCE;
  const long long groups = stage_groups(a.p);
  if (stage_plan_kind(a.p) == kStageImages)
    return groups >= kStageMinImageGroups ? MMS_CONV_STAGE_ROUTE_FUSED : MMS_CONV_STAGE_ROUTE_SEQUENCE;
  if (stage_band_shrunk(g, a) && groups > kStageMaxShrunkBandGroups) return MMS_CONV_STAGE_ROUTE_SEQUENCE;
  return MMS_CONV_STAGE_ROUTE_FUSED;
}

// MAX.  Measured (tools/bench_conv_maxpool_stage.py, profiles/conv_maxpool_stage_bench.txt): network_v3's and
// network_v5's five stages, N from 6 to 3000, fused against sequence; "faster" is a median ratio above 1 with the two
// ranges of seven passes apart, "level" is ranges that touch.  The rule: three kinds of plan, told apart by what a
// workgroup holds.  Each stage of a kind gives a span of workgroup counts: from the first measured count at which fused
// is faster and from which on it is never slower, to the last count measured.  The kind is FUSED on the counts that
// lie in the span of every one of its stages, and the SEQUENCE on everything else, unmeasured counts included.  A level
// point inside a span stays with it: a rule keyed on the count cannot carve it out from the faster points around it.
//   Several whole images (v3's second stage, ten each; v5's third, seven each).  v3's: slower at 5, 10, 20 and 40
//   workgroups (0.98 to 1.00 x), faster at 60, 80, 152 and 300 (1.01 to 1.03 x): 60 .. 300.  v5's: faster at all of
//   8 to 429 (1.04 to 1.12 x).  So v5's third stage is left on the sequence below 60 workgroups and above 300.
//   A band of rows of one image (v3's first stage, 4 rows where the convolution takes 6; v5's first, 6 rows).  v3's:
//   faster at 54, 450, 675, 900, 9900, 13653 and 18000 (1.06 to 1.50 x), level at 225, 1800, 3600 and 7200 (medians
//   1.42, 1.01, 1.03, 1.02 x): 54 .. 18000.  v5's: faster at all of 49 to 14000 (1.08 to 1.39 x) but 56, level for one
//   slow pass of each route (1.34 x).  A band the window made lower pays here (AVE's does not beyond 2048 workgroups).
//   One whole image (v5's second stage, 16 x 16).  Slower at 6 workgroups, level at 25, faster at 50 (1.01 x) and at
//   all of 100 to 2000 (1.03 to 1.06 x): 50 .. 2000.
constexpr StageSpan kMaxStageSpans[3] = {{60, 300}, {54, 14000}, {50, 2000}};      // by stage_plan_kind

template <>
inline int stage_route<true>(const StageDims& g) {
  const StageArgs a = stage_plan(g);
  if (!a.p.ok) return MMS_CONV_STAGE_ROUTE_SEQUENCE;
  return kMaxStageSpans[stage_plan_kind(a.p)].holds(stage_groups(a.p)) ? MMS_CONV_STAGE_ROUTE_FUSED
                                                                       : MMS_CONV_STAGE_ROUTE_SEQUENCE;
}

}  // namespace mms
#endif  // MMS_CONV_STAGE_PLANS_H_
