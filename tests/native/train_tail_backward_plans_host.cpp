// tests/native/train_tail_backward_plans_host.cpp -- the host plan of the tail's fused backward, read from the C++ itself
// (csrc/train_tail_backward_plans.h).  Host code only, no HIP call: it runs where there is no GPU.  Every plan is held
// to what the kernels of csrc/train_tail_backward.hip rely on; one line per violated invariant (the first of each
// kind), exit status 1.
//
//   train_tail_backward_plans_host N C H W K kh kw F1 Hd Cd [...]
//       per shape one line:  plan ok= chunks= bottom_G= wdiff_G= slabs= ups= bytes=
//   train_tail_backward_plans_host --sweep
//       N = 0 .. 300, K and C = 1 .. 65, maps of 1 .. 16, the head's limits on either side.  Prints how many plans left
//       by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "train_tail_backward_plans.h"

using namespace mms;

namespace {

std::map<std::string, long> g_failed, g_count;

void fail(const char* inv, const char* fmt, ...) {
  if (g_failed[inv]++) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  printf("VIOLATED %s: %s\n", inv, buf);
}

#define CHECK(inv, cond, ...)            \
  do {                                   \
    if (!(cond)) fail(inv, __VA_ARGS__); \
  } while (0)

constexpr StageSpan kEveryCount[2] = {{1, 1 << 30}, {1, 1 << 30}};    // a table that routes whatever the plan reaches

void check(int N, int C, int H, int W, int K, int kh, int kw, int F1, int Hd, int Cd, int pool, int images,
           size_t head_bytes, bool print) {
  mms_score_tail_shape s = {};
  s.conv = {N, C, H, W, K, kh, kw, 1, 1, 0, 0, 1, 1, 1};
  s.ph = H - kh + 1;
  s.pw = W - kw + 1;
  s.pool = pool;
  s.F1 = F1; s.H = Hd; s.C = Cd;
  s.normalization = MMS_HEAD_NORM_VALID;
  TrainTailDims g;
  ++g_count["shapes"];
  if (train_tail_check(&s, MMS_HEAD_TRAIN, 0.5f, &g) != MMS_OK) {
    ++g_count["refused"];
    if (print) printf("plan refused\n");
    return;
  }
  const TrainTailBackwardPlan p = train_tail_backward_plan(g, images, head_bytes);
  const int fused = N > 0 ? train_tail_backward_fused(g, images, kEveryCount) : 0;
  // whatever the table, a routed shape is reached and its images are in the measured class, stated here on its own
  CHECK("route_implies_plan", !fused || (p.ok && H * W <= 128 && (H - kh + 1) * (W - kw + 1) <= 128),
        "N %d C %d K %d %dx%d", N, C, K, H, W);
  if (p.ok && !fused && N > 0) ++g_count["reached_not_routed"];
  if (print)
    printf("plan ok=%d chunks=%d bottom_G=%d wdiff_G=%d slabs=%d ups=%d bytes=%zu\n", (int)p.ok,
           p.ok ? (p.bottom.Cin + p.bottom.CC - 1) / p.bottom.CC : 0, p.bottom.G, p.wdiff.G, p.wdiff.slabs, p.wdiff.ups,
           p.ok ? p.bytes : (size_t)0);
  if (!p.ok) {
    ++g_count["not_reached"];
    const bool head_past = K + F1 > kHeadFastFeatures || Hd > kHeadFastHidden || Cd > kHeadFastClasses;
    if (N == 0 || N > kTrainTailBackwardMaxN) ++g_count["past_n"];
    else if (head_past) ++g_count["past_head"];
    else if (C > kConvMaxChannels || K > kConvMaxChannels) ++g_count["past_channels"];
    else ++g_count["past_image"];
    return;
  }
  ++g_count["reached"];
  CHECK("reach", N >= 1 && N <= kTrainTailBackwardMaxN && C <= kConvMaxChannels && K <= kConvMaxChannels &&
                     K + F1 <= kHeadFastFeatures && Hd <= kHeadFastHidden && Cd <= kHeadFastClasses,
        "N %d C %d K %d F1 %d Hd %d Cd %d", N, C, K, F1, Hd, Cd);
  CHECK("lds", p.bottom_lds <= 163840 && p.wdiff_lds <= 163840 && p.head_lds <= 163840, "%zu %zu %zu", p.bottom_lds,
        p.wdiff_lds, p.head_lds);
  const ConvProdArgs& b = p.bottom;
  const ConvWdiffArgs& w = p.wdiff;
  CHECK("whole_images", b.bands == 1 && w.bands == 1 && b.R == H && w.R == g.d.OH && b.G >= 1 && b.G <= images &&
                            w.G >= 1 && w.G <= images,
        "bands %d %d G %d %d", b.bands, w.bands, b.G, w.G);
  CHECK("tile_pixels", b.G * H * W <= kConvTilePixels && w.G * g.d.OH * g.d.OW <= kConvTilePixels, "G %d %d", b.G, w.G);
  CHECK("bottom_lds_formula",
        b.lds_bytes == ((size_t)b.G * b.CC * b.plane + (size_t)16 * b.MT * b.Kpad + b.Kpad) * sizeof(float) &&
            b.CC >= 1 && b.CC <= K && b.Cin == K && b.Cout == C,
        "CC %d", b.CC);
  CHECK("wdiff_lds_formula",
        w.PP == conv_round4(w.G * w.R * g.d.OW) + 1 &&
            w.lds_bytes == ((size_t)w.G * C * w.plane + (size_t)16 * w.MT * w.PP + w.PP) * sizeof(float),
        "PP %d", w.PP);
  // the slabs cover every (n, oy) once: unit u holds images [u G, u G + G), all rows; slab s units [s ups, s ups + ups)
  std::vector<int> seen(N, 0);
  CHECK("slabs", w.slabs >= 1 && w.slabs <= kConvMaxSlabs && w.ups >= 1 && w.units == (N + w.G - 1) / w.G &&
                     (long long)w.slabs * w.ups >= w.units && (long long)(w.slabs - 1) * w.ups < w.units,
        "units %d ups %d slabs %d", w.units, w.ups, w.slabs);
  for (int sl = 0; sl < w.slabs; ++sl)
    for (int u = sl * w.ups; u < w.units && u < (sl + 1) * w.ups; ++u)
      for (int n = u * w.G; n < N && n < (u + 1) * w.G; ++n) ++seen[n];
  for (int n = 0; n < N; ++n) CHECK("cover_once", seen[n] == 1, "N %d image %d seen %d", N, n, seen[n]);
  if (w.slabs > 1) ++g_count["several_slabs"];
  if (w.ups > 1) ++g_count["long_slabs"];
  if (b.CC < K) ++g_count["chunked"];
  // the workspace: parts in order, disjoint, 16-byte aligned, inside the total
  const size_t NK = (size_t)N * K, nW = (size_t)K * C * kh * kw;
  CHECK("workspace",
        p.off_x0d == 0 && p.off_x0d % 16 == 0 && p.off_head % 16 == 0 && p.off_coef % 16 == 0 && p.off_part % 16 == 0 &&
            p.bytes % 16 == 0 && p.off_head >= p.off_x0d + NK * 4 && p.off_coef >= p.off_head + head_bytes &&
            p.off_part >= p.off_coef + (2 * (size_t)K + NK) * 4 + NK * 4 && p.coef_floats == 2 * (size_t)K + NK &&
            p.bytes >= p.off_part + (size_t)w.slabs * (nW + K) * 4,
        "offsets %zu %zu %zu %zu of %zu", p.off_x0d, p.off_head, p.off_coef, p.off_part, p.bytes);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) {
    const int maps[] = {1, 2, 3, 5, 6, 8, 11, 12, 13, 16};
    const int chans[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65};
    for (int N = 0; N <= 300; N += (N < 4 || (N >= 60 && N < 70) || N >= 250) ? 1 : 7)
      for (int K : chans)
        for (int C : chans)
          for (int m : maps)
            for (int k = 1; k <= 5 && k <= m; k += 2)
              check(N, C, m, m, K, k, k, (N + K) % 5, 32, 2, (N + m) & 1, 1 + (K + m) % 3, (size_t)(N * 12 + 1), false);
    for (int N = 0; N <= 300; ++N)
      for (int images = 1; images <= 10; images += 3) check(N, 32, 9, 9, 64, 5, 5, 4, 32, 2, N & 1, images, 777, false);
    for (int K = 1; K <= 65; ++K)
      for (int C = 1; C <= 65; ++C) check(50, C, 8, 8, K, 3, 3, 2, 32, 2, K & 1, 1, 0, false);
    for (int F1 : {0, 63, 64, 65})
      for (int Hd : {1, 63, 64, 65})
        for (int Cd : {1, 15, 16, 17}) check(50, 32, 9, 9, 64, 5, 5, F1, Hd, Cd, 0, 1, 16, false);
    for (const auto& c : g_count) printf("count %s=%ld\n", c.first.c_str(), c.second);
  } else if (argc > 1 && (argc - 1) % 10 == 0) {
    for (int i = 1; i + 9 < argc; i += 10) {
      int v[10];
      for (int j = 0; j < 10; ++j) v[j] = atoi(argv[i + j]);
      check(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], 0, 1, 0, true);
    }
  } else {
    fprintf(stderr, "usage: %s --sweep | N C H W K kh kw F1 Hd Cd [...]\n", argv[0]);
    return 2;
  }
  if (!g_failed.empty()) return 1;
  printf("every plan holds its invariants\n");
  return 0;
}
