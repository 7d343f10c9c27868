// tests/native/conv_stage_plans_host.cpp -- what the pooled conv stages launch at a shape and window, read from the
// C++ itself: stage_plan and stage_route<MAX> (csrc/conv_stage_plans.h), stage_tile_row, stage_lds_bytes,
// stage_plan_kind and stage_pool_dispatch (csrc/conv_pool_tile.h), and train_plan / train_route
// (csrc/conv_stage_train_plans.h).  Host code only, no HIP call: it runs where there is no GPU.  Every plan it computes is
// held to what the pooling epilogue relies on (check_tile below); one line per violated invariant (the first of each
// kind), exit status 1.
//
//   conv_stage_plans_host N C H W K kh kw ph pw [N C H W K kh kw ph pw ...]
//       stride 1, pad 0, group 1; the window tiles the map.  Per shape (key=value):
//         shape    N C H W K kh kw ph pw OH OW
//         plan     ok kind G R bands last_rows MT CC chunks last_chunk P PS fallback lds_bytes geo_R own_R own_CC
//                  ragged groups last_images
//                  kind: 0 several whole images per workgroup, 1 a band of rows, 2 one whole image; chunks: of input
//                  channels, the last of last_chunk; fallback: the tile's row is P because the padded row does not fit;
//                  geo_R: the band of conv_tile_geometry, before the LDS loop; own_R, own_CC: of the convolution's own
//                  plan (rq = 1); ragged: K is no multiple of 16
//         window   ave max          the window stage_pool_dispatch compiles in: its height, 0 for a run-time window
//         route    ave max          stage_route: 1 the sequence, 2 fused
//         train    ok kind G R bands MT CC chunks last_chunk P PS fallback lds_bytes groups ave max
//                  train_plan's figures, and train_route per method: 0 the sequence, 1 fused
//   conv_stage_plans_host --sweep
//       the shapes of conv_plans_host's sweep -- N in {1, 3}, C and K in {1, 4, 17, 33, 64}, H and W in {3, 9, 14, 40,
//       130, 258}, kernels 1 x 1 .. 11 x 11, 3 x 1 and 1 x 9 where they fit -- times the windows ph, pw in 1 .. 6 that
//       divide the map.  Prints how many plans left by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "conv_stage_plans.h"
#include "conv_stage_train_plans.h"

using namespace mms;

namespace {

std::map<std::string, long> g_failed;      // invariant -> times violated

void fail(const char* inv, const StageDims& g, const char* fmt, ...) {
  if (g_failed[inv]++) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  const ConvDims& d = g.d;
  printf("VIOLATED %s: ST(%d, %d, %d, %d, %d, %d, %d, (%d, %d)): %s\n", inv, d.N, d.C, d.H, d.W, d.K, d.kh, d.kw, g.ph, g.pw, buf);
}

#define CHECK(inv, cond, ...) \
  do {                        \
    if (!(cond)) fail(inv, g, __VA_ARGS__); \
  } while (0)

// the row length stage_tile_row tries first: the next one that is 4 or 12 mod 16
int padded_row(int P) {
  int PS = P;
  while (PS % 16 != 4 && PS % 16 != 12) ++PS;
  return PS;
}

// What stage_tile_store and the window walk of both phases rely on: `what` names the phase in a violation's line.
void check_tile(const char* what, const StageDims& g, const ConvProdArgs& p, int PS, size_t lds_bytes) {
  const int P = p.G * p.R * p.OWt;
  CHECK("tile", p.G >= 1 && p.R >= 1 && P <= kConvTilePixels, "%s: G %d R %d OWt %d", what, p.G, p.R, p.OWt);
  CHECK("lds", (size_t)p.Cout * PS * sizeof(float) <= lds_bytes && lds_bytes >= p.lds_bytes &&
                   lds_bytes <= sizeof(float) * (size_t)kConvLdsFloats,
        "%s: Cout %d PS %d lds_bytes %zu, the product's %zu", what, p.Cout, PS, lds_bytes, p.lds_bytes);
  const bool too_long = (long long)p.Cout * padded_row(P) > kConvLdsFloats;
  CHECK("row", PS == (too_long ? P : padded_row(P)) && PS >= P, "%s: PS %d, P %d, the padded row %d", what, PS, P, padded_row(P));
  // whole windows: every band starts at a window row and is whole window rows, the last one included
  bool whole = p.R % g.ph == 0 && p.OWt % g.pw == 0 && (p.G == 1 || (p.bands == 1 && p.R == p.OHt));
  for (int b = 0; b < p.bands; ++b) {
    const int oy0 = b * p.R;
    whole = whole && oy0 < p.OHt && oy0 % g.ph == 0 && (p.OHt - oy0) % g.ph == 0;
  }
  CHECK("windows", whole, "%s: R %d, bands %d, OHt %d, window %d x %d, G %d", what, p.R, p.bands, p.OHt, g.ph, g.pw, p.G);
  CHECK("bands", (long long)p.bands * p.R >= p.OHt && p.OHt > (long long)(p.bands - 1) * p.R, "%s: bands %d R %d OHt %d", what,
        p.bands, p.R, p.OHt);
  CHECK("channels", (p.MT == 1 || p.MT == 2 || p.MT == 4) && p.Cout <= 16 * p.MT && (p.MT == 1 || p.Cout > 8 * p.MT),
        "%s: MT %d Cout %d", what, p.MT, p.Cout);
  CHECK("chunk", p.CC >= 1 && p.CC <= p.Cin && p.Kpad == conv_round4(p.CC * p.kh * p.kw), "%s: CC %d Kpad %d", what, p.CC, p.Kpad);
}

bool dims(int N, int C, int H, int W, int K, int kh, int kw, int ph, int pw, StageDims* g) {
  const mms_conv_shape s = {N, C, H, W, K, kh, kw, 1, 1, 0, 0, 1, 1, 1};
  if (stage_window_check(&s, ph, pw, g) != MMS_OK) return false;
  g->max = false;
  return true;
}

template <bool MAX>
int window_form(int ph, int pw) {
  int form = -1;
  stage_pool_dispatch<MAX>(ph, pw, [&](auto PH, auto PW) {
    static_assert(decltype(PH)::value == decltype(PW)::value, "the compiled windows are square");
    form = decltype(PH)::value;
  });
  return form;
}

struct Figures {
  int ok, kind, chunks, last_chunk, P, fallback;
};
Figures figures(const ConvProdArgs& p, int PS) {
  Figures f = {};
  if (!p.ok) return f;
  f.ok = 1;
  f.kind = (int)stage_plan_kind(p);
  f.chunks = (p.Cin + p.CC - 1) / p.CC;
  f.last_chunk = p.Cin - (f.chunks - 1) * p.CC;
  f.P = p.G * p.R * p.OWt;
  f.fallback = PS == f.P && padded_row(f.P) != f.P;
  return f;
}

void print_shape(StageDims g) {
  const ConvDims& d = g.d;
  printf("shape N=%d C=%d H=%d W=%d K=%d kh=%d kw=%d ph=%d pw=%d OH=%d OW=%d\n", d.N, d.C, d.H, d.W, d.K, d.kh, d.kw, g.ph, g.pw, d.OH,
         d.OW);
  const StageArgs a = stage_plan(g);
  const ConvProdArgs& p = a.p;
  if (p.ok) check_tile("TEST", g, p, a.PS, a.lds_bytes);
  const Figures f = figures(p, a.PS);
  const ConvProdArgs own = conv_prod_plan(d, MMS_CONV_PASS_FORWARD, 1);
  int gG = 0, gR = 0, gB = 0;
  if (!conv_tile_geometry(d.OH, d.OW, g.ph, &gG, &gR, &gB)) gR = 0;
  printf("plan ok=%d kind=%d G=%d R=%d bands=%d last_rows=%d MT=%d CC=%d chunks=%d last_chunk=%d P=%d PS=%d fallback=%d lds_bytes=%zu "
         "geo_R=%d own_R=%d own_CC=%d ragged=%d groups=%lld last_images=%d\n",
         f.ok, f.kind, p.G, p.R, p.bands, f.ok ? p.OHt - (p.bands - 1) * p.R : 0, p.MT, p.CC, f.chunks, f.last_chunk, f.P, a.PS, f.fallback,
         a.lds_bytes, gR, own.R, own.CC, d.K % 16 != 0, f.ok ? stage_groups(p) : 0LL, f.ok ? d.N - (d.N - 1) / p.G * p.G : 0);
  printf("window ave=%d max=%d\n", window_form<false>(g.ph, g.pw), window_form<true>(g.ph, g.pw));
  g.max = false;
  const int ra = stage_route<false>(g);
  g.max = true;
  const int rm = stage_route<true>(g);
  printf("route ave=%d max=%d\n", ra, rm);
  g.max = false;
  const TrainArgs t = train_plan(g);
  if (t.p.ok) check_tile("TRAIN", g, t.p, t.PS, t.lds_bytes);
  const Figures tf = figures(t.p, t.PS);
  int tr[2];
  for (int m = 0; m < 2; ++m) {
    g.max = m != 0;
    tr[m] = train_route(g);
  }
  printf("train ok=%d kind=%d G=%d R=%d bands=%d MT=%d CC=%d chunks=%d last_chunk=%d P=%d PS=%d fallback=%d lds_bytes=%zu groups=%d "
         "ave=%d max=%d\n",
         tf.ok, tf.kind, t.p.G, t.p.R, t.p.bands, t.p.MT, t.p.CC, tf.chunks, tf.last_chunk, tf.P, t.PS, tf.fallback, t.lds_bytes, t.groups,
         tr[0], tr[1]);
}

void sweep() {
  static const int kN[] = {1, 3}, kCh[] = {1, 4, 17, 33, 64}, kHW[] = {3, 9, 14, 40, 130, 258};
  static const int kKernel[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 5}, {6, 6}, {7, 7}, {8, 8}, {9, 9}, {10, 10}, {11, 11},
                                   {3, 1}, {1, 9}};
  static const char* const kKind[] = {"images", "row_band", "one_image"};
  std::map<std::string, long> n;
  for (int N : kN) for (int C : kCh) for (int K : kCh) for (int H : kHW) for (int W : kHW) for (const auto& k : kKernel) {
    if (k[0] > H || k[1] > W) continue;
    ++n["shapes"];
    for (int ph = 1; ph <= 6; ++ph) for (int pw = 1; pw <= 6; ++pw) {
      StageDims g;
      if (!dims(N, C, H, W, K, k[0], k[1], ph, pw, &g)) continue;
      ++n["plans"];
      const StageArgs a = stage_plan(g);
      const TrainArgs t = train_plan(g);
      if (t.p.ok) {
        check_tile("TRAIN", g, t.p, t.PS, t.lds_bytes);
        ++n["train_ok"];
        if (figures(t.p, t.PS).fallback) ++n["train_fallback"];
      }
      if (!a.p.ok) { ++n["refused"]; continue; }
      check_tile("TEST", g, a.p, a.PS, a.lds_bytes);
      const Figures f = figures(a.p, a.PS);
      ++n["ok"];
      ++n[std::string("kind_") + kKind[f.kind]];
      ++n["mt_" + std::to_string(a.p.MT)];
      if (f.fallback) ++n[std::string("fallback_") + kKind[f.kind]];
      if (a.PS > f.P) ++n["tile_row_padded"];
      if (K % 16) ++n["ragged_mt_" + std::to_string(a.p.MT)];
      if (f.chunks > 1) ++n["several_chunks"];
      int gG, gR, gB;
      if (conv_tile_geometry(g.d.OH, g.d.OW, ph, &gG, &gR, &gB) && gG == 1 && a.p.R < gR && ph > 1) ++n["band_halved_in_units_of_ph"];
      if (a.p.OHt % a.p.R) ++n["ragged_last_band"];
      ++n["ave_window_" + std::to_string(window_form<false>(ph, pw)) + "_" + kKind[f.kind]];
      ++n["max_window_" + std::to_string(window_form<true>(ph, pw)) + "_" + kKind[f.kind]];
      if (stage_route<false>(g) == MMS_CONV_STAGE_ROUTE_FUSED) ++n["fused_ave"];
      g.max = true;
      if (stage_route<true>(g) == MMS_CONV_STAGE_ROUTE_FUSED) ++n["fused_max"];
    }
  }
  for (const auto& kv : n) printf("sweep %s=%ld\n", kv.first.c_str(), kv.second);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) {
    sweep();
  } else if (argc >= 10 && (argc - 1) % 9 == 0) {
    for (int i = 1; i < argc; i += 9) {
      int v[9];
      for (int k = 0; k < 9; ++k) v[k] = atoi(argv[i + k]);
      StageDims g;
      if (!dims(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], &g)) {
        fprintf(stderr, "%s: the shape or window check refuses argument %d onwards\n", argv[0], i);
        return 2;
      }
      print_shape(g);
    }
  } else {
    fprintf(stderr, "usage: %s --sweep | N C H W K kh kw ph pw [N C H W K kh kw ph pw ...]\n", argv[0]);
    return 2;
  }
  long bad = 0;
  for (const auto& kv : g_failed) {
    printf("invariant %s violated %ld time(s)\n", kv.first.c_str(), kv.second);
    bad += kv.second;
  }
  if (!bad) printf("conv_stage_plans_host ok: every plan holds its invariants\n");
  return bad ? 1 : 0;
}
