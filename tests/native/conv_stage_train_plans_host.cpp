// tests/native/conv_stage_train_plans_host.cpp -- the launch plans of the TRAIN stage's FUSED forward, read from the
// C++ itself: train_plan, train_route, fused_bytes and train_finish_grid (csrc/conv_stage_train_plans.h).  Host code
// only, no HIP call: it runs where there is no GPU.  Every plan it computes is held to what the two launches rely on
// (check_plan, check_finish below); one line per violated invariant (the first of each kind), exit status 1.
//
//   conv_stage_train_plans_host N C H W K kh kw ph pw [N C H W K kh kw ph pw ...]
//       stride 1, pad 0, group 1; the window tiles the map.  Per shape (key=value):
//         shape    N C H W K kh kw ph pw OH OW PP
//         plan     ok kind G R bands last_rows CC MT PS groups last_images partial_bytes lds_bytes
//                  kind: 0 several whole images per workgroup, 1 a band of rows, 2 one whole image;
//                  last_rows: rows of an image's last band; last_images: images of the last image group
//         finish   windows wpc chunks last        launch 2: pooled elements per channel, per chunk, chunks, in the last
//         route    ave max                         train_route: 0 the sequence, 1 fused
//   conv_stage_train_plans_host --sweep
//       the shapes of conv_plans_host's sweep -- N in {1, 3}, C and K in {1, 4, 17, 33, 64}, H and W in {3, 9, 14, 40,
//       130, 258}, kernels 1 x 1 .. 11 x 11, 3 x 1 and 1 x 9 where they fit -- times the windows ph, pw in 1 .. 6 that
//       divide the map; then launch 2's grid alone over batches up to 70 000 images of 1 .. 1296 pooled elements.
//       Prints how many plans left by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

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

// What train_product_kernel<MT, ...>, its launch and the partial sums' slots rely on.
void check_plan(const StageDims& g, const TrainArgs& a) {
  if (!a.p.ok) return;
  const ConvProdArgs& p = a.p;
  const ConvDims& d = g.d;
  const long long khkw = (long long)d.kh * d.kw, Mpad = 16LL * p.MT, P = (long long)p.G * p.R * p.OWt;
  CHECK("partials", fused_bytes(a) == (size_t)2 * d.K * a.groups * 4, "partial bytes %zu, K %d, groups %d", fused_bytes(a), d.K,
        a.groups);
  // wg = blockIdx.x * gridDim.y + blockIdx.y of the grid (image groups, bands): every slot of a channel, each once
  const long long gx = (d.N + p.G - 1) / p.G, gy = p.bands;
  CHECK("partials", a.groups == gx * gy && (gx - 1) * gy + (gy - 1) == a.groups - 1, "groups %d, grid %lld x %lld", a.groups, gx, gy);
  CHECK("chunk", p.CC == conv_prod_plan(d, MMS_CONV_PASS_FORWARD, 1).CC && p.CC >= 1 && p.CC <= p.Cin, "CC %d, the convolution's %d",
        p.CC, conv_prod_plan(d, MMS_CONV_PASS_FORWARD, 1).CC);
  CHECK("chunk", p.Kpad == conv_round4((int)(p.CC * khkw)), "Kpad %d CC %d", p.Kpad, p.CC);
  CHECK("lds", p.lds_bytes == 4 * ((size_t)p.G * p.CC * p.plane + (size_t)(Mpad * p.Kpad) + p.Kpad) &&
                   p.lds_bytes <= sizeof(float) * (size_t)kConvLdsFloats,
        "the product's lds_bytes %zu", p.lds_bytes);
  CHECK("lds", a.lds_bytes >= p.lds_bytes && a.lds_bytes >= (size_t)p.Cout * a.PS * 4 && a.PS >= P &&
                   a.lds_bytes <= sizeof(float) * (size_t)kConvLdsFloats,
        "lds_bytes %zu, PS %d, P %lld", a.lds_bytes, a.PS, P);
  CHECK("tile", p.G >= 1 && p.R >= 1 && P <= kConvTilePixels, "G %d R %d OWt %d", p.G, p.R, p.OWt);
  CHECK("band", p.BW == p.IW && p.plane == (p.R + p.kh - 1) * p.BW, "BW %d plane %d", p.BW, p.plane);
  // whole windows: every band, the last one included, is whole window rows; several images only as whole images
  CHECK("windows", p.R % g.ph == 0 && p.OHt % g.ph == 0 && p.OWt % g.pw == 0 && (p.G == 1 || (p.bands == 1 && p.R == p.OHt)),
        "R %d, window %d x %d, G %d, bands %d", p.R, g.ph, g.pw, p.G, p.bands);
  CHECK("bands", (long long)p.bands * p.R >= p.OHt && p.OHt > (long long)(p.bands - 1) * p.R, "bands %d R %d OHt %d", p.bands, p.R,
        p.OHt);
  CHECK("channels", (p.MT == 1 || p.MT == 2 || p.MT == 4) && p.Cout <= 16 * p.MT && (p.MT == 1 || p.Cout > 8 * p.MT), "MT %d Cout %d",
        p.MT, p.Cout);
  CHECK("windows", a.ph == g.ph && a.pw == g.pw && a.POH * g.ph == d.OH && a.POW * g.pw == d.OW, "POH %d POW %d", a.POH, a.POW);
}

// What train_finish_kernel and its launch rely on.  The kernel's own arithmetic, restated: workgroup y finishes
// [w0, w1) with w0 = y wpc, w1 = windows - w0 < wpc ? windows : w0 + wpc.
void check_finish(const StageDims& g, const TrainFinishGrid& f) {
  CHECK("finish", f.windows == (unsigned)g.d.N * (unsigned)(g.POH * g.POW), "windows %u", f.windows);
  if (!f.windows) return;
  CHECK("finish", f.chunks >= 1 && (f.chunks <= kTrainFinishChunks || f.wpc == kTrainFinishWindows) && f.wpc >= kTrainFinishWindows,
        "chunks %u wpc %u", f.chunks, f.wpc);
  CHECK("finish", f.chunks <= 65535, "chunks %u are a grid's y", f.chunks);
  unsigned long long next = 0;
  bool once = true;
  for (unsigned y = 0; y < f.chunks; ++y) {
    const unsigned w0 = y * f.wpc, w1 = f.windows - w0 < f.wpc ? f.windows : w0 + f.wpc;
    once = once && (unsigned long long)y * f.wpc == next && w0 < f.windows && w1 > w0 && w1 <= f.windows;
    next = w1;
  }
  CHECK("finish", once && next == f.windows, "%u chunks of %u do not cover %u windows once", f.chunks, f.wpc, f.windows);
}

bool dims(int N, int C, int H, int W, int K, int kh, int kw, int ph, int pw, int max, StageDims* g) {
  const mms_conv_shape s = {N, C, H, W, K, kh, kw, 1, 1, 0, 0, 1, 1, 1};
  if (stage_window_check(&s, ph, pw, g) != MMS_OK) return false;
  g->max = max != 0;
  return true;
}

void print_shape(StageDims g) {
  const ConvDims& d = g.d;
  const unsigned PP = (unsigned)(g.POH * g.POW);
  printf("shape N=%d C=%d H=%d W=%d K=%d kh=%d kw=%d ph=%d pw=%d OH=%d OW=%d PP=%u\n", d.N, d.C, d.H, d.W, d.K, d.kh, d.kw, g.ph, g.pw,
         d.OH, d.OW, PP);
  const TrainArgs a = train_plan(g);
  check_plan(g, a);
  const ConvProdArgs& p = a.p;
  const int ok = p.ok;
  printf("plan ok=%d kind=%d G=%d R=%d bands=%d last_rows=%d CC=%d MT=%d PS=%d groups=%d last_images=%d partial_bytes=%zu lds_bytes=%zu\n",
         ok, ok ? (int)stage_plan_kind(p) : 0, p.G, p.R, p.bands, ok ? p.OHt - (p.bands - 1) * p.R : 0, p.CC, p.MT, a.PS, a.groups,
         ok ? d.N - (d.N - 1) / p.G * p.G : 0, ok ? fused_bytes(a) : (size_t)0, a.lds_bytes);
  const TrainFinishGrid f = train_finish_grid(d.N, PP);
  check_finish(g, f);
  printf("finish windows=%u wpc=%u chunks=%u last=%u\n", f.windows, f.wpc, f.chunks, f.chunks ? f.windows - (f.chunks - 1) * f.wpc : 0);
  int route[2];
  for (int m = 0; m < 2; ++m) {
    g.max = m != 0;
    route[m] = train_route(g);
  }
  printf("route ave=%d max=%d\n", route[0], route[1]);
}

void sweep() {
  static const int kN[] = {1, 3}, kCh[] = {1, 4, 17, 33, 64}, kHW[] = {3, 9, 14, 40, 130, 258};
  static const int kKernel[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 5}, {6, 6}, {7, 7}, {8, 8}, {9, 9}, {10, 10}, {11, 11},
                                   {3, 1}, {1, 9}};
  std::map<std::string, long> n;
  for (int N : kN) for (int C : kCh) for (int K : kCh) for (int H : kHW) for (int W : kHW) for (const auto& k : kKernel) {
    if (k[0] > H || k[1] > W) continue;
    ++n["shapes"];
    for (int ph = 1; ph <= 6; ++ph) for (int pw = 1; pw <= 6; ++pw) {
      StageDims g;
      if (!dims(N, C, H, W, K, k[0], k[1], ph, pw, 0, &g)) continue;
      ++n["plans"];
      const TrainArgs a = train_plan(g);
      check_plan(g, a);
      check_finish(g, train_finish_grid(N, (unsigned)(g.POH * g.POW)));
      const ConvProdArgs own = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, 1), win = conv_prod_plan(g.d, MMS_CONV_PASS_FORWARD, ph);
      if (!a.p.ok) { ++n[own.ok ? (win.ok ? "refused_by_the_chunk" : "refused_by_the_window") : "refused_by_the_convolution"]; continue; }
      ++n["ok"];
      ++n[stage_plan_kind(a.p) == kStageImages ? "kind_images" : stage_plan_kind(a.p) == kStageRowBand ? "kind_row_band" : "kind_one_image"];
      if (a.p.R > own.R) ++n["band_higher_than_the_convolutions"];
      if (a.p.R < win.R) ++n["band_halved_for_the_chunk"];
      if (a.p.CC < a.p.Cin) ++n["several_chunks"];
      if (a.PS > a.p.G * a.p.R * a.p.OWt) ++n["tile_row_padded"];
      if (a.p.OHt % a.p.R) ++n["ragged_last_band"];
      for (int m = 0; m < 2; ++m) {
        g.max = m != 0;
        if (train_route(g) == MMS_CONV_STAGE_TRAIN_ROUTE_FUSED) ++n[m ? "fused_max" : "fused_ave"];
      }
    }
  }
  // launch 2's grid alone: a plan does not enter it
  static const int kBatch[] = {1, 2, 3, 40, 41, 50, 225, 513, 657, 1024, 1025, 1517, 4096, 65535, 65536, 65537, 70000};
  static const int kPooled[] = {1, 2, 5, 25, 81, 100, 324, 1024, 1296};
  for (int N : kBatch) for (int PP : kPooled) {
    StageDims g = {};
    g.d.N = N; g.POH = 1; g.POW = PP;
    const TrainFinishGrid f = train_finish_grid(N, (unsigned)PP);
    check_finish(g, f);
    ++n["finish_grids"];
    if (f.chunks == 1) ++n["finish_one_chunk"];
    if (f.chunks > 1 && f.wpc == kTrainFinishWindows) ++n["finish_least_chunks"];
    if (f.wpc > kTrainFinishWindows) ++n["finish_capped_chunks"];
    if (f.windows % f.wpc) ++n["finish_ragged_last_chunk"];
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
      if (!dims(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], 0, &g)) {
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
  if (!bad) printf("conv_stage_train_plans_host ok: every plan holds its invariants\n");
  return bad ? 1 : 0;
}
