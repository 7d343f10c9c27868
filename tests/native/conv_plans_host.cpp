// tests/native/conv_plans_host.cpp -- the launch plans of the fast convolution route, read from the C++ itself:
// conv_prod_plan (csrc/conv_tile.h) and conv_wdiff_plan / conv_generic_slabs (csrc/conv_plans.h).  Host code only, no
// HIP call: it runs where there is no GPU.  Every plan it computes is held to what the kernels rely on (check_* below);
// one line per violated invariant (the first of each kind), exit status 1.
//
//   conv_plans_host N C H W K kh kw [N C H W K kh kw ...]
//       stride 1, pad 0, group 1.  Per shape, one line per pass and two for the counts (key=value; G0 R0: the
//       geometry before the plan shrank it to the LDS):
//         forward | bottom_diff   ok G0 R0 G R bands BW plane Cin CC Kpad MT lds_bytes
//         param_diff              ok G0 R0 G R bands plane PP MT units ups slabs groups lds_bytes
//         generic_slabs           slabs rps
//         workspace               slabs bytes       max(generic slabs, fast slabs) * (nW + K) * 4
//   conv_plans_host --sweep
//       N in {1, 3}, C and K in {1, 4, 17, 33, 64}, H and W in {3, 9, 14, 40, 130, 258}, kernels 1 x 1 .. 11 x 11, 3 x 1
//       and 1 x 9 where they fit, rq in {1, 2, 4, 5} where it divides the output height, both passes of the product and
//       the parameter diff; prints how many plans left by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "conv_plans.h"

using namespace mms;

namespace {

std::map<std::string, long> g_failed;      // invariant -> times violated

void fail(const char* inv, const ConvDims& d, const char* what, int rq, const char* fmt, ...) {
  if (g_failed[inv]++) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  printf("VIOLATED %s: S(%d, %d, %d, %d, %d, %d, %d) %s rq=%d: %s\n", inv, d.N, d.C, d.H, d.W, d.K, d.kh, d.kw, what, rq, buf);
}

#define CHECK(inv, cond, ...) \
  do {                        \
    if (!(cond)) fail(inv, d, what, rq, __VA_ARGS__); \
  } while (0)

struct Geometry { bool ok; int G, R, bands; };

Geometry geometry(int OHt, int OWt, int rq) {
  Geometry g = {};
  g.ok = conv_tile_geometry(OHt, OWt, rq, &g.G, &g.R, &g.bands);
  return g;
}

// What conv_tile_product<MT> and its launch rely on.
void check_prod(const ConvDims& d, int pass, int rq, const ConvProdArgs& a) {
  const char* what = pass ? "bottom_diff" : "forward";
  if (!a.ok) return;
  const long long khkw = (long long)d.kh * d.kw, Mpad = 16LL * a.MT;
  CHECK("lds", a.lds_bytes <= sizeof(float) * (size_t)kConvLdsFloats, "lds_bytes %zu", a.lds_bytes);
  CHECK("lds", (long long)a.lds_bytes == 4 * ((long long)a.G * a.CC * a.plane + Mpad * a.Kpad + a.Kpad),
        "lds_bytes %zu is not band + weights + offsets", a.lds_bytes);
  CHECK("tile", a.G >= 1 && a.R >= 1 && (long long)a.G * a.R * a.OWt <= kConvTilePixels, "G %d R %d OWt %d", a.G, a.R, a.OWt);
  CHECK("rq", a.R % rq == 0, "R %d", a.R);
  CHECK("bands", (long long)a.bands * a.R >= a.OHt && a.OHt > (long long)(a.bands - 1) * a.R, "bands %d R %d OHt %d", a.bands,
        a.R, a.OHt);
  CHECK("chunk", a.CC >= 1 && a.CC <= a.Cin, "CC %d Cin %d", a.CC, a.Cin);
  CHECK("chunk", a.Kpad == conv_round4((int)(a.CC * khkw)) && a.Kpad % 4 == 0, "Kpad %d CC %d", a.Kpad, a.CC);
  CHECK("band", a.BW == a.IW + 2 * a.vpw && a.plane == (a.R + a.kh - 1) * a.BW, "BW %d plane %d", a.BW, a.plane);
  CHECK("band", a.OHt + a.kh - 1 == a.IH + 2 * a.vph && a.OWt + a.kw - 1 == a.IW + 2 * a.vpw, "OHt %d OWt %d", a.OHt, a.OWt);
  CHECK("channels", (a.MT == 1 || a.MT == 2 || a.MT == 4) && a.Cout <= 16 * a.MT && (a.MT == 1 || a.Cout > 8 * a.MT),
        "MT %d Cout %d", a.MT, a.Cout);
}

// What conv_wdiff_kernel<MT>, its launch and conv_reduce_kernel rely on.
void check_wdiff(const ConvDims& d, const ConvWdiffArgs& a) {
  const char* what = "param_diff";
  const int rq = 1;
  if (!a.ok) return;
  CHECK("lds", a.lds_bytes <= sizeof(float) * (size_t)kConvLdsFloats, "lds_bytes %zu", a.lds_bytes);
  CHECK("lds", (long long)a.lds_bytes == 4 * ((long long)a.G * d.C * a.plane + 16LL * a.MT * a.PP + a.PP),
        "lds_bytes %zu is not band + top_diff tile + offsets", a.lds_bytes);
  CHECK("tile", a.G >= 1 && a.R >= 1 && (long long)a.G * a.R * d.OW <= kConvTilePixels, "G %d R %d OW %d", a.G, a.R, d.OW);
  CHECK("tile", a.PP == conv_round4(a.G * a.R * d.OW) + 1 && a.plane == (a.R + d.kh - 1) * d.W, "PP %d plane %d", a.PP, a.plane);
  CHECK("bands", (long long)a.bands * a.R >= d.OH && d.OH > (long long)(a.bands - 1) * a.R, "bands %d R %d OH %d", a.bands,
        a.R, d.OH);
  CHECK("channels", (a.MT == 1 || a.MT == 2 || a.MT == 4) && d.K <= 16 * a.MT && (a.MT == 1 || d.K > 8 * a.MT), "MT %d K %d",
        a.MT, d.K);
  CHECK("slabs", a.units == (d.N + a.G - 1) / a.G * a.bands, "units %d G %d bands %d", a.units, a.G, a.bands);
  CHECK("slabs", a.slabs >= 1 && a.slabs <= kConvMaxSlabs && a.ups >= 1, "slabs %d ups %d", a.slabs, a.ups);
  CHECK("slabs", (long long)a.slabs * a.ups >= a.units && a.units > (long long)(a.slabs - 1) * a.ups, "units %d on %d slabs of %d",
        a.units, a.slabs, a.ups);
}

void check_generic(const ConvDims& d, int slabs, int rps) {
  const char* what = "generic_slabs";
  const int rq = 1;
  const long long rows = (long long)d.N * d.OH;
  CHECK("slabs", slabs >= 1 && slabs <= kConvMaxSlabs && rps >= 1, "slabs %d rps %d", slabs, rps);
  CHECK("slabs", (long long)slabs * rps >= rows && rows > (long long)(slabs - 1) * rps, "%lld rows on %d slabs of %d", rows, slabs, rps);
}

bool dims(int N, int C, int H, int W, int K, int kh, int kw, ConvDims* d) {
  const mms_conv_shape s = {N, C, H, W, K, kh, kw, 1, 1, 0, 0, 1, 1, 1};
  return conv_check(&s, d) == MMS_OK;
}

void print_shape(const ConvDims& d) {
  printf("shape N=%d C=%d H=%d W=%d K=%d kh=%d kw=%d OH=%d OW=%d\n", d.N, d.C, d.H, d.W, d.K, d.kh, d.kw, d.OH, d.OW);
  for (int pass = 0; pass < 2; ++pass) {
    const ConvProdArgs a = conv_prod_plan(d, pass, 1);
    check_prod(d, pass, 1, a);
    const Geometry g = geometry(pass ? d.H : d.OH, pass ? d.W : d.OW, 1);
    printf("%s ok=%d G0=%d R0=%d G=%d R=%d bands=%d BW=%d plane=%d Cin=%d CC=%d Kpad=%d MT=%d lds_bytes=%zu\n",
           pass ? "bottom_diff" : "forward", (int)a.ok, g.G, g.R, a.ok ? a.G : 0, a.ok ? a.R : 0, a.ok ? a.bands : 0,
           a.ok ? a.BW : 0, a.ok ? a.plane : 0, a.Cin, a.ok ? a.CC : 0, a.Kpad, a.ok ? a.MT : 0, a.lds_bytes);
  }
  const ConvWdiffArgs w = conv_wdiff_plan(d);
  check_wdiff(d, w);
  const Geometry g = geometry(d.OH, d.OW, 1);
  printf("param_diff ok=%d G0=%d R0=%d G=%d R=%d bands=%d plane=%d PP=%d MT=%d units=%d ups=%d slabs=%d groups=%d lds_bytes=%zu\n",
         (int)w.ok, g.G, g.R, w.ok ? w.G : 0, w.ok ? w.R : 0, w.ok ? w.bands : 0, w.ok ? w.plane : 0, w.ok ? w.PP : 0,
         w.ok ? w.MT : 0, w.units, w.ups, w.slabs, (d.C * d.kh * d.kw + 63) / 64, w.lds_bytes);
  int rps = 0;
  const int gs = conv_generic_slabs(d, &rps);
  check_generic(d, gs, rps);
  printf("generic_slabs slabs=%d rps=%d\n", gs, rps);
  const int slabs = w.ok && w.slabs > gs ? w.slabs : gs;
  printf("workspace slabs=%d bytes=%zu\n", slabs, (size_t)slabs * ((size_t)d.K * d.Cg * d.kh * d.kw + d.K) * sizeof(float));
}

int sweep() {
  static const int kN[] = {1, 3}, kCh[] = {1, 4, 17, 33, 64}, kHW[] = {3, 9, 14, 40, 130, 258}, kRq[] = {1, 2, 4, 5};
  static const int kKernel[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 5}, {6, 6}, {7, 7}, {8, 8}, {9, 9}, {10, 10}, {11, 11},
                                   {3, 1}, {1, 9}};
  std::map<std::string, long> n;
  for (int N : kN) for (int C : kCh) for (int K : kCh) for (int H : kHW) for (int W : kHW) for (const auto& k : kKernel) {
    if (k[0] > H || k[1] > W) continue;
    ConvDims d;
    if (!dims(N, C, H, W, K, k[0], k[1], &d)) { ++n["shape_refused"]; continue; }
    ++n["shapes"];
    for (int pass = 0; pass < 2; ++pass)
      for (int rq : kRq) {
        const int OHt = pass ? d.H : d.OH, OWt = pass ? d.W : d.OW;
        if (OHt % rq) continue;
        const ConvProdArgs a = conv_prod_plan(d, pass, rq);
        check_prod(d, pass, rq, a);
        const Geometry g = geometry(OHt, OWt, rq);
        ++n["prod_plans"];
        if (!a.ok) { ++n[g.ok ? "prod_refused_by_lds" : "prod_refused_by_tile"]; continue; }
        ++n["prod_ok"];
        if (a.G == g.G && a.R == g.R) ++n["prod_first_pass"];
        if (a.G < g.G) ++n["prod_G_halved"];
        if (a.G < g.G && a.G > 1) ++n["prod_G_halved_above_one"];
        if (a.R < g.R) ++n["prod_R_halved"];
        if (a.CC < (a.Cin < 4 ? a.Cin : 4)) ++n["prod_few_channels"];
        if (a.CC < a.Cin && a.bands > 1) ++n["prod_chunks_and_bands"];
        if (a.MT == 4 && pass == 1) ++n["prod_MT4_bottom_diff"];
      }
    const ConvWdiffArgs w = conv_wdiff_plan(d);
    check_wdiff(d, w);
    const Geometry g = geometry(d.OH, d.OW, 1);
    ++n["wdiff_plans"];
    if (!w.ok) {
      ++n[g.ok ? "wdiff_refused_by_lds" : "wdiff_refused_by_tile"];
    } else {
      ++n["wdiff_ok"];
      if (w.G == g.G && w.R == g.R) ++n["wdiff_first_pass"];
      if (w.G < g.G) ++n["wdiff_G_decremented"];
      if (w.R < g.R) ++n["wdiff_R_decremented"];
      if (w.ups > 1 && w.bands > 1) ++n["wdiff_slab_inside_image"];
      int rps = 0;
      if (conv_generic_slabs(d, &rps) != w.slabs) ++n["slab_counts_differ"];
    }
    if (conv_prod_plan(d, 0, 1).ok && !w.ok) ++n["forward_fast_param_diff_generic"];
    if (conv_prod_plan(d, 0, 1).ok && !conv_prod_plan(d, 1, 1).ok) ++n["forward_fast_bottom_diff_generic"];
    int rps = 0;
    check_generic(d, conv_generic_slabs(d, &rps), rps);
  }
  for (const auto& kv : n) printf("sweep %s=%ld\n", kv.first.c_str(), kv.second);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) {
    sweep();
  } else if (argc >= 8 && (argc - 1) % 7 == 0) {
    for (int i = 1; i < argc; i += 7) {
      int v[7];
      for (int k = 0; k < 7; ++k) v[k] = atoi(argv[i + k]);
      ConvDims d;
      if (!dims(v[0], v[1], v[2], v[3], v[4], v[5], v[6], &d)) {
        fprintf(stderr, "%s: the shape check refuses argument %d onwards\n", argv[0], i);
        return 2;
      }
      print_shape(d);
    }
  } else {
    fprintf(stderr, "usage: %s --sweep | N C H W K kh kw [N C H W K kh kw ...]\n", argv[0]);
    return 2;
  }
  long bad = 0;
  for (const auto& kv : g_failed) {
    printf("invariant %s violated %ld time(s)\n", kv.first.c_str(), kv.second);
    bad += kv.second;
  }
  if (!bad) printf("conv_plans_host ok: every plan holds its invariants\n");
  return bad ? 1 : 0;
}
