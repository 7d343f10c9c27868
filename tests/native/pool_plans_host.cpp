// tests/native/pool_plans_host.cpp -- the Pooling call's host decisions, read from the C++ itself: pool_geometry,
// pool_counts and pool_forward_plan (csrc/pool_plans.h).  Host code only, no HIP call: it runs where there is no GPU.
// Every plan is held to what the kernels of csrc/pool.hip rely on; one line per violated invariant (the first of each
// kind), exit status 1.
//
//   pool_plans_host N C H W kh kw sh sw ph pw [...]
//       per shape and element size one line:  plan elem= rc= PH= PW= route= P= R= bands= items= blocks= lds_bytes=
//   pool_plans_host --sweep
//       H, W in {1..12, 31, 64, 65, 130, 700, 4097}, kernels 1..5, 33 and the whole map, strides 1..4, every pad below
//       the kernel (three of them for the large kernels), planes in {1, 3, 2049, 70000}, float and double; prints how
//       many plans left by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pool_plans.h"

using namespace mms;

namespace {

std::map<std::string, long> g_failed, g_count;

void fail(const char* inv, const mms_pool_shape& s, int elem, const char* fmt, ...) {
  if (g_failed[inv]++) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  printf("VIOLATED %s: S(%d, %d, %d, %d) k(%d, %d) s(%d, %d) p(%d, %d) elem %d: %s\n", inv, s.N, s.C, s.H, s.W,
         s.kernel_h, s.kernel_w, s.stride_h, s.stride_w, s.pad_h, s.pad_w, elem, buf);
}

#define CHECK(inv, cond, ...)                   \
  do {                                          \
    if (!(cond)) fail(inv, s, elem, __VA_ARGS__); \
  } while (0)

// the size rule in integers
long long out_dim(int in, int k, int st, int p, bool any_pad) {
  const long long span = (long long)in + 2 * p - k;
  long long o = (span >= 0 ? (span + st - 1) / st : -((-span) / st)) + 1;
  if (any_pad)
    while (o > 1 && (o - 1) * st >= in + p) --o;
  return o;
}

int check_one(const mms_pool_shape& s, int elem, bool print) {
  PoolGeom g = {};
  const int rc = pool_geometry(&s, &g);
  if (rc != MMS_OK) {
    if (print) printf("plan elem=%d rc=%d\n", elem, rc);
    ++g_count[rc == MMS_ERR_UNSUPPORTED ? "refused_unsupported" : "refused_invalid"];
    return rc;
  }
  const bool any_pad = s.pad_h || s.pad_w;
  CHECK("size_rule", g.PH == out_dim(s.H, s.kernel_h, s.stride_h, s.pad_h, any_pad) &&
                         g.PW == out_dim(s.W, s.kernel_w, s.stride_w, s.pad_w, any_pad),
        "PH %d PW %d", g.PH, g.PW);
  CHECK("last_window_inside", (long long)(g.PH - 1) * g.sh - g.pad_h < g.H && (long long)(g.PW - 1) * g.sw - g.pad_w < g.W,
        "PH %d PW %d", g.PH, g.PW);
  CHECK("first_window_inside", g.kh - g.pad_h > 0 && g.kw - g.pad_w > 0, "pads");
  long long nb = 0, nt = 0;
  if (!pool_counts(&g, &nb, &nt)) {
    ++g_count["refused_counts"];
    if (print) printf("plan elem=%d rc=%d\n", elem, MMS_ERR_INVALID_ARG);
    return MMS_ERR_INVALID_ARG;
  }
  CHECK("counts", nb == (long long)s.N * s.C * s.H * s.W && nt == (long long)s.N * s.C * g.PH * g.PW && nb <= INT_MAX &&
                      nt <= INT_MAX, "nb %lld nt %lld", nb, nt);
  if (g.planes == 0) return MMS_OK;
  const PoolPlan p = pool_forward_plan(g, elem);
  const long long cap = kPoolLdsBytes / elem, vw = 16 / elem;
  if (print)
    printf("plan elem=%d rc=0 PH=%d PW=%d route=%d P=%d R=%d bands=%d items=%lld blocks=%d lds_bytes=%zu\n", elem, g.PH,
           g.PW, p.route, p.P, p.R, p.bands, p.items, p.blocks, p.lds_bytes);
  CHECK("blocks", p.blocks >= 1 && p.blocks <= kPoolMaxBlocks && p.blocks <= p.items && p.items <= INT_MAX,
        "blocks %d items %lld", p.blocks, p.items);
  if (p.blocks < p.items) ++g_count["items_outnumber_blocks"];
  if (p.route == kPoolStaged) {
    ++g_count[g.PH * g.PW == 1 ? "staged_whole_map_window" : "staged"];
    if (p.P > 1) ++g_count["staged_several_planes"];
    CHECK("staged_fits", p.P >= 1 && (long long)p.P * g.H * g.W <= cap, "P %d", p.P);
    // the image sits up to vw - 1 elements into the LDS
    CHECK("staged_lds", ((long long)p.P * g.H * g.W + vw) * elem <= (long long)p.lds_bytes, "P %d", p.P);
    CHECK("staged_covers", p.bands == 1 && p.R == g.PH && p.items * p.P >= g.planes && (p.items - 1) * p.P < g.planes,
          "P %d items %lld", p.P, p.items);
    if (p.P * ((long long)g.planes / p.P) != g.planes) ++g_count["staged_ragged_last_item"];
  } else if (p.route == kPoolBanded) {
    ++g_count["banded"];
    CHECK("banded_items", p.P == 1 && p.R >= 1 && p.bands == (g.PH + p.R - 1) / p.R && p.items == (long long)g.planes * p.bands,
          "R %d bands %d", p.R, p.bands);
    for (int b = 0; b < p.bands; ++b) {
      const int ph0 = b * p.R, ph1 = ph0 + p.R < g.PH ? ph0 + p.R : g.PH;
      const int lo = pool_band_lo(g, ph0), hi = pool_band_hi(g, ph1);
      CHECK("band_rows", 0 <= lo && lo < hi && hi <= g.H, "band %d rows [%d, %d)", b, lo, hi);
      CHECK("band_fits", ((long long)(hi - lo) * g.W + vw) * elem <= (long long)p.lds_bytes, "band %d rows [%d, %d)", b, lo, hi);
      for (int ph = ph0; ph < ph1; ++ph) {
        const long long hs = (long long)ph * g.sh - g.pad_h, he = hs + g.kh;
        CHECK("band_holds_its_windows", (hs < 0 ? 0 : hs) >= lo && (he < g.H ? he : g.H) <= hi, "band %d ph %d", b, ph);
      }
      if (ph1 - ph0 < p.R) ++g_count["banded_ragged_last_band"];
    }
  } else {
    ++g_count["direct"];
    CHECK("direct_needed", (long long)g.kh * g.W > cap && p.lds_bytes == 0, "kh %d W %d", g.kh, g.W);
    CHECK("direct_covers", p.items * kPoolThreads >= nt && (p.items - 1) * kPoolThreads < nt, "items %lld", p.items);
  }
  return MMS_OK;
}

int finish() {
  for (const auto& kv : g_count) printf("count %s=%ld\n", kv.first.c_str(), kv.second);
  long bad = 0;
  for (const auto& kv : g_failed) bad += kv.second;
  if (bad) {
    printf("%ld violations of %zu invariants\n", bad, g_failed.size());
    return 1;
  }
  printf("every plan holds its invariants\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--sweep")) {
    const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 31, 64, 65, 130, 700, 4097};
    const int planes[] = {1, 3, 2049, 70000};
    long shapes = 0;
    for (int H : sizes)
      for (int W : sizes) {
        std::vector<int> kernels = {1, 2, 3, 4, 5, 33};
        for (int kh : kernels)
          for (int whole = 0; whole < 2; ++whole)
            for (int st = 1; st <= 4; ++st) {
              const int k_h = whole ? H : kh, k_w = whole ? W : kh;
              if (whole && kh != 1) continue;
              for (int pad = 0; pad < (k_h < k_w ? k_h : k_w); pad = pad < 2 ? pad + 1 : (pad < k_h / 2 ? k_h / 2 : 1 << 30))
                for (int n : planes)
                  for (int elem : {4, 8}) {
                    const mms_pool_shape s = {n, 1, H, W, k_h, k_w, st, whole ? 1 : st, pad, whole ? 0 : pad, MMS_POOL_MAX};
                    check_one(s, elem, false);
                    ++shapes;
                  }
            }
      }
    // the rest of the refusal table
    const int elem = 4;
    mms_pool_shape s = {1, 1, 4, 4, 2, 2, 2, 2, 0, 0, MMS_POOL_STOCHASTIC};
    PoolGeom g;
    CHECK("stochastic", pool_geometry(&s, &g) == MMS_ERR_UNSUPPORTED, "rc");
    s.method = 3;
    CHECK("unknown_method", pool_geometry(&s, &g) == MMS_ERR_INVALID_ARG, "rc");
    CHECK("null_shape", pool_geometry(nullptr, &g) == MMS_ERR_INVALID_ARG, "rc");
    s.method = MMS_POOL_AVE;
    s.N = 70000;
    s.C = 70000;
    CHECK("counts_refused", pool_geometry(&s, &g) == MMS_OK && check_one(s, 4, false) == MMS_ERR_INVALID_ARG, "rc");
    printf("count shapes=%ld\n", shapes);
    return finish();
  }
  if (argc < 11 || (argc - 1) % 10) {
    fprintf(stderr, "usage: %s --sweep | N C H W kh kw sh sw ph pw [...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 9 < argc; i += 10) {
    int v[10];
    for (int j = 0; j < 10; ++j) v[j] = atoi(argv[i + j]);
    const mms_pool_shape s = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], MMS_POOL_MAX};
    printf("shape %d %d %d %d %d %d %d %d %d %d\n", v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
    for (int elem : {4, 8}) check_one(s, elem, true);
  }
  return finish();
}
