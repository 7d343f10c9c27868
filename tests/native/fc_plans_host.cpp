// tests/native/fc_plans_host.cpp -- the host decisions of the calls of include/mms_fc.h, read from the C++ itself
// (csrc/fc_plans.h).  Host code only, no HIP call: it runs where there is no GPU.  Every plan is held to what the
// kernels of csrc/fc.hip rely on; one line per violated invariant (the first of each kind), exit status 1.
//
//   fc_plans_host M K N [...]
//       per shape one line:  plan rc= fwd_route= bwd_route= slabs= slab_rows= fwd= wdiff= bottom= ws_elems=
//   fc_plans_host --sweep
//       M, K, N over sizes around every constant of the header, up to INT_MAX; the loss slabs for P likewise; Concat's
//       judgement.  Prints how many plans left by each branch.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "fc_plans.h"

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

#define CHECK(inv, cond, ...)           \
  do {                                  \
    if (!(cond)) fail(inv, __VA_ARGS__); \
  } while (0)

// one product of the fast route: the tile kernel's grid within the limits, its tiles covering the output once
const char* check_product(long long rows, long long cols, int slabs) {
  ++g_count["tiled"];
  const FcNarrowGrid g = fc_narrow_grid((int)rows, (int)cols, slabs);
  CHECK("tile_grid", g.blocks_x >= 1 && g.blocks_x <= kFcMaxBlocks && g.blocks_y == slabs && g.blocks_y >= 1 &&
                         g.blocks_y <= kFcMaxSlabs && (long long)g.row_tiles * 16 >= rows &&
                         (long long)(g.row_tiles - 1) * 16 < rows && (long long)g.col_tiles * 16 >= cols &&
                         (long long)(g.col_tiles - 1) * 16 < cols,
        "rows %lld cols %lld: %d x %d tiles, grid %d x %d", rows, cols, g.row_tiles, g.col_tiles, g.blocks_x, g.blocks_y);
  if ((long long)g.row_tiles * g.col_tiles > 4LL * g.blocks_x) ++g_count["tiles_outnumber_waves"];
  return "tiled";
}

int check_ip(int M, int K, int N, bool print) {
  const mms_inner_product_shape s = {M, K, N, 0, 1};
  FcDims d = {};
  const int rc = fc_ip_check(&s, &d);
  if (rc != MMS_OK) {
    ++g_count["ip_refused"];
    CHECK("refused_only_when_due", M < 0 || K < 1 || N < 1 || (long long)M * K > INT_MAX || (long long)M * N > INT_MAX ||
                                       (long long)K * N > INT_MAX, "M %d K %d N %d", M, K, N);
    if (print) printf("plan rc=%d\n", rc);
    return rc;
  }
  CHECK("accepted_counts_fit", (long long)M * K <= INT_MAX && (long long)M * N <= INT_MAX && (long long)K * N <= INT_MAX,
        "M %d K %d N %d", M, K, N);
  if (M == 0) {
    ++g_count["ip_empty"];
    CHECK("empty_workspace", fc_ip_workspace_elems(d) == 0, "M 0");
    if (print) printf("plan rc=0 empty\n");
    return MMS_OK;
  }
  // the slabs cover [0, M) once, and the last one's end, formed as the kernels form it, is M
  const int rows = fc_slab_rows(M), slabs = fc_slabs(M);
  CHECK("slab_rows", rows >= kFcSlabRows && rows % 32 == 0, "M %d rows %d", M, rows);
  CHECK("slabs_cover", slabs >= 1 && slabs <= kFcMaxSlabs && (long long)slabs * rows >= M && (long long)(slabs - 1) * rows < M,
        "M %d rows %d slabs %d", M, rows, slabs);
  CHECK("slab_starts_fit_int", (long long)(slabs - 1) * rows <= INT_MAX, "M %d", M);
  if (slabs > 1) ++g_count["several_slabs"];
  if (rows > kFcSlabRows) ++g_count["long_slabs"];
  CHECK("workspace", fc_ip_workspace_elems(d) == (long long)slabs * ((long long)K * N + N), "M %d K %d N %d", M, K, N);
  // exactly one route per pass
  const int fr = fc_ip_route(d, MMS_FC_PASS_FORWARD), br = fc_ip_route(d, MMS_FC_PASS_BACKWARD);
  CHECK("one_route", (fr == MMS_FC_ROUTE_FAST || fr == MMS_FC_ROUTE_GENERIC) && (br == MMS_FC_ROUTE_FAST || br == MMS_FC_ROUTE_GENERIC),
        "routes %d %d", fr, br);
  CHECK("no_other_pass", fc_ip_route(d, 2) == MMS_FC_ROUTE_NONE && fc_ip_route(d, -1) == MMS_FC_ROUTE_NONE, "pass");
  const bool big = (long long)M * K * N >= kFcFastMinMacs;
  CHECK("forward_rule", (fr == MMS_FC_ROUTE_FAST) == (big && (M <= kFcNarrowMax || N <= kFcNarrowMax || K >= kFcFastFwdMinK)), "M %d K %d N %d", M, K, N);
  CHECK("backward_rule", (br == MMS_FC_ROUTE_FAST) == (big && slabs > 1), "M %d K %d N %d", M, K, N);
  ++g_count[fr == MMS_FC_ROUTE_FAST ? "fwd_fast" : "fwd_generic"];
  ++g_count[br == MMS_FC_ROUTE_FAST ? "bwd_fast" : "bwd_generic"];
  const char *f = "-", *w = "-", *b = "-";
  if (fr == MMS_FC_ROUTE_FAST) f = check_product(M, N, 1);
  if (br == MMS_FC_ROUTE_FAST) {
    w = check_product(N, K, slabs);
    check_product(K, N, slabs);             // transpose
    b = check_product(M, K, 1);
  }
  // the sweeps of the generic kernels and of the finish
  for (long long units : {(long long)M * N, (long long)M * K, (long long)slabs * K * N, (long long)K * N + N}) {
    const int blocks = fc_sweep_blocks(units);
    CHECK("sweep_blocks", blocks >= 1 && blocks <= kFcMaxBlocks, "units %lld blocks %d", units, blocks);
  }
  if (print)
    printf("plan rc=0 fwd_route=%d bwd_route=%d slabs=%d slab_rows=%d fwd=%s wdiff=%s bottom=%s ws_elems=%lld\n", fr, br, slabs,
           rows, f, w, b, fc_ip_workspace_elems(d));
  return MMS_OK;
}

void check_loss(long long P) {
  const int len = fc_loss_slab_len(P), slabs = fc_loss_slabs(P);
  CHECK("loss_slabs", len >= kLossSlabMin && slabs >= 1 && slabs <= kLossMaxSlabs && slabs <= kFcThreads &&
                          (long long)slabs * len >= P && (long long)(slabs - 1) * len < P,
        "P %lld len %d slabs %d", P, len, slabs);
  CHECK("loss_workspace", fc_loss_workspace_bytes(P, 4) == (size_t)(slabs + 1) * 4 + (size_t)slabs * 4 &&
                              fc_loss_workspace_bytes(P, 8) == (size_t)(slabs + 1) * 8 + (size_t)slabs * 4,
        "P %lld", P);
  ++g_count[len > kLossSlabMin ? "loss_long_slabs" : "loss_slabs"];
}

void check_concat() {
  ConcatDims d;
  mms_concat_shape s = {7, 5, 4, {1, 3, 4, 64, 0, 0, 0, 0}};
  CHECK("concat_ok", fc_concat_check(&s, &d) == MMS_OK && d.top_axis == 72 && d.offset[3] == 8 && d.nb == 4, "axis");
  for (int nb : {0, 9, -1}) {
    s.num_bottoms = nb;
    CHECK("concat_bottoms", fc_concat_check(&s, &d) == MMS_ERR_INVALID_ARG, "num_bottoms %d", nb);
  }
  s.num_bottoms = 8;
  CHECK("concat_eight", fc_concat_check(&s, &d) == MMS_OK && d.top_axis == 72, "eight");
  s.axis_extent[5] = -1;
  CHECK("concat_negative_extent", fc_concat_check(&s, &d) == MMS_ERR_INVALID_ARG, "extent");
  s.axis_extent[5] = INT_MAX;
  CHECK("concat_counts", fc_concat_check(&s, &d) == MMS_ERR_INVALID_ARG, "INT_MAX extent");
  s.axis_extent[5] = 0;
  s.num_concats = 1 << 24;
  CHECK("concat_top_count", fc_concat_check(&s, &d) == MMS_ERR_INVALID_ARG, "top over INT_MAX");
  mms_concat_shape z = {1, 1, 2, {0, 0, 0, 0, 0, 0, 0, 0}};
  CHECK("concat_empty_axis", fc_concat_check(&z, &d) == MMS_ERR_INVALID_ARG, "axis 0");
  CHECK("concat_null", fc_concat_check(nullptr, &d) == MMS_ERR_INVALID_ARG, "null");
  ++g_count["concat"];
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
    const int sizes[] = {0,   1,   2,    3,    7,    15,   16,   17,      31,      32,        33,        50,        63,
                         64,  65,  127,  128,  129,  205,  256,  257,     1517,    2047,      2048,      8191,      8192,
                         8193, 65535, 65536, 1 << 20, 4194240, 4194241, 1 << 24, 46340, 46341, INT_MAX / 2, INT_MAX};
    long shapes = 0;
    for (int M : sizes)
      for (int K : sizes)
        for (int N : sizes) {
          check_ip(M, K, N, false);
          ++shapes;
        }
    check_ip(-1, 4, 4, false);
    for (long long P : {1LL, 63LL, 64LL, 65LL, 350LL, 1517LL, 16384LL, 16385LL, 1LL << 24, (long long)INT_MAX}) check_loss(P);
    check_concat();
    printf("count shapes=%ld\n", shapes);
    return finish();
  }
  if (argc < 4 || (argc - 1) % 3) {
    fprintf(stderr, "usage: %s --sweep | M K N [...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 2 < argc; i += 3) {
    printf("shape %s %s %s\n", argv[i], argv[i + 1], argv[i + 2]);
    check_ip(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), true);
  }
  return finish();
}
