// csrc/conv_plans.h -- the host-side plans of csrc/conv.hip's parameter diffs, in a header so that a host program can
// read them (tests/native/conv_plans_host.cpp prints every plan and asserts what the kernels rely on): the fast
// parameter-diff launch (ConvWdiffArgs, conv_wdiff_plan) and the slab count of the generic one (conv_generic_slabs).
// The product's plan, conv_prod_plan, is csrc/conv_tile.h's.  Host text only; the kernels are csrc/conv.hip's.
#ifndef MMS_CONV_PLANS_H_
#define MMS_CONV_PLANS_H_

#include "conv_tile.h"

namespace mms {

constexpr int kConvMaxSlabs = 64;          // partial sums of the parameter diffs per element, at most

inline int conv_generic_slabs(const ConvDims& d, int* rps) {
  const int rows = d.N * d.OH;
  const int want = rows < kConvMaxSlabs ? rows : kConvMaxSlabs;
  *rps = (rows + want - 1) / want;
  return (rows + *rps - 1) / *rps;
}

struct ConvWdiffArgs {
  const float* x;        // (N, C, H, W)
  const float* dy;       // (N, K, OH, OW)
  float* part;           // [slab][nW + K]
  int N, C, K, H, W, OH, OW, kh, kw;
  int G, R, bands;       // conv_tile_geometry of the top pixels, shrunk to the LDS
  int plane;             // (R + kh - 1) * W
  int PP;                // row length of the staged top_diff tile: conv_round4(G * R * OW) + 1
  int MT;
  int units, ups, slabs; // (image group, band) units; units per slab; slabs
  int want_w, want_b;
  bool ok;
  size_t lds_bytes;
};

inline ConvWdiffArgs conv_wdiff_plan(const ConvDims& d) {
  ConvWdiffArgs a = {};
  if (d.sh != 1 || d.sw != 1 || d.ph != 0 || d.pw != 0 || d.G != 1 || d.C > kConvMaxChannels || d.K > kConvMaxChannels)
    return a;
  a.N = d.N; a.C = d.C; a.K = d.K; a.H = d.H; a.W = d.W; a.OH = d.OH; a.OW = d.OW; a.kh = d.kh; a.kw = d.kw;
  if (!conv_tile_geometry(d.OH, d.OW, 1, &a.G, &a.R, &a.bands)) return a;
  a.MT = d.K <= 16 ? 1 : d.K <= 32 ? 2 : 4;
  for (;;) {
    a.plane = (a.R + d.kh - 1) * d.W;
    a.PP = conv_round4(a.G * a.R * d.OW) + 1;
    const long long need = (long long)a.G * d.C * a.plane + (long long)16 * a.MT * a.PP + a.PP;
    if (need <= kConvLdsFloats) break;
    if (a.G > 1) { --a.G; continue; }
    if (a.R > 1) { --a.R; a.bands = (d.OH + a.R - 1) / a.R; continue; }
    return a;
  }
  a.lds_bytes = ((size_t)a.G * d.C * a.plane + (size_t)16 * a.MT * a.PP + a.PP) * sizeof(float);
  a.units = d.N ? ((d.N + a.G - 1) / a.G) * a.bands : 0;
  const int want = a.units < kConvMaxSlabs ? a.units : kConvMaxSlabs;
  a.ups = want ? (a.units + want - 1) / want : 1;
  a.slabs = (a.units + a.ups - 1) / a.ups;
  a.ok = true;
  return a;
}

}  // namespace mms
#endif  // MMS_CONV_PLANS_H_
