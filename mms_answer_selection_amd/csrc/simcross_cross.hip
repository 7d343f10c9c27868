// csrc/simcross_cross.hip -- SimCross dist_mode 0 (cosine) and 1 (Euclidean) with fp32 storage: the float
// instantiations of the word-grid kernels and launch plan of cross_grid.h (reference semantics there), the Euclidean
// lane kernel, which exists for fp32 storage alone, and the three fp32 entry points.
//
// W1 == W2 == 1 (sentence-vector pairs) has kernels of its own in simcross_rows.hip (Euclid) and
// simcross_rows_cosine.hip; the entry points at the end of this file try those first and fall through to the grid
// kernels.
//
// Compiled with -ffp-contract=off: the reference CPU build has no FMA
// contraction, so mul and add must round separately to match it bitwise.
#include "cross_grid.h"

namespace mms {

// ---- Euclidean cross-geometry backward for MANY pairs of narrow word grids (cfg 4's 1517 x 40 x 40 x 50) ------
// cross_bwd_tiled_kernel computes every term tt[j,k,d] twice (once in the k-ordered sum of dq[j,d], once in
// the j-ordered sum of da[k,d]) and wastes 44 % of its second 32-wide d chunk at D = 50.  Here ONE WAVE owns a
// pair and a LANE owns a column d: the lane walks j (outer) and k (inner) over all W1*W2 terms of its column,
// each computed ONCE; dq[j,d] is the running sum over k inside one j (k ascending, as :209-223), and the W2
// accumulators da[k,d] stay in registers across the j loop (j ascending) -- the reference's accumulation
// orders, so the Euclidean results keep their bits.  The per-(j,k) coefficients are wave-uniform: built once
// into LDS (c and fl32(1/den), or c, den, 1/den for the reference rounding) and read back as broadcasts.
// W2 is a compile-time constant (even; the widths the dispatcher instantiates -- the reference pads sentences to
// one length, 40 in network_v4): the k loop is straight-line code, two k per packed sub / mul / mul, with all
// of a row's coefficient reads in flight together.  Other widths keep cross_bwd_tiled_kernel.
// NW = 2 (fp32 arithmetic only): TWO waves per pair, wave w takes the rows j of half w -- its own rows of the
// coefficient table, its own rows of dq (complete, k ascending as before), and a partial da over its rows; da is
// the sum of the two partials (one association away from the j-ascending sum: inside the mode's 2-ulp-per-term
// contract, not bit-identical -- the reference-rounding mode keeps one wave per pair).  1517 pairs are 1.5 waves
// per SIMD with one wave per pair -- the launch takes as long as the SIMDs that hold two -- and 3 with two.
template <int W2C, bool EXACT, int NW = 1>
__global__ __launch_bounds__(64 * NW) void cross_bwd_lane_kernel(
    const float* __restrict__ q, const float* __restrict__ a, const float* __restrict__ top,
    const float* __restrict__ top_diff, float* __restrict__ dq, float* __restrict__ da, int W1, int D) {
  static_assert(W2C % 2 == 0, "two k per packed operation");
  static_assert(NW == 1 || !EXACT, "the reference-rounding mode sums da in j order: one wave per pair");
  constexpr int KP = W2C / 2;
  extern __shared__ __attribute__((aligned(16))) double lds_lane[];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int JH = (W1 + NW - 1) / NW;                       // rows per wave
  const int jb = min(wv * JH, W1), je = min(jb + JH, W1);
  const int JK = W1 * W2C;
  // tables (index e = j*W2C + k, the blob's own order): EXACT: double den[], double rcp[], float c[];
  // otherwise float2 (c, fl32(1/den))[]
  double* t_den = lds_lane;
  double* t_rcp = lds_lane + (EXACT ? JK : 0);
  float* t_c = reinterpret_cast<float*>(lds_lane + (EXACT ? 2 * JK : 0));
  // fp32 mode: W2C/2 float4 (c_k, c_k+1, r_k, r_k+1) per row j
  const float* Tn = top + (size_t)n * JK;
  const float* gn = top_diff + (size_t)n * JK;
  const int eb = jb * W2C, ee = je * W2C;                  // this wave's rows of the table
  for (int e0 = eb + lane; e0 < ee; e0 += 64 * 8) {
    float tv[8], gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int e = min(e0 + 64 * u, JK - 1); tv[u] = Tn[e]; gv[u] = gn[e]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 64 * u;
      if (e >= ee) break;
      const EuclidCoef kc = euclid_coef(tv[u], gv[u]);
      if (EXACT) { t_c[e] = kc.c; t_den[e] = kc.den; t_rcp[e] = kc.rcp; }
      else {                                             // per k pair: (c_k, c_k+1, r_k, r_k+1)
        float* f = reinterpret_cast<float*>(lds_lane);
        const int p4 = (e >> 1) * 4 + (e & 1);           // W2C even: pairs never straddle rows
        f[p4] = kc.c;
        f[p4 + 2] = (float)kc.rcp;
      }
    }
  }
  const bool live = lane < D;
  const int d = live ? lane : D - 1;
  const float* qn = q + (size_t)n * W1 * D + d;
  const float* an = a + (size_t)n * W2C * D + d;
  float2v av[KP], acc[KP];
#pragma unroll
  for (int kp = 0; kp < KP; ++kp) {
    av[kp].x = an[(size_t)(2 * kp) * D];
    av[kp].y = an[(size_t)(2 * kp + 1) * D];
    acc[kp] = (float2v){0.f, 0.f};
  }
  wave_lds_sync();
  float* dqn = dq + (size_t)n * W1 * D + d;
  if (EXACT) {
    float qv = qn[0];
    for (int j = 0; j < W1; ++j) {
      const float qnext = qn[(size_t)min(j + 1, W1 - 1) * D];
      float accq = 0.f;
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) {
        EuclidCoef k0, k1;
        const int e = j * W2C + 2 * kp;
        k0.c = t_c[e]; k0.den = t_den[e]; k0.rcp = t_rcp[e];
        k1.c = t_c[e + 1]; k1.den = t_den[e + 1]; k1.rcp = t_rcp[e + 1];
        float2v tt;
        tt.x = euclid_tt(k0, qv - av[kp].x);
        tt.y = euclid_tt(k1, qv - av[kp].y);
        accq += tt.x;
        accq += tt.y;
        acc[kp] = acc[kp] - tt;                            // da += -tt, j ascending
      }
      if (live) dqn[(size_t)j * D] = accq;
      qv = qnext;
    }
  } else {
    typedef float float4v __attribute__((ext_vector_type(4)));
    const float4v* tab = reinterpret_cast<const float4v*>(lds_lane);
    // a row's W2C/2 (c0, c1, r0, r1) entries are read together at the top of its iteration (16-byte broadcast
    // reads); the next q value is requested one iteration ahead.  Measured alternatives at 1517 x 40 x 40 x 50
    // (this form: 39.5 us; cross_bwd_tiled_kernel: 62): a second row buffer (ping-pong) needs 290 VGPRs = one
    // wave per SIMD, 61 us; re-loading each entry right after its use 44 us; q staged through LDS as well 42.5 us.
    // What bounds it is the LDS return path -- every wave reads its whole 12.8 KB table for all 64 lanes, 18 us
    // of LDS cycles per CU -- next to the VALU issue of the SIMDs that hold two of the 1517 waves.  The
    // coefficients on the SCALAR path instead (a table in a workspace written by a first launch, read through
    // wave-uniform addresses: five s_load_dwordx16 per row, SGPR operands of the packed multiplies) was built and
    // measured: 61 us -- 80 SGPRs per row leave no room to run the loads ahead, so each row exposes its
    // scalar-cache misses (the 19 MB table streams through once).
    float qv = qn[(size_t)min(jb, W1 - 1) * D];
    for (int j = jb; j < je; ++j) {
      const float qnext = qn[(size_t)min(j + 1, W1 - 1) * D];
      const float2v qq = {qv, qv};
      float4v cr[KP];
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) cr[kp] = tab[(size_t)j * KP + kp];
      float accq = 0.f;
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) {
        const float2v c = {cr[kp].x, cr[kp].y}, r = {cr[kp].z, cr[kp].w};
        const float2v tt = (c * (qq - av[kp])) * r;
        accq += tt.x;
        accq += tt.y;
        acc[kp] = acc[kp] - tt;                            // da += -tt, j ascending
      }
      if (live) dqn[(size_t)j * D] = accq;
      qv = qnext;
    }
  }
  float* dan = da + (size_t)n * W2C * D + d;
  if (NW == 2) {                                             // wave 1 hands its partial da to wave 0 through LDS
    float2v* part = reinterpret_cast<float2v*>(reinterpret_cast<float*>(lds_lane) + 2 * JK);   // behind the table
    if (wv == 1) {
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) part[kp * 64 + lane] = acc[kp];
    }
    __syncthreads();
    if (wv == 1) return;
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) acc[kp] = acc[kp] + part[kp * 64 + lane];
  }
  if (live) {
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      dan[(size_t)(2 * kp) * D] = acc[kp].x;
      dan[(size_t)(2 * kp + 1) * D] = acc[kp].y;
    }
  }
}
static size_t cross_bwd_lane_lds(bool exact, int W1, int W2) {
  // fp32 mode: the table, then the second wave's partial da (W2 floats per lane)
  return (size_t)W1 * W2 * (exact ? 8 + 8 + 4 : 8) + (exact ? 0 : (size_t)W2 * 64 * sizeof(float)) + 16;
}
// the lane kernel pays when there are enough pairs to give every SIMD a wave and the grids are narrow
static bool cross_bwd_lane_ok(bool exact, int N, int W1, int W2, int D) {
  const bool width = W2 == 8 || W2 == 16 || W2 == 20 || W2 == 24 || W2 == 32 || W2 == 40 || W2 == 48;
  // reference rounding: 20 bytes of coefficients per (j,k); beyond ~16 KB per wave the table limits occupancy and
  // the tiled kernel wins (1517 x 40 x 40 x 50: 236 vs 183 us; 4096 x 20 x 20 x 50: 50 vs 92 us)
  return width && D <= 64 && N >= 512 && cross_bwd_lane_lds(exact, W1, W2) <= (exact ? 16 : 64) * 1024;
}
// cross_bwd_tiled_kernel (cross_grid.h), which the figures above compare this kernel with and which takes over where
// cross_bwd_lane_ok declines, walks d in chunks of kBwdDC.  Those figures (44 % of the second chunk idle at D = 50, the
// lane kernel up to D = 64 = two chunks) were taken at this width; a retune of the chunk has to revisit them.
namespace lane_figures {
constexpr int kBwdDC = 32;
static_assert(kBwdDC == ::mms::kBwdDC, "the lane kernel's thresholds were measured against 32-wide chunks of the tiled kernel");
}  // namespace lane_figures
// the first of cross_backward's three routes (cross_grid.h), for fp32 storage
template <>
inline bool launch_cross_bwd_lane<float>(int N, int W1, int W2, int D, const float* q, const float* a, const float* top,
                                         const float* top_diff, float* dq, float* da, bool exact, hipStream_t s) {
  if (!cross_bwd_lane_ok(exact, N, W1, W2, D)) return false;
  const size_t lds = cross_bwd_lane_lds(exact, W1, W2);
#define MMS_LANE(W2_)                                                                                     \
  case W2_:                                                                                               \
    if (exact)                                                                                            \
      hipLaunchKernelGGL((cross_bwd_lane_kernel<W2_, true>), dim3((unsigned)N), dim3(64), lds, s, q, a,   \
                         top, top_diff, dq, da, W1, D);                                                   \
    else                                                                                                  \
      hipLaunchKernelGGL((cross_bwd_lane_kernel<W2_, false, 2>), dim3((unsigned)N), dim3(128), lds, s, q, \
                         a, top, top_diff, dq, da, W1, D);                                                \
    break;
  switch (W2) { MMS_LANE(8) MMS_LANE(16) MMS_LANE(20) MMS_LANE(24) MMS_LANE(32) MMS_LANE(40) MMS_LANE(48) }
#undef MMS_LANE
  return true;
}

// =============================== entry points ===============================
// DESIGN.md 4.4b is the table this section is read against.  W1 == W2 == 1 tries simcross_rows.hip (Euclid) or
// simcross_rows_cosine.hip first.

static bool rows_geometry(int W1, int W2) { return W1 == 1 && W2 == 1; }

int simcross_elementwise_forward(int mode, int N, int W1, int W2, int D,
                                 const float* q, const float* a, float* top,
                                 float* norm0, float* norm1, hipStream_t s) {
  if (N == 0) return MMS_OK;
  const bool rows = rows_geometry(W1, W2);
  if (rows && mode == 0)
    launch_cosine_rows<true, false>(N, D, q, a, nullptr, top, norm0, norm1, nullptr, nullptr, s);
  else if (!(rows && launch_euclid_rows<true, false>(N, D, q, a, nullptr, nullptr, top, nullptr, nullptr, false, s)))
    cross_forward<float, false>(mode, N, W1, W2, D, q, a, top, norm0, norm1, s, kNoGather);
  return launch_status();
}

// top = SimCross(Embed(index_q), Embed(index_a)) for dist_mode 0 / 1; embed_bias = the Embed layers' bias blob
// (the driver's layers have one: `bias_term` stays at its default, do_trec_qa_clean.py:462-467) or null:
// embed_layer.cpp:135-152 followed by
// sim_cross_layer.cpp:96-139, with the gather done by SimCross's own loads.
int embed_simcross_forward(int mode, int N, int W1, int W2, int D, int K, const float* index_q,
                           const float* index_a, const float* weight, const float* embed_bias, float* top,
                           float* norm0, float* norm1, hipStream_t s) {
  if (N == 0) return MMS_OK;
  cross_forward<float, true>(mode, N, W1, W2, D, weight, weight, top, norm0, norm1, s,
                             CrossGather{index_q, index_a, K, embed_bias});
  return launch_status();
}

// `exact`: euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE, read once by the entry point
static int backward_with_mode(int mode, int N, int W1, int W2, int D, const float* q, const float* a,
                              const float* top, const float* top_diff, const float* norm0, const float* norm1,
                              float* dq, float* da, bool exact, hipStream_t s) {
  if (!rows_geometry(W1, W2))
    cross_backward<float>(mode, N, W1, W2, D, q, a, top, top_diff, norm0, norm1, dq, da, exact, s);
  else if (mode == 1)
    launch_euclid_rows<false, true>(N, D, q, a, top, top_diff, nullptr, dq, da, exact, s);
  else
    launch_cosine_rows<false, true>(N, D, q, a, top_diff, const_cast<float*>(top), const_cast<float*>(norm0),
                                    const_cast<float*>(norm1), dq, da, s);
  return launch_status();
}

int simcross_elementwise_backward(int mode, int N, int W1, int W2, int D,
                                  const float* q, const float* a, const float* top,
                                  const float* top_diff, const float* norm0,
                                  const float* norm1, float* dq, float* da,
                                  hipStream_t s) {
  if (N == 0) return MMS_OK;
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  return backward_with_mode(mode, N, W1, W2, D, q, a, top, top_diff, norm0, norm1, dq, da, exact, s);
}

// Forward+backward in one launch where the geometry allows (rows); otherwise
// the two passes back to back.
int simcross_elementwise_forward_backward(int mode, int N, int W1, int W2, int D,
                                          const float* q, const float* a,
                                          const float* top_diff, float* top,
                                          float* norm0, float* norm1, float* dq,
                                          float* da, hipStream_t s) {
  if (N == 0) return MMS_OK;
  const bool rows = rows_geometry(W1, W2);
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  if (rows && mode == 0) {
    launch_cosine_rows<true, true>(N, D, q, a, top_diff, top, norm0, norm1, dq, da, s);
    return launch_status();
  }
  if (rows && launch_euclid_rows<true, true>(N, D, q, a, nullptr, top_diff, top, dq, da, exact, s))
    return launch_status();
  int rc = simcross_elementwise_forward(mode, N, W1, W2, D, q, a, top, norm0, norm1, s);
  if (rc != MMS_OK) return rc;
  return backward_with_mode(mode, N, W1, W2, D, q, a, top, top_diff, norm0, norm1, dq, da, exact, s);
}

}  // namespace mms
