// csrc/bilinear.hip -- SimCross dist_mode 2, the learned-metric (bilinear W) layer on word grids, forward and
// backward, on the gfx950 matrix cores.
//
// Reference:
//   SimCross mode 2 fwd  sim_cross_layer.cpp:140-161   T[n,m] = Q_n W_m A_n^T (+ bias_m)
//   SimCross mode 2 bwd  sim_cross_layer.cpp:251-305   dW_m = sum_n Q_n^T dT_nm A_n (W.diff zeroed),
//                         dQ_n += dT_nm (W_m A_n^T)^T, dA_n += dT_nm^T (Q_n W_m), dbias += dT_n
// The reference issues 2 (fwd) / 6 (bwd) small cblas_sgemm calls per (pair,
// measure) on the host -- even in GPU mode (sim_cross_layer.cu:187-189,
// 240-242).  Here the contraction over the embedding dimension is regrouped so
// that all pairs share ONE large GEMM per weight matrix:
//   fwd:  tmp_m = Q_all W_m            (N*W1 x D x D)    then T = tmp A^T per pair
//   bwd:  U_nm = dT_nm A_n , V_nm = dT_nm^T Q_n           (small, per pair)
//         dQ_all = sum_m U_m W_m^T , dA_all = sum_m V_m W_m   (N*W x D x D)
//         dW_m   = Q_all^T U_m                              (D x D x N*W1, split-K)
// Algebraically identical to the reference's grouping; fp32 rounding differs
// (as it does between BLAS libraries), tests hold it to 1e-5.
//
// Three routes, all fp32 MFMA (fp32 in, fp32 accumulate): the fused per-pair / per-(pair, measure) kernels of this
// file for word grids that fit in LDS; the products above on the toolbox of gemm32.h for every other shape; and, at
// W1 = W2 = 1 with one measure, SimMatrix's launches (simmatrix.hip, through mms_internal.h), on whichever pipe
// mms_set_matrix_mode selects.  The dbias kernels (:301-304) are here because only this layer has a bias.
// Deterministic: split-K partial slabs are summed in a fixed order, no atomics.
#include <type_traits>

#include "euclid_math.h"
#include "gemm32.h"
#include "mms_internal.h"

namespace mms {

// ---- dbias[e] = dT[n][e] + dbias[e] for n ascending (sim_cross_layer.cpp:301-304: same order, bit-exact) ----
// The sum of one output is a dependent chain over n; what can be hidden is memory latency.  Three kernels, by the
// number of outputs per pair (per_n = M * W1 * W2; bilinear_backward picks).
// per_n == 1 (one scalar bias: SimCross bilinear at W1 = W2 = 1, one measure): dbias_chain_kernel would run on ONE
// lane that fetches its own operands, a memory round trip per 64 terms (300 us at 16384 pairs).  Here the whole
// wave fetches -- 64 consecutive terms per load, four loads ahead -- and the running sum, wave-uniform, takes them in
// n order through v_readlane: the dependent add is all that is left (~3 ns per term).
__global__ __launch_bounds__(64) void dbias_scalar_kernel(const float* __restrict__ top_diff, int N,
                                                          float* __restrict__ dbias) {
  const int lane = threadIdx.x;
  float s = dbias[0];
  float nx[4];
  auto fetch = [&](int base) {
#pragma unroll
    for (int u = 0; u < 4; ++u) nx[u] = top_diff[min(base + 64 * u + lane, N - 1)];
  };
  fetch(0);
  for (int base = 0; base < N; base += 256) {
    float cur[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = nx[u];
    if (base + 256 < N) fetch(base + 256);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int left = N - (base + 64 * u);
      if (left >= 64) {
#pragma unroll
        for (int l = 0; l < 64; ++l) s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur[u]), l)) + s;
      } else {
        for (int l = 0; l < left; ++l) s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur[u]), l)) + s;
      }
    }
  }
  if (lane == 0) dbias[0] = s;
}
// Many outputs (per_n > 256).  A workgroup owns 64 consecutive outputs: its four waves each fetch 16 of the next 64
// rows (coalesced 256-byte segments) into LDS while wave 0 adds the previous 64 rows in order.  (One thread per output
// with eight loads per round trip took 66 us at the 1517-candidate test split; this takes ~12.)
__global__ __launch_bounds__(256) void dbias_kernel(const float* __restrict__ top_diff, int N,
                                                    int per_n, float* __restrict__ dbias) {
  constexpr int CH = 64, RPW = CH / 4;
  __shared__ float buf[2][CH][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const bool ok = e < per_n;
  const int ec = ok ? e : per_n - 1;
  float s = dbias[ec];
  float r[RPW];
  auto fetch = [&](int c) {
#pragma unroll
    for (int u = 0; u < RPW; ++u) {
      const int n = c * CH + wave * RPW + u;
      r[u] = top_diff[(size_t)min(n, N - 1) * per_n + ec];
    }
  };
  const int nchunks = (N + CH - 1) / CH;
  fetch(0);
  for (int c = 0; c < nchunks; ++c) {
#pragma unroll
    for (int u = 0; u < RPW; ++u) buf[c & 1][wave * RPW + u][lane] = r[u];
    __syncthreads();                             // chunk c complete in LDS; adds of chunk c-1 finished
    if (c + 1 < nchunks) fetch(c + 1);
    if (wave == 0) {
      const int cnt = min(CH, N - c * CH);
      for (int u = 0; u < cnt; ++u) s = buf[c & 1][u][lane] + s;
    }
  }
  if (wave == 0 && ok) dbias[e] = s;
}

// Few outputs (sentence-vector geometry: per_n = M): the work IS the N-long dependent add chain of each
// output, and rows of consecutive n share cache lines.  One wave, 64 loads in flight while the previous 64
// values are added; no LDS, no barrier in the chain's way.
__global__ __launch_bounds__(64) void dbias_chain_kernel(const float* __restrict__ top_diff, int N,
                                                         int per_n, float* __restrict__ dbias) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= per_n) return;
  float s = dbias[e];
  constexpr int B = 64;
  float cur[B], nxt[B];
  const int full = N / B;
  if (full > 0) {
#pragma unroll
    for (int u = 0; u < B; ++u) cur[u] = top_diff[(size_t)u * per_n + e];
  }
  for (int b = 0; b < full; ++b) {
    if (b + 1 < full) {
#pragma unroll
      for (int u = 0; u < B; ++u) nxt[u] = top_diff[(size_t)((b + 1) * B + u) * per_n + e];
    }
#pragma unroll
    for (int u = 0; u < B; ++u) s = cur[u] + s;
#pragma unroll
    for (int u = 0; u < B; ++u) cur[u] = nxt[u];
  }
  for (int n = full * B; n < N; ++n) s = top_diff[(size_t)n * per_n + e] + s;
  dbias[e] = s;
}

// ------------------------------ workspace layout ----------------------------
// the word grids the fused per-(pair, measure) kernels stage whole in LDS (bilinear_pair_bwd_kernel,
// bilinear_pairm_fwd_kernel): image row stride, most words per sentence, widest embedding
constexpr int FB_LS = 68, FB_W = 48, FB_D = 64;
// does the fused per-pair backward (and its forward twin) take this shape?  Sizes the workspace AND picks the kernel.
static bool pair_bwd_eligible(int N, int W1, int W2, int D, int M) {
  return W1 <= FB_W && W2 <= FB_W && D <= FB_D && W1 * W2 > 1 && N <= 256 && (long long)N * M <= 65535;
}
// The sentence-vector geometry with ONE measure (W1 = W2 = 1, M = 1: BASELINE cfg 3 written as a SimCross layer) IS
// SimMatrix's arithmetic -- T_n = q_n^T W a_n (+ bias), dW = sum_n dT_n q_n a_n^T, dq_n = dT_n W a_n,
// da_n = dT_n W^T q_n -- so it takes SimMatrix's panel-GEMM launches (row dot and row scale as epilogues) instead
// of the generic GEMM + rowdot / rowscale launches: 45 + 136 us -> the SimMatrix figures (recomputing Q.W).
static bool bilinear_as_simmatrix(int W1, int W2, int M) { return W1 == 1 && W2 == 1 && M == 1; }

struct BilinearWs {
  size_t u_off, v_off, part_off, mpart_off, mpart2_off, total;
  size_t sm_off;                 // bilinear_as_simmatrix: [Q.W, N x D] at 0, SimMatrix's own workspace from here
  int ksplit, kchunk;
};
static BilinearWs bilinear_ws(int N, int W1, int W2, int D, int M) {
  BilinearWs w{};
  const size_t u = (size_t)M * N * W1 * D, v = (size_t)M * N * W2 * D;
  w.ksplit = pick_ksplit(D, D, N * W1, &w.kchunk, M);
  w.u_off = 0;
  w.v_off = round_up(u * sizeof(float), 256);
  w.part_off = w.v_off + round_up(v * sizeof(float), 256);
  // split-K slabs of dW -- or, when the fused per-pair backward runs, one D x D partial per (pair, measure)
  const size_t slabs = pair_bwd_eligible(N, W1, W2, D, M) && N > w.ksplit ? (size_t)N : (size_t)w.ksplit;
  w.mpart_off = w.part_off + round_up(slabs * M * D * D * sizeof(float), 256);
  // per-measure partial products of dQ and of dA (M > 1 only): [M][N*W1][D], [M][N*W2][D]
  w.mpart2_off = w.mpart_off + (M > 1 ? round_up(u * sizeof(float), 256) : 0);
  w.total = w.mpart2_off + (M > 1 ? round_up(v * sizeof(float), 256) : 0);
  if (bilinear_as_simmatrix(W1, W2, M)) {
    w.sm_off = round_up((size_t)N * D * sizeof(float), 256);
    const size_t sm = w.sm_off + simmatrix_workspace_bytes(N, D, D);
    if (sm > w.total) w.total = sm;
  }
  return w;
}
size_t bilinear_workspace_bytes(int N, int W1, int W2, int D, int M) {
  return bilinear_ws(N, W1, W2, D, M).total;
}

// ---- fused forward for word grids (the driver's 40 x 40 x Dw geometry) ---------------------------
// One workgroup per pair n: T[n,m] = (Q_n W_m) A_n^T + bias_m for every measure m, with Q_n W_m kept in
// LDS -- the (M, N*W1, D) intermediate of the two-GEMM formulation (written to and read back from HBM:
// 2 x 48 MB at the 1517-candidate test split) never exists, and the forward is ONE launch.
//   * q_n and a_n are staged once as zero-padded images, row stride 68 floats (rows 4 banks apart: the
//     16 rows x 4 k of an MFMA operand read hit 64 distinct banks);
//   * work items (measure m, 16-row tile of Q) are dealt to the four waves.  An item runs
//     stage 1  tmp (16 x D)  = Q rows x W_m : ceil(D/16) accumulators, B operand W_m[k][j] read straight
//              from global memory (M*D*D floats: L1/L2-resident), one 4-byte load per MFMA;
//     stage 2  T   (16 x W2) = tmp x A_n^T  : tmp goes through the wave's own LDS slice to become an A
//              operand (k-major per lane), B operand from the a image;
//   * v_mfma_f32_16x16x4_f32: W = 40 fills 40/48 of the tiles (32x32 tiles: 40/64).
// Eligible for W1, W2 <= 48 and D <= 64; anything else takes the two batched GEMMs below.
constexpr int PF_LS = 68, PF_ROWS = 48, PF_TD = 4;
typedef float v4f __attribute__((ext_vector_type(4)));

// Embed fused into the staging loads (the mode network_v4 scores with): with g.iq != nullptr,
// q and a are both the embedding TABLE (K x D) and row r of pair n is table row g.iq[n*W1 + r] (g.ia likewise):
// the (N, W, D) blobs the Embed layers would write and SimCross read back never exist.
struct PairGather {
  const float* iq;
  const float* ia;
  int K;
  const float* bias;     // the Embed layer's bias (D floats) or nullptr: row value = bias[d] + table[id][d]
};
__device__ __forceinline__ int pair_gather_id(float v, int K) {   // as mms_embed_forward_f32 clamps
  const int i = (int)v;
  return i < 0 ? 0 : (i >= K ? K - 1 : i);
}

template <int KS>                                  // k steps of 4: 13 covers D <= 52 (the driver's 50), 16 D <= 64
__global__ __launch_bounds__(256) void bilinear_pair_fwd_kernel(
    int N, int W1, int W2, int D, int M, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ top,
    PairGather g = PairGather{nullptr, nullptr, 0, nullptr}) {
  __shared__ float qs[PF_ROWS * PF_LS];
  __shared__ float as[PF_ROWS * PF_LS];
  __shared__ float ts[4][16 * PF_LS];
  const int n = blockIdx.x;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;
  const int li = lane & 15, lk = lane >> 4;
  const int ti_n = (W1 + 15) / 16;
  // Items are dealt in contiguous runs (m-major), so a wave mostly stays on one measure and keeps that
  // measure's B operands -- W_m[k][j] for its lane, all k steps -- in registers: they are fetched once,
  // all loads in flight together (a load per MFMA inside the k loop costs a memory round trip per step).
  const int items = M * ti_n, per = (items + 3) / 4;
  float wf[KS][PF_TD];
  auto fetch_w = [&](int m) {
    const float* Wm = W + (size_t)m * D * D;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + lk;
#pragma unroll
      for (int d = 0; d < PF_TD; ++d) wf[ks][d] = Wm[(size_t)min(k, D - 1) * D + min(16 * d + li, D - 1)];
    }
  };
  auto mask_w = [&]() {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int d = 0; d < PF_TD; ++d)
        if (!(4 * ks + lk < D && 16 * d + li < D)) wf[ks][d] = 0.f;
  };
  int have_m = -1;
  if (wave * per < items) {                        // the first measure's operands: in flight behind the staging
    have_m = (wave * per) / ti_n;
    fetch_w(have_m);
  }
  // zero-padded images: every load issued (clamped, unconditional) before the first LDS write
  constexpr int NE = (PF_ROWS * PF_LS + 255) / 256;
  float vq[NE], va[NE];
  if (g.iq) {                                      // ids first (all in flight), then the table rows
    float fq[NE], fa[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int r = (256 * u + t) / PF_LS;
      fq[u] = g.iq[(size_t)n * W1 + min(r, W1 - 1)];
      fa[u] = g.ia[(size_t)n * W2 + min(r, W2 - 1)];
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = 256 * u + t;
      const int c = e - (e / PF_LS) * PF_LS;
      vq[u] = q[(size_t)pair_gather_id(fq[u], g.K) * D + min(c, D - 1)];
      va[u] = a[(size_t)pair_gather_id(fa[u], g.K) * D + min(c, D - 1)];
      if (g.bias) { const float bv = g.bias[min(c, D - 1)]; vq[u] = bv + vq[u]; va[u] = bv + va[u]; }
    }
  } else {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = 256 * u + t;
      const int r = e / PF_LS, c = e - r * PF_LS;
      vq[u] = qn[(size_t)min(r, W1 - 1) * D + min(c, D - 1)];
      va[u] = an[(size_t)min(r, W2 - 1) * D + min(c, D - 1)];
    }
  }
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = 256 * u + t;
    const int r = e / PF_LS, c = e - r * PF_LS;
    if (e < PF_ROWS * PF_LS) {
      qs[e] = (r < W1 && c < D) ? vq[u] : 0.f;
      as[e] = (r < W2 && c < D) ? va[u] : 0.f;
    }
  }
  __syncthreads();
  if (have_m >= 0) mask_w();
  float* tw = ts[wave];
  for (int item = wave * per; item < min(items, (wave + 1) * per); ++item) {
    const int m = item / ti_n, ti = item - m * ti_n;
    if (m != have_m) {
      fetch_w(m);
      mask_w();
      have_m = m;
    }
    // this item's bias values: requested now, used after the two stages (a load in the epilogue would
    // expose a memory round trip per item)
    const float* bm = bias ? bias + (size_t)m * W1 * W2 : nullptr;
    float bv[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = min(16 * ti + 4 * lk + r, W1 - 1), col = min(16 * c + li, W2 - 1);
        bv[c][r] = bm ? bm[row * W2 + col] : 0.f;
      }
    // stage 1: tmp[16 x D] = Q[16 rows of tile ti] . W_m
    v4f acc1[PF_TD];
#pragma unroll
    for (int d = 0; d < PF_TD; ++d) acc1[d] = (v4f){0.f, 0.f, 0.f, 0.f};
    // padded tiles are computed too (their operands are zero): no branch between MFMAs
    float a1[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a1[ks] = qs[(16 * ti + li) * PF_LS + 4 * ks + lk];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int d = 0; d < PF_TD; ++d)
        acc1[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ks], wf[ks][d], acc1[d], 0, 0, 0);
    }
    // C layout: col = lane & 15, row = 4 * (lane >> 4) + reg  ->  the wave's LDS slice, row-major
#pragma unroll
    for (int d = 0; d < PF_TD; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) tw[(4 * lk + r) * PF_LS + 16 * d + li] = acc1[d][r];
    wave_lds_sync();                               // (euclid_math.h) this wave's LDS writes, before its own reads
    // stage 2: T[16 x W2] = tmp . A_n^T   (B[k][j] = a[j][k])
    v4f acc2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc2[c] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + lk;
      const float av = tw[li * PF_LS + k];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        acc2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, as[(16 * c + li) * PF_LS + k], acc2[c], 0, 0, 0);
    }
    wave_lds_sync();                               // tw is rewritten by this wave's next item
    float* tn = top + ((size_t)n * M + m) * W1 * W2;
#pragma unroll
    for (int c = 0; c < 3; ++c)                    // in registers before the first store (else: vmcnt(0) behind each)
      asm volatile("" : "+v"(bv[c][0]), "+v"(bv[c][1]), "+v"(bv[c][2]), "+v"(bv[c][3]));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int col = 16 * c + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + 4 * lk + r;
        if (row < W1 && col < W2) {
          float v = acc2[c][r];
          if (bm) v = bv[c][r] + v;                // the addend form of the GEMM epilogue (:156-158)
          tn[row * W2 + col] = v;
        }
      }
    }
  }
}


// ---- fused backward for word grids at TRAINING batch sizes (the driver's 50 x 40 x 40 x Dw) -----------------
// At a batch of 50 pairs every product of the bilinear backward is a 4-8 us launch at the latency floor (six
// launches, 27 us).  Here ONE launch runs all five products of a (pair, measure): a workgroup stages q_n, a_n,
// dT_nm and W_m as zero-padded LDS images (row stride 68, as in bilinear_pair_fwd_kernel), then
//   phase 1   U = dT A (W1 x D), V = dT^T Q (W2 x D)              -> LDS
//   phase 2   dQ_nm = U W_m^T, dA_nm = V W_m, dW_nm = Q^T U        -> per-(n, m) partials in the workspace
// on v_mfma_f32_16x16x4_f32, the 16 x 16 output tiles of a phase dealt round-robin to the four waves.  The sums
// the reference takes in place -- dQ_n over m (sim_cross_layer.cpp:291-294), dA_n over m (:296-299), dW_m over n
// (:286-289) -- are taken afterwards by ONE grouped reduction launch in the same ascending orders.
// (FB_LS, FB_W, FB_D: with the workspace layout above, which they size)
// KSW / KSD: k-steps of 4 over a word axis / the embedding axis, fixed at compile time so that a tile's operand
// reads are ALL issued before its MFMAs (a rolled read-read-MFMA loop paid an LDS round trip per k-step: 17.6 us);
// the images are zero beyond W and D, so steps past the real extent add exact zeros.
template <int KSW, int KSD>
__global__ __launch_bounds__(512) void bilinear_pair_bwd_kernel(
    int N, int W1, int W2, int D, int M, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ top_diff, float* __restrict__ mq,
    float* __restrict__ ma, float* __restrict__ wpart) {
  __shared__ float qs[FB_W * FB_LS], as[FB_W * FB_LS], ts[FB_W * FB_LS], ws[FB_D * FB_LS];
  __shared__ float us[FB_W * FB_LS], vs[FB_W * FB_LS];
  const int n = blockIdx.x / M, m = blockIdx.x - n * M;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;
  const float* Wm = W + (size_t)m * D * D;
  const float* dT = top_diff + ((size_t)n * M + m) * W1 * W2;
  // zero-padded images: every load issued (clamped, unconditional) before the first LDS write
  constexpr int NT = 512, NWV = NT / 64;
  constexpr int NE = (FB_W * FB_LS + NT - 1) / NT, NEW = (FB_D * FB_LS + NT - 1) / NT;
  {
    float vq[NE], va[NE], vt[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vq[u] = qn[(size_t)min(row, W1 - 1) * D + min(c, D - 1)];
      va[u] = an[(size_t)min(row, W2 - 1) * D + min(c, D - 1)];
      vt[u] = dT[(size_t)min(row, W1 - 1) * W2 + min(c, W2 - 1)];
    }
    // W_m's image is requested HERE, with the other three: behind the first LDS writes it was a second, exposed
    // memory round trip in a workgroup whose whole life is ~10 us
    float vw[NEW];
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vw[u] = Wm[(size_t)min(row, D - 1) * D + min(c, D - 1)];
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      if (e < FB_W * FB_LS) {
        qs[e] = (row < W1 && c < D) ? vq[u] : 0.f;
        as[e] = (row < W2 && c < D) ? va[u] : 0.f;
        ts[e] = (row < W1 && c < W2) ? vt[u] : 0.f;
        us[e] = 0.f;                                   // rows / columns no tile writes must read as zero
        vs[e] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      if (e < FB_D * FB_LS) ws[e] = (row < D && c < D) ? vw[u] : 0.f;
    }
  }
  __syncthreads();
  const int tw1 = (W1 + 15) >> 4, tw2 = (W2 + 15) >> 4, td = (D + 15) >> 4;
  // one 16 x 16 tile: C(i0 + 4g + j, j0 + r) = sum_k A(i0 + r', k) B(k, j0 + r); A / B given as (base, row stride,
  // k stride): element (x, k) of an operand lives at base[x * xs + k * ks]
  auto tile = [&](auto nks_tag, const float* A, int axs, int aks, const float* B, int bxs, int bks, int i0, int j0) {
    constexpr int NKS = decltype(nks_tag)::value;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    const float* ap = A + (i0 + r) * axs + g * aks;
    const float* bp = B + (j0 + r) * bxs + g * bks;
    float av[NKS], bv[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) { av[ks] = ap[4 * ks * aks]; bv[ks] = bp[4 * ks * bks]; }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], acc, 0, 0, 0);
    return acc;
  };
  const std::integral_constant<int, KSW> kw{};
  const std::integral_constant<int, KSD> kd{};
  auto put_lds = [&](float* dst, int i0, int j0, const v4f& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[(i0 + 4 * g + j) * FB_LS + j0 + r] = acc[j];
  };
  // phase 1: U (tw1 x td tiles) then V (tw2 x td tiles)
  const int nU = tw1 * td, nV = tw2 * td;
  for (int it = wave; it < nU + nV; it += NWV) {
    if (it < nU) {
      const int ti = it / td, tj = it - ti * td;
      // U[j][d] = sum_k dT[j][k] A[k][d]:  A-operand (row j, k) = ts[j*LS + k];  B-operand (k, col d) = as[k*LS + d]
      put_lds(us, 16 * ti, 16 * tj, tile(kw, ts, FB_LS, 1, as, 1, FB_LS, 16 * ti, 16 * tj));
    } else {
      const int e = it - nU, ti = e / td, tj = e - ti * td;
      // V[k][d] = sum_j dT[j][k] Q[j][d]:  A-operand (row k, kk = j) = ts[j*LS + k];  B-operand (j, col d) = qs[j*LS + d]
      put_lds(vs, 16 * ti, 16 * tj, tile(kw, ts, 1, FB_LS, qs, 1, FB_LS, 16 * ti, 16 * tj));
    }
  }
  __syncthreads();
  // phase 2
  const int nQ = tw1 * td, nA = tw2 * td, nW = td * td;
  float* mqn = mq + ((size_t)m * N + n) * W1 * D;       // [M][N*W1][D]
  float* man = ma + ((size_t)m * N + n) * W2 * D;       // [M][N*W2][D]
  float* wpn = wpart + ((size_t)n * M + m) * D * D;     // [N][M][D][D]
  auto put_global = [&](float* dst, int ld, int rows, int cols, int i0, int j0, const v4f& acc) {
    const int col = j0 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = i0 + 4 * g + j;
      if (row < rows && col < cols) dst[(size_t)row * ld + col] = acc[j];
    }
  };
  for (int it = wave; it < nQ + nA + nW; it += NWV) {
    if (it < nQ) {
      const int ti = it / td, tj = it - ti * td;
      // dQ[j][d'] = sum_d U[j][d] W[d'][d]:  A (row j, k = d) = us[j*LS + d];  B (k = d, col d') = ws[d'*LS + d]
      put_global(mqn, D, W1, D, 16 * ti, 16 * tj, tile(kd, us, FB_LS, 1, ws, FB_LS, 1, 16 * ti, 16 * tj));
    } else if (it < nQ + nA) {
      const int e = it - nQ, ti = e / td, tj = e - ti * td;
      // dA[k][d'] = sum_d V[k][d] W[d][d']:  A (row k, kk = d) = vs[k*LS + d];  B (d, col d') = ws[d*LS + d']
      put_global(man, D, W2, D, 16 * ti, 16 * tj, tile(kd, vs, FB_LS, 1, ws, 1, FB_LS, 16 * ti, 16 * tj));
    } else {
      const int e = it - nQ - nA, ti = e / td, tj = e - ti * td;
      // dW[d][d'] = sum_j Q[j][d] U[j][d']:  A (row d, k = j) = qs[j*LS + d];  B (j, col d') = us[j*LS + d']
      put_global(wpn, D, D, D, 16 * ti, 16 * tj, tile(kw, qs, 1, FB_LS, us, 1, FB_LS, 16 * ti, 16 * tj));
    }
  }
}

// The forward twin of bilinear_pair_bwd_kernel for training batches: a workgroup per (pair, measure) stages q_n,
// a_n and W_m, forms tmp = Q_n W_m in LDS and T_nm = tmp A_n^T (+ bias_m) straight to `top` -- one launch instead
// of two batched GEMMs with a (M, N*W1, D) intermediate in HBM.  (bilinear_pair_fwd_kernel, one workgroup per
// PAIR with W_m operands held in registers, stays the choice for evaluation batches of hundreds of pairs.)
template <int KSD>
__global__ __launch_bounds__(512) void bilinear_pairm_fwd_kernel(
    int N, int W1, int W2, int D, int M, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ top,
    PairGather gth = PairGather{nullptr, nullptr, 0, nullptr}) {
  __shared__ float qs[FB_W * FB_LS], as[FB_W * FB_LS], ws[FB_D * FB_LS], ps[FB_W * FB_LS];
  constexpr int NT = 512, NWV = NT / 64;
  const int n = blockIdx.x / M, m = blockIdx.x - n * M;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;
  const float* Wm = W + (size_t)m * D * D;
  constexpr int NE = (FB_W * FB_LS + NT - 1) / NT, NEW = (FB_D * FB_LS + NT - 1) / NT;
  {
    float vq[NE], va[NE], vw[NEW];
    if (gth.iq) {                                  // Embed fused in: ids first, then the table rows
      float fq[NE], fa[NE];
#pragma unroll
      for (int u = 0; u < NE; ++u) {
        const int row = (NT * u + t) / FB_LS;
        fq[u] = gth.iq[(size_t)n * W1 + min(row, W1 - 1)];
        fa[u] = gth.ia[(size_t)n * W2 + min(row, W2 - 1)];
      }
#pragma unroll
      for (int u = 0; u < NE; ++u) {
        const int e = NT * u + t, c = e - (e / FB_LS) * FB_LS;
        vq[u] = q[(size_t)pair_gather_id(fq[u], gth.K) * D + min(c, D - 1)];
        va[u] = a[(size_t)pair_gather_id(fa[u], gth.K) * D + min(c, D - 1)];
        if (gth.bias) { const float bv = gth.bias[min(c, D - 1)]; vq[u] = bv + vq[u]; va[u] = bv + va[u]; }
      }
    } else {
#pragma unroll
      for (int u = 0; u < NE; ++u) {
        const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
        vq[u] = qn[(size_t)min(row, W1 - 1) * D + min(c, D - 1)];
        va[u] = an[(size_t)min(row, W2 - 1) * D + min(c, D - 1)];
      }
    }
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vw[u] = Wm[(size_t)min(row, D - 1) * D + min(c, D - 1)];
    }
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      if (e < FB_W * FB_LS) {
        qs[e] = (row < W1 && c < D) ? vq[u] : 0.f;
        as[e] = (row < W2 && c < D) ? va[u] : 0.f;
        ps[e] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      if (e < FB_D * FB_LS) ws[e] = (row < D && c < D) ? vw[u] : 0.f;
    }
  }
  __syncthreads();
  const int tw1 = (W1 + 15) >> 4, tw2 = (W2 + 15) >> 4, td = (D + 15) >> 4;
  auto tile = [&](const float* A, int axs, int aks, const float* B, int bxs, int bks, int i0, int j0) {
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    const float* ap = A + (i0 + r) * axs + g * aks;
    const float* bp = B + (j0 + r) * bxs + g * bks;
    float av[KSD], bv[KSD];
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) { av[ks] = ap[4 * ks * aks]; bv[ks] = bp[4 * ks * bks]; }
#pragma unroll
    for (int ks = 0; ks < KSD; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv[ks], acc, 0, 0, 0);
    return acc;
  };
  // tmp[j][d'] = sum_d Q[j][d] W[d][d']:  A (row j, k = d) = qs[j*LS + d];  B (d, col d') = ws[d*LS + d']
  for (int it = wave; it < tw1 * td; it += NWV) {
    const int ti = it / td, tj = it - ti * td;
    const v4f acc = tile(qs, FB_LS, 1, ws, 1, FB_LS, 16 * ti, 16 * tj);
#pragma unroll
    for (int j = 0; j < 4; ++j) ps[(16 * ti + 4 * g + j) * FB_LS + 16 * tj + r] = acc[j];
  }
  __syncthreads();
  // T[j][k] = sum_d' tmp[j][d'] A[k][d'] (+ bias[j][k]):  A (row j, k = d') = ps[j*LS + d'];  B (d', col k) = as[k*LS + d']
  float* tn = top + ((size_t)n * M + m) * W1 * W2;
  const float* bm = bias ? bias + (size_t)m * W1 * W2 : nullptr;
  for (int it = wave; it < tw1 * tw2; it += NWV) {
    const int ti = it / tw2, tj = it - ti * tw2;
    const int col = 16 * tj + r;
    float bvv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bvv[j] = bm ? bm[min(16 * ti + 4 * g + j, W1 - 1) * W2 + min(col, W2 - 1)] : 0.f;
    const v4f acc = tile(ps, FB_LS, 1, as, FB_LS, 1, 16 * ti, 16 * tj);
    asm volatile("" : "+v"(bvv[0]), "+v"(bvv[1]), "+v"(bvv[2]), "+v"(bvv[3]));   // in registers before the first store (else: vmcnt(0) behind it)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 16 * ti + 4 * g + j;
      if (row < W1 && col < W2) tn[row * W2 + col] = bm ? bvv[j] + acc[j] : acc[j];   // the addend form (:156-158)
    }
  }
}

// The fused word-grid forward, when one of its two kernels takes the shape: one workgroup per pair for large batches
// (evaluation: the 1517 TREC-QA test candidates, 89 -> 59 us), one per (pair, measure) for training batches -- at 50
// pairs the per-pair form and the two small GEMMs both sit at the launch floor.  `g`: Embed fused in (q = a = the table).
// Returns whether it launched.
static bool pair_fwd_launch(int N, int W1, int W2, int D, int M, const float* q, const float* a, const float* W,
                            const float* bias, float* top, hipStream_t s,
                            const PairGather g = PairGather{nullptr, nullptr, 0, nullptr}) {
  if (W1 <= PF_ROWS && W2 <= PF_ROWS && D <= 16 * PF_TD && W1 * W2 > 1 && N >= 512) {
    if (D <= 52)
      hipLaunchKernelGGL(bilinear_pair_fwd_kernel<13>, dim3(N), dim3(256), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    else
      hipLaunchKernelGGL(bilinear_pair_fwd_kernel<16>, dim3(N), dim3(256), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    return true;
  }
  if (pair_bwd_eligible(N, W1, W2, D, M)) {
    if (D <= 52)
      hipLaunchKernelGGL((bilinear_pairm_fwd_kernel<13>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    else
      hipLaunchKernelGGL((bilinear_pairm_fwd_kernel<16>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    return true;
  }
  return false;
}

// top = SimCross_bilinear(Embed(index_q), Embed(index_a)) in ONE launch, for the word-grid geometries the two
// fused forward kernels cover (W1, W2 <= 48, D <= 64): embed_layer.cpp:135-152 (embed_bias: the Embed layers' bias blob or null) followed by
// sim_cross_layer.cpp:140-161, the gather done by the staging loads.  Same kernels, same operand values: the
// bits of mms_embed_forward_f32 x2 followed by mms_simcross_forward_f32.  Other geometries: MMS_ERR_UNSUPPORTED.
int embed_bilinear_forward(int N, int W1, int W2, int D, int M, int K, const float* index_q,
                           const float* index_a, const float* table, const float* embed_bias, const float* W,
                           const float* bias, float* top, hipStream_t s) {
  if (N == 0) return MMS_OK;
  if (!pair_fwd_launch(N, W1, W2, D, M, table, table, W, bias, top, s, PairGather{index_q, index_a, K, embed_bias}))
    return MMS_ERR_UNSUPPORTED;
  return launch_status();
}

int bilinear_forward(int N, int W1, int W2, int D, int M, const float* q, const float* a,
                     const float* W, const float* bias, float* top, void* ws, size_t ws_bytes,
                     hipStream_t s) {
  const BilinearWs lay = bilinear_ws(N, W1, W2, D, M);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  if (bilinear_as_simmatrix(W1, W2, M))
    return simmatrix_forward(N, D, D, q, a, W, top, static_cast<float*>(ws), s, bias, static_cast<char*>(ws) + lay.sm_off,
                             ws_bytes - lay.sm_off);
  if (pair_fwd_launch(N, W1, W2, D, M, q, a, W, bias, top, s)) return launch_status();
  float* tmp = reinterpret_cast<float*>(static_cast<char*>(ws) + lay.u_off);
  const long long R = (long long)N * W1;
  // tmp[m] = Q_all W_m   (:148-149, batched over all pairs)
  {
    GemmArgs g = gemm_args((int)R, D, D, q, D, 1, W, D, 1, tmp, D);
    g.nb1 = M; g.b_b1 = (long long)D * D; g.c_b1 = R * D;
    gemm_launch(g, 1, s);
  }
  if (W1 == 1 && W2 == 1) {
    // T[n,m] = tmp[m][n] . a[n] (+ bias[m])   (:151-158)
    for (int m = 0; m < M; ++m) rowdot_launch(tmp + (size_t)m * R * D, a, bias ? bias + m : nullptr, top + m, N, D, M, s);
  } else {
    // T[n,m] = tmp[m][n] A_n^T (+ bias_m), batched over (n, m)
    GemmArgs g = gemm_args(W1, W2, D, tmp, D, 1, a, 1, D, top, W2);
    g.nb1 = M;
    g.a_b0 = (long long)W1 * D; g.a_b1 = R * D;
    g.b_b0 = (long long)W2 * D; g.b_b1 = 0;
    g.c_b0 = (long long)M * W1 * W2; g.c_b1 = (long long)W1 * W2;
    g.addend = bias; g.ad_b1 = (long long)W1 * W2;
    gemm_launch(g, N, s);
  }
  return launch_status();
}

int bilinear_backward(int N, int W1, int W2, int D, int M, const float* q, const float* a,
                      const float* W, int bias_term, const float* top_diff, float* dq, float* da,
                      float* dW, float* dbias, void* ws, size_t ws_bytes, hipStream_t s) {
  const BilinearWs lay = bilinear_ws(N, W1, W2, D, M);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(ws);
  float* U = reinterpret_cast<float*>(base + lay.u_off);     // [M][N*W1][D]
  float* V = reinterpret_cast<float*>(base + lay.v_off);     // [M][N*W2][D]
  float* part = reinterpret_cast<float*>(base + lay.part_off);
  const long long R1 = (long long)N * W1, R2 = (long long)N * W2;

  if (pair_bwd_eligible(N, W1, W2, D, M)) {
    // one launch for the five products of every (pair, measure), one grouped launch for the three sums
    float* mq = M > 1 ? reinterpret_cast<float*>(base + lay.mpart_off) : dq;
    float* ma = M > 1 ? reinterpret_cast<float*>(base + lay.mpart2_off) : da;
    if (W1 <= 40 && W2 <= 40 && D <= 52)           // the driver's geometry: 10 / 13 k-steps
      hipLaunchKernelGGL((bilinear_pair_bwd_kernel<10, 13>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W,
                         top_diff, mq, ma, part);
    else
      hipLaunchKernelGGL((bilinear_pair_bwd_kernel<12, 16>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W,
                         top_diff, mq, ma, part);
    ReduceGroup rg{};
    if (M > 1) {
      reduce_group_add(rg, mq, dq, R1 * D, M);
      reduce_group_add(rg, ma, da, R2 * D, M);
    }
    reduce_group_add(rg, part, dW, (long long)M * D * D, N);      // W.diff is overwritten (:256), pairs summed ascending
    // bias.diff += dT_n, n ascending (:301-304): top_diff IS the [pair][M*W1*W2] stack of addends
    if (bias_term) reduce_group_add(rg, top_diff, dbias, (long long)M * W1 * W2, N, 1);
    reduce_group_launch(rg, s);
    return launch_status();
  }
  // dbias first: it depends on nothing the products write
  if (bias_term) {
    const int per_n = M * W1 * W2;
    if (per_n == 1)
      hipLaunchKernelGGL(dbias_scalar_kernel, dim3(1), dim3(64), 0, s, top_diff, N, dbias);
    else if (per_n <= 256)
      hipLaunchKernelGGL(dbias_chain_kernel, dim3((per_n + 63) / 64), dim3(64), 0, s, top_diff, N, per_n,
                         dbias);
    else
      hipLaunchKernelGGL(dbias_kernel, dim3((per_n + 63) / 64), dim3(256), 0, s, top_diff, N, per_n,
                         dbias);
  }
  if (bilinear_as_simmatrix(W1, W2, M)) {
    // W.diff is OVERWRITTEN by SimCross (:256) where SimMatrix accumulates: start from zero (0 + x = x exactly)
    if (hipMemsetAsync(dW, 0, sizeof(float) * (size_t)D * D, s) != hipSuccess) return MMS_ERR_LAUNCH;
    return simmatrix_backward(N, D, D, q, a, W, top_diff, 1, 1, 1, dq, da, dW, nullptr, base + lay.sm_off,
                              ws_bytes - lay.sm_off, s);
  }
  // U_nm = dT_nm A_n  (W1 x D x W2) ;  V_nm = dT_nm^T Q_n  (W2 x D x W1)
  GemmArgs guv[2];
  guv[0] = gemm_args(W1, D, W2, top_diff, W2, 1, a, D, 1, U, D);
  guv[0].nb1 = M;
  guv[0].a_b0 = (long long)M * W1 * W2; guv[0].a_b1 = (long long)W1 * W2;
  guv[0].b_b0 = (long long)W2 * D; guv[0].b_b1 = 0;
  guv[0].c_b0 = (long long)W1 * D; guv[0].c_b1 = R1 * D;
  guv[1] = gemm_args(W2, D, W1, top_diff, 1, W2, q, D, 1, V, D);
  guv[1].nb1 = M;
  guv[1].a_b0 = (long long)M * W1 * W2; guv[1].a_b1 = (long long)W1 * W2;
  guv[1].b_b0 = (long long)W1 * D; guv[1].b_b1 = 0;
  guv[1].c_b0 = (long long)W2 * D; guv[1].c_b1 = R2 * D;
  const int nb[2] = {N, N};
  if (!gemm_launch_group(guv, nb, 2, s)) {      // small batches: U and V in one launch
    gemm_launch(guv[0], N, s);
    gemm_launch(guv[1], N, s);
  }
  // dQ_all = sum_m U_m W_m^T ; dA_all = sum_m V_m W_m   (:291-299; m = 0 overwrites, which also realises
  // the unconditional zeroing of :176-177) ; dW_m = Q_all^T U_m  (:286-289), K = N*W1 split across
  // workgroups; W.diff is overwritten because the reference zeroes it first (:256).  The three products
  // are independent: one grouped launch when they are small, then one grouped reduction.
  GemmArgs g3[3];
  const int one3[3] = {1, 1, 1};
  const long long nW = (long long)M * D * D;
  g3[2] = gemm_args(D, D, (int)R1, q, 1, D, U, D, 1, part, D);
  g3[2].nb1 = M; g3[2].b_b1 = R1 * D; g3[2].c_b1 = (long long)D * D;
  g3[2].ksplit = lay.ksplit; g3[2].kchunk = lay.kchunk; g3[2].c_ks = nW;
  if (M == 1) {
    g3[0] = gemm_args((int)R1, D, D, U, D, 1, W, 1, D, dq, D);
    g3[1] = gemm_args((int)R2, D, D, V, D, 1, W, D, 1, da, D);
    if (!gemm_launch_group(g3, one3, 3, s)) {
      gemm_launch(g3[0], 1, s);
      gemm_launch(g3[1], 1, s);
      gemm_launch(g3[2], 1, s);
    }
    splitk_reduce_launch(part, lay.ksplit, nW, dW, 0, s);
  } else {
    // the M products of one operand run as ONE "stacked" split-K product (chunk m = measure m: M x the
    // workgroups of a single product, which alone covers a fraction of the chip at the driver's sizes);
    // their sum over m, ascending -- the order the reference accumulates in -- is taken by the reduction.
    float* mq = reinterpret_cast<float*>(base + lay.mpart_off);
    float* ma = reinterpret_cast<float*>(base + lay.mpart2_off);
    g3[0] = gemm_args((int)R1, D, D, U, D, 1, W, 1, D, mq, D);
    g3[0].ksplit = M; g3[0].ks_stacked = 1; g3[0].a_ks = R1 * D; g3[0].b_ks = (long long)D * D; g3[0].c_ks = R1 * D;
    g3[1] = gemm_args((int)R2, D, D, V, D, 1, W, D, 1, ma, D);
    g3[1].ksplit = M; g3[1].ks_stacked = 1; g3[1].a_ks = R2 * D; g3[1].b_ks = (long long)D * D; g3[1].c_ks = R2 * D;
    if (!gemm_launch_group(g3, one3, 3, s)) {
      gemm_launch(g3[0], 1, s);
      gemm_launch(g3[1], 1, s);
      gemm_launch(g3[2], 1, s);
    }
    ReduceGroup rg{};
    reduce_group_add(rg, mq, dq, R1 * D, M);
    reduce_group_add(rg, ma, da, R2 * D, M);
    reduce_group_add(rg, part, dW, nW, lay.ksplit);
    reduce_group_launch(rg, s);
  }
  return launch_status();
}
}  // namespace mms
