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
// Three routes, all fp32 MFMA (fp32 in, fp32 accumulate): the fused per-pair / per-(pair, measure) kernels of
// bilinear_pair.h (instantiated here for float storage) for word grids that fit in LDS; the products above on the
// toolbox of gemm32.h for every other shape; and, at W1 = W2 = 1 with one measure, SimMatrix's launches (simmatrix.hip, through mms_internal.h), on whichever pipe
// mms_set_matrix_mode selects.  The dbias kernels (:301-304) are here because only this layer has a bias.
// Deterministic: split-K partial slabs are summed in a fixed order, no atomics.
#include <type_traits>

#include "bilinear_pair.h"
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
// (FB_LS, FB_W, FB_D, pair_bwd_eligible and BilinearWs: bilinear_pair.h, shared with bilinear_f16.hip)
// The sentence-vector geometry with ONE measure (W1 = W2 = 1, M = 1: BASELINE cfg 3 written as a SimCross layer) IS
// SimMatrix's arithmetic -- T_n = q_n^T W a_n (+ bias), dW = sum_n dT_n q_n a_n^T, dq_n = dT_n W a_n,
// da_n = dT_n W^T q_n -- so it takes SimMatrix's panel-GEMM launches (row dot and row scale as epilogues) instead
// of the generic GEMM + rowdot / rowscale launches: 45 + 136 us -> the SimMatrix figures (recomputing Q.W).
static bool bilinear_as_simmatrix(int W1, int W2, int M) { return W1 == 1 && W2 == 1 && M == 1; }

BilinearWs bilinear_ws(int N, int W1, int W2, int D, int M) {
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
    pair_bwd_launch(N, W1, W2, D, M, q, a, W, top_diff, mq, ma, part, s);
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
