// csrc/simmatrix.hip -- SimMatrix (one learned metric W between two sentence vectors), forward and backward, its
// fp16-storage entry points, the matrix-mode switch and the fused learned-metric triplet step.
//
// Reference:
//   SimMatrix fwd        sim_matrix_layer.cpp:53-65    qw = Q W ; top_i = a_i . qw_i
//   SimMatrix bwd        sim_matrix_layer.cpp:68-95    dW += sum_i dT_i q_i a_i^T ; dq_i = dT_i W a_i ; da_i = dT_i W^T q_i
//   triplet step         the above twice, with pair_rank_loss_layer.cpp:26-84 between them
// The reference loops over the pairs on the host with one small BLAS call each; here all pairs share one
// tall-times-weight product per quantity, and the row dots / row scales are epilogues of those products.
//
// Which matrix pipe the products run on is mms_set_matrix_mode's choice: 0 (default) = the bf16 pipe on exact
// three-way splits of the fp32 operands, at fp32 accuracy (bx3_gemm.h; N >= 2048 rows and a workspace), 1 = fp32 MFMA
// (panel_gemm.h).  Shapes neither takes fall through to the toolbox of gemm32.h.  fp32 rounding differs from the
// reference's (as it does between BLAS libraries), tests hold it to 1e-5.
// Deterministic: split-K partial slabs are summed in a fixed order, no atomics.
#include "bx3_gemm.h"
#include "gemm32.h"
#include "mms_internal.h"
#include "panel_gemm.h"

namespace mms {

// SimMatrix backward on the bf16 pipe: the split-K reduction of dW and the operand image of W^T for the dq product are two
// independent small launches in a row; here they are ONE -- workgroups [0, red_blocks) reduce, the rest split.
__global__ __launch_bounds__(256) void splitk_reduce_split_kernel(const float* __restrict__ part, int splits, long long n,
                                                                  float* __restrict__ out, int accumulate, int red_blocks,
                                                                  const Bx3SplitArgs sp) {
  if ((int)blockIdx.x < red_blocks) {
    const long long stride = (long long)red_blocks * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
      const float s = ordered_slab_sum(part, n, e, splits, 0.f);
      out[e] = accumulate ? out[e] + s : s;
    }
    return;
  }
  bx3_split_b_body(sp, ((int)blockIdx.x - red_blocks) * 256 + threadIdx.x, ((int)gridDim.x - red_blocks) * 256);
}

// SimMatrix backward: the split-K reduction of dW and the transpose of W (the dq product's k-major B operand) are
// two independent ~5-us launches in a row; here they are ONE -- workgroups [0, red_blocks) reduce, the rest
// transpose 32 x 32 tiles -- which takes a launch (1.6 us of floor + the shorter kernel) off a cfg 3 step.
__global__ __launch_bounds__(256) void splitk_reduce_transpose_kernel(const float* __restrict__ part, int splits,
                                                                      long long n, float* __restrict__ out,
                                                                      int accumulate, int red_blocks,
                                                                      const float* __restrict__ tin,
                                                                      float* __restrict__ tout, int rows, int cols) {
  if ((int)blockIdx.x < red_blocks) {
    const long long stride = (long long)red_blocks * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
      const float s = ordered_slab_sum(part, n, e, splits, 0.f);
      out[e] = accumulate ? out[e] + s : s;
    }
    return;
  }
  __shared__ float tile[32][33];
  const int tb = (int)blockIdx.x - red_blocks, tiles_x = (cols + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int c0 = (tb % tiles_x) * 32, r0 = (tb / tiles_x) * 32;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rr = r0 + ty + 8 * u, cc = c0 + tx;
    if (rr < rows && cc < cols) tile[ty + 8 * u][tx] = tin[(long long)rr * cols + cc];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int oc = c0 + ty + 8 * u, orr = r0 + tx;          // tout[oc][orr] = tin[orr][oc]
    if (oc < cols && orr < rows) tout[(long long)oc * rows + orr] = tile[tx][ty + 8 * u];
  }
}

// ---------------------------------- SimMatrix -------------------------------
struct SimMatrixWs {
  size_t u_off, part_off, wt_off, img_off, total;
  int ksplit, kchunk;
};

// Which matrix pipe the tall-times-weight products of the learned-metric paths run on (mms_set_matrix_mode):
// 0 (default) = the bf16 pipe on exact three-way splits of the fp32 operands (bx3_gemm.h), 1 = fp32 MFMA (panel_gemm.h).
static int g_matrix_mode = 0;
int set_matrix_mode(int mode) {
  if (mode != 0 && mode != 1) return MMS_ERR_INVALID_ARG;
  g_matrix_mode = mode;
  return MMS_OK;
}
int get_matrix_mode() { return g_matrix_mode; }
// below this many rows the fp32 kernel's 64-row panels fill the chip better and the split launch is not worth its 3 us
static bool bx3_rows_worth(int M) { return M >= 2048; }
// May this call put its tall-times-weight products on the bf16 pipe?  `need`: the total of the call's workspace layout.
static bool bx3_pipe_ok(int mode, const void* ws, size_t ws_bytes, size_t need, int N) {
  return mode == 0 && ws && ws_bytes >= need && bx3_rows_worth(N);
}
// How the panel kernel / the bf16-pipe kernel split the N pairs of the dW product Q^T B (K1 x K2): read by the launch
// (panel_dw_args, bx3_dw_args) and by the workspace layouts, which size the slabs for whichever kernel runs
static int panel_dw_split(int N, int K1, int* kchunk) { return panel_pick_ksplit((K1 + 63) / 64, 1, N, kchunk); }
static int bx3_dw_split(int N, int K1, int K2, int* kchunk) { return bx3_tn_pick_chunks(N, bx3_tn_quads(K1, K2), kchunk); }

static SimMatrixWs simmatrix_ws(int N, int K1, int K2) {
  SimMatrixWs w{};
  w.ksplit = pick_ksplit(K1, K2, N, &w.kchunk);                           // gemm32's split (if it runs)
  int chunk = 0;
  const int psplit = panel_dw_split(N, K1, &chunk);
  w.u_off = 0;
  w.part_off = round_up((size_t)N * K2 * sizeof(float), 256);
  const int tsplit = bx3_dw_split(N, K1, K2, &chunk);
  int slabs = psplit > w.ksplit ? psplit : w.ksplit;
  if (tsplit > slabs) slabs = tsplit;
  w.wt_off = w.part_off + round_up((size_t)slabs * K1 * K2 * sizeof(float), 256);
  w.img_off = w.wt_off + round_up((size_t)K1 * K2 * sizeof(float), 256);    // W^T for the dq product (fp32 MFMA mode)
  const size_t ia = bx3_image_bytes(K2, K1), ib = bx3_image_bytes(K1, K2);  // the split image of W (forward) or W^T (dq)
  w.total = w.img_off + round_up(ia > ib ? ia : ib, 256);
  return w;
}
size_t simmatrix_workspace_bytes(int N, int K1, int K2) { return simmatrix_ws(N, K1, K2).total; }

static bx3_u4* simmatrix_img(void* ws, const SimMatrixWs& lay) {
  return reinterpret_cast<bx3_u4*>(static_cast<char*>(ws) + lay.img_off);
}

// ---- the launch sequences the entry points below are put together from ----
// X W on the bf16 pipe, X (N, K1) fp32 or (x_half) IEEE half, through the split image of W built at `img`: any of
// C = the product (scaled by rowscale[i] per row when given: then a bottom diff, stored streaming) and
// rowdot[i] = (rd_bias[0] +) row i of it . y_i (y stored like X).  Returns false, nothing launched, when not eligible.
static bool bx3_xw(int N, int K1, int K2, const void* x, int x_half, const float* W, bx3_u4* img, float* C, const void* y,
                   float* rowdot, const float* rd_bias, const float* rowscale, hipStream_t s) {
  Bx3Args b{};
  b.M = N; b.N = K2; b.K = K1; b.A = static_cast<const float*>(x); b.lda = K1; b.a_half = x_half; b.img = img;
  if (C) { b.C = C; b.ldc = K2; }
  if (y) { b.Y = static_cast<const float*>(y); b.ldy = K2; b.rowdot = rowdot; b.rd_stride = 1; b.rd_bias = rd_bias; }
  b.rowscale = rowscale; b.stream_c = rowscale != nullptr;
  if (!bx3_eligible(b)) return false;
  // the image of W; its launch also zeroes the scores when two column groups add their halves into them
  bx3_split_b(W, K2, 1, K1, K2, img, s, bx3_groups(K2) == 2 ? rowdot : nullptr, 1, N);
  bx3_launch(b, s);
  return true;
}

// dW += Q^T diag(kscale) B   (:73-80, accumulating), split over the N pairs into slabs at `part`, on the bf16 pipe: both
// operands (fp32, or IEEE half with ab_half) split on the fly (bx3_gemm.h, bx3_tn_kernel), slabs summed in chunk order
static Bx3TnArgs bx3_dw_args(int N, int K1, int K2, const void* q, const void* b, int ab_half, const float* kscale,
                             float* part) {
  Bx3TnArgs t{};
  t.M = K1; t.N = K2; t.K = N; t.A = static_cast<const float*>(q); t.lda = K1; t.B = static_cast<const float*>(b); t.ldb = K2;
  t.kscale = kscale; t.ab_half = ab_half; t.C = part; t.c_ks = (long long)K1 * K2;
  t.nchunks = bx3_dw_split(N, K1, K2, &t.kchunk);
  return t;
}
// dq_img: where the reduction's launch also builds the split image of W^T (the dq product's operand), or null.
// Returns whether it ran.
static bool bx3_dw(const Bx3TnArgs& t, float* dW, const float* W, bx3_u4* dq_img, hipStream_t s) {
  if (!bx3_tn_eligible(t)) return false;
  bx3_tn_launch(t, s);
  const unsigned rb = ew_blocks(t.c_ks);
  if (dq_img) {
    const Bx3SplitArgs sp = bx3_split_args(W, 1, t.N, t.N, t.M, dq_img);
    hipLaunchKernelGGL(splitk_reduce_split_kernel, dim3(rb + bx3_split_blocks(sp)), dim3(256), 0, s, t.C, t.nchunks, t.c_ks,
                       dW, 1, (int)rb, sp);
  } else {
    splitk_reduce_launch(t.C, t.nchunks, t.c_ks, dW, 1, s);
  }
  return true;
}

// The same product on the fp32 panel kernel: A(i, k = pair) = q_k[i] * kscale[k] (kscale is not optional there)
static PanelArgs panel_dw_args(int N, int K1, int K2, const float* q, const float* b, const float* kscale, float* part) {
  PanelArgs p = panel_args(K1, K2, N, q, K1, b, K2, part, K2);
  p.kscale = kscale;
  p.ksplit = panel_dw_split(N, K1, &p.kchunk);
  p.c_ks = (long long)K1 * K2;
  return p;
}
static bool panel_dw_eligible(const PanelArgs& p) { return p.ksplit > 1 && panel_eligible(p, false); }
// dq_wt: where the reduction's launch also writes W^T (the dq product's k-major operand), or null.  Returns whether it ran.
static bool panel_dw(const PanelArgs& p, float* dW, const float* W, float* dq_wt, hipStream_t s) {
  if (!panel_dw_eligible(p)) return false;
  panel_launch(p, false, s);
  const unsigned rb = ew_blocks(p.c_ks);
  if (dq_wt) {
    const unsigned tb = (unsigned)(((p.N + 31) / 32) * ((p.M + 31) / 32));
    hipLaunchKernelGGL(splitk_reduce_transpose_kernel, dim3(rb + tb), dim3(256), 0, s, p.C, p.ksplit, p.c_ks, dW, 1, (int)rb,
                       W, dq_wt, p.M, p.N);
  } else {
    splitk_reduce_launch(p.C, p.ksplit, p.c_ks, dW, 1, s);
  }
  return true;
}

// C = diag(rowscale) X W on the fp32 pipe (rowscale may be null), with the row dot against y (+ rd_bias) as the
// epilogue when y is given: the panel kernel, else gemm32 (+ rowdot_kernel).  A scaled product is a bottom diff, read
// next by another layer and not by this call: stored streaming.
static void fp32_xw(int N, int K1, int K2, const float* x, const float* W, float* C, const float* y, float* rowdot,
                    const float* rd_bias, const float* rowscale, hipStream_t s) {
  PanelArgs p = panel_args(N, K2, K1, x, K1, W, K2, C, K2);
  if (y) { p.Y = y; p.ldy = K2; p.rowdot = rowdot; p.rd_stride = 1; p.rd_bias = rd_bias; }
  p.rowscale = rowscale; p.stream_c = rowscale != nullptr;
  if (panel_eligible(p, true)) {
    panel_launch(p, true, s);
    return;
  }
  GemmArgs g = gemm_args(N, K2, K1, x, K1, 1, W, K2, 1, C, K2);
  g.rowscale = rowscale; g.stream_c = rowscale != nullptr;
  gemm_launch(g, 1, s);
  if (y) rowdot_launch(y, C, rd_bias, rowdot, N, K2, 1, s);
}

// qw = Q W  (:60-61) ; top_i = a_i . qw_i  (:62-64).  rd_bias: SimCross bilinear's bias (one scalar at W1 = W2 = 1), else null
int simmatrix_forward(int N, int K1, int K2, const float* q, const float* a, const float* W,
                      float* top, float* qw, hipStream_t s, const float* rd_bias, void* ws, size_t ws_bytes) {
  const SimMatrixWs lay = simmatrix_ws(N, K1, K2);
  if (!bx3_pipe_ok(g_matrix_mode, ws, ws_bytes, lay.total, N) ||
      !bx3_xw(N, K1, K2, q, 0, W, simmatrix_img(ws, lay), qw, a, top, rd_bias, nullptr, s))
    fp32_xw(N, K1, K2, q, W, qw, a, top, rd_bias, nullptr, s);
  return launch_status();
}

// fp16-STORAGE scoring (round 3): q (N, K1) and a (N, K2) are IEEE halves in HBM, W (K1, K2) and the scores fp32.
// top_i = a_i . (q_i W) on the bf16 pipe: a half is the exact sum of two bf16 values, the weight of three, so five of
// the six partial products exist and each is exact in fp32 -- the result is the fp32 layer's on the widened inputs
// to fp32 rounding (1e-5 bar as everywhere BLAS-ordered).  No Q.W output: scoring does not need it.  No fp32 fallback:
// shapes outside the kernel are MMS_ERR_UNSUPPORTED.
int simmatrix_forward_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, float* top, void* ws,
                          size_t ws_bytes, hipStream_t s) {
  return simmatrix_forward_train_f16(N, K1, K2, q, a, W, top, nullptr, ws, ws_bytes, s);
}

// da (halves) = diag(dT) . P  (P fp32: the training forward's Q.W), RNE at the store
__global__ __launch_bounds__(256) void rowscale_to_half_kernel(const float4* __restrict__ P, const float* __restrict__ dT,
                                                               void* __restrict__ out, long long rows, int cols4) {
  typedef _Float16 hf4 __attribute__((ext_vector_type(4)));
  const long long n = rows * cols4, stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    const float4 v = P[e];
    const float sc = dT[e / cols4];
    const hf4 o = {(_Float16)(0.f + sc * v.x), (_Float16)(0.f + sc * v.y), (_Float16)(0.f + sc * v.z), (_Float16)(0.f + sc * v.w)};
    __builtin_nontemporal_store(o, reinterpret_cast<hf4*>(out) + e);
  }
}

// fp16-STORAGE training forward / backward of SimMatrix (round 3): q, a and the bottom gradients dq, da are halves in
// HBM; W, dW, the scores, top_diff and the forward's Q.W (qw, (N, K2), the scratch the backward scales into da) fp32.
// All three products run on the bf16 pipe with the half operands split exactly into two planes (bx3_gemm.h);
// gradients are rounded to half (RNE) at the store.  No fp32 fallback: MMS_ERR_UNSUPPORTED outside the kernels' shapes.
int simmatrix_forward_train_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, float* top, float* qw,
                                void* ws, size_t ws_bytes, hipStream_t s) {
  const SimMatrixWs lay = simmatrix_ws(N, K1, K2);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  if (!bx3_xw(N, K1, K2, q, 1, W, simmatrix_img(ws, lay), qw, a, top, nullptr, nullptr, s)) return MMS_ERR_UNSUPPORTED;
  return launch_status();
}
int simmatrix_backward_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, const float* qw,
                           const float* top_diff, void* dq, void* da, float* dW, void* ws, size_t ws_bytes, hipStream_t s) {
  const SimMatrixWs lay = simmatrix_ws(N, K1, K2);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + lay.part_off);
  bx3_u4* img = simmatrix_img(ws, lay);
  const Bx3TnArgs t = bx3_dw_args(N, K1, K2, q, a, 1, top_diff, part);
  Bx3Args bq{};
  bq.M = N; bq.N = K1; bq.K = K2; bq.A = static_cast<const float*>(a); bq.lda = K2; bq.a_half = 1;
  bq.C = static_cast<float*>(dq); bq.ldc = K1; bq.c_half = 1; bq.rowscale = top_diff; bq.stream_c = 1; bq.img = img;
  bool da_written = false;
  if (dq && da && qw && K2 >= 8) {                 // da rides in the dq launch's loader waves (as in the fp32 path)
    bq.side_in = qw; bq.side_out = static_cast<float*>(da); bq.side_scale = top_diff; bq.side_ld = K2; bq.side_cols = K2;
    bq.side_half = 1;
    da_written = bx3_eligible(bq);
    if (!da_written) { bq.side_in = nullptr; bq.side_out = nullptr; bq.side_scale = nullptr; bq.side_half = 0; }
  }
  if ((dW && !bx3_tn_eligible(t)) || (dq && !bx3_eligible(bq)) || (da && (!qw || (K2 & 3) != 0 || !aligned16(qw) ||
                                                                         (reinterpret_cast<uintptr_t>(da) & 7u) != 0)))
    return MMS_ERR_UNSUPPORTED;
  // dW += Q^T diag(dT) A   (:73-80), both operands widened and split on the fly; W^T's image for dq built beside its sum
  if (dW) bx3_dw(t, dW, W, dq ? img : nullptr, s);
  else if (dq) bx3_split_b(W, 1, K2, K2, K1, img, s);
  if (dq) bx3_launch(bq, s);                       // dq_j = dT_j * (W a_j)   (:88, NoTrans)
  if (da && !da_written)                           // da_j = dT_j * (W^T q_j) (:88, Trans): the forward's product, scaled
    hipLaunchKernelGGL(rowscale_to_half_kernel, dim3(ew_blocks((long long)N * (K2 / 4))), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(qw), top_diff, da, (long long)N, K2 / 4);
  return launch_status();
}

// qw (optional): the forward's Q.W, unchanged since; may alias da.  da_j = dT_j * (W^T q_j) is row j of
// Q.W scaled by dT_j -- the product the forward already made with the same kernel and k order, so
// reusing it returns the same bits as recomputing it and saves one of the four GEMMs of a step.
int simmatrix_backward(int N, int K1, int K2, const float* q, const float* a, const float* W,
                       const float* top_diff, int ppd, int pd0, int pd1, float* dq, float* da,
                       float* dW, const float* qw, void* ws, size_t ws_bytes, hipStream_t s) {
  const SimMatrixWs lay = simmatrix_ws(N, K1, K2);
  const bool ws_ok = ws && ws_bytes >= lay.total;
  if (ppd && !ws_ok) return MMS_ERR_WORKSPACE;
  const bool bx3_ok = bx3_pipe_ok(g_matrix_mode, ws, ws_bytes, lay.total, N);
  char* base = static_cast<char*>(ws);

  // The dq product is planned first: the dW reduction's launch also builds the form of W that dq reads -- the split
  // image of W^T (bf16 pipe) or W^T itself (panel kernel) -- when dq will take that pipe.  dq_img / dq_wt: where, or null.
  Bx3Args bq{};                                 // dq_j = dT_j * (W a_j)   (:88, NoTrans, beta 0): B(k, n) = W[n][k]
  bx3_u4* dq_img = nullptr;
  if (pd0 && bx3_ok) {
    bq.M = N; bq.N = K1; bq.K = K2; bq.A = a; bq.lda = K2; bq.C = dq; bq.ldc = K1; bq.rowscale = top_diff; bq.stream_c = 1;
    bq.img = simmatrix_img(ws, lay);
    if (pd1 && qw && (K2 & 3) == 0 && K2 >= 8) {  // da rides in the dq launch's loader waves, if the kernel takes it so
      bq.side_in = qw; bq.side_out = da; bq.side_scale = top_diff; bq.side_ld = K2; bq.side_cols = K2;
      if (!bx3_eligible(bq)) { bq.side_in = nullptr; bq.side_out = nullptr; bq.side_scale = nullptr; }
    }
    if (bx3_eligible(bq)) dq_img = simmatrix_img(ws, lay);
  }
  PanelArgs pq{};                               // the same product on the panel kernel: B(k, n) = Wt[k][n]
  float* dq_wt = nullptr;
  if (pd0 && !dq_img && ws_ok) {
    float* Wt = reinterpret_cast<float*>(base + lay.wt_off);
    pq = panel_args(N, K1, K2, a, K2, Wt, K1, dq, K1);
    pq.rowscale = top_diff;
    pq.stream_c = 1;                            // read next by another layer, not by this call
    if (panel_eligible(pq, true)) dq_wt = Wt;
  }

  // dW += sum_i dT_i q_i a_i^T = Q^T (diag(dT) A)   (:73-80, accumulating)
  bool w_form_built = false;                    // the dW reduction's launch has produced what dq_img / dq_wt points to
  if (ppd) {
    float* part = reinterpret_cast<float*>(base + lay.part_off);
    if (bx3_ok && bx3_dw(bx3_dw_args(N, K1, K2, q, a, 0, top_diff, part), dW, W, dq_img, s)) {
      w_form_built = dq_img != nullptr;
    } else if (panel_dw(panel_dw_args(N, K1, K2, q, a, top_diff, part), dW, W, dq_wt, s)) {
      w_form_built = dq_wt != nullptr;
    } else {
      GemmArgs g = gemm_args(K1, K2, N, q, 1, K1, a, K2, 1, part, K2);
      g.ksplit = lay.ksplit; g.kchunk = lay.kchunk; g.c_ks = (long long)K1 * K2;
      g.bkscale = top_diff;                       // B(k = pair, j) = dT_k * a_k[j], scaled on load
      if (!gemm_fast_variant(g)) {                // generic kernel: materialise U = diag(dT) A first
        float* U = reinterpret_cast<float*>(base + lay.u_off);
        rowscale_launch(a, top_diff, U, N, K2, s);
        g.B = U;
        g.bkscale = nullptr;
      }
      gemm_launch(g, 1, s);
      splitk_reduce_launch(part, lay.ksplit, g.c_ks, dW, 1, s);
    }
  }

  // dq
  bool da_written = false;                      // by the dq launch's side job
  if (dq_img) {
    if (!w_form_built) bx3_split_b(W, 1, K2, K2, K1, dq_img, s);     // split straight from W's rows
    bx3_launch(bq, s);
    da_written = bq.side_in != nullptr;
  } else if (pd0) {
    if (dq_wt && pd1 && qw && K2 <= 304) {
      // da_j = dT_j * (row j of the forward's Q.W): a streaming pass with no arithmetic to speak of, carried
      // by this product's loader waves while its compute waves keep the matrix pipe busy
      pq.side_in = qw; pq.side_out = da; pq.side_scale = top_diff; pq.side_ld = K2; pq.side_cols = K2;
    }
    if (dq_wt && panel_eligible(pq, true)) {
      if (!w_form_built)
        hipLaunchKernelGGL(pg_transpose_kernel, dim3((K2 + 31) / 32, (K1 + 31) / 32), dim3(256), 0, s, W, dq_wt, K1, K2);
      panel_launch(pq, true, s);
      da_written = pq.side_in != nullptr;
    } else {
      GemmArgs g = gemm_args(N, K1, K2, a, K2, 1, W, 1, K2, dq, K1);
      g.rowscale = top_diff;
      g.stream_c = 1;
      gemm_launch(g, 1, s);
    }
  }

  // da_j = dT_j * (W^T q_j)   (:88, Trans, beta 0)
  if (!pd1 || da_written) {
    // not wanted, or written by the dq launch
  } else if (qw) {
    if ((K2 & 3) == 0 && aligned16(qw) && aligned16(da))
      rowscale4_launch(reinterpret_cast<const float4*>(qw), top_diff, reinterpret_cast<float4*>(da), N, K2 / 4, s);
    else
      rowscale_inplace_ok_launch(qw, top_diff, da, N, K2, s);
  } else if (!bx3_ok || !bx3_xw(N, K1, K2, q, 0, W, simmatrix_img(ws, lay), da, nullptr, nullptr, nullptr, top_diff, s)) {
    // (on the bf16 pipe it is the forward's product -- same kernel, same image, same k order: the bits of the cached
    // form above -- scaled in its epilogue)
    fp32_xw(N, K1, K2, q, W, da, nullptr, nullptr, nullptr, top_diff, s);
  }
  return launch_status();
}

// ------------------------- fused learned-metric triplet step (round 3) -------------------------
// The net  SimMatrix(q, a+) , SimMatrix(q, a-)  (W shared by parameter name) -> PairRankLoss, forward and backward, as
// THREE products instead of the layers' six (sim_matrix_layer.cpp:53-95 twice, pair_rank_loss_layer.cpp:26-84):
//   P = Q W is the same for both branches: one product, whose epilogue takes both row dots s+ = P_i . a+_i and
//   s- = P_i . a-_i, PairRankLoss's term and gradients g+, g- for the row, and writes da+ = g+ P_i, da- = g- P_i
//   (sim_matrix_layer.cpp:88, Trans) and B_i = g+ a+_i + g- a-_i;
//   dq = B W^T   (the Split sum of the two branches' dq_i = g W a_i, :88 NoTrans, as one product);
//   dW += Q^T B  (the two branches' sum_i g_i q_i a_i^T, :73-80, as one split-K product).
// Neither P nor the (N, 1) score gradients reach HBM.
struct TripSimWs {
  size_t b_off, terms_off, ones_off, wt_off, part_off, img_off, total;
};
static TripSimWs tripsim_ws(int N, int K1, int K2) {
  TripSimWs w{};
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += round_up(b, 256); return at; };
  w.b_off = take((size_t)N * K2 * sizeof(float));
  w.terms_off = take((size_t)N * sizeof(float));
  w.ones_off = take((size_t)N * sizeof(float));
  w.wt_off = take((size_t)K1 * K2 * sizeof(float));
  int chunk = 0;
  const int psplit = panel_dw_split(N, K1, &chunk), tsplit = bx3_dw_split(N, K1, K2, &chunk);
  const int slabs = tsplit > psplit ? tsplit : (psplit > 0 ? psplit : 1);
  w.part_off = take((size_t)slabs * K1 * K2 * sizeof(float));
  w.img_off = take(bx3_image_bytes(K1, K2));                                  // the split image of W^T (dq on the bf16 pipe)
  w.total = o;
  return w;
}

// MMS_ERR_UNSUPPORTED when the shapes are outside the panel kernel (triplet_simmatrix_step then runs the layers one by one)
static int tripsim_fused(int N, int K1, int K2, float margin, float loss_weight, const float* q, const float* ap,
                         const float* an, const float* y, const float* W, float* s_pos, float* s_neg, float* loss,
                         float* dq, float* dap, float* dan, float* dW, void* ws, size_t ws_bytes, hipStream_t s) {
  const TripSimWs lay = tripsim_ws(N, K1, K2);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(ws);
  float* B = reinterpret_cast<float*>(base + lay.b_off);
  float* terms = reinterpret_cast<float*>(base + lay.terms_off);
  float* ones = reinterpret_cast<float*>(base + lay.ones_off);
  float* Wt = reinterpret_cast<float*>(base + lay.wt_off);
  float* part = reinterpret_cast<float*>(base + lay.part_off);
  const float scale = loss_weight / (float)N;                       // pair_rank_loss_layer.cpp:64, count = N * 1
  // P = Q W with the triplet epilogue
  PanelArgs p1 = panel_args(N, K2, K1, q, K1, W, K2, nullptr, K2);
  p1.Y = ap; p1.Y2 = an; p1.ldy = K2; p1.rowdot = s_pos; p1.rd_stride = 1;
  p1.trip_y = y; p1.trip_margin = margin; p1.trip_s0 = -1.0f * scale; p1.trip_s1 = 1.0f * scale;
  p1.trip_hinge_ge = pairrank_hinge_mode() == MMS_PAIRRANK_HINGE_GPU ? 1 : 0;
  p1.trip_sneg = s_neg; p1.trip_terms = terms; p1.trip_dapos = dap; p1.trip_daneg = dan; p1.trip_b = B;
  // dq = B W^T  (B(k, n) = W[n][k] = Wt[k][n])
  PanelArgs p2 = panel_args(N, K1, K2, B, K2, Wt, K1, dq, K1);
  p2.stream_c = 1;
  // dW += Q^T B, split over the pairs (the ones are the fp32 split-K kernel's k-scale; the bf16-pipe kernel takes "no
  // scale" as such)
  const PanelArgs p3 = panel_dw_args(N, K1, K2, q, B, ones, part);
  if (!panel_eligible(p1, true) || !panel_eligible(p2, true) || !panel_dw_eligible(p3)) return MMS_ERR_UNSUPPORTED;
  // The two backward products on the bf16 pipe (matrix mode 0; bx3_gemm.h): dW += Q^T B from both operands split on the
  // fly, dq = B W^T with the image of W^T built in the reduction's launch.  (The forward stays on the fp32 pipe: its
  // epilogue needs whole rows of Q W in one workgroup, the bf16 kernel's workgroups own half a row each.)
  const Bx3TnArgs t = bx3_dw_args(N, K1, K2, q, B, 0, nullptr, part);
  bx3_u4* img = reinterpret_cast<bx3_u4*>(base + lay.img_off);
  Bx3Args bq{};
  bq.M = N; bq.N = K1; bq.K = K2; bq.A = B; bq.lda = K2; bq.C = dq; bq.ldc = K1; bq.stream_c = 1; bq.img = img;
  const bool back_bx3 = bx3_pipe_ok(g_matrix_mode, ws, ws_bytes, lay.total, N) && bx3_tn_eligible(t) && bx3_eligible(bq);
  if (!back_bx3 &&
      hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ones), 0x3f800000, (size_t)N, s) != hipSuccess) return MMS_ERR_LAUNCH;
  panel_launch(p1, true, s);
  if (loss) {
    const int rc = triplet_loss_from_terms(terms, N, loss, s);
    if (rc != MMS_OK) return rc;
  }
  if (back_bx3) {
    bx3_dw(t, dW, W, img, s);
    bx3_launch(bq, s);
  } else {
    panel_dw(p3, dW, W, Wt, s);
    panel_launch(p2, true, s);
  }
  return launch_status();
}

// The layers one by one, inside the call, for the shapes the fused route refuses:
// SimMatrix x 2 -> PairRankLoss -> PairRankLoss backward -> SimMatrix backward x 2 -> Split sum
struct TripSimSlow {
  size_t qwp, qwn, ord, sim, gsp, gsn, dq2, lossf, prws, smws, total;
};
static TripSimSlow tripsim_slow_layout(int N, int K1, int K2) {
  TripSimSlow w{};
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += round_up(b, 256); return at; };
  w.qwp = take((size_t)N * K2 * 4); w.qwn = take((size_t)N * K2 * 4);
  w.ord = take((size_t)N * 4); w.sim = take((size_t)N * 4); w.gsp = take((size_t)N * 4); w.gsn = take((size_t)N * 4);
  w.dq2 = take((size_t)N * K1 * 4); w.lossf = take(256);
  w.prws = take(pairrank_workspace_bytes(N)); w.smws = take(simmatrix_workspace_bytes(N, K1, K2));
  w.total = o;
  return w;
}
size_t triplet_simmatrix_workspace_bytes(int N, int K1, int K2) {
  const size_t fast = tripsim_ws(N, K1, K2).total, slow = tripsim_slow_layout(N, K1, K2).total;
  return fast > slow ? fast : slow;
}

int triplet_simmatrix_step(int N, int K1, int K2, float margin, float loss_weight, const float* q, const float* ap,
                           const float* an, const float* y, const float* W, float* s_pos, float* s_neg, float* loss,
                           float* dq, float* dap, float* dan, float* dW, void* ws, size_t ws_bytes, hipStream_t s) {
  const int rc = tripsim_fused(N, K1, K2, margin, loss_weight, q, ap, an, y, W, s_pos, s_neg, loss, dq, dap, dan, dW, ws,
                               ws_bytes, s);
  if (rc != MMS_ERR_UNSUPPORTED) return rc;
  const TripSimSlow lay = tripsim_slow_layout(N, K1, K2);
  if (ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  char* base = static_cast<char*>(ws);
  auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const size_t smb = simmatrix_workspace_bytes(N, K1, K2);
  int r = simmatrix_forward(N, K1, K2, q, ap, W, s_pos, f(lay.qwp), s, nullptr);
  if (r == MMS_OK) r = simmatrix_forward(N, K1, K2, q, an, W, s_neg, f(lay.qwn), s, nullptr);
  if (r == MMS_OK) r = pairrank_forward(N, margin, s_pos, s_neg, y, f(lay.ord), f(lay.sim), loss ? loss : f(lay.lossf),
                                       base + lay.prws, pairrank_workspace_bytes(N), s);
  if (r == MMS_OK) r = pairrank_backward(N, loss_weight, y, f(lay.ord), f(lay.sim), f(lay.gsp), f(lay.gsn), s);
  if (r == MMS_OK) r = simmatrix_backward(N, K1, K2, q, ap, W, f(lay.gsp), 1, 1, 1, dq, dap, dW, f(lay.qwp), base + lay.smws, smb, s);
  if (r == MMS_OK) r = simmatrix_backward(N, K1, K2, q, an, W, f(lay.gsn), 1, 1, 1, f(lay.dq2), dan, dW, f(lay.qwn),
                                         base + lay.smws, smb, s);
  if (r != MMS_OK) return r;
  const float* two[2] = {dq, f(lay.dq2)};
  return split_sum(N * K1, 2, two, dq, s);                      // Split: pos + neg, in place on pos
}

}  // namespace mms
