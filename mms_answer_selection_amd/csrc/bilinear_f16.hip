// csrc/bilinear_f16.hip -- fp16-STORAGE SimCross dist_mode 2 (the learned bilinear metric) on W1 x W2 word grids:
// mms_simcross_bilinear_forward_f16 / _backward_f16 / _forward_backward_f16 and mms_embed_simcross_bilinear_forward_f16.
// q (N,W1,D), a (N,W2,D), dq, da and the embedding table are IEEE halves in HBM; W (M,D,D), bias, dbias (M,W1,W2), top,
// top_diff (N,M,W1,W2) and dW are fp32.  Every half is widened exactly and everything after that is the fp32 arithmetic of
// bilinear.hip on the widened inputs; a gradient element is rounded ONCE (RNE; overflow gives +-Inf) when it is stored.
//
// Routes (the conditions are bilinear.hip's own: pair_fwd_route, pair_bwd_eligible in bilinear_pair.h):
//   fused     the three word-grid kernels of bilinear_pair.h instantiated for half storage: the halves are widened on
//             their way to the LDS images, no widened copy exists in HBM.  Backward with one measure: the kernel
//             stores the dq / da halves itself; with several, the per-measure fp32 partials stay in the workspace and
//             the grouped reduction (gemm32.h: reduce_group_add_half, the ordered_slab_sum of the fp32 layer) sums them
//             m ascending and rounds once.  dW and dbias are the fp32 layer's reductions.
//   generic   any other shape: one launch widens q and a into fp32 scratch, bilinear_forward / bilinear_backward run
//             unchanged on it (dq / da to fp32 scratch), one launch narrows both gradients.
// No arithmetic is defined here.  Compiled with -ffp-contract=off like every source of the library.
#include "bilinear_pair.h"
#include "gemm32.h"
#include "mms_internal.h"

namespace mms {

// x (nx halves) -> xf, y (ny halves) -> yf: exact
__global__ __launch_bounds__(256) void widen_pair_kernel(const _Float16* __restrict__ x, long long nx,
                                                         const _Float16* __restrict__ y, long long ny,
                                                         float* __restrict__ xf, float* __restrict__ yf) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nx + ny; e += stride) {
    if (e < nx) xf[e] = (float)x[e];
    else yf[e - nx] = (float)y[e - nx];
  }
}
// xf (nx floats) -> x, yf (ny floats) -> y: each element rounded once, RNE
__global__ __launch_bounds__(256) void narrow_pair_kernel(const float* __restrict__ xf, long long nx,
                                                          const float* __restrict__ yf, long long ny,
                                                          _Float16* __restrict__ x, _Float16* __restrict__ y) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nx + ny; e += stride) {
    if (e < nx) x[e] = (_Float16)xf[e];
    else y[e - nx] = (_Float16)yf[e - nx];
  }
}

// Workspace: the fp32 layer's (bilinear_ws) first; a shape whose forward or backward takes the generic route adds four
// fp32 arrays -- q, a widened and dq, da before narrowing -- 256-byte aligned whatever the caller's pointer is.
struct BilinearF16Ws {
  BilinearWs lay;
  size_t q_off, a_off, dq_off, da_off, total;     // offsets from the aligned scratch base; total includes the slack
  bool scratch;
};
static BilinearF16Ws bilinear_f16_ws(int N, int W1, int W2, int D, int M) {
  BilinearF16Ws w{};
  w.lay = bilinear_ws(N, W1, W2, D, M);
  w.total = w.lay.total;
  w.scratch = !(pair_fwd_route(N, W1, W2, D, M) != PAIR_FWD_NONE && pair_bwd_eligible(N, W1, W2, D, M));
  if (w.scratch) {
    const size_t qb = round_up((size_t)N * W1 * D * sizeof(float), 256), ab = round_up((size_t)N * W2 * D * sizeof(float), 256);
    w.q_off = 0; w.a_off = qb; w.dq_off = qb + ab; w.da_off = 2 * qb + ab;
    w.total = w.lay.total + 256 + 2 * (qb + ab);
  }
  return w;
}
size_t bilinear_workspace_bytes_f16(int N, int W1, int W2, int D, int M) {
  return bilinear_f16_ws(N, W1, W2, D, M).total;
}

// forward (fwd), backward (bwd) or the forward, then the backward, on `s`.  mms_abi.hip has checked the arguments:
// not W1 == W2 == 1, N >= 1, every pointer the selected passes need.
int simcross_bilinear_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16, const float* W,
                          const float* bias, int bias_term, const float* top_diff, float* top, void* dq_f16, void* da_f16,
                          float* dW, float* dbias, void* ws, size_t ws_bytes, bool fwd, bool bwd, hipStream_t s) {
  const BilinearF16Ws lay = bilinear_f16_ws(N, W1, W2, D, M);
  if (!ws || ws_bytes < lay.total) return MMS_ERR_WORKSPACE;
  const _Float16* q = static_cast<const _Float16*>(q_f16);
  const _Float16* a = static_cast<const _Float16*>(a_f16);
  _Float16* dq = static_cast<_Float16*>(dq_f16);
  _Float16* da = static_cast<_Float16*>(da_f16);
  char* base = static_cast<char*>(ws);
  const long long nq = (long long)N * W1 * D, na = (long long)N * W2 * D;
  const bool fwd_generic = fwd && pair_fwd_route(N, W1, W2, D, M) == PAIR_FWD_NONE;
  const bool bwd_generic = bwd && !pair_bwd_eligible(N, W1, W2, D, M);
  float *q32 = nullptr, *a32 = nullptr, *dq32 = nullptr, *da32 = nullptr;
  if (fwd_generic || bwd_generic) {
    char* x = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + lay.lay.total + 255) & ~(uintptr_t)255);
    q32 = reinterpret_cast<float*>(x + lay.q_off);
    a32 = reinterpret_cast<float*>(x + lay.a_off);
    dq32 = reinterpret_cast<float*>(x + lay.dq_off);
    da32 = reinterpret_cast<float*>(x + lay.da_off);
    hipLaunchKernelGGL(widen_pair_kernel, dim3(ew_blocks(nq + na)), dim3(256), 0, s, q, nq, a, na, q32, a32);
  }
  if (fwd) {
    if (fwd_generic) {
      const int rc = bilinear_forward(N, W1, W2, D, M, q32, a32, W, bias, top, ws, lay.lay.total, s);
      if (rc != MMS_OK) return rc;
    } else {
      pair_fwd_launch(N, W1, W2, D, M, q, a, W, bias, top, s);
    }
  }
  if (bwd && bwd_generic) {
    const int rc = bilinear_backward(N, W1, W2, D, M, q32, a32, W, bias_term, top_diff, dq32, da32, dW, dbias, ws,
                                     lay.lay.total, s);
    if (rc != MMS_OK) return rc;
    hipLaunchKernelGGL(narrow_pair_kernel, dim3(ew_blocks(nq + na)), dim3(256), 0, s, dq32, nq, da32, na, dq, da);
  } else if (bwd) {
    // one launch for the five products of every (pair, measure), one grouped launch for the sums (bilinear_backward)
    float* part = reinterpret_cast<float*>(base + lay.lay.part_off);
    ReduceGroup rg{};
    if (M == 1) {
      pair_bwd_launch(N, W1, W2, D, M, q, a, W, top_diff, dq, da, part, s);
    } else {
      float* mq = reinterpret_cast<float*>(base + lay.lay.mpart_off);
      float* ma = reinterpret_cast<float*>(base + lay.lay.mpart2_off);
      pair_bwd_launch(N, W1, W2, D, M, q, a, W, top_diff, mq, ma, part, s);
      reduce_group_add_half(rg, mq, dq, nq, M);
      reduce_group_add_half(rg, ma, da, na, M);
    }
    reduce_group_add(rg, part, dW, (long long)M * D * D, N);      // W.diff is overwritten (:256), pairs summed ascending
    if (bias_term) reduce_group_add(rg, top_diff, dbias, (long long)M * W1 * W2, N, 1);   // bias.diff += dT_n (:301-304)
    reduce_group_launch(rg, s);
  }
  return launch_status();
}

// top = SimCross_bilinear(Embed(index_q), Embed(index_a)) from a half table, in ONE launch: embed_bilinear_forward's
// kernels with the gather reading halves (row value = embed_bias[d] + widen(table[id][d]) in fp32).
int embed_bilinear_forward_f16(int N, int W1, int W2, int D, int M, int K, const float* index_q, const float* index_a,
                               const void* table_f16, const float* embed_bias, const float* W, const float* bias,
                               float* top, hipStream_t s) {
  const _Float16* table = static_cast<const _Float16*>(table_f16);
  if (!pair_fwd_launch(N, W1, W2, D, M, table, table, W, bias, top, s, PairGather{index_q, index_a, K, embed_bias}))
    return MMS_ERR_UNSUPPORTED;
  return launch_status();
}

}  // namespace mms
