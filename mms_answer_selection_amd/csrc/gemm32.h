// csrc/gemm32.h -- the one declaration of what gemm32.hip defines for the learned-metric sources (bilinear.hip,
// simmatrix.hip): the argument blocks, host functions only -- no __global__ symbol is named outside gemm32.hip --
// and the ordered slab sum, a device helper that split-K reductions fused with other work (simmatrix.hip) share.
// gemm32.hip includes it too, and default arguments live here only.
#ifndef MMS_GEMM32_H_
#define MMS_GEMM32_H_

#include "mms_common.h"

namespace mms {

struct GemmArgs {
  int M, N, K;
  const float* A; long long a_rs, a_cs;  // A(i,k) = A[i*a_rs + k*a_cs]
  const float* B; long long b_rs, b_cs;  // B(k,j) = B[k*b_rs + j*b_cs]
  float* C; long long ldc;               // C(i,j) = C[i*ldc + j]
  // blockIdx.z = (b0 * nb1 + b1) * ksplit + ks
  int nb1, ksplit, kchunk;
  long long a_b0, a_b1, b_b0, b_b1, c_b0, c_b1, c_ks;
  // "stacked" split-K: chunk ks is a product of its own, A + ks*a_ks times B + ks*b_ks over k in [0, K)
  // (sum over measures of U_m W_m: K is not one contiguous axis); partials land at C + ks*c_ks as usual.
  int ks_stacked; long long a_ks, b_ks;
  const float* rowscale; long long rs_b0;  // optional C(i,j) = rowscale[i] * acc
  const float* addend; long long ad_b1;    // optional C(i,j) += addend[i*ldc + j]
  const float* bkscale;                    // optional B(k,j) *= bkscale[k] on load (fast j-vector path)
  int beta_one;                            // C = result + C
  int stream_c;                            // C is written once and not re-read soon: non-temporal stores
  int a_ifast, b_jfast;                    // which index is contiguous in memory
};

constexpr int kGroupMax = 4;   // most problems of one grouped launch

GemmArgs gemm_args(int M, int N, int K, const float* A, long long a_rs, long long a_cs, const float* B, long long b_rs,
                   long long b_cs, float* C, long long ldc);
// which fast variant (if any) can run these arguments: 0 none, else 1 + 2*A_KVEC + B_JVEC; *vw_out = floats
// per global load (4, else 2)
int gemm_fast_variant(const GemmArgs& g, int* vw_out = nullptr);
// nb0 products, g's b0 strides apart: the fast kernel that takes the arguments, else the stride-generic one
void gemm_launch(const GemmArgs& g, int nb0, hipStream_t s);
// Launch up to kGroupMax independent small products as one grid.  Returns false -- nothing launched -- when a problem
// needs the stride-generic kernel or an epilogue the group kernel does not carry, or when the products are big
// enough to deserve their own tuned launches.
bool gemm_launch_group(const GemmArgs* gs, const int* nb0s, int n, hipStream_t s);
// Split count for a product with a long K (see gemm32.hip); *kchunk = the K extent of one split.
int pick_ksplit(int Mt, int Nt, int K, int* kchunk, int batch = 1);
// workgroups of 256 threads for n elements of a grid-stride element-wise kernel
unsigned ew_blocks(long long n);

// s + part[0*n + e] + part[1*n + e] + ... in s-ascending order (the reference accumulates over pairs / measures in
// that order).  All requests of a batch are in flight before the first add -- a load-add-load loop costs one
// memory round trip per slab; batches of 32 above eight slabs (a training batch of 50 pairs: two round trips
// instead of seven), of 8 below (dQ / dA over four measures: no wasted requests).
__device__ __forceinline__ float ordered_slab_sum(const float* __restrict__ part, long long n, long long e, int splits,
                                                  float s) {
  if (splits > 8) {
    for (int k0 = 0; k0 < splits; k0 += 32) {
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = part[(long long)min(k0 + u, splits - 1) * n + e];
#pragma unroll
      for (int u = 0; u < 32; ++u) s += (k0 + u < splits) ? v[u] : 0.f;
    }
    return s;
  }
  float v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) v[u] = part[(long long)min(u, splits - 1) * n + e];
#pragma unroll
  for (int u = 0; u < 8; ++u) s += (u < splits) ? v[u] : 0.f;
  return s;
}

// Several split-K reductions in one launch: problem p owns blocks [first[p], first[p+1]).
struct ReduceGroup {
  const float* part[kGroupMax];
  float* out[kGroupMax];
  long long n[kGroupMax];
  int splits[kGroupMax];
  int accumulate[kGroupMax];     // the sum starts from out[e] (bias.diff += ..., sim_cross_layer.cpp:301-304) instead of 0
  int first[kGroupMax + 1];
  int cnt;
  int half_out[kGroupMax];       // out holds IEEE halves: the fp32 sum is rounded once (RNE) as it is stored
};
// next problem of a grouped reduction: its blocks follow the previous problem's (first[cnt] = blocks so far)
void reduce_group_add(ReduceGroup& rg, const float* part, float* out, long long n, int splits, int accumulate = 0);
// the same with half storage of the result (fp16-storage gradients): out[e] = half(0 + part[0*n + e] + part[1*n + e] + ...)
void reduce_group_add_half(ReduceGroup& rg, const float* part, void* out_f16, long long n, int splits);
void reduce_group_launch(const ReduceGroup& rg, hipStream_t s);

// ---- one launch each of the element-wise kernels that more than one source uses ----
// out[e] (= or, with accumulate, +=) sum_s part[s*n + e], s ascending
void splitk_reduce_launch(const float* part, int splits, long long n, float* out, int accumulate, hipStream_t s);
// top[r * top_stride] = dot(x[r], y[r]) (+ bias[0])
void rowdot_launch(const float* x, const float* y, const float* bias, float* top, long long rows, int cols,
                   long long top_stride, hipStream_t s);
// out[r][c] = scale[r] * x[r][c]: out apart from x / out may BE x / out may be x, 16-byte-aligned rows of 4 * cols4
// floats, stored streaming
void rowscale_launch(const float* x, const float* scale, float* out, long long rows, int cols, hipStream_t s);
void rowscale_inplace_ok_launch(const float* x, const float* scale, float* out, long long rows, int cols, hipStream_t s);
void rowscale4_launch(const float4* x, const float* scale, float4* out, long long rows, int cols4, hipStream_t s);

}  // namespace mms
#endif  // MMS_GEMM32_H_
