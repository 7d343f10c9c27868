// csrc/simcross_rows_cosine.hip -- SimCross dist_mode 0 (cosine) for W1 == W2 == 1 (sentence-vector pairs), fp32, for
// gfx950.  HBM-bound: no MFMA here.  The three fp32 entry points of simcross_cross.hip call launch_cosine_rows below;
// the Euclidean rows kernels are in simcross_rows.hip, the fp16-storage ones in simcross_rows_f16.hip.
//
// Reference semantics (all file:line in src/caffe/layers/sim_cross_layer.cpp):
//   Cosine fwd  :112-139  n0,n1 = sqrt(dot) cached; T = dot/n0/n1.
//   Cosine bwd  :226-250.
// The accumulation order, the score and both forms of the backward are cosine_math.h's, shared with the fused cosine
// triplet step.  Compiled with -ffp-contract=off.
#include "cosine_math.h"
#include "euclid_math.h"
#include "mms_internal.h"

namespace mms {

// Cosine, W1=W2=1: one wave per pair; three dot products reduced with a fixed
// butterfly (the reference's order here is whatever its BLAS does).
// BWD fuses the backward with a known top_diff.
template <bool VEC4, bool FWD, bool BWD>
__global__ __launch_bounds__(256) void cosine_rows_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_diff, float* __restrict__ top,
    float* __restrict__ norm0, float* __restrict__ norm1,
    float* __restrict__ dq, float* __restrict__ da, int N, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* qr = q + (size_t)row * D;
  const float* ar = a + (size_t)row * D;
  float g = 0.f;
  if (BWD) g = top_diff[row];                    // requested up front; pinned before the stores of the forward
  float T, n0, n1;
  if (FWD) {
    float sqq = 0.f, saa = 0.f, sqa = 0.f;
    if (VEC4) {
      const float4* q4 = reinterpret_cast<const float4*>(qr);
      const float4* a4 = reinterpret_cast<const float4*>(ar);
      for (int i = lane; i < (D >> 2); i += 64) {
        const float4 x = q4[i], y = a4[i];
        cosine_acc4(sqq, x, x); cosine_acc4(saa, y, y); cosine_acc4(sqa, x, y);
      }
    } else {
      for (int i = lane; i < D; i += 64) {
        const float x = qr[i], y = ar[i];
        cosine_acc1(sqq, x, x); cosine_acc1(saa, y, y); cosine_acc1(sqa, x, y);
      }
    }
    sqq = wave_sum(sqq); saa = wave_sum(saa); sqa = wave_sum(sqa);
    const CosineScore c = cosine_score(sqq, saa, sqa);
    T = c.T; n0 = c.n0; n1 = c.n1;
    if (BWD) asm volatile("" : "+v"(g));
    if (lane == 0) { top[row] = T; norm0[row] = n0; norm1[row] = n1; }
  } else {
    T = top[row]; n0 = norm0[row]; n1 = norm1[row];
  }
  if (!BWD) return;
  float* dqr = dq + (size_t)row * D;
  float* dar = da + (size_t)row * D;
  // :239-245   dq += g*(a/n0/n1 - q*T/(n0*n0)) ; da += g*(q/n0/n1 - a*T/(n1*n1))
  const float n00 = n0 * n0, n11 = n1 * n1;
  if (VEC4) {
    const float4* q4 = reinterpret_cast<const float4*>(qr);
    const float4* a4 = reinterpret_cast<const float4*>(ar);
    float4* dq4 = reinterpret_cast<float4*>(dqr);
    float4* da4 = reinterpret_cast<float4*>(dar);
    for (int i = lane; i < (D >> 2); i += 64) {
      const float4 x = q4[i], y = a4[i];
      const float4 o0 = cosine_grad4_div(g, n0, n1, T, n00, y, x);
      const float4 o1 = cosine_grad4_div(g, n0, n1, T, n11, x, y);
      stream_store(dq4 + i, o0);
      stream_store(da4 + i, o1);
    }
  } else {
    for (int i = lane; i < D; i += 64) {
      const float x = qr[i], y = ar[i];
      dqr[i] = cosine_grad_div(g, n0, n1, T, n00, y, x);
      dar[i] = cosine_grad_div(g, n0, n1, T, n11, x, y);
    }
  }
}

// Cosine, W1=W2=1, the GloVe widths (D = 100 / 200 / 300): the data movement of
// euclid_pair32_kernel -- 32 lanes per pair, two pairs per wave, every 16-byte load of q and a issued
// up front and kept in registers for the backward, half-wave DPP reductions, streaming stores --
// without the ordered chain (the reference's dot products are cblas_sdot: no defined order, 1e-5
// contract).  The backward multiplies by per-pair factors 1/n0/n1, T/n0^2, T/n1^2 computed once
// (IEEE divisions) instead of dividing per element (:239-245 written out costs six divisions per
// (q_d, a_d)): a few ulp from the reference's expression, inside the same 1e-5.
template <int D4C, bool FWD, bool BWD, int WPB>
__global__ __launch_bounds__(64 * WPB) void cosine_pair32_kernel(
    int N, const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top_diff, float* __restrict__ top, float* __restrict__ norm0,
    float* __restrict__ norm1, float* __restrict__ dq, float* __restrict__ da) {
  constexpr int NIT = (D4C + 31) / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 5, j = lane & 31;
  const int want = (blockIdx.x * WPB + wave) * 2 + grp;
  const bool have = want < N;
  const int row = have ? want : N - 1;
  const float4* q4 = reinterpret_cast<const float4*>(q) + (size_t)row * D4C;
  const float4* a4 = reinterpret_cast<const float4*>(a) + (size_t)row * D4C;
  float4 x[NIT], y[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = j + 32 * it;
    const int ii = i < D4C ? i : 0;              // clamp: keep the load unconditional
    x[it] = q4[ii];
    y[it] = a4[ii];
  }
  float T, n0, n1;
  if (FWD) {
    float sqq = 0.f, saa = 0.f, sqa = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (j + 32 * it < D4C) {
        const float4 u = x[it], v = y[it];
        cosine_acc4(sqq, u, u); cosine_acc4(saa, v, v); cosine_acc4(sqa, u, v);
      }
    }
    sqq = half_wave_sum(sqq); saa = half_wave_sum(saa); sqa = half_wave_sum(sqa);
    const CosineScore c = cosine_score(sqq, saa, sqa);
    T = c.T; n0 = c.n0; n1 = c.n1;
    if (j == 0 && have) { top[row] = T; norm0[row] = n0; norm1[row] = n1; }
  } else {
    T = top[row]; n0 = norm0[row]; n1 = norm1[row];
  }
  if (!BWD) return;
  const float g = top_diff[row];
  const CosineFactors f = cosine_factors(T, n0, n1);
  float4* dq4 = reinterpret_cast<float4*>(dq) + (size_t)row * D4C;
  float4* da4 = reinterpret_cast<float4*>(da) + (size_t)row * D4C;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = j + 32 * it;
    if (i < D4C && have) {
      const float4 u = x[it], v = y[it];
      const float4 o0 = cosine_grad4_fac(g, f.inv01, f.cq, v, u);
      const float4 o1 = cosine_grad4_fac(g, f.inv01, f.ca, u, v);
      stream_store(dq4 + i, o0);
      stream_store(da4 + i, o1);
    }
  }
}

// ================ dispatch (DESIGN.md 4.4b is the table this section is read against) ================
enum class CosineRows { kPair32, kVec4, kScalar };
static CosineRows cosine_rows_route(int D, const void* q, const void* a, const void* dq, const void* da) {
  if (!vec4_ok(D, q, a, dq, da)) return CosineRows::kScalar;
  return glove_width(D) ? CosineRows::kPair32 : CosineRows::kVec4;
}

// Cosine, W1 = W2 = 1: always served.  A backward alone reads top / norm0 / norm1 through the same parameters the
// forward writes them through.
template <bool FWD, bool BWD>
void launch_cosine_rows(int N, int D, const float* q, const float* a, const float* top_diff, float* top,
                        float* norm0, float* norm1, float* dq, float* da, hipStream_t s) {
  const CosineRows route = cosine_rows_route(D, q, a, dq, da);
  if (route == CosineRows::kPair32) {
    constexpr int WPB = 8;
    const unsigned grid = (unsigned)((N + 2 * WPB - 1) / (2 * WPB));
    with_glove_d4(D, [&](auto W) {
      hipLaunchKernelGGL((cosine_pair32_kernel<decltype(W)::value, FWD, BWD, WPB>), dim3(grid), dim3(64 * WPB), 0, s,
                         N, q, a, top_diff, top, norm0, norm1, dq, da);
    });
  } else {
    hipLaunchKernelGGL((route == CosineRows::kVec4 ? cosine_rows_kernel<true, FWD, BWD> : cosine_rows_kernel<false, FWD, BWD>),
                       dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, q, a, top_diff, top, norm0, norm1, dq, da, N, D);
  }
}

#define MMS_ROWS_INSTANCE(F, B)                                                                              \
  template void launch_cosine_rows<F, B>(int, int, const float*, const float*, const float*, float*, float*, \
                                         float*, float*, float*, hipStream_t);
MMS_ROWS_INSTANCE(true, false) MMS_ROWS_INSTANCE(false, true) MMS_ROWS_INSTANCE(true, true)
#undef MMS_ROWS_INSTANCE

}  // namespace mms
