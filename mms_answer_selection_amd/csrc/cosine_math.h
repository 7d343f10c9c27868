// csrc/cosine_math.h -- SimCross dist_mode 0 (cosine) for ONE pair, W1 = W2 = 1: the per-lane accumulation
// order, the score and the two forms of the backward (src/caffe/layers/sim_cross_layer.cpp:112-139, 226-250).
// Shared by simcross_rows_cosine.hip (cosine_pair32_kernel, cosine_rows_kernel) and by the fused cosine triplet
// step in triplet_steps.hip, whose scores, norms and gradients must carry the bits of those kernels: one definition
// of every expression, built with -ffp-contract=off, so the same operands give the same bits wherever it is
// inlined.  The word-grid backward kernels (cross_grid.h) take their factors and their per-(j, k) terms from here too.
#ifndef MMS_COSINE_MATH_H_
#define MMS_COSINE_MATH_H_

#include <hip/hip_runtime.h>

namespace mms {

// One float4 of a dot product into a lane's running sum: x, y, z, w in that order.
__device__ __forceinline__ void cosine_acc4(float& s, const float4& a, const float4& b) {
  s += a.x * b.x; s += a.y * b.y; s += a.z * b.z; s += a.w * b.w;
}
__device__ __forceinline__ void cosine_acc1(float& s, float a, float b) { s += a * b; }

struct CosineScore {
  float T, n0, n1;
};
// From the three reduced dot products.  The NORM is cached, as on the CPU (:118); two successive divisions (:135).
__device__ __forceinline__ CosineScore cosine_score(float sqq, float saa, float sqa) {
  CosineScore c;
  c.n0 = sqrtf(sqq);
  c.n1 = sqrtf(saa);
  c.T = sqa / c.n0 / c.n1;
  return c;
}

// ---- backward, per-pair factors (cosine_pair32_kernel): 1/n0/n1, T/n0^2, T/n1^2 computed once (IEEE divisions),
// then per element  0 + g * (other * inv01 - self * c)  with c = cq for dq and ca for da.
struct CosineFactors {
  float inv01, cq, ca;
};
__device__ __forceinline__ CosineFactors cosine_factors(float T, float n0, float n1) {
  CosineFactors f;
  f.inv01 = 1.0f / n0 / n1;
  f.cq = T / (n0 * n0);
  f.ca = T / (n1 * n1);
  return f;
}
// The bare term, for callers that add it to an accumulator started at +0.f (the word-grid kernels of cross_grid.h):
// there `0.f +` changes no bit -- it turns a term of -0 into +0, and acc + (-0) = acc + (+0) for every acc such a
// sum can hold (an accumulation from +0 never reaches -0).  cosine_grad_fac is the element itself: -0 becomes +0.
__device__ __forceinline__ float cosine_term_fac(float g, float inv01, float c, float other, float self) {
  return g * (other * inv01 - self * c);
}
__device__ __forceinline__ float cosine_grad_fac(float g, float inv01, float c, float other, float self) {
  return 0.f + cosine_term_fac(g, inv01, c, other, self);
}
__device__ __forceinline__ float4 cosine_grad4_fac(float g, float inv01, float c, const float4& other, const float4& self) {
  float4 o;
  o.x = cosine_grad_fac(g, inv01, c, other.x, self.x); o.y = cosine_grad_fac(g, inv01, c, other.y, self.y);
  o.z = cosine_grad_fac(g, inv01, c, other.z, self.z); o.w = cosine_grad_fac(g, inv01, c, other.w, self.w);
  return o;
}

// ---- backward, the reference's expression written out (cosine_rows_kernel, :239-245):
//   dq += g*(a/n0/n1 - q*T/(n0*n0)) ; da += g*(q/n0/n1 - a*T/(n1*n1));   nss = n0*n0 for dq, n1*n1 for da.
// cosine_term_div: the bare term, as cosine_term_fac.
__device__ __forceinline__ float cosine_term_div(float g, float n0, float n1, float T, float nss, float other, float self) {
  return g * (other / n0 / n1 - self * T / nss);
}
__device__ __forceinline__ float cosine_grad_div(float g, float n0, float n1, float T, float nss, float other, float self) {
  return 0.f + cosine_term_div(g, n0, n1, T, nss, other, self);
}
__device__ __forceinline__ float4 cosine_grad4_div(float g, float n0, float n1, float T, float nss, const float4& other,
                                                   const float4& self) {
  float4 o;
  o.x = cosine_grad_div(g, n0, n1, T, nss, other.x, self.x); o.y = cosine_grad_div(g, n0, n1, T, nss, other.y, self.y);
  o.z = cosine_grad_div(g, n0, n1, T, nss, other.z, self.z); o.w = cosine_grad_div(g, n0, n1, T, nss, other.w, self.w);
  return o;
}

}  // namespace mms
#endif  // MMS_COSINE_MATH_H_
