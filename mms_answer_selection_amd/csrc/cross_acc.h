// csrc/cross_acc.h -- the register tile of one lane of the word-grid SimCross forward (dist_mode 0 / 1): the one
// definition of the d-ascending sums and of T, used by the two forward kernels of cross_grid.h for either storage
// (float, half): the operands are fp32 by the time they are in LDS.
#ifndef MMS_CROSS_ACC_H_
#define MMS_CROSS_ACC_H_

#include "euclid_math.h"

namespace mms {

// Lane (lj = lane>>3, lk = lane&7) of the wave that owns tile (j0, k0) holds outputs j = j0+lj+8*rj, k = k0+lk+8*rk.
// CrossAcc: the register tile of one lane.  Accumulators live in packed pairs (v_pk_add_f32 /
// v_pk_mul_f32 work on two fp32 per lane and per issue slot; each half is an ordinary IEEE op, so the
// d-ascending sums keep their bits): columns (2p, 2p+1) of a row pair up; with RK odd the last column
// pairs rows (2p, 2p+1); with both odd one scalar is left.
template <int RJ, int RK, int MODE>
struct CrossAcc {
  static constexpr int PK = RK / 2, PJ = (RK & 1) ? RJ / 2 : 0;
  static constexpr bool LAST = (RK & 1) && (RJ & 1);
  float2v accp[RJ][PK > 0 ? PK : 1], accq[PJ > 0 ? PJ : 1];
  float accs;

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int x = 0; x < RJ; ++x)
#pragma unroll
      for (int y = 0; y < (PK > 0 ? PK : 1); ++y) accp[x][y] = (float2v){0.f, 0.f};
#pragma unroll
    for (int x = 0; x < (PJ > 0 ? PJ : 1); ++x) accq[x] = (float2v){0.f, 0.f};
    accs = 0.f;
  }
  // dn steps of d: qrow / arow point at this lane's first row of each operand in LDS (column 0 of
  // the staged span), rows 8 apart are 8*ls floats apart
  __device__ __forceinline__ void accumulate(const float* qrow, const float* arow, int ls, int dn) {
    for (int dd = 0; dd < dn; ++dd) {
      float qv[RJ], av[RK];
#pragma unroll
      for (int x = 0; x < RJ; ++x) qv[x] = qrow[8 * x * ls + dd];
#pragma unroll
      for (int y = 0; y < RK; ++y) av[y] = arow[8 * y * ls + dd];
#pragma unroll
      for (int x = 0; x < RJ; ++x) {
        const float2v q2 = (float2v){qv[x], qv[x]};
#pragma unroll
        for (int y = 0; y < PK; ++y) {
          const float2v a2 = (float2v){av[2 * y], av[2 * y + 1]};
          if (MODE == 1) {
            const float2v df = q2 - a2;
            accp[x][y] += df * df;
          } else {
            accp[x][y] += q2 * a2;
          }
        }
      }
      if (PJ > 0) {
        const float2v a2 = (float2v){av[RK - 1], av[RK - 1]};
#pragma unroll
        for (int x = 0; x < PJ; ++x) {
          const float2v q2 = (float2v){qv[2 * x], qv[2 * x + 1]};
          if (MODE == 1) {
            const float2v df = q2 - a2;
            accq[x] += df * df;
          } else {
            accq[x] += q2 * a2;
          }
        }
      }
      if (LAST) {
        if (MODE == 1) {
          const float df = qv[RJ - 1] - av[RK - 1];
          accs += df * df;
        } else {
          accs += qv[RJ - 1] * av[RK - 1];
        }
      }
    }
  }
  __device__ __forceinline__ float get(int x, int y) const {
    if (y < 2 * PK) return (y & 1) ? accp[x][y / 2].y : accp[x][y / 2].x;
    if (x < 2 * PJ) return (x & 1) ? accq[x / 2].y : accq[x / 2].x;
    return accs;
  }
  // T from the sums (:106-107 / :131-136) and the stores of this lane's outputs
  __device__ __forceinline__ void finish(float* __restrict__ top, const float* __restrict__ norm0,
                                         const float* __restrict__ norm1, int n, int j0, int k0,
                                         int lj, int lk, int W1, int W2) const {
    // cosine: this lane's RJ + RK norms are in registers before its first store (a load between two stores
    // waits, with vmcnt(0), for the acknowledgement of the store in front of it)
    float n0v[RJ], n1v[RK];
    if (MODE != 1) {
#pragma unroll
      for (int x = 0; x < RJ; ++x) n0v[x] = norm0[(size_t)n * W1 + min(j0 + lj + 8 * x, W1 - 1)];
#pragma unroll
      for (int y = 0; y < RK; ++y) n1v[y] = norm1[(size_t)n * W2 + min(k0 + lk + 8 * y, W2 - 1)];
#pragma unroll
      for (int x = 0; x < RJ; ++x) asm volatile("" : "+v"(n0v[x]));
#pragma unroll
      for (int y = 0; y < RK; ++y) asm volatile("" : "+v"(n1v[y]));
    }
#pragma unroll
    for (int x = 0; x < RJ; ++x) {
      const int j = j0 + lj + 8 * x;
      if (j >= W1) continue;
#pragma unroll
      for (int y = 0; y < RK; ++y) {
        const int k = k0 + lk + 8 * y;
        if (k >= W2) continue;
        float T;
        if (MODE == 1) {
          T = 1.0f / (1.0f + sqrtf(get(x, y)));
        } else {
          T = get(x, y) / n0v[x] / n1v[y];
        }
        top[((size_t)n * W1 + j) * W2 + k] = T;
      }
    }
  }
};

}  // namespace mms
#endif  // MMS_CROSS_ACC_H_
