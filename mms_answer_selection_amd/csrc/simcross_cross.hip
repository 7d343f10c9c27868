// csrc/simcross_cross.hip -- SimCross dist_mode 0 (cosine) and 1 (Euclidean) on general W1 x W2 word grids
// (TREC-QA 40x40) for gfx950, and the three fp32 entry points.  HBM-bound: no MFMA here.
//
// Reference semantics (all file:line in src/caffe/layers/sim_cross_layer.cpp):
//   Euclid fwd  :96-111   T = 1/(1+sqrt(sum_d (q-a)^2)), d ascending, fp32.
//   Euclid bwd  :208-225  tt = dT*T*T*T*(q-a)/(T-1+1e-9) (double divide);
//                         dq[j,d] = sum_k tt (k ascending from 0),
//                         da[k,d] = sum_j -tt (j ascending from 0).
//   Cosine fwd  :112-139  n0,n1 = sqrt(dot) cached; T = dot/n0/n1.
//   Cosine bwd  :226-250.
//
// Forward: one wave per (pair, j-tile, k-tile), q/a d-chunks staged in LDS, an RJ x RK register tile per lane, d
// ascending per output.  W1 == W2 == 1 (sentence-vector pairs) has kernels of its own in simcross_rows.hip
// (Euclid) and simcross_rows_cosine.hip; the entry points at the end of this file try those first and fall through to
// the grid kernels.
//
// Compiled with -ffp-contract=off: the reference CPU build has no FMA
// contraction, so mul and add must round separately to match it bitwise.
#include "cosine_math.h"
#include "cross_acc.h"
#include "cross_gather.h"
#include "euclid_math.h"
#include "mms_internal.h"

namespace mms {

// L2 norms of `rows` rows of length D: one wave per row (cosine, general W).
// index != nullptr: row `row` is table row index[row] of x (K rows) -- the Embed gather fused in.
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ x,
                                                       float* __restrict__ nrm,
                                                       long long rows, int D,
                                                       const float* __restrict__ index, int K,
                                                       const float* __restrict__ ebias = nullptr) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* r = x + (index ? (long long)gather_id(index[row], K) : row) * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) { const float v = ebias ? ebias[i] + r[i] : r[i]; s += v * v; }
  s = wave_sum(s);
  if (lane == 0) nrm[row] = sqrtf(s);
}

// Forward for general W1 x W2, MODE 0 (cosine; norms precomputed) or 1.
// One wave per (pair, j-tile, k-tile); tile = (8*RJ) x (8*RK) outputs,
// lane (lj = lane>>3, lk = lane&7) owns outputs j = j0+lj+8*rj, k = k0+lk+8*rk: CrossAcc (cross_acc.h).
// The fused Embed gather (a CrossGather with iq != nullptr; gather_id clamps the ids): cross_gather.h.

// Generic staging: q/a are staged DC floats of d at a time in LDS with stride DC+1 (bank =
// (row + d) mod 32: conflict-free across rows, broadcast within a row).
template <int RJ, int RK, int MODE>
__global__ __launch_bounds__(256) void cross_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ norm0, const float* __restrict__ norm1,
    float* __restrict__ top, int N, int W1, int W2, int D, int tilesJ, int tilesK, CrossGather gt) {
  constexpr int TJ = 8 * RJ, TK = 8 * RK, DC = 32, LS = DC + 1;
  __shared__ float qs[4][TJ * LS];
  __shared__ float as[4][TK * LS];
  __shared__ int rowoff[4][TJ + TK];               // gather: element offset of each tile row in the table
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long work = (long long)blockIdx.x * 4 + wave;
  const long long total = (long long)N * tilesJ * tilesK;
  const bool valid = work < total;
  const long long w = valid ? work : 0;
  const int n = (int)(w / (tilesJ * tilesK));
  const int rem = (int)(w % (tilesJ * tilesK));
  const int j0 = (rem / tilesK) * TJ, k0 = (rem % tilesK) * TK;
  const int lj = lane >> 3, lk = lane & 7;
  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;

  CrossAcc<RJ, RK, MODE> acc;
  acc.clear();

  const int lrow = lane >> 5, lcol = lane & 31;
  // Staging: every load of a chunk is issued (clamped, hence unconditional, addresses) before the
  // first LDS write; out-of-range elements are zeroed when written.  Written as `ok ? load : 0` the
  // compiler emitted load / wait / write per row: 40 serialized round trips per chunk (18 of 38 us
  // at 1517 x 40 x 40 x 50).  The NEXT chunk's loads are issued right after the LDS writes of the
  // current one, so they are in flight behind its arithmetic.
  float rq[TJ / 2], ra[TK / 2];
  const bool gather = gt.iq != nullptr;
  if (gather) {                                  // word ids of this tile's rows -> table offsets, once
    for (int r = lane; r < TJ + TK; r += 64) {
      const bool isq = r < TJ;
      const int rr = isq ? min(j0 + r, W1 - 1) : min(k0 + r - TJ, W2 - 1);
      const float id = isq ? gt.iq[(size_t)n * W1 + rr] : gt.ia[(size_t)n * W2 + rr];
      rowoff[wave][r] = gather_id(id, gt.K) * D;
    }
    wave_lds_sync();
  }
  auto fetch = [&](int d0) {
    const int col = min(d0 + lcol, D - 1);
    if (gather) {
#pragma unroll
      for (int r = 0; r < TJ; r += 2) rq[r / 2] = q[(size_t)rowoff[wave][r + lrow] + col];
#pragma unroll
      for (int r = 0; r < TK; r += 2) ra[r / 2] = a[(size_t)rowoff[wave][TJ + r + lrow] + col];
      if (gt.bias) {
        const float bv = gt.bias[col];
#pragma unroll
        for (int r = 0; r < TJ; r += 2) rq[r / 2] = bv + rq[r / 2];
#pragma unroll
        for (int r = 0; r < TK; r += 2) ra[r / 2] = bv + ra[r / 2];
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < TJ; r += 2) rq[r / 2] = qn[(size_t)min(j0 + r + lrow, W1 - 1) * D + col];
#pragma unroll
    for (int r = 0; r < TK; r += 2) ra[r / 2] = an[(size_t)min(k0 + r + lrow, W2 - 1) * D + col];
  };
  fetch(0);
  for (int d0 = 0; d0 < D; d0 += DC) {
    const int dn = min(DC, D - d0);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TJ; r += 2)
      qs[wave][(r + lrow) * LS + lcol] = (valid && j0 + r + lrow < W1 && lcol < dn) ? rq[r / 2] : 0.f;
#pragma unroll
    for (int r = 0; r < TK; r += 2)
      as[wave][(r + lrow) * LS + lcol] = (valid && k0 + r + lrow < W2 && lcol < dn) ? ra[r / 2] : 0.f;
    __syncthreads();
    if (d0 + DC < D) fetch(d0 + DC);
    acc.accumulate(&qs[wave][lj * LS], &as[wave][lk * LS], LS, dn);
  }
  if (!valid) return;
  acc.finish(top, norm0, norm1, n, j0, k0, lj, lk, W1, W2);
}

// "Pair image" staging for small D (the driver's default 50-d vectors): a wave owns one whole pair,
// W1 = 8*RJ and W2 = 8*RK exactly, and the (W1 x D) and (W2 x D) blocks of q and a -- contiguous in
// memory -- are COPIED to LDS as they are, 16 bytes per lane per load, row stride D (no padding, no
// chunking over d, no index arithmetic).  Rows 8 apart must fall into different banks for the
// broadcast reads of accumulate(): gcd(D, 64) <= 8 (launch_cross_fwd checks).  Against the generic
// staging at 1517 x 40 x 40 x 50 this replaces 80 4-byte load instructions and 80 predicated LDS
// writes per wave by 16 + 16.  Waves are independent: 2 per workgroup, 32 KB of LDS each.
// D is a template parameter: with a run-time row stride the ten row addresses of accumulate() are
// recomputed per d step (VALU-bound loop: +15 % time); compiled in, they are immediate offsets.
template <int RJ, int RK, int MODE, int D>
__global__ __launch_bounds__(128) void cross_fwd_image_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ norm0, const float* __restrict__ norm1,
    float* __restrict__ top, int N, CrossGather gt) {
  constexpr int W1 = 8 * RJ, W2 = 8 * RK;
  extern __shared__ float4 img4[];                 // [2 waves][(W1 + W2) * D / 4]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int work = blockIdx.x * 2 + wave;
  const bool valid = work < N;
  const int n = valid ? work : N - 1;
  const int nq4 = W1 * D / 4, na4 = W2 * D / 4;
  float4* qs4 = img4 + (size_t)wave * (nq4 + na4);
  float4* as4 = qs4 + nq4;
  const float4* q4 = reinterpret_cast<const float4*>(q + (size_t)n * W1 * D);
  const float4* a4 = reinterpret_cast<const float4*>(a + (size_t)n * W2 * D);
  if (gt.iq != nullptr) {
    // Embed fused in: image row r is table row id[r]; rows are D floats = 8-byte aligned for even D, so
    // the copy runs in float2.  Per batch: the ids of 8 + 8 elements, then their 16 loads, then the writes.
    constexpr int R2 = D / 2;                      // float2 per row
    float2* qs2 = reinterpret_cast<float2*>(qs4);
    float2* as2 = reinterpret_cast<float2*>(as4);
    const float2* t2 = reinterpret_cast<const float2*>(q);
    const float* iq = gt.iq + (size_t)n * W1;
    const float* ia = gt.ia + (size_t)n * W2;
    constexpr int NQ2 = W1 * R2, NA2 = W2 * R2, NMAX = NQ2 > NA2 ? NQ2 : NA2;
    for (int e0 = 0; e0 < NMAX; e0 += 512) {
      float idq[8], ida[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        idq[u] = iq[min(e, NQ2 - 1) / R2];
        ida[u] = ia[min(e, NA2 - 1) / R2];
      }
      float2 rq[8], ra[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        rq[u] = t2[(size_t)gather_id(idq[u], gt.K) * R2 + min(e, NQ2 - 1) % R2];
        ra[u] = t2[(size_t)gather_id(ida[u], gt.K) * R2 + min(e, NA2 - 1) % R2];
      }
      if (gt.bias) {
        const float2* b2 = reinterpret_cast<const float2*>(gt.bias);   // D even: the row pitch makes this 8-byte aligned with the table
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = e0 + 64 * u + lane;
          const float2 bq = b2[min(e, NQ2 - 1) % R2], ba = b2[min(e, NA2 - 1) % R2];
          rq[u].x = bq.x + rq[u].x; rq[u].y = bq.y + rq[u].y;
          ra[u].x = ba.x + ra[u].x; ra[u].y = ba.y + ra[u].y;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 64 * u + lane;
        if (e < NQ2) qs2[e] = rq[u];
        if (e < NA2) as2[e] = ra[u];
      }
    }
  } else
  // copy in batches of 4 + 4 loads (all issued before the first LDS write of the batch)
  for (int i0 = 0; i0 < max(nq4, na4); i0 += 256) {
    float4 rq[4], ra[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 64 * u + lane;
      rq[u] = q4[min(i, nq4 - 1)];
      ra[u] = a4[min(i, na4 - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 64 * u + lane;
      if (i < nq4) qs4[i] = rq[u];
      if (i < na4) as4[i] = ra[u];
    }
  }
  wave_lds_sync();
  const int lj = lane >> 3, lk = lane & 7;
  CrossAcc<RJ, RK, MODE> acc;
  acc.clear();
  acc.accumulate(reinterpret_cast<const float*>(qs4) + lj * D, reinterpret_cast<const float*>(as4) + lk * D, D, D);
  if (!valid) return;
  acc.finish(top, norm0, norm1, n, 0, 0, lj, lk, W1, W2);
}

// Backward for general W1 x W2, MODE 0/1: one workgroup per pair n.  Thread
// owns one (j,d) of dq and walks k ascending, then one (k,d) of da and walks
// j ascending -- the reference's accumulation order (:209-223), so Euclidean
// is bit-exact.  q/a/top rows of one n stay L1/L2-resident across the walk.
template <int MODE>
__global__ __launch_bounds__(256) void cross_bwd_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top, const float* __restrict__ top_diff,
    const float* __restrict__ norm0, const float* __restrict__ norm1,
    float* __restrict__ dq, float* __restrict__ da, int W1, int W2, int D) {
  const int n = blockIdx.x;
  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;
  const float* Tn = top + (size_t)n * W1 * W2;
  const float* gn = top_diff + (size_t)n * W1 * W2;
  float* dqn = dq + (size_t)n * W1 * D;
  float* dan = da + (size_t)n * W2 * D;
  const float* n0n = MODE == 0 ? norm0 + (size_t)n * W1 : nullptr;
  const float* n1n = MODE == 0 ? norm1 + (size_t)n * W2 : nullptr;

  for (int e = threadIdx.x; e < W1 * D; e += 256) {
    const int j = e / D, d = e - j * D;
    const float qv = qn[e];
    float acc = 0.f;
    if (MODE == 1) {
      for (int k = 0; k < W2; ++k) {
        const EuclidCoef kc = euclid_coef(Tn[j * W2 + k], gn[j * W2 + k]);
        acc += euclid_tt_exact(kc.c, kc.den, qv - an[(size_t)k * D + d]);
      }
    } else {
      const float nrm0 = n0n[j];
      for (int k = 0; k < W2; ++k) {
        const float nrm1 = n1n[k];
        acc += gn[j * W2 + k] * (an[(size_t)k * D + d] / nrm0 / nrm1 -
                                 qv * Tn[j * W2 + k] / (nrm0 * nrm0));
      }
    }
    dqn[e] = acc;
  }
  for (int e = threadIdx.x; e < W2 * D; e += 256) {
    const int k = e / D, d = e - k * D;
    const float av = an[e];
    float acc = 0.f;
    if (MODE == 1) {
      for (int j = 0; j < W1; ++j) {
        const EuclidCoef kc = euclid_coef(Tn[j * W2 + k], gn[j * W2 + k]);
        acc += -euclid_tt_exact(kc.c, kc.den, qn[(size_t)j * D + d] - av);
      }
    } else {
      const float nrm1 = n1n[k];
      for (int j = 0; j < W1; ++j) {
        const float nrm0 = n0n[j];
        acc += gn[j * W2 + k] * (qn[(size_t)j * D + d] / nrm0 / nrm1 -
                                 av * Tn[j * W2 + k] / (nrm1 * nrm1));
      }
    }
    dan[e] = acc;
  }
}

// Tiled backward for general W1 x W2 (the fast path when the per-pair tables fit
// LDS).  One workgroup per (pair, 32-wide d chunk):
//   * per-(j,k) coefficient tables are built ONCE per workgroup in LDS
//     (Euclid: c, den, 1/den; cosine: g, 1/(n0 n1), T/n0^2, T/n1^2);
//   * the q / a chunk is staged in LDS (stride 33: conflict-free);
//   * a thread owns one (j,d) of dq and walks k ascending, then one (k,d) of da
//     walking j ascending -- the reference's accumulation order (:209-223).
// Euclid stays bit-exact (euclid_tt's self-checking reciprocal path).  Cosine
// multiplies by precomputed reciprocals instead of dividing per term: it is
// held to 1e-5 like everything that is BLAS-ordered in the reference.
constexpr int kBwdDC = 32;

template <int MODE, bool EXACT>
__global__ __launch_bounds__(256) void cross_bwd_tiled_kernel(
    const float* __restrict__ q, const float* __restrict__ a,
    const float* __restrict__ top, const float* __restrict__ top_diff,
    const float* __restrict__ norm0, const float* __restrict__ norm1,
    float* __restrict__ dq, float* __restrict__ da, int W1, int W2, int D, int nchunks, int split) {
  extern __shared__ double lds_d[];
  constexpr int LS = kBwdDC + 1;
  // split: blockIdx.x = (n * nchunks + chunk) * 2 + pass -- the dq pass and the da pass of one
  // (pair, chunk) run as separate workgroups (twice the parallelism; small batches).
  // Otherwise one workgroup does both and the tables are built once (large batches).
  const int bid = split ? (blockIdx.x >> 1) : blockIdx.x;
  const bool do_dq = !split || (blockIdx.x & 1) == 0, do_da = !split || (blockIdx.x & 1) == 1;
  const int n = bid / nchunks, chunk = bid % nchunks;
  const int d0 = chunk * kBwdDC, dn = min(kBwdDC, D - d0);
  const int JK = W1 * W2;
  // carve: doubles first (8-byte aligned), then floats
  double* t_den = lds_d;                          // MODE 1: [JK]
  double* t_rcp = lds_d + (MODE == 1 ? JK : 0);   // MODE 1: [JK]
  float* fbase = reinterpret_cast<float*>(lds_d + (MODE == 1 ? 2 * JK : 0));
  float* t_c = fbase;                             // MODE 1: c       MODE 0: g
  float* t_i01 = fbase + JK;                      // MODE 0: 1/(n0 n1)
  float* t_b1 = fbase + 2 * JK;                   // MODE 0: T/n0^2
  float* t_b2 = fbase + 3 * JK;                   // MODE 0: T/n1^2
  float* qs = fbase + (MODE == 1 ? JK : 4 * JK);
  float* as = qs + W1 * LS;
  // fp32 backward arithmetic (include/mms.h): the double tables are not needed; fl32(1/den)
  // lives in their place
  float* t_r = reinterpret_cast<float*>(lds_d);

  const float* qn = q + (size_t)n * W1 * D;
  const float* an = a + (size_t)n * W2 * D;
  const float* Tn = top + (size_t)n * JK;
  const float* gn = top_diff + (size_t)n * JK;

  for (int e0 = threadIdx.x; MODE == 1 && e0 < JK; e0 += 256 * 8) {
    float tv[8], gv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int e = min(e0 + 256 * u, JK - 1); tv[u] = Tn[e]; gv[u] = gn[e]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 256 * u;
      if (e >= JK) break;
      const EuclidCoef k = euclid_coef(tv[u], gv[u]);
      t_c[e] = k.c;
      if (EXACT) { t_den[e] = k.den; t_rcp[e] = k.rcp; } else { t_r[e] = (float)k.rcp; }
    }
  }
  for (int e = threadIdx.x; MODE != 1 && e < JK; e += 256) {
    if (MODE == 1) {
    } else {
      const int j = e / W2, kk = e - j * W2;
      const float n0 = norm0[(size_t)n * W1 + j], n1 = norm1[(size_t)n * W2 + kk];
      t_c[e] = gn[e];
      t_i01[e] = 1.0f / n0 / n1;
      t_b1[e] = Tn[e] / (n0 * n0);
      t_b2[e] = Tn[e] / (n1 * n1);
    }
  }
  // eight unconditional (clamped) loads per thread in flight before the first LDS write; a rolled
  // `ok ? load : 0` loop paid one memory round trip per iteration
  auto stage = [&](const float* src, float* dst, int W) {
    for (int base = 0; base < W * kBwdDC; base += 256 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + threadIdx.x + 256 * u;
        v[u] = src[(size_t)min(e >> 5, W - 1) * D + min(d0 + (e & 31), D - 1)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + threadIdx.x + 256 * u;
        if (e < W * kBwdDC) dst[(e >> 5) * LS + (e & 31)] = (e & 31) < dn ? v[u] : 0.f;
      }
    }
  };
  stage(qn, qs, W1);
  stage(an, as, W2);
  __syncthreads();

  float* dqn = dq + (size_t)n * W1 * D;
  float* dan = da + (size_t)n * W2 * D;
  if (MODE == 1 && !EXACT) {
    // fp32 arithmetic: a thread owns FOUR consecutive d of one row, so the per-(j,k) coefficients
    // c and fl32(1/den) are read from LDS once per four terms (6 LDS reads per 4 terms instead of
    // 12: this loop is LDS-bandwidth-bound); every sum still runs over k (or j) ascending.
    for (int e = threadIdx.x; do_dq && e < W1 * (kBwdDC / 4); e += 256) {
      const int j = e >> 3, dd0 = (e & 7) * 4;
      if (dd0 >= dn) continue;
      float qv[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) qv[u] = qs[j * LS + dd0 + u];
      for (int k = 0; k < W2; ++k) {
        const float c = t_c[j * W2 + k], r = t_r[j * W2 + k];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (c * (qv[u] - as[k * LS + dd0 + u])) * r;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (dd0 + u < dn) dqn[(size_t)j * D + d0 + dd0 + u] = acc[u];
    }
    for (int e = threadIdx.x; do_da && e < W2 * (kBwdDC / 4); e += 256) {
      const int k = e >> 3, dd0 = (e & 7) * 4;
      if (dd0 >= dn) continue;
      float av[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u) av[u] = as[k * LS + dd0 + u];
      for (int j = 0; j < W1; ++j) {
        const float c = t_c[j * W2 + k], r = t_r[j * W2 + k];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += -((c * (qs[j * LS + dd0 + u] - av[u])) * r);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (dd0 + u < dn) dan[(size_t)k * D + d0 + dd0 + u] = acc[u];
    }
    return;
  }
  for (int e = threadIdx.x; do_dq && e < W1 * kBwdDC; e += 256) {
    const int j = e >> 5, dd = e & 31;
    if (dd >= dn) continue;
    const float qv = qs[j * LS + dd];
    float acc = 0.f;
    for (int k = 0; k < W2; ++k) {
      const int t = j * W2 + k;
      const float av = as[k * LS + dd];
      if (MODE == 1 && EXACT) {
        EuclidCoef kc;
        kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
        acc += euclid_tt(kc, qv - av);
      } else if (MODE == 1) {
        acc += (t_c[t] * (qv - av)) * t_r[t];
      } else {
        acc += t_c[t] * (av * t_i01[t] - qv * t_b1[t]);
      }
    }
    dqn[(size_t)j * D + d0 + dd] = acc;
  }
  for (int e = threadIdx.x; do_da && e < W2 * kBwdDC; e += 256) {
    const int k = e >> 5, dd = e & 31;
    if (dd >= dn) continue;
    const float av = as[k * LS + dd];
    float acc = 0.f;
    for (int j = 0; j < W1; ++j) {
      const int t = j * W2 + k;
      const float qv = qs[j * LS + dd];
      if (MODE == 1 && EXACT) {
        EuclidCoef kc;
        kc.c = t_c[t]; kc.den = t_den[t]; kc.rcp = t_rcp[t];
        acc += -euclid_tt(kc, qv - av);
      } else if (MODE == 1) {
        acc += -((t_c[t] * (qv - av)) * t_r[t]);
      } else {
        acc += t_c[t] * (qv * t_i01[t] - av * t_b2[t]);
      }
    }
    dan[(size_t)k * D + d0 + dd] = acc;
  }
}

static size_t cross_bwd_tiled_lds(int mode, int W1, int W2) {
  const size_t JK = (size_t)W1 * W2;
  const size_t tables = mode == 1 ? JK * (8 + 8 + 4) : JK * 16;
  return tables + (size_t)(W1 + W2) * (kBwdDC + 1) * sizeof(float) + 16;
}

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

// ================================ dispatch ==================================

template <int MODE>
static void launch_cross_fwd(const float* q, const float* a, const float* n0,
                             const float* n1, float* top, int N, int W1, int W2,
                             int D, hipStream_t s, CrossGather gt = CrossGather{nullptr, nullptr, 0, nullptr}) {
  // Register tile per lane: as large as possible (fewer LDS reads per flop) while the
  // launch still has enough waves to occupy the chip (small N: smaller tiles, more waves).
  auto r_cap = [](int w, int cap) { int r = (w + 7) / 8; return r > cap ? cap : r; };
  int rj = 1, rk = 1, tilesJ = 1, tilesK = 1;
  for (int cap = 5; cap >= 1; --cap) {
    rj = r_cap(W1, cap); rk = r_cap(W2, cap);
    tilesJ = (W1 + 8 * rj - 1) / (8 * rj); tilesK = (W2 + 8 * rk - 1) / (8 * rk);
    if ((long long)N * tilesJ * tilesK >= 1024) break;
  }
  const long long work = (long long)N * tilesJ * tilesK;
  // small D: the whole pair as one LDS image per wave (cross_fwd_image_kernel)
  {
    auto gcd64 = [](int d) { int g = 64; while (d % g) g >>= 1; return g; };
    const size_t img = (size_t)(W1 + W2) * D * sizeof(float);
    constexpr int DI = 50;   // the driver's default embedding width (do_trec_qa_clean.py -d 50)
    const bool fits = W1 % 8 == 0 && W2 % 8 == 0 && W1 / 8 <= 5 && W2 / 8 <= 5 && N >= 1024 &&
                      D == DI && aligned16(q) && aligned16(a) && gcd64(D) <= 8 && 2 * img <= 64 * 1024;
    static_assert(DI % 2 == 0, "gather copies float2");
    if (fits) {
      const unsigned g2 = (unsigned)((N + 1) / 2);
#define MMS_IMG_CASE(J, K)                                                                      \
  if (W1 == 8 * J && W2 == 8 * K) {                                                             \
    hipLaunchKernelGGL((cross_fwd_image_kernel<J, K, MODE, DI>), dim3(g2), dim3(128), 2 * img,  \
                       s, q, a, n0, n1, top, N, gt);                                            \
    return;                                                                                     \
  }
#define MMS_IMG_ROW(J) MMS_IMG_CASE(J, 1) MMS_IMG_CASE(J, 2) MMS_IMG_CASE(J, 3) MMS_IMG_CASE(J, 4) MMS_IMG_CASE(J, 5)
      MMS_IMG_ROW(1) MMS_IMG_ROW(2) MMS_IMG_ROW(3) MMS_IMG_ROW(4) MMS_IMG_ROW(5)
#undef MMS_IMG_ROW
#undef MMS_IMG_CASE
    }
  }
  const unsigned grid = (unsigned)((work + 3) / 4);
#define MMS_CROSS_CASE(J, K)                                                        \
  if (rj == J && rk == K) {                                                         \
    hipLaunchKernelGGL((cross_fwd_kernel<J, K, MODE>), dim3(grid), dim3(256), 0, s, \
                       q, a, n0, n1, top, N, W1, W2, D, tilesJ, tilesK, gt);        \
    return;                                                                         \
  }
#define MMS_CROSS_ROW(J) MMS_CROSS_CASE(J, 1) MMS_CROSS_CASE(J, 2) MMS_CROSS_CASE(J, 3) \
                         MMS_CROSS_CASE(J, 4) MMS_CROSS_CASE(J, 5)
  MMS_CROSS_ROW(1) MMS_CROSS_ROW(2) MMS_CROSS_ROW(3) MMS_CROSS_ROW(4) MMS_CROSS_ROW(5)
#undef MMS_CROSS_ROW
#undef MMS_CROSS_CASE
}

// =============================== entry points ===============================
// DESIGN.md 4.4b is the table this section is read against.  W1 == W2 == 1 tries simcross_rows.hip (Euclid) or
// simcross_rows_cosine.hip first.

// The word-grid forward; gt.iq != nullptr: q and a are the embedding table and the Embed gather is fused in.
static void cross_forward(int mode, int N, int W1, int W2, int D, const float* q, const float* a, float* top,
                          float* norm0, float* norm1, hipStream_t s, CrossGather gt) {
  if (mode == 1) {
    launch_cross_fwd<1>(q, a, nullptr, nullptr, top, N, W1, W2, D, s, gt);
    return;
  }
  const long long r0 = (long long)N * W1, r1 = (long long)N * W2;
  hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((r0 + 3) / 4)), dim3(256), 0, s, q, norm0, r0, D, gt.iq, gt.K, gt.bias);
  hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)((r1 + 3) / 4)), dim3(256), 0, s, a, norm1, r1, D, gt.ia, gt.K, gt.bias);
  launch_cross_fwd<0>(q, a, norm0, norm1, top, N, W1, W2, D, s, gt);
}

// The word-grid backward: lane kernel (Euclid, narrow grids, many pairs), else tiled, else plain.
static void cross_backward(int mode, int N, int W1, int W2, int D, const float* q, const float* a, const float* top,
                           const float* top_diff, const float* norm0, const float* norm1, float* dq, float* da,
                           bool exact, hipStream_t s) {
  const int nchunks = (D + kBwdDC - 1) / kBwdDC;
  if (mode == 1) norm0 = norm1 = nullptr;                          // Euclid caches no norms
  if (mode == 1 && cross_bwd_lane_ok(exact, N, W1, W2, D)) {
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
  } else if (cross_bwd_tiled_lds(mode, W1, W2) <= 64 * 1024 && 2LL * N * nchunks <= 0x7fffffffLL) {
    const size_t lds = cross_bwd_tiled_lds(mode, W1, W2);
    const int split = ((long long)N * nchunks < 1024) ? 1 : 0;     // fill the chip when the batch is small
    const unsigned grid = (unsigned)((split ? 2LL : 1LL) * N * nchunks);
    // cosine has one arithmetic: its instance is <0, true>
    const auto k = mode == 0 ? cross_bwd_tiled_kernel<0, true>
                   : exact   ? cross_bwd_tiled_kernel<1, true> : cross_bwd_tiled_kernel<1, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, s, q, a, top, top_diff, norm0, norm1, dq, da, W1, W2, D,
                       nchunks, split);
  } else {
    hipLaunchKernelGGL((mode == 1 ? cross_bwd_kernel<1> : cross_bwd_kernel<0>), dim3(N), dim3(256), 0, s, q, a, top,
                       top_diff, norm0, norm1, dq, da, W1, W2, D);
  }
}

static bool rows_geometry(int W1, int W2) { return W1 == 1 && W2 == 1; }

int simcross_elementwise_forward(int mode, int N, int W1, int W2, int D,
                                 const float* q, const float* a, float* top,
                                 float* norm0, float* norm1, hipStream_t s) {
  if (N == 0) return MMS_OK;
  const bool rows = rows_geometry(W1, W2);
  if (rows && mode == 0)
    launch_cosine_rows<true, false>(N, D, q, a, nullptr, top, norm0, norm1, nullptr, nullptr, s);
  else if (!(rows && launch_euclid_rows<true, false>(N, D, q, a, nullptr, nullptr, top, nullptr, nullptr, false, s)))
    cross_forward(mode, N, W1, W2, D, q, a, top, norm0, norm1, s, CrossGather{nullptr, nullptr, 0, nullptr});
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
  cross_forward(mode, N, W1, W2, D, weight, weight, top, norm0, norm1, s, CrossGather{index_q, index_a, K, embed_bias});
  return launch_status();
}

// `exact`: euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE, read once by the entry point
static int backward_with_mode(int mode, int N, int W1, int W2, int D, const float* q, const float* a,
                              const float* top, const float* top_diff, const float* norm0, const float* norm1,
                              float* dq, float* da, bool exact, hipStream_t s) {
  if (!rows_geometry(W1, W2))
    cross_backward(mode, N, W1, W2, D, q, a, top, top_diff, norm0, norm1, dq, da, exact, s);
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
