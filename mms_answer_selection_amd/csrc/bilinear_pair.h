// csrc/bilinear_pair.h -- the three fused word-grid kernels of SimCross dist_mode 2 (T_nm = Q_n W_m A_n^T + bias_m) and
// the host decisions that pick them: the one definition shared by the fp32 layer (bilinear.hip) and the fp16-storage
// calls (bilinear_f16.hip).  The kernels are templated over the STORAGE type of q and a (and of the gathered embedding
// table), TIn, and of the dq / da outputs, TG: float or _Float16.  The element type appears in the staging loads and in
// the gradient stores and nowhere else -- the zero-padded fp32 LDS images (row stride 68), the item schedule and every
// MFMA are one definition, so a half instantiation carries the bits of the float one run on the widened operands.
#ifndef MMS_BILINEAR_PAIR_H_
#define MMS_BILINEAR_PAIR_H_

#include <type_traits>

#include "euclid_math.h"
#include "mms_common.h"

namespace mms {

// ------------------------------ workspace layout ----------------------------
// the word grids the fused per-(pair, measure) kernels stage whole in LDS (bilinear_pair_bwd_kernel,
// bilinear_pairm_fwd_kernel): image row stride, most words per sentence, widest embedding
constexpr int FB_LS = 68, FB_W = 48, FB_D = 64;
// does the fused per-pair backward (and its forward twin) take this shape?  Sizes the workspace AND picks the kernel.
inline bool pair_bwd_eligible(int N, int W1, int W2, int D, int M) {
  return W1 <= FB_W && W2 <= FB_W && D <= FB_D && W1 * W2 > 1 && N <= 256 && (long long)N * M <= 65535;
}

struct BilinearWs {
  size_t u_off, v_off, part_off, mpart_off, mpart2_off, total;
  size_t sm_off;                 // bilinear_as_simmatrix: [Q.W, N x D] at 0, SimMatrix's own workspace from here
  int ksplit, kchunk;
};
BilinearWs bilinear_ws(int N, int W1, int W2, int D, int M);      // bilinear.hip

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
// Eligible for W1, W2 <= 48 and D <= 64; anything else takes the two batched GEMMs of bilinear.hip.
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

// ---- half staging: the q and a images of one pair from IEEE halves -------------------------------
// The images are what the float kernels build -- element (r, c) of the pair at [r * LS + c], zero beyond W rows and D
// columns -- with every half widened exactly on its way to LDS.  A pair's W x D block is contiguous, so it is read as a
// flat run of VW-half vectors whatever D is (D = 50: a 16-byte load holds 8 halves of one or two rows); with the
// gather a vector lies inside one table row.  VW is the widest of 8, 2, 1 that both operands allow (half_stage_width:
// every vector aligned and whole); all loads of both images are issued, clamped and unconditional, before the first
// LDS write.  Thread t owns vectors t, t + NT, ...; the padding is written by whoever owns its LDS slot.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

template <int VW>
__device__ __forceinline__ void load_halves(const _Float16* p, _Float16 (&h)[VW]) {
  static_assert(VW == 8 || VW == 2 || VW == 1, "16-, 4- or 2-byte loads");
  if constexpr (VW == 8) {
    const half8 x = *reinterpret_cast<const half8*>(p);
#pragma unroll
    for (int u = 0; u < 8; ++u) h[u] = x[u];
  } else if constexpr (VW == 2) {
    const half2v x = *reinterpret_cast<const half2v*>(p);
    h[0] = x[0];
    h[1] = x[1];
  } else {
    h[0] = *p;
  }
}

// block-uniform: halves per load for images whose first elements are qn and an (the table, twice, with the gather)
__device__ __forceinline__ int half_stage_width(const _Float16* qn, const _Float16* an, int W1, int W2, int D, bool gather) {
  const unsigned addr = (unsigned)reinterpret_cast<uintptr_t>(qn) | (unsigned)reinterpret_cast<uintptr_t>(an);
  const int len = gather ? D : ((W1 * D) | (W2 * D));           // every vector whole: VW divides both lengths
  if ((addr & 15) == 0 && (len & 7) == 0) return 8;
  if ((addr & 3) == 0 && (len & 1) == 0) return 2;
  return 1;
}

template <int VW, int ROWS, int LS, int NT>
__device__ __forceinline__ void stage_half_images_vw(float* __restrict__ qs, float* __restrict__ as, const _Float16* qn,
                                                     const _Float16* an, int n, int W1, int W2, int D, int t,
                                                     const PairGather& g) {
  constexpr int NV = (ROWS * 64 / VW + NT - 1) / NT;            // vectors of one image per thread at D = 64
  const int eq_n = W1 * D, ea_n = W2 * D;
  _Float16 hq[NV][VW], ha[NV][VW];
  float bb[NV][VW];
  if (g.iq) {                                                   // ids first (all in flight), then the table rows
    float fq[NV], fa[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int row = VW * (NT * u + t) / D;
      fq[u] = g.iq[(size_t)n * W1 + min(row, W1 - 1)];
      fa[u] = g.ia[(size_t)n * W2 + min(row, W2 - 1)];
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = VW * (NT * u + t), row = e / D, c = e - row * D;
      load_halves<VW>(qn + (size_t)pair_gather_id(fq[u], g.K) * D + c, hq[u]);
      load_halves<VW>(an + (size_t)pair_gather_id(fa[u], g.K) * D + c, ha[u]);
#pragma unroll
      for (int k = 0; k < VW; ++k) bb[u][k] = g.bias ? g.bias[c + k] : 0.f;
    }
  } else {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = VW * (NT * u + t);
      load_halves<VW>(qn + min(e, eq_n - VW), hq[u]);
      load_halves<VW>(an + min(e, ea_n - VW), ha[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int e = VW * (NT * u + t);
    int row = e / D, c = e - row * D;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      float fq = (float)hq[u][k], fa = (float)ha[u][k];
      if (g.iq && g.bias) { fq = bb[u][k] + fq; fa = bb[u][k] + fa; }
      if (e < eq_n) qs[row * LS + c] = fq;
      if (e < ea_n) as[row * LS + c] = fa;
      if (++c == D) { c = 0; ++row; }
    }
  }
}

template <int ROWS, int LS, int NT>
__device__ __forceinline__ void stage_half_images(float* __restrict__ qs, float* __restrict__ as, const _Float16* qn,
                                                  const _Float16* an, int n, int W1, int W2, int D, int t,
                                                  const PairGather& g) {
  const int vw = half_stage_width(qn, an, W1, W2, D, g.iq != nullptr);
  if (vw == 8) stage_half_images_vw<8, ROWS, LS, NT>(qs, as, qn, an, n, W1, W2, D, t, g);
  else if (vw == 2) stage_half_images_vw<2, ROWS, LS, NT>(qs, as, qn, an, n, W1, W2, D, t, g);
  else stage_half_images_vw<1, ROWS, LS, NT>(qs, as, qn, an, n, W1, W2, D, t, g);
  constexpr int NE = (ROWS * LS + NT - 1) / NT;
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = NT * u + t;
    const int r = e / LS, c = e - r * LS;
    if (e < ROWS * LS) {
      if (!(r < W1 && c < D)) qs[e] = 0.f;
      if (!(r < W2 && c < D)) as[e] = 0.f;
    }
  }
}

template <int KS, class TIn>                       // k steps of 4: 13 covers D <= 52 (the driver's 50), 16 D <= 64
__global__ __launch_bounds__(256) void bilinear_pair_fwd_kernel(
    int N, int W1, int W2, int D, int M, const TIn* __restrict__ q, const TIn* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ top,
    PairGather g = PairGather{nullptr, nullptr, 0, nullptr}) {
  __shared__ float qs[PF_ROWS * PF_LS];
  __shared__ float as[PF_ROWS * PF_LS];
  __shared__ float ts[4][16 * PF_LS];
  const int n = blockIdx.x;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const TIn* qn = q + (size_t)n * W1 * D;
  const TIn* an = a + (size_t)n * W2 * D;
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
  if constexpr (std::is_same<TIn, float>::value) {
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
  } else {
    stage_half_images<PF_ROWS, PF_LS, 256>(qs, as, g.iq ? q : qn, g.iq ? a : an, n, W1, W2, D, t, g);
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
// TG: what mq / ma hold -- float partials, or (one measure, half storage) the dq / da halves themselves, each element
// rounded once (RNE) as it is stored.
template <int KSW, int KSD, class TIn, class TG>
__global__ __launch_bounds__(512) void bilinear_pair_bwd_kernel(
    int N, int W1, int W2, int D, int M, const TIn* __restrict__ q, const TIn* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ top_diff, TG* __restrict__ mq,
    TG* __restrict__ ma, float* __restrict__ wpart) {
  __shared__ float qs[FB_W * FB_LS], as[FB_W * FB_LS], ts[FB_W * FB_LS], ws[FB_D * FB_LS];
  __shared__ float us[FB_W * FB_LS], vs[FB_W * FB_LS];
  const int n = blockIdx.x / M, m = blockIdx.x - n * M;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  const TIn* qn = q + (size_t)n * W1 * D;
  const TIn* an = a + (size_t)n * W2 * D;
  const float* Wm = W + (size_t)m * D * D;
  const float* dT = top_diff + ((size_t)n * M + m) * W1 * W2;
  // zero-padded images: every load issued (clamped, unconditional) before the first LDS write
  constexpr int NT = 512, NWV = NT / 64;
  constexpr int NE = (FB_W * FB_LS + NT - 1) / NT, NEW = (FB_D * FB_LS + NT - 1) / NT;
  if constexpr (std::is_same<TIn, float>::value) {
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
  } else {
    // the two fp32 images first, then the halves: all four in flight before the first LDS write
    float vt[NE], vw[NEW];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vt[u] = dT[(size_t)min(row, W1 - 1) * W2 + min(c, W2 - 1)];
    }
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vw[u] = Wm[(size_t)min(row, D - 1) * D + min(c, D - 1)];
    }
    stage_half_images<FB_W, FB_LS, NT>(qs, as, qn, an, n, W1, W2, D, t, PairGather{nullptr, nullptr, 0, nullptr});
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      if (e < FB_W * FB_LS) {
        ts[e] = (row < W1 && c < W2) ? vt[u] : 0.f;
        us[e] = 0.f;
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
  TG* mqn = mq + ((size_t)m * N + n) * W1 * D;          // [M][N*W1][D]
  TG* man = ma + ((size_t)m * N + n) * W2 * D;          // [M][N*W2][D]
  float* wpn = wpart + ((size_t)n * M + m) * D * D;     // [N][M][D][D]
  auto put_global = [&](auto* dst, int ld, int rows, int cols, int i0, int j0, const v4f& acc) {
    typedef typename std::remove_pointer<decltype(dst)>::type TO;
    const int col = j0 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = i0 + 4 * g + j;
      if (row < rows && col < cols) dst[(size_t)row * ld + col] = (TO)acc[j];
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
template <int KSD, class TIn>
__global__ __launch_bounds__(512) void bilinear_pairm_fwd_kernel(
    int N, int W1, int W2, int D, int M, const TIn* __restrict__ q, const TIn* __restrict__ a,
    const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ top,
    PairGather gth = PairGather{nullptr, nullptr, 0, nullptr}) {
  __shared__ float qs[FB_W * FB_LS], as[FB_W * FB_LS], ws[FB_D * FB_LS], ps[FB_W * FB_LS];
  constexpr int NT = 512, NWV = NT / 64;
  const int n = blockIdx.x / M, m = blockIdx.x - n * M;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  const TIn* qn = q + (size_t)n * W1 * D;
  const TIn* an = a + (size_t)n * W2 * D;
  const float* Wm = W + (size_t)m * D * D;
  constexpr int NE = (FB_W * FB_LS + NT - 1) / NT, NEW = (FB_D * FB_LS + NT - 1) / NT;
  if constexpr (std::is_same<TIn, float>::value) {
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
  } else {
    float vw[NEW];                                 // W_m's image first, then the halves: all in flight together
#pragma unroll
    for (int u = 0; u < NEW; ++u) {
      const int e = NT * u + t, row = e / FB_LS, c = e - row * FB_LS;
      vw[u] = Wm[(size_t)min(row, D - 1) * D + min(c, D - 1)];
    }
    stage_half_images<FB_W, FB_LS, NT>(qs, as, gth.iq ? q : qn, gth.iq ? a : an, n, W1, W2, D, t, gth);
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = NT * u + t;
      if (e < FB_W * FB_LS) ps[e] = 0.f;
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

// ---- which fused kernel takes a shape: one definition per decision ----
enum { PAIR_FWD_NONE = 0, PAIR_FWD_EVAL = 1, PAIR_FWD_TRAIN = 2 };
// evaluation batches: one workgroup per pair; training batches: one per (pair, measure); else the GEMM route
inline int pair_fwd_route(int N, int W1, int W2, int D, int M) {
  if (W1 <= PF_ROWS && W2 <= PF_ROWS && D <= 16 * PF_TD && W1 * W2 > 1 && N >= 512) return PAIR_FWD_EVAL;
  if (pair_bwd_eligible(N, W1, W2, D, M)) return PAIR_FWD_TRAIN;
  return PAIR_FWD_NONE;
}

// The fused word-grid forward, when one of its two kernels takes the shape: one workgroup per pair for large batches
// (evaluation: the 1517 TREC-QA test candidates, 89 -> 59 us), one per (pair, measure) for training batches -- at 50
// pairs the per-pair form and the two small GEMMs both sit at the launch floor.  `g`: Embed fused in (q = a = the table).
// Returns whether it launched.
template <class TIn>
inline bool pair_fwd_launch(int N, int W1, int W2, int D, int M, const TIn* q, const TIn* a, const float* W,
                            const float* bias, float* top, hipStream_t s,
                            const PairGather g = PairGather{nullptr, nullptr, 0, nullptr}) {
  const int route = pair_fwd_route(N, W1, W2, D, M);
  if (route == PAIR_FWD_EVAL) {
    if (D <= 52)
      hipLaunchKernelGGL((bilinear_pair_fwd_kernel<13, TIn>), dim3(N), dim3(256), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    else
      hipLaunchKernelGGL((bilinear_pair_fwd_kernel<16, TIn>), dim3(N), dim3(256), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    return true;
  }
  if (route == PAIR_FWD_TRAIN) {
    if (D <= 52)
      hipLaunchKernelGGL((bilinear_pairm_fwd_kernel<13, TIn>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    else
      hipLaunchKernelGGL((bilinear_pairm_fwd_kernel<16, TIn>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W, bias, top, g);
    return true;
  }
  return false;
}

// The fused backward of a pair_bwd_eligible shape: per-(pair, measure) partials of dQ and dA to mq / ma ([M][N*W][D];
// with one measure these ARE dq and da), of dW to wpart ([N][M][D][D]).
template <class TIn, class TG>
inline void pair_bwd_launch(int N, int W1, int W2, int D, int M, const TIn* q, const TIn* a, const float* W,
                            const float* top_diff, TG* mq, TG* ma, float* wpart, hipStream_t s) {
  if (W1 <= 40 && W2 <= 40 && D <= 52)           // the driver's geometry: 10 / 13 k-steps
    hipLaunchKernelGGL((bilinear_pair_bwd_kernel<10, 13, TIn, TG>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W,
                       top_diff, mq, ma, wpart);
  else
    hipLaunchKernelGGL((bilinear_pair_bwd_kernel<12, 16, TIn, TG>), dim3(N * M), dim3(512), 0, s, N, W1, W2, D, M, q, a, W,
                       top_diff, mq, ma, wpart);
}

}  // namespace mms
#endif  // MMS_BILINEAR_PAIR_H_
