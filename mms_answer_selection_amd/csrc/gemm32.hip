// csrc/gemm32.hip -- the fp32-MFMA GEMM toolbox of the learned-metric paths (bilinear.hip, simmatrix.hip; declared
// in gemm32.h): strided / batched / split-K products C = A B, several small ones as one launch, and the element-wise
// kernels both sources launch around them (ordered split-K reduction, row dot, row scale).
//
// It stands where the reference calls cblas_sgemm / caffe_cpu_gemm once per pair or per (pair, measure) on the host:
//   sim_cross_layer.cpp:148-158 (fwd), :286-299 (bwd)    sim_matrix_layer.cpp:60-64 (fwd), :73-80, :88 (bwd)
// What is multiplied with what, and why, is the callers' business (their headers); fp32 rounding differs from the
// reference's (as it does between BLAS libraries), tests hold it to 1e-5.
//
// Every product here uses v_mfma_f32_32x32x2_f32: fp32 in, fp32 accumulate, each MFMA bit-equal to a k-ordered fmaf
// chain.  (The bf16-pipe and fp32 panel kernels that serve SimMatrix's large products are bx3_gemm.h / panel_gemm.h.)
// Deterministic: split-K partial slabs are summed in a fixed order, no atomics.
#include "gemm32.h"

namespace mms {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, BK = 16;
constexpr int LSA = BM + 4, LSB = BN + 4;

// 256 threads = 4 waves stacked along M; wave w owns rows [32w,32w+32) x 64 cols
// = two 32x32 MFMA tiles.  LDS tiles are k-major so a fragment read is 32
// consecutive floats per half-wave (conflict-free).
__global__ __launch_bounds__(256) void gemm32_kernel(GemmArgs g) {
  __shared__ float As[BK * LSA];
  __shared__ float Bs[BK * LSB];

  const int z = blockIdx.z;
  const int ks = z % g.ksplit;
  const int b1 = (z / g.ksplit) % g.nb1;
  const int b0 = (z / g.ksplit) / g.nb1;
  const float* A = g.A + b0 * g.a_b0 + b1 * g.a_b1;
  const float* B = g.B + b0 * g.b_b0 + b1 * g.b_b1;
  float* C = g.C + b0 * g.c_b0 + b1 * g.c_b1 + ks * g.c_ks;
  int kbeg = ks * g.kchunk;
  int kend = min(g.K, kbeg + g.kchunk);
  if (g.ks_stacked) { A += ks * g.a_ks; B += ks * g.b_ks; kbeg = 0; kend = g.K; }
  const int i0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;

  // staging registers: A tile 128x16 -> 8 per thread, B tile 16x64 -> 4 per thread
  float ra[8], rb[4];
  bool oka[8], okb[4];
  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      int i, k;
      if (g.a_ifast) { i = t & 127; k = (t >> 7) + 2 * p; }
      else { k = t & 15; i = (t >> 4) + 16 * p; }
      const int gi = i0 + i, gk = k0 + k;
      // clamped, unconditional load; zeroed at the LDS store (as `ok ? load : 0` the loads are
      // emitted one by one, each waited for: see the fast kernel below)
      oka[p] = gi < g.M && gk < kend;
      ra[p] = A[(long long)min(gi, g.M - 1) * g.a_rs + (long long)min(gk, g.K - 1) * g.a_cs];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      int j, k;
      if (g.b_jfast) { j = t & 63; k = (t >> 6) + 4 * p; }
      else { k = t & 15; j = (t >> 4) + 16 * p; }
      const int gj = j0 + j, gk = k0 + k;
      okb[p] = gj < g.N && gk < kend;
      rb[p] = B[(long long)min(gk, g.K - 1) * g.b_rs + (long long)min(gj, g.N - 1) * g.b_cs];
    }
  };
  auto store_tiles = [&]() {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      int i, k;
      if (g.a_ifast) { i = t & 127; k = (t >> 7) + 2 * p; }
      else { k = t & 15; i = (t >> 4) + 16 * p; }
      As[k * LSA + i] = oka[p] ? ra[p] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      int j, k;
      if (g.b_jfast) { j = t & 63; k = (t >> 6) + 4 * p; }
      else { k = t & 15; j = (t >> 4) + 16 * p; }
      Bs[k * LSB + j] = okb[p] ? rb[p] : 0.f;
    }
  };

  v16f acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

  if (kbeg < kend) {
    load_tiles(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
      __syncthreads();
      store_tiles();
      __syncthreads();
      if (k0 + BK < kend) load_tiles(k0 + BK);
      const int ar = wave * 32 + (lane & 31), kh = lane >> 5;
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        const float av = As[(kk + kh) * LSA + ar];
        const float bv0 = Bs[(kk + kh) * LSB + (lane & 31)];
        const float bv1 = Bs[(kk + kh) * LSB + 32 + (lane & 31)];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv1, acc1, 0, 0, 0);
      }
    }
  }

  // C/D layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  const float* rs = g.rowscale ? g.rowscale + b0 * g.rs_b0 : nullptr;
  const float* ad = g.addend ? g.addend + b1 * g.ad_b1 : nullptr;
  // everything the epilogue reads is requested before its first store (see gemm32_fast_tile)
  float rsv[16] = {}, adv[2][16] = {}, cv[2][16] = {};
  if (rs || ad || g.beta_one) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int gi = i0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const long long gic = gi < g.M ? gi : g.M - 1;
      rsv[r] = rs ? rs[gic] : 1.0f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int gj = j0 + 32 * h + (lane & 31);
        const long long gjc = gj < g.N ? gj : g.N - 1;
        adv[h][r] = ad ? ad[gic * g.ldc + gjc] : 0.f;
        cv[h][r] = g.beta_one ? C[gic * g.ldc + gjc] : 0.f;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    asm volatile("" : "+v"(rsv[r]), "+v"(adv[0][r]), "+v"(adv[1][r]), "+v"(cv[0][r]), "+v"(cv[1][r]));   // in registers HERE
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gi = i0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (gi >= g.M) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int gj = j0 + 32 * h + (lane & 31);
      if (gj >= g.N) continue;
      float v = h ? acc1[r] : acc0[r];
      if (rs) v = rsv[r] * v;
      if (ad) v = adv[h][r] + v;
      float* c = C + gi * g.ldc + gj;
      if (g.beta_one) v = v + cv[h][r];
      *c = v;
    }
  }
}

// ---- fast path: 64x64x16 tiles, 16-byte global loads, permuted-k fragments --
// Eligible when each operand is contiguous in one direction with 16-byte
// alignment (A along k or along i, B along j or along k) -- true for every
// large GEMM of the callers at D = 300 / 1024.  Differences from the generic
// kernel above:
//   * FK/16 float4 global loads per operand per thread per k-tile, issued for the
//     NEXT tile before the MFMAs of the current one; pointers are bumped, no
//     64-bit multiplies in the loop;
//   * A lives in LDS as [i][k] (k contiguous, row stride 20 floats).  A
//     32x32x2 MFMA consumes two k values per instruction and the pairing is
//     free as long as A and B agree, so instruction t of a tile uses
//     k = t (lanes 0-31) and k = t + FK/2 (lanes 32-63): every lane's FK/2 A
//     values are then CONTIGUOUS -- FK/8 ds_read_b128, conflict-free at stride
//     FK+4 (20 or 36 floats) -- instead of FK/2 ds_read_b32;
//   * 4 waves as 2 x 2, each one 32x32 accumulator: at M = 16384, N = 300 the
//     grid is 256 x 5 = 1280 workgroups = exactly 5 per CU (no tail).
// FK = 16 measured faster than 32 at cfg 3 (43 vs 67 us for the 16384x300x300 product):
// the shallower tile keeps more workgroups' loads in flight per CU.
// The k-tile depth FK is a template parameter: 16 when several workgroups share a CU (cfg 3: their
// MFMA phases cover each other's barriers), 32 when a product is so small that a CU holds one or
// two workgroups and every tile boundary (LDS write -> barrier -> LDS read, ~0.3 us) is exposed --
// half as many boundaries for the driver's 32 x 40 x 40 x 300 bilinear products.
constexpr int FM = 64, FN = 64, LSJ = FN + 4;

// VW = floats per global load: 4 (16-byte-aligned rows, e.g. D = 300 / 1024) or 2 (8-byte-aligned rows:
// the driver's default D = 50, whose rows are 200 bytes).
// One 64x64 output tile of one product.  AKT / BJT: 1 or 0 fix the operand layouts at compile time (the
// single-product kernel below), -1 takes them from rt_ak / rt_bj (the grouped kernel, whose problems differ).
template <int AKT, int BJT, bool KSCALE, int FK, int VW>
__device__ __forceinline__ void gemm32_fast_tile(const GemmArgs& g, int bx, int by, int z, bool rt_ak,
                                                 bool rt_bj, float* As2base, float* Bs2base) {
  const bool A_KVEC = AKT < 0 ? rt_ak : (AKT != 0);
  const bool B_JVEC = BJT < 0 ? rt_bj : (BJT != 0);
  typedef float VT __attribute__((ext_vector_type(VW)));
  constexpr int LSK = FK + 4;
  constexpr int FSL = FK / (4 * VW);   // vector load slots per operand per thread per tile
  constexpr int KV = FK / VW;          // vectors along the k extent of a tile
  constexpr int JV = 64 / VW;          // vectors along the 64-wide extent of a tile
  constexpr int FH = FK / 2;           // k values per half-wave per tile
  const int ks = z % g.ksplit;
  const int b1 = (z / g.ksplit) % g.nb1;
  const int b0 = (z / g.ksplit) / g.nb1;
  const float* A = g.A + b0 * g.a_b0 + b1 * g.a_b1;
  const float* B = g.B + b0 * g.b_b0 + b1 * g.b_b1;
  float* C = g.C + b0 * g.c_b0 + b1 * g.c_b1 + ks * g.c_ks;
  int kbeg = ks * g.kchunk;
  int kend = min(g.K, kbeg + g.kchunk);
  if (g.ks_stacked) { A += ks * g.a_ks; B += ks * g.b_ks; kbeg = 0; kend = g.K; }
  const int i0 = by * FM, j0 = bx * FN;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;

  // this thread's load slots: FSL float4 per operand per tile
  int ai[FSL], ak[FSL], bj[FSL], bk[FSL];  // tile-local coordinates
#pragma unroll
  for (int sl = 0; sl < FSL; ++sl) {
    const int u = t + 256 * sl;
    if (A_KVEC) { ai[sl] = u / KV; ak[sl] = (u % KV) * VW; } else { ak[sl] = u / JV; ai[sl] = (u % JV) * VW; }
    if (B_JVEC) { bk[sl] = u / JV; bj[sl] = (u % JV) * VW; } else { bj[sl] = u / KV; bk[sl] = (u % KV) * VW; }
  }
  const float* pa[FSL];
  const float* pb[FSL];
  bool a_ok[FSL], b_ok[FSL];
#pragma unroll
  for (int sl = 0; sl < FSL; ++sl) {
    a_ok[sl] = i0 + ai[sl] < g.M;              // M % VW == 0 on the i-vector path
    b_ok[sl] = j0 + bj[sl] < g.N;              // N % VW == 0 on the j-vector path
    pa[sl] = A + (long long)(i0 + ai[sl]) * g.a_rs + (long long)(kbeg + ak[sl]) * g.a_cs;
    pb[sl] = B + (long long)(kbeg + bk[sl]) * g.b_rs + (long long)(j0 + bj[sl]) * g.b_cs;
  }
  const long long a_step = (long long)FK * g.a_cs, b_step = (long long)FK * g.b_rs;
  const float* ksc = g.bkscale;

  VT ra[FSL], rb[FSL];
  float sc[FSL];
  bool la[FSL], lb[FSL];                       // was the slot inside the matrix?
#pragma unroll
  for (int sl = 0; sl < FSL; ++sl) sc[sl] = 1.f;
  // Out-of-range slots load from a valid address (the operand's base) and are zeroed when they
  // are WRITTEN TO LDS.  `cond ? *p : zero` instead makes the compiler select between p and the
  // address of a private zero: flat loads through scratch, each followed by vmcnt(0) -- nothing
  // stays in flight behind the MFMAs.
  auto load = [&](int k0) {
#pragma unroll
    for (int sl = 0; sl < FSL; ++sl) {
      la[sl] = a_ok[sl] && k0 + ak[sl] < kend;
      lb[sl] = b_ok[sl] && k0 + bk[sl] < kend;
      ra[sl] = *reinterpret_cast<const VT*>(la[sl] ? pa[sl] : A);
      rb[sl] = *reinterpret_cast<const VT*>(lb[sl] ? pb[sl] : B);
      // the scale is only FETCHED here (clamped index, no dependent use): multiplying now
      // would put a vmcnt(0) wait in front of the MFMAs and drain the prefetch
      if (KSCALE) sc[sl] = ksc[min(k0 + bk[sl], g.K - 1)];
      pa[sl] += a_step;
      pb[sl] += b_step;
    }
  };
  auto store = [&](int buf) {
    float* As = As2base + buf * (FM * LSK);
    float* Bs = Bs2base + buf * (FK * LSJ);
    const VT zv = 0.f;
#pragma unroll
    for (int sl = 0; sl < FSL; ++sl) {
      if (!la[sl]) ra[sl] = zv;
      if (!lb[sl]) rb[sl] = zv;
      if (A_KVEC) {
        *reinterpret_cast<VT*>(&As[ai[sl] * LSK + ak[sl]]) = ra[sl];
      } else {
#pragma unroll
        for (int c = 0; c < VW; ++c) As[(ai[sl] + c) * LSK + ak[sl]] = ra[sl][c];
      }
      if (B_JVEC) {
        VT v = rb[sl];
        if (KSCALE) v *= sc[sl];
        *reinterpret_cast<VT*>(&Bs[bk[sl] * LSJ + bj[sl]]) = v;
      } else {
#pragma unroll
        for (int c = 0; c < VW; ++c) Bs[(bk[sl] + c) * LSJ + bj[sl]] = rb[sl][c];
      }
    }
  };

  v16f acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;

  if (kbeg < kend) {
    load(kbeg);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += FK, cur ^= 1) {
      const bool more = k0 + FK < kend;
      if (more) load(k0 + FK);                    // global -> registers, in flight behind the MFMAs
      const float* As = As2base + cur * (FM * LSK);
      const float* Bs = Bs2base + cur * (FK * LSJ);
      const float4* arow = reinterpret_cast<const float4*>(&As[(wm * 32 + r) * LSK + FH * h]);
      float av[FH], bv[FH];
#pragma unroll
      for (int u4 = 0; u4 < FH / 4; ++u4) {
        const float4 v = arow[u4];
        av[4 * u4] = v.x; av[4 * u4 + 1] = v.y; av[4 * u4 + 2] = v.z; av[4 * u4 + 3] = v.w;
      }
#pragma unroll
      for (int u = 0; u < FH; ++u) bv[u] = Bs[(u + FH * h) * LSJ + wn * 32 + r];
#pragma unroll
      for (int u = 0; u < FH; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      if (more) store(cur ^ 1);                   // the other buffer: nobody reads it this tile
      __syncthreads();
    }
  }

  const float* rs = g.rowscale ? g.rowscale + b0 * g.rs_b0 : nullptr;
  const float* ad = g.addend ? g.addend + b1 * g.ad_b1 : nullptr;
  const int gj = j0 + wn * 32 + r;
  // Everything the epilogue reads is requested before its first store (clamped addresses keep the loads
  // unconditional).  Element by element -- load, use, store, next load -- every load waited with vmcnt(0) for
  // the acknowledgement of the store before it (C may alias what is read, so the compiler cannot hoist):
  // sixteen dependent memory round trips per thread whenever a row scale, an addend or C += was asked for.
  float rsv[16] = {}, adv[16] = {}, cv[16] = {};
  if (rs || ad || g.beta_one) {
    const long long gjc = gj < g.N ? gj : g.N - 1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int gi = i0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
      const long long gic = gi < g.M ? gi : g.M - 1;
      rsv[q] = rs ? rs[gic] : 1.0f;
      adv[q] = ad ? ad[gic * g.ldc + gjc] : 0.f;
      cv[q] = g.beta_one ? C[gic * g.ldc + gjc] : 0.f;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) asm volatile("" : "+v"(rsv[q]), "+v"(adv[q]), "+v"(cv[q]));   // in registers HERE
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int gi = i0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
    if (gi >= g.M || gj >= g.N) continue;
    float v = acc[q];
    if (rs) v = rsv[q] * v;
    if (ad) v = adv[q] + v;
    float* c = C + gi * g.ldc + gj;
    if (g.beta_one) *c = v + cv[q];
    else if (g.stream_c) __builtin_nontemporal_store(v, c);
    else *c = v;
  }
}


template <bool A_KVEC, bool B_JVEC, bool KSCALE, int FK, int VW>
__global__ __launch_bounds__(256) void gemm32_fast_kernel(GemmArgs g) {
  __shared__ float As2[2 * FM * (FK + 4)];      // double-buffered: one barrier per k-tile
  __shared__ float Bs2[2 * FK * LSJ];
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with its own
  // L2) in linear-id order (x fastest, then y, then z), so linear ids that differ by 8 share an L2.
  // Remap so that CONSECUTIVE logical tiles land on one XCD: the column tiles of one row panel
  // (they re-read the same A rows), and -- for a split-K product -- all tiles of one k-chunk (each
  // re-reads the chunk's A and B slabs; dealt over 8 L2s those slabs came from HBM 6 times over).
  int bx = blockIdx.x, by = blockIdx.y, z = blockIdx.z;
  {
    const int plane = gridDim.x * gridDim.y, total = plane * gridDim.z;
    if ((total & 7) == 0) {
      const int id = z * plane + by * gridDim.x + bx;
      int tl = (id & 7) * (total >> 3) + (id >> 3);
      z = tl / plane;
      tl -= z * plane;
      by = tl / gridDim.x;
      bx = tl - by * gridDim.x;
    }
  }
  gemm32_fast_tile<A_KVEC ? 1 : 0, B_JVEC ? 1 : 0, KSCALE, FK, VW>(g, bx, by, z, false, false, As2, Bs2);
}

// Several SMALL products in one launch (the driver's batch of 50 pairs makes every product of the bilinear
// backward a 5-8 us launch at the latency floor: U and V, then dQ, dA and dW, are independent of each
// other).  Workgroup w of the 1-D grid belongs to the problem whose [first, first + count) holds w; operand
// layouts are run-time flags.  No XCD remapping: the problems are small by construction.
struct GemmGroup {
  GemmArgs g[kGroupMax];
  int first[kGroupMax + 1];      // first workgroup of each problem; first[n] = total
  int gx[kGroupMax], gy[kGroupMax];
  int ak[kGroupMax], bj[kGroupMax];
  int n;
};

template <int FK, int VW>
__global__ __launch_bounds__(256) void gemm32_group_kernel(GemmGroup grp) {
  __shared__ float As2[2 * FM * (FK + 4)];
  __shared__ float Bs2[2 * FK * LSJ];
  const int w = blockIdx.x;
  int p = 0;
#pragma unroll
  for (int i = 1; i < kGroupMax; ++i)
    if (i < grp.n && w >= grp.first[i]) p = i;
  int l = w - grp.first[p];
  const int plane = grp.gx[p] * grp.gy[p];
  const int z = l / plane;
  l -= z * plane;
  const int by = l / grp.gx[p], bx = l - by * grp.gx[p];
  // p is uniform: the struct members come from the kernarg segment with scalar loads at a computed offset
  gemm32_fast_tile<-1, -1, false, FK, VW>(grp.g[p], bx, by, z, grp.ak[p] != 0, grp.bj[p] != 0, As2, Bs2);
}

static bool multv(long long x, int vw) { return x % vw == 0; }
int gemm_fast_variant(const GemmArgs& g, int* vw_out) {
  if (g.kchunk % 32 != 0 && g.ksplit > 1 && !g.ks_stacked) return 0;   // split boundaries must fall on k-tile boundaries (16 or 32)
  if (g.bkscale && !(g.b_cs == 1)) return 0;
  for (int vw = 4; vw >= 2; vw -= 2) {
    const uintptr_t am = (uintptr_t)(4 * vw - 1);
    const bool bases = (reinterpret_cast<uintptr_t>(g.A) & am) == 0 && (reinterpret_cast<uintptr_t>(g.B) & am) == 0 &&
                       multv(g.a_b0, vw) && multv(g.a_b1, vw) && multv(g.b_b0, vw) && multv(g.b_b1, vw) &&
                       (!g.ks_stacked || (multv(g.a_ks, vw) && multv(g.b_ks, vw)));
    if (!bases || !multv(g.K, vw)) continue;
    int a_kvec;
    if (g.a_cs == 1 && multv(g.a_rs, vw)) a_kvec = 1;
    else if (g.a_rs == 1 && multv(g.a_cs, vw) && multv(g.M, vw)) a_kvec = 0;
    else continue;
    int b_jvec;
    if (g.b_cs == 1 && multv(g.b_rs, vw) && multv(g.N, vw)) b_jvec = 1;
    else if (g.b_rs == 1 && multv(g.b_cs, vw)) b_jvec = 0;
    else continue;
    if (vw_out) *vw_out = vw;
    return 1 + 2 * a_kvec + b_jvec;
  }
  return 0;
}

GemmArgs gemm_args(int M, int N, int K, const float* A, long long a_rs, long long a_cs, const float* B, long long b_rs,
                   long long b_cs, float* C, long long ldc) {
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = A; g.a_rs = a_rs; g.a_cs = a_cs;
  g.B = B; g.b_rs = b_rs; g.b_cs = b_cs;
  g.C = C; g.ldc = ldc;
  g.nb1 = 1; g.ksplit = 1; g.kchunk = K;
  g.a_ifast = (a_rs == 1 && a_cs != 1);
  g.b_jfast = (b_cs == 1);
  return g;
}

void gemm_launch(const GemmArgs& g0, int nb0, hipStream_t s) {
  // gridDim.z <= 65535: slice the outer batch when (pairs x measures x splits) is larger.
  const int per_b0 = g0.nb1 * g0.ksplit;
  const int max_b0 = per_b0 > 65535 ? 1 : 65535 / per_b0;
  for (int b = 0; b < nb0; b += max_b0) {
    const int nb = (nb0 - b) < max_b0 ? (nb0 - b) : max_b0;
    GemmArgs g = g0;
    g.A += (long long)b * g.a_b0;
    g.B += (long long)b * g.b_b0;
    g.C += (long long)b * g.c_b0;
    if (g.rowscale) g.rowscale += (long long)b * g.rs_b0;
    int vw = 4;
    const int fv = gemm_fast_variant(g, &vw);
    if (fv) {
      dim3 grid((g.N + FN - 1) / FN, (g.M + FM - 1) / FM, nb * per_b0);
      const bool ksc = g.bkscale != nullptr;   // only with B_JVEC (gemm_fast_variant)
      const bool deep = (long long)grid.x * grid.y * grid.z <= 2 * 256;   // at most two workgroups per CU
#define MMS_FAST(a, b, c)                                                                              \
  do {                                                                                                 \
    if (deep && vw == 4) hipLaunchKernelGGL((gemm32_fast_kernel<a, b, c, 32, 4>), grid, dim3(256), 0, s, g);  \
    else if (vw == 4) hipLaunchKernelGGL((gemm32_fast_kernel<a, b, c, 16, 4>), grid, dim3(256), 0, s, g);     \
    else if (deep) hipLaunchKernelGGL((gemm32_fast_kernel<a, b, c, 32, 2>), grid, dim3(256), 0, s, g);        \
    else hipLaunchKernelGGL((gemm32_fast_kernel<a, b, c, 16, 2>), grid, dim3(256), 0, s, g);                  \
  } while (0)
      switch (fv - 1) {
        case 0: MMS_FAST(false, false, false); break;
        case 1: if (ksc) MMS_FAST(false, true, true); else MMS_FAST(false, true, false); break;
        case 2: MMS_FAST(true, false, false); break;
        default: if (ksc) MMS_FAST(true, true, true); else MMS_FAST(true, true, false); break;
      }
#undef MMS_FAST
      continue;
    }
    dim3 grid((g.N + BN - 1) / BN, (g.M + BM - 1) / BM, nb * per_b0);
    hipLaunchKernelGGL(gemm32_kernel, grid, dim3(256), 0, s, g);
  }
}

// (gemm32_group_kernel)
bool gemm_launch_group(const GemmArgs* gs, const int* nb0s, int n, hipStream_t s) {
  if (n < 2 || n > kGroupMax) return false;
  GemmGroup grp{};
  int vw = 4, total = 0;
  for (int i = 0; i < n; ++i) {
    const GemmArgs& g = gs[i];
    if (g.bkscale || g.rowscale || g.addend) return false;
    int v = 4;
    const int fv = gemm_fast_variant(g, &v);
    if (!fv) return false;
    vw = v < vw ? v : vw;
    grp.g[i] = g;
    grp.ak[i] = ((fv - 1) >> 1) & 1;
    grp.bj[i] = (fv - 1) & 1;
    grp.gx[i] = (g.N + FN - 1) / FN;
    grp.gy[i] = (g.M + FM - 1) / FM;
    const long long cnt = (long long)grp.gx[i] * grp.gy[i] * nb0s[i] * g.nb1 * g.ksplit;
    if (cnt > 1536) return false;                // a product this large keeps its own XCD-ordered launch
    grp.first[i] = total;
    total += (int)cnt;
  }
  if (total > 3072) return false;
  for (int i = n; i <= kGroupMax; ++i) grp.first[i] = total;
  grp.n = n;
  const bool deep = total <= 2 * 256;
  if (deep && vw == 4) hipLaunchKernelGGL((gemm32_group_kernel<32, 4>), dim3(total), dim3(256), 0, s, grp);
  else if (vw == 4) hipLaunchKernelGGL((gemm32_group_kernel<16, 4>), dim3(total), dim3(256), 0, s, grp);
  else if (deep) hipLaunchKernelGGL((gemm32_group_kernel<32, 2>), dim3(total), dim3(256), 0, s, grp);
  else hipLaunchKernelGGL((gemm32_group_kernel<16, 2>), dim3(total), dim3(256), 0, s, grp);
  return true;
}

// HALF: some problem of the group stores halves (reduce_group_add_half); the fp32 groups run the <false> instance
template <bool HALF>
__global__ __launch_bounds__(256) void splitk_reduce_group_kernel(ReduceGroup rg) {
  int p = 0;
#pragma unroll
  for (int i = 1; i < kGroupMax; ++i)
    if (i < rg.cnt && (int)blockIdx.x >= rg.first[i]) p = i;
  const float* __restrict__ part = rg.part[p];
  float* __restrict__ out = rg.out[p];
  const long long n = rg.n[p];
  const int splits = rg.splits[p];
  const long long stride = (long long)(rg.first[p + 1] - rg.first[p]) * 256;
  const bool accumulate = rg.accumulate[p] != 0;
  for (long long e = (long long)(blockIdx.x - rg.first[p]) * 256 + threadIdx.x; e < n; e += stride) {
    if (HALF && rg.half_out[p]) {
      reinterpret_cast<_Float16*>(out)[e] = (_Float16)ordered_slab_sum(part, n, e, splits, 0.f);
      continue;
    }
    out[e] = ordered_slab_sum(part, n, e, splits, accumulate ? out[e] : 0.f);
  }
}

// out[e] (= or +=) sum_s part[s*n + e], s ascending.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part,
                                                            int splits, long long n,
                                                            float* __restrict__ out,
                                                            int accumulate) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    const float s = ordered_slab_sum(part, n, e, splits, 0.f);
    out[e] = accumulate ? out[e] + s : s;
  }
}

// out[r][c] = scale[r] * x[r][c]
__global__ __launch_bounds__(256) void rowscale_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ scale,
                                                       float* __restrict__ out, long long rows,
                                                       int cols) {
  const long long n = rows * cols;
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride)
    out[e] = scale[e / cols] * x[e];
}

// out[r][c] = scale[r] * x[r][c]; out may BE x.
__global__ __launch_bounds__(256) void rowscale_inplace_ok_kernel(const float* x, const float* __restrict__ scale,
                                                                  float* out, long long rows, int cols) {
  const long long n = rows * cols;
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride)
    out[e] = scale[e / cols] * x[e];
}

// out[r][c] = scale[r] * x[r][c] for 16-byte-aligned rows (cols % 4 == 0); out may BE x (each thread
// reads the float4 it overwrites).  Streaming stores: the result is read next by another layer.
__global__ __launch_bounds__(256) void rowscale4_kernel(const float4* x, const float* __restrict__ scale,
                                                        float4* out, long long rows, int cols4) {
  const long long n = rows * cols4;
  const long long stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
    const float sc = scale[e / cols4];
    const float4 v = x[e];
    stream_store(out + e, make_float4(sc * v.x, sc * v.y, sc * v.z, sc * v.w));
  }
}

// top[r] = dot(x[r], y[r]) (+ bias)  -- one wave per row, fixed butterfly.
// top index = r*top_stride ; bias is a single value (may be null).
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ x,
                                                     const float* __restrict__ y,
                                                     const float* __restrict__ bias,
                                                     float* __restrict__ top, long long rows,
                                                     int cols, long long top_stride) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* xr = x + r * cols;
  const float* yr = y + r * cols;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += xr[c] * yr[c];
  s = wave_sum(s);
  if (lane == 0) top[r * top_stride] = bias ? (*bias + s) : s;
}

unsigned ew_blocks(long long n) {
  long long b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

void reduce_group_add(ReduceGroup& rg, const float* part, float* out, long long n, int splits, int accumulate) {
  const int i = rg.cnt++;
  rg.part[i] = part; rg.out[i] = out; rg.n[i] = n; rg.splits[i] = splits; rg.accumulate[i] = accumulate;
  for (int j = i + 1; j <= kGroupMax; ++j) rg.first[j] = rg.first[i] + (int)ew_blocks(n);
}
void reduce_group_add_half(ReduceGroup& rg, const float* part, void* out_f16, long long n, int splits) {
  rg.half_out[rg.cnt] = 1;
  reduce_group_add(rg, part, static_cast<float*>(out_f16), n, splits, 0);
}
void reduce_group_launch(const ReduceGroup& rg, hipStream_t s) {
  bool half = false;
  for (int i = 0; i < rg.cnt; ++i) half = half || rg.half_out[i] != 0;
  if (half)
    hipLaunchKernelGGL(splitk_reduce_group_kernel<true>, dim3(rg.first[rg.cnt]), dim3(256), 0, s, rg);
  else
    hipLaunchKernelGGL(splitk_reduce_group_kernel<false>, dim3(rg.first[rg.cnt]), dim3(256), 0, s, rg);
}

// Split count for a product with a long K (the dW products: K = pairs).  Workgroups = tiles x batch x
// splits; the chip takes them 256 x (workgroups per CU) at a time, so the count should (a) reach ~3 per CU
// and (b) nearly FILL its last round: 25 tiles x 32 splits = 800 is 3.1 per CU -- a fourth round for 12 %
// of the CUs, 78 % efficient -- while 25 x 40 = 1000 fills 97.6 % of four rounds (cfg 3's dW product:
// 52 -> 44 us).  Splits of 8 or more come in multiples of 8 so that the XCD-aware order applies.
int pick_ksplit(int Mt, int Nt, int K, int* kchunk, int batch) {
  const long long tiles = (long long)((Mt + FM - 1) / FM) * ((Nt + FN - 1) / FN) * (batch > 0 ? batch : 1);
  const long long maxs = (K + 63) / 64;           // at least 64 of K (two deep k-tiles) per split
  long long best = 1;
  double best_score = -1.0;
  for (long long sp = 1; sp <= maxs && sp <= 256; ++sp) {
    if (sp >= 8 && (sp & 7)) continue;
    const long long x = tiles * sp;
    if (x > 1280 && sp > 1) break;
    const double rounds = (double)((x + 255) / 256);
    const double eff = (double)x / 256.0 / rounds;              // how full the last round is
    const double fill = x >= 768 ? 1.0 : (double)x / 768.0;     // ~3 workgroups per CU hide latency
    const double score = eff * fill;
    if (score > best_score + 1e-9) { best_score = score; best = sp; }
  }
  int chunk = (int)((K + best - 1) / best);
  chunk = (chunk + 31) / 32 * 32;               // a multiple of either k-tile depth (16, 32)
  if (chunk < 32) chunk = 32;                   // K == 0 (the workspace size of an empty batch): one split, no division by zero
  *kchunk = chunk;
  const int splits = (K + chunk - 1) / chunk;
  return splits > 0 ? splits : 1;
}
// ---- the shared element-wise kernels, one launch each ----
void splitk_reduce_launch(const float* part, int splits, long long n, float* out, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, part, splits, n, out, accumulate);
}
void rowdot_launch(const float* x, const float* y, const float* bias, float* top, long long rows, int cols,
                   long long top_stride, hipStream_t s) {
  hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, y, bias, top, rows, cols, top_stride);
}
void rowscale_launch(const float* x, const float* scale, float* out, long long rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(rowscale_kernel, dim3(ew_blocks(rows * cols)), dim3(256), 0, s, x, scale, out, rows, cols);
}
void rowscale_inplace_ok_launch(const float* x, const float* scale, float* out, long long rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(rowscale_inplace_ok_kernel, dim3(ew_blocks(rows * cols)), dim3(256), 0, s, x, scale, out, rows, cols);
}
void rowscale4_launch(const float4* x, const float* scale, float4* out, long long rows, int cols4, hipStream_t s) {
  hipLaunchKernelGGL(rowscale4_kernel, dim3(ew_blocks(rows * cols4)), dim3(256), 0, s, x, scale, out, rows, cols4);
}

}  // namespace mms
