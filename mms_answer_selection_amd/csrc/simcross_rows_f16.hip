// csrc/simcross_rows_f16.hip -- fp16-STORAGE SimCross dist_mode 0 (cosine) and 1 (Euclidean) for W1 == W2 == 1
// (sentence-vector pairs; BASELINE cfg 5), for gfx950: the counterpart of simcross_rows.hip / simcross_rows_cosine.hip
// as simcross_cross_f16.hip is that of simcross_cross.hip.  HBM-bound: no MFMA here.  mms_abi.hip's _f16 entry points
// call simcross_euclid_rows_f16 / simcross_cosine_rows_f16 below; the per-thread distance mode lives here too.
//
// Compiled with -ffp-contract=off, as the fp32 kernels whose arithmetic these reproduce on the widened halves.
#include "euclid_math.h"
#include "mms_internal.h"

namespace mms {

// ---- fp16 storage, fp32 arithmetic (BASELINE cfg 5) --------------------------
// Same wave-centric structure with one pair per wave (cfg 5 is D = 1024): q, a,
// dq, da live in HBM as IEEE half (half the bytes per pair: s = 2 in SURVEY
// 8d's formulas); every half is widened exactly to fp32 on load, ALL arithmetic
// is the fp32 reference arithmetic in the reference order, and only the final
// dq / da are rounded (RNE) to half.  The scores stay fp32.  Hence:
//   top == oracle(fp32(q_half), fp32(a_half)) bit for bit, and
//   dq  == half(oracle dq) bit for bit.
// The reference has no fp16 instantiation (common.hpp:41-44); this is an
// MI355X-side storage format, not a change of the layer's numerics.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// RW pairs per wave (64 / RW lanes each).  The ordered sum runs with RW == 2 (D <= 400: beyond that its
// speculation windows of 32 lanes miss too often, see simcross_euclid_rows_f16, and the lane-chain kernel
// below takes over); a miss re-walks one segment exactly, so results never change, only time.
// TREE (RW == 1 only): the distance is the TREE sum of the squares that the ordered variants use only to centre
// their speculation windows -- no ordered chain, 8.3 instead of 19 us at cfg 5's shard.  The reference has no
// fp16 instantiation, so there is no reference rounding to reproduce; SURVEY 8(d) holds cfg 5 to 1e-3 relative
// against the fp32 oracle on the fp16-rounded inputs, and this sum is within ~1e-6 of it.  Opt-in
// (mms_set_f16_distance_mode): the default stays the ordered sum, bit-identical to the fp32 layer's.
template <int NIT, int RW, bool BWD, bool TREE = false>
__global__ __launch_bounds__(256) void euclid_rows_wave_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a,
    const float* __restrict__ top_diff, float* __restrict__ top_out,
    _Float16* __restrict__ dq, _Float16* __restrict__ da, int N, int D8) {
  constexpr int LPR = 64 / RW;
  extern __shared__ float4 lds4[];               // [4 waves][RW images] (euclid_math.h)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + wave) * RW;
  if (row0 >= N) return;
  const int rows = min(RW, N - row0);
  const int n8 = rows * D8;
  const int D4 = 2 * D8;
  const size_t base8 = (size_t)row0 * D8;
  const half8* q8 = reinterpret_cast<const half8*>(q) + base8;
  const half8* a8 = reinterpret_cast<const half8*>(a) + base8;
  const int h4 = spec_h4(D4), st4 = 3 * h4;
  float4* sq4 = lds4 + (size_t)wave * RW * st4;

  half8 x[NIT], y[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const int ii = i < n8 ? i : 0;
    x[it] = q8[ii];
    y[it] = a8[ii];
  }
  const int grp = lane / LPR, j = lane % LPR;
  const int grow = min(grp, rows - 1);           // a missing 2nd pair mirrors the 1st (results unused)
  float g = 0.f;
  if (BWD) g = top_diff[row0 + grow];

  float4 df[2 * NIT];
  float tree_total = 0.f;
  float2v pred[RW];                              // per pair: (pred1, pred2) partial sums
#pragma unroll
  for (int r = 0; r < RW; ++r) pred[r] = (float2v){0.f, 0.f};
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    const bool r1 = (RW == 2) && (i >= D8);
    const int ir = r1 ? i - D8 : i;              // half8 index inside its pair
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      float4 d;
      d.x = (float)x[it][4 * hh + 0] - (float)y[it][4 * hh + 0];
      d.y = (float)x[it][4 * hh + 1] - (float)y[it][4 * hh + 1];
      d.z = (float)x[it][4 * hh + 2] - (float)y[it][4 * hh + 2];
      d.w = (float)x[it][4 * hh + 3] - (float)y[it][4 * hh + 3];
      df[2 * it + hh] = d;
      float4 s;
      s.x = d.x * d.x; s.y = d.y * d.y; s.z = d.z * d.z; s.w = d.w * d.w;
      const int i4 = 2 * ir + hh;                // float4 index inside the pair's image
      if constexpr (!TREE) {
        if (i < n8) sq4[(r1 ? st4 : 0) + i4] = s;
      }
      const float s4 = (i < n8) ? (s.x + s.y) + (s.z + s.w) : 0.f;
      if (TREE) tree_total += s4;
      spec_pred_add<RW>(pred, r1, i4, h4, s4);
    }
  }
  if constexpr (!TREE) {                         // the tree sum reads no image: its launch has no LDS to pad
    const int npad = st4 - D4;
    if (lane < RW * npad) sq4[(lane / npad) * st4 + D4 + (lane % npad)] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float my1 = 0.f, my2 = 0.f;
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const float p1 = wave_sum(pred[r].x), p2 = wave_sum(pred[r].y);
    if (r == grow) { my1 = p1; my2 = p2; }
  }
  float dist;
  if constexpr (TREE) {
    dist = wave_sum(tree_total);
  } else {
    wave_lds_sync();
    dist = chain_sum_speculative<LPR>(sq4 + grow * st4, D4, my1, my2, j, grp * LPR);
  }
  const float T = 1.0f / (1.0f + sqrtf(dist));
  if (BWD) asm volatile("" : "+v"(g));          // in a register before the store of T (see euclid_pair32_kernel)
  if (j == 0 && grp < rows) top_out[row0 + grp] = T;
  if (!BWD) return;

  const EuclidCoef mine = euclid_coef(T, g);
  EuclidCoef kr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r)                   // lane r*LPR leads pair r's lane group
    kr[r] = EuclidCoef{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.c), r * LPR)),
                       readlane_f64(mine.den, r * LPR), readlane_f64(mine.rcp, r * LPR)};
  half8* dq8 = reinterpret_cast<half8*>(dq) + base8;
  half8* da8 = reinterpret_cast<half8*>(da) + base8;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i >= n8) break;
    const EuclidCoef& k = (RW == 2 && i >= D8) ? kr[RW - 1] : kr[0];
    half8 o0, o1;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const float4 t = euclid_tt4(k, df[2 * it + hh]);
      o0[4 * hh + 0] = (_Float16)(0.f + t.x); o0[4 * hh + 1] = (_Float16)(0.f + t.y);
      o0[4 * hh + 2] = (_Float16)(0.f + t.z); o0[4 * hh + 3] = (_Float16)(0.f + t.w);
      o1[4 * hh + 0] = (_Float16)(0.f + (-t.x)); o1[4 * hh + 1] = (_Float16)(0.f + (-t.y));
      o1[4 * hh + 2] = (_Float16)(0.f + (-t.z)); o1[4 * hh + 3] = (_Float16)(0.f + (-t.w));
    }
    stream_store_vec(dq8 + i, o0);
    stream_store_vec(da8 + i, o1);
  }
}

// The ORDERED distance at large D without speculation (round 3; D > 400, where a speculative chain with one pair per
// wave was 55 % of the launch: 20.2 us at cfg 5's shard against 13.2 here, profiles/r03_f16_lanewalk.txt).  One wave per pair loads,
// squares and later differentiates its pair exactly as above; the squares go to LDS as the pair's image, and after one
// workgroup barrier LANE p of wave 0 walks pair p's image front to back -- the reference's d-ascending fp32 sum
// (sim_cross_layer.cpp:100-106) as 4 D4 dependent adds fed by D4 ds_read_b128, about 2.4 us for D = 1024 whatever the
// number of lanes walking.  Eight pairs per workgroup, several workgroups per CU: one workgroup's walk hides behind the
// others' loads and stores (the launch is HBM-bound: 67 MB).  No windows, no misses, no re-walks; bit-identical by
// construction.
template <int NIT, bool BWD, int WPB = 8>
__global__ __launch_bounds__(64 * WPB) void euclid_rows_lanechain_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ top_diff,
    float* __restrict__ top_out, _Float16* __restrict__ dq, _Float16* __restrict__ da, int N, int D8) {
  extern __shared__ float4 lc_lds[];             // [WPB pairs][D4 + 1] float4, then WPB floats (the distances)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * WPB + wave;
  const int rowc = row < N ? row : N - 1;        // a missing pair mirrors the last one (results unused)
  const int D4 = 2 * D8, st4 = D4 + 1;
  const half8* q8 = reinterpret_cast<const half8*>(q) + (size_t)rowc * D8;
  const half8* a8 = reinterpret_cast<const half8*>(a) + (size_t)rowc * D8;
  float4* img = lc_lds + (size_t)wave * st4;
  float* dist_lds = reinterpret_cast<float*>(lc_lds + (size_t)WPB * st4);

  half8 x[NIT], y[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it, ii = i < D8 ? i : 0;
    x[it] = q8[ii];
    y[it] = a8[ii];
  }
  float g = 0.f;
  if (BWD) g = top_diff[rowc];
  float4 df[2 * NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      float4 d;
      d.x = (float)x[it][4 * hh + 0] - (float)y[it][4 * hh + 0];
      d.y = (float)x[it][4 * hh + 1] - (float)y[it][4 * hh + 1];
      d.z = (float)x[it][4 * hh + 2] - (float)y[it][4 * hh + 2];
      d.w = (float)x[it][4 * hh + 3] - (float)y[it][4 * hh + 3];
      df[2 * it + hh] = d;
      float4 sq;
      sq.x = d.x * d.x; sq.y = d.y * d.y; sq.z = d.z * d.z; sq.w = d.w * d.w;
      if (i < D8) img[2 * i + hh] = sq;
    }
  }
  __syncthreads();
  if (wave == 0 && lane < WPB) {
    const float4* mine = lc_lds + (size_t)lane * st4;
    float acc = 0.f;
#pragma unroll 8
    for (int i4 = 0; i4 < D4; ++i4) {
      const float4 v = mine[i4];
      acc += v.x; acc += v.y; acc += v.z; acc += v.w;
    }
    dist_lds[lane] = acc;
  }
  __syncthreads();
  if (row >= N) return;
  const float dist = dist_lds[wave];
  const float T = 1.0f / (1.0f + sqrtf(dist));
  if (BWD) asm volatile("" : "+v"(g));          // in a register before the store of T (see euclid_pair32_kernel)
  if (lane == 0) top_out[row] = T;
  if (!BWD) return;
  const EuclidCoef k = euclid_coef(T, g);
  half8* dq8 = reinterpret_cast<half8*>(dq) + (size_t)row * D8;
  half8* da8 = reinterpret_cast<half8*>(da) + (size_t)row * D8;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i >= D8) break;
    half8 o0, o1;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const float4 t = euclid_tt4(k, df[2 * it + hh]);
      o0[4 * hh + 0] = (_Float16)(0.f + t.x); o0[4 * hh + 1] = (_Float16)(0.f + t.y);
      o0[4 * hh + 2] = (_Float16)(0.f + t.z); o0[4 * hh + 3] = (_Float16)(0.f + t.w);
      o1[4 * hh + 0] = (_Float16)(0.f + (-t.x)); o1[4 * hh + 1] = (_Float16)(0.f + (-t.y));
      o1[4 * hh + 2] = (_Float16)(0.f + (-t.z)); o1[4 * hh + 3] = (_Float16)(0.f + (-t.w));
    }
    stream_store_vec(dq8 + i, o0);
    stream_store_vec(da8 + i, o1);
  }
}

// fp16-STORAGE cosine, W1 = W2 = 1 (round 3; cfg 5's "multi-modal concat embeddings, fp16" with dist_mode 0): one
// wave per pair, a lane holds NIT half8 of q and of a (all 16-byte loads up front, kept for the backward), fp32
// arithmetic on the exactly-widened inputs: three tree sums (the reference's cblas_sdot has no defined order), the
// reference's T = q.a / nq / na with its two successive divisions (sim_cross_layer.cpp:135) and its cached NORMS
// (:118); backward through per-pair factors as cosine_pair32_kernel (c1 = g / n0 / n1, c2 = g T / n0^2, c3 = g T / n1^2,
// IEEE divisions once per pair), gradients stored as RNE halves.  Bytes per pair: reads 2 D s + 4, writes 2 D s + 12.
template <int NIT, bool BWD>
__global__ __launch_bounds__(256) void cosine_rows_wave_f16_kernel(
    const _Float16* __restrict__ q, const _Float16* __restrict__ a, const float* __restrict__ top_diff,
    float* __restrict__ top, float* __restrict__ norm0, float* __restrict__ norm1,
    _Float16* __restrict__ dq, _Float16* __restrict__ da, int N, int D8) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const half8* q8 = reinterpret_cast<const half8*>(q) + (size_t)row * D8;
  const half8* a8 = reinterpret_cast<const half8*>(a) + (size_t)row * D8;
  half8 x[NIT], y[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it, ic = i < D8 ? i : D8 - 1;
    x[it] = q8[ic];
    y[it] = a8[ic];
  }
  float g = BWD ? top_diff[row] : 0.f;
  float sqq = 0.f, saa = 0.f, sqa = 0.f;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (lane + 64 * it < D8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = (float)x[it][e], yf = (float)y[it][e];
        sqq += xf * xf; saa += yf * yf; sqa += xf * yf;
      }
    }
  }
  sqq = wave_sum(sqq); saa = wave_sum(saa); sqa = wave_sum(sqa);
  const float n0 = sqrtf(sqq), n1 = sqrtf(saa);
  const float T = sqa / n0 / n1;                       // two successive divisions (:135)
  if (BWD) asm volatile("" : "+v"(g));
  if (lane == 0) {
    top[row] = T;
    if (norm0) norm0[row] = n0;
    if (norm1) norm1[row] = n1;
  }
  if (!BWD) return;
  const float c1 = g / n0 / n1, c2 = g * T / (n0 * n0), c3 = g * T / (n1 * n1);
  half8* dq8 = reinterpret_cast<half8*>(dq) + (size_t)row * D8;
  half8* da8 = reinterpret_cast<half8*>(da) + (size_t)row * D8;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = lane + 64 * it;
    if (i < D8) {
      half8 o0, o1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = (float)x[it][e], yf = (float)y[it][e];
        o0[e] = (_Float16)(0.f + (c1 * yf - c2 * xf));   // dq = g (a / n0 / n1 - q T / n0^2)   (:239-241)
        o1[e] = (_Float16)(0.f + (c1 * xf - c3 * yf));   // da = g (q / n0 / n1 - a T / n1^2)   (:243-245)
      }
      __builtin_nontemporal_store(o0, dq8 + i);
      __builtin_nontemporal_store(o1, da8 + i);
    }
  }
}

// ================ dispatch (DESIGN.md 4.4b is the table this section is read against) ================
// How the fp16-storage kernels sum a pair's squares (include/mms.h: mms_set_f16_distance_mode); per calling thread.
static thread_local int t_f16_distance_mode = MMS_F16_DISTANCE_ORDERED;
int f16_distance_mode() { return t_f16_distance_mode; }
void set_f16_distance_mode(int m) { t_f16_distance_mode = m; }

// half8 accesses of every array touched, at most four per operand per lane of a wave
static bool f16_rows_ok(int D, const void* q, const void* a, const void* dq, const void* da, bool bwd) {
  return D % 8 == 0 && D <= 2048 && aligned16(q) && aligned16(a) && (!bwd || (aligned16(dq) && aligned16(da)));
}

int simcross_cosine_rows_f16(int N, int D, const void* q, const void* a, const float* top_diff, float* top,
                             float* norm0, float* norm1, void* dq, void* da, bool bwd, hipStream_t s) {
  if (N == 0) return MMS_OK;
  if (!f16_rows_ok(D, q, a, dq, da, bwd)) return MMS_ERR_UNSUPPORTED;
  const int D8 = D / 8, nit = (D8 + 63) / 64;
  static constexpr decltype(&cosine_rows_wave_f16_kernel<1, true>) kernels[2][4] = {
      MMS_NIT4(cosine_rows_wave_f16_kernel, false), MMS_NIT4(cosine_rows_wave_f16_kernel, true)};
  hipLaunchKernelGGL(kernels[bwd][nit - 1], dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s,
                     static_cast<const _Float16*>(q), static_cast<const _Float16*>(a), top_diff, top, norm0, norm1,
                     static_cast<_Float16*>(dq), static_cast<_Float16*>(da), N, D8);
  return launch_status();
}

int simcross_euclid_rows_f16(int N, int D, const void* q, const void* a, const float* top_diff,
                             float* top, void* dq, void* da, bool bwd, hipStream_t s) {
  if (N == 0) return MMS_OK;
  if (!f16_rows_ok(D, q, a, dq, da, bwd)) return MMS_ERR_UNSUPPORTED;
  const int D8 = D / 8;
  const bool tree = f16_distance_mode() == MMS_F16_DISTANCE_TREE;
  const int rw = tree ? 1 : wave_pairs(D);        // tree sum: one pair per wave whatever D, no speculation windows to fit
  const int nit = (rw * D8 + 63) / 64;
  using Kernel = decltype(&euclid_rows_wave_f16_kernel<1, 1, true>);   // the three families share one signature
  Kernel k;
  unsigned grid, threads = 256;
  size_t lds;
  if (tree) {
    static constexpr Kernel kernels[2][4] = {MMS_NIT4(euclid_rows_wave_f16_kernel, 1, false, true),
                                             MMS_NIT4(euclid_rows_wave_f16_kernel, 1, true, true)};
    k = kernels[bwd][nit - 1];
    grid = (unsigned)((N + 3) / 4);
    lds = 0;                                          // no image: the tree instantiations touch no LDS
  } else if (rw == 2) {
    static constexpr Kernel kernels[2][4] = {MMS_NIT4(euclid_rows_wave_f16_kernel, 2, false),
                                             MMS_NIT4(euclid_rows_wave_f16_kernel, 2, true)};
    k = kernels[bwd][nit - 1];
    grid = (unsigned)((N + 4 * rw - 1) / (4 * rw));
    lds = spec_image_lds(4, rw, 2 * D8);
  } else {
    // ordered beyond two pairs per wave: lane p of wave 0 walks pair p's image
    constexpr int wpb = 8;                            // 4 / 8 / 16 waves measured alike (profiles/r03_f16_lanewalk.txt)
    static constexpr Kernel kernels[2][4] = {MMS_NIT4(euclid_rows_lanechain_f16_kernel, false, wpb),
                                             MMS_NIT4(euclid_rows_lanechain_f16_kernel, true, wpb)};
    static const bool once = [] {
      for (const auto& row : kernels)
        for (const Kernel f : row)
          (void)allow_dynamic_lds(f, 160 * 1024);
      return true;
    }();
    (void)once;
    k = kernels[bwd][nit - 1];
    grid = (unsigned)((N + wpb - 1) / wpb);
    threads = 64 * wpb;
    lds = ((size_t)wpb * (2 * D8 + 1) + 4) * sizeof(float4);
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, s, static_cast<const _Float16*>(q),
                     static_cast<const _Float16*>(a), top_diff, top, static_cast<_Float16*>(dq),
                     static_cast<_Float16*>(da), N, D8);
  return launch_status();
}

}  // namespace mms
