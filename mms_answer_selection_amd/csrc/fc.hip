// csrc/fc.hip -- InnerProduct, Softmax, SoftmaxWithLoss and Concat as layers of their own (include/mms_fc.h): the
// reference's inner_product_layer.cpp, softmax_layer.cpp, softmax_loss_layer.cpp and concat_layer.cpp.  What the host
// decides before a launch -- refusals, slabs, routes, grids -- is csrc/fc_plans.h.
//
//   InnerProduct, generic   kernels <T>, one thread per output element (top, bottom_diff, a slab's partial of w_diff or
//                           b_diff), the inner index ascending, every product and every add rounded on its own.
//   InnerProduct, fast      float.  Every product is fc_tile_kernel: a wave per 16 x 16 output tile on
//                           v_mfma_f32_16x16x4_f32, lane (l & 15, l >> 4) loading A[i][k] and B[k][j] straight from
//                           memory with any strides -- the operands of the head's products are a few KB and every
//                           element is used by a few tiles, so LDS staging would only add a barrier -- the inner index
//                           in steps of 4, the bias added in the epilogue.  Nothing depends on an address, so the words
//                           do not depend on how the arrays are aligned.  w_diff is one such product per slab
//                           (gridDim.y = slabs), into the workspace.
//   InnerProduct, finish    fc_reduce_kernel, both routes: per element of w_diff and b_diff the slabs' partials added in
//                           ascending order from the first, then that sum added into the diff.
//   Softmax                 fc_softmax_thread_kernel: a thread per (o, k) walks the channels; with inner > 1 the lanes
//                           of a wave are neighbours along k and every load is dense.  fc_softmax_wave_kernel
//                           (inner == 1, channels > kSoftmaxThreadRowMax): a wave per row, lane l holds channels
//                           l, l + 64, ...; the maximum is a butterfly (order-free), the sums walk each 64-channel chunk
//                           lane by lane, so they are the ascending sums the header states.
//   SoftmaxWithLoss         the softmax kernels, then fc_loss_finish_kernel: one workgroup, thread s sums slab s of the
//                           positions, thread 0 adds the slabs and forms the loss (forward) or the backward's scalar;
//                           fc_loss_diff_kernel applies it.
//   Concat                  fc_concat_kernel, one launch, blockIdx.y = bottom; per bottom 16-byte or element copies.
//
// No index exceeds int below the refused counts; offsets are formed in size_t / long long.  No grid dimension exceeds
// kFcMaxBlocks (x), kFcMaxSlabs (y) or MMS_CONCAT_MAX_BOTTOMS (y).
#include <float.h>

#include "fc_plans.h"
#include "mms_internal.h"

namespace mms {
namespace {

typedef float fc_v4f __attribute__((ext_vector_type(4)));
constexpr int kFcNarrowSteps = 8;            // k steps of 4 whose operands fc_tile_kernel has in flight at once

// w(n, k) = w[n * sn + k * sk]
struct FcW {
  long long sn, sk;
};
__host__ __device__ inline FcW fc_w_strides(const FcDims& d) {
  const FcW s = {d.transpose ? 1 : (long long)d.K, d.transpose ? (long long)d.N : 1};
  return s;
}

// ---- InnerProduct, generic -----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_forward_generic_kernel(FcDims d, const T* __restrict__ x,
                                                                       const T* __restrict__ w,
                                                                       const T* __restrict__ b, T* __restrict__ top) {
  const FcW ws = fc_w_strides(d);
  const long long total = (long long)d.M * d.N, stride = (long long)gridDim.x * kFcThreads;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const int m = (int)(e / d.N), n = (int)(e - (long long)m * d.N);
    const T* xr = x + (size_t)m * d.K;
    const T* wr = w + n * ws.sn;
    T acc = T(0);
    for (int k = 0; k < d.K; ++k) acc += xr[k] * wr[k * ws.sk];
    if (b) acc += b[n];
    top[e] = acc;
  }
}

template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_bottom_generic_kernel(FcDims d, const T* __restrict__ top_diff,
                                                                      const T* __restrict__ w,
                                                                      T* __restrict__ bottom_diff) {
  const FcW ws = fc_w_strides(d);
  const long long total = (long long)d.M * d.K, stride = (long long)gridDim.x * kFcThreads;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const int m = (int)(e / d.K), k = (int)(e - (long long)m * d.K);
    const T* tr = top_diff + (size_t)m * d.N;
    const T* wc = w + k * ws.sk;
    T acc = T(0);
    for (int n = 0; n < d.N; ++n) acc += tr[n] * wc[n * ws.sn];
    bottom_diff[e] = acc;
  }
}

// part[s][i] = sum over the rows of slab s of top_diff[m][n] * x[m][k], i = w_diff's index of (n, k)
template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_wpart_generic_kernel(FcDims d, int slab_rows, int slabs,
                                                                     const T* __restrict__ top_diff,
                                                                     const T* __restrict__ x, T* __restrict__ part) {
  const long long nw = (long long)d.K * d.N, total = nw * slabs, stride = (long long)gridDim.x * kFcThreads;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const int s = (int)(e / nw);
    const long long i = e - (long long)s * nw;
    int n, k;
    if (d.transpose) {
      k = (int)(i / d.N);
      n = (int)(i - (long long)k * d.N);
    } else {
      n = (int)(i / d.K);
      k = (int)(i - (long long)n * d.K);
    }
    const long long m0 = (long long)s * slab_rows, m1 = m0 + slab_rows < d.M ? m0 + slab_rows : d.M;
    T acc = T(0);
    for (long long m = m0; m < m1; ++m) acc += top_diff[m * d.N + n] * x[m * d.K + k];
    part[e] = acc;
  }
}

// part[s][n] = sum over the rows of slab s of top_diff[m][n]
template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_bpart_kernel(FcDims d, int slab_rows, int slabs,
                                                             const T* __restrict__ top_diff, T* __restrict__ part) {
  const long long total = (long long)d.N * slabs, stride = (long long)gridDim.x * kFcThreads;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const int s = (int)(e / d.N), n = (int)(e - (long long)s * d.N);
    const long long m0 = (long long)s * slab_rows, m1 = m0 + slab_rows < d.M ? m0 + slab_rows : d.M;
    T acc = T(0);
    for (long long m = m0; m < m1; ++m) acc += top_diff[m * d.N + n];
    part[e] = acc;
  }
}

// diff[i] += part[0][i] + part[1][i] + ... : the slabs from the first in ascending order, then into the diff.
// Elements [0, nw) are w_diff's, [nw, nw + nb) are b_diff's; either count may be 0.
template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_reduce_kernel(int slabs, long long nw, const T* __restrict__ wpart,
                                                              T* __restrict__ w_diff, long long nb,
                                                              const T* __restrict__ bpart, T* __restrict__ b_diff) {
  const long long total = nw + nb, stride = (long long)gridDim.x * kFcThreads;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const bool is_w = e < nw;
    const long long i = is_w ? e : e - nw, n = is_w ? nw : nb;
    const T* part = is_w ? wpart : bpart;
    T sum = part[i];
    for (int s = 1; s < slabs; ++s) sum += part[(long long)s * n + i];
    T* out = is_w ? w_diff : b_diff;
    out[i] = out[i] + sum;
  }
}

// ---- InnerProduct, fast --------------------------------------------------------------------------------------------
// C(i, j) = sum over k of slab blockIdx.y of A(i, k) B(k, j) [+ bias[j]], written to C + blockIdx.y * c_slab
struct FcProd {
  int rows, cols, kdim, slab_len;
  const float* A;
  long long a_rs, a_cs;       // A(i, k) = A[i * a_rs + k * a_cs]
  const float* B;
  long long b_rs, b_cs;       // B(k, j) = B[k * b_rs + j * b_cs]
  float* C;
  long long ldc, c_slab;
  const float* bias;
};

__global__ __launch_bounds__(kFcThreads) void fc_tile_kernel(FcProd p, int row_tiles, int col_tiles) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, grp = lane >> 4;
  // kbeg < kend: the plan's slabs.  The sum is long long: the last slab of an M near INT_MAX ends at 2^31.
  const int kbeg = blockIdx.y * p.slab_len, kend = (int)min((long long)p.kdim, (long long)kbeg + p.slab_len);
  float* const C = p.C + (long long)blockIdx.y * p.c_slab;
  const long long ntiles = (long long)row_tiles * col_tiles;
  // the trip count is the wave's: every lane is active at every MFMA
  for (long long t = (long long)blockIdx.x * 4 + wave; t < ntiles; t += (long long)gridDim.x * 4) {
    const int rt = (int)(t / col_tiles), ct = (int)(t - (long long)rt * col_tiles);
    const int i = rt * 16 + l16, j = ct * 16 + l16;
    // rows and columns past the edge read the last one's operands; their results are not stored
    const float* ap = p.A + (long long)min(i, p.rows - 1) * p.a_rs;
    const float* bp = p.B + (long long)min(j, p.cols - 1) * p.b_cs;
    fc_v4f acc = {0.f, 0.f, 0.f, 0.f};
    // eight k steps' operands are requested before the first of their MFMAs: a load per step would cost a memory
    // round trip per step.  Steps past the slab's end multiply zeros: acc + 0 * 0.
    for (long long k0 = kbeg; k0 < kend; k0 += 4 * kFcNarrowSteps) {      // long long: kend may be INT_MAX
      float av[kFcNarrowSteps], bv[kFcNarrowSteps];
#pragma unroll
      for (int u = 0; u < kFcNarrowSteps; ++u) {
        const long long k = k0 + 4 * u + grp, kc = k < kend ? k : kend - 1;
        av[u] = ap[kc * p.a_cs];
        bv[u] = bp[kc * p.b_rs];
        if (k >= kend) av[u] = 0.f, bv[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < kFcNarrowSteps; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    // C/D layout: column = lane & 15, row = 4 * (lane >> 4) + r
    if (j < p.cols) {
      const float bj = p.bias ? p.bias[j] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * grp + r;
        if (row < p.rows) C[(long long)row * p.ldc + j] = p.bias ? acc[r] + bj : acc[r];
      }
    }
  }
}

// one product of the fast route; slabs > 1 only for a product into the workspace
void fc_fast_product(const FcProd& p, int slabs, hipStream_t s) {
  const FcNarrowGrid g = fc_narrow_grid(p.rows, p.cols, slabs);
  hipLaunchKernelGGL(fc_tile_kernel, dim3((unsigned)g.blocks_x, (unsigned)g.blocks_y), dim3(kFcThreads), 0, s, p,
                     g.row_tiles, g.col_tiles);
}

// ---- Softmax -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fc_exp(float v) { return expf(v); }
__device__ __forceinline__ double fc_exp(double v) { return exp(v); }
__device__ __forceinline__ float fc_log(float v) { return logf(v); }
__device__ __forceinline__ double fc_log(double v) { return log(v); }

// a thread per position p = (o, k); element (o, c, k) is at (o * channels + c) * inner + k
template <typename T, bool BWD>
__global__ __launch_bounds__(kFcThreads) void fc_softmax_thread_kernel(SoftmaxDims d, const T* a, const T* b, T* out) {
  const long long P = (long long)d.outer * d.inner, stride = (long long)gridDim.x * kFcThreads;
  for (long long p = (long long)blockIdx.x * kFcThreads + threadIdx.x; p < P; p += stride) {
    const long long o = p / d.inner, k = p - o * d.inner;
    const size_t base = (size_t)o * d.channels * d.inner + (size_t)k, cs = (size_t)d.inner;
    if (BWD) {                               // a = top, b = top_diff
      T dot = T(0);
      for (int c = 0; c < d.channels; ++c) dot += b[base + c * cs] * a[base + c * cs];
      for (int c = 0; c < d.channels; ++c) out[base + c * cs] = (b[base + c * cs] - dot) * a[base + c * cs];
    } else {                                 // a = bottom
      T mx = a[base];
      for (int c = 1; c < d.channels; ++c) mx = max(mx, a[base + c * cs]);
      T sum = T(0);
      for (int c = 0; c < d.channels; ++c) {
        const T e = fc_exp(a[base + c * cs] - mx);
        out[base + c * cs] = e;
        sum += e;
      }
      for (int c = 0; c < d.channels; ++c) out[base + c * cs] = out[base + c * cs] / sum;
    }
  }
}

// s + v of lane 0 + v of lane 1 + ... + v of lane n - 1; n is the wave's
template <typename T>
__device__ __forceinline__ T fc_lanes_ascending(T s, T v, int n) {
  for (int l = 0; l < n; ++l) s += __shfl(v, l);
  return s;
}

// inner == 1: a wave per row
template <typename T, bool BWD>
__global__ __launch_bounds__(kFcThreads) void fc_softmax_wave_kernel(SoftmaxDims d, const T* a, const T* b, T* out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, C = d.channels;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < d.outer; row += (long long)gridDim.x * 4) {
    const size_t base = (size_t)row * C;
    if (BWD) {
      T dot = T(0);
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const T v = c < C ? b[base + c] * a[base + c] : T(0);
        dot = fc_lanes_ascending(dot, v, min(64, C - c0));
      }
      for (int c = lane; c < C; c += 64) out[base + c] = (b[base + c] - dot) * a[base + c];
    } else {
      T mx = a[base];
      for (int c = lane; c < C; c += 64) mx = max(mx, a[base + c]);
      for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
      T sum = T(0);
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        T e = T(0);
        if (c < C) {
          e = fc_exp(a[base + c] - mx);
          out[base + c] = e;
        }
        sum = fc_lanes_ascending(sum, e, min(64, C - c0));
      }
      for (int c = lane; c < C; c += 64) out[base + c] = out[base + c] / sum;   // the lane's own stores
    }
  }
}

// ---- SoftmaxWithLoss -----------------------------------------------------------------------------------------------
struct LossDims {
  int outer, channels, inner, normalization, has_ignore, ignore_label;
};

// the label of position p, or -1 where it is ignored or names no channel
template <typename T>
__device__ __forceinline__ int fc_label(const LossDims& d, const T* __restrict__ label, long long p) {
  const int v = static_cast<int>(label[p]);
  if (d.has_ignore && v == d.ignore_label) return -1;
  return (v >= 0 && v < d.channels) ? v : -1;
}

// One workgroup.  Thread s sums slab s of the positions (prob == NULL: the count only); thread 0 adds the slabs in
// ascending order.  loss != NULL: *loss = sum / max(1, normalizer).  scale != NULL: *scale = loss_weight / max(1, normalizer).
template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_loss_finish_kernel(LossDims d, int slabs, int slab_len,
                                                                   const T* __restrict__ prob,
                                                                   const T* __restrict__ label, T loss_weight,
                                                                   T* part, int* cnt, T* loss, T* scale) {
  const long long P = (long long)d.outer * d.inner;
  const int s = threadIdx.x;
  if (s < slabs) {
    const long long p0 = (long long)s * slab_len, p1 = p0 + slab_len < P ? p0 + slab_len : P;
    T acc = T(0);
    int n = 0;
    for (long long p = p0; p < p1; ++p) {
      const int l = fc_label(d, label, p);
      if (l < 0) continue;
      ++n;
      if (prob) {
        const long long o = p / d.inner, k = p - o * d.inner;
        const T v = prob[((size_t)o * d.channels + l) * d.inner + k];
        acc -= fc_log(max(v, T(FLT_MIN)));
      }
    }
    part[s] = acc;
    cnt[s] = n;
  }
  __syncthreads();
  if (s == 0) {
    T sum = part[0];
    int n = cnt[0];
    for (int i = 1; i < slabs; ++i) {
      sum += part[i];
      n += cnt[i];
    }
    T normalizer = T(1);
    if (d.normalization == MMS_LOSS_NORM_FULL) normalizer = T(P);
    else if (d.normalization == MMS_LOSS_NORM_VALID) normalizer = T(n);
    else if (d.normalization == MMS_LOSS_NORM_BATCH_SIZE) normalizer = T(d.outer);
    normalizer = max(T(1), normalizer);
    if (loss) *loss = sum / normalizer;
    if (scale) *scale = loss_weight / normalizer;
  }
}

template <typename T>
__global__ __launch_bounds__(kFcThreads) void fc_loss_diff_kernel(LossDims d, const T* __restrict__ prob,
                                                                 const T* __restrict__ label,
                                                                 const T* __restrict__ scale,
                                                                 T* __restrict__ bottom_diff) {
  const long long total = (long long)d.outer * d.channels * d.inner, stride = (long long)gridDim.x * kFcThreads;
  const T sc = *scale;
  for (long long e = (long long)blockIdx.x * kFcThreads + threadIdx.x; e < total; e += stride) {
    const long long k = e % d.inner, oc = e / d.inner, o = oc / d.channels;
    const int c = (int)(oc - o * d.channels), l = fc_label(d, label, o * d.inner + k);
    T v = T(0);
    if (l >= 0) v = c == l ? prob[e] - T(1) : prob[e];
    bottom_diff[e] = v * sc;
  }
}

// ---- Concat --------------------------------------------------------------------------------------------------------
// blockIdx.y = bottom.  TO_TOP: top's run <- the bottom's; otherwise the bottom diff's run <- top_diff's.  W is an
// unsigned integer of the element's size: the copies move bits.
struct ConcatArgs {
  const void* bottom[MMS_CONCAT_MAX_BOTTOMS];   // NULL: skipped
  int run[MMS_CONCAT_MAX_BOTTOMS];              // extent * inner: elements of one of its rows
  int offset[MMS_CONCAT_MAX_BOTTOMS];           // elements into top's row
  int vec[MMS_CONCAT_MAX_BOTTOMS];              // 16 bytes per lane
  int num_concats, top_run;
};

template <typename W, bool TO_TOP>
__global__ __launch_bounds__(kFcThreads) void fc_concat_kernel(ConcatArgs a, void* top_v) {
  const int b = blockIdx.y;
  W* const bot = static_cast<W*>(const_cast<void*>(a.bottom[b]));
  W* const top = static_cast<W*>(top_v) + a.offset[b];
  if (!bot || a.run[b] == 0) return;
  constexpr int VW = 16 / sizeof(W);
  const long long stride = (long long)gridDim.x * kFcThreads, first = (long long)blockIdx.x * kFcThreads + threadIdx.x;
  if (a.vec[b]) {
    const int per = a.run[b] / VW;
    const long long units = (long long)per * a.num_concats;
    for (long long u = first; u < units; u += stride) {
      const long long n = u / per, i = (u - n * per) * VW;
      uint4* const t = reinterpret_cast<uint4*>(top + n * a.top_run + i);
      uint4* const s = reinterpret_cast<uint4*>(bot + n * a.run[b] + i);
      if (TO_TOP) *t = *s; else *s = *t;
    }
  } else {
    const long long units = (long long)a.run[b] * a.num_concats;
    for (long long u = first; u < units; u += stride) {
      const long long n = u / a.run[b], i = u - n * a.run[b];
      if (TO_TOP) top[n * a.top_run + i] = bot[n * a.run[b] + i]; else bot[n * a.run[b] + i] = top[n * a.top_run + i];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
// The overlap refusals are csrc/host_args.h's: outputs_overlap over a list whose first spans are the call's outputs.
template <typename T>
int ip_forward(const mms_inner_product_shape* shape, const T* x, const T* w, const T* b, T* top, bool generic,
               hipStream_t s) {
  FcDims d;
  const int rc = fc_ip_check(shape, &d);
  if (rc != MMS_OK || d.M == 0) return rc;
  if (!x || !w || !top || (d.bias && !b)) return MMS_ERR_INVALID_ARG;
  const ByteSpan spans[] = {byte_span(top, (size_t)d.M * d.N * sizeof(T)), byte_span(x, (size_t)d.M * d.K * sizeof(T)),
                            byte_span(w, (size_t)d.K * d.N * sizeof(T)),
                            byte_span(d.bias ? b : nullptr, d.N * sizeof(T))};
  if (outputs_overlap(spans, 4, 1)) return MMS_ERR_INVALID_ARG;
  if (!d.bias) b = nullptr;
  if constexpr (sizeof(T) == 4) {
    if (!generic && fc_ip_route(d, MMS_FC_PASS_FORWARD) == MMS_FC_ROUTE_FAST) {
      const FcW ws = fc_w_strides(d);
      const FcProd p = {d.M, d.N, d.K, d.K, x, d.K, 1, w, ws.sk, ws.sn, top, d.N, 0, b};
      fc_fast_product(p, 1, s);
      return launch_status();
    }
  }
  hipLaunchKernelGGL(fc_forward_generic_kernel<T>, dim3((unsigned)fc_sweep_blocks((long long)d.M * d.N)),
                     dim3(kFcThreads), 0, s, d, x, w, b, top);
  return launch_status();
}

template <typename T>
int ip_backward(const mms_inner_product_shape* shape, const T* x, const T* w, const T* top_diff, T* w_diff, T* b_diff,
                T* bottom_diff, void* workspace, size_t workspace_bytes, bool generic, hipStream_t s) {
  FcDims d;
  const int rc = fc_ip_check(shape, &d);
  if (rc != MMS_OK || d.M == 0) return rc;
  if (!top_diff || (w_diff && !x) || (bottom_diff && !w) || (b_diff && !d.bias) || (!w_diff && !b_diff && !bottom_diff))
    return MMS_ERR_INVALID_ARG;
  const size_t nx = (size_t)d.M * d.K * sizeof(T), nw = (size_t)d.K * d.N * sizeof(T);
  const size_t need = (size_t)fc_ip_workspace_elems(d) * sizeof(T), nt = (size_t)d.M * d.N * sizeof(T);
  const bool sums = w_diff || b_diff;
  const ByteSpan spans[] = {byte_span(w_diff, nw), byte_span(b_diff, d.N * sizeof(T)), byte_span(bottom_diff, nx),
                            byte_span(sums ? workspace : nullptr, need), byte_span(top_diff, nt),
                            byte_span(w_diff ? x : nullptr, nx), byte_span(bottom_diff ? w : nullptr, nw)};
  if (outputs_overlap(spans, 7, 4)) return MMS_ERR_INVALID_ARG;
  if (sums && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  bool fast = false;
  if constexpr (sizeof(T) == 4) fast = !generic && fc_ip_route(d, MMS_FC_PASS_BACKWARD) == MMS_FC_ROUTE_FAST;
  const FcW ws = fc_w_strides(d);
  const int slab_rows = fc_slab_rows(d.M), slabs = fc_slabs(d.M);
  const long long nwe = (long long)d.K * d.N;
  T* const wpart = static_cast<T*>(workspace);
  T* const bpart = sums ? wpart + nwe * slabs : nullptr;
  if (w_diff) {
    if (fast) {
      if constexpr (sizeof(T) == 4) {
        // (N_out, K) = top_diff^T . x, or (K, N_out) = x^T . top_diff
        const FcProd p = d.transpose
                             ? FcProd{d.K, d.N, d.M, slab_rows, x, 1, d.K, top_diff, d.N, 1, wpart, d.N, nwe, nullptr}
                             : FcProd{d.N, d.K, d.M, slab_rows, top_diff, 1, d.N, x, d.K, 1, wpart, d.K, nwe, nullptr};
        fc_fast_product(p, slabs, s);
      }
    } else {
      hipLaunchKernelGGL(fc_wpart_generic_kernel<T>, dim3((unsigned)fc_sweep_blocks(nwe * slabs)), dim3(kFcThreads), 0,
                         s, d, slab_rows, slabs, top_diff, x, wpart);
    }
  }
  if (b_diff)
    hipLaunchKernelGGL(fc_bpart_kernel<T>, dim3((unsigned)fc_sweep_blocks((long long)d.N * slabs)), dim3(kFcThreads), 0,
                       s, d, slab_rows, slabs, top_diff, bpart);
  if (sums) {
    const long long rw = w_diff ? nwe : 0, rb = b_diff ? d.N : 0;
    hipLaunchKernelGGL(fc_reduce_kernel<T>, dim3((unsigned)fc_sweep_blocks(rw + rb)), dim3(kFcThreads), 0, s, slabs, rw,
                       wpart, w_diff, rb, bpart, b_diff);
  }
  if (bottom_diff) {
    if (fast) {
      if constexpr (sizeof(T) == 4) {
        const FcProd p = {d.M, d.K, d.N, d.N, top_diff, d.N, 1, w, ws.sn, ws.sk, bottom_diff, d.K, 0, nullptr};
        fc_fast_product(p, 1, s);
      }
    } else {
      hipLaunchKernelGGL(fc_bottom_generic_kernel<T>, dim3((unsigned)fc_sweep_blocks((long long)d.M * d.K)),
                         dim3(kFcThreads), 0, s, d, top_diff, w, bottom_diff);
    }
  }
  return launch_status();
}

size_t ip_workspace_bytes(const mms_inner_product_shape* shape, size_t elem) {
  FcDims d;
  if (fc_ip_check(shape, &d) != MMS_OK) return 0;
  return (size_t)fc_ip_workspace_elems(d) * elem;
}

// BWD: (a, b, out) = (top, top_diff, bottom_diff); otherwise (a, out) = (bottom, top) and b is NULL
template <typename T, bool BWD>
void softmax_launch(const SoftmaxDims& d, const T* a, const T* b, T* out, hipStream_t s) {
  if (d.inner == 1 && d.channels > kSoftmaxThreadRowMax) {
    const long long blocks = ((long long)d.outer + 3) / 4;
    hipLaunchKernelGGL((fc_softmax_wave_kernel<T, BWD>), dim3((unsigned)(blocks < kFcMaxBlocks ? blocks : kFcMaxBlocks)),
                       dim3(kFcThreads), 0, s, d, a, b, out);
  } else {
    hipLaunchKernelGGL((fc_softmax_thread_kernel<T, BWD>),
                       dim3((unsigned)fc_sweep_blocks((long long)d.outer * d.inner)), dim3(kFcThreads), 0, s, d, a, b,
                       out);
  }
}

template <typename T, bool BWD>
int softmax_call(const mms_softmax_shape* shape, const T* a, const T* b, T* out, hipStream_t s) {
  if (!shape) return MMS_ERR_INVALID_ARG;
  SoftmaxDims d;
  const int rc = fc_softmax_check(shape->outer, shape->channels, shape->inner, &d);
  if (rc != MMS_OK || d.outer == 0) return rc;
  if (!a || !out || (BWD && !b)) return MMS_ERR_INVALID_ARG;
  const size_t bytes = (size_t)d.outer * d.channels * d.inner * sizeof(T);
  const ByteSpan so = byte_span(out, bytes), sa = byte_span(a, bytes), sb = byte_span(b, bytes);
  if (spans_meet(so, sa) || (BWD && spans_meet(sa, sb))) return MMS_ERR_INVALID_ARG;
  if (BWD && out != b && spans_meet(so, sb)) return MMS_ERR_INVALID_ARG;     // bottom_diff may BE top_diff
  softmax_launch<T, BWD>(d, a, b, out, s);
  return launch_status();
}

template <typename T>
int loss_check(const mms_softmax_loss_shape* shape, SoftmaxDims* d, LossDims* l) {
  const int rc = fc_loss_check(shape, d);
  if (rc != MMS_OK) return rc;
  const LossDims out = {d->outer, d->channels, d->inner, shape->normalization, shape->has_ignore_label != 0,
                        shape->ignore_label};
  *l = out;
  return MMS_OK;
}

// the workspace's three parts
template <typename T>
struct LossWs {
  T* part;
  T* scale;
  int* cnt;
  LossWs(void* ws, int slabs) : part(static_cast<T*>(ws)), scale(part + slabs), cnt(reinterpret_cast<int*>(scale + 1)) {}
};

template <typename T>
int loss_forward(const mms_softmax_loss_shape* shape, const T* bottom, const T* label, T* prob, T* loss, void* workspace,
                 size_t workspace_bytes, hipStream_t s) {
  SoftmaxDims d;
  LossDims l;
  const int rc = loss_check<T>(shape, &d, &l);
  if (rc != MMS_OK || d.outer == 0) return rc;
  if (!bottom || !label || !prob || !loss) return MMS_ERR_INVALID_ARG;
  const long long P = (long long)d.outer * d.inner;
  const size_t bytes = (size_t)P * d.channels * sizeof(T), need = fc_loss_workspace_bytes(P, sizeof(T));
  const ByteSpan spans[] = {byte_span(prob, bytes), byte_span(loss, sizeof(T)), byte_span(workspace, need),
                            byte_span(bottom, bytes), byte_span(label, (size_t)P * sizeof(T))};
  if (outputs_overlap(spans, 5, 3)) return MMS_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < need) return MMS_ERR_WORKSPACE;
  const int slabs = fc_loss_slabs(P);
  const LossWs<T> w(workspace, slabs);
  softmax_launch<T, false>(d, bottom, static_cast<const T*>(nullptr), prob, s);
  hipLaunchKernelGGL(fc_loss_finish_kernel<T>, dim3(1), dim3(kFcThreads), 0, s, l, slabs, fc_loss_slab_len(P),
                     (const T*)prob, label, T(0), w.part, w.cnt, loss, static_cast<T*>(nullptr));
  return launch_status();
}

template <typename T>
int loss_backward(const mms_softmax_loss_shape* shape, const T* prob, const T* label, T loss_weight, T* bottom_diff,
                  void* workspace, size_t workspace_bytes, hipStream_t s) {
  SoftmaxDims d;
  LossDims l;
  const int rc = loss_check<T>(shape, &d, &l);
  if (rc != MMS_OK || d.outer == 0) return rc;
  if (!prob || !label || !bottom_diff) return MMS_ERR_INVALID_ARG;
  const long long P = (long long)d.outer * d.inner;
  const size_t bytes = (size_t)P * d.channels * sizeof(T), need = fc_loss_workspace_bytes(P, sizeof(T));
  const ByteSpan spans[] = {byte_span(bottom_diff, bytes), byte_span(workspace, need), byte_span(prob, bytes),
                            byte_span(label, (size_t)P * sizeof(T))};
  if (outputs_overlap(spans, 4, 2)) return MMS_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < need) return MMS_ERR_WORKSPACE;
  const int slabs = fc_loss_slabs(P);
  const LossWs<T> w(workspace, slabs);
  hipLaunchKernelGGL(fc_loss_finish_kernel<T>, dim3(1), dim3(kFcThreads), 0, s, l, slabs, fc_loss_slab_len(P),
                     static_cast<const T*>(nullptr), label, loss_weight, w.part, w.cnt, static_cast<T*>(nullptr),
                     w.scale);
  hipLaunchKernelGGL(fc_loss_diff_kernel<T>, dim3((unsigned)fc_sweep_blocks(P * d.channels)), dim3(kFcThreads), 0, s, l,
                     prob, label, (const T*)w.scale, bottom_diff);
  return launch_status();
}

size_t loss_workspace_bytes(const mms_softmax_loss_shape* shape, size_t elem) {
  SoftmaxDims d;
  if (fc_loss_check(shape, &d) != MMS_OK) return 0;
  return fc_loss_workspace_bytes((long long)d.outer * d.inner, elem);
}

// TO_TOP: ptrs = the bottoms, whole = top; otherwise ptrs = the bottom diffs (NULL: skipped), whole = top_diff
template <typename T, bool TO_TOP>
int concat_call(const mms_concat_shape* shape, const T* const* ptrs, const T* whole, hipStream_t s) {
  ConcatDims d;
  const int rc = fc_concat_check(shape, &d);
  if (rc != MMS_OK || d.num_concats == 0) return rc;
  if (!ptrs || !whole) return MMS_ERR_INVALID_ARG;
  ConcatArgs a = {};
  a.num_concats = d.num_concats;
  a.top_run = d.top_axis * d.inner;
  const size_t top_bytes = (size_t)d.num_concats * a.top_run * sizeof(T);
  const ByteSpan top_span = byte_span(whole, top_bytes);
  ByteSpan bs[MMS_CONCAT_MAX_BOTTOMS];
  bool any = false;
  for (int b = 0; b < d.nb; ++b) {
    a.run[b] = d.extent[b] * d.inner;
    a.offset[b] = d.offset[b] * d.inner;
    a.bottom[b] = a.run[b] ? ptrs[b] : nullptr;
    if (TO_TOP && a.run[b] && !ptrs[b]) return MMS_ERR_INVALID_ARG;
    bs[b] = byte_span(a.bottom[b], (size_t)d.num_concats * a.run[b] * sizeof(T));
    if (spans_meet(bs[b], top_span)) return MMS_ERR_INVALID_ARG;
    if (!TO_TOP)
      for (int c = 0; c < b; ++c)
        if (spans_meet(bs[b], bs[c])) return MMS_ERR_INVALID_ARG;
    any = any || a.bottom[b];
    const size_t run_bytes = (size_t)a.run[b] * sizeof(T);
    a.vec[b] = a.bottom[b] && run_bytes % 16 == 0 && ((size_t)a.top_run * sizeof(T)) % 16 == 0 &&
               aligned16(a.bottom[b]) && aligned16(whole + a.offset[b]);
  }
  if (!TO_TOP && !any) return MMS_ERR_INVALID_ARG;
  if (!any) return MMS_OK;                  // every bottom has extent 0: refused above, top_axis >= 1
  long long most = 0;
  for (int b = 0; b < d.nb; ++b) {
    const long long units = a.bottom[b] ? (long long)d.num_concats * (a.run[b] / (a.vec[b] ? 16 / (int)sizeof(T) : 1)) : 0;
    most = units > most ? units : most;
  }
  typedef typename std::conditional<sizeof(T) == 4, unsigned int, unsigned long long>::type W;
  hipLaunchKernelGGL((fc_concat_kernel<W, TO_TOP>), dim3((unsigned)fc_sweep_blocks(most), (unsigned)d.nb),
                     dim3(kFcThreads), 0, s, a, const_cast<void*>(static_cast<const void*>(whole)));
  return launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

size_t mms_inner_product_workspace_bytes(const mms_inner_product_shape* shape) { return ip_workspace_bytes(shape, 4); }
size_t mms_inner_product_workspace_bytes_f64(const mms_inner_product_shape* shape) { return ip_workspace_bytes(shape, 8); }

int mms_inner_product_route(const mms_inner_product_shape* shape, int pass) {
  FcDims d;
  if (fc_ip_check(shape, &d) != MMS_OK) return MMS_FC_ROUTE_NONE;
  return fc_ip_route(d, pass);
}

int mms_inner_product_forward_f32(const mms_inner_product_shape* shape, const float* x, const float* w, const float* b,
                                  float* top, void* stream) {
  return ip_forward<float>(shape, x, w, b, top, false, as_stream(stream));
}
int mms_inner_product_forward_f64(const mms_inner_product_shape* shape, const double* x, const double* w,
                                  const double* b, double* top, void* stream) {
  return ip_forward<double>(shape, x, w, b, top, true, as_stream(stream));
}
int mms_inner_product_forward_generic_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                          const float* b, float* top, void* stream) {
  return ip_forward<float>(shape, x, w, b, top, true, as_stream(stream));
}
int mms_inner_product_backward_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                   const float* top_diff, float* w_diff, float* b_diff, float* bottom_diff,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return ip_backward<float>(shape, x, w, top_diff, w_diff, b_diff, bottom_diff, workspace, workspace_bytes, false,
                            as_stream(stream));
}
int mms_inner_product_backward_f64(const mms_inner_product_shape* shape, const double* x, const double* w,
                                   const double* top_diff, double* w_diff, double* b_diff, double* bottom_diff,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return ip_backward<double>(shape, x, w, top_diff, w_diff, b_diff, bottom_diff, workspace, workspace_bytes, true,
                             as_stream(stream));
}
int mms_inner_product_backward_generic_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                           const float* top_diff, float* w_diff, float* b_diff, float* bottom_diff,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return ip_backward<float>(shape, x, w, top_diff, w_diff, b_diff, bottom_diff, workspace, workspace_bytes, true,
                            as_stream(stream));
}

int mms_softmax_forward_f32(const mms_softmax_shape* shape, const float* bottom, float* top, void* stream) {
  return softmax_call<float, false>(shape, bottom, nullptr, top, as_stream(stream));
}
int mms_softmax_forward_f64(const mms_softmax_shape* shape, const double* bottom, double* top, void* stream) {
  return softmax_call<double, false>(shape, bottom, nullptr, top, as_stream(stream));
}
int mms_softmax_backward_f32(const mms_softmax_shape* shape, const float* top, const float* top_diff, float* bottom_diff,
                             void* stream) {
  return softmax_call<float, true>(shape, top, top_diff, bottom_diff, as_stream(stream));
}
int mms_softmax_backward_f64(const mms_softmax_shape* shape, const double* top, const double* top_diff,
                             double* bottom_diff, void* stream) {
  return softmax_call<double, true>(shape, top, top_diff, bottom_diff, as_stream(stream));
}

size_t mms_softmax_loss_workspace_bytes(const mms_softmax_loss_shape* shape) { return loss_workspace_bytes(shape, 4); }
size_t mms_softmax_loss_workspace_bytes_f64(const mms_softmax_loss_shape* shape) { return loss_workspace_bytes(shape, 8); }

int mms_softmax_loss_forward_f32(const mms_softmax_loss_shape* shape, const float* bottom, const float* label,
                                 float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return loss_forward<float>(shape, bottom, label, prob, loss, workspace, workspace_bytes, as_stream(stream));
}
int mms_softmax_loss_forward_f64(const mms_softmax_loss_shape* shape, const double* bottom, const double* label,
                                 double* prob, double* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return loss_forward<double>(shape, bottom, label, prob, loss, workspace, workspace_bytes, as_stream(stream));
}
int mms_softmax_loss_backward_f32(const mms_softmax_loss_shape* shape, const float* prob, const float* label,
                                  float loss_weight, float* bottom_diff, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return loss_backward<float>(shape, prob, label, loss_weight, bottom_diff, workspace, workspace_bytes,
                              as_stream(stream));
}
int mms_softmax_loss_backward_f64(const mms_softmax_loss_shape* shape, const double* prob, const double* label,
                                  double loss_weight, double* bottom_diff, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return loss_backward<double>(shape, prob, label, loss_weight, bottom_diff, workspace, workspace_bytes,
                               as_stream(stream));
}

int mms_concat_forward_f32(const mms_concat_shape* shape, const float* const* bottoms, float* top, void* stream) {
  return concat_call<float, true>(shape, bottoms, top, as_stream(stream));
}
int mms_concat_forward_f64(const mms_concat_shape* shape, const double* const* bottoms, double* top, void* stream) {
  return concat_call<double, true>(shape, bottoms, top, as_stream(stream));
}
int mms_concat_backward_f32(const mms_concat_shape* shape, const float* top_diff, float* const* bottom_diffs,
                            void* stream) {
  return concat_call<float, false>(shape, bottom_diffs, top_diff, as_stream(stream));
}
int mms_concat_backward_f64(const mms_concat_shape* shape, const double* top_diff, double* const* bottom_diffs,
                            void* stream) {
  return concat_call<double, false>(shape, bottom_diffs, top_diff, as_stream(stream));
}

}  // extern "C"
