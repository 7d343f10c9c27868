// csrc/fm.hip -- FM (second-order factorization-machine pooling) over the channels of an (N, C, dim) blob, and
// its extern "C" entry points (include/mms.h: mms_fm_*).  The reference's FMLayer<Dtype>::Forward_gpu / Backward_gpu
// call the CPU functions (fm_layer.cu:12-21); the arithmetic restated here is fm_layer.cpp:42-61 and :76-98, whose
// results are fixed by loop order, so every result below is BIT-IDENTICAL to that code (built without contraction:
// `t1 -= x*x` is a rounded multiply, then a subtract).
//
//   forward, per sample:  t1 = 0;  for j = 1..dim-1 { t2 = 0; for k { t2 += x[k,j]; t1 -= x[k,j]*x[k,j]; } t1 += t2*t2; }
//                         t1 /= 2;  for k: t1 += x[k,0];  t1 += bias;  top = t1
//   backward:             bias_diff = 0 + top_diff[0] + top_diff[1] + ...;  bottom_diff[k,0] = g;
//                         bottom_diff[k,j] = g * (t2_j - x[k,j])
//
// t2_j is a C-long chain, independent across j: one thread per (sample, column).  t1 is ONE ordered chain of
// (dim-1)(C+1) + C + 1 dependent adds per sample: it is walked by one lane from an LDS image of its addends, in the
// form of euclid_rows_lanechain_f16_kernel (simcross_rows_f16.hip) -- exact by construction, no speculation.
#include <limits.h>

#include "mms_internal.h"

namespace mms {
namespace {

constexpr int kFmThreads = 256;
constexpr int kFmLoaders = kFmThreads - kWave;      // waves 1..3 stage, wave 0 walks
constexpr int kFmChainChunk = 2048;                 // elements of top_diff staged per step of the bias_diff chain
constexpr int kFmLdsBytes = 48 * 1024;              // both image buffers of the lane-walk kernel (3 workgroups / CU)

// bias_diff[0] = 0 + top_diff[0] + top_diff[1] + ... (fm_layer.cpp:77-80), by ONE workgroup: every thread keeps the
// next chunk's elements in registers (loads in flight during the walk), thread 0 walks the current chunk from LDS.
template <typename T>
__device__ __forceinline__ void fm_bias_chain(const T* __restrict__ top_diff, int N, T* __restrict__ bias_diff,
                                              T* buf) {
  constexpr int PER = kFmChainChunk / kFmThreads;
  const int tid = threadIdx.x;
  T r[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const long long idx = (long long)e * kFmThreads + tid;
    r[e] = idx < N ? top_diff[idx] : T(0);
  }
  T acc = T(0);
  for (long long c0 = 0; c0 < N; c0 += kFmChainChunk) {
#pragma unroll
    for (int e = 0; e < PER; ++e) buf[e * kFmThreads + tid] = r[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const long long idx = c0 + kFmChainChunk + (long long)e * kFmThreads + tid;
      r[e] = idx < N ? top_diff[idx] : T(0);
    }
    if (tid == 0) {
      const int n = (int)((N - c0) < kFmChainChunk ? (N - c0) : kFmChainChunk);
#pragma unroll 8
      for (int i = 0; i < n; ++i) acc += buf[i];
    }
    __syncthreads();
  }
  if (tid == 0) bias_diff[0] = acc;
}

// Forward (BWD = false) or forward + backward (BWD = true), fp32.  A workgroup owns S <= 64 consecutive samples and
// streams their latent columns in panels of P: waves 1..3 load panel p+1 (a thread per (sample, column): the C-long
// t2 chain, coalesced along the columns) and write each sample's addends to LDS IN CHAIN ORDER -- per column
// -(x*x) for k = 0..C-1, then t2*t2 (t1 - v and t1 + (-v) are the same IEEE operation) -- while lane s of wave 0
// walks sample s's image of panel p front to back.  Two buffers, one barrier per panel.  The last "panel" is the
// linear column: t1 /= 2, the C adds of x[k,0], the bias, the store.  With BWD the staging thread, which holds
// t2_j = tt_j, also writes the column's gradients; x is then read twice by the same thread, once from HBM.
// st: floats per sample image, a multiple of 4 with st/4 odd (the walkers' ds_read_b128 spread over the banks).
// With BWD and bias_diff, workgroup 0 is the bias_diff chain and the samples start at workgroup 1.
template <bool BWD>
__global__ __launch_bounds__(kFmThreads) void fm_lanewalk_f32_kernel(
    const float* __restrict__ x, const float* __restrict__ bias, const float* __restrict__ top_diff,
    float* __restrict__ top, float* __restrict__ bottom_diff, float* __restrict__ bias_diff, int N, int C, int dim,
    int S, int P, int st) {
  extern __shared__ float4 fm_lds4[];
  float* lds = reinterpret_cast<float*>(fm_lds4);
  int blk = blockIdx.x;
  if (BWD && bias_diff) {
    if (blk == 0) {
      fm_bias_chain<float>(top_diff, N, bias_diff, lds);
      return;
    }
    --blk;
  }
  const int tid = threadIdx.x;
  const int s0 = blk * S;
  const int ns = (N - s0) < S ? (N - s0) : S;
  const int np = (dim - 1 + P - 1) / P;              // latent panels; panel np is the linear column
  const int C1 = C + 1;
  const size_t sample = (size_t)C * dim;
  const float* xs = x + (size_t)s0 * sample;
  float* bs = BWD ? bottom_diff + (size_t)s0 * sample : nullptr;

  auto stage = [&](int p, float* buf) {
    const int lt = tid - kWave;
    if (p < np) {
      const int j0 = 1 + p * P;
      const int pc = (dim - j0) < P ? (dim - j0) : P;
      for (int it = lt; it < ns * pc; it += kFmLoaders) {
        const int s = it / pc, jj = it - s * pc;
        const float* xp = xs + (size_t)s * sample + j0 + jj;
        float* o = buf + s * st + jj * C1;
        float t2 = 0.f;
#pragma unroll 4
        for (int k = 0; k < C; ++k) {
          const float v = xp[(size_t)k * dim];
          t2 += v;
          o[k] = -(v * v);
        }
        o[C] = t2 * t2;
        if (BWD) {
          const float g = top_diff[s0 + s];
          float* bp = bs + (size_t)s * sample + j0 + jj;
#pragma unroll 4
          for (int k = 0; k < C; ++k)
            __builtin_nontemporal_store(g * (t2 - xp[(size_t)k * dim]), bp + (size_t)k * dim);
        }
      }
    } else {
      for (int it = lt; it < ns * C; it += kFmLoaders) {
        const int s = it / C, k = it - s * C;
        const size_t off = (size_t)s * sample + (size_t)k * dim;
        buf[s * st + k] = xs[off];
        if (BWD) __builtin_nontemporal_store(top_diff[s0 + s], bs + off);
      }
    }
  };

  float t1 = 0.f;
  if (tid >= kWave) stage(0, lds);
  __syncthreads();
  for (int p = 0; p <= np; ++p) {
    if (tid < kWave) {
      if (tid < ns) {
        const float* m = lds + (size_t)(p & 1) * S * st + tid * st;
        if (p < np) {
          const int j0 = 1 + p * P;
          const int n = ((dim - j0) < P ? (dim - j0) : P) * C1;
          const float4* m4 = reinterpret_cast<const float4*>(m);
          const int n4 = n >> 2;
#pragma unroll 4
          for (int i = 0; i < n4; ++i) {
            const float4 v = m4[i];
            t1 += v.x; t1 += v.y; t1 += v.z; t1 += v.w;
          }
          for (int i = n4 * 4; i < n; ++i) t1 += m[i];
        } else {
          t1 = t1 / 2.0f;
          for (int k = 0; k < C; ++k) t1 += m[k];
          if (bias) t1 += bias[0];
          top[s0 + tid] = t1;
        }
      }
    } else if (p < np) {
      stage(p + 1, lds + (size_t)((p + 1) & 1) * S * st);
    }
    __syncthreads();
  }
}

// One thread per sample, the reference's loop as written: the double instantiation, and fp32 shapes whose single
// column (C + 1 addends per sample) does not fit the lane-walk kernel's LDS image.
template <typename T>
__global__ __launch_bounds__(kFmThreads) void fm_forward_thread_kernel(const T* __restrict__ x,
                                                                       const T* __restrict__ bias,
                                                                       T* __restrict__ top, int N, int C, int dim) {
  const int i = blockIdx.x * kFmThreads + threadIdx.x;
  if (i >= N) return;
  const T* xi = x + (size_t)i * C * dim;
  T t1 = T(0);
  for (int j = 1; j < dim; ++j) {
    T t2 = T(0);
    for (int k = 0; k < C; ++k) {
      const T v = xi[(size_t)k * dim + j];
      t2 += v;
      t1 -= v * v;
    }
    t1 += t2 * t2;
  }
  t1 /= T(2);
  for (int k = 0; k < C; ++k) t1 += xi[(size_t)k * dim];
  if (bias) t1 += bias[0];
  top[i] = t1;
}

// Backward, streaming: one thread per (sample, column), consecutive threads on consecutive columns.  Column 0 gets
// top_diff[i] in every channel; column j >= 1 the ascending-k sum tt_j (the forward's t2_j, bit for bit) and then
// g * (tt_j - x).  x is read twice by the same thread; every element of bottom_diff is written once.  With bias_diff,
// workgroup 0 is the bias_diff chain and the columns start at workgroup 1 (no second launch, no atomics).
template <typename T>
__global__ __launch_bounds__(kFmThreads) void fm_backward_kernel(const T* __restrict__ x,
                                                                 const T* __restrict__ top_diff,
                                                                 T* __restrict__ bottom_diff,
                                                                 T* __restrict__ bias_diff, int N, int C, int dim) {
  __shared__ T chain_buf[kFmChainChunk];
  unsigned blk = blockIdx.x;
  if (bias_diff) {
    if (blk == 0) {
      fm_bias_chain<T>(top_diff, N, bias_diff, chain_buf);
      return;
    }
    --blk;
  }
  if (!bottom_diff) return;
  const unsigned idx = blk * kFmThreads + threadIdx.x;       // N * dim <= INT_MAX: the last workgroup stays below 2^32
  if (idx >= (unsigned)N * (unsigned)dim) return;
  const int i = (int)(idx / (unsigned)dim), j = (int)(idx - (unsigned)i * (unsigned)dim);
  const T g = top_diff[i];
  const size_t base = (size_t)i * C * dim + j;
  const T* xp = x + base;
  T* bp = bottom_diff + base;
  if (j == 0) {
    for (int k = 0; k < C; ++k) __builtin_nontemporal_store(g, bp + (size_t)k * dim);
    return;
  }
  T tt = T(0);
#pragma unroll 4
  for (int k = 0; k < C; ++k) tt += xp[(size_t)k * dim];
#pragma unroll 4
  for (int k = 0; k < C; ++k) __builtin_nontemporal_store(g * (tt - xp[(size_t)k * dim]), bp + (size_t)k * dim);
}

// Samples per workgroup, columns per panel and the LDS stride of a sample's image for the lane-walk kernel; false
// when one column's C + 1 addends of 8 samples do not fit (the caller takes the one-thread-per-sample kernel).
// Fewer samples per workgroup while the grid would not reach two workgroups per CU: a walk costs the same time for
// 1 or 64 lanes, so with few samples more workgroups is more chains walked at once; and fewer while a panel would be
// narrower than 8 columns (the staging threads' reads coalesce along the columns of a panel).
struct FmPlan { int S, P, st; };
bool fm_plan(int N, int C, int dim, FmPlan* plan) {
  const int C1 = C + 1;
  for (int S = 64; S >= 8; S /= 2) {
    if ((N + S - 1) / S < 512 && S > 8) continue;
    int room = kFmLdsBytes / (int)sizeof(float) / (2 * S);   // floats per sample per buffer
    room &= ~3;
    if (((room >> 2) & 1) == 0) room -= 4;                   // the largest allowed stride: room / 4 odd
    const int cols = dim > 1 ? dim - 1 : 1;
    if (C1 > room || (S > 8 && room / C1 < (cols < 8 ? cols : 8))) continue;   // panels under 8 columns: 32-byte reads
    int P = room / C1;
    if (P > cols) P = cols;
    const int np = (cols + P - 1) / P;
    P = (cols + np - 1) / np;                                // same number of panels, evenly wide
    int st = (P * C1 + 3) & ~3;
    if (((st >> 2) & 1) == 0) st += 4;                       // <= room: room is of this form and >= P * C1
    plan->S = S; plan->P = P; plan->st = st;
    return true;
  }
  return false;
}

size_t fm_lds_bytes(const FmPlan& p, bool chain) {
  size_t b = (size_t)2 * p.S * p.st * sizeof(float);
  if (chain && b < kFmChainChunk * sizeof(float)) b = kFmChainChunk * sizeof(float);
  return b;
}

unsigned fm_blocks(long long items) { return (unsigned)((items + kFmThreads - 1) / kFmThreads); }

template <typename T>
int fm_backward_launch(int N, int C, int dim, const T* x, const T* top_diff, T* bottom_diff, T* bias_diff,
                       hipStream_t s) {
  if (!bottom_diff && !bias_diff) return MMS_OK;
  const unsigned grid = (bottom_diff ? fm_blocks((long long)N * dim) : 0u) + (bias_diff ? 1u : 0u);
  hipLaunchKernelGGL((fm_backward_kernel<T>), dim3(grid), dim3(kFmThreads), 0, s, x, top_diff, bottom_diff, bias_diff,
                     N, C, dim);
  return launch_status();
}

// N < 0, C <= 0, dim <= 0, or more elements than the reference's int index reaches
bool fm_bad_shape(int N, int C, int dim) {
  if (N < 0 || C <= 0 || dim <= 0) return true;
  const long long nc = (long long)N * C;
  return nc > INT_MAX || nc * dim > INT_MAX;
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_fm_forward_f32(int N, int C, int dim, const float* x, const float* bias, float* top, void* stream) {
  if (fm_bad_shape(N, C, dim)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top) return MMS_ERR_INVALID_ARG;
  hipStream_t s = as_stream(stream);
  FmPlan p;
  if (fm_plan(N, C, dim, &p)) {
    hipLaunchKernelGGL((fm_lanewalk_f32_kernel<false>), dim3((unsigned)((N + p.S - 1) / p.S)), dim3(kFmThreads),
                       fm_lds_bytes(p, false), s, x, bias, (const float*)nullptr, top, (float*)nullptr,
                       (float*)nullptr, N, C, dim, p.S, p.P, p.st);
  } else {
    hipLaunchKernelGGL((fm_forward_thread_kernel<float>), dim3(fm_blocks(N)), dim3(kFmThreads), 0, s, x, bias, top, N,
                       C, dim);
  }
  return launch_status();
}

int mms_fm_backward_f32(int N, int C, int dim, const float* x, const float* top_diff, float* bottom_diff,
                        float* bias_diff, void* stream) {
  if (fm_bad_shape(N, C, dim)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top_diff) return MMS_ERR_INVALID_ARG;
  return fm_backward_launch<float>(N, C, dim, x, top_diff, bottom_diff, bias_diff, as_stream(stream));
}

int mms_fm_forward_backward_f32(int N, int C, int dim, const float* x, const float* bias, const float* top_diff,
                                float* top, float* bottom_diff, float* bias_diff, void* stream) {
  if (fm_bad_shape(N, C, dim)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top_diff || !top || !bottom_diff) return MMS_ERR_INVALID_ARG;
  hipStream_t s = as_stream(stream);
  FmPlan p;
  if (fm_plan(N, C, dim, &p)) {
    const unsigned grid = (unsigned)((N + p.S - 1) / p.S) + (bias_diff ? 1u : 0u);
    hipLaunchKernelGGL((fm_lanewalk_f32_kernel<true>), dim3(grid), dim3(kFmThreads), fm_lds_bytes(p, bias_diff != nullptr),
                       s, x, bias, top_diff, top, bottom_diff, bias_diff, N, C, dim, p.S, p.P, p.st);
    return launch_status();
  }
  hipLaunchKernelGGL((fm_forward_thread_kernel<float>), dim3(fm_blocks(N)), dim3(kFmThreads), 0, s, x, bias, top, N, C,
                     dim);
  if (launch_status() != MMS_OK) return MMS_ERR_LAUNCH;
  return fm_backward_launch<float>(N, C, dim, x, top_diff, bottom_diff, bias_diff, s);
}

int mms_fm_forward_f64(int N, int C, int dim, const double* x, const double* bias, double* top, void* stream) {
  if (fm_bad_shape(N, C, dim)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top) return MMS_ERR_INVALID_ARG;
  hipLaunchKernelGGL((fm_forward_thread_kernel<double>), dim3(fm_blocks(N)), dim3(kFmThreads), 0,
                     as_stream(stream), x, bias, top, N, C, dim);
  return launch_status();
}

int mms_fm_backward_f64(int N, int C, int dim, const double* x, const double* top_diff, double* bottom_diff,
                        double* bias_diff, void* stream) {
  if (fm_bad_shape(N, C, dim)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top_diff) return MMS_ERR_INVALID_ARG;
  return fm_backward_launch<double>(N, C, dim, x, top_diff, bottom_diff, bias_diff, as_stream(stream));
}

}  // extern "C"
