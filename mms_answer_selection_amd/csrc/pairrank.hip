// csrc/pairrank.hip -- PairRankLoss forward/backward and the loss reducers for gfx950 (the fused
// (q, a+, a-) training steps that end in those reducers: triplet_steps.hip, simmatrix.hip).
//
// Reference (src/caffe/layers/pair_rank_loss_layer.cpp):
//   forward  :26-52  diff = a-b ; similar = diff ; ordered = margin - y*diff
//                    (built as sub, mul, axpby(-1,0), add_scalar);
//                    loss = sum_i [max(0,ordered_i) + |(1-y_i)*similar_i|] / count
//   backward :55-84  sign = (i==0 ? -1 : +1) * top_diff/count ;
//                    diff_i = sign*(1[ordered>0]*y - ((1-y)*similar>0 ? 1 : -1)*(1-y))
// Per-element values are bit-identical to the CPU code.  The loss scalar is a
// fixed-shape tree sum (deterministic; the reference's 1-thread running sum
// is not reproduced -- tests hold it to 1e-5 relative).
#include <cmath>

#include "pairrank_math.h"
#include "mms_internal.h"

namespace mms {

// Which comparison gates the hinge term of the backward (include/mms.h: mms_set_pairrank_hinge_mode):
// the reference's Backward_cpu uses `ordered > 0` (pair_rank_loss_layer.cpp:76), its Backward_gpu kernel
// `ordered >= 0` (pair_rank_loss_layer.cu:51).  They differ only where margin - y*(a-b) is exactly 0.
// Per calling thread (a Caffe host runs one thread per GPU); default: the CPU code's strict `>`.
static thread_local int t_hinge_mode = MMS_PAIRRANK_HINGE_CPU;
int pairrank_hinge_mode() { return t_hinge_mode; }
void set_pairrank_hinge_mode(int m) { t_hinge_mode = m; }
static thread_local int t_loss_sum = MMS_LOSS_SUM_FAST;
int loss_sum_mode() { return t_loss_sum; }
void set_loss_sum_mode(int m) { t_loss_sum = m; }

constexpr int kPairThreads = 256;

// Each block reduces a grid-strided slice; block b writes partials[b], or the
// final loss when it is the only block.
__global__ __launch_bounds__(kPairThreads) void pairrank_fwd_kernel(
    int count, float margin, const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ y, float* __restrict__ ordered, float* __restrict__ similar,
    float* __restrict__ partials, float* __restrict__ loss) {
  __shared__ float red[kPairThreads / 64];
  float s = 0.f;
  const int stride = gridDim.x * kPairThreads;
  for (int i = blockIdx.x * kPairThreads + threadIdx.x; i < count; i += stride) {
    const PairTerm p = pair_term(a[i], b[i], y[i], margin);
    ordered[i] = p.ordered;
    similar[i] = p.similar;
    s += p.term;
  }
  s = block_sum<kPairThreads>(s, red);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *loss = s / (float)count;  // :49
    else partials[blockIdx.x] = s;
  }
}

// One block: sums `n` partials in a fixed order and writes sum/count.
__global__ __launch_bounds__(kPairThreads) void loss_finish_kernel(
    const float* __restrict__ partials, int n, int count, float* __restrict__ loss) {
  __shared__ float red[kPairThreads / 64];
  float s = 0.f;
  // eight independent loads in flight per thread (a one-block kernel is pure latency: a
  // load-add-load-add loop costs one memory round trip per element), added in index order
  for (int base = threadIdx.x; base < n; base += 8 * kPairThreads) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = base + u * kPairThreads;
      v[u] = partials[i < n ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (base + u * kPairThreads < n) ? v[u] : 0.f;
  }
  s = block_sum<kPairThreads>(s, red);
  if (threadIdx.x == 0) *loss = s / (float)count;
}

// MMS_LOSS_SUM_REFERENCE: the reference's own sum -- ONE running fp32 accumulator over the terms in index order
// (pair_rank_loss_layer.cpp:41-49) -- so that the loss scalar carries the CPU code's bits, drift and all.  A
// dependent chain of `count` adds by one lane (~3 ns each); the other threads only stage the next terms in LDS.
// terms != nullptr: the per-element terms as the fused step stored them; otherwise they are formed from the
// layer's own outputs, max(0, ordered) + |(1 - y) * similar| (:43-44).
constexpr int kRunChunk = 4096;
__global__ __launch_bounds__(256) void loss_running_sum_kernel(
    const float* __restrict__ terms, const float* __restrict__ ordered, const float* __restrict__ similar,
    const float* __restrict__ y, int count, float* __restrict__ loss) {
  __shared__ float buf[2][kRunChunk];
  auto stage = [&](int b, int base, int first, int nthreads) {   // threads [first, first + nthreads) fill buf[b]
    for (int e = (int)threadIdx.x - first; e < kRunChunk; e += nthreads) {
      const int i = base + e;
      float t = 0.f;
      if (i < count) {
        if (terms) t = terms[i];
        else {
          const float o = ordered[i];
          const float hinge = (0.0f < o) ? o : 0.0f;
          t = hinge + fabsf((1.0f - y[i]) * similar[i]);
        }
      }
      buf[b][e] = t;
    }
  };
  stage(0, 0, 0, 256);
  __syncthreads();
  float l = 0.f;
  for (int base = 0, b = 0; base < count; base += kRunChunk, b ^= 1) {
    if (threadIdx.x >= 64) {                       // the other waves fetch the next chunk meanwhile
      if (base + kRunChunk < count) stage(b ^ 1, base + kRunChunk, 64, 192);
    } else if (threadIdx.x == 0) {
      const int n = min(kRunChunk, count - base);
      int e = 0;
      for (; e + 8 <= n; e += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = buf[b][e + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) l += v[u];
      }
      for (; e < n; ++e) l += buf[b][e];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = l / (float)count;  // :49
}

__global__ __launch_bounds__(256) void pairrank_bwd_kernel(
    int count, float s0, float s1, const float* __restrict__ y,
    const float* __restrict__ ordered, const float* __restrict__ similar,
    float* __restrict__ da, float* __restrict__ db, int hinge_ge) {
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
    float ga, gb;
    pair_grad(y[i], ordered[i], similar[i], s0, s1, ga, gb, hinge_ge != 0);
    if (da) da[i] = ga;
    if (db) db[i] = gb;
  }
}

static int pair_blocks(int count) {
  int b = (count + kPairThreads * 4 - 1) / (kPairThreads * 4);  // ~4 elements per thread
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return b;
}
// Batches of at most 8192 elements (the reference's use: one score column of 50 .. 4096 pairs) in ONE
// launch: a single 1024-thread workgroup, up to eight elements per thread with all 24 loads issued
// before the first use, fixed-order block sum.  Saves the separate loss-finish launch.
constexpr int kSmallThreads = 1024, kSmallMax = 8 * kSmallThreads;
__global__ __launch_bounds__(kSmallThreads) void pairrank_fwd_small_kernel(
    int count, float margin, const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ y, float* __restrict__ ordered, float* __restrict__ similar,
    float* __restrict__ loss) {
  __shared__ float red[kSmallThreads / 64];
  float va[8], vb[8], vy[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = threadIdx.x + u * kSmallThreads;
    const int ii = i < count ? i : 0;
    va[u] = a[ii]; vb[u] = b[ii]; vy[u] = y[ii];
  }
  // all 24 values in registers before the first store: the stores sit under `i < count`, so the compiler cannot
  // count them and the wait for the NEXT value became vmcnt(0) -- the acknowledgement of the stores just issued
#pragma unroll
  for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(va[u]), "+v"(vb[u]), "+v"(vy[u]));
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = threadIdx.x + u * kSmallThreads;
    if (i < count) {
      const PairTerm p = pair_term(va[u], vb[u], vy[u], margin);
      ordered[i] = p.ordered;
      similar[i] = p.similar;
      s += p.term;
    }
  }
  s = block_sum<kSmallThreads>(s, red);
  if (threadIdx.x == 0) *loss = s / (float)count;   // :49
}

size_t pairrank_workspace_bytes(int count) {
  const int b = pair_blocks(count);
  return b > 1 ? (size_t)b * sizeof(float) : 0;
}

int pairrank_forward(int count, float margin, const float* a, const float* b, const float* y,
                     float* ordered, float* similar, float* loss, void* ws, size_t ws_bytes,
                     hipStream_t s) {
  if (count <= kSmallMax) {
    hipLaunchKernelGGL(pairrank_fwd_small_kernel, dim3(1), dim3(kSmallThreads), 0, s, count, margin, a,
                       b, y, ordered, similar, loss);
    if (loss_sum_mode() == MMS_LOSS_SUM_REFERENCE)
      hipLaunchKernelGGL(loss_running_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)nullptr, ordered,
                         similar, y, count, loss);
    return launch_status();
  }
  const int blocks = pair_blocks(count);
  if (blocks > 1 && (ws == nullptr || ws_bytes < (size_t)blocks * sizeof(float)))
    return MMS_ERR_WORKSPACE;
  float* partials = static_cast<float*>(ws);
  hipLaunchKernelGGL(pairrank_fwd_kernel, dim3(blocks), dim3(kPairThreads), 0, s, count, margin,
                     a, b, y, ordered, similar, partials, loss);
  if (loss_sum_mode() == MMS_LOSS_SUM_REFERENCE)
    hipLaunchKernelGGL(loss_running_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)nullptr, ordered,
                       similar, y, count, loss);
  else if (blocks > 1)
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kPairThreads), 0, s, partials, blocks,
                       count, loss);
  return launch_status();
}

int pairrank_backward(int count, float top_diff, const float* y, const float* ordered,
                      const float* similar, float* da, float* db, hipStream_t s) {
  if (count == 0 || (da == nullptr && db == nullptr)) return MMS_OK;
  // :64  sign *= top[0]->cpu_diff()[0] / bottom[0]->count()   (float / int -> float)
  const float scale = top_diff / (float)count;
  const float s0 = -1.0f * scale, s1 = 1.0f * scale;
  int blocks = (count + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pairrank_bwd_kernel, dim3(blocks), dim3(256), 0, s, count, s0, s1, y,
                     ordered, similar, da, db, pairrank_hinge_mode() == MMS_PAIRRANK_HINGE_GPU ? 1 : 0);
  return launch_status();
}

// loss = (sum of the N per-triplet terms) / N from a device array of terms: the tail of both fused steps
// (pair_rank_loss_layer.cpp:41-49).  MMS_LOSS_SUM_REFERENCE: the reference's running fp32 sum, else the fixed tree.
int triplet_loss_from_terms(const float* terms, int N, float* loss, hipStream_t s) {
  if (loss_sum_mode() == MMS_LOSS_SUM_REFERENCE)
    hipLaunchKernelGGL(loss_running_sum_kernel, dim3(1), dim3(256), 0, s, terms, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, N, loss);
  else
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kPairThreads), 0, s, terms, N, N, loss);
  return launch_status();
}

}  // namespace mms
