// csrc/bn_common.h -- what csrc/bn.hip (BN) and csrc/bn_pool.hip (BN -> AvePool / MaxPool -> TanH) share: the sizes of
// the two routes, the workgroup sum with its fixed order, the ascending fold of a channel's chunk sums and the TRAIN
// statistics made from them; and what csrc/bn_pool.hip shares with csrc/conv_stage.hip: a window's TEST-phase finish,
// AVE and MAX, and MAX's scan step; and with csrc/conv_stage_train.hip: the TRAIN-phase finish and the statistics.
#ifndef MMS_BN_COMMON_H_
#define MMS_BN_COMMON_H_

#include "mms_common.h"

namespace mms {

constexpr int kBnThreads = 256;             // a (channel, chunk) workgroup of the large route
constexpr int kBnSmallThreads = 1024;       // the one workgroup of a channel on the small route
constexpr int kBnBatch = 4;                 // groups a thread has in flight before it uses the first
// The routing threshold, in 16-byte groups per channel (16384 floats, 8192 doubles: 64 KB).  Up to here the one
// workgroup of 1024 threads covers its channel with ONE batch of kBnBatch loads per thread and pass, i.e. in about one
// memory round trip, which is what the second launch of the large route would cost on its own.
constexpr unsigned kBnSmallGroups = kBnSmallThreads * kBnBatch;
constexpr unsigned kBnChunkGroups = 2048;   // smallest chunk: 32 KB, two batches per thread of 256
constexpr int kBnMaxChunks = 64;            // longest fold every workgroup of launch 2 repeats in its prologue
constexpr int kBnSlots = 4;                 // workspace words per (channel, chunk): forward uses 2, backward 4

template <typename T>
using bn_vec = T __attribute__((ext_vector_type(16 / sizeof(T))));

__device__ __forceinline__ float bn_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double bn_sqrt(double v) { return sqrt(v); }

__device__ __forceinline__ float bn_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ double bn_tanh(double v) { return tanh(v); }

// The TEST-phase finish of one pooling window of BN -> AvePool -> TanH, from the window's sum s (its ke elements added
// in (h, w) order, starting from 0), nmean = -mean and std = sqrt(var + 1e-9) of its channel: *save_pool and the return
// value, top.  csrc/bn_pool.hip's sweep and csrc/conv_stage.hip's epilogue both finish with it.
template <typename T>
__device__ __forceinline__ T bn_pool_test_finish(T s, T ke, T nmean, T std, T sc, T sh, T* save_pool) {
  const T m = s / ke;
  const T sp = (m + nmean) / std;
  *save_pool = sp;
  return bn_tanh(sp * sc + sh);
}

// BN for one element, from nmean = -mean, std, scale and shift of its channel, in its two steps: bn_out(x) is
// bp_bn_out(bp_normalised(x, ...), ...).  The only place that forms them: the MAX forward's finish and the MAX
// backward's search for the mask compare their words.
template <typename T>
__device__ __forceinline__ T bp_normalised(T x, T nmean, T std) {
  return (x + nmean) / std;
}
template <typename T>
__device__ __forceinline__ T bp_bn_out(T xn, T sc, T sh) {
  return xn * sc + sh;
}

// MAX: one step of the scan for a window's extremum, in (h, w) order.  The first element starts it; a later one
// replaces *e where it is strictly larger (dir > 0: the channel's scale is positive) or smaller (dir < 0: negative); a
// NaN never does, and with dir == 0 (scale == 0: every BN output is shift, the mask is the first element) nothing does.
// csrc/bn_pool.hip's sweeps and csrc/conv_stage.hip's MAX epilogue all scan with it.
template <typename T>
__device__ __forceinline__ void bp_keep(bool first, T v, int dir, T* e) {
  const bool less = v < *e, more = v > *e;           // both formed, then selected: no branch per element
  *e = first || (dir < 0 ? less : dir > 0 && more) ? v : *e;
}

// dir of bp_keep for a channel's scale
template <typename T>
__device__ __forceinline__ int bp_dir(T sc) {
  return sc < T(0) ? -1 : sc > T(0) ? 1 : 0;
}

// The TEST-phase finish of one pooling window of BN -> MaxPool -> TanH, from the window's extremum e (bp_keep's):
// *save_pool and the return value, top.  csrc/bn_pool.hip's sweep and csrc/conv_stage.hip's MAX epilogue both finish
// with it.
template <typename T>
__device__ __forceinline__ T bn_maxpool_test_finish(T e, T nmean, T std, T sc, T sh, T* save_pool) {
  const T sp = bp_normalised(e, nmean, std);
  *save_pool = sp;
  return bn_tanh(bp_bn_out(sp, sc, sh));
}

// The TRAIN-phase finish of one pooling window, AVE and MAX alike, once the channel's statistics are known: from m, the
// window's mean (AVE: its sum / (kh kw)) or extremum (MAX: bp_keep's) as the sweep left it, *save_pool and the return
// value, top.  csrc/bn_pool.hip's bp_finish and csrc/conv_stage_train.hip's second launch both finish with it.
template <typename T>
__device__ __forceinline__ T bn_pool_train_finish(T m, T nmean, T std, T sc, T sh, T* save_pool) {
  const T sp = bp_normalised(m, nmean, std);
  *save_pool = sp;
  return bn_tanh(bp_bn_out(sp, sc, sh));
}

__device__ __forceinline__ float bn_wave_sum(float v) { return wave_sum(v); }
__device__ __forceinline__ double bn_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// NQ sums across a workgroup at once; every thread ends with the totals.  red: NQ * THREADS / 64 words of LDS.
template <int THREADS, int NQ, typename T>
__device__ __forceinline__ void bn_block_sum(T (&v)[NQ], T* red) {
  constexpr int W = THREADS / kWave;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = bn_wave_sum(v[q]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q * W + wid] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    T t = red[q * W];
    for (int w = 1; w < W; ++w) t += red[q * W + w];
    v[q] = t;
  }
}

// The channel's NQ sums from its chunks' workspace slots, ascending: ((chunk 0 + chunk 1) + chunk 2) + ...
template <int NQ, typename T>
__device__ __forceinline__ void bn_fold(const T* __restrict__ ws, int c, int chunks, T (&tot)[NQ]) {
  const T* p = ws + (size_t)c * chunks * kBnSlots;
#pragma unroll
  for (int q = 0; q < NQ; ++q) tot[q] = p[q];
  for (int j = 1; j < chunks; ++j) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) tot[q] += p[j * kBnSlots + q];
  }
}

// TRAIN: mean, var and std of channel c from its two sums over N images of S elements (inv_N, inv_S: the reciprocals);
// the writer updates the running blobs and stores mean and std for the backward.  *nmean = -mean.  Both TRAIN forwards
// of csrc/bn_pool.hip call it, and a new caller should.  bn_forward_kernel (csrc/bn.hip) still spells the same formulas
// out, with one sqrt after its TRAIN and TEST branches join: calling this there changes the kernel's instructions.
template <typename T>
__device__ __forceinline__ void bn_statistics(const T (&tot)[2], int c, bool writer, T bn_memory, T inv_S, T inv_N,
                                              T* running_mean, T* running_var, T* save_mean, T* save_std, T* nmean,
                                              T* std) {
  const T mean = inv_N * (inv_S * tot[0]);
  const T var = inv_N * (inv_S * tot[1]) - mean * mean;        // not clamped: the reference does not either
  *nmean = -mean;
  *std = bn_sqrt(var + T(1e-9));
  if (writer) {
    const T keep = bn_memory, take = T(1) - bn_memory;
    running_mean[c] = take * mean + keep * running_mean[c];
    running_var[c] = take * var + keep * running_var[c];
    save_mean[c] = mean;
    save_std[c] = *std;
  }
}

}  // namespace mms
#endif  // MMS_BN_COMMON_H_
