// csrc/dropout.hip -- Dropout (include/mms_dropout.h: mms_dropout_*): the reference's y = x * mask * scale with the mask
// a pure function of (seed, sequence, global element index), Philox4x32-10, so that the backward regenerates it and no
// rand_vec_ (4 bytes per element, written in the forward and read in the backward) exists.
//
// The work is elementwise and streaming: one array in, one out, nothing reused.  So:
//
//   work unit   one Philox GROUP: the four consecutive global indices 4G .. 4G+3 that one generator call serves.  A lane
//               owns whole groups, so no word is computed twice and none is thrown away but in the ragged first and
//               last group of a call.  Group k of a call is G = (offset >> 2) + k and holds the call's elements
//               4k - p .. 4k - p + 3, p = offset & 3; ceil((p + count) / 4) groups in all.
//   access      VEC: p == 0 and both arrays 16-byte aligned -- a full group is one 16-byte load and store in float, two
//               in double.  Otherwise, and in a partial group, one element at a time under 0 <= i < count.  Both run
//               drop_element on the same (x, word): the same words.
//   loop        grid-stride over groups, kDropGroupsPerTrip = 2 groups per trip: both loads are issued before either
//               generator call, whose ~20 integer multiplies then run under the loads.  At most kDropMaxBlocks
//               workgroups of 256: eight per CU, which is the residency of a kernel this small.
//   operands    thr and scale come from the host (dropout_consts, one definition for the threshold calls and the
//               launches).  Every kernel argument is a plain scalar, 13 dwords in float and 14 in double (the mask
//               writer: 10): the 14 user SGPRs that kernarg preload (build.py) has beside the argument pointer hold
//               them all.  What can be derived is derived in the kernel rather than passed or fetched: the first group
//               and the phase from the offset, the group count from count and phase, the stride from the group count
//               (drop_blocks, the host's own grid rule, so no hidden-argument load of gridDim).  In the ISA the only
//               scalar loads left are those of the compatibility prologue in front of the kernel's entry.
//
// Forward and backward are the same map on other arrays and share the kernel.  TEST out of place is a device copy.
#include <limits.h>

#include "mms_dropout.h"
#include "mms_internal.h"

namespace mms {
namespace {

constexpr int kDropThreads = MMS_DROPOUT_THREADS;
constexpr int kDropMaxBlocks = MMS_DROPOUT_MAX_BLOCKS;
constexpr int kDropGroupsPerTrip = MMS_DROPOUT_GROUPS_PER_TRIP;
static_assert(kDropGroupsPerTrip == 2, "dropout_kernel's trip is written out for two groups");

template <typename T>
struct DropVec;
template <>
struct DropVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct DropVec<double> { typedef double type __attribute__((ext_vector_type(2))); };
typedef unsigned mms_v4u __attribute__((ext_vector_type(4)));

struct DropKey {                 // what the words of a call depend on, but for the group; host side and in registers
  uint32_t k0, k1, s0, s1;       // lo32 / hi32 of seed and of sequence
  uint64_t first;                // offset >> 2: the call's first group
  int p;                         // offset & 3
};

__host__ __device__ __forceinline__ DropKey drop_key(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, uint64_t offset) {
  const DropKey key = {k0, k1, s0, s1, offset >> 2, (int)(offset & 3u)};
  return key;
}
// groups of a call of count > 0 elements at phase p, and the workgroups launched for them
__host__ __device__ __forceinline__ long long drop_groups(long long count, int p) { return (p + count + 3) >> 2; }
__host__ __device__ __forceinline__ long long drop_blocks(long long ngroups) {
  const long long blocks = (ngroups + kDropThreads - 1) / kDropThreads;
  return blocks < kDropMaxBlocks ? blocks : kDropMaxBlocks;
}

// Philox4x32-10 of the counter (lo32(G), hi32(G), s0, s1) under the key (k0, k1)
__device__ __forceinline__ void drop_words(const DropKey& key, uint64_t k, uint32_t w[4]) {
  const uint64_t G = key.first + k;
  uint32_t c0 = (uint32_t)G, c1 = (uint32_t)(G >> 32), c2 = key.s0, c3 = key.s1, k0 = key.k0, k1 = key.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// One element; two roundings (include/mms_dropout.h).
template <typename T>
__device__ __forceinline__ T drop_element(T x, uint32_t word, uint32_t thr, T scale) {
  const T m = x * T(word > thr ? 1u : 0u);
  return m * scale;
}

// the four elements i0 .. i0 + 3 of the call (i0 may be negative in the first group, i0 + 3 >= count in the last)
template <typename T, bool VEC>
__device__ __forceinline__ void drop_load(const T* x, long long i0, long long count, T v[4]) {
  typedef typename DropVec<T>::type V;
  constexpr int VW = 16 / sizeof(T), NV = 4 / VW;
  if (VEC && i0 + 4 <= count) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const V xv = reinterpret_cast<const V*>(x + i0)[q];
#pragma unroll
      for (int j = 0; j < VW; ++j) v[q * VW + j] = xv[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i0 + j;
      v[j] = (i >= 0 && i < count) ? x[i] : T(0);
    }
  }
}

template <typename T, bool VEC>
__device__ __forceinline__ void drop_store(T* y, long long i0, long long count, const T v[4]) {
  typedef typename DropVec<T>::type V;
  constexpr int VW = 16 / sizeof(T), NV = 4 / VW;
  if (VEC && i0 + 4 <= count) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      V yv;
#pragma unroll
      for (int j = 0; j < VW; ++j) yv[j] = v[q * VW + j];
      reinterpret_cast<V*>(y + i0)[q] = yv;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i0 + j;
      if (i >= 0 && i < count) y[i] = v[j];
    }
  }
}

// y = (x * keep) * scale over the call's groups [0, ngroups)
template <typename T, bool VEC>
__global__ __launch_bounds__(kDropThreads) void dropout_kernel(const T* x, T* y, uint64_t offset, T scale, int count32,
                                                               uint32_t thr, uint32_t k0, uint32_t k1, uint32_t s0,
                                                               uint32_t s1) {
  const DropKey key = drop_key(k0, k1, s0, s1, offset);
  const long long count = count32;
  const long long ngroups = drop_groups(count, key.p);
  const long long stride = drop_blocks(ngroups) * kDropThreads;
  for (long long ka = (long long)blockIdx.x * kDropThreads + threadIdx.x; ka < ngroups;
       ka += kDropGroupsPerTrip * stride) {
    const long long kb = ka + stride;
    const bool two = kb < ngroups;
    const long long ia = 4 * ka - key.p, ib = 4 * kb - key.p;
    T a[4], b[4];
    drop_load<T, VEC>(x, ia, count, a);
    if (two) drop_load<T, VEC>(x, ib, count, b);
    uint32_t w[4];
    drop_words(key, (uint64_t)ka, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = drop_element(a[j], w[j], thr, scale);
    drop_store<T, VEC>(y, ia, count, a);
    if (two) {
      drop_words(key, (uint64_t)kb, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = drop_element(b[j], w[j], thr, scale);
      drop_store<T, VEC>(y, ib, count, b);
    }
  }
}

// mask = keep, as 0 / 1 words
template <bool VEC>
__global__ __launch_bounds__(kDropThreads) void dropout_mask_kernel(unsigned* mask, uint64_t offset, int count32,
                                                                    uint32_t thr, uint32_t k0, uint32_t k1, uint32_t s0,
                                                                    uint32_t s1) {
  const DropKey key = drop_key(k0, k1, s0, s1, offset);
  const long long count = count32;
  const long long ngroups = drop_groups(count, key.p);
  const long long stride = drop_blocks(ngroups) * kDropThreads;
  for (long long k = (long long)blockIdx.x * kDropThreads + threadIdx.x; k < ngroups; k += stride) {
    const long long i0 = 4 * k - key.p;
    uint32_t w[4];
    drop_words(key, (uint64_t)k, w);
    if (VEC && i0 + 4 <= count) {
      mms_v4u m;
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = w[j] > thr ? 1u : 0u;
      *reinterpret_cast<mms_v4u*>(mask + i0) = m;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = i0 + j;
        if (i >= 0 && i < count) mask[i] = w[j] > thr ? 1u : 0u;
      }
    }
  }
}

// thr and scale of a ratio, as the reference's LayerSetUp computes them in Dtype = T
template <typename T>
int dropout_consts(T r, unsigned* thr, T* scale) {
  if (!(r > T(0) && r < T(1))) return MMS_ERR_INVALID_ARG;   // NaN fails both
  const T t = T(UINT_MAX) * r;
  if (!(t < T(4294967296.0))) return MMS_ERR_INVALID_ARG;
  *thr = (unsigned)t;
  *scale = T(1. / (1. - (double)r));
  return MMS_OK;
}

// what every launching call judges alike; *key and *ngroups are set for count > 0
int dropout_check(long long count, unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                  DropKey* key, long long* ngroups) {
  if (count < 0 || count > INT_MAX) return MMS_ERR_INVALID_ARG;
  if (offset > ULLONG_MAX - (unsigned long long)count) return MMS_ERR_INVALID_ARG;
  *key = drop_key((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)sequence, (uint32_t)(sequence >> 32), offset);
  *ngroups = drop_groups(count, key->p);
  return MMS_OK;
}

inline dim3 dropout_grid(long long ngroups) { return dim3((unsigned)drop_blocks(ngroups)); }

template <typename T>
int dropout_apply(const T* x, T* y, long long count, T ratio, int phase, unsigned long long seed,
                  unsigned long long sequence, unsigned long long offset, hipStream_t s) {
  unsigned thr = 0;
  T scale = T(0);
  DropKey key;
  long long ngroups = 0;
  int rc = dropout_consts<T>(ratio, &thr, &scale);
  if (rc != MMS_OK) return rc;
  if (phase != MMS_DROPOUT_TRAIN && phase != MMS_DROPOUT_TEST) return MMS_ERR_INVALID_ARG;
  if ((rc = dropout_check(count, seed, sequence, offset, &key, &ngroups)) != MMS_OK) return rc;
  if (count == 0) return MMS_OK;
  if (!x || !y) return MMS_ERR_INVALID_ARG;
  const size_t bytes = (size_t)count * sizeof(T);
  if (x != y && spans_meet(byte_span(x, bytes), byte_span(y, bytes))) return MMS_ERR_INVALID_ARG;     // in place, or apart
  if (phase == MMS_DROPOUT_TEST) {
    if (x == y) return MMS_OK;
    return hipMemcpyAsync(y, x, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? MMS_OK : MMS_ERR_LAUNCH;
  }
  const dim3 grid = dropout_grid(ngroups), block(kDropThreads);
  if (key.p == 0 && aligned16(x) && aligned16(y))
    hipLaunchKernelGGL((dropout_kernel<T, true>), grid, block, 0, s, x, y, offset, scale, (int)count, thr, key.k0, key.k1,
                       key.s0, key.s1);
  else
    hipLaunchKernelGGL((dropout_kernel<T, false>), grid, block, 0, s, x, y, offset, scale, (int)count, thr, key.k0, key.k1,
                       key.s0, key.s1);
  return launch_status();
}

template <typename T>
int dropout_mask(unsigned* mask, long long count, T ratio, unsigned long long seed, unsigned long long sequence,
                 unsigned long long offset, hipStream_t s) {
  unsigned thr = 0;
  T scale = T(0);
  DropKey key;
  long long ngroups = 0;
  int rc = dropout_consts<T>(ratio, &thr, &scale);
  if (rc != MMS_OK) return rc;
  if ((rc = dropout_check(count, seed, sequence, offset, &key, &ngroups)) != MMS_OK) return rc;
  if (count == 0) return MMS_OK;
  if (!mask) return MMS_ERR_INVALID_ARG;
  const dim3 grid = dropout_grid(ngroups), block(kDropThreads);
  if (key.p == 0 && aligned16(mask))
    hipLaunchKernelGGL((dropout_mask_kernel<true>), grid, block, 0, s, mask, offset, (int)count, thr, key.k0, key.k1,
                       key.s0, key.s1);
  else
    hipLaunchKernelGGL((dropout_mask_kernel<false>), grid, block, 0, s, mask, offset, (int)count, thr, key.k0, key.k1,
                       key.s0, key.s1);
  return launch_status();
}

template <typename T>
int dropout_threshold(T ratio, unsigned* thr, T* scale) {
  if (!thr || !scale) return MMS_ERR_INVALID_ARG;
  unsigned t = 0;
  T sc = T(0);
  const int rc = dropout_consts<T>(ratio, &t, &sc);
  if (rc != MMS_OK) return rc;
  *thr = t;
  *scale = sc;
  return MMS_OK;
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_dropout_threshold_f32(float ratio, unsigned int* thr, float* scale) {
  return dropout_threshold<float>(ratio, thr, scale);
}

int mms_dropout_threshold_f64(double ratio, unsigned int* thr, double* scale) {
  return dropout_threshold<double>(ratio, thr, scale);
}

int mms_dropout_forward_f32(const float* x, float* y, long long count, float ratio, int phase, unsigned long long seed,
                            unsigned long long sequence, unsigned long long offset, void* stream) {
  return dropout_apply<float>(x, y, count, ratio, phase, seed, sequence, offset, as_stream(stream));
}

int mms_dropout_forward_f64(const double* x, double* y, long long count, double ratio, int phase,
                            unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                            void* stream) {
  return dropout_apply<double>(x, y, count, ratio, phase, seed, sequence, offset, as_stream(stream));
}

int mms_dropout_backward_f32(const float* dy, float* dx, long long count, float ratio, int phase,
                             unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                             void* stream) {
  return dropout_apply<float>(dy, dx, count, ratio, phase, seed, sequence, offset, as_stream(stream));
}

int mms_dropout_backward_f64(const double* dy, double* dx, long long count, double ratio, int phase,
                             unsigned long long seed, unsigned long long sequence, unsigned long long offset,
                             void* stream) {
  return dropout_apply<double>(dy, dx, count, ratio, phase, seed, sequence, offset, as_stream(stream));
}

int mms_dropout_mask_u32(unsigned int* mask, long long count, float ratio, unsigned long long seed,
                         unsigned long long sequence, unsigned long long offset, void* stream) {
  return dropout_mask<float>(mask, count, ratio, seed, sequence, offset, as_stream(stream));
}

int mms_dropout_mask_u32_f64(unsigned int* mask, long long count, double ratio, unsigned long long seed,
                             unsigned long long sequence, unsigned long long offset, void* stream) {
  return dropout_mask<double>(mask, count, ratio, seed, sequence, offset, as_stream(stream));
}

}  // extern "C"
