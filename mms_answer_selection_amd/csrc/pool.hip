// csrc/pool.hip -- Pooling and TanH as layers of their own (include/mms_pool.h: mms_pool_*, mms_tanh_*): the reference's
// pooling_layer.cpp loops, MAX and AVE over any kernel, stride and padding, and tanh_layer.cpp.  Every call is one
// launch, HBM-bound: bottom (or bottom_diff) is the large array, top is its (stride_h * stride_w)-th part.
//
//   forward    A workgroup takes ITEMS (csrc/pool_plans.h: whole planes, or a band of output rows of one plane), copies
//              an item's input rows -- one contiguous range of bottom -- into LDS and pools from there: each row is read
//              from memory once per workgroup, however the windows overlap.  The copy runs in 16-byte loads between the
//              first and the last 16-byte boundary of the range and one element at a time outside them, and the LDS
//              image keeps the range's offset from a 16-byte boundary so that the 16-byte LDS writes are aligned too:
//              any W and any element-aligned base take the same code and give the same words.  Then one lane per output
//              walks its clipped window in the reference's order (pool_window).  A window that is the whole map is one
//              dependent chain per plane: the item is then many planes, lane p walks plane p, and the other workgroups
//              of the CU load meanwhile (eight are resident).  Where not even one output row's rows fit the LDS a
//              thread per output reads its window from memory.
//   backward   The reference's scatter stated as a gather (the header has the order argument): a thread owns 16 bytes
//              of bottom_diff (one element where the array is not 16-byte aligned, and in the ragged tail), and for
//              each element walks the windows that contain it in ascending (ph, pw).  top_diff and the mask are the
//              small arrays and come through the caches.
//   tanh       16 bytes per thread and trip where every array of the call is 16-byte aligned, an element otherwise;
//              pool_tanh / pool_tanh_diff are the only arithmetic, so both give the same words.
//
// No index exceeds int below the refused counts: element indices of bottom and top are < 2^31, offsets are formed in
// size_t.  No grid dimension exceeds kPoolMaxBlocks.
#include <float.h>

#include "bn_common.h"
#include "mms_internal.h"
#include "pool_plans.h"

namespace mms {
namespace {

// One output: the clipped window of (ph, pw), walked in (h, w) order over `m`, which is indexed as the plane is
// (m[h * W + w]).  MAX: *idx = h * W + w of the first maximum, -1 where nothing replaced -FLT_MAX.
template <typename T, int METHOD>
__device__ __forceinline__ T pool_window(const PoolGeom& g, const T* m, int ph, int pw, int* idx) {
  int hs = ph * g.sh - g.pad_h, ws = pw * g.sw - g.pad_w;
  if (METHOD == MMS_POOL_MAX) {
    const int he = min(hs + g.kh, g.H), we = min(ws + g.kw, g.W);
    hs = max(hs, 0);
    ws = max(ws, 0);
    T best = T(-FLT_MAX);
    int at = -1;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) {
        const T v = m[h * g.W + w];
        if (v > best) {
          best = v;
          at = h * g.W + w;
        }
      }
    *idx = at;
    return best;
  } else {
    int he = min(hs + g.kh, g.H + g.pad_h), we = min(ws + g.kw, g.W + g.pad_w);
    const int pool_size = (he - hs) * (we - ws);
    hs = max(hs, 0);
    ws = max(ws, 0);
    he = min(he, g.H);
    we = min(we, g.W);
    T sum = T(0);
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) sum += m[h * g.W + w];
    return sum / T(pool_size);
  }
}

template <typename T>
__device__ __forceinline__ void pool_store(T* top, int* mask, T* top_mask, size_t i, T v, int idx) {
  top[i] = v;
  if (mask) mask[i] = idx;
  if (top_mask) top_mask[i] = T(idx);
}

// kPoolStaged (bands == 1: P planes per item) and kPoolBanded (P == 1: a band of R output rows per item)
template <typename T, int METHOD>
__global__ __launch_bounds__(kPoolThreads) void pool_forward_staged_kernel(PoolGeom g, int P, int R, int bands, int items,
                                                                          const T* __restrict__ bottom,
                                                                          T* __restrict__ top, int* __restrict__ mask,
                                                                          T* __restrict__ top_mask) {
  extern __shared__ float4 pool_lds4[];
  T* const lds = reinterpret_cast<T*>(pool_lds4);
  typedef bn_vec<T> V;
  constexpr int VW = 16 / sizeof(T);
  const int tid = threadIdx.x, HW = g.H * g.W, PHW = g.PH * g.PW;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    int plane0, np, ph0, ph1;
    if (bands == 1) {
      plane0 = item * P;
      np = min(P, g.planes - plane0);
      ph0 = 0;
      ph1 = g.PH;
    } else {
      plane0 = item / bands;
      np = 1;
      ph0 = (item - plane0 * bands) * R;
      ph1 = min(g.PH, ph0 + R);
    }
    const int h_lo = bands == 1 ? 0 : pool_band_lo(g, ph0), h_hi = bands == 1 ? g.H : pool_band_hi(g, ph1);
    const int cnt = bands == 1 ? np * HW : (h_hi - h_lo) * g.W;          // <= kPoolLdsBytes / sizeof(T): the plan's
    const T* const src = bottom + (size_t)plane0 * HW + (size_t)h_lo * g.W;
    const int off = (int)((reinterpret_cast<uintptr_t>(src) / sizeof(T)) % VW);   // elements past a 16-byte boundary
    T* const dst = lds + off;
    const int lead = min(cnt, (VW - off) % VW), nvec = (cnt - lead) / VW;
    if (tid < lead) dst[tid] = src[tid];
    for (int i = tid; i < nvec; i += kPoolThreads)
      *reinterpret_cast<V*>(dst + lead + i * VW) = *reinterpret_cast<const V*>(src + lead + i * VW);
    for (int i = lead + nvec * VW + tid; i < cnt; i += kPoolThreads) dst[i] = src[i];
    __syncthreads();
    const int rows = ph1 - ph0, per = rows * g.PW, nout = np * per;
    for (int o = tid; o < nout; o += kPoolThreads) {
      const int pl = o / per, r = o - pl * per, pr = r / g.PW, ph = ph0 + pr, pw = r - pr * g.PW;
      int idx = -1;
      const T v = pool_window<T, METHOD>(g, dst + pl * HW - h_lo * g.W, ph, pw, &idx);
      pool_store(top, mask, top_mask, (size_t)(plane0 + pl) * PHW + (size_t)ph * g.PW + pw, v, idx);
    }
    __syncthreads();
  }
}

// kPoolDirect: a thread per output
template <typename T, int METHOD>
__global__ __launch_bounds__(kPoolThreads) void pool_forward_direct_kernel(PoolGeom g, int ntop,
                                                                          const T* __restrict__ bottom,
                                                                          T* __restrict__ top, int* __restrict__ mask,
                                                                          T* __restrict__ top_mask) {
  const int PHW = g.PH * g.PW;
  const long long stride = (long long)gridDim.x * kPoolThreads;
  for (long long i = (long long)blockIdx.x * kPoolThreads + threadIdx.x; i < ntop; i += stride) {
    const int o = (int)i, pl = o / PHW, r = o - pl * PHW, ph = r / g.PW, pw = r - ph * g.PW;
    int idx = -1;
    const T v = pool_window<T, METHOD>(g, bottom + (size_t)pl * g.H * g.W, ph, pw, &idx);
    pool_store(top, mask, top_mask, (size_t)o, v, idx);
  }
}

// The index a top_mask entry stands for; -1 where it is none of the plane's.
template <typename T>
__device__ __forceinline__ int pool_top_mask_index(T m, int HW) {
  return (m >= T(0) && m < T(HW)) ? (int)m : -1;
}

// bottom_diff of element e: +0, then the contributions of the windows that contain it, in ascending (ph, pw)
template <typename T, int METHOD>
__device__ __forceinline__ T pool_gather(const PoolGeom& g, int e, const T* __restrict__ top_diff,
                                         const int* __restrict__ mask, const T* __restrict__ top_mask) {
  const int HW = g.H * g.W, pl = e / HW, r = e - pl * HW, h = r / g.W, w = r - h * g.W;
  const int hp = h + g.pad_h, wp = w + g.pad_w;
  const int ph_lo = hp < g.kh ? 0 : (hp - g.kh) / g.sh + 1, ph_hi = min(hp / g.sh + 1, g.PH);
  const int pw_lo = wp < g.kw ? 0 : (wp - g.kw) / g.sw + 1, pw_hi = min(wp / g.sw + 1, g.PW);
  const size_t base = (size_t)pl * g.PH * g.PW;
  T acc = T(0);
  for (int ph = ph_lo; ph < ph_hi; ++ph)
    for (int pw = pw_lo; pw < pw_hi; ++pw) {
      const size_t i = base + (size_t)ph * g.PW + pw;
      if (METHOD == MMS_POOL_MAX) {
        const int at = mask ? mask[i] : pool_top_mask_index(top_mask[i], HW);
        if (at == r) acc += top_diff[i];
      } else {
        const int hs = ph * g.sh - g.pad_h, ws = pw * g.sw - g.pad_w;
        const int he = min(hs + g.kh, g.H + g.pad_h), we = min(ws + g.kw, g.W + g.pad_w);
        const T q = top_diff[i] / T((he - hs) * (we - ws));
        acc += q;
      }
    }
  return acc;
}

template <typename T, int METHOD, bool VEC>
__global__ __launch_bounds__(kPoolThreads) void pool_backward_kernel(PoolGeom g, int count,
                                                                    const T* __restrict__ top_diff,
                                                                    const int* __restrict__ mask,
                                                                    const T* __restrict__ top_mask,
                                                                    T* __restrict__ bottom_diff) {
  typedef bn_vec<T> V;
  constexpr int VW = VEC ? 16 / sizeof(T) : 1;
  const long long ngroups = ((long long)count + VW - 1) / VW, stride = (long long)gridDim.x * kPoolThreads;
  for (long long k = (long long)blockIdx.x * kPoolThreads + threadIdx.x; k < ngroups; k += stride) {
    const long long e0 = k * VW;
    if (VEC && e0 + VW <= count) {
      V v;
#pragma unroll
      for (int j = 0; j < VW; ++j) v[j] = pool_gather<T, METHOD>(g, (int)e0 + j, top_diff, mask, top_mask);
      *reinterpret_cast<V*>(bottom_diff + e0) = v;
    } else {
      for (int j = 0; j < VW && e0 + j < count; ++j)
        bottom_diff[e0 + j] = pool_gather<T, METHOD>(g, (int)(e0 + j), top_diff, mask, top_mask);
    }
  }
}

template <typename T>
__device__ __forceinline__ T pool_tanh(T x) { return bn_tanh(x); }

// tanh_layer.cpp:29-32: three roundings
template <typename T>
__device__ __forceinline__ T pool_tanh_diff(T y, T dy) {
  const T t = y * y;
  const T u = T(1) - t;
  return dy * u;
}

// BWD: out = pool_tanh_diff(a, b); otherwise out = pool_tanh(a) and b is not read
template <typename T, bool BWD, bool VEC>
__global__ __launch_bounds__(kPoolThreads) void pool_tanh_kernel(long long count, const T* a, const T* b, T* out) {
  typedef bn_vec<T> V;
  constexpr int VW = VEC ? 16 / sizeof(T) : 1;
  const long long ngroups = (count + VW - 1) / VW, stride = (long long)gridDim.x * kPoolThreads;
  for (long long k = (long long)blockIdx.x * kPoolThreads + threadIdx.x; k < ngroups; k += stride) {
    const long long e0 = k * VW;
    if (VEC && e0 + VW <= count) {
      const V av = *reinterpret_cast<const V*>(a + e0);
      V bv = av, ov;
      if (BWD) bv = *reinterpret_cast<const V*>(b + e0);
#pragma unroll
      for (int j = 0; j < VW; ++j) ov[j] = BWD ? pool_tanh_diff<T>(av[j], bv[j]) : pool_tanh<T>(av[j]);
      *reinterpret_cast<V*>(out + e0) = ov;
    } else {
      for (int j = 0; j < VW && e0 + j < count; ++j)
        out[e0 + j] = BWD ? pool_tanh_diff<T>(a[e0 + j], b[e0 + j]) : pool_tanh<T>(a[e0 + j]);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
// The overlap refusals are csrc/host_args.h's: arrays_overlap, no two arrays of a call share a byte.

// what forward and backward judge alike; *done: MMS_OK with nothing to launch
int pool_check(const mms_pool_shape* shape, PoolGeom* g, long long* nbottom, long long* ntop, bool* done) {
  *done = false;
  const int rc = pool_geometry(shape, g);
  if (rc != MMS_OK) return rc;
  if (g->N == 0) {
    *done = true;
    return MMS_OK;
  }
  return pool_counts(g, nbottom, ntop) ? MMS_OK : MMS_ERR_INVALID_ARG;
}

template <typename T>
int pool_forward(const mms_pool_shape* shape, const T* bottom, T* top, int* mask, T* top_mask, hipStream_t s) {
  PoolGeom g;
  long long nb = 0, nt = 0;
  bool done = false;
  const int rc = pool_check(shape, &g, &nb, &nt, &done);
  if (rc != MMS_OK || done) return rc;
  if (!bottom || !top) return MMS_ERR_INVALID_ARG;
  const ByteSpan spans[] = {byte_span(bottom, (size_t)nb * sizeof(T)), byte_span(top, (size_t)nt * sizeof(T)),
                            byte_span(mask, (size_t)nt * sizeof(int)), byte_span(top_mask, (size_t)nt * sizeof(T))};
  if (arrays_overlap(spans, 4, false)) return MMS_ERR_INVALID_ARG;
  if (g.method == MMS_POOL_AVE) mask = nullptr, top_mask = nullptr;          // ignored
  const PoolPlan p = pool_forward_plan(g, (int)sizeof(T));
  const dim3 grid((unsigned)p.blocks), block(kPoolThreads);
  if (p.route == kPoolDirect) {
    if (g.method == MMS_POOL_MAX)
      hipLaunchKernelGGL((pool_forward_direct_kernel<T, MMS_POOL_MAX>), grid, block, 0, s, g, (int)nt, bottom, top, mask,
                         top_mask);
    else
      hipLaunchKernelGGL((pool_forward_direct_kernel<T, MMS_POOL_AVE>), grid, block, 0, s, g, (int)nt, bottom, top, mask,
                         top_mask);
  } else {
    if (g.method == MMS_POOL_MAX)
      hipLaunchKernelGGL((pool_forward_staged_kernel<T, MMS_POOL_MAX>), grid, block, p.lds_bytes, s, g, p.P, p.R, p.bands,
                         (int)p.items, bottom, top, mask, top_mask);
    else
      hipLaunchKernelGGL((pool_forward_staged_kernel<T, MMS_POOL_AVE>), grid, block, p.lds_bytes, s, g, p.P, p.R, p.bands,
                         (int)p.items, bottom, top, mask, top_mask);
  }
  return launch_status();
}

template <typename T>
int pool_backward(const mms_pool_shape* shape, const T* top_diff, const int* mask, const T* top_mask, T* bottom_diff,
                  hipStream_t s) {
  PoolGeom g;
  long long nb = 0, nt = 0;
  bool done = false;
  const int rc = pool_check(shape, &g, &nb, &nt, &done);
  if (rc != MMS_OK || done) return rc;
  if (!top_diff || !bottom_diff) return MMS_ERR_INVALID_ARG;
  if (g.method == MMS_POOL_MAX && !mask && !top_mask) return MMS_ERR_INVALID_ARG;
  const ByteSpan spans[] = {byte_span(top_diff, (size_t)nt * sizeof(T)), byte_span(mask, (size_t)nt * sizeof(int)),
                            byte_span(top_mask, (size_t)nt * sizeof(T)), byte_span(bottom_diff, (size_t)nb * sizeof(T))};
  if (arrays_overlap(spans, 4, false)) return MMS_ERR_INVALID_ARG;
  const bool vec = aligned16(bottom_diff);
  const int VW = vec ? 16 / (int)sizeof(T) : 1;
  const dim3 grid((unsigned)pool_sweep_blocks((nb + VW - 1) / VW)), block(kPoolThreads);
  with_bool(vec, [&](auto B) {
    constexpr bool VEC = decltype(B)::value;
    if (g.method == MMS_POOL_MAX)
      hipLaunchKernelGGL((pool_backward_kernel<T, MMS_POOL_MAX, VEC>), grid, block, 0, s, g, (int)nb, top_diff, mask,
                         top_mask, bottom_diff);
    else
      hipLaunchKernelGGL((pool_backward_kernel<T, MMS_POOL_AVE, VEC>), grid, block, 0, s, g, (int)nb, top_diff, mask,
                         top_mask, bottom_diff);
  });
  return launch_status();
}

// BWD: (a, b, out) = (top, top_diff, bottom_diff); otherwise (a, out) = (bottom, top) and b is NULL
template <typename T, bool BWD>
int pool_tanh_call(long long count, const T* a, const T* b, T* out, hipStream_t s) {
  if (count < 0) return MMS_ERR_INVALID_ARG;
  if (count == 0) return MMS_OK;
  if (!a || !out || (BWD && !b)) return MMS_ERR_INVALID_ARG;
  if ((unsigned long long)count > (unsigned long long)(SIZE_MAX / sizeof(T))) return MMS_ERR_INVALID_ARG;
  const size_t bytes = (size_t)count * sizeof(T);
  // the in-place pair is (b, out) in the backward and (a, out) in the forward: first and last of the list
  const ByteSpan fwd[] = {byte_span(a, bytes), byte_span(out, bytes)};
  const ByteSpan bwd[] = {byte_span(b, bytes), byte_span(a, bytes), byte_span(out, bytes)};
  if (BWD ? arrays_overlap(bwd, 3, true) : arrays_overlap(fwd, 2, true)) return MMS_ERR_INVALID_ARG;
  const bool vec = aligned16(a) && aligned16(out) && (!BWD || aligned16(b));
  const int VW = vec ? 16 / (int)sizeof(T) : 1;
  const dim3 grid((unsigned)pool_sweep_blocks((count + VW - 1) / VW)), block(kPoolThreads);
  with_bool(vec, [&](auto B) {
    hipLaunchKernelGGL((pool_tanh_kernel<T, BWD, decltype(B)::value>), grid, block, 0, s, count, a, b, out);
  });
  return launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_pool_output_dims(const mms_pool_shape* shape, int* PH, int* PW) {
  if (!PH || !PW) return MMS_ERR_INVALID_ARG;
  PoolGeom g;
  const int rc = pool_geometry(shape, &g);
  if (rc != MMS_OK) return rc;
  *PH = g.PH;
  *PW = g.PW;
  return MMS_OK;
}

int mms_pool_forward_f32(const mms_pool_shape* shape, const float* bottom, float* top, int* mask, float* top_mask,
                         void* stream) {
  return pool_forward<float>(shape, bottom, top, mask, top_mask, as_stream(stream));
}

int mms_pool_forward_f64(const mms_pool_shape* shape, const double* bottom, double* top, int* mask, double* top_mask,
                         void* stream) {
  return pool_forward<double>(shape, bottom, top, mask, top_mask, as_stream(stream));
}

int mms_pool_backward_f32(const mms_pool_shape* shape, const float* top_diff, const int* mask, const float* top_mask,
                          float* bottom_diff, void* stream) {
  return pool_backward<float>(shape, top_diff, mask, top_mask, bottom_diff, as_stream(stream));
}

int mms_pool_backward_f64(const mms_pool_shape* shape, const double* top_diff, const int* mask, const double* top_mask,
                          double* bottom_diff, void* stream) {
  return pool_backward<double>(shape, top_diff, mask, top_mask, bottom_diff, as_stream(stream));
}

int mms_tanh_forward_f32(long long count, const float* bottom, float* top, void* stream) {
  return pool_tanh_call<float, false>(count, bottom, nullptr, top, as_stream(stream));
}

int mms_tanh_forward_f64(long long count, const double* bottom, double* top, void* stream) {
  return pool_tanh_call<double, false>(count, bottom, nullptr, top, as_stream(stream));
}

int mms_tanh_backward_f32(long long count, const float* top, const float* top_diff, float* bottom_diff, void* stream) {
  return pool_tanh_call<float, true>(count, top, top_diff, bottom_diff, as_stream(stream));
}

int mms_tanh_backward_f64(long long count, const double* top, const double* top_diff, double* bottom_diff,
                          void* stream) {
  return pool_tanh_call<double, true>(count, top, top_diff, bottom_diff, as_stream(stream));
}

}  // extern "C"
