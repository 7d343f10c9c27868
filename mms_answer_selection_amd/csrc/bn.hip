// csrc/bn.hip -- BN, the fork's batch normalisation over the (N, H*W) elements of each channel of an (N, C, H, W) blob,
// and its extern "C" entry points (include/mms.h: mms_bn_*).  The arithmetic restated here is
// src/caffe/layers/bn_layer.cpp:131-256 (forward) and :262-383 (backward, the `#if 1` branch); the reference's GPU
// path (bn_layer.cu) is the same sequence of BLAS calls.  With S = H*W, per channel c:
//
//   TRAIN   mean = (1/N) (1/S) sum x        ex2 = (1/N) (1/S) sum x*x        var = ex2 - mean*mean
//           running = (1 - bn_memory) * batch + bn_memory * running          (mean and var; two products, one add)
//   TEST    mean = running_mean, var = running_var                            (both left alone)
//   both    std = sqrt(var + 1e-9);  xn = (x + (-mean)) / std;  top = xn * scale + shift
//   backward  shift_diff = sum dy;  scale_diff = sum xn*dy;  g = dy*scale;  b = sum g;  a = sum xn*g
//             dx = (g + (-1/(N S)) * (xn*a + b)) / std
//
// The reference's sums are BLAS gemv's, so their order is the library's: this is the "BLAS-ordered, 1e-5" class.  The
// order here is fixed (below), there are no atomics, and every run gives the same words.  xn is never stored: the
// backward recomputes it from x, save_mean and save_std with the forward's two operations, hence the forward's bits.
//
// A channel is N runs of S contiguous elements at stride C*S.  Its N*S elements, in (n, s) order, are cut into GROUPS
// of 16 bytes (4 floats, 2 doubles); thread t of a workgroup of T threads that owns groups [g0, g1) takes g0 + t,
// g0 + t + T, ... in turn and adds each group's elements in ascending order into ONE accumulator per sum.  The T
// accumulators are then combined per wave (xor butterfly) and the waves' totals in ascending order.  A group is one
// 16-byte access where S is a multiple of the group and the arrays are 16-byte aligned, and one access per element
// otherwise: the same elements go to the same thread in the same order, so both forms give the same words.
//
// Two routes (bn_route, the one place that decides):
//   small  at most kBnSmallGroups groups per channel: one launch per pass, one workgroup of 1024 per channel, which
//          sums its channel and then walks it again (from L2) to normalise it.
//   large  the channel is cut into at most kBnMaxChunks chunks of whole groups; launch 1, a grid of (channel, chunk)
//          workgroups of 256, writes each chunk's sums to the workspace; launch 2, the same grid, has every workgroup
//          add its channel's chunk sums in ASCENDING CHUNK ORDER (first chunk + second + ...) -- all of them get the same
//          bits -- and then normalise its chunk.  Chunk 0 writes the per-channel results.
// TEST-phase forward is launch 2 alone on either route.
#include <limits.h>

#include "bn_common.h"        // the routes' sizes, bn_block_sum, bn_fold: shared with csrc/bn_pool.hip
#include "mms_internal.h"

namespace mms {
namespace {

struct BnRoute {
  bool small;
  int chunks;                 // per channel
  unsigned groups_per_chunk;
};

// The one routing decision.  T: float or double; N >= 1, S >= 1, N * S <= INT_MAX.
template <typename T>
BnRoute bn_route(int N, int S) {
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned total = (unsigned)N * (unsigned)S;
  const unsigned groups = (total + V - 1) / V;
  if (groups <= kBnSmallGroups) return {true, 1, groups};
  unsigned gpc = (groups + kBnMaxChunks - 1) / kBnMaxChunks;
  if (gpc < kBnChunkGroups) gpc = kBnChunkGroups;
  return {false, (int)((groups + gpc - 1) / gpc), gpc};
}

// N < 0, C <= 0, S <= 0, or more elements than the reference's int index reaches
bool bn_bad_shape(int N, int C, int S) {
  if (N < 0 || C <= 0 || S <= 0) return true;
  const long long nc = (long long)N * C;
  return nc > INT_MAX || nc * S > INT_MAX;
}

template <typename T>
size_t bn_workspace_bytes(int N, int C, int S) {
  if (bn_bad_shape(N, C, S) || N == 0) return 0;
  const BnRoute r = bn_route<T>(N, S);
  return r.small ? 0 : (size_t)C * r.chunks * kBnSlots * sizeof(T);
}

struct BnGeom {
  unsigned S;        // elements per run
  unsigned total;    // N * S, the elements of one channel
  size_t stride;     // C * S, from one run of a channel to the next
};

struct BnPos {       // a group's first element: index in the channel, run, offset in the run
  unsigned i, n, s;
};

// The group at p of each of NIN arrays (pointers to the channel's first run).  Elements past the channel's end read 0.
template <typename T, bool VEC, int NIN>
__device__ __forceinline__ void bn_load(const T* const (&in)[NIN], const BnGeom& geo, const BnPos& p,
                                        T (&v)[NIN][16 / sizeof(T)]) {
  constexpr int V = 16 / sizeof(T);
  const size_t off0 = (size_t)p.n * geo.stride + p.s;
  if constexpr (VEC) {
#pragma unroll
    for (int a = 0; a < NIN; ++a) {
      const bn_vec<T> t = *reinterpret_cast<const bn_vec<T>*>(in[a] + off0);
#pragma unroll
      for (int e = 0; e < V; ++e) v[a][e] = t[e];
    }
  } else {
    unsigned n = p.n, s = p.s;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool ok = p.i + e < geo.total;
      const size_t off = ok ? (size_t)n * geo.stride + s : off0;     // off0 is in range: every load is issued
#pragma unroll
      for (int a = 0; a < NIN; ++a) {
        const T t = in[a][off];
        v[a][e] = ok ? t : T(0);
      }
      if (++s == geo.S) { s = 0; ++n; }
    }
  }
}

template <typename T, bool VEC>
__device__ __forceinline__ void bn_store(T* out, const BnGeom& geo, const BnPos& p, const T (&v)[16 / sizeof(T)]) {
  constexpr int V = 16 / sizeof(T);
  if constexpr (VEC) {
    bn_vec<T> t;
#pragma unroll
    for (int e = 0; e < V; ++e) t[e] = v[e];
    *reinterpret_cast<bn_vec<T>*>(out + (size_t)p.n * geo.stride + p.s) = t;
  } else {
    unsigned n = p.n, s = p.s;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (p.i + e < geo.total) out[(size_t)n * geo.stride + s] = v[e];
      if (++s == geo.S) { s = 0; ++n; }
    }
  }
}

// Thread t visits groups g0 + t, g0 + t + THREADS, ... below g1 in turn: f(position, values[NIN][V]) per group, the
// loads of kBnBatch groups issued before the first is used.  One division per thread; the walk itself only adds.
template <typename T, bool VEC, int THREADS, int NIN, class F>
__device__ __forceinline__ void bn_sweep(const BnGeom& geo, unsigned g0, unsigned g1, const T* const (&in)[NIN],
                                         F&& f) {
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned first = g0 + threadIdx.x;
  if (first >= g1) return;
  unsigned cnt = (g1 - first + THREADS - 1) / THREADS;
  constexpr unsigned step = THREADS * V;
  const unsigned step_n = step / geo.S, step_s = step - step_n * geo.S;
  BnPos p;
  p.i = first * V;
  p.n = p.i / geo.S;
  p.s = p.i - p.n * geo.S;
  auto advance = [&]() {
    p.i += step;
    p.n += step_n;
    p.s += step_s;
    if (p.s >= geo.S) { p.s -= geo.S; ++p.n; }
  };
  while (cnt >= kBnBatch) {
    BnPos at[kBnBatch];
    T v[kBnBatch][NIN][V];
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) {
      at[u] = p;
      bn_load<T, VEC, NIN>(in, geo, p, v[u]);
      advance();
    }
#pragma unroll
    for (int u = 0; u < kBnBatch; ++u) f(at[u], v[u]);
    cnt -= kBnBatch;
  }
  while (cnt) {
    T v[NIN][V];
    bn_load<T, VEC, NIN>(in, geo, p, v);
    f(p, v);
    advance();
    --cnt;
  }
}

// sum x and sum x*x over groups [g0, g1) of channel c, reduced over the workgroup
template <typename T, bool VEC, int THREADS>
__device__ __forceinline__ void bn_forward_sums(const T* __restrict__ x, int c, const BnGeom& geo, unsigned g0,
                                                unsigned g1, T (&acc)[2], T* red) {
  constexpr int V = 16 / sizeof(T);
  const T* const in[1] = {x + (size_t)c * geo.S};
  acc[0] = acc[1] = T(0);
  bn_sweep<T, VEC, THREADS, 1>(geo, g0, g1, in, [&](const BnPos&, const T(&v)[1][V]) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      acc[0] += v[0][e];
      acc[1] += v[0][e] * v[0][e];
    }
  });
  bn_block_sum<THREADS, 2>(acc, red);
}

// sum dy, sum xn*dy, sum g, sum xn*g (g = dy*scale) over groups [g0, g1) of channel c, reduced over the workgroup
template <typename T, bool VEC, int THREADS>
__device__ __forceinline__ void bn_backward_sums(const T* __restrict__ x, const T* __restrict__ dy, int c,
                                                 const BnGeom& geo, unsigned g0, unsigned g1, T nmean, T std, T sc,
                                                 T (&acc)[4], T* red) {
  constexpr int V = 16 / sizeof(T);
  const T* const in[2] = {x + (size_t)c * geo.S, dy + (size_t)c * geo.S};
  acc[0] = acc[1] = acc[2] = acc[3] = T(0);
  bn_sweep<T, VEC, THREADS, 2>(geo, g0, g1, in, [&](const BnPos& p, const T(&v)[2][V]) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (VEC || p.i + e < geo.total) {          // past the end x reads 0, and (0 - mean) / std is not 0
        const T xn = (v[0][e] + nmean) / std;
        const T d = v[1][e];
        const T g = d * sc;
        acc[0] += d;
        acc[1] += xn * d;
        acc[2] += g;
        acc[3] += xn * g;
      }
    }
  });
  bn_block_sum<THREADS, 4>(acc, red);
}

// Chunk k's share of the channel's groups.
__device__ __forceinline__ void bn_chunk(unsigned groups, unsigned gpc, unsigned k, unsigned* g0, unsigned* g1) {
  *g0 = k * gpc;                                  // k < chunks: k * gpc < groups
  *g1 = groups - *g0 < gpc ? groups : *g0 + gpc;
}

// Large route, launch 1.  BWD false: slots 0, 1 = sum x, sum x*x.  BWD true: slots 0..3 = the four backward sums.
template <typename T, bool VEC, bool BWD>
__global__ __launch_bounds__(kBnThreads) void bn_partial_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                const T* __restrict__ scale,
                                                                const T* __restrict__ save_mean,
                                                                const T* __restrict__ save_std, T* __restrict__ ws,
                                                                int C, unsigned S, unsigned total, unsigned gpc) {
  constexpr unsigned V = 16 / sizeof(T);
  constexpr int NQ = BWD ? 4 : 2;
  __shared__ T red[NQ * kBnThreads / kWave];
  const int c = blockIdx.x;
  const BnGeom geo = {S, total, (size_t)C * S};
  unsigned g0, g1;
  bn_chunk((total + V - 1) / V, gpc, blockIdx.y, &g0, &g1);
  T acc[NQ];
  if constexpr (BWD) {
    bn_backward_sums<T, VEC, kBnThreads>(x, dy, c, geo, g0, g1, -save_mean[c], save_std[c], scale[c], acc, red);
  } else {
    bn_forward_sums<T, VEC, kBnThreads>(x, c, geo, g0, g1, acc, red);
  }
  if (threadIdx.x == 0) {
    T* o = ws + ((size_t)c * gridDim.y + blockIdx.y) * kBnSlots;
#pragma unroll
    for (int q = 0; q < NQ; ++q) o[q] = acc[q];
  }
}

// Forward: the only launch of the small route (SMALL: grid (C, 1), 1024 threads, the workgroup sums its own channel)
// and launch 2 of the large route (grid (C, chunks), 256 threads, the sums come from the workspace).  phase 1 (TEST)
// takes mean and var from the running blobs and needs no sums on either route.
template <typename T, bool VEC, bool SMALL>
__global__ __launch_bounds__(SMALL ? kBnSmallThreads : kBnThreads) void bn_forward_kernel(
    const T* __restrict__ x, const T* __restrict__ scale, const T* __restrict__ shift, T* running_mean,
    T* running_var, T* __restrict__ top, T* save_mean, T* save_std, const T* __restrict__ ws, int C, unsigned S,
    unsigned total, unsigned gpc, int chunks, int phase, T bn_memory, T inv_S, T inv_N) {
  constexpr unsigned V = 16 / sizeof(T);
  constexpr int THREADS = SMALL ? kBnSmallThreads : kBnThreads;
  __shared__ T red[2 * THREADS / kWave];
  const int c = blockIdx.x;
  const BnGeom geo = {S, total, (size_t)C * S};
  unsigned g0, g1;
  bn_chunk((total + V - 1) / V, gpc, blockIdx.y, &g0, &g1);
  const bool writer = blockIdx.y == 0 && threadIdx.x == 0;
  T mean, var;
  if (phase == 0) {
    T tot[2];
    if constexpr (SMALL) bn_forward_sums<T, VEC, THREADS>(x, c, geo, g0, g1, tot, red);
    else bn_fold<2>(ws, c, chunks, tot);
    mean = inv_N * (inv_S * tot[0]);
    var = inv_N * (inv_S * tot[1]) - mean * mean;        // not clamped: the reference does not either
    if (writer) {
      const T keep = bn_memory, take = T(1) - bn_memory;
      running_mean[c] = take * mean + keep * running_mean[c];
      running_var[c] = take * var + keep * running_var[c];
    }
  } else {
    mean = running_mean[c];
    var = running_var[c];
  }
  const T std = bn_sqrt(var + T(1e-9));
  if (writer) {
    save_mean[c] = mean;
    save_std[c] = std;
  }
  const T nmean = -mean, sc = scale[c], sh = shift[c];
  const T* const in[1] = {x + (size_t)c * S};
  T* out = top + (size_t)c * S;
  bn_sweep<T, VEC, THREADS, 1>(geo, g0, g1, in, [&](const BnPos& p, const T(&v)[1][V]) {
    T o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = (v[0][e] + nmean) / std * sc + sh;
    bn_store<T, VEC>(out, geo, p, o);
  });
}

// Backward, the same two uses.  scale_diff, shift_diff and dx may each be NULL; with dx NULL the large route launches
// one workgroup per channel (gridDim.y == 1), which only folds.
template <typename T, bool VEC, bool SMALL>
__global__ __launch_bounds__(SMALL ? kBnSmallThreads : kBnThreads) void bn_backward_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ scale, const T* __restrict__ save_mean,
    const T* __restrict__ save_std, T* __restrict__ dx, T* __restrict__ scale_diff, T* __restrict__ shift_diff,
    const T* __restrict__ ws, int C, unsigned S, unsigned total, unsigned gpc, int chunks, T minus_inv_count) {
  constexpr unsigned V = 16 / sizeof(T);
  constexpr int THREADS = SMALL ? kBnSmallThreads : kBnThreads;
  __shared__ T red[4 * THREADS / kWave];
  const int c = blockIdx.x;
  const BnGeom geo = {S, total, (size_t)C * S};
  unsigned g0, g1;
  bn_chunk((total + V - 1) / V, gpc, blockIdx.y, &g0, &g1);
  const T nmean = -save_mean[c], std = save_std[c], sc = scale[c];
  T tot[4];
  if constexpr (SMALL) bn_backward_sums<T, VEC, THREADS>(x, dy, c, geo, g0, g1, nmean, std, sc, tot, red);
  else bn_fold<4>(ws, c, chunks, tot);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    if (shift_diff) shift_diff[c] = tot[0];
    if (scale_diff) scale_diff[c] = tot[1];
  }
  if (!dx) return;
  const T b = tot[2], a = tot[3];
  const T* const in[2] = {x + (size_t)c * S, dy + (size_t)c * S};
  T* out = dx + (size_t)c * S;
  bn_sweep<T, VEC, THREADS, 2>(geo, g0, g1, in, [&](const BnPos& p, const T(&v)[2][V]) {
    T o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const T xn = (v[0][e] + nmean) / std;
      const T g = v[1][e] * sc;
      o[e] = (g + minus_inv_count * (xn * a + b)) / std;
    }
    bn_store<T, VEC>(out, geo, p, o);
  });
}

// 16-byte groups are single accesses when every run starts on a 16-byte boundary in every array the pass touches
template <typename T>
bool bn_vector_ok(int S, const void* a, const void* b, const void* c) {
  return S % (int)(16 / sizeof(T)) == 0 && aligned16(a) && aligned16(b) && aligned16(c);
}

template <typename T>
int bn_forward(int phase, int N, int C, int S, T bn_memory, const T* x, const T* scale, const T* shift,
               T* running_mean, T* running_var, T* top, T* save_mean, T* save_std, void* workspace,
               size_t workspace_bytes, hipStream_t s) {
  if (bn_bad_shape(N, C, S) || (phase != 0 && phase != 1)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !scale || !shift || !running_mean || !running_var || !top || !save_mean || !save_std || top == x)
    return MMS_ERR_INVALID_ARG;
  const BnRoute r = bn_route<T>(N, S);
  const size_t need = bn_workspace_bytes<T>(N, C, S);
  if (need && phase == 0 && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  T* ws = static_cast<T*>(workspace);
  const unsigned total = (unsigned)N * (unsigned)S;
  const T inv_S = T(1. / S), inv_N = T(1. / N);
  const dim3 grid((unsigned)C, (unsigned)r.chunks);
  int rc = MMS_OK;
  with_bool(bn_vector_ok<T>(S, x, top, nullptr), [&](auto VEC) {
    constexpr bool V = decltype(VEC)::value;
    if (r.small) {
      hipLaunchKernelGGL((bn_forward_kernel<T, V, true>), grid, dim3(kBnSmallThreads), 0, s, x, scale, shift,
                         running_mean, running_var, top, save_mean, save_std, (const T*)nullptr, C, (unsigned)S, total,
                         r.groups_per_chunk, 1, phase, bn_memory, inv_S, inv_N);
      return;
    }
    if (phase == 0) {
      hipLaunchKernelGGL((bn_partial_kernel<T, V, false>), grid, dim3(kBnThreads), 0, s, x, (const T*)nullptr,
                         (const T*)nullptr, (const T*)nullptr, (const T*)nullptr, ws, C, (unsigned)S, total,
                         r.groups_per_chunk);
      if ((rc = launch_status()) != MMS_OK) return;
    }
    hipLaunchKernelGGL((bn_forward_kernel<T, V, false>), grid, dim3(kBnThreads), 0, s, x, scale, shift, running_mean,
                       running_var, top, save_mean, save_std, (const T*)ws, C, (unsigned)S, total, r.groups_per_chunk,
                       r.chunks, phase, bn_memory, inv_S, inv_N);
  });
  return rc != MMS_OK ? rc : launch_status();
}

template <typename T>
int bn_backward(int N, int C, int S, const T* x, const T* top_diff, const T* scale, const T* save_mean,
                const T* save_std, T* bottom_diff, T* scale_diff, T* shift_diff, void* workspace,
                size_t workspace_bytes, hipStream_t s) {
  if (bn_bad_shape(N, C, S)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top_diff || !scale || !save_mean || !save_std || (!bottom_diff && !scale_diff && !shift_diff))
    return MMS_ERR_INVALID_ARG;
  const BnRoute r = bn_route<T>(N, S);
  const size_t need = bn_workspace_bytes<T>(N, C, S);
  if (need && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  T* ws = static_cast<T*>(workspace);
  const unsigned total = (unsigned)N * (unsigned)S;
  const T minus_inv_count = T(-1. / total);
  const dim3 grid((unsigned)C, (unsigned)r.chunks);
  int rc = MMS_OK;
  with_bool(bn_vector_ok<T>(S, x, top_diff, bottom_diff), [&](auto VEC) {
    constexpr bool V = decltype(VEC)::value;
    if (r.small) {
      hipLaunchKernelGGL((bn_backward_kernel<T, V, true>), grid, dim3(kBnSmallThreads), 0, s, x, top_diff, scale,
                         save_mean, save_std, bottom_diff, scale_diff, shift_diff, (const T*)nullptr, C, (unsigned)S,
                         total, r.groups_per_chunk, 1, minus_inv_count);
      return;
    }
    hipLaunchKernelGGL((bn_partial_kernel<T, V, true>), grid, dim3(kBnThreads), 0, s, x, top_diff, scale, save_mean,
                       save_std, ws, C, (unsigned)S, total, r.groups_per_chunk);
    if ((rc = launch_status()) != MMS_OK) return;
    hipLaunchKernelGGL((bn_backward_kernel<T, V, false>), bottom_diff ? grid : dim3((unsigned)C), dim3(kBnThreads), 0,
                       s, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff, (const T*)ws, C,
                       (unsigned)S, total, r.groups_per_chunk, r.chunks, minus_inv_count);
  });
  return rc != MMS_OK ? rc : launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

size_t mms_bn_workspace_bytes(int N, int C, int S) { return bn_workspace_bytes<float>(N, C, S); }
size_t mms_bn_workspace_bytes_f64(int N, int C, int S) { return bn_workspace_bytes<double>(N, C, S); }

int mms_bn_forward_f32(int phase, int N, int C, int S, float bn_memory, const float* x, const float* scale,
                       const float* shift, float* running_mean, float* running_var, float* top, float* save_mean,
                       float* save_std, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_forward<float>(phase, N, C, S, bn_memory, x, scale, shift, running_mean, running_var, top, save_mean,
                           save_std, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_backward_f32(int N, int C, int S, const float* x, const float* top_diff, const float* scale,
                        const float* save_mean, const float* save_std, float* bottom_diff, float* scale_diff,
                        float* shift_diff, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_backward<float>(N, C, S, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff,
                            workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_forward_f64(int phase, int N, int C, int S, double bn_memory, const double* x, const double* scale,
                       const double* shift, double* running_mean, double* running_var, double* top, double* save_mean,
                       double* save_std, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_forward<double>(phase, N, C, S, bn_memory, x, scale, shift, running_mean, running_var, top, save_mean,
                            save_std, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_backward_f64(int N, int C, int S, const double* x, const double* top_diff, const double* scale,
                        const double* save_mean, const double* save_std, double* bottom_diff, double* scale_diff,
                        double* shift_diff, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_backward<double>(N, C, S, x, top_diff, scale, save_mean, save_std, bottom_diff, scale_diff, shift_diff,
                             workspace, workspace_bytes, as_stream(stream));
}

}  // extern "C"
