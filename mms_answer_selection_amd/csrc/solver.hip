// csrc/solver.hip -- the solver update (include/mms_solver.h: mms_solver_*): the reference's SGDSolver::ApplyUpdate
// for SGD and AdaDelta over ALL learnable blobs in one launch, with Net::ClearParamDiffs folded in on request.
// The reference's GPU path takes three launches per blob (regularize axpy, the update kernel, Blob::Update's axpy),
// about 60 for network_v4's 20 blobs, whose sizes run from 2 elements to the word-vector table.
//
// The work is elementwise and streaming: per element 16 bytes in (w, g, h, h2) and 16 bytes out, no reuse.  So:
//
//   work item   kSolverChunk = MMS_SOLVER_CHUNK = 2048 elements of one blob, one workgroup of 256 threads per item.
//               Thread t takes elements 4t .. 4t+3 and 4t+1024 .. 4t+1027 of the chunk: all its loads (8 x 16 bytes in
//               float, 16 x 16 bytes in double) are issued before the first result is needed, 32 KB (64 KB) in flight
//               per workgroup, so two or three resident workgroups cover a CU's HBM latency.  The word table alone gives
//               over a thousand items; a larger chunk would leave CUs idle on it, a smaller one buys nothing for the
//               19 small blobs, which are one item each whatever the chunk.
//   blob table  by value in the kernel arguments (SolverTable, 1.8 KB in double: under the 4 KB a launch may carry):
//               four pointers, count, lr, ld per blob and the prefix of chunk counts.  blockIdx.x is wave-uniform, so
//               the binary search over the prefix and the blob's fields are scalar loads from the argument block.
//   access      16-byte vector loads and stores when all four arrays of the blob are 16-byte aligned (a bit of
//               SolverTable::vec), one element at a time otherwise and in the last, partial group of a blob.  Both run
//               solver_element on the same (w, g, h, h2) in the same order of operations: the same words.
//
// Clipping adds two launches in front: solver_sumsq_kernel (one chunk sum per item, to the workspace) and
// solver_norm_kernel (one workgroup: the chunk sums in ascending order within a blob, the blobs in ascending order;
// it stages 256 sums at a time in LDS and thread 0 adds them).  Workspace: [T l2norm, T scale, T running, T pad]
// [T chunk_sum[items]].  With more than MMS_SOLVER_BLOBS_PER_LAUNCH blobs every launch is repeated per table, in blob
// order; the running sum crosses from one norm launch to the next in the workspace.  Every workspace word that is
// read has been written by this call.
#include <limits.h>

#include <algorithm>
#include <exception>
#include <vector>

#include "mms_internal.h"
#include "mms_solver.h"

namespace mms {
namespace {

constexpr int kSolverThreads = 256;
constexpr int kSolverChunk = MMS_SOLVER_CHUNK;
constexpr int kSolverBlobs = MMS_SOLVER_BLOBS_PER_LAUNCH;
constexpr int kSolverRounds = kSolverChunk / (4 * kSolverThreads);   // groups of 4 elements per thread and item
constexpr int kSolverRoundStride = 4 * kSolverThreads;
constexpr size_t kSolverHeaderWords = 4;                             // l2norm, scale, running, pad
static_assert(kSolverChunk % kSolverRoundStride == 0 && kSolverRounds >= 1, "a chunk is whole rounds of the workgroup");

template <typename T>
struct SolverTable {
  T* data[kSolverBlobs];
  T* diff[kSolverBlobs];
  T* h[kSolverBlobs];
  T* h2[kSolverBlobs];
  T lr[kSolverBlobs];            // rate * lr_mult
  T ld[kSolverBlobs];            // weight_decay * decay_mult
  int count[kSolverBlobs];
  int first[kSolverBlobs + 1];   // first[b]: the first work item of blob b; first[nblobs]: the items of the launch
  unsigned vec;                  // bit b: data, diff, h and h2 of blob b are 16-byte aligned
  int nblobs;
};
static_assert(sizeof(SolverTable<double>) + 64 <= 4096, "the table travels in the kernel arguments");

template <typename T>
struct SolverConsts {
  T m, om, d, accum;             // momentum, 1 - momentum, delta, 1 / iter_size
  const T* scale;                // the clip scale in the workspace, or NULL: no clipping
  int l1, normalize, zero;
};

template <typename T>
struct SolverVec;
template <>
struct SolverVec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct SolverVec<double> { typedef double type __attribute__((ext_vector_type(2))); };

// the blob of work item `item` (wave-uniform): first[b] <= item < first[b + 1]
template <typename T>
__device__ __forceinline__ int solver_find(const SolverTable<T>& tab, int item) {
  int lo = 0, hi = tab.nblobs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.first[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

// One element; every statement is one rounding (include/mms_solver.h).  Leaves the update in g.
template <typename T, int SOLVER>
__device__ __forceinline__ void solver_element(T& w, T& g, T& h, T& h2, T lr, T ld, T scale, const SolverConsts<T>& c) {
  if (c.scale) g = g * scale;
  if (c.normalize) g = g * c.accum;
  if (ld != T(0)) {
    const T r = c.l1 ? T((T(0) < w) - (w < T(0))) : w;
    const T p = ld * r;
    g = g + p;
  }
  if constexpr (SOLVER == MMS_SOLVER_ADADELTA) {
    T u = g * g;
    T a = c.om * u;
    T b = c.m * h;
    h = a + b;
    u = c.d + h2;
    const T t = c.d + h;
    u = u / t;
    u = sqrt(u);
    g = g * u;
    u = g * g;
    a = c.om * u;
    b = c.m * h2;
    h2 = a + b;
    g = lr * g;
  } else {
    const T a = lr * g;
    const T b = c.m * h;
    h = a + b;
    g = h;
  }
  w = w - g;
}

template <typename T, int SOLVER>
__global__ __launch_bounds__(kSolverThreads) void solver_update_kernel(const SolverTable<T> tab, const SolverConsts<T> c) {
  typedef typename SolverVec<T>::type V;
  constexpr int VW = 16 / sizeof(T), NV = 4 / VW;
  constexpr bool ADA = SOLVER == MMS_SOLVER_ADADELTA;
  const int item = blockIdx.x;
  const int b = solver_find(tab, item);
  const size_t n = (size_t)tab.count[b];
  const size_t base = (size_t)(item - tab.first[b]) * kSolverChunk + 4 * threadIdx.x;
  T* const wp = tab.data[b];
  T* const gp = tab.diff[b];
  T* const hp = tab.h[b];
  T* const h2p = tab.h2[b];
  const T lr = tab.lr[b], ld = tab.ld[b];
  const T scale = c.scale ? *c.scale : T(1);
  const bool vec = (tab.vec >> b) & 1u;

  T w[kSolverRounds][4], g[kSolverRounds][4], h[kSolverRounds][4], h2[kSolverRounds][4];
#pragma unroll
  for (int k = 0; k < kSolverRounds; ++k) {
    const size_t e = base + (size_t)k * kSolverRoundStride;
    if (vec && e + 4 <= n) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const V wv = reinterpret_cast<const V*>(wp + e)[v], gv = reinterpret_cast<const V*>(gp + e)[v];
        const V hv = reinterpret_cast<const V*>(hp + e)[v];
        V h2v = {};
        if constexpr (ADA) h2v = reinterpret_cast<const V*>(h2p + e)[v];
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          w[k][v * VW + j] = wv[j]; g[k][v * VW + j] = gv[j]; h[k][v * VW + j] = hv[j]; h2[k][v * VW + j] = h2v[j];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = e + j < n;
        w[k][j] = in ? wp[e + j] : T(0);
        g[k][j] = in ? gp[e + j] : T(0);
        h[k][j] = in ? hp[e + j] : T(0);
        h2[k][j] = T(0);
        if constexpr (ADA) h2[k][j] = in ? h2p[e + j] : T(0);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSolverRounds; ++k) {
    const size_t e = base + (size_t)k * kSolverRoundStride;
    if (e >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      solver_element<T, SOLVER>(w[k][j], g[k][j], h[k][j], h2[k][j], lr, ld, scale, c);
      if (c.zero) g[k][j] = T(0);
    }
    if (vec && e + 4 <= n) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        V wv, gv, hv, h2v;
#pragma unroll
        for (int j = 0; j < VW; ++j) {
          wv[j] = w[k][v * VW + j]; gv[j] = g[k][v * VW + j]; hv[j] = h[k][v * VW + j]; h2v[j] = h2[k][v * VW + j];
        }
        reinterpret_cast<V*>(wp + e)[v] = wv;
        reinterpret_cast<V*>(gp + e)[v] = gv;
        reinterpret_cast<V*>(hp + e)[v] = hv;
        if constexpr (ADA) reinterpret_cast<V*>(h2p + e)[v] = h2v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e + j < n) {
          wp[e + j] = w[k][j];
          gp[e + j] = g[k][j];
          hp[e + j] = h[k][j];
          if constexpr (ADA) h2p[e + j] = h2[k][j];
        }
      }
    }
  }
}

// chunk_sum[item] = the sum of squares of the item's diff elements, in the order the header states
template <typename T>
__global__ __launch_bounds__(kSolverThreads) void solver_sumsq_kernel(const SolverTable<T> tab, T* chunk_sum) {
  typedef typename SolverVec<T>::type V;
  constexpr int VW = 16 / sizeof(T), NV = 4 / VW;
  __shared__ T red[kSolverThreads];
  const int item = blockIdx.x;
  const int b = solver_find(tab, item);
  const size_t n = (size_t)tab.count[b];
  const size_t base = (size_t)(item - tab.first[b]) * kSolverChunk + 4 * threadIdx.x;
  const T* const gp = tab.diff[b];
  const bool vec = (tab.vec >> b) & 1u;
  T x[kSolverRounds][4];
#pragma unroll
  for (int k = 0; k < kSolverRounds; ++k) {
    const size_t e = base + (size_t)k * kSolverRoundStride;
    if (vec && e + 4 <= n) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const V gv = reinterpret_cast<const V*>(gp + e)[v];
#pragma unroll
        for (int j = 0; j < VW; ++j) x[k][v * VW + j] = gv[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[k][j] = e + j < n ? gp[e + j] : T(0);
    }
  }
  T acc = T(0);
#pragma unroll
  for (int k = 0; k < kSolverRounds; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T sq = x[k][j] * x[k][j];
      acc = acc + sq;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kSolverThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) chunk_sum[item] = red[0];
}

// One workgroup: the table's chunk sums in ascending order within a blob, the blob sums in ascending order onto the
// running sum (0 for the first table, head[2] after it); the last table's launch writes l2norm and the scale.
template <typename T>
__global__ __launch_bounds__(kSolverThreads) void solver_norm_kernel(const SolverTable<T> tab, const T* chunk_sum, T* head,
                                                                     int first_table, int last_table, T clip,
                                                                     T* clip_info) {
  __shared__ T buf[kSolverThreads];
  const int t = threadIdx.x;
  T total = T(0);
  if (t == 0 && !first_table) total = head[2];
  for (int b = 0; b < tab.nblobs; ++b) {
    const int lo = tab.first[b], items = tab.first[b + 1] - lo;
    T s = T(0);
    for (int c0 = 0; c0 < items; c0 += kSolverThreads) {
      if (c0 + t < items) buf[t] = chunk_sum[lo + c0 + t];
      __syncthreads();
      if (t == 0) {
        const int m = items - c0 < kSolverThreads ? items - c0 : kSolverThreads;
        int i = 0;
        for (; i + 16 <= m; i += 16) {          // sixteen LDS reads in flight in front of the sixteen dependent adds
          T v[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = buf[i + j];
#pragma unroll
          for (int j = 0; j < 16; ++j) s = s + v[j];
        }
        for (; i < m; ++i) s = s + buf[i];
      }
      __syncthreads();
    }
    total = total + s;
  }
  if (t != 0) return;
  if (!last_table) {
    head[2] = total;
    return;
  }
  const T norm = sqrt(total);
  const T scale = norm > clip ? clip / norm : T(1);
  head[0] = norm;
  head[1] = scale;
  if (clip_info) {
    clip_info[0] = norm;
    clip_info[1] = scale;
  }
}

// what the query and the step judge alike: the parameters and the counts.  *items: work items over all blobs.
int solver_check(const mms_solver_param* p, const mms_solver_blob* blobs, int nblobs, long long* items) {
  if (!p) return MMS_ERR_INVALID_ARG;
  if (p->type != MMS_SOLVER_SGD && p->type != MMS_SOLVER_ADADELTA) return MMS_ERR_UNSUPPORTED;
  if (nblobs < 0 || (nblobs > 0 && !blobs) || p->iter_size < 1) return MMS_ERR_INVALID_ARG;
  if (p->regularization != MMS_SOLVER_L2 && p->regularization != MMS_SOLVER_L1) return MMS_ERR_INVALID_ARG;
  if (p->diff_out != MMS_SOLVER_DIFF_UPDATE && p->diff_out != MMS_SOLVER_DIFF_ZERO) return MMS_ERR_INVALID_ARG;
  long long n = 0;
  for (int i = 0; i < nblobs; ++i) {
    if (blobs[i].count < 0 || blobs[i].count > INT_MAX) return MMS_ERR_INVALID_ARG;
    n += (blobs[i].count + kSolverChunk - 1) / kSolverChunk;
  }
  *items = n;
  return MMS_OK;
}

inline bool solver_clips(const mms_solver_param* p) { return p->clip_gradients >= 0.f; }

template <typename T>
size_t solver_workspace_bytes(const mms_solver_param* p, const mms_solver_blob* blobs, int nblobs) {
  long long items = 0;
  if (solver_check(p, blobs, nblobs, &items) != MMS_OK || items == 0 || !solver_clips(p)) return 0;
  return (kSolverHeaderWords + (size_t)items) * sizeof(T);
}

// The next table: up to kSolverBlobs blobs of count > 0 from blobs[*next ...], in blob order; *next moves past them.
template <typename T>
void solver_next_table(const mms_solver_blob* blobs, int nblobs, int* next, bool ada, T rate, T wd, SolverTable<T>* tab) {
  *tab = SolverTable<T>();
  int i = *next;
  for (; i < nblobs && tab->nblobs < kSolverBlobs; ++i) {
    const mms_solver_blob& bl = blobs[i];
    if (bl.count == 0) continue;
    const int b = tab->nblobs++;
    tab->data[b] = static_cast<T*>(bl.data);
    tab->diff[b] = static_cast<T*>(bl.diff);
    tab->h[b] = static_cast<T*>(bl.hist_grad);
    tab->h2[b] = ada ? static_cast<T*>(bl.hist_update) : nullptr;
    tab->lr[b] = rate * T(bl.lr_mult);
    tab->ld[b] = wd * T(bl.decay_mult);
    tab->count[b] = (int)bl.count;
    tab->first[b + 1] = tab->first[b] + (int)((bl.count + kSolverChunk - 1) / kSolverChunk);
    if (aligned16(bl.data) && aligned16(bl.diff) && aligned16(bl.hist_grad) && (!ada || aligned16(bl.hist_update)))
      tab->vec |= 1u << b;
  }
  *next = i;
}

template <typename T>
int solver_step(const mms_solver_param* p, const mms_solver_blob* blobs, int nblobs, T rate, T* clip_info,
                void* workspace, size_t workspace_bytes, hipStream_t s) {
  long long items = 0;
  int rc = solver_check(p, blobs, nblobs, &items);
  if (rc != MMS_OK) return rc;
  const bool ada = p->type == MMS_SOLVER_ADADELTA, clips = solver_clips(p);
  const size_t need = solver_workspace_bytes<T>(p, blobs, nblobs);
  int nonempty = 0;
  for (int i = 0; i < nblobs; ++i) {
    const mms_solver_blob& bl = blobs[i];
    if (bl.count == 0) continue;
    if (!bl.data || !bl.diff || !bl.hist_grad || (ada && !bl.hist_update)) return MMS_ERR_INVALID_ARG;
    ++nonempty;
  }
  if (nonempty == 0) return MMS_OK;

  // no two arrays overlap: the address ranges (csrc/host_args.h), none of them NULL or empty, sorted by (lo, hi), so
  // that two that meet are neighbours -- O(n log n) for O(blobs) spans.  One launch's worth of them fits the stack; a
  // longer list takes host memory, and a call that cannot have it is refused like any other (nothing crosses the C
  // boundary).
  const size_t nspans_max = 4 * (size_t)nonempty + 2;
  ByteSpan on_stack[4 * kSolverBlobs + 2];
  std::vector<ByteSpan> on_heap;
  ByteSpan* spans = on_stack;
  if (nspans_max > sizeof(on_stack) / sizeof(on_stack[0])) {
    try {
      on_heap.resize(nspans_max);
    } catch (const std::exception&) {
      return MMS_ERR_UNSUPPORTED;
    }
    spans = on_heap.data();
  }
  size_t nspans = 0;
  for (int i = 0; i < nblobs; ++i) {
    const mms_solver_blob& bl = blobs[i];
    if (bl.count == 0) continue;
    const size_t bytes = (size_t)bl.count * sizeof(T);
    spans[nspans++] = byte_span(bl.data, bytes);
    spans[nspans++] = byte_span(bl.diff, bytes);
    spans[nspans++] = byte_span(bl.hist_grad, bytes);
    if (ada) spans[nspans++] = byte_span(bl.hist_update, bytes);
  }
  if (clip_info) spans[nspans++] = byte_span(clip_info, 2 * sizeof(T));
  if (clips && workspace) spans[nspans++] = byte_span(workspace, need);
  std::sort(spans, spans + nspans);
  for (size_t i = 1; i < nspans; ++i)
    if (spans_meet(spans[i - 1], spans[i])) return MMS_ERR_INVALID_ARG;
  if (clips && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;

  const T wd = T(p->weight_decay);
  const int ntables = (nonempty + kSolverBlobs - 1) / kSolverBlobs;
  SolverTable<T> tab;
  SolverConsts<T> c = {};
  c.m = T(p->momentum);
  c.om = T(1) - c.m;
  c.d = T(p->delta);
  c.accum = T(1) / T(p->iter_size);
  c.l1 = p->regularization == MMS_SOLVER_L1;
  c.normalize = p->iter_size != 1;
  c.zero = p->diff_out == MMS_SOLVER_DIFF_ZERO;
  if (clips) {
    T* const head = static_cast<T*>(workspace);
    T* chunk_sum = head + kSolverHeaderWords;
    int next = 0;
    for (int k = 0; k < ntables; ++k) {
      solver_next_table(blobs, nblobs, &next, ada, rate, wd, &tab);
      const int n = tab.first[tab.nblobs];
      hipLaunchKernelGGL((solver_sumsq_kernel<T>), dim3(n), dim3(kSolverThreads), 0, s, tab, chunk_sum);
      if ((rc = launch_status()) != MMS_OK) return rc;
      hipLaunchKernelGGL((solver_norm_kernel<T>), dim3(1), dim3(kSolverThreads), 0, s, tab, chunk_sum, head, k == 0,
                         k + 1 == ntables, T(p->clip_gradients), clip_info);
      if ((rc = launch_status()) != MMS_OK) return rc;
      chunk_sum += n;
    }
    c.scale = head + 1;
  }
  int next = 0;
  for (int k = 0; k < ntables; ++k) {
    solver_next_table(blobs, nblobs, &next, ada, rate, wd, &tab);
    const dim3 grid(tab.first[tab.nblobs]), block(kSolverThreads);
    if (ada)
      hipLaunchKernelGGL((solver_update_kernel<T, MMS_SOLVER_ADADELTA>), grid, block, 0, s, tab, c);
    else
      hipLaunchKernelGGL((solver_update_kernel<T, MMS_SOLVER_SGD>), grid, block, 0, s, tab, c);
    if ((rc = launch_status()) != MMS_OK) return rc;
  }
  return MMS_OK;
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

size_t mms_solver_workspace_bytes(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs) {
  return solver_workspace_bytes<float>(param, blobs, nblobs);
}

size_t mms_solver_workspace_bytes_f64(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs) {
  return solver_workspace_bytes<double>(param, blobs, nblobs);
}

int mms_solver_step_f32(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs, float rate,
                        float* clip_info, void* workspace, size_t workspace_bytes, void* stream) {
  return solver_step<float>(param, blobs, nblobs, rate, clip_info, workspace, workspace_bytes,
                            as_stream(stream));
}

int mms_solver_step_f64(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs, double rate,
                        double* clip_info, void* workspace, size_t workspace_bytes, void* stream) {
  return solver_step<double>(param, blobs, nblobs, rate, clip_info, workspace, workspace_bytes,
                             as_stream(stream));
}

}  // extern "C"
