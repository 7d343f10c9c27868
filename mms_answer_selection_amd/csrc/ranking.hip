// csrc/ranking.hip -- the forward-only ranking metrics that consume the scores of the hot path:
// MAP, MRR, AUC, RankAccuracy.  Here: the host entry points, the radix path and the libstdc++ tie emulation;
// rank_onewg.hip: one workgroup for n <= 2048; rank_common.h: the device pieces both share.  Reference:
//   MAPLayer::Forward_cpu            src/caffe/layers/map_layer.cpp:41-100
//   MRRLayer::Forward_cpu            src/caffe/layers/mrr_layer.cpp:38-79
//   AUCLayer::Forward_cpu            src/caffe/layers/auc_layer.cpp:47-136
//   RankAccuracyLayer::Forward_cpu   src/caffe/layers/rank_accuracy_layer.cpp:36-50
// The reference buckets items by int(group) in a std::map (ascending group id), std::sort's each bucket by score
// descending, and walks it sequentially.  Here: one 64-bit radix sort (rocPRIM) on
//   key = (group id, biased to unsigned) << 32 | order-reversed score bits
// gives "group ascending, score descending" for all buckets at once; one thread per bucket then walks its items and
// one wave folds the buckets in group order, both with the reference's float expressions (`ap += ++rank/(i+1)`,
// `mrr += 1.0/(rank+1)` through double, ...), so MAP/MRR/AUC are bit-identical to the CPU code whenever the order is
// defined.  Ties: std::sort is unstable, so the reference's order among EQUAL scores is implementation-defined; the
// radix sort is stable (original index ascending).  Results can differ from a particular libstdc++ only when equal
// scores carry different labels IN A BUCKET OF MORE THAN 16 ITEMS: up to 16, std::sort is libstdc++'s insertion sort,
// which is stable -- the same order as here (tests/test_gpu_ranking.py, tests/test_gpu_ranking_edges.py,
// tools/soak_ranking_embed.py).  -0.0 and +0.0 are equal scores there, and one key here (desc_bits).
#include <algorithm>
#include <cstdint>
#include <cstring>   // rocPRIM's texture_cache_iterator.hpp calls memset without including it
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "libstdcxx_sort.h"
#include "rank_common.h"

namespace mms {

// How EQUAL scores with different labels are ordered (include/mms.h: mms_set_rank_tie_mode); per calling thread.
static thread_local int t_rank_ties = MMS_RANK_TIES_INPUT_ORDER;
int rank_tie_mode() { return t_rank_ties; }
void set_rank_tie_mode(int m) { t_rank_ties = m; }

// ---- the radix path: keys -> rocPRIM sort -> one walk per bucket -> one-wave fold ----------------------------------
template <class T>
__global__ __launch_bounds__(256) void rank_keys_kernel(int n, int stride, int offset, int inner,
                                                        const T* __restrict__ prob, const T* __restrict__ group,
                                                        unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  keys[i] = rank_key(i, stride, offset, inner, prob, group);
  vals[i] = (unsigned)i;
}
template <class T>
__global__ __launch_bounds__(256) void rank_bucket_pos_kernel(int n, const unsigned long long* __restrict__ keys,
                                                              const T* __restrict__ lab_pos, T* __restrict__ ap_out,
                                                              int* __restrict__ rank_out, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rank_bucket_at<true>(i, n, keys, nullptr, lab_pos, ap_out, rank_out, flags);
}
template <class T>
__global__ __launch_bounds__(256) void rank_bucket_kernel(int n, const unsigned long long* __restrict__ keys,
                                                          const unsigned* __restrict__ vals,
                                                          const T* __restrict__ label, T* __restrict__ ap_out,
                                                          int* __restrict__ rank_out, int* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rank_bucket_at(i, n, keys, vals, label, ap_out, rank_out, flags);
}
template <class T>
__global__ __launch_bounds__(64) void rank_fold_kernel(int n, const T* __restrict__ ap, const int* __restrict__ rank,
                                                       const int* __restrict__ flags, T* __restrict__ map_out,
                                                       T* __restrict__ mrr_out, int* __restrict__ effective) {
  rank_fold_wave(threadIdx.x, n, ap, rank, flags, map_out, mrr_out, effective);
}
template <class T>
__global__ __launch_bounds__(64) void auc_fold_kernel(int n, const unsigned* __restrict__ vals,
                                                      const T* __restrict__ label, int has_ignore, int ignore_label,
                                                      T* __restrict__ auc_out) {
  auc_fold_wave(threadIdx.x, n, vals, label, has_ignore, ignore_label, auc_out);
}

// ---- MMS_RANK_TIES_LIBSTDCXX: the order a libstdc++ build of the reference leaves EQUAL scores in -----------------
// std::sort is not stable; where equal scores carry different labels the metrics depend on what that algorithm
// does.  Up to 16 items it is a stable insertion sort (= the stable order above).  For larger buckets with such a
// tie the bucket is re-sorted by ONE lane running libstdcxx_sort.h on the bucket's items in their original
// (push_back) order -- sequential by nature, hence opt-in: a few microseconds for a TREC-QA candidate group, but
// milliseconds for AUC's single bucket of thousands of items.
constexpr int kTieLds = 4096;
template <class T>
__global__ __launch_bounds__(256) void rank_ties_detect_kernel(int n, const unsigned long long* __restrict__ keys,
                                                               const unsigned* __restrict__ vals,
                                                               const T* __restrict__ label, T* __restrict__ lab_pos,
                                                               int* __restrict__ work, int* __restrict__ nwork) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  lab_pos[i] = label[vals[i]];
  const unsigned g = (unsigned)(keys[i] >> 32);
  if (i != 0 && (unsigned)(keys[i - 1] >> 32) == g) return;
  int m = 0;
  bool cross = false;
  for (int p = i; p < n && (unsigned)(keys[p] >> 32) == g; ++p) {
    ++m;
    if (p > i && (unsigned)keys[p] == (unsigned)keys[p - 1] && (int)label[vals[p]] != (int)label[vals[p - 1]])
      cross = true;
  }
  if (cross && m > 16) {
    const int w = atomicAdd(nwork, 1);
    work[2 * w] = i;
    work[2 * w + 1] = m;
  }
}
template <class T>
__global__ __launch_bounds__(64) void rank_ties_emulate_kernel(int stride, int offset, int inner,
                                                               const T* __restrict__ prob, const T* __restrict__ label,
                                                               const unsigned* __restrict__ vals,
                                                               const int* __restrict__ work,
                                                               const int* __restrict__ nwork, int skip_ignored,
                                                               int ignore_label, T* __restrict__ lab_pos,
                                                               SortItem* __restrict__ g_items,
                                                               unsigned* __restrict__ g_idx) {
  __shared__ SortItem s_items[kTieLds];
  __shared__ unsigned s_idx[kTieLds];
  if (threadIdx.x != 0) return;                      // the algorithm is sequential: one lane per bucket
  const int cnt = *nwork;
  for (int w = blockIdx.x; w < cnt; w += gridDim.x) {
    const int start = work[2 * w], m = work[2 * w + 1];
    SortItem* it = m <= kTieLds ? s_items : g_items + start;
    unsigned* ix = m <= kTieLds ? s_idx : g_idx + start;
    // the bucket in push_back order = ascending item index (a heap sort of the indices: they are distinct)
    for (int j = 0; j < m; ++j) ix[j] = vals[start + j];
    for (int root0 = m / 2 - 1; root0 >= 0; --root0) {
      int root = root0;
      const unsigned v = ix[root];
      for (int c = 2 * root + 1; c < m; c = 2 * root + 1) {
        if (c + 1 < m && ix[c + 1] > ix[c]) ++c;
        if (ix[c] <= v) break;
        ix[root] = ix[c]; root = c;
      }
      ix[root] = v;
    }
    for (int end = m - 1; end > 0; --end) {
      const unsigned v = ix[end];
      ix[end] = ix[0];
      int root = 0;
      for (int c = 1; c < end; c = 2 * root + 1) {
        if (c + 1 < end && ix[c + 1] > ix[c]) ++c;
        if (ix[c] <= v) break;
        ix[root] = ix[c]; root = c;
      }
      ix[root] = v;
    }
    int used = 0;
    for (int j = 0; j < m; ++j) {
      const int idx = (int)ix[j], lab = (int)label[idx];
      if (skip_ignored && lab == ignore_label) continue;                        // auc_layer.cpp:68-70: never pushed
      const int o = idx / inner, jj = idx - o * inner;
      it[used].key = (float)prob[(size_t)o * stride + (size_t)offset * inner + jj];   // pair<float, int>
      it[used].lab = lab;
      ++used;
    }
    libstdcxx_sort(it, used);
    for (int j = 0; j < used; ++j) lab_pos[start + j] = (T)it[j].lab;
    for (int j = used; j < m; ++j) lab_pos[start + j] = (T)ignore_label;   // skipped: behind the rest, still skipped
  }
}

template <class T>
__global__ __launch_bounds__(256) void rank_accuracy_kernel(int count, const T* __restrict__ a,
                                                            const T* __restrict__ b, const T* __restrict__ label,
                                                            unsigned* __restrict__ partial) {
  __shared__ unsigned red[4];
  unsigned c = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256)
    c += (label[i] * (a[i] - b[i])) > 0 ? 1u : 0u;      // :45
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
template <class T>
__global__ void rank_accuracy_finish_kernel(int blocks, int count, const unsigned* __restrict__ partial,
                                            T* __restrict__ out) {
  if (threadIdx.x != 0) return;
  unsigned long long c = 0;
  for (int i = 0; i < blocks; ++i) c += partial[i];
  // the reference accumulates 0/1 into a Dtype: for float exact up to 2^24, then it sticks (a double never gets there)
  T acc = sizeof(T) == 4 && c > 16777216ull ? (T)16777216 : (T)c;
  *out = acc / count;
}

// ---- the workspace of the radix path: typed views of the caller's buffer, each 256-byte aligned --------------------
template <class T>
struct RankWs {
  unsigned long long *keys0, *keys1;                   // keys0 / vals0: unsorted; keys1 / vals1: sorted
  unsigned *vals0, *vals1, *tidx;
  T *ap, *labpos;                                      // labpos, work, nwork, titems, tidx: MMS_RANK_TIES_LIBSTDCXX
  int *rr, *flags, *work, *nwork;
  SortItem* titems;
  size_t front, total;                                 // front: bytes of the above; behind them rocPRIM's scratch
};
template <class T>
static RankWs<T> rank_ws(int n, void* ws) {            // ws == nullptr: for the sizes only
  RankWs<T> w{};
  size_t o = 0;
  auto take = [&](auto*& p, size_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(ws) + o);
    o += round_up(bytes, 256);
  };
  take(w.keys0, (size_t)n * 8); take(w.keys1, (size_t)n * 8);
  take(w.vals0, (size_t)n * 4); take(w.vals1, (size_t)n * 4);
  take(w.ap, (size_t)n * sizeof(T)); take(w.rr, (size_t)n * 4); take(w.flags, (size_t)n * 4);
  take(w.labpos, (size_t)n * sizeof(T)); take(w.work, (size_t)n * 8); take(w.nwork, 256);
  take(w.titems, (size_t)n * sizeof(SortItem)); take(w.tidx, (size_t)n * 4);
  w.front = o;
  w.total = o + (size_t)n * 8 + (4u << 20);   // generous bound for rocPRIM's scratch; checked at run time
  return w;
}
size_t rank_workspace_bytes(int n) { return rank_ws<float>(n, nullptr).total; }
size_t rank_workspace_bytes_f64(int n) { return rank_ws<double>(n, nullptr).total; }
// The front both metrics share: keys kernel -> radix sort -> in libstdc++ mode the tie emulation.  On MMS_OK the sorted
// pairs are in w.keys1 / w.vals1 and *labpos is the labels by sorted position (libstdc++ mode) or null (gather them).
// key_bits: 64 with groups, 32 without; emulate_grid: one-lane workgroups (AUC has one bucket); skip_ignored: :68-70.
template <class T>
static int rank_sorted_front(const RankWs<T>& w, void* ws, size_t ws_bytes, int n, int stride, int offset, int inner,
                             const T* prob, const T* label, const T* group, bool libstd, unsigned key_bits,
                             unsigned emulate_grid, int skip_ignored, int ignore_label, const T** labpos,
                             hipStream_t s) {
  *labpos = nullptr;
  if (!ws || ws_bytes < w.front) return MMS_ERR_WORKSPACE;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(rank_keys_kernel<T>, dim3(grid), dim3(256), 0, s, n, stride, offset, inner, prob, group, w.keys0,
                     w.vals0);
  size_t need = 0;
  const size_t N = (size_t)n;
  if (rocprim::radix_sort_pairs(nullptr, need, w.keys0, w.keys1, w.vals0, w.vals1, N, 0u, key_bits, s) != hipSuccess)
    return MMS_ERR_LAUNCH;
  if (w.front + need > ws_bytes) return MMS_ERR_WORKSPACE;                     // the run-time check of rank_ws's bound
  void* temp = static_cast<char*>(ws) + w.front;
  if (rocprim::radix_sort_pairs(temp, need, w.keys0, w.keys1, w.vals0, w.vals1, N, 0u, key_bits, s) != hipSuccess)
    return MMS_ERR_LAUNCH;
  if (!libstd) return MMS_OK;
  if (hipMemsetAsync(w.nwork, 0, sizeof(int), s) != hipSuccess) return MMS_ERR_LAUNCH;
  hipLaunchKernelGGL(rank_ties_detect_kernel<T>, dim3(grid), dim3(256), 0, s, n, w.keys1, w.vals1, label, w.labpos,
                     w.work, w.nwork);
  hipLaunchKernelGGL(rank_ties_emulate_kernel<T>, dim3(emulate_grid), dim3(64), 0, s, stride, offset, inner, prob,
                     label, w.vals1, w.work, w.nwork, skip_ignored, ignore_label, w.labpos, w.titems, w.tidx);
  *labpos = w.labpos;
  return MMS_OK;
}

template <class T>
int rank_map_mrr(int n, int fixed_axis, const T* prob, const T* label, const T* group, T* map_out, T* mrr_out,
                 int* effective, void* ws, size_t ws_bytes, hipStream_t s) {
  const bool libstd = rank_tie_mode() == MMS_RANK_TIES_LIBSTDCXX;
  const RankRoute route = rank_route(n, libstd);
  // score of item i: prob[i*(fixed_axis+1) + fixed_axis]  (map_layer.cpp:50, mrr_layer.cpp:49)
  if (route != RankRoute::kRadix)
    return rank_onewg(route, false, n, fixed_axis + 1, fixed_axis, 1, prob, label, group, 0, 0, map_out, mrr_out,
                      effective, s);
  const RankWs<T> w = rank_ws<T>(n, ws);
  const T* labpos;
  const int rc = rank_sorted_front(w, ws, ws_bytes, n, fixed_axis + 1, fixed_axis, 1, prob, label, group, libstd, 64u,
                                   256u, 0, 0, &labpos, s);
  if (rc != MMS_OK) return rc;
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
  if (labpos) hipLaunchKernelGGL(rank_bucket_pos_kernel<T>, g, b, 0, s, n, w.keys1, labpos, w.ap, w.rr, w.flags);
  else hipLaunchKernelGGL(rank_bucket_kernel<T>, g, b, 0, s, n, w.keys1, w.vals1, label, w.ap, w.rr, w.flags);
  hipLaunchKernelGGL(rank_fold_kernel<T>, dim3(1), dim3(64), 0, s, n, w.ap, w.rr, w.flags, map_out, mrr_out,
                     effective);
  return launch_status();
}

// n = outer * inner items; dim = channels * inner elements per outer index
template <class T>
int rank_auc(int n, int dim, int fixed_axis, int inner, const T* prob, const T* label, int has_ignore, int ignore_label,
             T* auc_out, void* ws, size_t ws_bytes, hipStream_t s) {
  const bool libstd = rank_tie_mode() == MMS_RANK_TIES_LIBSTDCXX;
  const RankRoute route = rank_route(n, libstd);
  const T* const no_group = nullptr;
  // score of item i: prob[i*dim + fixed_axis]  (auc_layer.cpp:75-76 with inner_num = 1)
  if (route != RankRoute::kRadix)
    return rank_onewg(route, true, n, dim, fixed_axis, inner, prob, label, no_group, has_ignore, ignore_label, auc_out,
                      static_cast<T*>(nullptr), static_cast<int*>(nullptr), s);
  const RankWs<T> w = rank_ws<T>(n, ws);
  const T* labpos;
  const int rc = rank_sorted_front(w, ws, ws_bytes, n, dim, fixed_axis, inner, prob, label, no_group, libstd, 32u, 1u,
                                   has_ignore, ignore_label, &labpos, s);
  if (rc != MMS_OK) return rc;
  hipLaunchKernelGGL(auc_fold_kernel<T>, dim3(1), dim3(64), 0, s, n, labpos ? nullptr : w.vals1,   // null: label[p]
                     labpos ? labpos : label, has_ignore, ignore_label, auc_out);
  return launch_status();
}
template <class T>
int rank_accuracy(int count, const T* a, const T* b, const T* label, T* out, void* ws, size_t ws_bytes, hipStream_t s) {
  const int blocks = std::min(std::max((count + 1023) / 1024, 1), 1024);
  if (!ws || ws_bytes < (size_t)blocks * sizeof(unsigned)) return MMS_ERR_WORKSPACE;
  unsigned* partial = static_cast<unsigned*>(ws);
  hipLaunchKernelGGL(rank_accuracy_kernel<T>, dim3(blocks), dim3(256), 0, s, count, a, b, label, partial);
  hipLaunchKernelGGL(rank_accuracy_finish_kernel<T>, dim3(1), dim3(64), 0, s, blocks, count, partial, out);
  return launch_status();
}

// Layer<float> and Layer<double>: the two instantiations the reference makes (INSTANTIATE_CLASS, common.hpp:41-44)
#define MMS_RANK_INSTANTIATE(T)                                                                                        \
  template int rank_map_mrr<T>(int, int, const T*, const T*, const T*, T*, T*, int*, void*, size_t, hipStream_t);      \
  template int rank_auc<T>(int, int, int, int, const T*, const T*, int, int, T*, void*, size_t, hipStream_t);          \
  template int rank_accuracy<T>(int, const T*, const T*, const T*, T*, void*, size_t, hipStream_t)
MMS_RANK_INSTANTIATE(float);
MMS_RANK_INSTANTIATE(double);
#undef MMS_RANK_INSTANTIATE

}  // namespace mms
