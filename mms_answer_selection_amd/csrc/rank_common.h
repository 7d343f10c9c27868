// csrc/rank_common.h -- the device pieces of the ranking metrics that both ranking.hip and rank_onewg.hip use: the sort
// key, the (key, index) order, the bucket rule and walk, the one-wave folds.
#ifndef MMS_RANK_COMMON_H_
#define MMS_RANK_COMMON_H_

#include "mms_internal.h"

namespace mms {

// -0.0 and +0.0 are one key: the reference's `lhs.first > rhs.first` holds them equal (map_layer.cpp:33-38), so they
// keep input order in the stable sorts and are seen as a tie by rank_ties_detect_kernel
__device__ __forceinline__ unsigned desc_bits(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;                      // -0.0 -> +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending total order
  return ~u;                                         // descending
}
// item i = (outer o, inner j) = (i / inner, i % inner); its score is prob[o*stride + offset*inner + j]
// (auc_layer.cpp:75-76; inner = 1 for MAP / MRR and for prob (N, C))
// T = double: the reference's comparators take std::pair<float, int> for every Dtype (map_layer.cpp:34,
// mrr_layer.cpp:33, auc_layer.cpp:42 -- AUC's vector holds pair<Dtype, int>, but std::sort hands them over through
// the converting constructor), so the ORDER is always that of the scores narrowed to float: one key for both types.
// Only the folds below run in Dtype.
template <class T>
__device__ __forceinline__ unsigned long long rank_key(int i, int stride, int offset, int inner,
                                                        const T* __restrict__ prob, const T* __restrict__ group) {
  const unsigned g = group ? (unsigned)((int)group[i]) + 0x80000000u : 0u;   // map<int,...> key order
  const int o = i / inner, j = i - o * inner;
  return ((unsigned long long)g << 32) | desc_bits((float)prob[(size_t)o * stride + (size_t)offset * inner + j]);
}
// (key, original index) in lexicographic order: does pair a come after pair b?  The index as the minor key makes every
// sort of such pairs the STABLE order the radix sort gives, and the pairs distinct (no tie rule needed)
__device__ __forceinline__ bool pair_after(unsigned long long ka, unsigned va, unsigned long long kb, unsigned vb) {
  return ka > kb || (ka == kb && va > vb);
}
// a lane's value of the element type, by compile-time or wave-uniform lane number
__device__ __forceinline__ float wave_readlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double wave_readlane(double v, int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int wave_inclusive_scan_i32(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
// The bucket rule, from a walked bucket's count of labels == 1, whether it holds a label != 1 and a label == 0, and the
// position of its first label 1 (-1: none).  Bit 0: the bucket counts for MAP (a label == 1 and a label != 1 present,
// map_layer.cpp:80-92), with ap_sum / map_rank (:93); bit 1: it counts for MRR (a label == 1 and a label == 0 present,
// mrr_layer.cpp:61-73), with 1.0 / (first + 1) (:75).  The two quotients stay with the callers: one stores the rank.
__device__ __forceinline__ int rank_bucket_flags(int map_rank, int not_one, int zero, int first) {
  int fl = 0;
  if (map_rank >= 1 && not_one) fl |= 1;
  if (first >= 0 && zero) fl |= 2;
  return fl;
}
// One thread per sorted position; the thread at a bucket's first position walks the bucket (map_layer.cpp:76-96,
// mrr_layer.cpp:57-75) and stores its results at that position (the MRR rank itself: the fold divides).
// BYPOS: `label` is already in sorted order (label[p]); otherwise it is gathered through the permutation
template <bool BYPOS = false, class T>
__device__ __forceinline__ void rank_bucket_at(int i, int n, const unsigned long long* keys, const unsigned* vals,
                                               const T* label, T* ap_out, int* rank_out, int* flags) {
  const unsigned g = (unsigned)(keys[i] >> 32);
  int fl = 0;
  if (i == 0 || (unsigned)(keys[i - 1] >> 32) != g) {
    T ap = 0;
    int map_rank = 0, not_one = 0, zero = 0, mrr_rank = -1;
    for (int p = i; p < n && (unsigned)(keys[p] >> 32) == g; ++p) {
      const int lab = (int)(BYPOS ? label[p] : label[vals[p]]);
      const int pos = p - i;
      if (lab == 1) {
        ap += (++map_rank) / (T)(pos + 1);
        if (mrr_rank < 0) mrr_rank = pos;
      } else {
        not_one = 1;
        if (lab == 0) zero = 1;
      }
    }
    fl = rank_bucket_flags(map_rank, not_one, zero, mrr_rank);
    if (fl & 1) ap_out[i] = ap / map_rank;
    if (fl & 2) rank_out[i] = mrr_rank;
  }
  flags[i] = fl;
}
// Folds the buckets in sorted (= ascending group id) order with the reference's running sums.  The sums are sequential
// by definition; ONE WAVE runs them on 64 positions per step: ballots pick the lanes that carry a bucket result, and
// the wave-uniform running sums are advanced in lane order with v_readlane.
template <class T>
struct RankSums {
  T map_ = 0, mrr = 0;
  int eff_map = 0, eff_mrr = 0;
  // one step: this lane's bucket flags `fl` and ap; inv_of(l) gives lane l's 1.0 / (mrr_rank + 1) as a double
  template <class Inv>
  __device__ __forceinline__ void step(int fl, T ap, Inv inv_of) {
    unsigned long long m1 = __ballot(fl & 1), m2 = __ballot(fl & 2);
    eff_map += __popcll(m1);
    eff_mrr += __popcll(m2);
    while (m1) {                                                   // map_layer.cpp:93-94
      const int l = __ffsll((long long)m1) - 1;
      m1 &= m1 - 1;
      map_ += wave_readlane(ap, l);
    }
    while (m2) {   // mrr += 1.0/(mrr_rank+1): Dtype + double, stored back to Dtype (mrr_layer.cpp:75)
      const int l = __ffsll((long long)m2) - 1;
      m2 &= m2 - 1;
      mrr = (T)((double)mrr + inv_of(l));
    }
  }
  __device__ __forceinline__ void finish(int lane, T* __restrict__ map_out, T* __restrict__ mrr_out,
                                         int* __restrict__ effective) const {
    if (lane != 0) return;
    if (map_out) *map_out = map_ / eff_map;   // NaN when no bucket counts, like the reference (:99)
    if (mrr_out) *mrr_out = mrr / eff_mrr;
    if (effective) *effective = eff_map;
  }
};
// the fold over what rank_bucket_at stored, one entry per sorted position: the operands arrive 64 positions per
// coalesced load (four loads in flight) instead of one dependent load per position
template <class T>
__device__ __forceinline__ void rank_fold_wave(int lane, int n, const T* ap, const int* rank, const int* flags,
                                               T* __restrict__ map_out, T* __restrict__ mrr_out,
                                               int* __restrict__ effective) {
  RankSums<T> s;
  int nfl[4], nrk[4];
  T na[4];
  auto fetch = [&](int base) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + 64 * u + lane, ic = i < n ? i : n - 1;
      nfl[u] = flags[ic];
      na[u] = ap[ic];
      nrk[u] = rank[ic];
    }
  };
  fetch(0);
  for (int base = 0; base < n; base += 256) {
    int fl[4], rk[4];
    T a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fl[u] = (base + 64 * u + lane < n) ? nfl[u] : 0;
      a[u] = na[u];
      rk[u] = nrk[u];
    }
    if (base + 256 < n) fetch(base + 256);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      s.step(fl[u], a[u], [&](int l) { return 1.0 / (__builtin_amdgcn_readlane(rk[u], l) + 1); });
  }
  s.finish(lane, map_out, mrr_out, effective);
}

// AUC: global descending sort, then the reference's sequential walk (auc_layer.cpp:119-134):
//   high += lab; auc += high * (1 - lab)     (ints; the product is converted to float and added)
// `high` is an integer prefix sum (exact in any order); the float running sum is the only sequential part.  One wave:
// 64 sorted items per step, labels gathered through the sort permutation four steps ahead, `high` by a wave scan, and
// the 64 terms added in item order with compile-time-lane v_readlane (two instructions per item, one dependent add).
template <class T>
__device__ __forceinline__ void auc_fold_wave(int lane, int n, const unsigned* vals, const T* __restrict__ label,
                                              int has_ignore, int ignore_label, T* __restrict__ auc_out) {
  T auc = 0;
  int high = 0, count = 0;
  T nxt[4];
  auto fetch = [&](int base) {                    // clamped addresses: unconditional loads
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + 64 * u + lane;
      nxt[u] = vals ? label[vals[i < n ? i : n - 1]] : label[i < n ? i : n - 1];  // vals == nullptr: labels by position
    }
  };
  fetch(0);
  for (int base = 0; base < n; base += 256) {
    int lab[4];
    bool use[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + 64 * u + lane;
      lab[u] = (int)nxt[u];
      use[u] = i < n && !(has_ignore && lab[u] == ignore_label);     // :68-70 (skipped items keep their order)
      if (!use[u]) lab[u] = 0;
    }
    if (base + 256 < n) fetch(base + 256);        // in flight behind this block's 256 dependent adds
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int incl = high + wave_inclusive_scan_i32(lab[u], lane);
      const T term = use[u] ? (T)(incl * (1 - lab[u])) : (T)0;   // skipped items add +0: exact (auc >= 0 ... or any)
      count += __popcll(__ballot(use[u]));
      high = __builtin_amdgcn_readlane(incl, 63);
#pragma unroll
      for (int l = 0; l < 64; ++l)
        auc += wave_readlane(term, l);
    }
  }
  if (lane == 0) *auc_out = high > 0 ? auc / high / (count - high) : (T)0;
}

}  // namespace mms
#endif  // MMS_RANK_COMMON_H_
