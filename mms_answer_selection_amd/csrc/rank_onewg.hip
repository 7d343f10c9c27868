// csrc/rank_onewg.hip -- MAP / MRR / AUC of up to 2,048 items as ONE workgroup and one launch instead of the radix
// path's seven (ranking.hip).  Same expressions in the same order (rank_common.h): the same bits.
#include "rank_common.h"

namespace mms {

// ---- n <= 512: a bitonic sort in LDS, then rank_bucket_at and rank_fold_wave reading LDS ----------------------------
// Measured with the capacity at 2048: 1,517 items 47 us against 45-51 us for the multi-launch path -- one CU's LDS and
// barriers are no faster than rocPRIM's several launches at that size -- so it serves n <= 512 only.
constexpr int kRankSmall = 512;
template <int MODE, class T>                         // 0: MAP / MRR, 1: AUC
__global__ __launch_bounds__(1024) void rank_small_kernel(int n, int stride, int offset, int inner,
                                                          const T* __restrict__ prob, const T* __restrict__ label,
                                                          const T* __restrict__ group, int has_ignore, int ignore_label,
                                                          T* __restrict__ out0, T* __restrict__ out1,
                                                          int* __restrict__ effective) {
  __shared__ unsigned long long keys[kRankSmall];
  __shared__ unsigned vals[kRankSmall];
  __shared__ T ap[MODE == 0 ? kRankSmall : 1];
  __shared__ int rk[MODE == 0 ? kRankSmall : 1];
  __shared__ int fl[MODE == 0 ? kRankSmall : 1];
  __shared__ T slab[MODE == 0 ? kRankSmall : 1];   // labels in sorted order: the bucket walks read LDS only
  const int t = threadIdx.x;
  int P = 64;
  while (P < n) P <<= 1;                             // sorted size: a power of two, padded with maximal keys
  for (int i = t; i < P; i += 1024) {
    keys[i] = i < n ? rank_key(i, stride, offset, inner, prob, group) : ~0ull;
    vals[i] = (unsigned)i;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (P >> 1); p += 1024) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;   // the pair (i, i ^ j) with i < q; j = 2^m
        const bool up = (i & k) == 0;
        const unsigned long long ki = keys[i], kq = keys[q];
        const unsigned vi = vals[i], vq = vals[q];
        if (pair_after(ki, vi, kq, vq) == up) { keys[i] = kq; keys[q] = ki; vals[i] = vq; vals[q] = vi; }
      }
      __syncthreads();
    }
  }
  if (MODE == 0) {
    // a walk that gathers label[vals[p]] itself pays one memory round trip per item (its loop exit depends on
    // the keys, so the loads cannot be issued ahead)
    for (int i = t; i < n; i += 1024) slab[i] = label[vals[i]];
    __syncthreads();
    for (int i = t; i < n; i += 1024) rank_bucket_at<true>(i, n, keys, vals, slab, ap, rk, fl);
    __syncthreads();
    if (t < 64) rank_fold_wave(t, n, ap, rk, fl, out0, out1, effective);
  } else if (t < 64) {
    auc_fold_wave(t, n, vals, label, has_ignore, ignore_label, out0);
  }
}

// ---- 512 < n <= 2048: the same one-workgroup metric with a sort that starts in registers ----------------------------
// The LDS bitonic sort above pays a workgroup barrier and two LDS round trips for each of its log^2 passes: at 2,048
// padded items that is 66 passes and 47 us, no better than rocPRIM's launches -- while 1,517 candidates are exactly
// the TREC-QA test split a TEST net ranks per pass (cfg 4).  Here thread t of 1,024 holds items 2t and 2t + 1.
// Sort = (1) each wave sorts its 128 items in registers (bitonic network of 28 passes; the partner of a lane at
// distance 1 / 2 / 4 / 8 / 16 / 32 comes by DPP or v_permlane{16,32}_swap, no LDS), then (2) four MERGE rounds
// 128 -> 256 -> 512 -> 1024 -> 2048: every item finds by binary search how many items of the sibling run precede it
// and is written to its merged position in the other LDS buffer.  8 + 9 + 10 + 11 dependent LDS reads and four barriers
// instead of the 66 passes (56 of them 6 ds_bpermute each, 10 through LDS with a barrier) of one flat bitonic network:
// 19 -> 11.8 us at 1,517 items on a lone workgroup (profiles/r03_rank_mid_phases_merge_sort.txt: the 38 search steps
// are bound by the LDS round trip at that clock).
constexpr int kRankMid = 2048;

// thread t's (key, index) pairs 2t and 2t + 1; by value through the sort phases: their exchanges stay register selects
struct MidItems {
  unsigned long long k[2];
  unsigned v[2];
};
// the value lane (lane ^ m) holds, m a compile-time power of two
__device__ __forceinline__ unsigned lane_xor(unsigned x, int m, int lane) {
  switch (m) {
    case 1: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
    case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
    case 4: {                                          // row_shl:4: lane i <- i + 4, row_shr:4: lane i <- i - 4
      const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xf, 0xf, true);
      const unsigned dn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);
      return (lane & 4) ? dn : up;
    }
    case 8: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, true);     // row_ror:8 = lane ^ 8
    case 16: { const auto sw = __builtin_amdgcn_permlane16_swap(x, x, false, false); return sw[0] ^ sw[1] ^ x; }
    default: { const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false); return sw[0] ^ sw[1] ^ x; }
  }
}
// phase 1: the wave's 128 (key, index) pairs, two per lane at local positions 2 lane and 2 lane + 1, sorted ascending
__device__ __forceinline__ MidItems mid_sort_wave(MidItems it) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int kk = 2; kk <= 128; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
      if (j == 1) {                                   // both positions inside the thread
        const bool up = ((2 * lane) & kk) == 0;
        if (pair_after(it.k[0], it.v[0], it.k[1], it.v[1]) == up) {
          const unsigned long long tk = it.k[0]; it.k[0] = it.k[1]; it.k[1] = tk;
          const unsigned tv = it.v[0]; it.v[0] = it.v[1]; it.v[1] = tv;
        }
      } else {
        const int m = j >> 1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int p = 2 * lane + e;                 // position inside the wave's block of 128
          const unsigned lo = lane_xor((unsigned)it.k[e], m, lane), hi = lane_xor((unsigned)(it.k[e] >> 32), m, lane);
          const unsigned vo = lane_xor(it.v[e], m, lane);
          const unsigned long long ko = ((unsigned long long)hi << 32) | lo;
          // `lower`: this element is at the smaller position of its pair; an ascending pair keeps the smaller one there
          const bool lower = (p & j) == 0, up = (p & kk) == 0;
          if (pair_after(it.k[e], it.v[e], ko, vo) == (lower == up)) { it.k[e] = ko; it.v[e] = vo; }
        }
      }
    }
  }
  return it;
}
// phase 2: the four merge rounds, ping-pong between keys / vals and xk / xv; on return the sorted pairs are in keys /
// vals, thread t's two in `it` as well, and xk / xv are free
__device__ __forceinline__ MidItems mid_merge_rounds(MidItems it, unsigned long long* keys, unsigned* vals,
                                                     unsigned long long* xk, unsigned* xv) {
  const int t = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 2; ++e) { keys[2 * t + e] = it.k[e]; vals[2 * t + e] = it.v[e]; }
  int buf = 0;                                        // 0: the runs are in keys / vals, 1: in xk / xv
#pragma unroll 1
  for (int L = 128; L < kRankMid; L <<= 1) {
    __syncthreads();
    const unsigned long long* ck = buf ? xk : keys;
    const unsigned* cv = buf ? xv : vals;
    unsigned long long* nk = buf ? keys : xk;
    unsigned* nv = buf ? vals : xv;
    int cnt[2], sbase[2];
    unsigned long long mk[2];
    unsigned mv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pos = 2 * t + e;
      mk[e] = ck[pos]; mv[e] = cv[pos];
      sbase[e] = (pos & ~(L - 1)) ^ L;                // first position of the sibling run
      cnt[e] = 0;
    }
    for (int sstep = L >> 1; sstep >= 1; sstep >>= 1) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int q = sbase[e] + cnt[e] + sstep - 1;
        if (pair_after(mk[e], mv[e], ck[q], cv[q])) cnt[e] += sstep;
      }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int q = sbase[e] + cnt[e];                // (cnt <= L - 1 here: one more look decides cnt == L)
      if (pair_after(mk[e], mv[e], ck[q], cv[q])) cnt[e] += 1;
      const int pos = 2 * t + e;
      const int np = (pos & ~(2 * L - 1)) + (pos & (L - 1)) + cnt[e];
      nk[np] = mk[e]; nv[np] = mv[e];
    }
    buf ^= 1;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e) { it.k[e] = (buf ? xk : keys)[2 * t + e]; it.v[e] = (buf ? xv : vals)[2 * t + e]; }
  __syncthreads();                                    // the last readers of keys / vals as exchange buffers are done
#pragma unroll
  for (int e = 0; e < 2; ++e) { keys[2 * t + e] = it.k[e]; vals[2 * t + e] = it.v[e]; }
  __syncthreads();
  return it;
}
// phase 3: two workgroup scans at once over the items in position order: (a) bucket number = inclusive count of bucket
// heads, (b) inclusive count of label == 1; thread t's own come back in lab / a / b.  Stored for after the caller's
// next barrier: slab[i] label (int bits), npos[i] count (b), hd[bucket] its head, *nb_s the bucket count.  One barrier.
template <class T>
__device__ __forceinline__ void mid_scan_heads(int t, int n, const unsigned long long (&k)[2], const T* label,
                                               const unsigned long long* keys, const unsigned* vals, int (*wtot)[16],
                                               float* slab, unsigned* npos, int* hd, int* nb_s, int (&lab)[2],
                                               int (&a)[2], int (&b)[2]) {
  const int i0 = 2 * t, i1 = 2 * t + 1, lane = t & 63, wv = t >> 6;
  // labels in sorted order (the gather through the permutation: global loads, all independent)
  const int l0 = lab[0] = i0 < n ? (int)label[vals[i0]] : 0, l1 = lab[1] = i1 < n ? (int)label[vals[i1]] : 0;
  const unsigned g0 = (unsigned)(k[0] >> 32), g1 = (unsigned)(k[1] >> 32);
  const unsigned gprev = __shfl_up(g1, 1, 64);
  unsigned gp = gprev;                             // group of position i0 - 1: the previous thread's second item
  if (lane == 0) gp = t ? (unsigned)(keys[i0 - 1] >> 32) : 0u;
  const int h0 = i0 < n && (i0 == 0 || gp != g0), h1 = i1 < n && g1 != g0;
  int a0 = h0, a1 = h0 + h1, b0 = (l0 == 1), b1 = b0 + (l1 == 1);
  int sa = a1, sb = b1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oa = __shfl_up(sa, d, 64), ob = __shfl_up(sb, d, 64);
    if (lane >= d) { sa += oa; sb += ob; }
  }
  if (lane == 63) { wtot[0][wv] = sa; wtot[1][wv] = sb; }
  __syncthreads();
  int pa = sa - a1, pb = sb - b1;                  // exclusive prefix inside the wave
#pragma unroll
  for (int w = 0; w < 16; ++w) { if (w < wv) { pa += wtot[0][w]; pb += wtot[1][w]; } }
  a0 += pa; a1 += pa; b0 += pb; b1 += pb;          // inclusive counts at positions i0, i1
  if (t == 1023) *nb_s = a1;                       // (padding positions add nothing)
  slab[i0] = __int_as_float(l0); slab[i1] = __int_as_float(l1);
  npos[i0] = (unsigned)b0; npos[i1] = (unsigned)b1;
  if (h0) hd[a0 - 1] = i0;
  if (h1) hd[a1 - 1] = i1;
  a[0] = a0; a[1] = a1; b[0] = b0; b[1] = b1;
}
// phase 4: one thread per bucket (buckets t, t + 1024, ...: B reaches n = 2048): the ordered sum of its terms
// (x + 0.0f == x: the non-positive items add nothing), its flags and its two quotients, stored for the fold.  The
// bucket's extent is known, so the loads run ahead of the adds.
template <class T>
__device__ __forceinline__ void mid_bucket_walk(int t, int B, const int* hd, const T* term, const float* slab,
                                                const unsigned* npos, T* bap, double* binv, int* bfl) {
  for (int bk = t; bk < B; bk += 1024) {
    const int head = hd[bk], end = hd[bk + 1];
    T apv = 0;
    int not_one = 0, zero = 0, first = -1;
    for (int p = head; p < end; p += 8) {
      T tv[8];
      int lv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = p + u < end ? p + u : end - 1;
        tv[u] = term[q]; lv[u] = __float_as_int(slab[q]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (p + u < end) {
          apv += tv[u];
          if (lv[u] == 1) { if (first < 0) first = p + u - head; }
          else { not_one = 1; if (lv[u] == 0) zero = 1; }
        }
      }
    }
    const int map_rank = (int)npos[end - 1] - (head ? (int)npos[head - 1] : 0);
    const int b_fl = rank_bucket_flags(map_rank, not_one, zero, first);
    bap[bk] = (b_fl & 1) ? apv / map_rank : (T)0;                                          // map_layer.cpp:92-94
    binv[bk] = (b_fl & 2) ? 1.0 / (first + 1) : 0.0;                                       // mrr_layer.cpp:75
    bfl[bk] = b_fl;
  }
}
// phase 5: the fold over the buckets in sorted (ascending group) order: one wave, 64 buckets per step
template <class T>
__device__ __forceinline__ void mid_fold(int lane, int B, const T* bap, const double* binv, const int* bfl,
                                         T* __restrict__ out0, T* __restrict__ out1, int* __restrict__ effective) {
  RankSums<T> s;
  for (int base = 0; base < B; base += 64) {
    const int bi = base + lane < B ? base + lane : B - 1;
    const T la = bap[bi];
    const double li = binv[bi];
    s.step(base + lane < B ? bfl[bi] : 0, la, [&](int l) { return wave_readlane(li, l); });
  }
  s.finish(lane, out0, out1, effective);
}
template <int MODE, class T>                         // 0: MAP / MRR, 1: AUC
__global__ __launch_bounds__(1024) void rank_mid_kernel(int n, int stride, int offset, int inner,
                                                        const T* __restrict__ prob, const T* __restrict__ label,
                                                        const T* __restrict__ group, int has_ignore, int ignore_label,
                                                        T* __restrict__ out0, T* __restrict__ out1,
                                                        int* __restrict__ effective) {
  __shared__ unsigned long long keys[kRankMid];
  __shared__ unsigned vals[kRankMid];
  __shared__ unsigned long long xk[kRankMid];          // the second exchange buffer of the merge rounds
  __shared__ unsigned xv[kRankMid];
  __shared__ T ap[MODE == 0 ? kRankMid : 1];
  __shared__ int rk[MODE == 0 ? kRankMid + 1 : 1];     // + 1: as `hd` it holds B + 1 <= 2049 bucket bounds
  __shared__ int fl[MODE == 0 ? kRankMid : 1];
  __shared__ float slab[MODE == 0 ? kRankMid : 1];     // labels as ints, position order
  __shared__ int wtot[2][16];
  __shared__ int nb_s;
  // What the metric part (MODE 0) keeps where.  Free once the sort is done: xk / xv, and ap / rk / fl until the walk.
  int* hd = rk;                                        // compacted bucket heads, hd[B] = n
  unsigned* npos = xv;                                 // inclusive counts of label == 1
  T* term = ap;
  // The walk reads hd / term / slab / npos only; what it stores for the fold aliases keys / xk / fl, which nothing
  // reads between the barrier before it and the one after it (the sorted keys are not needed any more).
  T* bap = reinterpret_cast<T*>(keys);
  double* binv = reinterpret_cast<double*>(xk);
  int* bfl = fl;
  const int t = threadIdx.x;
  MidItems it;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = 2 * t + e;
    it.k[e] = i < n ? rank_key(i, stride, offset, inner, prob, group) : ~0ull;   // padding sorts behind everything
    it.v[e] = (unsigned)i;
  }
  it = mid_merge_rounds(mid_sort_wave(it), keys, vals, xk, xv);
  if (MODE == 0) {
    // A lone workgroup runs at a fraction of the chip's loaded clock: rank_bucket_at's walks (a data-dependent exit and
    // a division per item) took 15.8 us at 1,517 items and rank_fold_wave with its double divisions 7.6 us
    // (profiles/r03_rank_mid_phases.txt).  Same expressions and summation orders, but all that is not a running fp sum
    // happens in parallel: heads, lengths and positive counts by workgroup scans, every term and every bucket's two
    // quotients by its own thread; what is left sequential is adds over loads whose addresses are known up front.
    int lab[2], a[2], b[2];
    mid_scan_heads(t, n, it.k, label, keys, vals, wtot, slab, npos, hd, &nb_s, lab, a, b);
    __syncthreads();
    const int B = nb_s;
    if (t == 0) hd[B] = n;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {                      // every positive's term: (++map_rank) / (float)(pos + 1), :84-86
      const int i = 2 * t + e, head = i < n ? hd[a[e] - 1] : 0;
      const int before = head ? (int)npos[head - 1] : 0;               // positives in front of the bucket
      if (i < n) term[i] = lab[e] == 1 ? (b[e] - before) / (T)(i - head + 1) : (T)0;
    }
    __syncthreads();
    mid_bucket_walk(t, B, hd, term, slab, npos, bap, binv, bfl);
    __syncthreads();
    if (t < 64) mid_fold(t, B, bap, binv, bfl, out0, out1, effective);
  } else if (t < 64) {
    auc_fold_wave(t, n, vals, label, has_ignore, ignore_label, out0);
  }
}
RankRoute rank_route(int n, bool libstd) {
  if (libstd || n <= 0 || n > kRankMid) return RankRoute::kRadix;
  return n <= kRankSmall ? RankRoute::kOneWgSmall : RankRoute::kOneWgMid;   // a mini-batch's / a test split's worth
}
template <class T>
int rank_onewg(RankRoute route, bool auc, int n, int stride, int offset, int inner, const T* prob, const T* label,
               const T* group, int has_ignore, int ignore_label, T* out0, T* out1, int* effective, hipStream_t s) {
  const bool small = route == RankRoute::kOneWgSmall;
  void (*const kernel)(int, int, int, int, const T*, const T*, const T*, int, int, T*, T*, int*) =
      auc ? (small ? rank_small_kernel<1, T> : rank_mid_kernel<1, T>)
          : (small ? rank_small_kernel<0, T> : rank_mid_kernel<0, T>);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(1024), 0, s, n, stride, offset, inner, prob, label, group, has_ignore,
                     ignore_label, out0, out1, effective);
  return launch_status();
}
template int rank_onewg<float>(RankRoute, bool, int, int, int, int, const float*, const float*, const float*, int, int,
                               float*, float*, int*, hipStream_t);
template int rank_onewg<double>(RankRoute, bool, int, int, int, int, const double*, const double*, const double*, int,
                                int, double*, double*, int*, hipStream_t);

}  // namespace mms
