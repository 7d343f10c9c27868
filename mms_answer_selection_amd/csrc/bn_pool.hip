// csrc/bn_pool.hip -- BN -> average pooling over windows that tile the map -> TanH as one call, and its extern "C" entry
// points (include/mms.h: mms_bn_pool_tanh_*), and the MAX form beside it (at the end of this comment).  The three layers
// restated are src/caffe/layers/bn_layer.cpp (csrc/bn.hip has the formulas), pooling_layer.cpp:197-212 / :291-317 (AVE;
// every window here has pool_size = kh*kw) and tanh_layer.cpp:13-33.  Pooling over disjoint windows is linear and BN
// is affine per channel, so with
// m = window_mean(x) (the window's elements added in (h, w) order, divided once by kh*kw), per channel c:
//
//   forward   mean, var, std, running blobs: as mms_bn_forward, from sum x and sum x*x over the channel
//             save_pool = (m + (-mean)) / std          the pooled normalised map, kept for the backward
//             top = tanh(save_pool * scale + shift)
//   backward  gp = top_diff * (1 - top*top);  shift_diff = sum gp;  scale_diff = sum gp*save_pool
//             a = scale*scale_diff;  b = scale*shift_diff;  xn = (x + (-mean)) / std;  g = gp / (kh*kw) * scale
//             dx = (g + (-1/(N H W)) * (xn*a + b)) / std          for every element of gp's window
//
// x is read once per pass and bottom_diff written once; everything else is pooled-size ((N, C, H/kh, W/kw)) or C-size.
//
// Order (fixed; no atomics).  A channel's windows, in (n, ph, pw) order, are numbered 0 .. N*P-1 (P = windows per map).
// A workgroup of T threads that owns windows [w0, w1) gives thread t the windows w0 + t, w0 + t + T, ...; the thread adds
// each window's elements in (h, w) order into its window sum and -- the same values, the same order -- into ONE
// accumulator for sum x and one for sum x*x (backward: gp and gp*save_pool of each of its windows).  The T accumulators
// are combined per wave and the waves in ascending order (bn_block_sum); chunk sums are folded in ascending chunk order
// by every workgroup that needs them (bn_fold).  A window row is read in 16-byte accesses where kw*sizeof(T) and
// W*sizeof(T) are multiples of 16 and x (and bottom_diff) are 16-byte aligned, element by element otherwise: the same
// elements in the same order, hence the same words.
//
// Two routes (bp_route, the one place that decides), with BN's threshold:
//   small  at most kBnSmallGroups 16-byte groups of x per channel: one launch per pass, one workgroup of 1024 per
//          channel.  Forward: sweep x (window means to save_pool, the two sums), then finish its own pooled elements.
//          Backward: the two sums over the pooled tensors, then the sweep x -> bottom_diff.
//   large  the channel's windows are cut into at most kBnMaxChunks chunks of whole windows, each at least
//          kBnChunkGroups groups of x.  Forward: launch 1, a grid of (channel, chunk) workgroups of 256, sweeps x and
//          leaves window means in save_pool and chunk sums in the workspace; launch 2 (pooled-size only) folds and
//          finishes save_pool and top.  Backward: launch 1 sums over the pooled tensors, launch 2 folds and sweeps.
// TEST-phase forward knows mean and var beforehand: the sweep finishes each window itself, one launch on either route.
//
// The MAX form (include/mms_bn_maxpool.h: mms_bn_maxpool_tanh_*; pooling_layer.cpp:149-170 / :269-287) is the same
// geometry, routes, walk, statistics and pooled-size sums with another thing kept per window.  Per channel BN's output
// bn_out(x) = ((x + (-mean)) / std)*scale + shift (bp_normalised, then bp_bn_out: the one place that forms it) is a
// chain of correctly rounded monotone operations, non-decreasing for scale >= 0 and non-increasing for scale < 0, so the
// largest BN output of a window is, word for word, bn_out(e) with e = the window's largest x (smallest for scale < 0;
// for scale == 0 every BN output is shift, and e is the window's first element, where the reference's mask is): the
// forward sweep keeps e where AVE keeps the sum (bp_keep), and everything after the sweep is AVE's with e in place
// of the mean.  The reference's mask -- the first element in (h, w) order whose BN output is strictly greater than
// every earlier one, i.e. the first that attains the maximum -- is not stored: the backward finds e again, then gives
// gp*scale to the first element whose bn_out equals bn_out(e), which is not arg-ext x where rounding made distinct x
// collapse.  The backward therefore reads shift, which AVE's does not.
#include <limits.h>

#include "bn_common.h"
#include "mms_bn_maxpool.h"
#include "mms_internal.h"

namespace mms {
namespace {

struct BpRoute {
  bool small;
  int chunks;                  // per channel
  unsigned windows_per_chunk;
};

struct BpGeom {
  unsigned C, H, W, kh, kw;
  unsigned PW, P;              // windows per map row, per map
  unsigned windows;            // N * P, the windows of one channel
};

// N < 0, a size below 1, windows that do not tile the map, or more elements than the reference's int index reaches
bool bp_bad_shape(int N, int C, int H, int W, int kh, int kw) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || kh > H || kw > W || H % kh || W % kw) return true;
  long long n = (long long)N * C;
  if (n > INT_MAX) return true;
  n *= H;
  return n > INT_MAX || n * W > INT_MAX;
}

// The one routing decision.  T: float or double; N >= 1 and a shape bp_bad_shape accepts.
template <typename T>
BpRoute bp_route(int N, int H, int W, int kh, int kw) {
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned ke = (unsigned)kh * (unsigned)kw;
  const unsigned total = (unsigned)N * (unsigned)H * (unsigned)W;
  const unsigned windows = total / ke;
  if ((total + V - 1) / V <= kBnSmallGroups) return {true, 1, windows};
  const unsigned least = (kBnChunkGroups * V + ke - 1) / ke;          // windows that hold kBnChunkGroups groups of x
  unsigned wpc = (windows + kBnMaxChunks - 1) / kBnMaxChunks;
  if (wpc < least) wpc = least;
  return {false, (int)((windows + wpc - 1) / wpc), wpc};
}

// Never below what the route uses (chunks <= kBnMaxChunks and chunks <= windows / least, rounded up), and monotone
// in N, which the chunk count itself is not.
template <typename T>
size_t bp_workspace_bytes(int N, int C, int H, int W, int kh, int kw) {
  if (bp_bad_shape(N, C, H, W, kh, kw) || N == 0) return 0;
  if (bp_route<T>(N, H, W, kh, kw).small) return 0;
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned ke = (unsigned)kh * (unsigned)kw;
  const unsigned least = (kBnChunkGroups * V + ke - 1) / ke;
  const unsigned windows = (unsigned)N * (unsigned)H * (unsigned)W / ke;
  unsigned bound = (windows + least - 1) / least;
  if (bound > (unsigned)kBnMaxChunks) bound = kBnMaxChunks;
  return (size_t)C * bound * kBnSlots * sizeof(T);
}

// Chunk k's share of the channel's windows.
__device__ __forceinline__ void bp_chunk(unsigned windows, unsigned wpc, unsigned k, unsigned* w0, unsigned* w1) {
  *w0 = k * wpc;                                  // k < chunks: k * wpc < windows
  *w1 = windows - *w0 < wpc ? windows : *w0 + wpc;
}

struct BpWin {
  size_t x0;     // the window's first element in x / bottom_diff
  size_t p;      // its element in top / top_diff / save_pool
};

__device__ __forceinline__ BpWin bp_window(const BpGeom& g, unsigned c, unsigned w) {
  const unsigned n = w / g.P, r = w - n * g.P, ph = r / g.PW, pw = r - ph * g.PW;
  const size_t plane = (size_t)n * g.C + c;
  return {(plane * g.H + (size_t)ph * g.kh) * g.W + (size_t)pw * g.kw, plane * g.P + r};
}

template <typename T, bool VEC>
__device__ __forceinline__ void bp_load(const T* p, T (&v)[VEC ? 16 / sizeof(T) : 1]) {
  if constexpr (VEC) {
    const bn_vec<T> t = *reinterpret_cast<const bn_vec<T>*>(p);
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); ++e) v[e] = t[e];
  } else {
    v[0] = *p;
  }
}

template <typename T, bool VEC>
__device__ __forceinline__ void bp_store(T* p, const T (&v)[VEC ? 16 / sizeof(T) : 1]) {
  if constexpr (VEC) {
    bn_vec<T> t;
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); ++e) t[e] = v[e];
    *reinterpret_cast<bn_vec<T>*>(p) = t;
  } else {
    *p = v[0];
  }
}

// f(offset from xw, values[E]) for each piece of the window at xw, in (h, w) order; a piece is E elements of one row:
// 16 bytes (VEC) or one element.  KH, KW > 0: the window's size at compile time (== g.kh, g.kw), every load of the
// window issued before the first value is used.  KH == KW == 0: any window, piece by piece.  With a second f the window
// is passed over again after the first pass is complete: from the registers that hold it the first way, read again
// the second.
template <typename T, bool VEC>
constexpr int bp_piece = VEC ? 16 / sizeof(T) : 1;

// One pass: over the held window v[KH][KW / E][E], or loading a run-time window (v unused).
template <typename T, bool VEC, int KH, int KW, class F>
__device__ __forceinline__ void bp_pass(const T* xw, const BpGeom& g,
                                        const T (*v)[KH ? KW / bp_piece<T, VEC> : 1][bp_piece<T, VEC>], F&& f) {
  constexpr int E = bp_piece<T, VEC>;
  if constexpr (KH > 0) {
#pragma unroll
    for (int i = 0; i < KH; ++i) {
#pragma unroll
      for (int j = 0; j < KW / E; ++j) f((size_t)i * g.W + j * E, v[i][j]);
    }
  } else {
    for (unsigned i = 0; i < g.kh; ++i) {
      for (unsigned j = 0; j < g.kw; j += E) {
        T w[E];
        bp_load<T, VEC>(xw + (size_t)i * g.W + j, w);
        f((size_t)i * g.W + j, w);
      }
    }
  }
}

template <typename T, bool VEC, int KH, int KW, class... F>
__device__ __forceinline__ void bp_walk(const T* xw, const BpGeom& g, F&&... f) {
  constexpr int E = VEC ? 16 / sizeof(T) : 1;
  if constexpr (KH > 0) {
    static_assert(KW % E == 0, "a row is whole pieces");
    T v[KH][KW / E][E];
#pragma unroll
    for (int i = 0; i < KH; ++i) {
#pragma unroll
      for (int j = 0; j < KW / E; ++j) bp_load<T, VEC>(xw + (size_t)i * g.W + j * E, v[i][j]);
    }
    (bp_pass<T, VEC, KH, KW>(xw, g, v, f), ...);
  } else {
    (bp_pass<T, VEC, KH, KW>(xw, g, nullptr, f), ...);
  }
}

// Window w of channel c in top / top_diff / save_pool (bp_window's p, without the division by PW).
__device__ __forceinline__ size_t bp_pooled_index(const BpGeom& g, unsigned c, unsigned w) {
  const unsigned n = w / g.P, r = w - n * g.P;
  return ((size_t)n * g.C + c) * g.P + r;
}

// TRAIN, after the sweep: windows [w0, w1) of channel c, whose means (MAX: extrema) are in save_pool, become save_pool
// and top.
template <typename T, int THREADS>
__device__ __forceinline__ void bp_finish(const BpGeom& g, unsigned c, unsigned w0, unsigned w1, T nmean, T std, T sc,
                                          T sh, T* save_pool, T* __restrict__ top) {
  for (unsigned w = w0 + threadIdx.x; w < w1; w += THREADS) {
    const size_t p = bp_pooled_index(g, c, w);
    T sp;
    const T t = bn_pool_train_finish(save_pool[p], nmean, std, sc, sh, &sp);
    save_pool[p] = sp;
    top[p] = t;
  }
}

// Forward sweep: the only launch of the small route and of the TEST phase, launch 1 of the large route's TRAIN phase.
// SMALL: grid (C, 1), 1024 threads; otherwise grid (C, chunks), 256 threads.  MAX: the window's extremum where AVE has
// its mean.
template <typename T, bool VEC, int KH, int KW, bool SMALL, bool MAX>
__global__ __launch_bounds__(SMALL ? kBnSmallThreads : kBnThreads) void bp_forward_kernel(
    const T* __restrict__ x, const T* __restrict__ scale, const T* __restrict__ shift, T* running_mean,
    T* running_var, T* __restrict__ top, T* save_pool, T* save_mean, T* save_std, T* __restrict__ ws, BpGeom g,
    unsigned wpc, int phase, T bn_memory, T inv_S, T inv_N) {
  constexpr int THREADS = SMALL ? kBnSmallThreads : kBnThreads;
  constexpr int E = VEC ? 16 / sizeof(T) : 1;
  __shared__ T red[2 * THREADS / kWave];
  const unsigned c = blockIdx.x;
  unsigned w0, w1;
  bp_chunk(g.windows, wpc, blockIdx.y, &w0, &w1);
  const bool writer = blockIdx.y == 0 && threadIdx.x == 0;
  const bool test = phase != 0;
  const T sc = scale[c], sh = shift[c], ke = T(g.kh * g.kw);
  const int dir = bp_dir(sc);
  T nmean = T(0), std = T(1);
  if (test) {
    const T mean = running_mean[c];
    nmean = -mean;
    std = bn_sqrt(running_var[c] + T(1e-9));
    if (writer) {
      save_mean[c] = mean;
      save_std[c] = std;
    }
  }
  T acc[2] = {T(0), T(0)};
  for (unsigned w = w0 + threadIdx.x; w < w1; w += THREADS) {
    const BpWin at = bp_window(g, c, w);
    T s = T(0);                                    // AVE: the window's sum; MAX: its extremum
    bp_walk<T, VEC, KH, KW>(x + at.x0, g, [&](size_t off, const T(&v)[E]) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if constexpr (MAX) bp_keep(off == 0 && e == 0, v[e], dir, &s);
        else s += v[e];
        acc[0] += v[e];
        acc[1] += v[e] * v[e];
      }
    });
    if (test) {
      T sp;
      const T t = MAX ? bn_maxpool_test_finish(s, nmean, std, sc, sh, &sp)
                      : bn_pool_test_finish(s, ke, nmean, std, sc, sh, &sp);
      save_pool[at.p] = sp;
      top[at.p] = t;
    } else {
      save_pool[at.p] = MAX ? s : s / ke;
    }
  }
  if (test) return;
  bn_block_sum<THREADS, 2>(acc, red);
  if constexpr (SMALL) {
    // the barrier inside bn_block_sum also orders this workgroup's save_pool writes before bp_finish's reads
    bn_statistics(acc, (int)c, writer, bn_memory, inv_S, inv_N, running_mean, running_var, save_mean, save_std, &nmean,
                  &std);
    bp_finish<T, THREADS>(g, c, w0, w1, nmean, std, sc, sh, save_pool, top);
  } else if (threadIdx.x == 0) {
    T* o = ws + ((size_t)c * gridDim.y + blockIdx.y) * kBnSlots;
    o[0] = acc[0];
    o[1] = acc[1];
  }
}

// Large route, TRAIN forward, launch 2: grid (C, chunks), 256 threads; pooled-size and C-size arrays only.
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bp_forward_finish_kernel(
    const T* __restrict__ scale, const T* __restrict__ shift, T* running_mean, T* running_var, T* __restrict__ top,
    T* save_pool, T* save_mean, T* save_std, const T* __restrict__ ws, BpGeom g, unsigned wpc, T bn_memory, T inv_S,
    T inv_N) {
  const unsigned c = blockIdx.x;
  unsigned w0, w1;
  bp_chunk(g.windows, wpc, blockIdx.y, &w0, &w1);
  T tot[2], nmean, std;
  bn_fold<2>(ws, (int)c, (int)gridDim.y, tot);
  bn_statistics(tot, (int)c, blockIdx.y == 0 && threadIdx.x == 0, bn_memory, inv_S, inv_N, running_mean, running_var,
                save_mean, save_std, &nmean, &std);
  bp_finish<T, kBnThreads>(g, c, w0, w1, nmean, std, scale[c], shift[c], save_pool, top);
}

// sum gp and sum gp*save_pool over windows [w0, w1) of channel c, reduced over the workgroup
template <typename T, int THREADS>
__device__ __forceinline__ void bp_backward_sums(const T* __restrict__ top, const T* __restrict__ top_diff,
                                                 const T* __restrict__ save_pool, const BpGeom& g, unsigned c,
                                                 unsigned w0, unsigned w1, T (&acc)[2], T* red) {
  acc[0] = acc[1] = T(0);
  for (unsigned w = w0 + threadIdx.x; w < w1; w += THREADS) {
    const size_t p = bp_pooled_index(g, c, w);
    const T t = top[p];
    const T gp = top_diff[p] * (T(1) - t * t);
    acc[0] += gp;
    acc[1] += gp * save_pool[p];
  }
  bn_block_sum<THREADS, 2>(acc, red);
}

// Large route, backward, launch 1: grid (C, chunks), 256 threads; slots 0, 1 = sum gp, sum gp*save_pool.
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bp_backward_partial_kernel(const T* __restrict__ top,
                                                                         const T* __restrict__ top_diff,
                                                                         const T* __restrict__ save_pool,
                                                                         T* __restrict__ ws, BpGeom g, unsigned wpc) {
  __shared__ T red[2 * kBnThreads / kWave];
  const unsigned c = blockIdx.x;
  unsigned w0, w1;
  bp_chunk(g.windows, wpc, blockIdx.y, &w0, &w1);
  T acc[2];
  bp_backward_sums<T, kBnThreads>(top, top_diff, save_pool, g, c, w0, w1, acc, red);
  if (threadIdx.x == 0) {
    T* o = ws + ((size_t)c * gridDim.y + blockIdx.y) * kBnSlots;
    o[0] = acc[0];
    o[1] = acc[1];
  }
}

// Backward: the only launch of the small route (grid (C, 1), 1024 threads, the workgroup sums its own channel) and
// launch 2 of the large route (grid (C, chunks), 256 threads, the sums come from the workspace).  scale_diff, shift_diff
// and dx may each be NULL; with dx NULL the large route launches one workgroup per channel, which only folds.
// The body of both pooling methods' kernels; shift is read by MAX only.
template <typename T, bool VEC, int KH, int KW, bool SMALL, bool MAX>
__device__ __forceinline__ void bp_backward_sweep(
    const T* __restrict__ x, const T* __restrict__ top, const T* __restrict__ top_diff,
    const T* __restrict__ save_pool, const T* __restrict__ scale, const T* __restrict__ shift,
    const T* __restrict__ save_mean, const T* __restrict__ save_std, T* __restrict__ dx, T* __restrict__ scale_diff,
    T* __restrict__ shift_diff, const T* __restrict__ ws, const BpGeom& g, unsigned wpc, int chunks,
    T minus_inv_count) {
  constexpr int THREADS = SMALL ? kBnSmallThreads : kBnThreads;
  constexpr int E = VEC ? 16 / sizeof(T) : 1;
  __shared__ T red[2 * THREADS / kWave];
  const unsigned c = blockIdx.x;
  unsigned w0, w1;
  bp_chunk(g.windows, wpc, blockIdx.y, &w0, &w1);
  const T nmean = -save_mean[c], std = save_std[c], sc = scale[c], ke = T(g.kh * g.kw);
  T sh = T(0);
  if constexpr (MAX) sh = shift[c];
  const int dir = bp_dir(sc);
  T tot[2];
  if constexpr (SMALL) bp_backward_sums<T, THREADS>(top, top_diff, save_pool, g, c, w0, w1, tot, red);
  else bn_fold<2>(ws, (int)c, chunks, tot);
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    if (shift_diff) shift_diff[c] = tot[0];
    if (scale_diff) scale_diff[c] = tot[1];
  }
  if (!dx) return;
  const T b = sc * tot[0], a = sc * tot[1];
  for (unsigned w = w0 + threadIdx.x; w < w1; w += THREADS) {
    const BpWin at = bp_window(g, c, w);
    const T t = top[at.p];
    const T gp = top_diff[at.p] * (T(1) - t * t);
    if constexpr (MAX) {
      // The mask again: the window's extremum as the forward kept it, its BN output, then the first element whose BN
      // output is that word receives the pooling's top_diff (BN's dy * scale of it); every other element has dy == 0.
      const T gs = gp * sc;
      T* out = dx + at.x0;
      T ext = T(0), ymax = T(0);
      bool open = true;                            // no element of the window has had ymax yet
      bp_walk<T, VEC, KH, KW>(
          x + at.x0, g,
          [&](size_t off, const T(&v)[E]) {
#pragma unroll
            for (int e = 0; e < E; ++e) bp_keep(off == 0 && e == 0, v[e], dir, &ext);
          },
          [&](size_t off, const T(&v)[E]) {
            if (off == 0) ymax = bp_bn_out(bp_normalised(ext, nmean, std), sc, sh);
            T o[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const T xn = bp_normalised(v[e], nmean, std);
              const bool same = bp_bn_out(xn, sc, sh) == ymax, hit = open & same;
              open = open & !same;
              o[e] = ((hit ? gs : T(0)) + minus_inv_count * (xn * a + b)) / std;
            }
            bp_store<T, VEC>(out + off, o);
          });
    } else {
      const T gs = gp / ke * sc;                 // the pooling's top_diff / pool_size, then BN's dy * scale
      T* out = dx + at.x0;
      bp_walk<T, VEC, KH, KW>(x + at.x0, g, [&](size_t off, const T(&v)[E]) {
        T o[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const T xn = (v[e] + nmean) / std;
          o[e] = (gs + minus_inv_count * (xn * a + b)) / std;
        }
        bp_store<T, VEC>(out + off, o);
      });
    }
  }
}

template <typename T, bool VEC, int KH, int KW, bool SMALL>
__global__ __launch_bounds__(SMALL ? kBnSmallThreads : kBnThreads) void bp_backward_kernel(
    const T* __restrict__ x, const T* __restrict__ top, const T* __restrict__ top_diff,
    const T* __restrict__ save_pool, const T* __restrict__ scale, const T* __restrict__ save_mean,
    const T* __restrict__ save_std, T* __restrict__ dx, T* __restrict__ scale_diff, T* __restrict__ shift_diff,
    const T* __restrict__ ws, BpGeom g, unsigned wpc, int chunks, T minus_inv_count) {
  bp_backward_sweep<T, VEC, KH, KW, SMALL, false>(x, top, top_diff, save_pool, scale, nullptr, save_mean, save_std, dx,
                                                  scale_diff, shift_diff, ws, g, wpc, chunks, minus_inv_count);
}

template <typename T, bool VEC, int KH, int KW, bool SMALL>
__global__ __launch_bounds__(SMALL ? kBnSmallThreads : kBnThreads) void bp_max_backward_kernel(
    const T* __restrict__ x, const T* __restrict__ top, const T* __restrict__ top_diff,
    const T* __restrict__ save_pool, const T* __restrict__ scale, const T* __restrict__ shift,
    const T* __restrict__ save_mean, const T* __restrict__ save_std, T* __restrict__ dx, T* __restrict__ scale_diff,
    T* __restrict__ shift_diff, const T* __restrict__ ws, BpGeom g, unsigned wpc, int chunks, T minus_inv_count) {
  bp_backward_sweep<T, VEC, KH, KW, SMALL, true>(x, top, top_diff, save_pool, scale, shift, save_mean, save_std, dx,
                                                 scale_diff, shift_diff, ws, g, wpc, chunks, minus_inv_count);
}

// A window row is whole 16-byte accesses: kw elements are, every row starts on a 16-byte boundary (W elements are, and
// so are the maps), and the arrays the sweep touches are aligned.
template <typename T>
bool bp_vector_ok(int W, int kw, const void* a, const void* b) {
  constexpr int V = 16 / sizeof(T);
  return kw % V == 0 && W % V == 0 && aligned16(a) && aligned16(b);
}

template <int K>
using bp_int = std::integral_constant<int, K>;

// f(VEC, KH, KW) as types: network_v4's two windows at compile time (4 x 4 where its rows are 16-byte accesses; 5 x 5's
// 100-byte rows never are), any other window at run time.  They are network_v3's too; MAX adds network_v5's 2 x 2 and
// 6 x 6, whose rows are 16-byte accesses in double only.
template <typename T, bool MAX, class F>
void bp_dispatch(bool vec, int kh, int kw, F&& f) {
  if (vec && kh == 4 && kw == 4) return f(std::true_type{}, bp_int<4>{}, bp_int<4>{});
  if (!vec && kh == 5 && kw == 5) return f(std::false_type{}, bp_int<5>{}, bp_int<5>{});
  if constexpr (MAX) {
    if (kh == kw && (kh == 2 || kh == 6)) {
      auto square = [&](auto K) {
        if constexpr (decltype(K)::value * sizeof(T) % 16 == 0) {      // bp_vector_ok: vec is false everywhere else
          if (vec) return f(std::true_type{}, K, K);
        }
        f(std::false_type{}, K, K);
      };
      return kh == 2 ? square(bp_int<2>{}) : square(bp_int<6>{});
    }
  }
  with_bool(vec, [&](auto VEC) { f(VEC, bp_int<0>{}, bp_int<0>{}); });
}

BpGeom bp_geom(int N, int C, int H, int W, int kh, int kw) {
  const unsigned PW = (unsigned)(W / kw), P = (unsigned)(H / kh) * PW;
  return {(unsigned)C, (unsigned)H, (unsigned)W, (unsigned)kh, (unsigned)kw, PW, P, (unsigned)N * P};
}

// MAX: the pooling method, here and in bp_backward; the argument rules are one list for both.
template <typename T, bool MAX>
int bp_forward(int phase, int N, int C, int H, int W, int kh, int kw, T bn_memory, const T* x, const T* scale,
               const T* shift, T* running_mean, T* running_var, T* top, T* save_pool, T* save_mean, T* save_std,
               void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (bp_bad_shape(N, C, H, W, kh, kw) || (phase != 0 && phase != 1)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !scale || !shift || !running_mean || !running_var || !top || !save_pool || !save_mean || !save_std)
    return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, scale, shift, running_mean, running_var};
  const void* const outputs[] = {top, save_pool};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  const BpRoute r = bp_route<T>(N, H, W, kh, kw);
  const size_t need = bp_workspace_bytes<T>(N, C, H, W, kh, kw);
  if (need && phase == 0 && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  T* ws = static_cast<T*>(workspace);
  const BpGeom g = bp_geom(N, C, H, W, kh, kw);
  const T inv_S = T(1. / ((double)H * W)), inv_N = T(1. / N);
  const dim3 grid((unsigned)C, (unsigned)r.chunks);
  int rc = MMS_OK;
  bp_dispatch<T, MAX>(bp_vector_ok<T>(W, kw, x, nullptr), kh, kw, [&](auto VEC, auto KH, auto KW) {
    constexpr bool V = decltype(VEC)::value;
    constexpr int kH = decltype(KH)::value, kW = decltype(KW)::value;
    if (r.small) {
      hipLaunchKernelGGL((bp_forward_kernel<T, V, kH, kW, true, MAX>), grid, dim3(kBnSmallThreads), 0, s, x, scale, shift,
                         running_mean, running_var, top, save_pool, save_mean, save_std, (T*)nullptr, g,
                         r.windows_per_chunk, phase, bn_memory, inv_S, inv_N);
      return;
    }
    hipLaunchKernelGGL((bp_forward_kernel<T, V, kH, kW, false, MAX>), grid, dim3(kBnThreads), 0, s, x, scale, shift,
                       running_mean, running_var, top, save_pool, save_mean, save_std, ws, g, r.windows_per_chunk,
                       phase, bn_memory, inv_S, inv_N);
  });
  if ((rc = launch_status()) != MMS_OK || r.small || phase != 0) return rc;
  hipLaunchKernelGGL((bp_forward_finish_kernel<T>), grid, dim3(kBnThreads), 0, s, scale, shift, running_mean,
                     running_var, top, save_pool, save_mean, save_std, (const T*)ws, g, r.windows_per_chunk, bn_memory,
                     inv_S, inv_N);
  return launch_status();
}

// shift: an input of the MAX form only (the mask is found from BN's output); AVE passes none.
template <typename T, bool MAX>
int bp_backward(int N, int C, int H, int W, int kh, int kw, const T* x, const T* top, const T* top_diff,
                const T* save_pool, const T* scale, const T* shift, const T* save_mean, const T* save_std,
                T* bottom_diff, T* scale_diff, T* shift_diff, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (bp_bad_shape(N, C, H, W, kh, kw)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!x || !top || !top_diff || !save_pool || !scale || (MAX && !shift) || !save_mean || !save_std ||
      (!bottom_diff && !scale_diff && !shift_diff))
    return MMS_ERR_INVALID_ARG;
  const void* const inputs[] = {x, top, top_diff, save_pool, scale, save_mean, save_std, MAX ? shift : nullptr};
  const void* const outputs[] = {bottom_diff};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  const BpRoute r = bp_route<T>(N, H, W, kh, kw);
  const size_t need = bp_workspace_bytes<T>(N, C, H, W, kh, kw);
  if (need && (!workspace || workspace_bytes < need)) return MMS_ERR_WORKSPACE;
  T* ws = static_cast<T*>(workspace);
  const BpGeom g = bp_geom(N, C, H, W, kh, kw);
  const T minus_inv_count = T(-1. / ((double)N * H * W));
  const dim3 grid((unsigned)C, (unsigned)r.chunks);
  if (!r.small) {
    hipLaunchKernelGGL((bp_backward_partial_kernel<T>), grid, dim3(kBnThreads), 0, s, top, top_diff, save_pool, ws, g,
                       r.windows_per_chunk);
    const int rc = launch_status();
    if (rc != MMS_OK) return rc;
  }
  bp_dispatch<T, MAX>(bp_vector_ok<T>(W, kw, x, bottom_diff), kh, kw, [&](auto VEC, auto KH, auto KW) {
    constexpr bool V = decltype(VEC)::value;
    constexpr int kH = decltype(KH)::value, kW = decltype(KW)::value;
    with_bool(r.small, [&](auto SMALL) {
      constexpr bool S = decltype(SMALL)::value;
      const dim3 gr = S || bottom_diff ? grid : dim3((unsigned)C), threads(S ? kBnSmallThreads : kBnThreads);
      const T* sums = S ? nullptr : ws;
      if constexpr (MAX) {
        hipLaunchKernelGGL((bp_max_backward_kernel<T, V, kH, kW, S>), gr, threads, 0, s, x, top, top_diff, save_pool,
                           scale, shift, save_mean, save_std, bottom_diff, scale_diff, shift_diff, sums, g,
                           r.windows_per_chunk, r.chunks, minus_inv_count);
      } else {
        hipLaunchKernelGGL((bp_backward_kernel<T, V, kH, kW, S>), gr, threads, 0, s, x, top, top_diff, save_pool, scale,
                           save_mean, save_std, bottom_diff, scale_diff, shift_diff, sums, g, r.windows_per_chunk,
                           r.chunks, minus_inv_count);
      }
    });
  });
  return launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

size_t mms_bn_pool_tanh_workspace_bytes(int N, int C, int H, int W, int kh, int kw) {
  return bp_workspace_bytes<float>(N, C, H, W, kh, kw);
}
size_t mms_bn_pool_tanh_workspace_bytes_f64(int N, int C, int H, int W, int kh, int kw) {
  return bp_workspace_bytes<double>(N, C, H, W, kh, kw);
}

int mms_bn_pool_tanh_forward_f32(int phase, int N, int C, int H, int W, int kh, int kw, float bn_memory,
                                 const float* x, const float* scale, const float* shift, float* running_mean,
                                 float* running_var, float* top, float* save_pool, float* save_mean, float* save_std,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return bp_forward<float, false>(phase, N, C, H, W, kh, kw, bn_memory, x, scale, shift, running_mean, running_var, top,
                           save_pool, save_mean, save_std, workspace, workspace_bytes,
                           as_stream(stream));
}

int mms_bn_pool_tanh_backward_f32(int N, int C, int H, int W, int kh, int kw, const float* x, const float* top,
                                  const float* top_diff, const float* save_pool, const float* scale,
                                  const float* save_mean, const float* save_std, float* bottom_diff, float* scale_diff,
                                  float* shift_diff, void* workspace, size_t workspace_bytes, void* stream) {
  return bp_backward<float, false>(N, C, H, W, kh, kw, x, top, top_diff, save_pool, scale, nullptr, save_mean, save_std,
                                   bottom_diff, scale_diff, shift_diff, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_pool_tanh_forward_f64(int phase, int N, int C, int H, int W, int kh, int kw, double bn_memory,
                                 const double* x, const double* scale, const double* shift, double* running_mean,
                                 double* running_var, double* top, double* save_pool, double* save_mean,
                                 double* save_std, void* workspace, size_t workspace_bytes, void* stream) {
  return bp_forward<double, false>(phase, N, C, H, W, kh, kw, bn_memory, x, scale, shift, running_mean, running_var, top,
                            save_pool, save_mean, save_std, workspace, workspace_bytes,
                            as_stream(stream));
}

int mms_bn_pool_tanh_backward_f64(int N, int C, int H, int W, int kh, int kw, const double* x, const double* top,
                                  const double* top_diff, const double* save_pool, const double* scale,
                                  const double* save_mean, const double* save_std, double* bottom_diff,
                                  double* scale_diff, double* shift_diff, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return bp_backward<double, false>(N, C, H, W, kh, kw, x, top, top_diff, save_pool, scale, nullptr, save_mean,
                                    save_std, bottom_diff, scale_diff, shift_diff, workspace, workspace_bytes,
                                    as_stream(stream));
}

// include/mms_bn_maxpool.h: the MAX form.  The workspace is AVE's: the route and the chunk sums are.
size_t mms_bn_maxpool_tanh_workspace_bytes(int N, int C, int H, int W, int kh, int kw) {
  return bp_workspace_bytes<float>(N, C, H, W, kh, kw);
}
size_t mms_bn_maxpool_tanh_workspace_bytes_f64(int N, int C, int H, int W, int kh, int kw) {
  return bp_workspace_bytes<double>(N, C, H, W, kh, kw);
}

int mms_bn_maxpool_tanh_forward_f32(int phase, int N, int C, int H, int W, int kh, int kw, float bn_memory,
                                    const float* x, const float* scale, const float* shift, float* running_mean,
                                    float* running_var, float* top, float* save_pool, float* save_mean,
                                    float* save_std, void* workspace, size_t workspace_bytes, void* stream) {
  return bp_forward<float, true>(phase, N, C, H, W, kh, kw, bn_memory, x, scale, shift, running_mean, running_var, top,
                                 save_pool, save_mean, save_std, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_maxpool_tanh_backward_f32(int N, int C, int H, int W, int kh, int kw, const float* x, const float* top,
                                     const float* top_diff, const float* save_pool, const float* scale,
                                     const float* shift, const float* save_mean, const float* save_std,
                                     float* bottom_diff, float* scale_diff, float* shift_diff, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return bp_backward<float, true>(N, C, H, W, kh, kw, x, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                                  bottom_diff, scale_diff, shift_diff, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_maxpool_tanh_forward_f64(int phase, int N, int C, int H, int W, int kh, int kw, double bn_memory,
                                    const double* x, const double* scale, const double* shift, double* running_mean,
                                    double* running_var, double* top, double* save_pool, double* save_mean,
                                    double* save_std, void* workspace, size_t workspace_bytes, void* stream) {
  return bp_forward<double, true>(phase, N, C, H, W, kh, kw, bn_memory, x, scale, shift, running_mean, running_var, top,
                                  save_pool, save_mean, save_std, workspace, workspace_bytes, as_stream(stream));
}

int mms_bn_maxpool_tanh_backward_f64(int N, int C, int H, int W, int kh, int kw, const double* x, const double* top,
                                     const double* top_diff, const double* save_pool, const double* scale,
                                     const double* shift, const double* save_mean, const double* save_std,
                                     double* bottom_diff, double* scale_diff, double* shift_diff, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return bp_backward<double, true>(N, C, H, W, kh, kw, x, top, top_diff, save_pool, scale, shift, save_mean, save_std,
                                   bottom_diff, scale_diff, shift_diff, workspace, workspace_bytes, as_stream(stream));
}

}  // extern "C"
