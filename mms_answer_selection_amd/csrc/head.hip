// csrc/head.hip -- network_v4's classifier head (do_trec_qa_clean.py:452-498): Concat -> InnerProduct -> TanH (in
// place) -> Dropout -> InnerProduct -> SoftmaxWithLoss / Softmax, one call per pass, and its extern "C" entry points
// (include/mms_head.h: mms_head_*).  The reference issues some fifteen BLAS and elementwise calls each way; here, with
// F = F0 + F1, feat = [x0 | x1], d = Dropout(h) and coef = loss_weight / max(1, normalizer):
//
//   forward   h[n,j]    = tanh(sum_f feat[n,f] w1[j,f] + b1[j])
//             prob[n,:] = softmax(sum_j d[n,j] w2[:,j] + b2)          loss = -sum_n log(max(prob[n,label_n], FLT_MIN)) / normalizer
//   backward  dz2[n,c]  = (prob[n,c] - [c == label_n]) coef, 0 for an ignored n
//             dz1[n,j]  = Dropout'(sum_c dz2[n,c] w2[c,j]) (1 - h[n,j]^2)
//             w2_diff  += dz2^T d    b2_diff += sum_n dz2    w1_diff += dz1^T feat    b1_diff += sum_n dz1    x_diff = dz1 w1
//
// The sample range is cut into tiles of kHeadTileSamples and the tiles are dealt in ascending runs to slabs
// (head_slabs): one slab up to kHeadSingleSamples samples, else at most kHeadMaxSlabs.  Both routes use the same cut.
// Workspace: [int count[kHeadMaxSlabs]] [T loss[kHeadMaxSlabs], 8 bytes each] [T coef] [T part[slabs][P]] with
// P = H F + H + C H + C, the parameter diffs in the order w1, b1, w2, b2.
//
// Two routes (mms_head_route, the one place that decides):
//
//   generic  kernels <T>, one thread per output element (h, x_diff, a slab's partial of a parameter diff) or per sample
//            (fc2, softmax, the loss term); every sum in ascending index order.  The backward recomputes dz2 and dz1
//            where it needs them, so nothing of size N goes to the workspace.  All of double, and float past the limits.
//            Launches: forward 2 (+1 for a loss), backward 2 + 2 (coef, x_diff, slab partials, finish).
//   fast     float, F <= kHeadMaxFeatures, H <= kHeadMaxHidden, C <= kHeadMaxClasses.  A workgroup of four waves stages
//            w1, w2 and the biases in LDS once and walks its slab's tiles; wave w owns samples 16 w .. 16 w + 15 of a tile.
//            Forward: the tile's feat rows are staged in LDS, zero-padded to a multiple of four columns (the x0 | x1
//            seam may fall inside a K step; nothing is read past a row); fc1 is v_mfma_f32_16x16x4_f32 with samples as
//            rows and 16 hidden units as columns; tanh and Dropout are applied to the accumulators, h goes to memory
//            and d to LDS; fc2 is VALU, lane (sample, c mod 4); the softmax and the loss term are one lane per sample.
//            A tile's 64 loss terms are added by a fixed butterfly of wave 0, the tiles in ascending order.
//            Backward: dz2 of the tile to LDS; one pass over the tile's (sample, j) elements gives d and dz1; then, all
//            from LDS, w2_diff / b2_diff / b1_diff on the VALU in ascending sample order, dz1^T feat on the matrix pipe
//            (rows hidden units, columns 16 features, the sum over the tile's samples; a wave keeps up to eight 16 x 16
//            accumulators across its slab's tiles) and dz1 w1 (rows samples, columns 16 features) into x0_diff | x1_diff.
//            One slab: the workgroup finishes the loss / adds its sums into the diffs itself -- one launch.  Otherwise
//            the slab partials go to the workspace and head_loss_finish_kernel / head_param_finish_kernel add them in
//            ascending order -- two launches.  The VALID count of the backward is an integer sum each workgroup takes
//            over all labels itself, so coef needs no launch of its own.
//            LDS strides: an operand read as [row = lane & 15][k = lane >> 4] has a stride of 2 mod 4 floats, so that the
//            32 lanes of a ds_read_b32 group fall on 32 banks; one read as [k][column = lane & 15] has 16 mod 32.
//
// z1, d, z2 and dz1 never go to memory on the fast route.  Nothing is read 16 bytes at a time, so alignment cannot
// change an order; every workspace word that is read has been written by this call.
//
// head_loss_from_terms (declared in csrc/mms_internal.h) is for the fused tails, csrc/score_tail.hip and
// csrc/train_tail.hip, whose kernels run csrc/head_tile.h's steps themselves: the loss from each sample's term.
#include "head_tile.h"
#include "mms_head.h"
#include "mms_internal.h"

namespace mms {
namespace {

constexpr int kHeadTileSamples = 64;       // samples of a tile: 16 per wave
constexpr int kHeadSingleSamples = 256;    // up to here one workgroup walks every tile: one launch per pass
constexpr int kHeadMaxSlabs = 256;         // one workgroup per CU
constexpr int kHeadMaxFeatures = 128;      // fast route: F0 + F1, eight column tiles of 16
constexpr int kHeadMaxHidden = 64;         // fast route: H, four tiles of 16
constexpr int kHeadMaxClasses = 16;        // fast route: C; C H <= 4 elements of w2_diff per thread
constexpr int kHeadHeaderBytes = 3088;     // count[256], loss[256] (8 bytes each), coef (16 bytes)
// The tile and the three limits are csrc/head_tile.h's, which the fast plan and the forward's steps are written
// against; they stay named here, where the backward kernel and the tests' model of the route read them.
static_assert(kHeadTileSamples == kHeadFastSamples && kHeadMaxFeatures == kHeadFastFeatures &&
                  kHeadMaxHidden == kHeadFastHidden && kHeadMaxClasses == kHeadFastClasses,
              "csrc/head_tile.h states the same tile and limits");

template <typename T>
struct HeadArgs {
  HeadDims d;
  T scale, loss_weight;
  const T *x0, *x1, *w1, *b1, *w2, *b2, *label, *h_in, *prob_in;
  const unsigned* mask;
  T *h, *prob, *loss;
  T *x0d, *x1d, *w1d, *b1d, *w2d, *b2d;
  int* counts;       // [kHeadMaxSlabs]
  T* lossp;          // [kHeadMaxSlabs]
  T* coef;           // [1]
  T* part;           // [slabs][P]
  int slabs, tps;    // head_slabs
};

inline int head_params(const HeadDims& d) { return d.H * d.F + d.H + d.C * d.H + d.C; }

// slabs, and *tps tiles per slab
int head_slabs(int N, int* tps) {
  const int tiles = (N + kHeadTileSamples - 1) / kHeadTileSamples;
  if (N <= kHeadSingleSamples) {
    *tps = tiles;
    return 1;
  }
  const int want = tiles < kHeadMaxSlabs ? tiles : kHeadMaxSlabs;
  *tps = (tiles + want - 1) / want;
  return (tiles + *tps - 1) / *tps;
}

// ---- what both routes compute with ----------------------------------------------------------------------------------
template <typename T>
__device__ inline T head_feat(const HeadArgs<T>& a, int n, int f) {
  return f < a.d.F0 ? a.x0[(size_t)n * a.d.F0 + f] : a.x1[(size_t)n * a.d.F1 + (f - a.d.F0)];
}

// the class of sample n, or -1: ignored (the ignore label, or outside [0, C))
template <typename T>
__device__ inline int head_label(const HeadArgs<T>& a, int n) {
  return head_class(a.d, a.label[n]);
}

template <typename T>
__device__ inline T head_dz2(const HeadArgs<T>& a, int n, int c, int lv, T coef) {
  return lv < 0 ? T(0) : (a.prob_in[(size_t)n * a.d.C + c] - (c == lv ? T(1) : T(0))) * coef;
}

// d[n,j] and dz1[n,j] from dd = sum_c dz2[n,c] w2[c,j]
template <typename T>
__device__ inline void head_hidden(const HeadArgs<T>& a, int n, int j, T dd, T* dval, T* dz1) {
  const T hv = a.h_in[(size_t)n * a.d.H + j];
  T dh = dd;
  *dval = hv;
  if (a.d.train) {
    const T m = T(a.mask[(size_t)n * a.d.H + j]);
    *dval = (hv * m) * a.scale;
    dh = (dd * m) * a.scale;
  }
  *dz1 = dh * (T(1) - hv * hv);
}

// ---- generic route --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_fc1_kernel(HeadArgs<T> a, int total) {
  const int idx = blockIdx.x * kHeadThreads + threadIdx.x;
  if (idx >= total) return;
  const int n = idx / a.d.H, j = idx - n * a.d.H;
  const T* wj = a.w1 + (size_t)j * a.d.F;
  T acc = T(0);
  for (int f = 0; f < a.d.F; ++f) acc += head_feat(a, n, f) * wj[f];
  if (a.b1) acc += a.b1[j];
  a.h[idx] = tanh(acc);
}

// fixed tree over the workgroup's 256 values: red[t] += red[t + s], s = 128, 64, .. 1
template <typename V>
__device__ inline V head_block_sum(V* red, V mine) {
  red[threadIdx.x] = mine;
  __syncthreads();
  for (int s = kHeadThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const V out = red[0];
  __syncthreads();
  return out;
}

// workgroup = slab; a thread walks the slab's samples t, t + 256, ... and writes z2, then exp, then prob in place
template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_out_kernel(HeadArgs<T> a) {
  __shared__ T red[kHeadThreads];
  __shared__ int redc[kHeadThreads];
  const HeadDims& d = a.d;
  const int per = a.tps * kHeadTileSamples;
  const int n0 = blockIdx.x * per, n1 = min(d.N, n0 + per);
  T mine = T(0);
  int cnt = 0;
  for (int n = n0 + threadIdx.x; n < n1; n += kHeadThreads) {
    T* pr = a.prob + (size_t)n * d.C;
    const T* hr = a.h + (size_t)n * d.H;
    T mx = T(0);
    for (int c = 0; c < d.C; ++c) {
      const T* wc = a.w2 + (size_t)c * d.H;
      T z = T(0);
      for (int j = 0; j < d.H; ++j) {
        const T dv = d.train ? (hr[j] * T(a.mask[(size_t)n * d.H + j])) * a.scale : hr[j];
        z += dv * wc[j];
      }
      if (a.b2) z += a.b2[c];
      pr[c] = z;
      mx = (c == 0 || z > mx) ? z : mx;
    }
    T sum = T(0);
    for (int c = 0; c < d.C; ++c) {
      const T e = exp(pr[c] - mx);
      pr[c] = e;
      sum += e;
    }
    for (int c = 0; c < d.C; ++c) pr[c] = pr[c] / sum;
    if (a.label) {
      const int lv = head_label(a, n);
      if (lv >= 0) {
        mine += head_loss_term(pr[lv]);
        ++cnt;
      }
    }
  }
  if (!a.loss) return;                     // uniform
  const T tot = head_block_sum(red, mine);
  const int tc = head_block_sum(redc, cnt);
  if (threadIdx.x == 0) {
    a.lossp[blockIdx.x] = tot;
    a.counts[blockIdx.x] = tc;
  }
}

// both routes: loss = (slab 0 + slab 1 + ...) / max(1, normalizer)
template <typename T>
__global__ void head_loss_finish_kernel(HeadArgs<T> a) {
  if (threadIdx.x || blockIdx.x) return;
  T s = a.lossp[0];
  int c = a.counts[0];
  for (int k = 1; k < a.slabs; ++k) {
    s += a.lossp[k];
    c += a.counts[k];
  }
  *a.loss = s / head_normalizer<T>(a.d, c);
}

// the fused tails (head_loss_from_terms): loss = (term 0 + term 1 + ...) / max(1, normalizer), n ascending
__global__ void head_loss_from_terms_kernel(const float* terms, const int* valid, HeadDims d, float* loss) {
  if (threadIdx.x || blockIdx.x) return;
  float sum = terms[0];
  int c = valid[0];
  for (int n = 1; n < d.N; ++n) {
    sum += terms[n];
    c += valid[n];
  }
  *loss = sum / head_normalizer<float>(d, c);
}

template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_coef_kernel(HeadArgs<T> a) {
  __shared__ int redc[kHeadThreads];
  int cnt = 0;
  for (int n = threadIdx.x; n < a.d.N; n += kHeadThreads) cnt += head_label(a, n) >= 0;
  const int tc = head_block_sum(redc, cnt);
  if (threadIdx.x == 0) *a.coef = a.loss_weight / head_normalizer<T>(a.d, tc);
}

template <typename T>
__device__ inline T head_dz1_direct(const HeadArgs<T>& a, int n, int j, int lv, T coef, T* dval) {
  T dd = T(0);
  for (int c = 0; c < a.d.C; ++c) dd += head_dz2(a, n, c, lv, coef) * a.w2[(size_t)c * a.d.H + j];
  T z;
  head_hidden(a, n, j, dd, dval, &z);
  return z;
}

template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_xdiff_kernel(HeadArgs<T> a, int total) {
  const int idx = blockIdx.x * kHeadThreads + threadIdx.x;
  if (idx >= total) return;
  const HeadDims& d = a.d;
  const int n = idx / d.F, f = idx - n * d.F;
  T* out = f < d.F0 ? (a.x0d ? a.x0d + (size_t)n * d.F0 + f : nullptr)
                    : (a.x1d ? a.x1d + (size_t)n * d.F1 + (f - d.F0) : nullptr);
  if (!out) return;
  const T coef = *a.coef;
  const int lv = head_label(a, n);
  T acc = T(0), dv;
  for (int j = 0; j < d.H; ++j) acc += head_dz1_direct(a, n, j, lv, coef, &dv) * a.w1[(size_t)j * d.F + f];
  *out = acc;
}

// slab blockIdx.y, element e of (w1 | b1 | w2 | b2): the sum over the slab's samples, ascending
template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_param_kernel(HeadArgs<T> a, int P) {
  const int e = blockIdx.x * kHeadThreads + threadIdx.x;
  if (e >= P) return;
  const HeadDims& d = a.d;
  const int o1 = d.H * d.F, o2 = o1 + d.H, o3 = o2 + d.C * d.H;
  const T* want = e < o1 ? a.w1d : e < o2 ? a.b1d : e < o3 ? a.w2d : a.b2d;
  if (!want) return;
  const int per = a.tps * kHeadTileSamples;
  const int n0 = blockIdx.y * per, n1 = min(d.N, n0 + per);
  const T coef = *a.coef;
  T acc = T(0), dv;
  if (e < o2) {
    const int j = e < o1 ? e / d.F : e - o1, f = e < o1 ? e - j * d.F : -1;
    for (int n = n0; n < n1; ++n) {
      const T z = head_dz1_direct(a, n, j, head_label(a, n), coef, &dv);
      acc += f < 0 ? z : z * head_feat(a, n, f);
    }
  } else {
    const int c = e < o3 ? (e - o2) / d.H : e - o3, j = e < o3 ? (e - o2) - c * d.H : -1;
    for (int n = n0; n < n1; ++n) {
      const T g = head_dz2(a, n, c, head_label(a, n), coef);
      if (j < 0) {
        acc += g;
      } else {
        T z;
        head_hidden(a, n, j, T(0), &dv, &z);
        acc += g * dv;
      }
    }
  }
  a.part[(size_t)blockIdx.y * P + e] = acc;
}

// both routes: diff[e] = diff[e] + (part[0][e] + part[1][e] + ...), slabs ascending
template <typename T>
__global__ __launch_bounds__(kHeadThreads) void head_param_finish_kernel(HeadArgs<T> a, int P) {
  const int e = blockIdx.x * kHeadThreads + threadIdx.x;
  if (e >= P) return;
  const HeadDims& d = a.d;
  const int o1 = d.H * d.F, o2 = o1 + d.H, o3 = o2 + d.C * d.H;
  T* out = e < o1 ? (a.w1d ? a.w1d + e : nullptr)
                  : e < o2 ? (a.b1d ? a.b1d + (e - o1) : nullptr)
                           : e < o3 ? (a.w2d ? a.w2d + (e - o2) : nullptr) : (a.b2d ? a.b2d + (e - o3) : nullptr);
  if (!out) return;
  T s = a.part[e];
  for (int k = 1; k < a.slabs; ++k) s += a.part[(size_t)k * P + e];
  *out = *out + s;
}

// ---- fast route -----------------------------------------------------------------------------------------------------
__device__ inline float head_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ inline int head_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(kHeadThreads) void head_fast_forward_kernel(HeadArgs<float> a, HeadFastPlan p) {
  constexpr int TS = kHeadTileSamples;
  extern __shared__ float head_lds[];
  const HeadDims& d = a.d;
  const HeadFwdLds L = head_fwd_carve(head_lds, d, p, TS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;

  head_stage_weights(L, d, p, a.w1, a.b1, a.w2, a.b2);

  float lossacc = 0.f;
  int cntacc = 0;
  const int t0 = blockIdx.x * a.tps, t1 = min((d.N + TS - 1) / TS, t0 + a.tps);
  for (int t = t0; t < t1; ++t) {
    const int n0 = t * TS, n1 = min(d.N, n0 + TS);
    __syncthreads();                        // the previous tile has been consumed (first tile: nothing to wait for)
    for (int e = tid; e < TS * p.Fp; e += kHeadThreads) {
      const int r = e / p.Fp, f = e - r * p.Fp, n = n0 + r;
      L.feats[r * p.Fa + f] = (n < n1 && f < d.F) ? head_feat(a, n, f) : 0.f;
    }
    __syncthreads();
    // fc1: rows = this wave's 16 samples, columns = 16 hidden units; tanh and Dropout on the accumulators
    for (int ht = 0; ht < p.HT; ++ht)
      head_fc1_block(L, d, p, wave, ht, a.b1 != nullptr, n0, n1, a.h, [&](float hv, int n, int j) {
        return d.train ? head_dropout(hv, a.mask[(size_t)n * d.H + j], a.scale) : hv;
      });
    __syncthreads();
    // fc2: lane (sample l16 of the wave, classes grp, grp + 4, ...)
    for (int c = grp; c < d.C; c += 4) head_fc2_one(L, d, p, 16 * wave + l16, c, a.b2 != nullptr);
    __syncthreads();
    if (grp == 0) {                          // softmax and the loss term: one lane per sample
      const int row = 16 * wave + l16, n = n0 + row;
      float term = 0.f;
      int ok = 0;
      if (n < n1)
        term = head_softmax_row(L, d, row, a.prob + (size_t)n * d.C, a.label ? head_label(a, n) : -1, &ok);
      L.terms[row] = term;
      L.valid[row] = ok;
    }
    if (a.loss) {                            // uniform
      __syncthreads();
      if (wave == 0) {
        lossacc += head_wave_sum(L.terms[lane]);
        cntacc += head_wave_sum(L.valid[lane]);
      }
    }
  }
  if (a.loss && tid == 0) {
    if (a.slabs == 1) {
      *a.loss = lossacc / head_normalizer<float>(d, cntacc);
    } else {
      a.lossp[blockIdx.x] = lossacc;
      a.counts[blockIdx.x] = cntacc;
    }
  }
}

__global__ __launch_bounds__(kHeadThreads) void head_fast_backward_kernel(HeadArgs<float> a, HeadFastPlan p) {
  constexpr int TS = kHeadTileSamples;
  extern __shared__ float head_lds[];
  const HeadDims& d = a.d;
  const int Hw = 16 * p.HT, Fw = 16 * p.FT, W2 = d.H + 1, Z2 = d.C + 1;
  float* w1s = head_lds;                    // [Hw][Fk]: w1, rows past H and columns past F zero
  float* feats = w1s + Hw * p.Fk;           // [TS][Fk]: feat, rows past the tile and columns past F zero
  float* bufa = feats + TS * p.Fk;          // [TS][Ha]: d, then dz1
  float* bufk = bufa + TS * p.Ha;           // [TS][Hk]: dz1
  float* w2s = bufk + TS * p.Hk;            // [C][H + 1]
  float* dz2s = w2s + d.C * W2;             // [TS][C + 1]
  int* red = reinterpret_cast<int*>(dz2s + TS * Z2);      // [4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, grp = lane >> 4;
  const bool want_x = a.x0d || a.x1d, want_p = a.w1d || a.b1d || a.w2d || a.b2d;

  if (want_x)
    for (int e = tid; e < Hw * Fw; e += kHeadThreads) {
      const int j = e / Fw, f = e - j * Fw;
      w1s[j * p.Fk + f] = (j < d.H && f < d.F) ? a.w1[(size_t)j * d.F + f] : 0.f;
    }
  for (int e = tid; e < d.C * d.H; e += kHeadThreads) {
    const int c = e / d.H, j = e - c * d.H;
    w2s[c * W2 + j] = a.w2[e];
  }
  int count = 0;
  if (d.norm == MMS_HEAD_NORM_VALID) {       // every workgroup counts every label: an integer sum, the same in any order
    for (int n = tid; n < d.N; n += kHeadThreads) count += head_label(a, n) >= 0;
    count = head_wave_sum(count);
    if (lane == 0) red[wave] = count;
    __syncthreads();
    count = red[0] + red[1] + red[2] + red[3];
  }
  const float coef = a.loss_weight / head_normalizer<float>(d, count);

  head_v4f acc1[8];                         // dz1^T feat: tiles wave, wave + 4, ... of the HT x FT tiles
#pragma unroll
  for (int i = 0; i < 8; ++i) acc1[i] = (head_v4f){0.f, 0.f, 0.f, 0.f};
  float acc2[4] = {0.f, 0.f, 0.f, 0.f};     // w2_diff elements tid, tid + 256, ...
  float b1acc = 0.f, b2acc = 0.f;           // b1_diff[tid], b2_diff[tid]
  const int ntiles1 = p.HT * p.FT;

  const int t0 = blockIdx.x * a.tps, t1 = min((d.N + TS - 1) / TS, t0 + a.tps);
  for (int t = t0; t < t1; ++t) {
    const int n0 = t * TS, n1 = min(d.N, n0 + TS);
    __syncthreads();                        // the previous tile has been consumed
    if (a.w1d)
      for (int e = tid; e < TS * Fw; e += kHeadThreads) {
        const int r = e / Fw, f = e - r * Fw, n = n0 + r;
        feats[r * p.Fk + f] = (n < n1 && f < d.F) ? head_feat(a, n, f) : 0.f;
      }
    for (int e = tid; e < TS * d.C; e += kHeadThreads) {
      const int r = e / d.C, c = e - r * d.C, n = n0 + r;
      dz2s[r * Z2 + c] = n < n1 ? head_dz2(a, n, c, head_label(a, n), coef) : 0.f;
    }
    __syncthreads();
    float z1[16];                           // dz1 of elements tid, tid + 256, ... of the tile's [TS][Hw]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      z1[i] = 0.f;
      if (i < 4 * p.HT) {
        const int e = tid + kHeadThreads * i, r = e / Hw, j = e - r * Hw, n = n0 + r;
        float dv = 0.f;
        if (n < n1 && j < d.H) {
          float dd = 0.f;
          for (int c = 0; c < d.C; ++c) dd += dz2s[r * Z2 + c] * w2s[c * W2 + j];
          head_hidden(a, n, j, dd, &dv, &z1[i]);
        }
        bufa[r * p.Ha + j] = dv;
        bufk[r * p.Hk + j] = z1[i];
      }
    }
    __syncthreads();
    if (want_p) {
      if (a.w2d) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + kHeadThreads * i;
          if (e < d.C * d.H) {
            const int c = e / d.H, j = e - c * d.H;
            for (int r = 0; r < TS; ++r) acc2[i] += dz2s[r * Z2 + c] * bufa[r * p.Ha + j];
          }
        }
      }
      if (a.b2d && tid < d.C)
        for (int r = 0; r < TS; ++r) b2acc += dz2s[r * Z2 + tid];
      if (a.b1d && tid < d.H)
        for (int r = 0; r < TS; ++r) b1acc += bufk[r * p.Hk + tid];
      if (a.w1d) {
        // rows = 16 hidden units, columns = 16 features, K = the tile's samples in steps of 4
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int tile = wave + 4 * i;
          if (tile < ntiles1) {               // wave-uniform
            const int ht = tile / p.FT, ft = tile - ht * p.FT;
            const float* ap = bufk + grp * p.Hk + 16 * ht + l16;
            const float* bp = feats + grp * p.Fk + 16 * ft + l16;
            for (int s = 0; s < TS; s += 4)
              acc1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s * p.Hk], bp[s * p.Fk], acc1[i], 0, 0, 0);
          }
        }
      }
    }
    if (want_x) {
      __syncthreads();                      // d has been consumed
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < 4 * p.HT) {
          const int e = tid + kHeadThreads * i, r = e / Hw, j = e - r * Hw;
          bufa[r * p.Ha + j] = z1[i];
        }
      __syncthreads();
      // rows = this wave's 16 samples, columns = 16 features, K = the hidden units in steps of 4
      for (int ft = 0; ft < p.FT; ++ft) {
        head_v4f acc = {0.f, 0.f, 0.f, 0.f};
        const float* ap = bufa + (16 * wave + l16) * p.Ha + grp;
        const float* bp = w1s + grp * p.Fk + 16 * ft + l16;
        for (int s = 0; s < Hw; s += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s], bp[s * p.Fk], acc, 0, 0, 0);
        const int f = 16 * ft + l16;
        if (f < d.F) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = n0 + 16 * wave + 4 * grp + r;
            if (n >= n1) continue;
            if (f < d.F0) {
              if (a.x0d) a.x0d[(size_t)n * d.F0 + f] = acc[r];
            } else if (a.x1d) {
              a.x1d[(size_t)n * d.F1 + (f - d.F0)] = acc[r];
            }
          }
        }
      }
    }
  }
  if (!want_p) return;
  // one slab: into the diffs; else slab blockIdx.x of the workspace, for head_param_finish_kernel
  const int P = d.H * d.F + d.H + d.C * d.H + d.C;
  const int o1 = d.H * d.F, o2 = o1 + d.H, o3 = o2 + d.C * d.H;
  const bool direct = a.slabs == 1;
  float* slab = direct ? nullptr : a.part + (size_t)blockIdx.x * P;
  if (a.w1d) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int tile = wave + 4 * i;
      if (tile < ntiles1) {
        const int ht = tile / p.FT, ft = tile - ht * p.FT, f = 16 * ft + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * ht + 4 * grp + r;
          if (j < d.H && f < d.F) {
            const int e = j * d.F + f;
            if (direct) a.w1d[e] = a.w1d[e] + acc1[i][r];
            else slab[e] = acc1[i][r];
          }
        }
      }
    }
  }
  if (a.b1d && tid < d.H) {
    if (direct) a.b1d[tid] = a.b1d[tid] + b1acc;
    else slab[o1 + tid] = b1acc;
  }
  if (a.w2d) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + kHeadThreads * i;
      if (e < d.C * d.H) {
        if (direct) a.w2d[e] = a.w2d[e] + acc2[i];
        else slab[o2 + e] = acc2[i];
      }
    }
  }
  if (a.b2d && tid < d.C) {
    if (direct) a.b2d[tid] = a.b2d[tid] + b2acc;
    else slab[o3 + tid] = b2acc;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
int head_route(const HeadDims& d, int pass) {
  if (pass != MMS_HEAD_PASS_FORWARD && pass != MMS_HEAD_PASS_BACKWARD) return MMS_HEAD_ROUTE_NONE;
  return head_fast_plan(d).ok ? MMS_HEAD_ROUTE_FAST : MMS_HEAD_ROUTE_GENERIC;
}

template <typename T>
size_t head_workspace_bytes(const mms_head_shape* shape) {
  HeadDims d;
  if (head_check(shape, &d) != MMS_OK || d.N == 0) return 0;
  int tps;
  const int slabs = head_slabs(d.N, &tps);
  return (size_t)kHeadHeaderBytes + (size_t)slabs * head_params(d) * sizeof(T);
}

template <typename T>
void head_bind_workspace(HeadArgs<T>* a, void* workspace) {
  char* base = static_cast<char*>(workspace);
  a->counts = reinterpret_cast<int*>(base);
  a->lossp = reinterpret_cast<T*>(base + kHeadMaxSlabs * sizeof(int));
  a->coef = reinterpret_cast<T*>(base + kHeadMaxSlabs * (sizeof(int) + 8));
  a->part = reinterpret_cast<T*>(base + kHeadHeaderBytes);
}

template <typename T>
T head_scale(const mms_head_shape* s) {
  return T(1. / (1. - s->dropout_ratio));   // dropout_layer.cpp:14-18: threshold_ is a float, the quotient a double
}

template <typename T>
int head_forward(const mms_head_shape* shape, const T* x0, const T* x1, const T* w1, const T* b1, const unsigned* mask,
                 const T* w2, const T* b2, const T* label, T* h, T* prob, T* loss, void* workspace,
                 size_t workspace_bytes, bool generic, hipStream_t s) {
  HeadDims d;
  int rc = head_check(shape, &d);
  if (rc != MMS_OK) return rc;
  if (d.N == 0) return MMS_OK;
  if (!x0 || !w1 || !w2 || !h || !prob || (d.F1 > 0 && !x1) || (d.train && !mask) || (loss && !label))
    return MMS_ERR_INVALID_ARG;
  const void* const outs[] = {h, prob, loss};
  const void* const ins[] = {x0, x1, w1, b1, mask, w2, b2, label};
  if (outputs_alias(outs, ins)) return MMS_ERR_INVALID_ARG;
  if (loss && (!workspace || workspace_bytes < head_workspace_bytes<T>(shape))) return MMS_ERR_WORKSPACE;
  HeadArgs<T> a = {};
  a.d = d;
  a.scale = head_scale<T>(shape);
  a.x0 = x0; a.x1 = x1; a.w1 = w1; a.b1 = b1; a.mask = mask; a.w2 = w2; a.b2 = b2; a.label = label;
  a.h = h; a.prob = prob; a.loss = loss;
  a.slabs = head_slabs(d.N, &a.tps);
  if (loss) head_bind_workspace(&a, workspace);
  if constexpr (std::is_same<T, float>::value) {
    if (!generic && head_route(d, MMS_HEAD_PASS_FORWARD) == MMS_HEAD_ROUTE_FAST) {
      const HeadFastPlan p = head_fast_plan(d);
      static const hipError_t once = allow_dynamic_lds(&head_fast_forward_kernel, kHeadMaxLdsBytes);
      if (once != hipSuccess) return MMS_ERR_LAUNCH;
      hipLaunchKernelGGL(head_fast_forward_kernel, dim3(a.slabs), dim3(kHeadThreads), p.fwd_lds, s, a, p);
      if ((rc = launch_status()) != MMS_OK || !loss || a.slabs == 1) return rc;
      hipLaunchKernelGGL((head_loss_finish_kernel<float>), dim3(1), dim3(64), 0, s, a);
      return launch_status();
    }
  }
  const int total = d.N * d.H;
  hipLaunchKernelGGL((head_fc1_kernel<T>), dim3((total + kHeadThreads - 1) / kHeadThreads), dim3(kHeadThreads), 0, s, a,
                     total);
  if ((rc = launch_status()) != MMS_OK) return rc;
  hipLaunchKernelGGL((head_out_kernel<T>), dim3(a.slabs), dim3(kHeadThreads), 0, s, a);
  if ((rc = launch_status()) != MMS_OK || !loss) return rc;
  hipLaunchKernelGGL((head_loss_finish_kernel<T>), dim3(1), dim3(64), 0, s, a);
  return launch_status();
}

template <typename T>
int head_backward(const mms_head_shape* shape, const T* x0, const T* x1, const T* w1, const T* w2, const unsigned* mask,
                  const T* h, const T* prob, const T* label, T loss_weight, T* x0d, T* x1d, T* w1d, T* b1d, T* w2d,
                  T* b2d, void* workspace, size_t workspace_bytes, bool generic, hipStream_t s) {
  HeadDims d;
  int rc = head_check(shape, &d);
  if (rc != MMS_OK) return rc;
  if (d.N == 0) return MMS_OK;
  if (!x0 || !w1 || !w2 || !h || !prob || !label || (d.F1 > 0 && !x1) || (d.train && !mask))
    return MMS_ERR_INVALID_ARG;
  if (d.F1 == 0) x1d = nullptr;             // an array of no elements
  if (!x0d && !x1d && !w1d && !b1d && !w2d && !b2d) return MMS_ERR_INVALID_ARG;
  const void* const outs[] = {x0d, x1d, w1d, b1d, w2d, b2d};
  const void* const ins[] = {x0, x1, w1, w2, mask, h, prob, label};
  if (outputs_alias(outs, ins)) return MMS_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < head_workspace_bytes<T>(shape)) return MMS_ERR_WORKSPACE;
  HeadArgs<T> a = {};
  a.d = d;
  a.scale = head_scale<T>(shape);
  a.loss_weight = loss_weight;
  a.x0 = x0; a.x1 = x1; a.w1 = w1; a.w2 = w2; a.mask = mask; a.h_in = h; a.prob_in = prob; a.label = label;
  a.x0d = x0d; a.x1d = x1d; a.w1d = w1d; a.b1d = b1d; a.w2d = w2d; a.b2d = b2d;
  a.slabs = head_slabs(d.N, &a.tps);
  head_bind_workspace(&a, workspace);
  const int P = head_params(d);
  const bool want_p = w1d || b1d || w2d || b2d;
  const dim3 pgrid((P + kHeadThreads - 1) / kHeadThreads);
  if constexpr (std::is_same<T, float>::value) {
    if (!generic && head_route(d, MMS_HEAD_PASS_BACKWARD) == MMS_HEAD_ROUTE_FAST) {
      const HeadFastPlan p = head_fast_plan(d);
      static const hipError_t once = allow_dynamic_lds(&head_fast_backward_kernel, kHeadMaxLdsBytes);
      if (once != hipSuccess) return MMS_ERR_LAUNCH;
      hipLaunchKernelGGL(head_fast_backward_kernel, dim3(a.slabs), dim3(kHeadThreads), p.bwd_lds, s, a, p);
      if ((rc = launch_status()) != MMS_OK || !want_p || a.slabs == 1) return rc;
      hipLaunchKernelGGL((head_param_finish_kernel<float>), pgrid, dim3(kHeadThreads), 0, s, a, P);
      return launch_status();
    }
  }
  hipLaunchKernelGGL((head_coef_kernel<T>), dim3(1), dim3(kHeadThreads), 0, s, a);
  if ((rc = launch_status()) != MMS_OK) return rc;
  if (x0d || x1d) {
    const int total = d.N * d.F;
    hipLaunchKernelGGL((head_xdiff_kernel<T>), dim3((total + kHeadThreads - 1) / kHeadThreads), dim3(kHeadThreads), 0, s,
                       a, total);
    if ((rc = launch_status()) != MMS_OK) return rc;
  }
  if (!want_p) return MMS_OK;
  hipLaunchKernelGGL((head_param_kernel<T>), dim3(pgrid.x, a.slabs), dim3(kHeadThreads), 0, s, a, P);
  if ((rc = launch_status()) != MMS_OK) return rc;
  hipLaunchKernelGGL((head_param_finish_kernel<T>), pgrid, dim3(kHeadThreads), 0, s, a, P);
  return launch_status();
}

}  // namespace

int head_loss_from_terms(const float* terms, const int* valid, const HeadDims& d, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(head_loss_from_terms_kernel, dim3(1), dim3(64), 0, s, terms, valid, d, loss);
  return launch_status();
}

}  // namespace mms

using namespace mms;

extern "C" {

size_t mms_head_workspace_bytes(const mms_head_shape* shape) { return head_workspace_bytes<float>(shape); }
size_t mms_head_workspace_bytes_f64(const mms_head_shape* shape) { return head_workspace_bytes<double>(shape); }

int mms_head_route(const mms_head_shape* shape, int pass) {
  HeadDims d;
  if (head_check(shape, &d) != MMS_OK) return MMS_HEAD_ROUTE_NONE;
  return head_route(d, pass);
}

int mms_head_forward_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1, const float* b1,
                         const unsigned int* mask, const float* w2, const float* b2, const float* label, float* h,
                         float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  return head_forward<float>(shape, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, workspace, workspace_bytes, false,
                             as_stream(stream));
}

int mms_head_backward_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                          const float* w2, const unsigned int* mask, const float* h, const float* prob,
                          const float* label, float loss_weight, float* x0_diff, float* x1_diff, float* w1_diff,
                          float* b1_diff, float* w2_diff, float* b2_diff, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return head_backward<float>(shape, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff,
                              w2_diff, b2_diff, workspace, workspace_bytes, false, as_stream(stream));
}

int mms_head_forward_f64(const mms_head_shape* shape, const double* x0, const double* x1, const double* w1,
                         const double* b1, const unsigned int* mask, const double* w2, const double* b2,
                         const double* label, double* h, double* prob, double* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return head_forward<double>(shape, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, workspace, workspace_bytes, true,
                              as_stream(stream));
}

int mms_head_backward_f64(const mms_head_shape* shape, const double* x0, const double* x1, const double* w1,
                          const double* w2, const unsigned int* mask, const double* h, const double* prob,
                          const double* label, double loss_weight, double* x0_diff, double* x1_diff, double* w1_diff,
                          double* b1_diff, double* w2_diff, double* b2_diff, void* workspace, size_t workspace_bytes,
                          void* stream) {
  return head_backward<double>(shape, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff,
                               b1_diff, w2_diff, b2_diff, workspace, workspace_bytes, true,
                               as_stream(stream));
}

int mms_head_forward_generic_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                                 const float* b1, const unsigned int* mask, const float* w2, const float* b2,
                                 const float* label, float* h, float* prob, float* loss, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return head_forward<float>(shape, x0, x1, w1, b1, mask, w2, b2, label, h, prob, loss, workspace, workspace_bytes, true,
                             as_stream(stream));
}

int mms_head_backward_generic_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                                  const float* w2, const unsigned int* mask, const float* h, const float* prob,
                                  const float* label, float loss_weight, float* x0_diff, float* x1_diff,
                                  float* w1_diff, float* b1_diff, float* w2_diff, float* b2_diff, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return head_backward<float>(shape, x0, x1, w1, w2, mask, h, prob, label, loss_weight, x0_diff, x1_diff, w1_diff, b1_diff,
                              w2_diff, b2_diff, workspace, workspace_bytes, true, as_stream(stream));
}

}  // extern "C"
