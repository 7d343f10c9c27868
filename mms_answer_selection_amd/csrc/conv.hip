// csrc/conv.hip -- Convolution, the reference's 2-d ConvolutionLayer (conv_layer.cpp:25-73, base_conv_layer.cpp:257-321),
// and its extern "C" entry points (include/mms_conv.h: mms_conv_*).  The reference forms an im2col buffer and calls BLAS
// per image; nothing here writes such a buffer.  With Cg = C / group, Kg = K / group and g = k / Kg:
//
//   forward      top[n,k,oy,ox]  = sum_{c<Cg, i<kh, j<kw} w[k,c,i,j] * x[n, g Cg + c, oy sh - ph + i, ox sw - pw + j] + bias[k]
//   bottom_diff  dx[n,c,y,x]     = sum_{k in group of c, i, j : (y + ph - i) = oy sh, (x + pw - j) = ox sw} w[k,c,i,j] * dy[n,k,oy,ox]
//   weight_diff  dw[k,c,i,j]    += sum_{n,oy,ox} dy[n,k,oy,ox] * x[n, g Cg + c, oy sh - ph + i, ox sw - pw + j]
//   bias_diff    db[k]          += sum_{n,oy,ox} dy[n,k,oy,ox]
//
// Two routes (mms_conv_route, the one place that decides; conv_prod_plan of csrc/conv_tile.h and conv_wdiff_plan of
// csrc/conv_plans.h say what the fast one takes):
//
//   generic  direct kernels <T>, one thread per output element, sums in ascending (c, i, j) (forward), (k, i, j)
//            (bottom_diff, gather form: no col2im scatter) and (n, oy, ox) (parameter diffs) order.  Every accepted
//            shape; all of double; float where the fast route does not reach.
//   fast     float, stride 1, pad 0, group 1, C and K <= 64: an implicit GEMM on v_mfma_f32_16x16x4_f32.
//            PRODUCT kernel (forward, and bottom_diff as the same product on top_diff with C and K swapped, the taps
//            flipped and a border of kh-1 / kw-1 zeros, which the staging writes by predication): a workgroup of four
//            waves owns up to 256 output pixels -- a band of whole rows of one image, or several whole small images
//            -- and all output channels.  Per chunk of input channels it stages the chunk's input band
//            [image][channel][row][col] and the chunk's weights [k][m] in LDS; the im2col operand B[k][pixel] is
//            band[koff[k] + pix[pixel]], two offsets added.  MFMA rows are output channels and columns are 16
//            consecutive pixels of the band, so a store instruction writes runs along OW.  Wave w owns pixel tiles
//            w, w+4, w+8, w+12 x all MT channel tiles.  Order of a sum: channels ascending in chunks, (c, i, j)
//            ascending inside a chunk in steps of four, the four of a step as the MFMA adds them.
//            PARAMETER-DIFF kernel: rows are output channels, columns 16 consecutive (c, i, j), the sum runs over
//            pixels.  The (image group, row band) units of the batch are dealt in ascending runs to at most 64 slabs
//            (blockIdx.y); a workgroup owns four column tiles x all MT channel tiles, walks its slab's units in
//            ascending order -- staging the unit's x band and top_diff tile in LDS -- and writes its partial sums to
//            slab s of the workspace.  The workgroups of column group 0 also add each channel's top_diff from the
//            staged tile, pixel by pixel: bias_diff comes from the same sweep.
//   both     conv_reduce_kernel adds the slabs in ascending order, first to last, and then into weight_diff / bias_diff.
//
// Nothing is read 16 bytes at a time, so alignment cannot change an order; every workspace word that is read has been
// written by this call.
#include "conv_plans.h"
#include "conv_tile.h"
#include "conv_wdiff_tile.h"
#include "mms_conv.h"
#include "mms_internal.h"

namespace mms {
namespace {

// ---- generic route ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kConvThreads) void conv_forward_direct_kernel(ConvDims d, const T* __restrict__ x,
                                                                           const T* __restrict__ w,
                                                                           const T* __restrict__ bias,
                                                                           T* __restrict__ top, int total) {
  const int idx = blockIdx.x * kConvThreads + threadIdx.x;
  if (idx >= total) return;
  const int ox = idx % d.OW;
  int t = idx / d.OW;
  const int oy = t % d.OH;
  t /= d.OH;
  const int k = t % d.K, n = t / d.K;
  const int g = k / d.Kg;
  const int y0 = oy * d.sh - d.ph, x0 = ox * d.sw - d.pw;
  T acc = T(0);
  for (int c = 0; c < d.Cg; ++c) {
    const T* xc = x + ((size_t)n * d.C + g * d.Cg + c) * d.H * d.W;
    const T* wc = w + ((size_t)k * d.Cg + c) * d.kh * d.kw;
    for (int i = 0; i < d.kh; ++i) {
      const int iy = y0 + i;
      if (iy < 0 || iy >= d.H) continue;
      for (int j = 0; j < d.kw; ++j) {
        const int ix = x0 + j;
        if (ix < 0 || ix >= d.W) continue;
        acc += wc[i * d.kw + j] * xc[(size_t)iy * d.W + ix];
      }
    }
  }
  top[idx] = bias ? acc + bias[k] : acc;
}

// gather form: the (k, i, j) whose forward term read this bottom element
template <typename T>
__global__ __launch_bounds__(kConvThreads) void conv_bottom_direct_kernel(ConvDims d, const T* __restrict__ w,
                                                                          const T* __restrict__ dy,
                                                                          T* __restrict__ dx, int total) {
  const int idx = blockIdx.x * kConvThreads + threadIdx.x;
  if (idx >= total) return;
  const int xx = idx % d.W;
  int t = idx / d.W;
  const int yy = t % d.H;
  t /= d.H;
  const int c = t % d.C, n = t / d.C;
  const int g = c / d.Cg, cl = c - g * d.Cg;
  T acc = T(0);
  for (int kk = 0; kk < d.Kg; ++kk) {
    const int k = g * d.Kg + kk;
    const T* wk = w + ((size_t)k * d.Cg + cl) * d.kh * d.kw;
    const T* dk = dy + ((size_t)n * d.K + k) * d.OH * d.OW;
    for (int i = 0; i < d.kh; ++i) {
      const int ty = yy + d.ph - i;
      if (ty < 0 || ty % d.sh) continue;
      const int oy = ty / d.sh;
      if (oy >= d.OH) continue;
      for (int j = 0; j < d.kw; ++j) {
        const int tx = xx + d.pw - j;
        if (tx < 0 || tx % d.sw) continue;
        const int ox = tx / d.sw;
        if (ox >= d.OW) continue;
        acc += wk[i * d.kw + j] * dk[(size_t)oy * d.OW + ox];
      }
    }
  }
  dx[idx] = acc;
}

// Slab blockIdx.y sums rows [y * rps, (y + 1) * rps) of the N * OH (n, oy) rows; element e < nW is a weight, e - nW a bias.
template <typename T>
__global__ __launch_bounds__(kConvThreads) void conv_param_direct_kernel(ConvDims d, const T* __restrict__ x,
                                                                         const T* __restrict__ dy,
                                                                         T* __restrict__ part, int nW, int want_w,
                                                                         int want_b, int rps) {
  const int e = blockIdx.x * kConvThreads + threadIdx.x;
  if (e >= nW + d.K) return;
  if (e < nW ? !want_w : !want_b) return;
  const int rows = d.N * d.OH;
  const int r0 = blockIdx.y * rps, r1 = min(rows, r0 + rps);
  T acc = T(0);
  if (e < nW) {
    const int j = e % d.kw;
    int t = e / d.kw;
    const int i = t % d.kh;
    t /= d.kh;
    const int c = t % d.Cg, k = t / d.Cg;
    const int g = k / d.Kg;
    for (int r = r0; r < r1; ++r) {
      const int n = r / d.OH, oy = r - n * d.OH;
      const int iy = oy * d.sh - d.ph + i;
      if (iy < 0 || iy >= d.H) continue;
      const T* dr = dy + (((size_t)n * d.K + k) * d.OH + oy) * d.OW;
      const T* xr = x + (((size_t)n * d.C + g * d.Cg + c) * d.H + iy) * d.W;
      for (int ox = 0; ox < d.OW; ++ox) {
        const int ix = ox * d.sw - d.pw + j;
        if (ix < 0 || ix >= d.W) continue;
        acc += dr[ox] * xr[ix];
      }
    }
  } else {
    const int k = e - nW;
    for (int r = r0; r < r1; ++r) {
      const int n = r / d.OH, oy = r - n * d.OH;
      const T* dr = dy + (((size_t)n * d.K + k) * d.OH + oy) * d.OW;
      for (int ox = 0; ox < d.OW; ++ox) acc += dr[ox];
    }
  }
  part[(size_t)blockIdx.y * (nW + d.K) + e] = acc;
}

// conv_reduce_element (csrc/conv_wdiff_tile.h) for every element; both routes
template <typename T>
__global__ __launch_bounds__(kConvThreads) void conv_reduce_kernel(const T* __restrict__ part, int slabs, int nW, int K,
                                                                   T* __restrict__ weight_diff,
                                                                   T* __restrict__ bias_diff) {
  conv_reduce_element(part, slabs, nW, K, weight_diff, bias_diff);
}

// ---- fast route ---------------------------------------------------------------------------------------------------
// The product's tile, plan, loop and the epilogue that stores the map (ConvStoreEpilogue) are csrc/conv_tile.h's.
template <int MT>
__global__ __launch_bounds__(kConvThreads) void conv_prod_kernel(ConvProdArgs a) {
  extern __shared__ float conv_lds[];
  ConvStoreEpilogue epi;
  epi.PI = (size_t)a.OHt * a.OWt;
  conv_tile_product<MT>(a, conv_lds, epi);
}

// The parameter-diff tile (csrc/conv_wdiff_tile.h) on top_diff as it lies in memory.
template <int MT>
__global__ __launch_bounds__(kConvThreads) void conv_wdiff_kernel(ConvWdiffArgs a) {
  extern __shared__ float conv_lds[];
  conv_wdiff_tile<MT>(a, conv_lds, ConvLoadTopDiff());
}

void conv_prod_launch(ConvProdArgs a, const float* in, const float* w, const float* bias, float* out, hipStream_t s) {
  a.in = in; a.w = w; a.bias = bias; a.out = out;
  const dim3 grid((unsigned)((a.N + a.G - 1) / a.G), (unsigned)a.bands);
  conv_with_mt(a.MT, [&](auto M) {
    hipLaunchKernelGGL((conv_prod_kernel<decltype(M)::value>), grid, dim3(kConvThreads), a.lds_bytes, s, a);
  });
}

// ---- host -----------------------------------------------------------------------------------------------------------
int conv_route(const ConvDims& d, int pass) {
  if (pass == MMS_CONV_PASS_FORWARD || pass == MMS_CONV_PASS_BOTTOM_DIFF)
    return conv_prod_plan(d, pass, 1).ok ? MMS_CONV_ROUTE_FAST : MMS_CONV_ROUTE_GENERIC;
  if (pass == MMS_CONV_PASS_PARAM_DIFF) return conv_wdiff_plan(d).ok ? MMS_CONV_ROUTE_FAST : MMS_CONV_ROUTE_GENERIC;
  return MMS_CONV_ROUTE_NONE;
}

template <typename T>
size_t conv_workspace_bytes(const mms_conv_shape* shape) {
  ConvDims d;
  if (conv_check(shape, &d) != MMS_OK || d.N == 0) return 0;
  int rps;
  int slabs = conv_generic_slabs(d, &rps);
  if (std::is_same<T, float>::value) {
    const ConvWdiffArgs f = conv_wdiff_plan(d);
    if (f.ok && f.slabs > slabs) slabs = f.slabs;
  }
  return (size_t)slabs * ((size_t)d.K * d.Cg * d.kh * d.kw + d.K) * sizeof(T);
}

template <typename T>
int conv_forward(const mms_conv_shape* shape, const T* x, const T* w, const T* bias, T* top, bool generic,
                 hipStream_t s) {
  ConvDims d;
  const int rc = conv_check(shape, &d);
  if (rc != MMS_OK) return rc;
  if (d.N == 0) return MMS_OK;
  if (!x || !w || !top) return MMS_ERR_INVALID_ARG;
  const void* const outputs[] = {top};
  const void* const inputs[] = {x};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  if constexpr (std::is_same<T, float>::value) {
    if (!generic && conv_route(d, MMS_CONV_PASS_FORWARD) == MMS_CONV_ROUTE_FAST) {
      conv_prod_launch(conv_prod_plan(d, MMS_CONV_PASS_FORWARD, 1), x, w, bias, top, s);
      return launch_status();
    }
  }
  const int total = d.N * d.K * d.OH * d.OW;
  hipLaunchKernelGGL((conv_forward_direct_kernel<T>), dim3((total + kConvThreads - 1) / kConvThreads),
                     dim3(kConvThreads), 0, s, d, x, w, bias, top, total);
  return launch_status();
}

template <typename T>
int conv_backward(const mms_conv_shape* shape, const T* x, const T* w, const T* dy, T* dx, T* dw, T* db, void* workspace,
                  size_t workspace_bytes, bool generic, hipStream_t s) {
  ConvDims d;
  int rc = conv_check(shape, &d);
  if (rc != MMS_OK) return rc;
  if (d.N == 0) return MMS_OK;
  if (!x || !w || !dy || (!dx && !dw && !db)) return MMS_ERR_INVALID_ARG;
  const void* const outputs[] = {dx};
  const void* const inputs[] = {x, dy};
  if (outputs_alias(outputs, inputs)) return MMS_ERR_INVALID_ARG;
  if ((dw || db) && (!workspace || workspace_bytes < conv_workspace_bytes<T>(shape))) return MMS_ERR_WORKSPACE;
  constexpr bool kFloat = std::is_same<T, float>::value;
  if (dx) {
    bool done = false;
    if constexpr (kFloat) {
      if (!generic && conv_route(d, MMS_CONV_PASS_BOTTOM_DIFF) == MMS_CONV_ROUTE_FAST) {
        conv_prod_launch(conv_prod_plan(d, MMS_CONV_PASS_BOTTOM_DIFF, 1), dy, w, nullptr, dx, s);
        done = true;
      }
    }
    if (!done) {
      const int total = d.N * d.C * d.H * d.W;
      hipLaunchKernelGGL((conv_bottom_direct_kernel<T>), dim3((total + kConvThreads - 1) / kConvThreads),
                         dim3(kConvThreads), 0, s, d, w, dy, dx, total);
    }
    if ((rc = launch_status()) != MMS_OK) return rc;
  }
  if (!dw && !db) return MMS_OK;
  const int nW = d.K * d.Cg * d.kh * d.kw;
  T* part = static_cast<T*>(workspace);
  int slabs = 0;
  if constexpr (kFloat) {
    if (!generic && conv_route(d, MMS_CONV_PASS_PARAM_DIFF) == MMS_CONV_ROUTE_FAST) {
      ConvWdiffArgs a = conv_wdiff_plan(d);
      a.x = x; a.dy = dy; a.part = part; a.want_w = dw != nullptr; a.want_b = db != nullptr;
      const int groups = dw ? (d.C * d.kh * d.kw + 63) / 64 : 1;     // four column tiles of 16 per workgroup
      conv_with_mt(a.MT, [&](auto M) {
        hipLaunchKernelGGL((conv_wdiff_kernel<decltype(M)::value>), dim3((unsigned)groups, (unsigned)a.slabs),
                           dim3(kConvThreads), a.lds_bytes, s, a);
      });
      slabs = a.slabs;
    }
  }
  if (!slabs) {
    int rps;
    slabs = conv_generic_slabs(d, &rps);
    hipLaunchKernelGGL((conv_param_direct_kernel<T>), dim3((nW + d.K + kConvThreads - 1) / kConvThreads, slabs),
                       dim3(kConvThreads), 0, s, d, x, dy, part, nW, dw != nullptr, db != nullptr, rps);
  }
  if ((rc = launch_status()) != MMS_OK) return rc;
  hipLaunchKernelGGL((conv_reduce_kernel<T>), dim3((nW + d.K + kConvThreads - 1) / kConvThreads), dim3(kConvThreads),
                     0, s, (const T*)part, slabs, nW, d.K, dw, db);
  return launch_status();
}

}  // namespace
}  // namespace mms

using namespace mms;

extern "C" {

int mms_conv_output_dims(const mms_conv_shape* shape, int* OH, int* OW) {
  ConvDims d;
  const int rc = conv_check(shape, &d);
  if (rc != MMS_OK) return rc;
  if (!OH || !OW) return MMS_ERR_INVALID_ARG;
  *OH = d.OH;
  *OW = d.OW;
  return MMS_OK;
}

size_t mms_conv_workspace_bytes(const mms_conv_shape* shape) { return conv_workspace_bytes<float>(shape); }
size_t mms_conv_workspace_bytes_f64(const mms_conv_shape* shape) { return conv_workspace_bytes<double>(shape); }

int mms_conv_route(const mms_conv_shape* shape, int pass) {
  ConvDims d;
  if (conv_check(shape, &d) != MMS_OK) return MMS_CONV_ROUTE_NONE;
  return conv_route(d, pass);
}

int mms_conv_forward_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* bias,
                         float* top, void*, size_t, void* stream) {
  return conv_forward<float>(shape, x, weight, bias, top, false, as_stream(stream));
}

int mms_conv_backward_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* top_diff,
                          float* bottom_diff, float* weight_diff, float* bias_diff, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return conv_backward<float>(shape, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, workspace,
                              workspace_bytes, false, as_stream(stream));
}

int mms_conv_forward_f64(const mms_conv_shape* shape, const double* x, const double* weight, const double* bias,
                         double* top, void*, size_t, void* stream) {
  return conv_forward<double>(shape, x, weight, bias, top, true, as_stream(stream));
}

int mms_conv_backward_f64(const mms_conv_shape* shape, const double* x, const double* weight, const double* top_diff,
                          double* bottom_diff, double* weight_diff, double* bias_diff, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return conv_backward<double>(shape, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, workspace,
                               workspace_bytes, true, as_stream(stream));
}

int mms_conv_forward_generic_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* bias,
                                 float* top, void*, size_t, void* stream) {
  return conv_forward<float>(shape, x, weight, bias, top, true, as_stream(stream));
}

int mms_conv_backward_generic_f32(const mms_conv_shape* shape, const float* x, const float* weight,
                                  const float* top_diff, float* bottom_diff, float* weight_diff, float* bias_diff,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return conv_backward<float>(shape, x, weight, top_diff, bottom_diff, weight_diff, bias_diff, workspace,
                              workspace_bytes, true, as_stream(stream));
}

}  // extern "C"
