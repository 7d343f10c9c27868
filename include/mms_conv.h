/* include/mms_conv.h -- Convolution (the reference's ConvolutionLayer, 2-d) on the C ABI of libmms_hip.so.
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  All arrays are device memory,
 * contiguous and row-major; a call enqueues its launches on `stream` and returns without waiting.
 *
 * The layer (conv_layer.cpp:25-73, base_conv_layer.cpp:257-321), with OH, OW from mms_conv_output_dims:
 *
 *   forward   top[n, k, oy, ox] = sum_{c, i, j} weight[k, c, i, j] * x[n, g*C/group + c, oy*stride_h - pad_h + i,
 *                                                                      ox*stride_w - pad_w + j]  (+ bias[k])
 *             for k in group g = k / (K/group), c in [0, C/group); x reads 0 outside the image.
 *   backward  bottom_diff  = the transpose of that map applied to top_diff         OVERWRITTEN  (beta 0)
 *             weight_diff += sum_{n, oy, ox} top_diff[n, k, oy, ox] * x[...]        ACCUMULATED  (beta 1)
 *             bias_diff   += sum_{n, oy, ox} top_diff[n, k, oy, ox]                 ACCUMULATED  (beta 1)
 *
 *   x, bottom_diff (N, C, H, W)    weight, weight_diff (K, C/group, kh, kw)    bias, bias_diff (K)
 *   top, top_diff  (N, K, OH, OW)  bias == NULL: bias_term false
 *
 * Summation order.  The reference's sums are BLAS-ordered; here the order is a fixed function of the shape, the
 * element type and the route: no floating-point atomics, the same words on every run, for every alignment of the
 * arrays and whatever the workspace held before the call.  Parameter diffs are summed in slabs of the (n, oy) range:
 * each slab's partial sum goes to the workspace, and the slabs are added in ascending order, first to last, and then
 * into the diff.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  a NULL shape; N < 0; C, H, W, K, kh, kw, stride_*, dilation_*, group <= 0; pad_* < 0; C or K
 *                        not divisible by group; OH or OW < 1; x, top or weight over INT_MAX elements; with N > 0, a NULL
 *                        x, weight, top / top_diff; top == x; a backward with no output; bottom_diff == x or
 *                        bottom_diff == top_diff.
 *   MMS_ERR_UNSUPPORTED  dilation_h or dilation_w other than 1 (the fields exist so that the ABI need not change).
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query, for a backward that has a weight_diff or bias_diff.
 *   N == 0               MMS_OK, nothing is written.
 */
#ifndef MMS_CONV_H_
#define MMS_CONV_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mms_conv_shape {
  int N, C, H, W;            /* bottom (N, C, H, W), contiguous, row-major        */
  int K;                     /* num_output                                         */
  int kh, kw, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group;
} mms_conv_shape;

/* OH = (H + 2 pad_h - (dilation_h (kh - 1) + 1)) / stride_h + 1, OW alike (conv_layer.cpp:14-21; the division
 * truncates, so a stride may leave rows over).  MMS_OK, or the refusal the calls give for this shape; OH / OW are
 * written only with MMS_OK. */
int mms_conv_output_dims(const mms_conv_shape* shape, int* OH, int* OW);

/* Bytes of workspace that mms_conv_backward_* needs for its slabs, on whichever route; 0 for a shape the calls
 * refuse and for N == 0.  The forward needs none. */
size_t mms_conv_workspace_bytes(const mms_conv_shape* shape);
size_t mms_conv_workspace_bytes_f64(const mms_conv_shape* shape);

/* The one routing decision of the float calls: the launchers call it, and so may a host.  pass: */
#define MMS_CONV_PASS_FORWARD 0
#define MMS_CONV_PASS_BOTTOM_DIFF 1
#define MMS_CONV_PASS_PARAM_DIFF 2      /* weight_diff and bias_diff */
/* returns: */
#define MMS_CONV_ROUTE_NONE (-1)        /* the calls refuse this shape, or pass is not one of the three */
#define MMS_CONV_ROUTE_GENERIC 0        /* direct kernels: one thread per output element, any accepted shape */
#define MMS_CONV_ROUTE_FAST 1           /* implicit GEMM on the fp32 matrix pipe: stride 1, pad 0, group 1, K and C at
                                           most 64, rows short enough for the tile (csrc/conv.hip: conv_fast_plan) */
/* The _f64 calls and the *_generic_* calls always take MMS_CONV_ROUTE_GENERIC. */
int mms_conv_route(const mms_conv_shape* shape, int pass);

int mms_conv_forward_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* bias,
                         float* top, void* workspace, size_t workspace_bytes, void* stream);
int mms_conv_backward_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* top_diff,
                          float* bottom_diff, float* weight_diff, float* bias_diff, void* workspace,
                          size_t workspace_bytes, void* stream);
int mms_conv_forward_f64(const mms_conv_shape* shape, const double* x, const double* weight, const double* bias,
                         double* top, void* workspace, size_t workspace_bytes, void* stream);
int mms_conv_backward_f64(const mms_conv_shape* shape, const double* x, const double* weight, const double* top_diff,
                          double* bottom_diff, double* weight_diff, double* bias_diff, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The same two float calls on MMS_CONV_ROUTE_GENERIC whatever mms_conv_route says: the summation order of the _f64
 * calls, in float.  For a host that wants one order at every shape, and for checking one route against the other. */
int mms_conv_forward_generic_f32(const mms_conv_shape* shape, const float* x, const float* weight, const float* bias,
                                 float* top, void* workspace, size_t workspace_bytes, void* stream);
int mms_conv_backward_generic_f32(const mms_conv_shape* shape, const float* x, const float* weight,
                                  const float* top_diff, float* bottom_diff, float* weight_diff, float* bias_diff,
                                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_CONV_H_ */
