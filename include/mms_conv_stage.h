/* include/mms_conv_stage.h -- one scoring (TEST-phase) stage of network_v4, Convolution -> BN -> AvePool -> TanH, as
 * one call on the C ABI of libmms_hip.so.
 *
 * This header adds to include/mms_conv.h and include/mms.h and changes nothing in them: the shape struct, the error
 * codes, the stream convention and MMS_VERSION are theirs.  All arrays are device memory, contiguous and row-major; a
 * call enqueues its launches on `stream` and returns without waiting.
 *
 * With (OH, OW) from mms_conv_output_dims and a pooling window (ph, pw) that tiles (OH, OW), the stage is exactly what
 * these two calls compute one after the other, the convolution's map being an intermediate nobody else reads:
 *
 *   mms_conv_forward_*            y = conv(x, weight) (+ bias)                            (N, K, OH, OW)
 *   mms_bn_pool_tanh_forward_*    phase = TEST (1), running_mean = mean, running_var = var:
 *                                 m   = the window's y added in (h, w) order, starting from 0, / (ph*pw)
 *                                 sp  = (m + (-mean[k])) / sqrt(var[k] + 1e-9)
 *                                 top = tanh(sp * scale[k] + shift[k])
 *
 *   x (N, C, H, W)   weight (K, C/group, kh, kw)   bias (K) or NULL   mean, var, scale, shift (K)
 *   top, save_pool (N, K, OH/ph, OW/pw); save_pool (= sp) is optional: NULL skips it.
 *
 * TRAIN phase needs the batch statistics of y and is not offered here: include/mms_conv_stage_train.h has it.
 *
 * Two routes (mms_conv_stage_route, the one place that decides; the launchers call it too):
 *   SEQUENCE  the two calls above, y in the caller's workspace.
 *   FUSED     float only.  One launch: the convolution's fast route (mms_conv_route: MMS_CONV_ROUTE_FAST) with
 *             workgroups whose output pixels are whole pooling windows; the sums of a workgroup go to on-chip memory
 *             and are pooled and finished there.  y never reaches device memory and no workspace is needed.
 *             Reached where the forward is FAST and at least `ph` whole rows of y fit a workgroup's 256 pixels;
 *             taken there unless measured slower than the SEQUENCE: workgroups of whole small images on a grid of
 *             fewer than 10, or a band of rows the window made lower than the convolution's own on more than 2048.
 * Every element's sum is the convolution route's own (mms_conv.h: a fixed function of the shape), the window is added
 * in the order above on both routes and the finish is one expression shared by both: no atomics, the same words on
 * every run, for every alignment of the arrays and whatever the workspace held.  The two routes give the same words
 * wherever they cut the input channels into the same chunks (network_v4's two stages do).
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   whatever mms_conv_forward_* refuses, with its code (MMS_ERR_INVALID_ARG / MMS_ERR_UNSUPPORTED for the shape, then,
 *                        with N > 0, MMS_ERR_INVALID_ARG for a NULL x, weight or top, or top == x);
 *   MMS_ERR_INVALID_ARG  ph or pw < 1; OH % ph or OW % pw != 0; with N > 0, a NULL mean, var, scale or shift; top or
 *                        save_pool equal to an input (x, weight, bias, mean, var, scale, shift) or to each other;
 *   MMS_ERR_WORKSPACE    on the SEQUENCE route, workspace NULL or smaller than the query;
 *   N == 0               MMS_OK, nothing is written.
 */
#ifndef MMS_CONV_STAGE_H_
#define MMS_CONV_STAGE_H_

#include "mms_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_CONV_STAGE_ROUTE_NONE (-1)     /* the calls refuse this shape or window */
#define MMS_CONV_STAGE_ROUTE_SEQUENCE 0
#define MMS_CONV_STAGE_ROUTE_FUSED 1
/* The route of mms_conv_stage_forward_f32.  mms_conv_stage_forward_f64 and mms_conv_stage_forward_sequence_f32 always
 * take MMS_CONV_STAGE_ROUTE_SEQUENCE. */
int mms_conv_stage_route(const mms_conv_shape* shape, int ph, int pw);

/* Bytes of workspace for the call of the same element type: on the SEQUENCE route y, 2 K elements that receive the
 * BN call's save_mean / save_std, and a save_pool for a caller that passes NULL; 0 on the FUSED route, for a shape or
 * window the calls refuse and for N == 0.  mms_conv_stage_forward_sequence_f32 needs
 * mms_conv_stage_sequence_workspace_bytes, which is the same figure whatever the route. */
size_t mms_conv_stage_workspace_bytes(const mms_conv_shape* shape, int ph, int pw);
size_t mms_conv_stage_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw);
size_t mms_conv_stage_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw);

int mms_conv_stage_forward_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                               const float* bias, const float* mean, const float* var, const float* scale,
                               const float* shift, float* top, float* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream);
int mms_conv_stage_forward_f64(const mms_conv_shape* shape, int ph, int pw, const double* x, const double* weight,
                               const double* bias, const double* mean, const double* var, const double* scale,
                               const double* shift, double* top, double* save_pool, void* workspace,
                               size_t workspace_bytes, void* stream);

/* The float call on MMS_CONV_STAGE_ROUTE_SEQUENCE whatever mms_conv_stage_route says.  For a host that wants one
 * order at every shape, and for checking one route against the other. */
int mms_conv_stage_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, const float* x,
                                        const float* weight, const float* bias, const float* mean, const float* var,
                                        const float* scale, const float* shift, float* top, float* save_pool,
                                        void* workspace, size_t workspace_bytes, void* stream);

/* The float call on MMS_CONV_STAGE_ROUTE_FUSED wherever the fused launch reaches, whatever the measured rules of
 * mms_conv_stage_route say; MMS_ERR_UNSUPPORTED (after the refusals above) where it does not reach: the forward is not
 * FAST, or fewer than `ph` rows fit a workgroup.  No workspace.  For measuring one route against the other -- the
 * rules of mms_conv_stage_route rest on such measurements (tools/bench_conv_stage.py) -- and for testing the launch at
 * shapes the rules send to the sequence. */
int mms_conv_stage_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, const float* x, const float* weight,
                                     const float* bias, const float* mean, const float* var, const float* scale,
                                     const float* shift, float* top, float* save_pool, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_CONV_STAGE_H_ */
