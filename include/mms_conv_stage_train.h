/* include/mms_conv_stage_train.h -- one TRAIN-phase stage Convolution -> BN -> Pool -> TanH of network_v3 / v4 / v4_2 /
 * v5 on the C ABI of libmms_hip.so: the forward as one call and the backward as one call, for AvePool and MaxPool.
 * The TEST-phase halves are include/mms_conv_stage.h (AVE) and include/mms_conv_maxpool_stage.h (MAX).
 *
 * This header adds to include/mms_conv.h, include/mms_bn_maxpool.h and include/mms.h and changes nothing in them: the
 * shape struct, the error codes, the stream convention and MMS_VERSION are theirs.  All arrays are device memory,
 * contiguous and row-major; a call enqueues its launches on `stream` and returns without waiting.
 *
 * With (OH, OW) from mms_conv_output_dims and a pooling window (ph, pw) that tiles (OH, OW) (OH % ph == 0,
 * OW % pw == 0: the rule of mms_bn_pool_tanh_*), `pool` one of MMS_STAGE_POOL_*:
 *
 *   forward   exactly these two calls, one after the other:
 *     mms_conv_forward_*                 y = conv(x, weight) (+ bias)            (N, K, OH, OW), into the caller's y
 *     mms_bn_pool_tanh_forward_*         (AVE) or mms_bn_maxpool_tanh_forward_* (MAX) on y with phase = 0 (TRAIN) and
 *                                        every rule of those calls: mean and var from sum y and sum y*y over the
 *                                        channel, var = E[y*y] - mean*mean NOT clamped, std = sqrt(var + 1e-9),
 *                                        running = (1 - bn_memory)*batch + bn_memory*running, in place; MAX scans a
 *                                        window in (h, w) order from its first element, keeps the larger for
 *                                        scale[k] > 0, the smaller for scale[k] < 0, the first for scale[k] == 0, and
 *                                        a NaN never wins a comparison.
 *     outputs: y, top, save_pool (N, K, OH/ph, OW/pw), save_mean, save_std (K); running_mean, running_var (K) are
 *     updated.  All are required: the backward reads y, top, save_pool, save_mean and save_std.
 *
 *   backward  exactly these two calls, one after the other:
 *     mms_bn_pool_tanh_backward_*        (AVE) or mms_bn_maxpool_tanh_backward_* (MAX) on y: dy into the workspace
 *     mms_conv_backward_*                with top_diff = dy
 *     outputs, each may be NULL to skip it, at least one required; each keeps the rule of the call that makes it:
 *       bottom_diff (N, C, H, W)           OVERWRITTEN   (mms_conv_backward_*)
 *       weight_diff (K, C/group, kh, kw)   ACCUMULATED: += this batch's sum   (mms_conv_backward_*)
 *       bias_diff   (K)                    ACCUMULATED: += this batch's sum   (mms_conv_backward_*)
 *       scale_diff, shift_diff (K)         OVERWRITTEN   (mms_bn_*pool_tanh_backward_*)
 *     With bottom_diff, weight_diff and bias_diff all NULL the convolution's backward is not run and dy is not formed.
 *     `shift` is read by MAX only (its mask is a property of BN's output) and may be NULL for AVE.
 *
 *   x (N, C, H, W)   weight (K, C/group, kh, kw)   bias (K) or NULL   scale, shift (K)   top_diff (N, K, OH/ph, OW/pw)
 *
 * Routes of the forward (mms_conv_stage_train_route, the one place that decides; the launchers call it too):
 *   SEQUENCE  the two public calls above, their workspaces carved from the caller's.  All of double; float wherever
 *             the fused launches do not reach or have not been measured faster.
 *   FUSED     float only, two launches where the SEQUENCE has three.
 *             Launch 1 is the convolution's fast route (mms_conv_route: MMS_CONV_ROUTE_FAST) with workgroups whose
 *             output pixels are whole pooling windows and with the convolution's own cut of the input channels into
 *             chunks, so every word of y is the word mms_conv_forward_f32 writes: the same chain, the bias added
 *             after.  Besides y, a workgroup leaves (a) in save_pool each of its windows' raw pooled value -- AVE: the
 *             window's y added in (h, w) order from 0, divided once by ph*pw; MAX: the scan's winner -- and (b) in the
 *             workspace, per channel, its partial sums of y and y*y over its real pixels, at slot
 *             [(channel * workgroups + workgroup) * 2 + {0, 1}], workgroup = image group * bands + band.
 *             Launch 2 is pooled-size: per channel it adds the partials, forms mean and var, updates the running
 *             blobs, writes save_mean / save_std and finishes every pooled element in place (save_pool, top).
 *             Order of a channel's sums (a function of the shape alone; no atomics):
 *               in a workgroup of launch 1, T = 256 / (16 MT) threads serve a channel (MT = 1, 2, 4 for K <= 16, 32,
 *               64); thread j takes the workgroup's windows j, j + T, ... of that channel in (image, window row,
 *               window column) order and adds each window's elements in (h, w) order into ONE running sum of y and one
 *               of y*y; the T sums are then added pairwise: lanes 1 apart, then 2 apart (, 4, 8);
 *               in launch 2, thread t of 256 adds the partials of workgroups t, t + 256, ... in ascending order; the
 *               256 sums are added within each wave of 64 as a butterfly (32, 16, 8, 4, 2, 1 apart) and the four
 *               waves in ascending order.
 *             Reached where mms_conv_stage_forward_fused_f32 reaches -- the forward is FAST and at least `ph` whole
 *             rows of y fit a workgroup's 256 pixels -- and such a band with the convolution's own chunk of input
 *             channels fits the 64 KB of on-chip memory (it does at every stage of the four nets; where it does not,
 *             y could not be the convolution's words, and the forced call says MMS_ERR_UNSUPPORTED).
 *             Taken only where measured faster than the SEQUENCE by more than the run-to-run spread
 *             (profiles/conv_stage_train_bench.txt; the classes and their thresholds are listed at
 *             mms_conv_stage_train_route below).
 *   What the two routes share: y word for word; the window scan and the finish (one definition each).  The order of
 *   the statistics' sums differs, so on real data top, save_pool, save_mean, save_std and the running blobs agree to
 *   the bar (1e-5 of float), not to the word; wherever every partial sum is exact they are the same words.  Either
 *   route gives the same words on every run, for every alignment of the arrays and whatever the workspace held; no
 *   word of the workspace is read before this call wrote it.
 *
 * The backward has one route: the two calls.  (Forming dy inside the convolution's backward loaders is not done.)
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   whatever mms_conv_forward_* / mms_conv_backward_* refuse for the shape, with their codes (MMS_ERR_INVALID_ARG /
 *                        MMS_ERR_UNSUPPORTED) and first;
 *   MMS_ERR_INVALID_ARG  pool not one of MMS_STAGE_POOL_*; ph or pw < 1; OH % ph or OW % pw != 0; then N == 0 is
 *                        MMS_OK with nothing written; with N > 0: a NULL required array (forward: all but bias;
 *                        backward: every input but shift for AVE, and at least one output); an output equal to an
 *                        input or to another output (the running blobs count as outputs);
 *   MMS_ERR_UNSUPPORTED  the forced fused call where the fused launches do not reach (after the rules above);
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query where one is needed (a backward with only
 *                        scale_diff / shift_diff on BN's one-launch route needs none).
 */
#ifndef MMS_CONV_STAGE_TRAIN_H_
#define MMS_CONV_STAGE_TRAIN_H_

#include "mms_bn_maxpool.h"
#include "mms_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_STAGE_POOL_AVE 0
#define MMS_STAGE_POOL_MAX 1

#define MMS_CONV_STAGE_TRAIN_ROUTE_NONE (-1)     /* the calls refuse this shape, window or pool */
#define MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE 0
#define MMS_CONV_STAGE_TRAIN_ROUTE_FUSED 1
/* The route of mms_conv_stage_train_forward_f32.  mms_conv_stage_train_forward_f64 and
 * mms_conv_stage_train_forward_sequence_f32 always take MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE.
 * FUSED, by the pooling method, what a workgroup of launch 1 holds and the number of workgroups, each span the counts
 * at which profiles/conv_stage_train_bench.txt records a median gain beyond the run-to-run spread:
 *   AVE, a band of rows of one image     450 workgroups (network_v4's first stage at the training batch of 50)
 *   MAX, a band of rows of one image     450 to 10619 workgroups
 * Measured slower or level, hence the SEQUENCE: AVE bands from 1800 workgroups on, AVE and MAX workgroups of several
 * whole images, MAX workgroups of one whole image.  Not measured, hence the SEQUENCE: AVE workgroups of one whole
 * image, and every count outside the spans above. */
int mms_conv_stage_train_route(const mms_conv_shape* shape, int ph, int pw, int pool);

/* Bytes of workspace that cover BOTH passes of a step with the calls of the same element type: the larger of what the
 * forward (on the route mms_conv_stage_train_route names) and the backward (with every output) need.
 *   forward, SEQUENCE   mms_bn_pool_tanh_workspace_bytes[_f64](N, K, OH, OW, ph, pw)
 *   forward, FUSED      2 * K * workgroups floats
 *   backward            dy (N K OH OW elements, rounded up to 16 bytes), then the BN call's workspace (rounded up to 16
 *                       bytes), then mms_conv_workspace_bytes[_f64]
 * 0 for a shape, window or pool the calls refuse and for N == 0.  mms_conv_stage_train_sequence_workspace_bytes is
 * the float figure with the forward on the SEQUENCE whatever the route (for
 * mms_conv_stage_train_forward_sequence_f32), mms_conv_stage_train_fused_workspace_bytes the one with the forward
 * FUSED (for mms_conv_stage_train_forward_fused_f32; 0 where that call does not reach). */
size_t mms_conv_stage_train_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool);
size_t mms_conv_stage_train_workspace_bytes_f64(const mms_conv_shape* shape, int ph, int pw, int pool);
size_t mms_conv_stage_train_sequence_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool);
size_t mms_conv_stage_train_fused_workspace_bytes(const mms_conv_shape* shape, int ph, int pw, int pool);

int mms_conv_stage_train_forward_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                     const float* x, const float* weight, const float* bias, const float* scale,
                                     const float* shift, float* running_mean, float* running_var, float* y, float* top,
                                     float* save_pool, float* save_mean, float* save_std, void* workspace,
                                     size_t workspace_bytes, void* stream);
int mms_conv_stage_train_forward_f64(const mms_conv_shape* shape, int ph, int pw, int pool, double bn_memory,
                                     const double* x, const double* weight, const double* bias, const double* scale,
                                     const double* shift, double* running_mean, double* running_var, double* y,
                                     double* top, double* save_pool, double* save_mean, double* save_std,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* The float forward on MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE whatever mms_conv_stage_train_route says.  For a host that
 * wants one order at every shape, and for checking one route against the other. */
int mms_conv_stage_train_forward_sequence_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                              const float* x, const float* weight, const float* bias,
                                              const float* scale, const float* shift, float* running_mean,
                                              float* running_var, float* y, float* top, float* save_pool,
                                              float* save_mean, float* save_std, void* workspace,
                                              size_t workspace_bytes, void* stream);

/* The float forward on MMS_CONV_STAGE_TRAIN_ROUTE_FUSED wherever the fused launches reach, whatever the measured rules
 * of mms_conv_stage_train_route say; MMS_ERR_UNSUPPORTED (after the argument rules) where they do not.  For measuring
 * one route against the other -- the rules rest on such measurements (tools/bench_conv_stage_train.py) -- and for
 * testing the launches at shapes the rules send to the sequence. */
int mms_conv_stage_train_forward_fused_f32(const mms_conv_shape* shape, int ph, int pw, int pool, float bn_memory,
                                           const float* x, const float* weight, const float* bias, const float* scale,
                                           const float* shift, float* running_mean, float* running_var, float* y,
                                           float* top, float* save_pool, float* save_mean, float* save_std,
                                           void* workspace, size_t workspace_bytes, void* stream);

int mms_conv_stage_train_backward_f32(const mms_conv_shape* shape, int ph, int pw, int pool, const float* x,
                                      const float* weight, const float* y, const float* top, const float* top_diff,
                                      const float* save_pool, const float* scale, const float* shift,
                                      const float* save_mean, const float* save_std, float* bottom_diff,
                                      float* weight_diff, float* bias_diff, float* scale_diff, float* shift_diff,
                                      void* workspace, size_t workspace_bytes, void* stream);
int mms_conv_stage_train_backward_f64(const mms_conv_shape* shape, int ph, int pw, int pool, const double* x,
                                      const double* weight, const double* y, const double* top, const double* top_diff,
                                      const double* save_pool, const double* scale, const double* shift,
                                      const double* save_mean, const double* save_std, double* bottom_diff,
                                      double* weight_diff, double* bias_diff, double* scale_diff, double* shift_diff,
                                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_CONV_STAGE_TRAIN_H_ */
