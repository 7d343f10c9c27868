/* include/mms_train_tail.h -- the TRAIN-phase tail of the driver's nets, Convolution -> BN -> Pool -> TanH -> Flatten ->
 * Concat -> InnerProduct -> TanH -> Dropout -> InnerProduct -> SoftmaxWithLoss, as one forward call and one backward
 * call on the C ABI of libmms_hip.so.  The TEST-phase (scoring) counterpart is include/mms_score_tail.h.
 *
 * This header adds to include/mms_conv_stage_train.h, include/mms_head.h and include/mms_score_tail.h and changes
 * nothing in them: the shape struct (mms_score_tail_shape), the error codes, the stream convention and MMS_VERSION are
 * theirs.  All arrays are device memory, contiguous and row-major; a call enqueues its launches on `stream` and returns
 * without waiting.  Dtype is float (_f32) or double (_f64).
 *
 * With (OH, OW) from mms_conv_output_dims, the pooling window must be the whole map (ph == OH, pw == OW), so that
 * F0 = K (OH/ph) (OW/pw) = K and Flatten is a no-op: flt (N, K) is the stage's top.  `phase` must be MMS_HEAD_TRAIN.
 *
 *   forward   exactly these two calls, one after the other:
 *     mms_conv_stage_train_forward_*    (shape->conv, ph, pw, pool, bn_memory) on x, weight, bias, scale, shift,
 *                                       running_mean, running_var -> y, top = flt, save_pool, save_mean, save_std;
 *                                       the running_* update rules are that call's
 *     mms_head_forward_*                phase = MMS_HEAD_TRAIN, dropout_ratio; x0 = flt, x1 = overlap (N, F1), mask (N, H)
 *                                       the caller's Dropout mask -> h, prob, loss
 *     y (N, K, OH, OW), flt, save_pool (N, K), save_mean, save_std (K), h (N, H) and prob (N, C) are required outputs: the
 *     backward reads y, flt, save_pool, save_mean, save_std, h and prob.  loss (1) is optional and requires label;
 *     label (N) may be NULL (then no loss).  bias, b1, b2 may be NULL; overlap may be NULL only with F1 == 0.
 *
 *   backward  exactly mms_head_backward_* (x0 = flt, x1 = overlap, phase = MMS_HEAD_TRAIN) followed by
 *     mms_conv_stage_train_backward_* with top = flt and top_diff = the head's x0_diff, which is kept in the workspace.
 *     Every output may be NULL to skip it, at least one of the ten is required; each keeps the rule of the call that
 *     makes it:
 *       overlap_diff (N, F1)                    OVERWRITTEN   (the head's x1_diff; ignored with F1 == 0)
 *       w1_diff, b1_diff, w2_diff, b2_diff      ACCUMULATED
 *       bottom_diff, scale_diff, shift_diff     OVERWRITTEN
 *       weight_diff, bias_diff                  ACCUMULATED
 *     With bottom_diff, weight_diff, bias_diff, scale_diff and shift_diff all NULL the stage's backward is not run and
 *     x0_diff is not formed.  `shift` is read by MAX only and may be NULL for AVE.
 *     The backward has one route, the two calls, in both element types.
 *
 * Routes of the forward (mms_train_tail_route, the one place that decides; the launchers call it too):
 *   SEQUENCE  the two public calls above, each on the route it chooses itself.  All of double; float wherever the fused
 *             launches do not reach or have not been measured faster.
 *   FUSED     float only, two launches (three with a loss and more than 64 samples).
 *             Launch 1 is the convolution's fast route (mms_conv_route: MMS_CONV_ROUTE_FAST) with workgroups of whole
 *             images -- at most kTrainTailImages of them (csrc/train_tail.hip: one), the tail's own constant -- and the
 *             convolution's own cut of the input channels into chunks, so every word of y is the word
 *             mms_conv_forward_f32 writes.  Besides y a workgroup leaves in save_pool each (image, channel) window's raw
 *             pooled value (AVE: the window's y added in (h, w) order from 0, divided once by ph*pw; MAX: the scan's
 *             winner) and in the workspace, per channel, its partial sums of y and y*y, at slot
 *             [(channel * workgroups + workgroup) * 2 + {0, 1}].
 *             Launch 2 has ceil(N / 64) workgroups.  Each adds every channel's partials in the order of
 *             mms_conv_stage_train_forward_fused_f32's second launch (thread t of 256 the workgroups t, t + 256, ...
 *             ascending; a butterfly within each wave; the four waves ascending), forms mean, var and std, finishes
 *             its own 64 samples' pooled elements (save_pool and flt), and runs the head's fast forward on those rows:
 *             fc1 on the matrix pipe with tanh, the Dropout mask, fc2, softmax.  Workgroup 0 alone writes save_mean,
 *             save_std and the running_* update.
 *             loss: with one workgroup in launch 2 (N <= 64) its thread 0 adds the samples' terms in ascending n.  Else
 *             each sample's term and whether it counts go to the workspace and a third, one-thread launch adds them in
 *             ascending n.  The same chain either way.
 *             Reached where all of these hold: the convolution's forward is FAST (stride 1, pad 0, group 1, at most 64
 *             channels in and out); a workgroup's whole images are cut into the input-channel chunks the convolution's
 *             own launch cuts; the head is within its fast limits, K + F1 <= 128, H <= 64, C <= 16; both launches'
 *             on-chip memory fits the CU's 160 KB.
 *             Taken only where measured faster than the SEQUENCE beyond the spread of alternating passes
 *             (tools/bench_train_tail.py, profiles/train_tail_bench.txt; csrc/train_tail.hip names each threshold):
 *             with one image per workgroup, on 50 to 100 images of at most 128 pixels, AVE and MAX alike -- 1.27 and
 *             1.29 x at network_v4's tail at N = 50 and 100, 1.53 and 1.51 x at network_v3's, 1.16 and 1.17 x at
 *             network_v5's.  Measured slower, hence the SEQUENCE: 400 and 1517 images.  Not measured, hence the
 *             SEQUENCE: every other count, and larger images.
 *   What the two routes share: y word for word, and the chain of every element of save_pool, flt, h and prob, except for
 *   the two channel statistics, whose sums are taken in another order.  On real data the routes agree to the bar (1e-5 of
 *   float); wherever every partial sum is exact they give the same words.  loss is the same value up to the order of its
 *   sum over n: slabs on the SEQUENCE (mms_head.h), one ascending chain on FUSED.  Either route gives the same words on
 *   every run, for every alignment of the arrays and whatever the workspace held: no floating-point atomics, no arrival
 *   counters -- the launches are ordered by the stream -- and no word of the workspace is read before this call wrote it.
 *
 * Workspace.  One buffer serves both passes of a step; every part starts at a multiple of 16 bytes from its start:
 *   [stage]    round16(mms_conv_stage_train_workspace_bytes[_f64](conv, ph, pw, pool)): the stage call's, both passes
 *   [x0_diff]  round16(N * K elements): the backward's, between its two calls
 *   [head]     round16(mms_head_workspace_bytes[_f64]): the head call's, both passes
 *   The FUSED forward lays its own two parts over the same buffer from its start:
 *   [partials] round16(2 * K * workgroups floats), workgroups = ceil(N / images per workgroup)
 *   [loss]     round16(N floats + N ints): each sample's term and whether it counts
 *   and the FUSED figure is the larger of the two layouts.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing.  In this
 * order, the first that applies:
 *   MMS_ERR_INVALID_ARG  a NULL shape; a pool that is neither MMS_STAGE_POOL_AVE nor MMS_STAGE_POOL_MAX;
 *   whatever the stage call refuses of the shape and the window, with its code (the convolution's MMS_ERR_INVALID_ARG /
 *                        MMS_ERR_UNSUPPORTED, then MMS_ERR_INVALID_ARG for a window that does not tile the map);
 *   MMS_ERR_INVALID_ARG  a window that is not the whole map (ph != OH or pw != OW; F0 is K by construction, so a w1 of
 *                        another width cannot be stated); phase != MMS_HEAD_TRAIN;
 *   MMS_ERR_INVALID_ARG  whatever mms_head_*_* refuses of (N, F0, F1, H, C, dropout_ratio, normalization);
 *   N == 0               MMS_OK, nothing is written;
 *   MMS_ERR_INVALID_ARG  forward: a NULL x, weight, scale, shift, running_mean, running_var, w1, mask, w2, y, flt,
 *                        save_pool, save_mean, save_std, h or prob; overlap == NULL with F1 > 0; loss without label;
 *                        backward: a NULL x, weight, y, flt, save_pool, scale, save_mean, save_std, w1, w2, mask, h, prob
 *                        or label; shift == NULL with MAX; overlap == NULL with F1 > 0; no output at all;
 *                        both: any two arrays of the call at the same address, the workspace included;
 *   MMS_ERR_UNSUPPORTED  mms_train_tail_forward_fused_f32 where the fused launches do not reach;
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query.
 */
#ifndef MMS_TRAIN_TAIL_H_
#define MMS_TRAIN_TAIL_H_

#include "mms_conv_stage_train.h"
#include "mms_head.h"
#include "mms_score_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_TRAIN_TAIL_ROUTE_NONE (-1)     /* the calls refuse this shape */
#define MMS_TRAIN_TAIL_ROUTE_SEQUENCE 0
#define MMS_TRAIN_TAIL_ROUTE_FUSED 1
/* The route of mms_train_tail_forward_f32.  mms_train_tail_forward_f64 and mms_train_tail_forward_sequence_f32 always
 * take MMS_TRAIN_TAIL_ROUTE_SEQUENCE. */
int mms_train_tail_route(const mms_score_tail_shape* shape);

/* Bytes of workspace that cover BOTH passes of a step with the calls of the same element type, on the route the forward
 * chooses (layout above).  0 for a shape the calls refuse and for N == 0.  mms_train_tail_sequence_workspace_bytes is the
 * float figure with the forward on the SEQUENCE whatever the route (for mms_train_tail_forward_sequence_f32),
 * mms_train_tail_fused_workspace_bytes the one with the forward FUSED (for mms_train_tail_forward_fused_f32; 0 where
 * that call does not reach). */
size_t mms_train_tail_workspace_bytes(const mms_score_tail_shape* shape);
size_t mms_train_tail_workspace_bytes_f64(const mms_score_tail_shape* shape);
size_t mms_train_tail_sequence_workspace_bytes(const mms_score_tail_shape* shape);
size_t mms_train_tail_fused_workspace_bytes(const mms_score_tail_shape* shape);

int mms_train_tail_forward_f32(const mms_score_tail_shape* shape, int phase, float bn_memory, float dropout_ratio,
                               const float* x, const float* weight, const float* bias, const float* scale,
                               const float* shift, float* running_mean, float* running_var, const float* overlap,
                               const float* w1, const float* b1, const unsigned int* mask, const float* w2,
                               const float* b2, const float* label, float* y, float* flt, float* save_pool,
                               float* save_mean, float* save_std, float* h, float* prob, float* loss, void* workspace,
                               size_t workspace_bytes, void* stream);
int mms_train_tail_forward_f64(const mms_score_tail_shape* shape, int phase, double bn_memory, float dropout_ratio,
                               const double* x, const double* weight, const double* bias, const double* scale,
                               const double* shift, double* running_mean, double* running_var, const double* overlap,
                               const double* w1, const double* b1, const unsigned int* mask, const double* w2,
                               const double* b2, const double* label, double* y, double* flt, double* save_pool,
                               double* save_mean, double* save_std, double* h, double* prob, double* loss,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The float forward on MMS_TRAIN_TAIL_ROUTE_SEQUENCE whatever mms_train_tail_route says.  For a host that wants the two
 * calls' own launches at every shape, and for checking one route against the other. */
int mms_train_tail_forward_sequence_f32(const mms_score_tail_shape* shape, int phase, float bn_memory,
                                        float dropout_ratio, const float* x, const float* weight, const float* bias,
                                        const float* scale, const float* shift, float* running_mean,
                                        float* running_var, const float* overlap, const float* w1, const float* b1,
                                        const unsigned int* mask, const float* w2, const float* b2, const float* label,
                                        float* y, float* flt, float* save_pool, float* save_mean, float* save_std,
                                        float* h, float* prob, float* loss, void* workspace, size_t workspace_bytes,
                                        void* stream);

/* The float forward on MMS_TRAIN_TAIL_ROUTE_FUSED wherever the fused launches reach, whatever the measured rules of
 * mms_train_tail_route say; MMS_ERR_UNSUPPORTED (after the refusals of the arguments) where they do not.  For measuring
 * one route against the other (tools/bench_train_tail.py) and for testing the launches at shapes the rules send to the
 * sequence. */
int mms_train_tail_forward_fused_f32(const mms_score_tail_shape* shape, int phase, float bn_memory, float dropout_ratio,
                                     const float* x, const float* weight, const float* bias, const float* scale,
                                     const float* shift, float* running_mean, float* running_var, const float* overlap,
                                     const float* w1, const float* b1, const unsigned int* mask, const float* w2,
                                     const float* b2, const float* label, float* y, float* flt, float* save_pool,
                                     float* save_mean, float* save_std, float* h, float* prob, float* loss,
                                     void* workspace, size_t workspace_bytes, void* stream);

int mms_train_tail_backward_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio, float loss_weight,
                                const float* x, const float* weight, const float* y, const float* flt,
                                const float* save_pool, const float* scale, const float* shift, const float* save_mean,
                                const float* save_std, const float* overlap, const float* w1, const float* w2,
                                const unsigned int* mask, const float* h, const float* prob, const float* label,
                                float* bottom_diff, float* weight_diff, float* bias_diff, float* scale_diff,
                                float* shift_diff, float* overlap_diff, float* w1_diff, float* b1_diff, float* w2_diff,
                                float* b2_diff, void* workspace, size_t workspace_bytes, void* stream);
int mms_train_tail_backward_f64(const mms_score_tail_shape* shape, int phase, float dropout_ratio, double loss_weight,
                                const double* x, const double* weight, const double* y, const double* flt,
                                const double* save_pool, const double* scale, const double* shift,
                                const double* save_mean, const double* save_std, const double* overlap,
                                const double* w1, const double* w2, const unsigned int* mask, const double* h,
                                const double* prob, const double* label, double* bottom_diff, double* weight_diff,
                                double* bias_diff, double* scale_diff, double* shift_diff, double* overlap_diff,
                                double* w1_diff, double* b1_diff, double* w2_diff, double* b2_diff, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_TRAIN_TAIL_H_ */
