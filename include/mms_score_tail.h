/* include/mms_score_tail.h -- the scoring (TEST-phase) tail of the driver's nets, Convolution -> BN -> Pool -> TanH ->
 * Flatten -> Concat -> InnerProduct -> TanH -> InnerProduct -> Softmax (/ SoftmaxWithLoss), as one call on the C ABI of
 * libmms_hip.so.
 *
 * This header adds to include/mms_conv_stage.h, include/mms_conv_maxpool_stage.h and include/mms_head.h and changes
 * nothing in them: the convolution's shape struct, the error codes, the stream convention and MMS_VERSION are theirs.
 * All arrays are device memory, contiguous and row-major; a call enqueues its launches on `stream` and returns without
 * waiting.  Dtype is float (_f32) or double (_f64).
 *
 * With (OH, OW) from mms_conv_output_dims and a pooling window (ph, pw) that tiles (OH, OW), the tail is exactly what
 * these two calls compute one after the other, flt and h being intermediates the caller need not receive:
 *
 *   mms_conv_stage_forward_*            pool == MMS_STAGE_POOL_AVE, or
 *   mms_conv_maxpool_stage_forward_*    pool == MMS_STAGE_POOL_MAX:  window (ph, pw), save_pool = NULL,
 *                                       top = flt (N, F0), F0 = K (OH/ph) (OW/pw): Flatten is a no-op
 *   mms_head_forward_*                  phase = MMS_HEAD_TEST, x0 = flt, x1 = overlap (N, F1), mask = NULL:
 *                                       h = tanh([flt | overlap] . w1^T + b1)   prob = softmax(h . w2^T + b2)
 *                                       loss as include/mms_head.h states it, from label
 *
 *   x (N, C, H, W)   weight (K, C/group, kh, kw)   bias (K) or NULL   mean, var, scale, shift (K)
 *   overlap (N, F1), F1 may be 0   w1 (H, F0 + F1)   b1 (H) or NULL   w2 (C, H)   b2 (C) or NULL   label (N) or NULL
 *   prob (N, C) is the only required output.  flt (N, F0), h (N, H) and loss (1) are optional: NULL skips them.
 *   loss requires label.
 *
 * Two routes (mms_score_tail_route, the one place that decides; the launchers call it too):
 *   SEQUENCE  the two calls above, each on the route it chooses itself; flt and h live in the caller's workspace when
 *             the caller passed NULL.  Every shape those calls accept -- pooled maps larger than 1 x 1 included -- and
 *             all of double.
 *   FUSED     float only.  One launch for prob (and flt and h where asked): the convolution's fast route
 *             (mms_conv_route: MMS_CONV_ROUTE_FAST) with workgroups of whole images; a workgroup pools and finishes its
 *             images on chip, keeps their flt rows there and runs the head's fast forward on them.  Neither the
 *             convolution's map nor an flt or h the caller did not ask for reaches device memory.
 *             Reached where all of these hold: the convolution's forward is FAST; the window is the whole map
 *             (OH == ph, OW == pw); whole images fit a workgroup's 256 pixels and are cut into the input-channel chunks
 *             the convolution's own launch cuts; the head is within its fast limits, K + F1 <= 128, H <= 64, C <= 16.
 *             Taken only where measured faster than the SEQUENCE beyond the spread of alternating passes
 *             (tools/bench_score_tail.py, profiles/score_tail_bench.txt); csrc/score_tail.hip names each threshold.
 *             With label and loss the launch writes each sample's loss term and whether its label counts to the
 *             workspace, and a second, one-thread launch adds them in ascending sample order and divides.
 * Every element's chain is the underlying calls' chain: the convolution's k = (c, i, j) ascending, then the bias; the
 * window in (h, w) order from 0, or the MAX scan; the finish shared with the stage calls; fc1's features ascending four
 * per step; fc2 and the softmax as the head's fast route.  None depends on which images share a workgroup: no
 * floating-point atomics, the same words on every run, for every alignment of the arrays and whatever the workspace
 * held, and wherever FUSED reaches it gives the words of the SEQUENCE for flt, h and prob.  loss is the same value up to
 * the order of its sum over n: slabs on the SEQUENCE (mms_head.h), one ascending chain on FUSED.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing.  In this
 * order, the first that applies:
 *   MMS_ERR_INVALID_ARG  a NULL shape; a pool that is neither MMS_STAGE_POOL_AVE nor MMS_STAGE_POOL_MAX;
 *   whatever the stage call refuses of the shape and the window, with its code (mms_conv_stage.h: the convolution's
 *                        MMS_ERR_INVALID_ARG / MMS_ERR_UNSUPPORTED, then MMS_ERR_INVALID_ARG for the window);
 *   whatever mms_head_forward_* refuses of (N, F0, F1, H, C, normalization), MMS_ERR_INVALID_ARG;
 *   N == 0               MMS_OK, nothing is written;
 *   MMS_ERR_INVALID_ARG  a NULL x, weight, mean, var, scale or shift; a NULL w1, w2 or prob; overlap == NULL with
 *                        F1 > 0; loss without label; an output (flt, h, prob, loss) that is an input or another output;
 *   MMS_ERR_UNSUPPORTED  mms_score_tail_forward_fused_f32 where the fused launch does not reach;
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query: on the SEQUENCE route always, on the FUSED route for
 *                        a call that has a loss.
 */
#ifndef MMS_SCORE_TAIL_H_
#define MMS_SCORE_TAIL_H_

#include "mms_conv.h"
#include "mms_head.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_STAGE_POOL_AVE 0               /* mms_conv_stage_*          */
#define MMS_STAGE_POOL_MAX 1               /* mms_conv_maxpool_stage_*  */

typedef struct mms_score_tail_shape {
  mms_conv_shape conv;       /* the last convolution; conv.N is the number of samples                   */
  int ph, pw;                /* pooling window = stride; tiles the convolution's (OH, OW)               */
  int pool;                  /* MMS_STAGE_POOL_AVE / MMS_STAGE_POOL_MAX                                 */
  int F1;                    /* width of overlap, the second Concat bottom; may be 0                    */
  int H;                     /* fc1 num_output                                                          */
  int C;                     /* fc2 num_output = number of classes, >= 1                                */
  int normalization;         /* MMS_HEAD_NORM_*                                                         */
  int has_ignore_label, ignore_label;
} mms_score_tail_shape;

#define MMS_SCORE_TAIL_ROUTE_NONE (-1)     /* the calls refuse this shape */
#define MMS_SCORE_TAIL_ROUTE_SEQUENCE 0
#define MMS_SCORE_TAIL_ROUTE_FUSED 1
/* The route of mms_score_tail_forward_f32.  mms_score_tail_forward_f64 and mms_score_tail_forward_sequence_f32 always
 * take MMS_SCORE_TAIL_ROUTE_SEQUENCE. */
int mms_score_tail_route(const mms_score_tail_shape* shape);

/* Bytes of workspace for the call of the same element type, whichever outputs it is given.  SEQUENCE: the stage call's
 * workspace, flt, h and the head call's workspace, each rounded up to 16 bytes.  FUSED: a float and an int per sample,
 * needed only by a call that has a loss.  0 for a shape the calls refuse and for N == 0.
 * mms_score_tail_forward_sequence_f32 needs mms_score_tail_sequence_workspace_bytes, which is the SEQUENCE figure
 * whatever the route; mms_score_tail_forward_fused_f32 needs the FUSED figure, 8 N, and only with a loss. */
size_t mms_score_tail_workspace_bytes(const mms_score_tail_shape* shape);
size_t mms_score_tail_workspace_bytes_f64(const mms_score_tail_shape* shape);
size_t mms_score_tail_sequence_workspace_bytes(const mms_score_tail_shape* shape);

int mms_score_tail_forward_f32(const mms_score_tail_shape* shape, const float* x, const float* weight, const float* bias,
                               const float* mean, const float* var, const float* scale, const float* shift,
                               const float* overlap, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* label, float* flt, float* h, float* prob, float* loss, void* workspace,
                               size_t workspace_bytes, void* stream);
int mms_score_tail_forward_f64(const mms_score_tail_shape* shape, const double* x, const double* weight,
                               const double* bias, const double* mean, const double* var, const double* scale,
                               const double* shift, const double* overlap, const double* w1, const double* b1,
                               const double* w2, const double* b2, const double* label, double* flt, double* h,
                               double* prob, double* loss, void* workspace, size_t workspace_bytes, void* stream);

/* The float call on MMS_SCORE_TAIL_ROUTE_SEQUENCE whatever mms_score_tail_route says.  For a host that wants the two
 * calls' own launches at every shape, and for checking one route against the other. */
int mms_score_tail_forward_sequence_f32(const mms_score_tail_shape* shape, const float* x, const float* weight,
                                        const float* bias, const float* mean, const float* var, const float* scale,
                                        const float* shift, const float* overlap, const float* w1, const float* b1,
                                        const float* w2, const float* b2, const float* label, float* flt, float* h,
                                        float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream);

/* The float call on MMS_SCORE_TAIL_ROUTE_FUSED wherever the fused launch reaches, whatever the measured rules of
 * mms_score_tail_route say; MMS_ERR_UNSUPPORTED (after the refusals of the arguments) where it does not reach.  For
 * measuring one route against the other -- the rules of mms_score_tail_route rest on such measurements
 * (tools/bench_score_tail.py) -- and for testing the launch at shapes the rules send to the sequence. */
int mms_score_tail_forward_fused_f32(const mms_score_tail_shape* shape, const float* x, const float* weight,
                                     const float* bias, const float* mean, const float* var, const float* scale,
                                     const float* shift, const float* overlap, const float* w1, const float* b1,
                                     const float* w2, const float* b2, const float* label, float* flt, float* h,
                                     float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_SCORE_TAIL_H_ */
