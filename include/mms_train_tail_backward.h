/* include/mms_train_tail_backward.h -- a routed and a fused backward of the TRAIN-phase tail Convolution -> BN -> Pool ->
 * TanH -> head on the C ABI of libmms_hip.so, in float.  This header adds to include/mms_train_tail.h and changes nothing
 * in it: the shape struct, the error codes, the route constants (MMS_TRAIN_TAIL_ROUTE_*), the stream convention and
 * MMS_VERSION are its own, and mms_train_tail_backward_f32 / _f64 keep their one route, the two public calls.  double
 * stays on mms_train_tail_backward_f64.
 *
 * Both calls below take the argument list of mms_train_tail_backward_f32 and keep its rules: which outputs may be NULL
 * (each of the ten, at least one required), which are OVERWRITTEN (bottom_diff, scale_diff, shift_diff, overlap_diff)
 * and which ACCUMULATED (weight_diff, bias_diff, w1_diff, b1_diff, w2_diff, b2_diff), `shift` read by MAX only, and its
 * refusals in its order (include/mms_train_tail.h), with MMS_ERR_UNSUPPORTED -- mms_train_tail_backward_fused_f32 where
 * the fused launches do not reach -- between the arguments' refusals and MMS_ERR_WORKSPACE.  A call that does not return
 * MMS_OK writes nothing; N == 0 returns MMS_OK and writes nothing.
 *
 * Routes (mms_train_tail_backward_route, the one place that decides; the launchers call it too):
 *   SEQUENCE  mms_train_tail_backward_f32 itself.
 *   FUSED     The window is the whole map (S = OH OW, M = N S), so with g = x0_diff (1 - flt^2), x0_diff the head's
 *             gradient w.r.t. flt, and p^ = save_pool (the forward leaves the pooled value already normalised there,
 *             (pooled y - mean) / std), BN -> Pool -> TanH's backward needs pooled-size sums only:
 *               shift_diff[k] = sum_n g[n,k]        scale_diff[k] = sum_n g[n,k] p^[n,k]
 *               dy[n,k,oy,ox] = A0[k] + B[k] y[n,k,oy,ox] + cg[n,k]   (MAX: cg at the mask's pixel alone)
 *             and no (N, K, OH, OW) top_diff of the convolution is written or read: both convolution launches form it
 *             from y and 2 K + N K coefficients as they stage it.  Launches, ordered by the stream:
 *             1. mms_head_backward_f32 on its fast route (one launch; its ordered reduce behind it with more than 64
 *                samples and a parameter diff): overlap_diff, w1_diff, b1_diff, w2_diff and b2_diff are that call's
 *                words; x0_diff goes to the workspace.
 *             2. The coefficients.  Workgroup 0: thread k adds channel k's g and g p^ over n = 0, 1, ..., N - 1, one
 *                ascending chain each -- the one order -- and it alone writes scale_diff, shift_diff, A0 and B.  The other
 *                workgroups: one thread per (n, k) writes cg and, MAX, the mask's pixel -- the first pixel, in (h, w)
 *                order, whose BN output is the BN output of the window's extremum, as mms_bn_maxpool_tanh_backward_f32
 *                finds it.
 *             3. bottom_diff: the convolution's fast bottom_diff product (mms_conv_route: MMS_CONV_ROUTE_FAST) with
 *                workgroups of whole images, at most kTrainTailBackwardImages of them (csrc/train_tail_backward.hip:
 *                one), the tail's own constant, and the convolution's own order of every sum.
 *             4. The parameter diffs: the convolution's fast parameter-diff launch with the same cut of images; the
 *                image groups are dealt in ascending runs to at most 64 slabs, whose partial sums go to the workspace.
 *                bias_diff comes from this sweep -- each channel's dy added pixel by pixel -- not from the coefficients.
 *             5. One reduce adds the slabs in ascending order and then into weight_diff / bias_diff.
 *             A launch none of whose outputs is asked for is not issued.  No floating-point atomics, no arrival
 *             counters, and no word of the workspace is read before this call wrote it: the same words on every run,
 *             for every alignment of the arrays, whatever the workspace held.
 *             Reached where all of these hold: 1 <= N <= 256; the convolution's bottom_diff and parameter-diff passes
 *             are FAST (stride 1, pad 0, group 1, at most 64 channels in and out); an image is whole in a workgroup of
 *             either launch (the convolution's plans do not cut it into bands of rows: every image of at most 128
 *             pixels in and out, and larger ones of at most 256 whose rows fit); the head is within its fast limits,
 *             K + F1 <= 128, H <= 64, C <= 16; every launch's on-chip memory fits the CU's 160 KB.
 *             Taken only where measured faster than the SEQUENCE beyond the spread of alternating passes
 *             (tools/bench_train_tail_backward.py, profiles/train_tail_backward_bench.txt;
 *             csrc/train_tail_backward.hip names each threshold), on images of at most 128 pixels in and out, the
 *             only class measured (larger images are the SEQUENCE): with one image per workgroup
 *             (two and three were measured slower at every net and N), AVE on 50 to 100 images -- 1.23 and 1.10 x at
 *             network_v4's tail at N = 50 and 100 -- and MAX on 50 -- 1.11 x at network_v3's tail, 1.31 x at
 *             network_v5's.  Not faster beyond the spread, hence the SEQUENCE: 256 images (AVE 1.00 x, v5 0.86 x) and
 *             MAX at 100 (v3 1.17 x; v5 1.12 x in one run, ranges overlapping in another).  Every other workgroup
 *             count, unmeasured ones included, is the SEQUENCE.
 *   The two routes agree to the bar (1e-5 of float) on real data and give the same words wherever every product and sum
 *   is exact.
 *
 * Workspace of the FUSED route; every part starts at a multiple of 16 bytes from its start:
 *   [x0_diff]  round16(N K floats)
 *   [head]     round16(mms_head_workspace_bytes)
 *   [coef]     round16((2 K + N K) floats + N K ints): A0, B, cg, the mask's pixels
 *   [part]     round16(slabs (K C kh kw + K) floats)
 */
#ifndef MMS_TRAIN_TAIL_BACKWARD_H_
#define MMS_TRAIN_TAIL_BACKWARD_H_

#include "mms_train_tail.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The route of mms_train_tail_backward_routed_f32: MMS_TRAIN_TAIL_ROUTE_NONE, _SEQUENCE or _FUSED. */
int mms_train_tail_backward_route(const mms_score_tail_shape* shape);

/* Bytes that cover mms_train_tail_backward_routed_f32 on the route it takes; never below
 * mms_train_tail_workspace_bytes(shape), so one buffer still serves both passes of a step.  0 for a shape the calls
 * refuse and for N == 0. */
size_t mms_train_tail_backward_workspace_bytes(const mms_score_tail_shape* shape);
/* Bytes of mms_train_tail_backward_fused_f32 (layout above); 0 where that call does not reach. */
size_t mms_train_tail_backward_fused_workspace_bytes(const mms_score_tail_shape* shape);

/* FUSED where mms_train_tail_backward_route says so, else mms_train_tail_backward_f32 itself. */
int mms_train_tail_backward_routed_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio,
                                       float loss_weight, const float* x, const float* weight, const float* y,
                                       const float* flt, const float* save_pool, const float* scale, const float* shift,
                                       const float* save_mean, const float* save_std, const float* overlap,
                                       const float* w1, const float* w2, const unsigned int* mask, const float* h,
                                       const float* prob, const float* label, float* bottom_diff, float* weight_diff,
                                       float* bias_diff, float* scale_diff, float* shift_diff, float* overlap_diff,
                                       float* w1_diff, float* b1_diff, float* w2_diff, float* b2_diff, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* FUSED wherever the fused launches reach, whatever the measured rule says; MMS_ERR_UNSUPPORTED (after the refusals of
 * the arguments) where they do not.  For measuring one route against the other and for testing the launches at shapes
 * the rule sends to the sequence. */
int mms_train_tail_backward_fused_f32(const mms_score_tail_shape* shape, int phase, float dropout_ratio,
                                      float loss_weight, const float* x, const float* weight, const float* y,
                                      const float* flt, const float* save_pool, const float* scale, const float* shift,
                                      const float* save_mean, const float* save_std, const float* overlap,
                                      const float* w1, const float* w2, const unsigned int* mask, const float* h,
                                      const float* prob, const float* label, float* bottom_diff, float* weight_diff,
                                      float* bias_diff, float* scale_diff, float* shift_diff, float* overlap_diff,
                                      float* w1_diff, float* b1_diff, float* w2_diff, float* b2_diff, void* workspace,
                                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_TRAIN_TAIL_BACKWARD_H_ */
