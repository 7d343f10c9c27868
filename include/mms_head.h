/* include/mms_head.h -- network_v4's classifier head on the C ABI of libmms_hip.so: the reference's
 * Concat -> InnerProduct -> TanH (in place) -> Dropout -> InnerProduct -> SoftmaxWithLoss / Softmax as one call per pass.
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  All arrays are device memory,
 * contiguous and row-major; a call enqueues its launches on `stream` and returns without waiting.  Dtype is float
 * (_f32) or double (_f64).
 *
 *   x0 (N, F0) = Flatten(pool1)   x1 (N, F1) = overlap_feat, F1 may be 0   w1 (H, F0 + F1)   b1 (H) or NULL
 *   mask (N, H) unsigned 32-bit, 0 or 1: Dropout's rand_vec_               w2 (C, H)         b2 (C) or NULL
 *   label (N) Dtype, read as static_cast<int> (softmax_loss_layer.cpp:100), like the ranking calls of mms.h do
 *   h (N, H)   prob (N, C)   loss (1)
 *
 * Forward
 *   feat = [x0 | x1]                                   concat_layer.cpp:57-74, axis 1
 *   z1   = feat . w1^T + b1                            inner_product_layer.cpp:84-97
 *   h    = tanh(z1)                                    tanh_layer.cpp:11-19, in place: z1 itself is never stored
 *   d    = (h * Dtype(mask)) * scale  in TRAIN         dropout_layer.cpp:37-45, scale = Dtype(1. / (1. - ratio)),
 *        = h                          in TEST          dropout_layer.cpp:14-18.  The caller draws the mask; the library
 *                                                      draws no random numbers.  mask is ignored in TEST and may be NULL.
 *   z2   = d . w2^T + b2
 *   prob = softmax(z2), the row maximum subtracted     softmax_layer.cpp:28-60
 *   loss = - sum_n log(max(prob[n, label_n], Dtype(FLT_MIN))) / max(1, normalizer)     softmax_loss_layer.cpp:89-115
 *          over the labels that are not ignored; inner_num is 1.  normalizer (softmax_loss_layer.cpp:59-86): N for
 *          FULL and BATCH_SIZE, the number of labels not ignored for VALID, 1 for NONE.
 *   label == NULL is the deploy net, which has only Softmax: loss must then be NULL and no loss is computed.
 *   A label outside [0, C) is a DCHECK in the reference (undefined behaviour in its release build).  Here it is
 *   treated as IGNORED, in both passes and in the VALID count, so that no call indexes out of a row.
 *
 * Backward, from the saved h and prob (Caffe's blobs hold them)
 *   dz2  = (prob - onehot(label)) * (loss_weight / max(1, normalizer)), zero rows for ignored labels
 *                                                      softmax_loss_layer.cpp:118-149
 *   w2_diff += dz2^T . d      b2_diff += sum_n dz2     ACCUMULATED  (beta 1)
 *   dd   = dz2 . w2
 *   dh   = (dd * Dtype(mask)) * scale in TRAIN, dd in TEST                             dropout_layer.cpp:49-65
 *   dz1  = dh * (1 - h * h)                            tanh_layer.cpp:22-36
 *   w1_diff += dz1^T . feat   b1_diff += sum_n dz1     ACCUMULATED  (beta 1)
 *   [x0_diff | x1_diff] = dz1 . w1                     OVERWRITTEN  (beta 0)
 *   A NULL output is not computed.  loss_weight is a host scalar: top[0]->cpu_diff()[0].
 *
 * Summation order.  The reference's sums are BLAS-ordered; here the order is a fixed function of the shape, the
 * element type and the route: no floating-point atomics, the same words on every run, for every alignment of the
 * arrays and whatever the workspace held before the call.  Sums over n (the parameter diffs, the loss, the count of
 * labels not ignored) are taken in slabs of the sample range: each slab's partial sum goes to the workspace, and the
 * slabs are added in ascending order, first to last, and then into the diff.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  a NULL shape; N < 0; F0 <= 0; F1 < 0; H <= 0; C <= 0; dropout_ratio not in (0, 1); an unknown
 *                        phase or normalization; x0, x1, h, prob, w1 or w2 over INT_MAX elements; with N > 0: a NULL
 *                        x0, w1, w2, h or prob (forward), x0, w1, w2, h, prob or label (backward); x1 == NULL with
 *                        F1 > 0; TRAIN with a NULL mask; loss without label; an output that is an input or another
 *                        output; a backward with no output.
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query, for a forward that has a loss and for every backward.
 *   N == 0               MMS_OK, nothing is written.
 */
#ifndef MMS_HEAD_H_
#define MMS_HEAD_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_HEAD_TRAIN 0                  /* caffe.proto: Phase */
#define MMS_HEAD_TEST 1

#define MMS_HEAD_NORM_FULL 0              /* caffe.proto: LossParameter.NormalizationMode */
#define MMS_HEAD_NORM_VALID 1             /* Caffe's default */
#define MMS_HEAD_NORM_BATCH_SIZE 2
#define MMS_HEAD_NORM_NONE 3

typedef struct mms_head_shape {
  int N;                     /* samples                                                                 */
  int F0, F1;                /* widths of the two Concat bottoms; F1 may be 0                           */
  int H;                     /* fc1 num_output                                                          */
  int C;                     /* fc2 num_output = number of classes, >= 1                                */
  int phase;                 /* MMS_HEAD_TRAIN / MMS_HEAD_TEST: Dropout's only switch                   */
  float dropout_ratio;       /* in (0, 1), in TEST too                                                  */
  int normalization;         /* MMS_HEAD_NORM_*                                                         */
  int has_ignore_label, ignore_label;
} mms_head_shape;

/* Bytes of workspace that either pass needs, on whichever route; 0 for a shape the calls refuse and for N == 0. */
size_t mms_head_workspace_bytes(const mms_head_shape* shape);
size_t mms_head_workspace_bytes_f64(const mms_head_shape* shape);

/* The one routing decision of the float calls: the launchers call it, and so may a host.  pass: */
#define MMS_HEAD_PASS_FORWARD 0
#define MMS_HEAD_PASS_BACKWARD 1
/* returns: */
#define MMS_HEAD_ROUTE_NONE (-1)          /* the calls refuse this shape, or pass is neither of the two */
#define MMS_HEAD_ROUTE_GENERIC 0          /* one thread per output element or per sample, any accepted shape */
#define MMS_HEAD_ROUTE_FAST 1             /* weights in LDS, fc1 and its two backward products on the fp32 matrix pipe:
                                             F0 + F1 <= 128, H <= 64 and C <= 16 (csrc/head.hip: kHeadMaxFeatures,
                                             kHeadMaxHidden, kHeadMaxClasses); the same in both passes */
/* The _f64 calls and the *_generic_* calls always take MMS_HEAD_ROUTE_GENERIC. */
int mms_head_route(const mms_head_shape* shape, int pass);

int mms_head_forward_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1, const float* b1,
                         const unsigned int* mask, const float* w2, const float* b2, const float* label, float* h,
                         float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mms_head_backward_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                          const float* w2, const unsigned int* mask, const float* h, const float* prob,
                          const float* label, float loss_weight, float* x0_diff, float* x1_diff, float* w1_diff,
                          float* b1_diff, float* w2_diff, float* b2_diff, void* workspace, size_t workspace_bytes,
                          void* stream);
int mms_head_forward_f64(const mms_head_shape* shape, const double* x0, const double* x1, const double* w1,
                         const double* b1, const unsigned int* mask, const double* w2, const double* b2,
                         const double* label, double* h, double* prob, double* loss, void* workspace,
                         size_t workspace_bytes, void* stream);
int mms_head_backward_f64(const mms_head_shape* shape, const double* x0, const double* x1, const double* w1,
                          const double* w2, const unsigned int* mask, const double* h, const double* prob,
                          const double* label, double loss_weight, double* x0_diff, double* x1_diff, double* w1_diff,
                          double* b1_diff, double* w2_diff, double* b2_diff, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The same two float calls on MMS_HEAD_ROUTE_GENERIC whatever mms_head_route says: the summation order of the _f64
 * calls, in float.  For a host that wants one order at every shape, and for checking one route against the other. */
int mms_head_forward_generic_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                                 const float* b1, const unsigned int* mask, const float* w2, const float* b2,
                                 const float* label, float* h, float* prob, float* loss, void* workspace,
                                 size_t workspace_bytes, void* stream);
int mms_head_backward_generic_f32(const mms_head_shape* shape, const float* x0, const float* x1, const float* w1,
                                  const float* w2, const unsigned int* mask, const float* h, const float* prob,
                                  const float* label, float loss_weight, float* x0_diff, float* x1_diff,
                                  float* w1_diff, float* b1_diff, float* w2_diff, float* b2_diff, void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_HEAD_H_ */
