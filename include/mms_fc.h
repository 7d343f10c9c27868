/* include/mms_fc.h -- the layers of the classifier head on the C ABI of libmms_hip.so, each as a call of its own: the
 * reference's InnerProductLayer (inner_product_layer.cpp:10-141, `transpose` included), SoftmaxLayer
 * (softmax_layer.cpp:10-90, any axis), SoftmaxWithLossLayer (softmax_loss_layer.cpp:12-149) and ConcatLayer
 * (concat_layer.cpp:10-96, up to MMS_CONCAT_MAX_BOTTOMS bottoms).  mms_head_* (mms_head.h) fuses one topology of them;
 * a host with another one -- four Concat bottoms, a second hidden layer, no Dropout, a spatial softmax -- runs
 *   mms_concat_forward -> mms_inner_product_forward -> mms_tanh_forward -> mms_dropout_forward ->
 *   mms_inner_product_forward -> mms_softmax_loss_forward
 * and the backward calls in reverse.  Flatten needs no call: it shares its bottom's data (flatten_layer.cpp), and the
 * rows of a contiguous (N, C, H, W) blob ARE the rows of (N, C * H * W).
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  All arrays are device memory, contiguous
 * and row-major, aligned to their element; a call enqueues its launches on `stream` and returns without waiting; it
 * allocates nothing and synchronises nothing.  Dtype is float (_f32) or double (_f64).
 *
 * Summation order.  A fixed function of the shape, the element type and the route: no floating-point atomics, the same
 * words on every run, for every alignment of the arrays and whatever the workspace held before the call.  Sums over
 * rows (the parameter diffs of InnerProduct, the loss and the count of labels not ignored) are taken in SLABS of the
 * row range: each slab's partial sum goes to the workspace, the partials are added in ascending slab order, first to
 * last, and that sum is then added into the diff -- the rule of mms_head.h.
 *
 * InnerProduct.  x (M, K) with M = count(0, axis), K = count(axis) -- host arithmetic; w (N_out, K), or (K, N_out) with
 * `transpose`; b (N_out); top (M, N_out).
 *   forward   top = x . w^T (x . w with transpose); with bias_term, top += b: one add per element after its complete
 *             sum, as the reference's second gemm with beta 1 (:93-96).
 *   backward  w_diff += top_diff^T . x   (N_out, K), or x^T . top_diff (K, N_out) with transpose     ACCUMULATED (:108-123)
 *             b_diff += sum_m top_diff                                                               ACCUMULATED (:125-130)
 *             bottom_diff = top_diff . w (top_diff . w^T with transpose)                             OVERWRITTEN (:132-146)
 *             A NULL output is not computed.  w_diff and b_diff are sums over m: slabs (above).
 *   routes    MMS_FC_ROUTE_GENERIC: one thread per output element, the inner index ascending, products and adds rounded
 *             separately.  Any accepted shape; the _f64 calls and the *_generic_f32 calls always take it.
 *             MMS_FC_ROUTE_FAST (float): the three products on the fp32 matrix pipe (v_mfma_f32_*_f32, each a k-ordered
 *             fused chain), the bias in the forward's epilogue.  Which shapes take it in which pass -- the two passes
 *             are routed apart, each by what was timed -- and which kernel each product then takes, is stated once, in
 *             csrc/fc_plans.h; mms_inner_product_route is that decision.
 *
 * Softmax.  The blob is (outer, channels, inner) = (count(0, axis), shape(axis), count(axis + 1)).
 *   forward   per (o, k): max over channels; e_c = exp(x_c - max); sum of e_c, c ascending; top_c = e_c / sum.
 *   backward  per (o, k): dot = sum_c top_diff_c * top_c, c ascending; bottom_diff_c = (top_diff_c - dot) * top_c.
 *             bottom_diff may be top_diff (the reference's backward runs in place); the words are the same.
 *
 * SoftmaxWithLoss.  bottom and prob (outer, channels, inner); label (outer, inner) Dtype, read as static_cast<int>
 * (:100); loss (1).
 *   forward   prob = softmax(bottom) as above;
 *             loss = - sum log(max(prob[o, label, k], Dtype(FLT_MIN))) / max(1, normalizer)
 *             over the labels that are not ignored.  normalizer (:59-86): outer * inner for FULL, the number of labels
 *             not ignored for VALID, outer for BATCH_SIZE, 1 for NONE.  The legacy `normalize` flag is the host's to
 *             map (:28-35): without `normalization`, normalize = true is VALID and normalize = false is BATCH_SIZE.
 *   backward  bottom_diff = prob, minus 1 at the label, zero rows for ignored labels; all of it times the one scalar
 *             loss_weight / max(1, normalizer), formed on the device in Dtype (:145-147).  loss_weight is a host
 *             scalar: top[0]->cpu_diff()[0].
 *   A label outside [0, channels) is a DCHECK in the reference.  Here it is treated as IGNORED, in both passes and in
 *   the VALID count, so that no call indexes out of a row (mms_head.h has the same rule).  The loss sum and the count
 *   are taken in slabs of the (o, k) range.
 *
 * Concat.  bottom b is (num_concats, axis_extent[b], concat_input_size), top is (num_concats, sum_b axis_extent[b],
 * concat_input_size); `bottoms` / `bottom_diffs` are HOST arrays of num_bottoms device pointers, read before the call
 * returns.  Forward: one launch copies every bottom into top.  Backward: one launch splits top_diff into the bottom
 * diffs; a NULL diff stands for propagate_down == false and is skipped.  Bit copies: 16 bytes per lane where a bottom's
 * run, the top's row and both addresses allow it, single elements otherwise.  A bottom of extent 0 is not looked at.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  a NULL shape.
 *                        InnerProduct: M < 0; K < 1; N_out < 1; transpose or bias_term neither 0 nor 1; x, w or top over
 *                        INT_MAX elements; with M > 0: a NULL x, w or top, bias_term with a NULL b (forward); a NULL
 *                        top_diff, a NULL x with w_diff, a NULL w with bottom_diff, b_diff without bias_term, no output
 *                        at all (backward); an output overlapping an input or another output.
 *                        Softmax, SoftmaxWithLoss: outer < 0; channels < 1; inner < 1; the blob over INT_MAX elements;
 *                        an unknown normalization; with outer > 0: a NULL array; any two arrays overlapping, other than
 *                        bottom_diff == top_diff in mms_softmax_backward_*.
 *                        Concat: num_concats < 0; concat_input_size < 1; num_bottoms < 1 or > MMS_CONCAT_MAX_BOTTOMS; a
 *                        negative extent; a top axis of 0; top over INT_MAX elements; with num_concats > 0: a NULL
 *                        pointer array, top or top_diff; a NULL bottom of extent > 0 (forward); a bottom or bottom diff
 *                        that overlaps top / top_diff; two bottom diffs overlapping; a backward with no diff.
 *   MMS_ERR_WORKSPACE    workspace NULL or smaller than the query: an InnerProduct backward with w_diff or b_diff, and
 *                        both SoftmaxWithLoss passes.
 *   M == 0, outer == 0, num_concats == 0     MMS_OK, nothing is written, the pointers are not looked at.
 * The workspace queries return 0 for a shape the calls refuse and for an empty one.
 */
#ifndef MMS_FC_H_
#define MMS_FC_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- InnerProduct ---- */
typedef struct mms_inner_product_shape {
  int M;                      /* rows: count(0, axis)                                */
  int K;                      /* inputs per row: count(axis)                         */
  int N_out;                  /* num_output                                          */
  int transpose;              /* 0: w is (N_out, K); 1: w is (K, N_out)              */
  int bias_term;              /* 0 / 1                                               */
} mms_inner_product_shape;

/* Bytes the backward needs for the slab partials of w_diff and b_diff, on whichever route. */
size_t mms_inner_product_workspace_bytes(const mms_inner_product_shape* shape);
size_t mms_inner_product_workspace_bytes_f64(const mms_inner_product_shape* shape);

#define MMS_FC_PASS_FORWARD 0
#define MMS_FC_PASS_BACKWARD 1
#define MMS_FC_ROUTE_NONE (-1)            /* the calls refuse this shape, or pass is neither of the two */
#define MMS_FC_ROUTE_GENERIC 0
#define MMS_FC_ROUTE_FAST 1
/* The one routing decision of the float calls, per pass: the launchers call it, and so may a host. */
int mms_inner_product_route(const mms_inner_product_shape* shape, int pass);

int mms_inner_product_forward_f32(const mms_inner_product_shape* shape, const float* x, const float* w, const float* b,
                                  float* top, void* stream);
int mms_inner_product_forward_f64(const mms_inner_product_shape* shape, const double* x, const double* w,
                                  const double* b, double* top, void* stream);
int mms_inner_product_backward_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                   const float* top_diff, float* w_diff, float* b_diff, float* bottom_diff,
                                   void* workspace, size_t workspace_bytes, void* stream);
int mms_inner_product_backward_f64(const mms_inner_product_shape* shape, const double* x, const double* w,
                                   const double* top_diff, double* w_diff, double* b_diff, double* bottom_diff,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* The float calls on MMS_FC_ROUTE_GENERIC whatever mms_inner_product_route says: the summation order of _f64, in float. */
int mms_inner_product_forward_generic_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                          const float* b, float* top, void* stream);
int mms_inner_product_backward_generic_f32(const mms_inner_product_shape* shape, const float* x, const float* w,
                                           const float* top_diff, float* w_diff, float* b_diff, float* bottom_diff,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- Softmax ---- */
typedef struct mms_softmax_shape {
  int outer, channels, inner;
} mms_softmax_shape;

int mms_softmax_forward_f32(const mms_softmax_shape* shape, const float* bottom, float* top, void* stream);
int mms_softmax_forward_f64(const mms_softmax_shape* shape, const double* bottom, double* top, void* stream);
/* bottom_diff may be top_diff */
int mms_softmax_backward_f32(const mms_softmax_shape* shape, const float* top, const float* top_diff, float* bottom_diff,
                             void* stream);
int mms_softmax_backward_f64(const mms_softmax_shape* shape, const double* top, const double* top_diff,
                             double* bottom_diff, void* stream);

/* ---- SoftmaxWithLoss ---- */
#define MMS_LOSS_NORM_FULL 0              /* caffe.proto: LossParameter.NormalizationMode; the values of MMS_HEAD_NORM_* */
#define MMS_LOSS_NORM_VALID 1             /* Caffe's default */
#define MMS_LOSS_NORM_BATCH_SIZE 2
#define MMS_LOSS_NORM_NONE 3

typedef struct mms_softmax_loss_shape {
  int outer, channels, inner;
  int normalization;          /* MMS_LOSS_NORM_* */
  int has_ignore_label, ignore_label;
} mms_softmax_loss_shape;

/* Bytes either pass needs for the slab partials of the loss and of the count. */
size_t mms_softmax_loss_workspace_bytes(const mms_softmax_loss_shape* shape);
size_t mms_softmax_loss_workspace_bytes_f64(const mms_softmax_loss_shape* shape);

int mms_softmax_loss_forward_f32(const mms_softmax_loss_shape* shape, const float* bottom, const float* label,
                                 float* prob, float* loss, void* workspace, size_t workspace_bytes, void* stream);
int mms_softmax_loss_forward_f64(const mms_softmax_loss_shape* shape, const double* bottom, const double* label,
                                 double* prob, double* loss, void* workspace, size_t workspace_bytes, void* stream);
int mms_softmax_loss_backward_f32(const mms_softmax_loss_shape* shape, const float* prob, const float* label,
                                  float loss_weight, float* bottom_diff, void* workspace, size_t workspace_bytes,
                                  void* stream);
int mms_softmax_loss_backward_f64(const mms_softmax_loss_shape* shape, const double* prob, const double* label,
                                  double loss_weight, double* bottom_diff, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* ---- Concat ---- */
#define MMS_CONCAT_MAX_BOTTOMS 8

typedef struct mms_concat_shape {
  int num_concats;            /* count(0, axis)                                      */
  int concat_input_size;      /* count(axis + 1)                                     */
  int num_bottoms;            /* 1 .. MMS_CONCAT_MAX_BOTTOMS                         */
  int axis_extent[MMS_CONCAT_MAX_BOTTOMS];   /* shape(axis) of each bottom; the first num_bottoms are read */
} mms_concat_shape;

int mms_concat_forward_f32(const mms_concat_shape* shape, const float* const* bottoms, float* top, void* stream);
int mms_concat_forward_f64(const mms_concat_shape* shape, const double* const* bottoms, double* top, void* stream);
int mms_concat_backward_f32(const mms_concat_shape* shape, const float* top_diff, float* const* bottom_diffs,
                            void* stream);
int mms_concat_backward_f64(const mms_concat_shape* shape, const double* top_diff, double* const* bottom_diffs,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_FC_H_ */
