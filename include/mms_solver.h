/* include/mms_solver.h -- the solver update on the C ABI of libmms_hip.so: the reference's SGDSolver::ApplyUpdate
 * (ClipGradients, then per blob Normalize, Regularize, ComputeUpdateValue, then Net::Update) for the SGD and AdaDelta
 * solvers, with Net::ClearParamDiffs folded in on request, as ONE launch over all learnable blobs (three with gradient
 * clipping).  network_v4 trains with AdaDelta (do_trec_qa_clean.py:322-348).
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  The calls are stateless: the state of a
 * solver (history_) lives in the caller's arrays.  All arrays are device memory; the blob table and the parameters are
 * HOST memory, read before the call returns.  A call enqueues its launches on `stream` and returns without waiting; it
 * allocates no device memory and uses no floating-point atomics.  Dtype is float (_f32) or double (_f64).
 *
 * Arithmetic.  The reference's CPU path, element by element; every line is one rounding in Dtype (the library is built
 * without contraction and with correctly rounded divide and sqrt).  m = Dtype(momentum), om = Dtype(1) - m,
 * d = Dtype(delta), w = data, g = diff, h = hist_grad, h2 = hist_update:
 *
 *   clip       if clip_gradients >= 0 and l2norm > clip:  g = g * (clip / l2norm)       sgd_solver.cpp:81-99, before Normalize
 *   normalize  if iter_size != 1:                         g = g * (Dtype(1) / iter_size) sgd_solver.cpp:119-127
 *   regularize ld = Dtype(weight_decay) * decay_mult; only if ld != 0:                   sgd_solver.cpp:145-173
 *                L2: g = g + ld * w          L1: g = g + ld * sign(w), sign(0) = sign(NaN) = 0
 *   AdaDelta   u = g * g;  h  = om * u + m * h           (two products, one sum)         adadelta_solver.cpp:36-43
 *              u = d + h2; t = d + h; u = u / t; u = sqrt(u); g = g * u                  adadelta_solver.cpp:46-74
 *              u = g * g;  h2 = om * u + m * h2                                          adadelta_solver.cpp:77-84
 *              g = lr * g,  lr = rate * lr_mult                                          adadelta_solver.cpp:87-89
 *   SGD        h = lr * g + m * h;  g = h                                                sgd_solver.cpp:221-226
 *   update     w = w - g                                                                 blob.cpp:161
 *   diff       g as computed (MMS_SOLVER_DIFF_UPDATE) or +0 (MMS_SOLVER_DIFF_ZERO)
 *
 * Three places where this restates the reference, or where the reference is not pinned:
 *   - caffe_powx(x, 0.5) is restated as sqrt(x), and caffe_powx(x, 2) as x * x;
 *   - caffe_cpu_axpby and caffe_axpy are restated as two rounded products (one for axpy) and a rounded sum;
 *   - the bits the reference's libm (pow) and BLAS (axpby, axpy, an FMA or not) give for these three are not pinned.
 * Everything else is as the reference does it: a blob with lr_mult = 0 still moves its histories; delta = 0 is not
 * guarded; ld == 0 skips the regularizer rather than adding zero.  The reference's GPU path narrows delta and momentum
 * to float even for double (adadelta_solver.cu:10-11); this is the CPU path in both element types.
 *
 * Clipping (clip_gradients >= 0).  l2norm = sqrt(sum over blobs of sumsq(diff)).  The sum's order is a fixed function
 * of the counts alone: a blob is cut into chunks of MMS_SOLVER_CHUNK elements; inside a chunk, thread t of 256 adds the
 * squares of elements 4t .. 4t+3, 4t+1024 .. 4t+1027, ... in ascending order, and the 256 sums are added by a binary
 * tree (t with t + 128, then t + 64, ...); the chunk sums go to the workspace and one workgroup adds them in ascending
 * chunk order within a blob, and the blob sums in ascending blob order.  It writes l2norm and the scale
 * (clip / l2norm, or 1 where l2norm > clip does not hold) to the workspace, from where the update reads the scale, and
 * to clip_info when that is given.  The same words on every run, for every alignment of the arrays and whatever the
 * workspace held before.  Without clipping no workspace is touched and none is required, and clip_info is not written.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  a NULL param; NULL blobs with nblobs > 0; nblobs < 0; iter_size < 1; an unknown regularization
 *                        or diff_out; a count < 0 or > INT_MAX; with count > 0: a NULL data, diff or hist_grad, and for
 *                        AdaDelta a NULL hist_update; any two arrays of the call overlapping, across blobs too (a
 *                        parameter shared by name is passed once, as Net::learnable_params() lists it): data, diff,
 *                        hist_grad and, for AdaDelta, hist_update of every blob with count > 0, clip_info (2 words)
 *                        and, with clipping, the workspace (the bytes of the query).  SGD ignores hist_update.
 *   MMS_ERR_UNSUPPORTED  any other solver type (Nesterov, AdaGrad, RMSProp, Adam), judged right after param != NULL.
 *                        Also, with more than MMS_SOLVER_BLOBS_PER_LAUNCH blobs of count > 0, when the host memory for
 *                        the overlap check cannot be had (up to that many blobs the call allocates no host memory).
 *   MMS_ERR_WORKSPACE    clipping on, some count > 0, and the workspace NULL or smaller than the query.
 *   nblobs == 0, or every count 0: MMS_OK, nothing is written.
 */
#ifndef MMS_SOLVER_H_
#define MMS_SOLVER_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_SOLVER_SGD 0                  /* solver type "SGD"      */
#define MMS_SOLVER_ADADELTA 1             /* solver type "AdaDelta" */

#define MMS_SOLVER_L2 0                   /* regularization_type "L2", the proto's default */
#define MMS_SOLVER_L1 1

#define MMS_SOLVER_DIFF_UPDATE 0          /* diff holds the applied update, as the reference leaves it    */
#define MMS_SOLVER_DIFF_ZERO 1            /* diff is zeroed: Net::ClearParamDiffs (net.cpp:923) folded in */

/* Elements of one work item of a workgroup: a multiple of 4.  A blob of count elements is ceil(count / CHUNK) items. */
#define MMS_SOLVER_CHUNK 2048
/* Blobs (with count > 0) of one launch: the size of the blob table that travels in the kernel arguments. */
#define MMS_SOLVER_BLOBS_PER_LAUNCH 32

typedef struct mms_solver_blob {      /* one learnable parameter, as Net::learnable_params() lists it              */
  void* data;                         /* count elements each                                                       */
  void* diff;
  void* hist_grad;                    /* history_[i]     : SGD's momentum buffer / AdaDelta's E[g^2]               */
  void* hist_update;                  /* history_[P + i] : AdaDelta's E[dx^2]; ignored (may be NULL) for SGD       */
  long long count;                    /* 0 .. INT_MAX; a blob of count 0 is skipped                                */
  float lr_mult, decay_mult;          /* Net::params_lr() / params_weight_decay(): float in the reference          */
} mms_solver_blob;

typedef struct mms_solver_param {
  int type;                           /* MMS_SOLVER_SGD, MMS_SOLVER_ADADELTA                                       */
  int regularization;                 /* MMS_SOLVER_L2, MMS_SOLVER_L1                                              */
  int iter_size;                      /* >= 1                                                                      */
  int diff_out;                       /* MMS_SOLVER_DIFF_UPDATE, MMS_SOLVER_DIFF_ZERO                              */
  float momentum, delta, weight_decay;/* SolverParameter's fields are float; converted to Dtype as the reference does */
  float clip_gradients;               /* < 0: off (the proto's default is -1)                                      */
} mms_solver_param;

/* Bytes of workspace a step needs: 0 without clipping, for a param, nblobs or count the step refuses (the pointers of
 * the blobs are not looked at), and when every count is 0. */
size_t mms_solver_workspace_bytes(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs);
size_t mms_solver_workspace_bytes_f64(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs);

/* One solver step.  rate: GetLearningRate()'s result (the learning-rate policies are host arithmetic).
 * clip_info: device, 2 words -- l2norm and the scale applied (1 if not clipped); may be NULL; written only with
 * clipping on.  ceil(blobs with count > 0 / MMS_SOLVER_BLOBS_PER_LAUNCH) update launches, in blob order. */
int mms_solver_step_f32(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs, float rate,
                        float* clip_info, void* workspace, size_t workspace_bytes, void* stream);
int mms_solver_step_f64(const mms_solver_param* param, const mms_solver_blob* blobs, int nblobs, double rate,
                        double* clip_info, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_SOLVER_H_ */
