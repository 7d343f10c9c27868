/* include/mms_pool.h -- Pooling and TanH on the C ABI of libmms_hip.so as layers of their own: the reference's
 * PoolingLayer (pooling_layer.cpp:78-307: MAX and AVE, any kernel, stride and padding, the ceil-mode output size with its
 * clipped last windows, max_idx_ or a second top) and its TanHLayer (tanh_layer.cpp:11-36).  The fused calls
 * (mms_bn_pool_tanh_*, mms_bn_maxpool_tanh_*, the conv stages, the tails) take windows that tile the map only; a host
 * whose geometry they refuse runs mms_bn_forward_* -> mms_pool_forward_* -> mms_tanh_forward_* instead.
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention (`stream` is a
 * hipStream_t, NULL = the default stream) and MMS_VERSION are those of mms.h.  All arrays are device memory, contiguous
 * and aligned to their element; a call enqueues one launch on `stream` and returns without waiting; it takes no
 * workspace, allocates nothing, synchronises nothing and uses no atomics, so it can be captured in a graph.  Dtype is
 * float (_f32) or double (_f64).  bottom and bottom_diff are (N, C, H, W); top, top_diff, mask and top_mask are
 * (N, C, PH, PW).
 *
 * Output size (pooling_layer.cpp:90-105), per axis:
 *
 *   PH = (int)ceil((float)(H + 2 pad_h - kernel_h) / stride_h) + 1
 *   if pad_h != 0 or pad_w != 0:  while (PH - 1) * stride_h >= H + pad_h:  --PH
 *
 * Global pooling is kernel = (H, W), stride 1, pad 0, set by the host.  Window (ph, pw) starts at
 * hs = ph * stride_h - pad_h, ws = pw * stride_w - pad_w.
 *
 * Forward, MAX (:140-187).  The clipped window [max(hs, 0), min(hs + kernel_h, H)) x [max(ws, 0), min(ws + kernel_w, W))
 * is scanned in row-major order from best = Dtype(-FLT_MAX) -- in double too: the float constant, widened -- and an
 * element replaces best where it is strictly greater.  top = best; mask = h * W + w of the element that replaced last,
 * i.e. of the FIRST maximum, or -1 where none did (every element NaN, or <= -FLT_MAX: top is then -FLT_MAX); top_mask is
 * the same index as Dtype.  A NaN is never selected.  Either of mask and top_mask may be NULL, and both (a TEST pass).
 *
 * Forward, AVE (:188-220).  pool_size = (min(hs + kernel_h, H + pad_h) - hs) * (min(ws + kernel_w, W + pad_w) - ws),
 * before the window is clipped to the image; the sum starts from +0 and adds the clipped window's elements in row-major
 * order, every add rounded in Dtype; top = sum / Dtype(pool_size), one correctly rounded division.  mask and top_mask
 * are ignored.
 *
 * Backward (:229-307).  The reference zeroes bottom_diff and adds into it walking (ph, pw) in ascending order.  Here one
 * thread owns a bottom element, starts from +0 and adds, in ascending (ph, pw) order over the windows that contain it,
 *   MAX:  top_diff[ph, pw]                         where that window's mask equals the element's h * W + w
 *   AVE:  top_diff[ph, pw] / Dtype(pool_size)      the quotient rounded once, then the add
 * which are the reference's operations on that element in the reference's order: the same bits, the sign of a zero
 * included; an element no window reaches gets +0.  Two deviations: a mask entry of -1, or one that names an element
 * outside its own window, contributes nothing (the reference writes out of bounds for the first; the forward never
 * produces the second).  MAX needs mask or top_mask; when both are given, mask is read.  A top_mask entry counts as the
 * index (int)entry where 0 <= entry < H * W, as nothing otherwise.
 *
 * TanH (tanh_layer.cpp:11-36).  Forward: top = tanh(bottom), the device function the fused stages use.  Backward:
 * t = top * top; u = 1 - t; bottom_diff = top_diff * u -- three roundings, no contraction.
 *
 * Refusals, all host-side, before anything is enqueued; a call that does not return MMS_OK writes nothing:
 *   MMS_ERR_INVALID_ARG  a NULL shape (mms_pool_output_dims: a NULL PH or PW too); N < 0; C, H, W, a kernel or a stride
 *                        < 1; a negative pad; pad >= kernel (CHECK_LT, :73-74); a method that is none of the three
 *                        below; a kernel so much larger than the padded map that the size rule gives PH or PW < 1;
 *                        then, with N > 0: bottom or top element count above INT_MAX; a NULL required array (bottom,
 *                        top; top_diff, bottom_diff); MAX backward with mask and top_mask both NULL; any two arrays
 *                        of the call overlapping.  TanH: count < 0; with count > 0 a NULL array, or two arrays
 *                        overlapping other than top == bottom (forward) and bottom_diff == top_diff (backward), the
 *                        in-place forms.
 *   MMS_ERR_UNSUPPORTED  MMS_POOL_STOCHASTIC (the reference's CPU path is NOT_IMPLEMENTED); a geometry whose last
 *                        window starts at or beyond the map, (PH - 1) * stride_h >= H + pad_h -- only with both pads
 *                        0 and stride > kernel; the reference computes a pool_size <= 0 there.
 *   N == 0, count == 0   MMS_OK, nothing is written, the pointers are not looked at.
 * mms_pool_output_dims judges the shape as the launching calls do, the method included, and writes PH and PW only when
 * it returns MMS_OK.
 */
#ifndef MMS_POOL_H_
#define MMS_POOL_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMS_POOL_AVE 0                    /* the values of MMS_STAGE_POOL_AVE / _MAX, not caffe.proto's order */
#define MMS_POOL_MAX 1
#define MMS_POOL_STOCHASTIC 2             /* refused: MMS_ERR_UNSUPPORTED */

typedef struct mms_pool_shape {
  int N, C, H, W;
  int kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w;
  int method;                             /* MMS_POOL_AVE, MMS_POOL_MAX */
} mms_pool_shape;

/* PH and PW of a shape.  Host only: nothing is enqueued. */
int mms_pool_output_dims(const mms_pool_shape* shape, int* PH, int* PW);

int mms_pool_forward_f32(const mms_pool_shape* shape, const float* bottom, float* top, int* mask, float* top_mask,
                         void* stream);
int mms_pool_forward_f64(const mms_pool_shape* shape, const double* bottom, double* top, int* mask, double* top_mask,
                         void* stream);
int mms_pool_backward_f32(const mms_pool_shape* shape, const float* top_diff, const int* mask, const float* top_mask,
                          float* bottom_diff, void* stream);
int mms_pool_backward_f64(const mms_pool_shape* shape, const double* top_diff, const int* mask, const double* top_mask,
                          double* bottom_diff, void* stream);

/* top may be bottom */
int mms_tanh_forward_f32(long long count, const float* bottom, float* top, void* stream);
int mms_tanh_forward_f64(long long count, const double* bottom, double* top, void* stream);
/* bottom_diff may be top_diff */
int mms_tanh_backward_f32(long long count, const float* top, const float* top_diff, float* bottom_diff, void* stream);
int mms_tanh_backward_f64(long long count, const double* top, const double* top_diff, double* bottom_diff, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_POOL_H_ */
