/* include/mms_bn_maxpool.h -- BN -> MaxPool -> TanH in one call on the C ABI of libmms_hip.so: what network_v3 and
 * network_v5 do with their BN outputs (do_trec_qa_clean.py:403-407, :577-583), as mms_bn_pool_tanh_* (include/mms.h) is
 * what network_v4 does with its own.  Replaces, in sequence, BNLayer (bn_layer.cpp), PoolingLayer MAX
 * (pooling_layer.cpp:149-170, :269-287) and the in-place TanHLayer (tanh_layer.cpp:13-33).
 *
 * This header adds to include/mms.h and changes nothing in it: the error codes, the stream convention and MMS_VERSION
 * are its.  Shapes, arrays, refusals (their order and codes), the optional backward outputs, the two routes and the
 * workspace are those of mms_bn_pool_tanh_*: windows (kh, kw) that TILE the map (H % kh == 0, W % kw == 0, stride ==
 * kernel, no padding) or one window that is the whole map; x and bottom_diff (N, C, H, W); top, top_diff and save_pool
 * (N, C, H/kh, W/kw); every other array C elements.  The workspace queries return mms_bn_pool_tanh_workspace_bytes'
 * figure.  ONE difference in the argument lists: the backward also reads `shift` (after `scale`; required, and
 * bottom_diff must not be it), because the mask is a property of BN's OUTPUT, shift included -- see "backward".
 *
 * Per channel c, with bn_out(x) = ((x + (-mean)) / std)*scale + shift, every operation rounded once, in that order:
 *
 *   forward   mean, var, std = sqrt(var + 1e-9), running blobs, save_mean, save_std: as mms_bn_pool_tanh_forward, from
 *             sum x and sum x*x over the channel accumulated in that call's order (the same words); TEST reads the
 *             running blobs.
 *             e = ext(window): the window's elements compared in (h, w) order, starting from the first; the scan keeps
 *             the larger for scale[c] > 0, the smaller for scale[c] < 0; a NaN never wins a comparison.  For
 *             scale[c] == 0 every BN output is shift[c] and e is the window's first element, which is i* below.
 *             save_pool = (e + (-mean)) / std
 *             top = tanh(bn_out(e))
 *   backward  gp = top_diff*(1 - top*top);  shift_diff = sum gp;  scale_diff = sum gp*save_pool;
 *             a = scale*scale_diff;  b = scale*shift_diff       (both sums over the pooled tensor, in the AVE
 *             backward's order);  xn = (x + (-mean)) / std
 *             i* = the first element of the window, in (h, w) order, with bn_out(x_i) > bn_out(x_j) for every earlier
 *             j: the reference's scan, started from the window's first element
 *             g_i = gp*scale for i == i*, 0 otherwise
 *             bottom_diff_i = (g_i + (-1/(N*H*W))*(xn_i*a + b)) / std          for every element of the window
 *
 * Why one sweep of x per pass is enough and no mask is stored.  bn_out is a chain of correctly
 * rounded monotone operations (std > 0), non-decreasing for scale >= 0 and non-increasing for scale < 0, so
 * max_i bn_out(x_i) == bn_out(e) word for word: the forward compares x, whose order is known before the statistics
 * are.  i* is the first element that attains that maximum, so the backward finds e again and gives the gradient to the
 * first element whose bn_out equals bn_out(e).  Where distinct x collapse to one BN output in the element type, that
 * is the first of them, not arg-ext x -- as in the reference, whose mask is made from the BN output.
 *
 * Against BNLayer -> PoolingLayer(MAX) -> TanHLayer on finite inputs: 1e-5 (float) / 1e-12 (double); the statistics
 * are BLAS sums there.  Deviations:
 *   - scale_diff uses save_pool, xn at the extremum of x, where the reference uses xn at i*: the same value unless
 *     rounding collapsed the BN outputs of the two, which (scale == 0 apart, see e) takes x that differ by less than
 *     an ulp of shift/scale*std;
 *   - the sign of a zero top where scale == 0;
 *   - the reference starts its scan from -FLT_MAX, this one from the window's first element.  That shows only for
 *     windows that are all NaN or all below -FLT_MAX, where the reference's own backward indexes mask = -1; such
 *     inputs are outside the contract.
 * Sums have a fixed order (no atomics): the same words on every run, on either route, whatever the arrays' alignment
 * and whatever the workspace held.
 */
#ifndef MMS_BN_MAXPOOL_H_
#define MMS_BN_MAXPOOL_H_

#include "mms.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t mms_bn_maxpool_tanh_workspace_bytes(int N, int C, int H, int W, int kh, int kw);
int mms_bn_maxpool_tanh_forward_f32(int phase, int N, int C, int H, int W, int kh, int kw, float bn_memory,
                                    const float* x, const float* scale, const float* shift, float* running_mean,
                                    float* running_var, float* top, float* save_pool, float* save_mean,
                                    float* save_std, void* workspace, size_t workspace_bytes, void* stream);
int mms_bn_maxpool_tanh_backward_f32(int N, int C, int H, int W, int kh, int kw, const float* x, const float* top,
                                     const float* top_diff, const float* save_pool, const float* scale,
                                     const float* shift, const float* save_mean, const float* save_std,
                                     float* bottom_diff, float* scale_diff, float* shift_diff, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* The same with every float a double (a 16-byte access is 2 elements). */
size_t mms_bn_maxpool_tanh_workspace_bytes_f64(int N, int C, int H, int W, int kh, int kw);
int mms_bn_maxpool_tanh_forward_f64(int phase, int N, int C, int H, int W, int kh, int kw, double bn_memory,
                                    const double* x, const double* scale, const double* shift, double* running_mean,
                                    double* running_var, double* top, double* save_pool, double* save_mean,
                                    double* save_std, void* workspace, size_t workspace_bytes, void* stream);
int mms_bn_maxpool_tanh_backward_f64(int N, int C, int H, int W, int kh, int kw, const double* x, const double* top,
                                     const double* top_diff, const double* save_pool, const double* scale,
                                     const double* shift, const double* save_mean, const double* save_std,
                                     double* bottom_diff, double* scale_diff, double* shift_diff, void* workspace,
                                     size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* MMS_BN_MAXPOOL_H_ */
