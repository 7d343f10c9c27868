/* tests/native/fc_abi_is_c.c -- include/mms_fc.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_fc.h"

typedef size_t (*ipws_t)(const mms_inner_product_shape*);
typedef int (*iproute_t)(const mms_inner_product_shape*, int);
typedef int (*ipf32_t)(const mms_inner_product_shape*, const float*, const float*, const float*, float*, void*);
typedef int (*ipf64_t)(const mms_inner_product_shape*, const double*, const double*, const double*, double*, void*);
typedef int (*ipb32_t)(const mms_inner_product_shape*, const float*, const float*, const float*, float*, float*, float*,
                       void*, size_t, void*);
typedef int (*ipb64_t)(const mms_inner_product_shape*, const double*, const double*, const double*, double*, double*,
                       double*, void*, size_t, void*);
typedef int (*smf32_t)(const mms_softmax_shape*, const float*, float*, void*);
typedef int (*smf64_t)(const mms_softmax_shape*, const double*, double*, void*);
typedef int (*smb32_t)(const mms_softmax_shape*, const float*, const float*, float*, void*);
typedef int (*smb64_t)(const mms_softmax_shape*, const double*, const double*, double*, void*);
typedef size_t (*slws_t)(const mms_softmax_loss_shape*);
typedef int (*slf32_t)(const mms_softmax_loss_shape*, const float*, const float*, float*, float*, void*, size_t, void*);
typedef int (*slf64_t)(const mms_softmax_loss_shape*, const double*, const double*, double*, double*, void*, size_t, void*);
typedef int (*slb32_t)(const mms_softmax_loss_shape*, const float*, const float*, float, float*, void*, size_t, void*);
typedef int (*slb64_t)(const mms_softmax_loss_shape*, const double*, const double*, double, double*, void*, size_t, void*);
typedef int (*ccf32_t)(const mms_concat_shape*, const float* const*, float*, void*);
typedef int (*ccf64_t)(const mms_concat_shape*, const double* const*, double*, void*);
typedef int (*ccb32_t)(const mms_concat_shape*, const float*, float* const*, void*);
typedef int (*ccb64_t)(const mms_concat_shape*, const double*, double* const*, void*);

int mms_fc_abi_is_c_probe(void) {
  const ipws_t w0 = &mms_inner_product_workspace_bytes, w1 = &mms_inner_product_workspace_bytes_f64;
  const iproute_t rt = &mms_inner_product_route;
  const ipf32_t f0 = &mms_inner_product_forward_f32, f1 = &mms_inner_product_forward_generic_f32;
  const ipf64_t f2 = &mms_inner_product_forward_f64;
  const ipb32_t b0 = &mms_inner_product_backward_f32, b1 = &mms_inner_product_backward_generic_f32;
  const ipb64_t b2 = &mms_inner_product_backward_f64;
  const smf32_t s0 = &mms_softmax_forward_f32;
  const smf64_t s1 = &mms_softmax_forward_f64;
  const smb32_t s2 = &mms_softmax_backward_f32;
  const smb64_t s3 = &mms_softmax_backward_f64;
  const slws_t l0 = &mms_softmax_loss_workspace_bytes, l1 = &mms_softmax_loss_workspace_bytes_f64;
  const slf32_t l2 = &mms_softmax_loss_forward_f32;
  const slf64_t l3 = &mms_softmax_loss_forward_f64;
  const slb32_t l4 = &mms_softmax_loss_backward_f32;
  const slb64_t l5 = &mms_softmax_loss_backward_f64;
  const ccf32_t c0 = &mms_concat_forward_f32;
  const ccf64_t c1 = &mms_concat_forward_f64;
  const ccb32_t c2 = &mms_concat_backward_f32;
  const ccb64_t c3 = &mms_concat_backward_f64;
  mms_inner_product_shape ip;
  mms_softmax_shape sm;
  mms_softmax_loss_shape sl;
  mms_concat_shape cc;
  ip.M = 1; ip.K = 1; ip.N_out = 1; ip.transpose = 0; ip.bias_term = 1;
  sm.outer = 1; sm.channels = 2; sm.inner = 1;
  sl.outer = 1; sl.channels = 2; sl.inner = 1; sl.normalization = MMS_LOSS_NORM_VALID; sl.has_ignore_label = 0;
  sl.ignore_label = 0;
  cc.num_concats = 1; cc.concat_input_size = 1; cc.num_bottoms = 1; cc.axis_extent[MMS_CONCAT_MAX_BOTTOMS - 1] = 0;
  return w0 && w1 && rt && f0 && f1 && f2 && b0 && b1 && b2 && s0 && s1 && s2 && s3 && l0 && l1 && l2 && l3 && l4 && l5 &&
         c0 && c1 && c2 && c3 && ip.M && sm.outer && sl.outer && cc.num_concats && MMS_FC_ROUTE_NONE == -1 &&
         MMS_FC_ROUTE_FAST == 1 && MMS_FC_PASS_BACKWARD == 1 && MMS_LOSS_NORM_NONE == 3 && MMS_CONCAT_MAX_BOTTOMS == 8 && MMS_ERR_WORKSPACE == 3;
}
