/* tests/native/conv_abi_is_c.c -- include/mms_conv.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_conv.h"

typedef int (*fwd_t)(const mms_conv_shape*, const float*, const float*, const float*, float*, void*, size_t, void*);
typedef int (*bwd_t)(const mms_conv_shape*, const float*, const float*, const float*, float*, float*, float*, void*,
                     size_t, void*);
typedef int (*fwd64_t)(const mms_conv_shape*, const double*, const double*, const double*, double*, void*, size_t,
                       void*);
typedef int (*bwd64_t)(const mms_conv_shape*, const double*, const double*, const double*, double*, double*, double*,
                       void*, size_t, void*);
typedef size_t (*query_t)(const mms_conv_shape*);

int mms_conv_abi_is_c_probe(void) {
  const fwd_t f[2] = {&mms_conv_forward_f32, &mms_conv_forward_generic_f32};
  const bwd_t b[2] = {&mms_conv_backward_f32, &mms_conv_backward_generic_f32};
  const fwd64_t f64 = &mms_conv_forward_f64;
  const bwd64_t b64 = &mms_conv_backward_f64;
  const query_t q[2] = {&mms_conv_workspace_bytes, &mms_conv_workspace_bytes_f64};
  int (*const dims)(const mms_conv_shape*, int*, int*) = &mms_conv_output_dims;
  int (*const route)(const mms_conv_shape*, int) = &mms_conv_route;
  mms_conv_shape s = {1, 4, 40, 40, 32, 5, 5, 1, 1, 0, 0, 1, 1, 1};
  return f[0] && f[1] && b[0] && b[1] && f64 && b64 && q[0] && q[1] && dims && route && s.group == 1 &&
         MMS_CONV_ROUTE_FAST == 1 && MMS_CONV_ROUTE_GENERIC == 0 && MMS_CONV_ROUTE_NONE == -1 &&
         MMS_CONV_PASS_PARAM_DIFF == 2 && MMS_ERR_WORKSPACE == 3;
}
