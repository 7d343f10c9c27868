/* tests/native/head_abi_is_c.c -- include/mms_head.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_head.h"

typedef int (*fwd_t)(const mms_head_shape*, const float*, const float*, const float*, const float*, const unsigned int*,
                     const float*, const float*, const float*, float*, float*, float*, void*, size_t, void*);
typedef int (*bwd_t)(const mms_head_shape*, const float*, const float*, const float*, const float*, const unsigned int*,
                     const float*, const float*, const float*, float, float*, float*, float*, float*, float*, float*,
                     void*, size_t, void*);
typedef int (*fwd64_t)(const mms_head_shape*, const double*, const double*, const double*, const double*,
                       const unsigned int*, const double*, const double*, const double*, double*, double*, double*,
                       void*, size_t, void*);
typedef int (*bwd64_t)(const mms_head_shape*, const double*, const double*, const double*, const double*,
                       const unsigned int*, const double*, const double*, const double*, double, double*, double*,
                       double*, double*, double*, double*, void*, size_t, void*);
typedef size_t (*query_t)(const mms_head_shape*);

int mms_head_abi_is_c_probe(void) {
  const fwd_t f[2] = {&mms_head_forward_f32, &mms_head_forward_generic_f32};
  const bwd_t b[2] = {&mms_head_backward_f32, &mms_head_backward_generic_f32};
  const fwd64_t f64 = &mms_head_forward_f64;
  const bwd64_t b64 = &mms_head_backward_f64;
  const query_t q[2] = {&mms_head_workspace_bytes, &mms_head_workspace_bytes_f64};
  int (*const route)(const mms_head_shape*, int) = &mms_head_route;
  mms_head_shape s = {50, 64, 2, 32, 2, MMS_HEAD_TRAIN, 0.5f, MMS_HEAD_NORM_VALID, 0, 0};
  return f[0] && f[1] && b[0] && b[1] && f64 && b64 && q[0] && q[1] && route && s.C == 2 && MMS_HEAD_ROUTE_FAST == 1 &&
         MMS_HEAD_ROUTE_GENERIC == 0 && MMS_HEAD_ROUTE_NONE == -1 && MMS_HEAD_PASS_BACKWARD == 1 &&
         MMS_HEAD_TEST == 1 && MMS_HEAD_NORM_NONE == 3 && MMS_ERR_WORKSPACE == 3;
}
