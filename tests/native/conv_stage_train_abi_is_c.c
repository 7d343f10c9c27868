/* tests/native/conv_stage_train_abi_is_c.c -- include/mms_conv_stage_train.h must be consumable from plain C: `gcc
 * -std=c99 -Wall -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_conv_stage_train.h"

typedef int (*fwd_t)(const mms_conv_shape*, int, int, int, float, const float*, const float*, const float*,
                     const float*, const float*, float*, float*, float*, float*, float*, float*, float*, void*, size_t,
                     void*);
typedef int (*fwd64_t)(const mms_conv_shape*, int, int, int, double, const double*, const double*, const double*,
                       const double*, const double*, double*, double*, double*, double*, double*, double*, double*,
                       void*, size_t, void*);
typedef int (*bwd_t)(const mms_conv_shape*, int, int, int, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, const float*, const float*, const float*, float*, float*,
                     float*, float*, float*, void*, size_t, void*);
typedef int (*bwd64_t)(const mms_conv_shape*, int, int, int, const double*, const double*, const double*,
                       const double*, const double*, const double*, const double*, const double*, const double*,
                       const double*, double*, double*, double*, double*, double*, void*, size_t, void*);
typedef size_t (*query_t)(const mms_conv_shape*, int, int, int);

int mms_conv_stage_train_abi_is_c_probe(void) {
  const fwd_t f[3] = {&mms_conv_stage_train_forward_f32, &mms_conv_stage_train_forward_sequence_f32,
                      &mms_conv_stage_train_forward_fused_f32};
  const fwd64_t f64 = &mms_conv_stage_train_forward_f64;
  const bwd_t b = &mms_conv_stage_train_backward_f32;
  const bwd64_t b64 = &mms_conv_stage_train_backward_f64;
  const query_t q[4] = {&mms_conv_stage_train_workspace_bytes, &mms_conv_stage_train_workspace_bytes_f64,
                        &mms_conv_stage_train_sequence_workspace_bytes, &mms_conv_stage_train_fused_workspace_bytes};
  int (*const route)(const mms_conv_shape*, int, int, int) = &mms_conv_stage_train_route;
  mms_conv_shape s = {50, 4, 40, 40, 32, 5, 5, 1, 1, 0, 0, 1, 1, 1};
  return f[0] && f[1] && f[2] && f64 && b && b64 && q[0] && q[1] && q[2] && q[3] && route && s.group == 1 &&
         MMS_STAGE_POOL_AVE == 0 && MMS_STAGE_POOL_MAX == 1 && MMS_CONV_STAGE_TRAIN_ROUTE_FUSED == 1 &&
         MMS_CONV_STAGE_TRAIN_ROUTE_SEQUENCE == 0 && MMS_CONV_STAGE_TRAIN_ROUTE_NONE == -1 && MMS_ERR_WORKSPACE == 3;
}
