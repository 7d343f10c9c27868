/* tests/native/conv_maxpool_stage_abi_is_c.c -- include/mms_conv_maxpool_stage.h must be consumable from plain C: `gcc
 * -std=c99 -Wall -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_conv_maxpool_stage.h"

typedef int (*fwd_t)(const mms_conv_shape*, int, int, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, float*, float*, void*, size_t, void*);
typedef int (*fwd64_t)(const mms_conv_shape*, int, int, const double*, const double*, const double*, const double*,
                       const double*, const double*, const double*, double*, double*, void*, size_t, void*);
typedef int (*fused_t)(const mms_conv_shape*, int, int, const float*, const float*, const float*, const float*,
                       const float*, const float*, const float*, float*, float*, void*);
typedef size_t (*query_t)(const mms_conv_shape*, int, int);

int mms_conv_maxpool_stage_abi_is_c_probe(void) {
  const fwd_t f[2] = {&mms_conv_maxpool_stage_forward_f32, &mms_conv_maxpool_stage_forward_sequence_f32};
  const fwd64_t f64 = &mms_conv_maxpool_stage_forward_f64;
  const fused_t fused = &mms_conv_maxpool_stage_forward_fused_f32;
  const query_t q[3] = {&mms_conv_maxpool_stage_workspace_bytes, &mms_conv_maxpool_stage_workspace_bytes_f64,
                        &mms_conv_maxpool_stage_sequence_workspace_bytes};
  int (*const route)(const mms_conv_shape*, int, int) = &mms_conv_maxpool_stage_route;
  mms_conv_shape s = {1, 1, 40, 40, 64, 5, 5, 1, 1, 0, 0, 1, 1, 1};
  return f[0] && f[1] && f64 && fused && q[0] && q[1] && q[2] && route && s.group == 1 &&
         MMS_CONV_MAXPOOL_STAGE_ROUTE_FUSED == 1 && MMS_CONV_MAXPOOL_STAGE_ROUTE_SEQUENCE == 0 &&
         MMS_CONV_MAXPOOL_STAGE_ROUTE_NONE == -1 && MMS_CONV_ROUTE_FAST == 1 && MMS_ERR_WORKSPACE == 3;
}
