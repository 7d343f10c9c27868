/* tests/native/score_tail_abi_is_c.c -- include/mms_score_tail.h must be consumable from plain C: `gcc -std=c99 -Wall
 * -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_score_tail.h"

typedef int (*fwd_t)(const mms_score_tail_shape*, const float*, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                     const float*, float*, float*, float*, float*, void*, size_t, void*);
typedef int (*fwd64_t)(const mms_score_tail_shape*, const double*, const double*, const double*, const double*,
                       const double*, const double*, const double*, const double*, const double*, const double*,
                       const double*, const double*, const double*, double*, double*, double*, double*, void*, size_t,
                       void*);
typedef size_t (*query_t)(const mms_score_tail_shape*);

int mms_score_tail_abi_is_c_probe(void) {
  const fwd_t f[3] = {&mms_score_tail_forward_f32, &mms_score_tail_forward_sequence_f32,
                      &mms_score_tail_forward_fused_f32};
  const fwd64_t f64 = &mms_score_tail_forward_f64;
  const query_t q[3] = {&mms_score_tail_workspace_bytes, &mms_score_tail_workspace_bytes_f64,
                        &mms_score_tail_sequence_workspace_bytes};
  int (*const route)(const mms_score_tail_shape*) = &mms_score_tail_route;
  mms_score_tail_shape s = {{50, 32, 9, 9, 64, 5, 5, 1, 1, 0, 0, 1, 1, 1}, 5, 5, MMS_STAGE_POOL_AVE, 2, 32, 2,
                            MMS_HEAD_NORM_VALID, 0, 0};
  return f[0] && f[1] && f[2] && f64 && q[0] && q[1] && q[2] && route && s.C == 2 && s.conv.K == 64 &&
         MMS_STAGE_POOL_MAX == 1 && MMS_SCORE_TAIL_ROUTE_FUSED == 1 && MMS_SCORE_TAIL_ROUTE_SEQUENCE == 0 &&
         MMS_SCORE_TAIL_ROUTE_NONE == -1 && MMS_ERR_WORKSPACE == 3;
}
