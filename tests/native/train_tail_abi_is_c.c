/* tests/native/train_tail_abi_is_c.c -- include/mms_train_tail.h must be consumable from plain C: `gcc -std=c99 -Wall
 * -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_train_tail.h"

typedef const mms_score_tail_shape* shape_t;
typedef int (*fwd_t)(shape_t, int, float, float, const float*, const float*, const float*, const float*, const float*,
                     float*, float*, const float*, const float*, const float*, const unsigned int*, const float*,
                     const float*, const float*, float*, float*, float*, float*, float*, float*, float*, float*, void*,
                     size_t, void*);
typedef int (*fwd64_t)(shape_t, int, double, float, const double*, const double*, const double*, const double*,
                       const double*, double*, double*, const double*, const double*, const double*,
                       const unsigned int*, const double*, const double*, const double*, double*, double*, double*,
                       double*, double*, double*, double*, double*, void*, size_t, void*);
typedef int (*bwd_t)(shape_t, int, float, float, const float*, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                     const unsigned int*, const float*, const float*, const float*, float*, float*, float*, float*,
                     float*, float*, float*, float*, float*, float*, void*, size_t, void*);
typedef int (*bwd64_t)(shape_t, int, float, double, const double*, const double*, const double*, const double*,
                       const double*, const double*, const double*, const double*, const double*, const double*,
                       const double*, const double*, const unsigned int*, const double*, const double*, const double*,
                       double*, double*, double*, double*, double*, double*, double*, double*, double*, double*, void*,
                       size_t, void*);
typedef size_t (*query_t)(shape_t);

int mms_train_tail_abi_is_c_probe(void) {
  const fwd_t f[3] = {&mms_train_tail_forward_f32, &mms_train_tail_forward_sequence_f32,
                      &mms_train_tail_forward_fused_f32};
  const fwd64_t f64 = &mms_train_tail_forward_f64;
  const bwd_t b = &mms_train_tail_backward_f32;
  const bwd64_t b64 = &mms_train_tail_backward_f64;
  const query_t q[4] = {&mms_train_tail_workspace_bytes, &mms_train_tail_workspace_bytes_f64,
                        &mms_train_tail_sequence_workspace_bytes, &mms_train_tail_fused_workspace_bytes};
  int (*const route)(shape_t) = &mms_train_tail_route;
  mms_score_tail_shape s = {{50, 32, 9, 9, 64, 5, 5, 1, 1, 0, 0, 1, 1, 1}, 5, 5, MMS_STAGE_POOL_AVE, 2, 32, 2,
                            MMS_HEAD_NORM_VALID, 0, 0};
  return f[0] && f[1] && f[2] && f64 && b && b64 && q[0] && q[1] && q[2] && q[3] && route && s.C == 2 &&
         s.conv.K == 64 && MMS_STAGE_POOL_MAX == 1 && MMS_TRAIN_TAIL_ROUTE_FUSED == 1 &&
         MMS_TRAIN_TAIL_ROUTE_SEQUENCE == 0 && MMS_TRAIN_TAIL_ROUTE_NONE == -1 && MMS_HEAD_TRAIN == 0 &&
         MMS_ERR_WORKSPACE == 3;
}
