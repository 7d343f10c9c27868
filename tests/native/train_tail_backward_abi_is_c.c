/* tests/native/train_tail_backward_abi_is_c.c -- include/mms_train_tail_backward.h must be consumable from plain C:
 * `gcc -std=c99 -Wall -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type, and the
 * routed and the fused call have the type of mms_train_tail_backward_f32. */
#include <stddef.h>
#include "mms_train_tail_backward.h"

typedef const mms_score_tail_shape* shape_t;
typedef int (*bwd_t)(shape_t, int, float, float, const float*, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                     const unsigned int*, const float*, const float*, const float*, float*, float*, float*, float*,
                     float*, float*, float*, float*, float*, float*, void*, size_t, void*);
typedef size_t (*query_t)(shape_t);

int mms_train_tail_backward_abi_is_c_probe(void) {
  const bwd_t b[3] = {&mms_train_tail_backward_f32, &mms_train_tail_backward_routed_f32,
                      &mms_train_tail_backward_fused_f32};
  const query_t q[2] = {&mms_train_tail_backward_workspace_bytes, &mms_train_tail_backward_fused_workspace_bytes};
  int (*const route)(shape_t) = &mms_train_tail_backward_route;
  return b[0] && b[1] && b[2] && q[0] && q[1] && route && MMS_TRAIN_TAIL_ROUTE_FUSED == 1;
}
