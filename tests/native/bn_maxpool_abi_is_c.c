/* tests/native/bn_maxpool_abi_is_c.c -- include/mms_bn_maxpool.h must be consumable from plain C: `gcc -std=c99 -Wall
 * -Werror -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_bn_maxpool.h"

typedef size_t (*query_t)(int, int, int, int, int, int);
typedef int (*fwd_t)(int, int, int, int, int, int, int, float, const float*, const float*, const float*, float*, float*,
                     float*, float*, float*, float*, void*, size_t, void*);
typedef int (*bwd_t)(int, int, int, int, int, int, const float*, const float*, const float*, const float*, const float*,
                     const float*, const float*, const float*, float*, float*, float*, void*, size_t, void*);
typedef int (*fwd64_t)(int, int, int, int, int, int, int, double, const double*, const double*, const double*, double*,
                       double*, double*, double*, double*, double*, void*, size_t, void*);
typedef int (*bwd64_t)(int, int, int, int, int, int, const double*, const double*, const double*, const double*,
                       const double*, const double*, const double*, const double*, double*, double*, double*, void*,
                       size_t, void*);

int mms_bn_maxpool_abi_is_c_probe(void) {
  const query_t q[2] = {&mms_bn_maxpool_tanh_workspace_bytes, &mms_bn_maxpool_tanh_workspace_bytes_f64};
  const fwd_t f = &mms_bn_maxpool_tanh_forward_f32;
  const bwd_t b = &mms_bn_maxpool_tanh_backward_f32;
  const fwd64_t f64 = &mms_bn_maxpool_tanh_forward_f64;
  const bwd64_t b64 = &mms_bn_maxpool_tanh_backward_f64;
  return q[0] && q[1] && f && b && f64 && b64 && MMS_ERR_WORKSPACE == 3 && MMS_ERR_INVALID_ARG == 1;
}
