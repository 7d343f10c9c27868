/* tests/native/pool_abi_is_c.c -- include/mms_pool.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_pool.h"

typedef int (*dims_t)(const mms_pool_shape*, int*, int*);
typedef int (*fwd32_t)(const mms_pool_shape*, const float*, float*, int*, float*, void*);
typedef int (*fwd64_t)(const mms_pool_shape*, const double*, double*, int*, double*, void*);
typedef int (*bwd32_t)(const mms_pool_shape*, const float*, const int*, const float*, float*, void*);
typedef int (*bwd64_t)(const mms_pool_shape*, const double*, const int*, const double*, double*, void*);
typedef int (*tf32_t)(long long, const float*, float*, void*);
typedef int (*tf64_t)(long long, const double*, double*, void*);
typedef int (*tb32_t)(long long, const float*, const float*, float*, void*);
typedef int (*tb64_t)(long long, const double*, const double*, double*, void*);

int mms_pool_abi_is_c_probe(void) {
  const dims_t d = &mms_pool_output_dims;
  const fwd32_t f32 = &mms_pool_forward_f32;
  const fwd64_t f64 = &mms_pool_forward_f64;
  const bwd32_t b32 = &mms_pool_backward_f32;
  const bwd64_t b64 = &mms_pool_backward_f64;
  const tf32_t tf32 = &mms_tanh_forward_f32;
  const tf64_t tf64 = &mms_tanh_forward_f64;
  const tb32_t tb32 = &mms_tanh_backward_f32;
  const tb64_t tb64 = &mms_tanh_backward_f64;
  mms_pool_shape s;
  s.N = 1; s.C = 1; s.H = 4; s.W = 4;
  s.kernel_h = 2; s.kernel_w = 2; s.stride_h = 2; s.stride_w = 2; s.pad_h = 0; s.pad_w = 0;
  s.method = MMS_POOL_MAX;
  return d && f32 && f64 && b32 && b64 && tf32 && tf64 && tb32 && tb64 && s.method == 1 && MMS_POOL_AVE == 0 &&
         MMS_POOL_STOCHASTIC == 2 && MMS_ERR_UNSUPPORTED == 2;
}
