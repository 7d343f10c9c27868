/* tests/native/dropout_abi_is_c.c -- include/mms_dropout.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_dropout.h"

typedef unsigned long long u64;
typedef int (*thr32_t)(float, unsigned int*, float*);
typedef int (*thr64_t)(double, unsigned int*, double*);
typedef int (*apply32_t)(const float*, float*, long long, float, int, u64, u64, u64, void*);
typedef int (*apply64_t)(const double*, double*, long long, double, int, u64, u64, u64, void*);
typedef int (*mask32_t)(unsigned int*, long long, float, u64, u64, u64, void*);
typedef int (*mask64_t)(unsigned int*, long long, double, u64, u64, u64, void*);

int mms_dropout_abi_is_c_probe(void) {
  const thr32_t t32 = &mms_dropout_threshold_f32;
  const thr64_t t64 = &mms_dropout_threshold_f64;
  const apply32_t a32[2] = {&mms_dropout_forward_f32, &mms_dropout_backward_f32};
  const apply64_t a64[2] = {&mms_dropout_forward_f64, &mms_dropout_backward_f64};
  const mask32_t m32 = &mms_dropout_mask_u32;
  const mask64_t m64 = &mms_dropout_mask_u32_f64;
  return t32 && t64 && a32[0] && a32[1] && a64[0] && a64[1] && m32 && m64 && MMS_DROPOUT_TRAIN == 0 &&
         MMS_DROPOUT_TEST == 1 && MMS_DROPOUT_THREADS % 64 == 0 && MMS_DROPOUT_MAX_BLOCKS >= 1 && MMS_DROPOUT_GROUPS_PER_TRIP >= 1 &&
         MMS_ERR_INVALID_ARG == 1;
}
