/* tests/native/solver_abi_is_c.c -- include/mms_solver.h must be consumable from plain C: `gcc -std=c99 -Wall -Werror
 * -pedantic -fsyntax-only`.  Every entry point is referenced with its declared type. */
#include <stddef.h>
#include "mms_solver.h"

typedef size_t (*query_t)(const mms_solver_param*, const mms_solver_blob*, int);
typedef int (*step_t)(const mms_solver_param*, const mms_solver_blob*, int, float, float*, void*, size_t, void*);
typedef int (*step64_t)(const mms_solver_param*, const mms_solver_blob*, int, double, double*, void*, size_t, void*);

int mms_solver_abi_is_c_probe(void) {
  const query_t q[2] = {&mms_solver_workspace_bytes, &mms_solver_workspace_bytes_f64};
  const step_t s = &mms_solver_step_f32;
  const step64_t s64 = &mms_solver_step_f64;
  mms_solver_param p = {MMS_SOLVER_ADADELTA, MMS_SOLVER_L2, 1, MMS_SOLVER_DIFF_ZERO, 0.95f, 5e-7f, 5e-4f, -1.f};
  mms_solver_blob b = {NULL, NULL, NULL, NULL, 0, 1.f, 1.f};
  return q[0] && q[1] && s && s64 && p.iter_size == 1 && b.count == 0 && MMS_SOLVER_SGD == 0 && MMS_SOLVER_L1 == 1 &&
         MMS_SOLVER_DIFF_UPDATE == 0 && MMS_SOLVER_CHUNK % 4 == 0 && MMS_SOLVER_BLOBS_PER_LAUNCH >= 1 &&
         MMS_ERR_WORKSPACE == 3;
}
