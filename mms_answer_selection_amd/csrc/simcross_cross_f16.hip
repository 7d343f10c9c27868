// csrc/simcross_cross_f16.hip -- fp16-STORAGE SimCross dist_mode 0 (cosine) and 1 (Euclidean) on W1 x W2 word grids
// (mms_simcross_forward_f16 / _backward_f16 / _forward_backward_f16, and mms_embed_simcross_forward_f16, the forward
// straight from word ids and a half embedding table): q, a, dq, da are IEEE halves in HBM; top, top_diff and the norms
// fp32.  The _Float16 instantiations of the word-grid kernels and launch plan of cross_grid.h, which says what a half
// call computes (the fp32 call's arithmetic on the exactly-widened inputs, each gradient element rounded once), and
// the four entry points.
//
// Compiled with -ffp-contract=off like every source of the library.
#include "cross_grid.h"

namespace mms {

// =============================== entry points ===============================
// mms_abi.hip has checked the arguments: mode 0 or 1, not W1 == W2 == 1 (the gathered forward serves that too), N >= 1.

int simcross_grid_forward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, float* top,
                              float* norm0, float* norm1, hipStream_t s) {
  cross_forward<_Float16, false>(mode, N, W1, W2, D, static_cast<const _Float16*>(q), static_cast<const _Float16*>(a),
                                 top, norm0, norm1, s, kNoGather);
  return launch_status();
}

// top = SimCross(Embed(index_q), Embed(index_a)) for dist_mode 0 / 1 from a half table (K, D): embed_simcross_forward
// (simcross_cross.hip) with the table's halves widened by the gathering loads.  No workspace, one launch for Euclid and
// three for cosine.
int embed_simcross_forward_f16(int mode, int N, int W1, int W2, int D, int K, const float* index_q, const float* index_a,
                               const void* table, const float* embed_bias, float* top, float* norm0, float* norm1,
                               hipStream_t s) {
  const _Float16* t = static_cast<const _Float16*>(table);
  cross_forward<_Float16, true>(mode, N, W1, W2, D, t, t, top, norm0, norm1, s,
                                CrossGather{index_q, index_a, K, embed_bias});
  return launch_status();
}

int simcross_grid_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, const float* top,
                               const float* top_diff, const float* norm0, const float* norm1, void* dq, void* da,
                               hipStream_t s) {
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  cross_backward<_Float16>(mode, N, W1, W2, D, static_cast<const _Float16*>(q), static_cast<const _Float16*>(a), top,
                           top_diff, norm0, norm1, static_cast<_Float16*>(dq), static_cast<_Float16*>(da), exact, s);
  return launch_status();
}

int simcross_grid_forward_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a,
                                       const float* top_diff, float* top, float* norm0, float* norm1, void* dq,
                                       void* da, hipStream_t s) {
  const bool exact = euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE;
  const _Float16* qh = static_cast<const _Float16*>(q);
  const _Float16* ah = static_cast<const _Float16*>(a);
  cross_forward<_Float16, false>(mode, N, W1, W2, D, qh, ah, top, norm0, norm1, s, kNoGather);
  cross_backward<_Float16>(mode, N, W1, W2, D, qh, ah, top, top_diff, norm0, norm1, static_cast<_Float16*>(dq),
                           static_cast<_Float16*>(da), exact, s);
  return launch_status();
}

}  // namespace mms
