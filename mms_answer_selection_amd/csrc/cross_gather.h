// csrc/cross_gather.h -- the Embed gather fused into the word-grid SimCross forward (dist_mode 0 / 1): the one
// definition of the id clamp and of the gather's operands, used by the forward and norm kernels of cross_grid.h for
// either element type of the table (float, half).
#ifndef MMS_CROSS_GATHER_H_
#define MMS_CROSS_GATHER_H_

#include "mms_common.h"

namespace mms {

// Word id stored as a float (Caffe feeds ids as Dtype), clamped into the table like embed_fwd_kernel.
__device__ __forceinline__ int gather_id(float v, int K) {
  const int i = (int)v;
  return i < 0 ? 0 : (i >= K ? K - 1 : i);
}

// Embed fused into the load: with iq != nullptr, q and a are both the embedding
// TABLE (K x D) and row j of pair n is table row iq[n*W1 + j] (ia likewise) -- the (N, W, D) blobs
// the Embed layer would write and SimCross read back never exist.
struct CrossGather {
  const float* iq;
  const float* ia;
  int K;
  const float* bias;     // the Embed layer's bias (D floats) or nullptr: row value = bias[d] + table[id][d], the
                         // one rounding of embed_layer.cpp:146-151 (gemm with alpha = beta = 1)
};

}  // namespace mms
#endif  // MMS_CROSS_GATHER_H_
