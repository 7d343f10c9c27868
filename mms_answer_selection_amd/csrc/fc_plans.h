// csrc/fc_plans.h -- what the host decides for the calls of include/mms_fc.h before it launches: each shape's
// judgement, the slabs of the row sums, InnerProduct's route and the kernel each of its products takes, and the grids.
// Inline host text with no HIP call, so that tests/native/fc_plans_host.cpp sweeps it where there is no GPU.
#ifndef MMS_FC_PLANS_H_
#define MMS_FC_PLANS_H_

#include <limits.h>
#include <stddef.h>

#include "mms_fc.h"

namespace mms {

constexpr int kFcThreads = 256;
// One resident round of the chip: 8 workgroups on each of 256 CUs.  A larger call strides over its work.
constexpr int kFcMaxBlocks = 2048;

// ---- InnerProduct --------------------------------------------------------------------------------------------------
// Slabs of the row range [0, M) that the sums over m (w_diff, b_diff) are taken in: 128 rows each -- a multiple of the
// 32 rows the tile kernel has in flight at once -- and longer, in steps of 32, where there would be more than
// kFcMaxSlabs of them (M > 8192).
constexpr int kFcSlabRows = 128;
constexpr int kFcMaxSlabs = 64;
// The route of the float calls, per pass (fc_ip_route; DESIGN.md 4.18 has the times behind it).  Below kFcFastMinMacs
// multiply-adds (M * K * N_out) a product is a handful of waves whichever kernel runs it, and the generic one has no
// tile to pad: generic; no shape that small was timed.  From there on:
//   forward    fast where K is at least kFcFastFwdMinK (a generic thread walks K serially; timed at K = 203), or where
//              top is at most kFcNarrowMax rows or columns (timed at fc2, N_out = 2: level with generic).  A top wider
//              than that with a shorter K (network_v4's fc1, K = 66) stays generic: the tile kernel was not timed
//              there, and the generic forward is within 2 us of an empty launch.
//   backward   fast where the rows make more than one slab (M > 128; timed at M = 1517), generic below (M = 50: the
//              tile kernel was not timed there).
// Neither threshold was searched: each lies between two timed shapes.  Every product of the fast route, whatever its
// extents, takes the one tile kernel of csrc/fc.hip (16 x 16 tiles of v_mfma_f32_16x16x4_f32, operands straight from
// memory, strided): the head's operands are a few KB.  With M <= 16 and K, N_out in the thousands it is still picked
// and its strided, unshared loads are then a poor fit; no such shape was timed.  gemm32.h's gemm_launch is NOT used:
// it picks its kernel, and with it the pairing of k inside an MFMA, by the operands' addresses, so the same call on
// an array shifted by one float would give other words.
constexpr int kFcFastMinMacs = 2048;
constexpr int kFcFastFwdMinK = 128;
constexpr int kFcNarrowMax = 16;

struct FcDims {
  int M, K, N, transpose, bias;
};

// The shape's judgement (the refusal table of include/mms_fc.h up to the pointers); *d is set on MMS_OK.
inline int fc_ip_check(const mms_inner_product_shape* s, FcDims* d) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->M < 0 || s->K < 1 || s->N_out < 1 || (s->transpose != 0 && s->transpose != 1) ||
      (s->bias_term != 0 && s->bias_term != 1))
    return MMS_ERR_INVALID_ARG;
  const long long M = s->M, K = s->K, N = s->N_out;
  if (M * K > INT_MAX || M * N > INT_MAX || K * N > INT_MAX) return MMS_ERR_INVALID_ARG;
  const FcDims out = {s->M, s->K, s->N_out, s->transpose, s->bias_term};
  *d = out;
  return MMS_OK;
}

inline int fc_slab_rows(int M) {
  const long long per = ((long long)M + kFcMaxSlabs - 1) / kFcMaxSlabs, r = (per + 31) / 32 * 32;
  return (int)(r < kFcSlabRows ? kFcSlabRows : r);
}
inline int fc_slabs(int M) {
  const int r = fc_slab_rows(M);
  return (int)(((long long)M + r - 1) / r);
}

// elements of workspace the backward takes: every slab's partial of w_diff, then every slab's partial of b_diff
inline long long fc_ip_workspace_elems(const FcDims& d) {
  return d.M == 0 ? 0 : (long long)fc_slabs(d.M) * ((long long)d.K * d.N + d.N);
}

// pass: MMS_FC_PASS_FORWARD / _BACKWARD; MMS_FC_ROUTE_NONE for any other
inline int fc_ip_route(const FcDims& d, int pass) {
  if (pass != MMS_FC_PASS_FORWARD && pass != MMS_FC_PASS_BACKWARD) return MMS_FC_ROUTE_NONE;
  if ((long long)d.M * d.K * d.N < kFcFastMinMacs) return MMS_FC_ROUTE_GENERIC;
  const bool fast = pass == MMS_FC_PASS_FORWARD ? (d.M <= kFcNarrowMax || d.N <= kFcNarrowMax || d.K >= kFcFastFwdMinK)
                                                : fc_slabs(d.M) > 1;
  return fast ? MMS_FC_ROUTE_FAST : MMS_FC_ROUTE_GENERIC;
}

// The tile kernel's grid: x workgroups of four waves stride over the 16 x 16 tiles, y = the slabs of the inner index
struct FcNarrowGrid {
  int row_tiles, col_tiles, blocks_x, blocks_y;
};
inline FcNarrowGrid fc_narrow_grid(int rows, int cols, int slabs) {
  FcNarrowGrid g;
  g.row_tiles = (int)(((long long)rows + 15) / 16);
  g.col_tiles = (int)(((long long)cols + 15) / 16);
  const long long tiles = (long long)g.row_tiles * g.col_tiles, b = (tiles + 3) / 4;
  g.blocks_x = (int)(b < kFcMaxBlocks ? b : kFcMaxBlocks);
  g.blocks_y = slabs;
  return g;
}

// Workgroups of a sweep over `units` units of work, one per thread and trip.
inline int fc_sweep_blocks(long long units) {
  const long long b = (units + kFcThreads - 1) / kFcThreads;
  return (int)(b < 1 ? 1 : b < kFcMaxBlocks ? b : kFcMaxBlocks);
}

// ---- Softmax, SoftmaxWithLoss --------------------------------------------------------------------------------------
// inner == 1: a thread per row up to this many channels, a wave per row beyond.  inner > 1: a thread per (o, k), lanes
// along k.
constexpr int kSoftmaxThreadRowMax = 32;
// The loss and the count of labels not ignored are summed over the P = outer * inner positions in slabs of 64, longer
// where there would be more than 256 of them: one workgroup of 256 threads takes a slab per thread, then adds them.
constexpr int kLossSlabMin = 64;
constexpr int kLossMaxSlabs = 256;

struct SoftmaxDims {
  int outer, channels, inner;
};

inline int fc_softmax_check(int outer, int channels, int inner, SoftmaxDims* d) {
  if (outer < 0 || channels < 1 || inner < 1) return MMS_ERR_INVALID_ARG;
  const long long oi = (long long)outer * inner;
  if (oi > INT_MAX || oi * channels > INT_MAX) return MMS_ERR_INVALID_ARG;
  const SoftmaxDims out = {outer, channels, inner};
  *d = out;
  return MMS_OK;
}

inline int fc_loss_check(const mms_softmax_loss_shape* s, SoftmaxDims* d) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->normalization < MMS_LOSS_NORM_FULL || s->normalization > MMS_LOSS_NORM_NONE) return MMS_ERR_INVALID_ARG;
  return fc_softmax_check(s->outer, s->channels, s->inner, d);
}

inline int fc_loss_slab_len(long long P) {
  const long long per = (P + kLossMaxSlabs - 1) / kLossMaxSlabs;
  return (int)(per < kLossSlabMin ? kLossSlabMin : per);
}
inline int fc_loss_slabs(long long P) {
  const int len = fc_loss_slab_len(P);
  return (int)((P + len - 1) / len);
}
// per slab a Dtype partial of the loss; one Dtype for the backward's scalar; per slab an int count
inline size_t fc_loss_workspace_bytes(long long P, size_t elem) {
  if (P == 0) return 0;
  const size_t s = (size_t)fc_loss_slabs(P);
  return (s + 1) * elem + s * sizeof(int);
}

// ---- Concat --------------------------------------------------------------------------------------------------------
struct ConcatDims {
  int num_concats, inner, nb, top_axis;
  int extent[MMS_CONCAT_MAX_BOTTOMS], offset[MMS_CONCAT_MAX_BOTTOMS];
};

inline int fc_concat_check(const mms_concat_shape* s, ConcatDims* d) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->num_concats < 0 || s->concat_input_size < 1 || s->num_bottoms < 1 || s->num_bottoms > MMS_CONCAT_MAX_BOTTOMS)
    return MMS_ERR_INVALID_ARG;
  ConcatDims out = {};
  out.num_concats = s->num_concats;
  out.inner = s->concat_input_size;
  out.nb = s->num_bottoms;
  long long axis = 0;
  for (int b = 0; b < s->num_bottoms; ++b) {
    if (s->axis_extent[b] < 0) return MMS_ERR_INVALID_ARG;
    out.extent[b] = s->axis_extent[b];
    out.offset[b] = (int)axis;
    axis += s->axis_extent[b];
    if (axis > INT_MAX) return MMS_ERR_INVALID_ARG;
  }
  if (axis < 1) return MMS_ERR_INVALID_ARG;
  const long long row = axis * s->concat_input_size;
  if (row > INT_MAX || row * (s->num_concats > 0 ? s->num_concats : 1) > INT_MAX) return MMS_ERR_INVALID_ARG;
  out.top_axis = (int)axis;
  *d = out;
  return MMS_OK;
}

}  // namespace mms
#endif  // MMS_FC_PLANS_H_
