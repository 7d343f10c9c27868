// csrc/train_tail_check.h -- the refusals of the TRAIN-phase tail's calls, once, for csrc/train_tail.hip
// (include/mms_train_tail.h) and csrc/train_tail_backward.hip (include/mms_train_tail_backward.h): the shape's, in the
// header's order, and the backward's argument list.  Host text only.
#ifndef MMS_TRAIN_TAIL_CHECK_H_
#define MMS_TRAIN_TAIL_CHECK_H_

#include "conv_pool_tile.h"
#include "head_tile.h"
#include "mms_score_tail.h"

namespace mms {

struct TrainTailDims : StageDims {
  mms_head_shape hs;         // the head call's shape
  HeadDims hd;
  int pool;
};

// the refusal of the shape, else MMS_OK and *g
inline int train_tail_check(const mms_score_tail_shape* s, int phase, float dropout_ratio, TrainTailDims* g) {
  if (!s) return MMS_ERR_INVALID_ARG;
  if (s->pool != MMS_STAGE_POOL_AVE && s->pool != MMS_STAGE_POOL_MAX) return MMS_ERR_INVALID_ARG;
  const int rc = stage_window_check(&s->conv, s->ph, s->pw, g);
  if (rc != MMS_OK) return rc;
  if (g->d.OH != g->ph || g->d.OW != g->pw) return MMS_ERR_INVALID_ARG;
  if (phase != MMS_HEAD_TRAIN) return MMS_ERR_INVALID_ARG;
  g->max = s->pool == MMS_STAGE_POOL_MAX;
  g->pool = s->pool;
  g->hs = {g->d.N, g->d.K, s->F1, s->H, s->C, MMS_HEAD_TRAIN, dropout_ratio, s->normalization, s->has_ignore_label,
           s->ignore_label};
  return head_check(&g->hs, &g->hd);
}

// The backward's arguments, for a checked shape with N > 0: MMS_ERR_INVALID_ARG for a NULL input, no output at all, or
// two arrays at one address (the workspace included); else MMS_OK, *doverlap NULL where F1 == 0 (an array of no
// elements) and *stage = whether any output of the stage's backward is asked for.
template <typename T>
int train_tail_backward_args(const TrainTailDims& g, const T* x, const T* w, const T* y, const T* flt, const T* save_pool,
                             const T* scale, const T* shift, const T* save_mean, const T* save_std, const T* overlap,
                             const T* w1, const T* w2, const unsigned* mask, const T* h, const T* prob, const T* label,
                             const T* dx, const T* dw, const T* db, const T* dscale, const T* dshift, T** doverlap,
                             const T* w1d, const T* b1d, const T* w2d, const T* b2d, const void* workspace, bool* stage) {
  if (!x || !w || !y || !flt || !save_pool || !scale || (g.max && !shift) || !save_mean || !save_std || !w1 || !w2 ||
      !mask || !h || !prob || !label || (g.hd.F1 > 0 && !overlap))
    return MMS_ERR_INVALID_ARG;
  if (g.hd.F1 == 0) *doverlap = nullptr;      // an array of no elements
  *stage = dx || dw || db || dscale || dshift;
  const bool head = *doverlap || w1d || b1d || w2d || b2d;
  if (!*stage && !head) return MMS_ERR_INVALID_ARG;
  const void* const arrays[] = {x,    w,    y,     flt, save_pool, scale,  shift,  save_mean, save_std,  overlap, w1,  w2,  mask,
                                h,    prob, label, dx,  dw,        db,     dscale, dshift,    *doverlap, w1d,     b1d, w2d, b2d};
  const void* const ws_only[] = {workspace};
  if (outputs_alias(arrays, ws_only)) return MMS_ERR_INVALID_ARG;     // any two arrays, the workspace included
  return MMS_OK;
}

}  // namespace mms
#endif  // MMS_TRAIN_TAIL_CHECK_H_
