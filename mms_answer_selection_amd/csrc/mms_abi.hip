// csrc/mms_abi.hip -- extern "C" entry points declared in include/mms.h:
// argument validation and dispatch only; kernels live in the sibling files.
#include <limits.h>

#include "mms_internal.h"

using namespace mms;

// The argument rules, each family's once for all of its element types and entry points.  A `*_refusal` returns the
// code to refuse with, or MMS_OK: go on -- unless the batch is empty, which is MMS_OK as well and enqueues nothing.
// `arrays`: every array the call requires whatever the dist_mode is there.
namespace {
// element counts must fit the int indexing the reference itself uses
bool fits_int(long long count) { return count <= INT_MAX; }

bool dims_ok(int mode, int N, int W1, int W2, int D, int M) {
  if (mode < 0 || mode > 2) return false;
  if (N < 0 || W1 <= 0 || W2 <= 0 || D <= 0 || M <= 0) return false;
  if (mode != 2 && M != 1) return false;
  return fits_int((long long)N * W1 * D) && fits_int((long long)N * W2 * D) && fits_int((long long)N * M * W1 * W2);
}
// a table of K rows of D for the Embed-fused scoring calls
bool table_ok(int K, int D) { return K > 0 && fits_int((long long)K * D); }

// SimCross on fp32 and fp64 storage: the sizes, the empty batch, the arrays, then those of dist_mode 0 and of dist_mode 2
int simcross_refusal(int dist_mode, int N, int W1, int W2, int D, int M, bool arrays, const void* norm0,
                     const void* norm1, const void* W) {
  if (!dims_ok(dist_mode, N, W1, W2, D, M)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  if (!arrays || (dist_mode == 0 && (!norm0 || !norm1)) || (dist_mode == 2 && !W)) return MMS_ERR_INVALID_ARG;
  return MMS_OK;
}
// ... and a backward, in dist_mode 2, its parameter gradients
int simcross_backward_refusal(int dist_mode, int N, int W1, int W2, int D, int M, bool arrays, const void* norm0,
                              const void* norm1, const void* W, int bias_term, const void* dW, const void* dbias) {
  const int rc = simcross_refusal(dist_mode, N, W1, W2, D, M, arrays, norm0, norm1, W);
  if (rc != MMS_OK || N == 0) return rc;
  return dist_mode == 2 && (!dW || (bias_term && !dbias)) ? MMS_ERR_INVALID_ARG : MMS_OK;
}

// fp16-storage sentence-vector pairs (W1 == W2 == 1)
int rows_f16_refusal(int N, int D, bool arrays) {
  if (N < 0 || D <= 0 || !fits_int((long long)N * D)) return MMS_ERR_INVALID_ARG;
  return N == 0 || arrays ? MMS_OK : MMS_ERR_INVALID_ARG;
}

// The word-grid fp16-storage calls of dist_mode 0 / 1
int grid_f16_refusal(int dist_mode, int N, int W1, int W2, int D, bool arrays, const float* norm0, const float* norm1) {
  if (!dims_ok(dist_mode, N, W1, W2, D, 1)) return MMS_ERR_INVALID_ARG;
  if (dist_mode == 2) return MMS_ERR_UNSUPPORTED;                 // the bilinear mode: mms_simcross_bilinear_*_f16
  if (W1 == 1 && W2 == 1) return MMS_ERR_UNSUPPORTED;             // the rows family: mms_simcross_{euclid,cosine}_*_f16
  if (N == 0) return MMS_OK;
  return arrays && (dist_mode != 0 || (norm0 && norm1)) ? MMS_OK : MMS_ERR_INVALID_ARG;
}
// ... and of dist_mode 2
int bilinear_f16_refusal(int N, int W1, int W2, int D, int M, bool arrays) {
  if (!dims_ok(2, N, W1, W2, D, M)) return MMS_ERR_INVALID_ARG;
  if (W1 == 1 && W2 == 1) return MMS_ERR_UNSUPPORTED;             // the rows family of the learned metric: mms_simmatrix_*_f16
  return N == 0 || arrays ? MMS_OK : MMS_ERR_INVALID_ARG;
}

// mms_embed_simcross_forward_f32 / _f16
int embed_simcross_refusal(int dist_mode, int N, int W1, int W2, int D, int K, bool arrays, const float* norm0,
                           const float* norm1) {
  if (dist_mode != 0 && dist_mode != 1) return MMS_ERR_UNSUPPORTED;   // bilinear: mms_embed_simcross_bilinear_forward_*
  if (!dims_ok(dist_mode, N, W1, W2, D, 1) || !table_ok(K, D)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;
  return arrays && (dist_mode != 0 || (norm0 && norm1)) ? MMS_OK : MMS_ERR_INVALID_ARG;
}
// mms_embed_simcross_bilinear_forward_f32 / _f16
int embed_bilinear_refusal(int N, int W1, int W2, int D, int M, int K, bool arrays) {
  if (!dims_ok(2, N, W1, W2, D, M) || !table_ok(K, D)) return MMS_ERR_INVALID_ARG;
  return N == 0 || arrays ? MMS_OK : MMS_ERR_INVALID_ARG;
}

// SimMatrix: N pairs of a K1- and a K2-vector
bool simmatrix_dims_ok(int N, int K1, int K2) { return N >= 0 && K1 > 0 && K2 > 0; }
int simmatrix_refusal(int N, int K1, int K2, bool arrays) {
  if (!simmatrix_dims_ok(N, K1, K2)) return MMS_ERR_INVALID_ARG;
  return N == 0 || arrays ? MMS_OK : MMS_ERR_INVALID_ARG;
}
// ... and a backward a gradient array under each propagate-down flag that is set
bool propagate_down_ok(int param, int down0, int down1, const void* dq, const void* da, const void* dW) {
  return (!param || dW) && (!down0 || dq) && (!down1 || da);
}

// The two-valued arithmetic switches: a value that is neither is refused and the switch stays
int set_mode(int mode, int first, int second, void (*set)(int)) {
  if (mode != first && mode != second) return MMS_ERR_INVALID_ARG;
  set(mode);
  return MMS_OK;
}

// The Embed and ranking-metric calls (the _f32 / _f64 twins below).
template <class T>
int rank_map_mrr_abi(int n, int fixed_axis, const T* prob, const T* label, const T* group, T* map_out, T* mrr_out,
                     int* effective_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n <= 0 || fixed_axis < 0 || !fits_int((long long)n * (fixed_axis + 1))) return MMS_ERR_INVALID_ARG;
  if (!prob || !label || !group) return MMS_ERR_INVALID_ARG;
  return rank_map_mrr(n, fixed_axis, prob, label, group, map_out, mrr_out, effective_out,
                      workspace, workspace_bytes, as_stream(stream));
}
template <class T>
int rank_auc_abi(int n, int dim, int fixed_axis, const T* prob, const T* label, int has_ignore_label, int ignore_label,
                 T* auc_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n <= 0 || dim <= 0 || fixed_axis < 0 || fixed_axis >= dim || !fits_int((long long)n * dim))
    return MMS_ERR_INVALID_ARG;
  if (!prob || !label || !auc_out) return MMS_ERR_INVALID_ARG;
  return rank_auc(n, dim, fixed_axis, 1, prob, label, has_ignore_label, ignore_label, auc_out,
                  workspace, workspace_bytes, as_stream(stream));
}
template <class T>
int rank_auc_nd_abi(int outer, int channels, int inner, int fixed_axis, const T* prob, const T* label,
                    int has_ignore_label, int ignore_label, T* auc_out, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (outer <= 0 || channels <= 0 || inner <= 0 || fixed_axis < 0 || fixed_axis >= channels ||
      !fits_int((long long)outer * channels * inner))
    return MMS_ERR_INVALID_ARG;
  if (!prob || !label || !auc_out) return MMS_ERR_INVALID_ARG;
  return rank_auc(outer * inner, channels * inner, fixed_axis, inner, prob, label, has_ignore_label, ignore_label,
                  auc_out, workspace, workspace_bytes, as_stream(stream));
}
template <class T>
int rank_accuracy_abi(int count, const T* a, const T* b, const T* label, T* acc_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (count <= 0) return MMS_ERR_INVALID_ARG;
  if (!a || !b || !label || !acc_out) return MMS_ERR_INVALID_ARG;
  return rank_accuracy(count, a, b, label, acc_out, workspace, workspace_bytes, as_stream(stream));
}
// (S: how table / top / top_diff are stored -- T, or _Float16 for the _f16 calls: one set of checks for every twin)
template <class T, class S>
int embed_forward_abi(int M, int N, int K, const T* index, const S* weight, const T* bias, S* top, void* stream) {
  if (M < 0 || N <= 0 || K <= 0 || !fits_int((long long)M * N)) return MMS_ERR_INVALID_ARG;
  if (M == 0) return MMS_OK;
  if (!index || !weight || !top) return MMS_ERR_INVALID_ARG;
  return embed_forward(M, N, K, index, weight, bias, top, as_stream(stream));
}
template <class T, class S>
int embed_backward_abi(int M, int N, int K, const T* index, const S* top_diff, T* weight_diff, T* bias_diff,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (M < 0 || N <= 0 || K <= 0 || !fits_int((long long)M * N)) return MMS_ERR_INVALID_ARG;
  if (M == 0 || (!weight_diff && !bias_diff)) return MMS_OK;
  if (!index || !top_diff) return MMS_ERR_INVALID_ARG;
  return embed_backward(M, N, K, index, top_diff, weight_diff, bias_diff, workspace, workspace_bytes,
                        as_stream(stream));
}
// indexed: the workspace holds the inverted index the pair forward built for these ids (mms_embed_backward_pair_indexed_*)
template <class S>
int embed_backward_pair_abi(int M0, int M1, int N, int K, const float* index0, const S* top_diff0, const float* index1,
                            const S* top_diff1, float* weight_diff, float* bias_diff, void* workspace,
                            size_t workspace_bytes, void* stream, bool indexed) {
  if (M0 <= 0 || M1 <= 0 || N <= 0 || K <= 0 || !index0 || !top_diff0 || !index1 || !top_diff1) return MMS_ERR_INVALID_ARG;
  if (!fits_int(((long long)M0 + M1) * N)) return MMS_ERR_INVALID_ARG;         // N >= 1: M0 + M1 is an int as well
  if (indexed && !embed_pair_index_supported(M0, M1, K)) return MMS_ERR_UNSUPPORTED;   // no index was built for these sizes
  if (!weight_diff && !bias_diff) return MMS_OK;
  return embed_backward_pair(M0, M1, N, K, index0, top_diff0, index1, top_diff1, weight_diff, bias_diff, workspace,
                             workspace_bytes, as_stream(stream), indexed ? 1 : 0);
}
template <class S>
int embed_forward_pair_abi(int M0, int M1, int N, int K, const float* index0, const float* index1, const S* weight,
                           const float* bias, S* top0, S* top1, void* index_workspace, size_t index_workspace_bytes,
                           void* stream) {
  if (M0 <= 0 || M1 <= 0 || N <= 0 || K <= 0 || !index0 || !index1 || !weight || !top0 || !top1) return MMS_ERR_INVALID_ARG;
  if (!fits_int(((long long)M0 + M1) * N)) return MMS_ERR_INVALID_ARG;
  return embed_forward_pair(M0, M1, N, K, index0, index1, weight, bias, top0, top1, index_workspace,
                            index_workspace_bytes, as_stream(stream));
}
}  // namespace

extern "C" {

int mms_version(void) { return MMS_VERSION; }

const char* mms_error_string(int code) {
  switch (code) {
    case MMS_OK: return "ok";
    case MMS_ERR_INVALID_ARG: return "invalid argument";
    case MMS_ERR_UNSUPPORTED: return "unsupported configuration";
    case MMS_ERR_WORKSPACE: return "workspace missing or too small";
    case MMS_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown error";
  }
}

size_t mms_simcross_workspace_bytes(int dist_mode, int N, int W1, int W2, int D, int M) {
  if (!dims_ok(dist_mode, N, W1, W2, D, M)) return 0;
  if (dist_mode == 2) return bilinear_workspace_bytes(N, W1, W2, D, M);
  return 0;
}

int mms_simcross_forward_f32(int dist_mode, int N, int W1, int W2, int D, int M, const float* q, const float* a,
                             const float* W, const float* bias, float* top, float* norm0, float* norm1,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simcross_refusal(dist_mode, N, W1, W2, D, M, q && a && top, norm0, norm1, W);
  if (rc != MMS_OK || N == 0) return rc;
  if (dist_mode == 2)
    return bilinear_forward(N, W1, W2, D, M, q, a, W, bias, top, workspace, workspace_bytes, as_stream(stream));
  return simcross_elementwise_forward(dist_mode, N, W1, W2, D, q, a, top, norm0, norm1, as_stream(stream));
}

int mms_simcross_backward_f32(int dist_mode, int N, int W1, int W2, int D, int M, const float* q, const float* a,
                              const float* W, int bias_term, const float* top, const float* top_diff,
                              const float* norm0, const float* norm1, int propagate_down0, int propagate_down1,
                              float* dq, float* da, float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const int rc = simcross_backward_refusal(dist_mode, N, W1, W2, D, M, q && a && top && top_diff && dq && da, norm0, norm1,
                                           W, bias_term, dW, dbias);
  if (rc != MMS_OK || N == 0) return rc;
  hipStream_t s = as_stream(stream);
  if (!(propagate_down0 || propagate_down1)) {
    // sim_cross_layer.cpp:176-177 then nothing else (:201)
    if (hipMemsetAsync(dq, 0, sizeof(float) * (size_t)N * W1 * D, s) != hipSuccess ||
        hipMemsetAsync(da, 0, sizeof(float) * (size_t)N * W2 * D, s) != hipSuccess)
      return MMS_ERR_LAUNCH;
    return MMS_OK;
  }
  if (dist_mode == 2)
    return bilinear_backward(N, W1, W2, D, M, q, a, W, bias_term, top_diff, dq, da, dW, dbias, workspace,
                             workspace_bytes, s);
  return simcross_elementwise_backward(dist_mode, N, W1, W2, D, q, a, top, top_diff, norm0, norm1, dq, da, s);
}

int mms_simcross_forward_block_f32(const mms_simcross_args_f32* p, void* stream) {
  if (!p) return MMS_ERR_INVALID_ARG;
  return mms_simcross_forward_f32(p->dist_mode, p->N, p->W1, p->W2, p->D, p->M, p->q, p->a, p->W, p->bias, p->top,
                                  p->norm0, p->norm1, p->workspace, p->workspace_bytes, stream);
}
int mms_simcross_backward_block_f32(const mms_simcross_args_f32* p, void* stream) {
  if (!p) return MMS_ERR_INVALID_ARG;
  return mms_simcross_backward_f32(p->dist_mode, p->N, p->W1, p->W2, p->D, p->M, p->q, p->a, p->W, p->bias_term,
                                   p->top, p->top_diff, p->norm0, p->norm1, p->propagate_down0, p->propagate_down1,
                                   p->dq, p->da, p->dW, p->dbias, p->workspace, p->workspace_bytes, stream);
}

int mms_simcross_forward_backward_f32(int dist_mode, int N, int W1, int W2, int D, int M, const float* q,
                                      const float* a, const float* W, const float* bias, const float* top_diff,
                                      float* top, float* norm0, float* norm1, float* dq, float* da, float* dW,
                                      float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  // (in dist_mode 2 the call is its two halves one after the other: dW and dbias are judged where the second begins)
  int rc = simcross_refusal(dist_mode, N, W1, W2, D, M, q && a && top && top_diff && dq && da, norm0, norm1, W);
  if (rc != MMS_OK || N == 0) return rc;
  if (dist_mode == 2) {
    rc = mms_simcross_forward_f32(2, N, W1, W2, D, M, q, a, W, bias, top, norm0, norm1, workspace, workspace_bytes,
                                  stream);
    if (rc != MMS_OK) return rc;
    return mms_simcross_backward_f32(2, N, W1, W2, D, M, q, a, W, bias != nullptr, top, top_diff, norm0, norm1, 1, 1,
                                     dq, da, dW, dbias, workspace, workspace_bytes, stream);
  }
  return simcross_elementwise_forward_backward(dist_mode, N, W1, W2, D, q, a, top_diff, top, norm0, norm1, dq, da,
                                               as_stream(stream));
}

// fp16-storage sentence-vector pairs (W1 == W2 == 1): the kernels and their routing are simcross_rows_f16.hip's
int mms_simcross_euclid_forward_f16(int N, int D, const void* q_f16, const void* a_f16, float* top, void* stream) {
  const int rc = rows_f16_refusal(N, D, q_f16 && a_f16 && top);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_euclid_rows_f16(N, D, q_f16, a_f16, nullptr, top, nullptr, nullptr, false, as_stream(stream));
}

int mms_simcross_cosine_forward_f16(int N, int D, const void* q_f16, const void* a_f16, float* top, float* norm0,
                                    float* norm1, void* stream) {
  const int rc = rows_f16_refusal(N, D, q_f16 && a_f16 && top);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_cosine_rows_f16(N, D, q_f16, a_f16, nullptr, top, norm0, norm1, nullptr, nullptr, false, as_stream(stream));
}

int mms_simcross_cosine_forward_backward_f16(int N, int D, const void* q_f16, const void* a_f16, const float* top_diff,
                                             float* top, float* norm0, float* norm1, void* dq_f16, void* da_f16,
                                             void* stream) {
  const int rc = rows_f16_refusal(N, D, q_f16 && a_f16 && top_diff && top && dq_f16 && da_f16);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_cosine_rows_f16(N, D, q_f16, a_f16, top_diff, top, norm0, norm1, dq_f16, da_f16, true, as_stream(stream));
}

int mms_simcross_euclid_forward_backward_f16(int N, int D, const void* q_f16, const void* a_f16, const float* top_diff,
                                             float* top, void* dq_f16, void* da_f16, void* stream) {
  const int rc = rows_f16_refusal(N, D, q_f16 && a_f16 && top_diff && top && dq_f16 && da_f16);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_euclid_rows_f16(N, D, q_f16, a_f16, top_diff, top, dq_f16, da_f16, true, as_stream(stream));
}

int mms_simcross_forward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16, const void* a_f16,
                             float* top, float* norm0, float* norm1, void* stream) {
  const int rc = grid_f16_refusal(dist_mode, N, W1, W2, D, q_f16 && a_f16 && top, norm0, norm1);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_grid_forward_f16(dist_mode, N, W1, W2, D, q_f16, a_f16, top, norm0, norm1, as_stream(stream));
}

int mms_simcross_backward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16, const void* a_f16,
                              const float* top, const float* top_diff, const float* norm0, const float* norm1,
                              void* dq_f16, void* da_f16, void* stream) {
  const int rc = grid_f16_refusal(dist_mode, N, W1, W2, D, q_f16 && a_f16 && top && top_diff && dq_f16 && da_f16, norm0,
                                  norm1);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_grid_backward_f16(dist_mode, N, W1, W2, D, q_f16, a_f16, top, top_diff, norm0, norm1, dq_f16, da_f16,
                                    as_stream(stream));
}

int mms_simcross_forward_backward_f16(int dist_mode, int N, int W1, int W2, int D, const void* q_f16,
                                      const void* a_f16, const float* top_diff, float* top, float* norm0,
                                      float* norm1, void* dq_f16, void* da_f16, void* stream) {
  const int rc = grid_f16_refusal(dist_mode, N, W1, W2, D, q_f16 && a_f16 && top_diff && top && dq_f16 && da_f16, norm0,
                                  norm1);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_grid_forward_backward_f16(dist_mode, N, W1, W2, D, q_f16, a_f16, top_diff, top, norm0, norm1, dq_f16,
                                            da_f16, as_stream(stream));
}

size_t mms_simcross_bilinear_workspace_bytes_f16(int N, int W1, int W2, int D, int M) {
  if (bilinear_f16_refusal(N, W1, W2, D, M, true) != MMS_OK) return 0;
  return bilinear_workspace_bytes_f16(N, W1, W2, D, M);
}

int mms_simcross_bilinear_forward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                      const float* W, const float* bias, float* top, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const int rc = bilinear_f16_refusal(N, W1, W2, D, M, q_f16 && a_f16 && W && top);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_bilinear_f16(N, W1, W2, D, M, q_f16, a_f16, W, bias, 0, nullptr, top, nullptr, nullptr, nullptr, nullptr,
                               workspace, workspace_bytes, true, false, as_stream(stream));
}

int mms_simcross_bilinear_backward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                       const float* W, int bias_term, const float* top_diff, void* dq_f16, void* da_f16,
                                       float* dW, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  const bool arrays = q_f16 && a_f16 && W && top_diff && dq_f16 && da_f16 && dW && (!bias_term || dbias);
  const int rc = bilinear_f16_refusal(N, W1, W2, D, M, arrays);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_bilinear_f16(N, W1, W2, D, M, q_f16, a_f16, W, nullptr, bias_term, top_diff, nullptr, dq_f16, da_f16, dW,
                               dbias, workspace, workspace_bytes, false, true, as_stream(stream));
}

int mms_simcross_bilinear_forward_backward_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16,
                                               const float* W, const float* bias, const float* top_diff, float* top,
                                               void* dq_f16, void* da_f16, float* dW, float* dbias, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  const bool arrays = q_f16 && a_f16 && W && top && top_diff && dq_f16 && da_f16 && dW && (!bias || dbias);
  const int rc = bilinear_f16_refusal(N, W1, W2, D, M, arrays);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_bilinear_f16(N, W1, W2, D, M, q_f16, a_f16, W, bias, bias != nullptr, top_diff, top, dq_f16, da_f16, dW,
                               dbias, workspace, workspace_bytes, true, true, as_stream(stream));
}

int mms_embed_simcross_bilinear_forward_f16(int N, int W1, int W2, int D, int M, int K, const float* index_q,
                                            const float* index_a, const void* table_f16, const float* embed_bias,
                                            const float* W, const float* bias, float* top, void* stream) {
  const int rc = embed_bilinear_refusal(N, W1, W2, D, M, K, index_q && index_a && table_f16 && W && top);
  if (rc != MMS_OK || N == 0) return rc;
  return embed_bilinear_forward_f16(N, W1, W2, D, M, K, index_q, index_a, table_f16, embed_bias, W, bias, top,
                                    as_stream(stream));
}

int mms_embed_simcross_forward_f32(int dist_mode, int N, int W1, int W2, int D, int K,
                                   const float* index_q, const float* index_a, const float* weight,
                                   const float* embed_bias, float* top, float* norm0, float* norm1, void* stream) {
  const int rc = embed_simcross_refusal(dist_mode, N, W1, W2, D, K, index_q && index_a && weight && top, norm0, norm1);
  if (rc != MMS_OK || N == 0) return rc;
  return embed_simcross_forward(dist_mode, N, W1, W2, D, K, index_q, index_a, weight, embed_bias, top, norm0,
                                norm1, as_stream(stream));
}

int mms_embed_simcross_forward_f16(int dist_mode, int N, int W1, int W2, int D, int K,
                                   const float* index_q, const float* index_a, const void* table_f16,
                                   const float* embed_bias, float* top, float* norm0, float* norm1, void* stream) {
  const int rc = embed_simcross_refusal(dist_mode, N, W1, W2, D, K, index_q && index_a && table_f16 && top, norm0, norm1);
  if (rc != MMS_OK || N == 0) return rc;
  return embed_simcross_forward_f16(dist_mode, N, W1, W2, D, K, index_q, index_a, table_f16, embed_bias, top, norm0,
                                    norm1, as_stream(stream));
}

int mms_embed_simcross_bilinear_forward_f32(int N, int W1, int W2, int D, int M, int K, const float* index_q,
                                            const float* index_a, const float* weight, const float* embed_bias,
                                            const float* W, const float* bias, float* top, void* stream) {
  const int rc = embed_bilinear_refusal(N, W1, W2, D, M, K, index_q && index_a && weight && W && top);
  if (rc != MMS_OK || N == 0) return rc;
  return embed_bilinear_forward(N, W1, W2, D, M, K, index_q, index_a, weight, embed_bias, W, bias, top,
                                as_stream(stream));
}

size_t mms_simmatrix_workspace_bytes(int N, int K1, int K2) {
  return simmatrix_dims_ok(N, K1, K2) ? simmatrix_workspace_bytes(N, K1, K2) : 0;
}

int mms_simmatrix_forward_f32(int N, int K1, int K2, const float* q, const float* a, const float* W, float* top,
                              float* qw_scratch, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && top && qw_scratch);
  if (rc != MMS_OK || N == 0) return rc;
  return simmatrix_forward(N, K1, K2, q, a, W, top, qw_scratch, as_stream(stream), nullptr);
}

int mms_simmatrix_forward_ws_f32(int N, int K1, int K2, const float* q, const float* a, const float* W, float* top,
                                 float* qw_scratch, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && top && qw_scratch);
  if (rc != MMS_OK || N == 0) return rc;
  if (!workspace || workspace_bytes < simmatrix_workspace_bytes(N, K1, K2)) return MMS_ERR_WORKSPACE;
  return simmatrix_forward(N, K1, K2, q, a, W, top, qw_scratch, as_stream(stream), nullptr, workspace, workspace_bytes);
}

int mms_simmatrix_forward_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16, const float* W, float* top,
                              void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q_f16 && a_f16 && W && top);
  if (rc != MMS_OK || N == 0) return rc;
  return simmatrix_forward_f16(N, K1, K2, q_f16, a_f16, W, top, workspace, workspace_bytes, as_stream(stream));
}

int mms_simmatrix_forward_train_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16, const float* W, float* top,
                                    float* qw_scratch, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q_f16 && a_f16 && W && top && qw_scratch);
  if (rc != MMS_OK || N == 0) return rc;
  return simmatrix_forward_train_f16(N, K1, K2, q_f16, a_f16, W, top, qw_scratch, workspace, workspace_bytes, as_stream(stream));
}

int mms_simmatrix_backward_f16(int N, int K1, int K2, const void* q_f16, const void* a_f16, const float* W,
                               const float* qw, const float* top_diff, void* dq_f16, void* da_f16, float* dW,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q_f16 && a_f16 && W && top_diff);
  if (rc != MMS_OK || N == 0) return rc;
  return simmatrix_backward_f16(N, K1, K2, q_f16, a_f16, W, qw, top_diff, dq_f16, da_f16, dW, workspace,
                                workspace_bytes, as_stream(stream));
}

int mms_set_matrix_mode(int mode) { return set_matrix_mode(mode); }
int mms_get_matrix_mode(void) { return get_matrix_mode(); }

int mms_simmatrix_backward_f32(int N, int K1, int K2, const float* q, const float* a, const float* W,
                               const float* top_diff, int param_propagate_down, int propagate_down0,
                               int propagate_down1, float* dq, float* da, float* dW, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && top_diff);
  if (rc != MMS_OK || N == 0) return rc;
  if (!propagate_down_ok(param_propagate_down, propagate_down0, propagate_down1, dq, da, dW)) return MMS_ERR_INVALID_ARG;
  return simmatrix_backward(N, K1, K2, q, a, W, top_diff, param_propagate_down, propagate_down0, propagate_down1, dq,
                            da, dW, nullptr, workspace, workspace_bytes, as_stream(stream));
}

int mms_simmatrix_backward_cached_f32(int N, int K1, int K2, const float* q, const float* a, const float* W,
                                      const float* qw, const float* top_diff, int param_propagate_down,
                                      int propagate_down0, int propagate_down1, float* dq, float* da, float* dW,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && qw && top_diff);
  if (rc != MMS_OK || N == 0) return rc;
  if (!propagate_down_ok(param_propagate_down, propagate_down0, propagate_down1, dq, da, dW)) return MMS_ERR_INVALID_ARG;
  return simmatrix_backward(N, K1, K2, q, a, W, top_diff, param_propagate_down, propagate_down0, propagate_down1, dq,
                            da, dW, qw, workspace, workspace_bytes, as_stream(stream));
}

size_t mms_pairrank_workspace_bytes(int count) {
  return count > 0 ? pairrank_workspace_bytes(count) : 0;
}

int mms_pairrank_forward_f32(int count, float margin, const float* a, const float* b,
                             const float* y, float* ordered, float* similar, float* loss,
                             void* workspace, size_t workspace_bytes, void* stream) {
  // count == 0 would be 0/0 in the reference (:49); reject instead of writing NaN.
  if (count <= 0) return MMS_ERR_INVALID_ARG;
  if (!a || !b || !y || !ordered || !similar || !loss) return MMS_ERR_INVALID_ARG;
  return pairrank_forward(count, margin, a, b, y, ordered, similar, loss, workspace,
                          workspace_bytes, as_stream(stream));
}

int mms_pairrank_backward_f32(int count, float top_diff, const float* y, const float* ordered,
                              const float* similar, int propagate_down0, int propagate_down1,
                              float* da, float* db, void* stream) {
  if (count <= 0) return MMS_ERR_INVALID_ARG;
  if (!y || !ordered || !similar) return MMS_ERR_INVALID_ARG;
  if ((propagate_down0 && !da) || (propagate_down1 && !db)) return MMS_ERR_INVALID_ARG;
  return pairrank_backward(count, top_diff, y, ordered, similar, propagate_down0 ? da : nullptr,
                           propagate_down1 ? db : nullptr, as_stream(stream));
}

size_t mms_triplet_simmatrix_workspace_bytes(int N, int K1, int K2) {
  if (N <= 0 || K1 <= 0 || K2 <= 0) return 0;
  return triplet_simmatrix_workspace_bytes(N, K1, K2);
}

int mms_triplet_simmatrix_step_f32(int N, int K1, int K2, float margin, float loss_weight, const float* q,
                                   const float* a_pos, const float* a_neg, const float* y, const float* W,
                                   float* s_pos, float* s_neg, float* loss, float* dq, float* da_pos, float* da_neg,
                                   float* dW, void* workspace, size_t workspace_bytes, void* stream) {
  if (N <= 0 || K1 <= 0 || K2 <= 0 || !fits_int((long long)N * K1) || !fits_int((long long)N * K2))
    return MMS_ERR_INVALID_ARG;
  if (!q || !a_pos || !a_neg || !y || !W || !s_pos || !s_neg || !dq || !da_pos || !da_neg || !dW)   // loss may be NULL
    return MMS_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < triplet_simmatrix_workspace_bytes(N, K1, K2)) return MMS_ERR_WORKSPACE;
  return triplet_simmatrix_step(N, K1, K2, margin, loss_weight, q, a_pos, a_neg, y, W, s_pos, s_neg, loss, dq, da_pos,
                                da_neg, dW, workspace, workspace_bytes, as_stream(stream));
}

size_t mms_triplet_workspace_bytes(int N) { return N > 0 ? triplet_workspace_bytes(N) : 0; }

int mms_triplet_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
  return triplet_workspace_init(workspace, workspace_bytes, as_stream(stream));
}

int mms_triplet_euclid_step_f32(int N, int D, float margin, float loss_weight, const float* q,
                                const float* a_pos, const float* a_neg, const float* y,
                                float* s_pos, float* s_neg, float* loss, float* dq, float* da_pos,
                                float* da_neg, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (N <= 0 || D <= 0 || !fits_int((long long)N * D)) return MMS_ERR_INVALID_ARG;
  if (!q || !a_pos || !a_neg || !y || !s_pos || !s_neg || !dq || !da_pos || !da_neg)   // loss may be NULL
    return MMS_ERR_INVALID_ARG;
  return triplet_euclid_step(N, D, margin, loss_weight, q, a_pos, a_neg, y, s_pos, s_neg, loss,
                             dq, da_pos, da_neg, workspace, workspace_bytes, as_stream(stream));
}

int mms_triplet_cosine_step_f32(int N, int D, float margin, float loss_weight, const float* q,
                                const float* a_pos, const float* a_neg, const float* y,
                                float* s_pos, float* s_neg, float* norm_q, float* norm_pos,
                                float* norm_neg, float* loss, float* dq, float* da_pos,
                                float* da_neg, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (N < 0 || D <= 0 || !fits_int((long long)N * D)) return MMS_ERR_INVALID_ARG;
  if (N == 0) return MMS_OK;                                                           // an empty batch: nothing enqueued
  if (!q || !a_pos || !a_neg || !y || !s_pos || !s_neg || !dq || !da_pos || !da_neg)   // loss and the norms may be NULL
    return MMS_ERR_INVALID_ARG;
  return triplet_cosine_step(N, D, margin, loss_weight, q, a_pos, a_neg, y, s_pos, s_neg, norm_q, norm_pos,
                             norm_neg, loss, dq, da_pos, da_neg, workspace, workspace_bytes, as_stream(stream));
}

size_t mms_rank_workspace_bytes(int n) { return n > 0 ? rank_workspace_bytes(n) : 0; }

int mms_rank_map_mrr_f32(int n, int fixed_axis, const float* prob, const float* label,
                         const float* group, float* map_out, float* mrr_out, int* effective_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return rank_map_mrr_abi(n, fixed_axis, prob, label, group, map_out, mrr_out, effective_out, workspace,
                          workspace_bytes, stream);
}

int mms_rank_auc_f32(int n, int dim, int fixed_axis, const float* prob, const float* label,
                     int has_ignore_label, int ignore_label, float* auc_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return rank_auc_abi(n, dim, fixed_axis, prob, label, has_ignore_label, ignore_label, auc_out, workspace,
                      workspace_bytes, stream);
}

int mms_rank_auc_nd_f32(int outer, int channels, int inner, int fixed_axis, const float* prob,
                        const float* label, int has_ignore_label, int ignore_label, float* auc_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return rank_auc_nd_abi(outer, channels, inner, fixed_axis, prob, label, has_ignore_label, ignore_label, auc_out,
                         workspace, workspace_bytes, stream);
}

int mms_rank_accuracy_f32(int count, const float* a, const float* b, const float* label,
                          float* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
  return rank_accuracy_abi(count, a, b, label, acc_out, workspace, workspace_bytes, stream);
}

int mms_embed_backward_pair_f32(int M0, int M1, int N, int K, const float* index0, const float* top_diff0,
                                const float* index1, const float* top_diff1, float* weight_diff, float* bias_diff,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return embed_backward_pair_abi(M0, M1, N, K, index0, top_diff0, index1, top_diff1, weight_diff, bias_diff, workspace,
                                 workspace_bytes, stream, false);
}

int mms_embed_pair_index_supported(int M0, int M1, int K) {
  return M0 > 0 && M1 > 0 && K > 0 && embed_pair_index_supported(M0, M1, K) ? 1 : 0;
}

int mms_embed_forward_pair_f32(int M0, int M1, int N, int K, const float* index0, const float* index1,
                               const float* weight, const float* bias, float* top0, float* top1, void* index_workspace,
                               size_t index_workspace_bytes, void* stream) {
  return embed_forward_pair_abi(M0, M1, N, K, index0, index1, weight, bias, top0, top1, index_workspace,
                                index_workspace_bytes, stream);
}

int mms_embed_backward_pair_indexed_f32(int M0, int M1, int N, int K, const float* index0, const float* top_diff0,
                                        const float* index1, const float* top_diff1, float* weight_diff, float* bias_diff,
                                        void* index_workspace, size_t index_workspace_bytes, void* stream) {
  return embed_backward_pair_abi(M0, M1, N, K, index0, top_diff0, index1, top_diff1, weight_diff, bias_diff,
                                 index_workspace, index_workspace_bytes, stream, true);
}

size_t mms_embed_workspace_bytes(int M, int N) { return (M > 0 && N > 0) ? embed_workspace_bytes(M, N) : 0; }

int mms_embed_forward_f32(int M, int N, int K, const float* index, const float* weight,
                          const float* bias, float* top, void* stream) {
  return embed_forward_abi(M, N, K, index, weight, bias, top, stream);
}

int mms_embed_backward_f32(int M, int N, int K, const float* index, const float* top_diff,
                           float* weight_diff, float* bias_diff, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return embed_backward_abi(M, N, K, index, top_diff, weight_diff, bias_diff, workspace, workspace_bytes, stream);
}

// fp16 storage: half table / top / top_diff, fp32 ids, bias and gradients; the checks and the workspace of the _f32 twins
int mms_embed_forward_f16(int M, int N, int K, const float* index, const void* table_f16, const float* bias,
                          void* top_f16, void* stream) {
  return embed_forward_abi(M, N, K, index, static_cast<const _Float16*>(table_f16), bias, static_cast<_Float16*>(top_f16),
                           stream);
}

int mms_embed_forward_pair_f16(int M0, int M1, int N, int K, const float* index0, const float* index1,
                               const void* table_f16, const float* bias, void* top0_f16, void* top1_f16,
                               void* index_workspace, size_t index_workspace_bytes, void* stream) {
  return embed_forward_pair_abi(M0, M1, N, K, index0, index1, static_cast<const _Float16*>(table_f16), bias,
                                static_cast<_Float16*>(top0_f16), static_cast<_Float16*>(top1_f16), index_workspace,
                                index_workspace_bytes, stream);
}

int mms_embed_backward_f16(int M, int N, int K, const float* index, const void* top_diff_f16, float* weight_diff,
                           float* bias_diff, void* workspace, size_t workspace_bytes, void* stream) {
  return embed_backward_abi(M, N, K, index, static_cast<const _Float16*>(top_diff_f16), weight_diff, bias_diff, workspace,
                            workspace_bytes, stream);
}

int mms_embed_backward_pair_f16(int M0, int M1, int N, int K, const float* index0, const void* top_diff0_f16,
                                const float* index1, const void* top_diff1_f16, float* weight_diff, float* bias_diff,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return embed_backward_pair_abi(M0, M1, N, K, index0, static_cast<const _Float16*>(top_diff0_f16), index1,
                                 static_cast<const _Float16*>(top_diff1_f16), weight_diff, bias_diff, workspace,
                                 workspace_bytes, stream, false);
}

int mms_embed_backward_pair_indexed_f16(int M0, int M1, int N, int K, const float* index0, const void* top_diff0_f16,
                                        const float* index1, const void* top_diff1_f16, float* weight_diff,
                                        float* bias_diff, void* index_workspace, size_t index_workspace_bytes,
                                        void* stream) {
  return embed_backward_pair_abi(M0, M1, N, K, index0, static_cast<const _Float16*>(top_diff0_f16), index1,
                                 static_cast<const _Float16*>(top_diff1_f16), weight_diff, bias_diff, index_workspace,
                                 index_workspace_bytes, stream, true);
}

int mms_feed_gather_rows_f32(int rows, int row_elems, int src_rows, const float* src, const int* perm,
                             int first, float* dst, void* stream) {
  if (rows < 0 || row_elems <= 0 || src_rows <= 0 || first < 0) return MMS_ERR_INVALID_ARG;
  if (!fits_int((long long)rows * row_elems) || (long long)first + rows > src_rows) return MMS_ERR_INVALID_ARG;
  if (rows == 0) return MMS_OK;
  if (!src || !dst) return MMS_ERR_INVALID_ARG;
  return feed_gather_rows(rows, row_elems, src_rows, src, perm, first, dst, as_stream(stream));
}

int mms_set_euclid_backward_mode(int mode) {
  return set_mode(mode, MMS_EUCLID_BWD_FP32, MMS_EUCLID_BWD_REFERENCE, set_euclid_backward_mode);
}
int mms_get_euclid_backward_mode(void) { return euclid_backward_mode(); }

int mms_null_launch(int workgroups, void* stream) {
  if (workgroups <= 0) return MMS_ERR_INVALID_ARG;
  return null_launch(workgroups, as_stream(stream));
}
int mms_dot_f32(int n, const float* x, const float* y, float* out, void* stream) {
  if (n < 0 || !out || (n > 0 && (!x || !y))) return MMS_ERR_INVALID_ARG;
  return dot(n, x, y, out, as_stream(stream));
}
int mms_split_backward_f32(int count, int ntop, const float* const* top_diffs, float* bottom_diff, void* stream) {
  if (count < 0 || ntop < 1 || !top_diffs || (count > 0 && !bottom_diff)) return MMS_ERR_INVALID_ARG;
  for (int i = 0; i < ntop; ++i) if (count > 0 && !top_diffs[i]) return MMS_ERR_INVALID_ARG;
  if (count == 0) return MMS_OK;
  return split_sum(count, ntop, top_diffs, bottom_diff, as_stream(stream));
}
int mms_dot_f64(int n, const double* x, const double* y, double* out, void* stream) {
  if (n < 0 || !out || (n > 0 && (!x || !y))) return MMS_ERR_INVALID_ARG;
  return dot(n, x, y, out, as_stream(stream));
}

int mms_set_pairrank_hinge_mode(int mode) {
  return set_mode(mode, MMS_PAIRRANK_HINGE_CPU, MMS_PAIRRANK_HINGE_GPU, set_pairrank_hinge_mode);
}
int mms_get_pairrank_hinge_mode(void) { return pairrank_hinge_mode(); }
int mms_set_triplet_finish_mode(int mode) {
  return set_mode(mode, MMS_TRIPLET_FINISH_LAUNCH, MMS_TRIPLET_FINISH_INLAUNCH, set_triplet_finish_mode);
}
int mms_get_triplet_finish_mode(void) { return triplet_finish_mode(); }

int mms_set_loss_sum_mode(int mode) {
  return set_mode(mode, MMS_LOSS_SUM_FAST, MMS_LOSS_SUM_REFERENCE, set_loss_sum_mode);
}
int mms_get_loss_sum_mode(void) { return loss_sum_mode(); }

int mms_set_rank_tie_mode(int mode) {
  return set_mode(mode, MMS_RANK_TIES_INPUT_ORDER, MMS_RANK_TIES_LIBSTDCXX, set_rank_tie_mode);
}
int mms_get_rank_tie_mode(void) { return rank_tie_mode(); }
int mms_set_f16_distance_mode(int mode) {
  return set_mode(mode, MMS_F16_DISTANCE_ORDERED, MMS_F16_DISTANCE_TREE, set_f16_distance_mode);
}
int mms_get_f16_distance_mode(void) { return f16_distance_mode(); }

// ---- double instantiation (csrc/f64_paths.hip): same contracts as the _f32 entry points ----
size_t mms_simcross_workspace_bytes_f64(int dist_mode, int N, int W1, int W2, int D, int M) {
  if (!dims_ok(dist_mode, N, W1, W2, D, M)) return 0;
  return simcross_workspace_bytes_f64(dist_mode, N, W1, W2, D, M);
}

int mms_simcross_forward_f64(int dist_mode, int N, int W1, int W2, int D, int M, const double* q, const double* a,
                             const double* W, const double* bias, double* top, double* norm0, double* norm1,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = simcross_refusal(dist_mode, N, W1, W2, D, M, q && a && top, norm0, norm1, W);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_forward_f64(dist_mode, N, W1, W2, D, M, q, a, W, bias, top, norm0, norm1, workspace, workspace_bytes,
                              as_stream(stream));
}

int mms_simcross_backward_f64(int dist_mode, int N, int W1, int W2, int D, int M, const double* q, const double* a,
                              const double* W, int bias_term, const double* top, const double* top_diff,
                              const double* norm0, const double* norm1, int propagate_down0, int propagate_down1,
                              double* dq, double* da, double* dW, double* dbias, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int rc = simcross_backward_refusal(dist_mode, N, W1, W2, D, M, q && a && top && top_diff && dq && da, norm0, norm1,
                                           W, bias_term, dW, dbias);
  if (rc != MMS_OK || N == 0) return rc;
  return simcross_backward_f64(dist_mode, N, W1, W2, D, M, q, a, W, bias_term, top, top_diff, norm0, norm1,
                               propagate_down0, propagate_down1, dq, da, dW, dbias, workspace, workspace_bytes,
                               as_stream(stream));
}

int mms_simmatrix_forward_f64(int N, int K1, int K2, const double* q, const double* a, const double* W, double* top,
                              double* qw_scratch, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && top && qw_scratch);
  if (rc != MMS_OK || N == 0) return rc;
  return simmatrix_forward_f64(N, K1, K2, q, a, W, top, qw_scratch, as_stream(stream));
}

int mms_simmatrix_backward_f64(int N, int K1, int K2, const double* q, const double* a, const double* W,
                               const double* top_diff, int param_propagate_down, int propagate_down0,
                               int propagate_down1, double* dq, double* da, double* dW, void* stream) {
  const int rc = simmatrix_refusal(N, K1, K2, q && a && W && top_diff);
  if (rc != MMS_OK || N == 0) return rc;
  if (!propagate_down_ok(param_propagate_down, propagate_down0, propagate_down1, dq, da, dW)) return MMS_ERR_INVALID_ARG;
  return simmatrix_backward_f64(N, K1, K2, q, a, W, top_diff, param_propagate_down, propagate_down0, propagate_down1,
                                dq, da, dW, as_stream(stream));
}

int mms_pairrank_forward_f64(int count, double margin, const double* a, const double* b,
                             const double* y, double* ordered, double* similar, double* loss,
                             void* stream) {
  if (count <= 0) return MMS_ERR_INVALID_ARG;
  if (!a || !b || !y || !ordered || !similar || !loss) return MMS_ERR_INVALID_ARG;
  return pairrank_forward_f64(count, margin, a, b, y, ordered, similar, loss, as_stream(stream));
}

int mms_pairrank_backward_f64(int count, double top_diff, const double* y, const double* ordered,
                              const double* similar, int propagate_down0, int propagate_down1,
                              double* da, double* db, void* stream) {
  if (count <= 0) return MMS_ERR_INVALID_ARG;
  if (!y || !ordered || !similar) return MMS_ERR_INVALID_ARG;
  if ((propagate_down0 && !da) || (propagate_down1 && !db)) return MMS_ERR_INVALID_ARG;
  return pairrank_backward_f64(count, top_diff, y, ordered, similar, propagate_down0 ? da : nullptr,
                               propagate_down1 ? db : nullptr, as_stream(stream));
}

size_t mms_rank_workspace_bytes_f64(int n) { return n > 0 ? rank_workspace_bytes_f64(n) : 0; }
int mms_rank_map_mrr_f64(int n, int fixed_axis, const double* prob, const double* label,
                         const double* group, double* map_out, double* mrr_out, int* effective_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  return rank_map_mrr_abi(n, fixed_axis, prob, label, group, map_out, mrr_out, effective_out, workspace,
                          workspace_bytes, stream);
}

int mms_rank_auc_f64(int n, int dim, int fixed_axis, const double* prob, const double* label,
                     int has_ignore_label, int ignore_label, double* auc_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return rank_auc_abi(n, dim, fixed_axis, prob, label, has_ignore_label, ignore_label, auc_out, workspace,
                      workspace_bytes, stream);
}

int mms_rank_auc_nd_f64(int outer, int channels, int inner, int fixed_axis, const double* prob,
                        const double* label, int has_ignore_label, int ignore_label, double* auc_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  return rank_auc_nd_abi(outer, channels, inner, fixed_axis, prob, label, has_ignore_label, ignore_label, auc_out,
                         workspace, workspace_bytes, stream);
}

int mms_rank_accuracy_f64(int count, const double* a, const double* b, const double* label,
                          double* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
  return rank_accuracy_abi(count, a, b, label, acc_out, workspace, workspace_bytes, stream);
}

size_t mms_embed_workspace_bytes_f64(int M, int N) { return (M > 0 && N > 0) ? embed_workspace_bytes_f64(M, N) : 0; }
int mms_embed_forward_f64(int M, int N, int K, const double* index, const double* weight,
                          const double* bias, double* top, void* stream) {
  return embed_forward_abi(M, N, K, index, weight, bias, top, stream);
}

int mms_embed_backward_f64(int M, int N, int K, const double* index, const double* top_diff,
                           double* weight_diff, double* bias_diff, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return embed_backward_abi(M, N, K, index, top_diff, weight_diff, bias_diff, workspace, workspace_bytes, stream);
}

}  // extern "C"
