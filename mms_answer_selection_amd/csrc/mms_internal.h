// csrc/mms_internal.h -- the one declaration of every mms:: function that one .hip source defines and another calls.
// Every .hip source includes it, the defining one too, and default arguments live here only.
#ifndef MMS_INTERNAL_H_
#define MMS_INTERNAL_H_

#include "host_args.h"
#include "mms_common.h"

namespace mms {
// simcross_rows.hip (W1 == W2 == 1, Euclid)
// false: no rows kernel serves this Euclid forward or fused launch, and the word-grid kernels take it.  `exact`:
// euclid_backward_mode() == MMS_EUCLID_BWD_REFERENCE, read once by the entry point.  Instantiated for
// <true, false>, <false, true> and <true, true>.
template <bool FWD, bool BWD>
bool launch_euclid_rows(int N, int D, const float* q, const float* a, const float* top_in, const float* top_diff,
                        float* top_out, float* dq, float* da, bool exact, hipStream_t s);
int euclid_backward_mode();
void set_euclid_backward_mode(int m);
// simcross_rows_cosine.hip (W1 == W2 == 1, cosine; the same three instantiations)
template <bool FWD, bool BWD>
void launch_cosine_rows(int N, int D, const float* q, const float* a, const float* top_diff, float* top, float* norm0,
                        float* norm1, float* dq, float* da, hipStream_t s);
// simcross_rows_f16.hip (W1 == W2 == 1, fp16 storage)
int simcross_euclid_rows_f16(int N, int D, const void* q, const void* a, const float* top_diff, float* top, void* dq,
                             void* da, bool bwd, hipStream_t s);
int simcross_cosine_rows_f16(int N, int D, const void* q, const void* a, const float* top_diff, float* top, float* norm0,
                             float* norm1, void* dq, void* da, bool bwd, hipStream_t s);
int f16_distance_mode();
void set_f16_distance_mode(int m);
// simcross_cross.hip
int simcross_elementwise_forward(int mode, int N, int W1, int W2, int D, const float* q, const float* a, float* top,
                                 float* norm0, float* norm1, hipStream_t s);
int simcross_elementwise_backward(int mode, int N, int W1, int W2, int D, const float* q, const float* a, const float* top,
                                  const float* top_diff, const float* norm0, const float* norm1, float* dq, float* da,
                                  hipStream_t s);
int simcross_elementwise_forward_backward(int mode, int N, int W1, int W2, int D, const float* q, const float* a,
                                          const float* top_diff, float* top, float* norm0, float* norm1, float* dq,
                                          float* da, hipStream_t s);
int embed_simcross_forward(int mode, int N, int W1, int W2, int D, int K, const float* index_q, const float* index_a,
                           const float* weight, const float* embed_bias, float* top, float* norm0, float* norm1,
                           hipStream_t s);
// simcross_cross_f16.hip (fp16 storage, word grids, dist_mode 0 / 1; the caller has checked the arguments)
int simcross_grid_forward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, float* top,
                              float* norm0, float* norm1, hipStream_t s);
int simcross_grid_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a, const float* top,
                               const float* top_diff, const float* norm0, const float* norm1, void* dq, void* da,
                               hipStream_t s);
int simcross_grid_forward_backward_f16(int mode, int N, int W1, int W2, int D, const void* q, const void* a,
                                       const float* top_diff, float* top, float* norm0, float* norm1, void* dq,
                                       void* da, hipStream_t s);
int embed_simcross_forward_f16(int mode, int N, int W1, int W2, int D, int K, const float* index_q, const float* index_a,
                               const void* table_f16, const float* embed_bias, float* top, float* norm0, float* norm1,
                               hipStream_t s);
// bilinear.hip (SimCross dist_mode 2)
size_t bilinear_workspace_bytes(int N, int W1, int W2, int D, int M);
int bilinear_forward(int N, int W1, int W2, int D, int M, const float* q, const float* a, const float* W,
                     const float* bias, float* top, void* ws, size_t ws_bytes, hipStream_t s);
int bilinear_backward(int N, int W1, int W2, int D, int M, const float* q, const float* a, const float* W, int bias_term,
                      const float* top_diff, float* dq, float* da, float* dW, float* dbias, void* ws, size_t ws_bytes,
                      hipStream_t s);
int embed_bilinear_forward(int N, int W1, int W2, int D, int M, int K, const float* index_q, const float* index_a,
                           const float* table, const float* embed_bias, const float* W, const float* bias, float* top,
                           hipStream_t s);
// bilinear_f16.hip (fp16 storage, word grids, dist_mode 2; the caller has checked the arguments)
size_t bilinear_workspace_bytes_f16(int N, int W1, int W2, int D, int M);
int simcross_bilinear_f16(int N, int W1, int W2, int D, int M, const void* q_f16, const void* a_f16, const float* W,
                          const float* bias, int bias_term, const float* top_diff, float* top, void* dq_f16, void* da_f16,
                          float* dW, float* dbias, void* ws, size_t ws_bytes, bool fwd, bool bwd, hipStream_t s);
int embed_bilinear_forward_f16(int N, int W1, int W2, int D, int M, int K, const float* index_q, const float* index_a,
                               const void* table_f16, const float* embed_bias, const float* W, const float* bias,
                               float* top, hipStream_t s);
// simmatrix.hip
int set_matrix_mode(int mode);
int get_matrix_mode();
size_t simmatrix_workspace_bytes(int N, int K1, int K2);
int simmatrix_forward(int N, int K1, int K2, const float* q, const float* a, const float* W, float* top, float* qw,
                      hipStream_t s, const float* rd_bias, void* ws = nullptr, size_t ws_bytes = 0);
int simmatrix_backward(int N, int K1, int K2, const float* q, const float* a, const float* W, const float* top_diff,
                       int ppd, int pd0, int pd1, float* dq, float* da, float* dW, const float* qw, void* ws,
                       size_t ws_bytes, hipStream_t s);
int simmatrix_forward_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, float* top, void* ws,
                          size_t ws_bytes, hipStream_t s);
int simmatrix_forward_train_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, float* top,
                                float* qw, void* ws, size_t ws_bytes, hipStream_t s);
int simmatrix_backward_f16(int N, int K1, int K2, const void* q, const void* a, const float* W, const float* qw,
                           const float* top_diff, void* dq, void* da, float* dW, void* ws, size_t ws_bytes, hipStream_t s);
size_t triplet_simmatrix_workspace_bytes(int N, int K1, int K2);
int triplet_simmatrix_step(int N, int K1, int K2, float margin, float loss_weight, const float* q, const float* ap,
                           const float* an, const float* y, const float* W, float* s_pos, float* s_neg, float* loss,
                           float* dq, float* dap, float* dan, float* dW, void* ws, size_t ws_bytes, hipStream_t s);
// pairrank.hip
size_t pairrank_workspace_bytes(int count);
int pairrank_forward(int count, float margin, const float* a, const float* b, const float* y, float* ordered,
                     float* similar, float* loss, void* ws, size_t ws_bytes, hipStream_t s);
int pairrank_backward(int count, float top_diff, const float* y, const float* ordered, const float* similar, float* da,
                      float* db, hipStream_t s);
int triplet_loss_from_terms(const float* terms, int N, float* loss, hipStream_t s);
int pairrank_hinge_mode();
void set_pairrank_hinge_mode(int m);
int loss_sum_mode();
void set_loss_sum_mode(int m);
// triplet_steps.hip
size_t triplet_workspace_bytes(int N);
int triplet_workspace_init(void* ws, size_t ws_bytes, hipStream_t s);
int triplet_euclid_step(int N, int D, float margin, float loss_weight, const float* q, const float* ap, const float* an,
                        const float* y, float* s_pos, float* s_neg, float* loss, float* dq, float* dap, float* dan,
                        void* ws, size_t ws_bytes, hipStream_t s);
int triplet_cosine_step(int N, int D, float margin, float loss_weight, const float* q, const float* ap, const float* an,
                        const float* y, float* s_pos, float* s_neg, float* norm_q, float* norm_pos, float* norm_neg,
                        float* loss, float* dq, float* dap, float* dan, void* ws, size_t ws_bytes, hipStream_t s);
int triplet_finish_mode();
void set_triplet_finish_mode(int m);
// ranking.hip (host entry points, radix path; device pieces shared with rank_onewg.hip: rank_common.h)
// (T = float or double: the folds run in T, the order is that of the scores narrowed to float for both)
size_t rank_workspace_bytes(int n);
size_t rank_workspace_bytes_f64(int n);
template <class T>
int rank_map_mrr(int n, int fixed_axis, const T* prob, const T* label, const T* group, T* map_out, T* mrr_out,
                 int* effective, void* ws, size_t ws_bytes, hipStream_t s);
template <class T>
int rank_auc(int n, int dim, int fixed_axis, int inner, const T* prob, const T* label, int has_ignore, int ignore_label,
             T* auc_out, void* ws, size_t ws_bytes, hipStream_t s);
template <class T>
int rank_accuracy(int count, const T* a, const T* b, const T* label, T* out, void* ws, size_t ws_bytes, hipStream_t s);
int rank_tie_mode();
void set_rank_tie_mode(int m);
// rank_onewg.hip: the whole metric in one workgroup and one launch, for the sizes it is the fastest at
enum class RankRoute { kOneWgSmall, kOneWgMid, kRadix };
RankRoute rank_route(int n, bool libstd);              // libstd: MMS_RANK_TIES_LIBSTDCXX (the radix path emulates it)
// route: one of the two kOneWg; auc: AUC into out0 (group, out1 and effective unused), otherwise MAP / MRR / effective
template <class T>
int rank_onewg(RankRoute route, bool auc, int n, int stride, int offset, int inner, const T* prob, const T* label,
               const T* group, int has_ignore, int ignore_label, T* out0, T* out1, int* effective, hipStream_t s);
// embed.hip
size_t embed_workspace_bytes(int M, int N);
size_t embed_workspace_bytes_f64(int M, int N);
// (T: ids, bias, gradients and all arithmetic; S: how table / top / top_diff are stored -- T itself, or _Float16 with
// T = float, whose workspace is embed_workspace_bytes too.  Instantiated: <float, float>, <double, double>,
// <float, _Float16>; the pair calls for S = float and _Float16.)
template <class T, class S>
int embed_forward(int M, int N, int K, const T* index, const S* weight, const T* bias, S* top, hipStream_t s);
template <class T, class S>
int embed_backward(int M, int N, int K, const T* index, const S* top_diff, T* weight_diff, T* bias_diff, void* ws,
                   size_t ws_bytes, hipStream_t s);
template <class S>
int embed_backward_pair(int M0, int M1, int N, int K, const float* index0, const S* top_diff0, const float* index1,
                        const S* top_diff1, float* weight_diff, float* bias_diff, void* ws, size_t ws_bytes,
                        hipStream_t s, int index_ready);
bool embed_pair_index_supported(int M0, int M1, int K);
template <class S>
int embed_forward_pair(int M0, int M1, int N, int K, const float* index0, const float* index1, const S* weight,
                       const float* bias, S* top0, S* top1, void* index_ws, size_t index_ws_bytes, hipStream_t s);
int feed_gather_rows(int rows, int row_elems, int src_rows, const float* src, const int* perm, int first, float* dst,
                     hipStream_t s);
// net_glue.hip
int null_launch(int workgroups, hipStream_t s);
template <class T>
int dot(int n, const T* x, const T* y, T* out, hipStream_t s);
int split_sum(int count, int ntop, const float* const* top_diffs, float* bottom_diff, hipStream_t s);
// head.hip: what the fused tails (score_tail.hip, train_tail.hip) end a loss with, from each sample's term and whether
// it counts: one launch of one thread, the terms added in ascending n.  d: the head's dims (csrc/head_tile.h)
struct HeadDims;
int head_loss_from_terms(const float* terms, const int* valid, const HeadDims& d, float* loss, hipStream_t s);
// f64_paths.hip
size_t simcross_workspace_bytes_f64(int mode, int N, int W1, int W2, int D, int M);
int simcross_forward_f64(int mode, int N, int W1, int W2, int D, int M, const double* q, const double* a, const double* W,
                         const double* bias, double* top, double* norm0, double* norm1, void* ws, size_t ws_bytes,
                         hipStream_t s);
int simcross_backward_f64(int mode, int N, int W1, int W2, int D, int M, const double* q, const double* a, const double* W,
                          int bias_term, const double* top, const double* top_diff, const double* norm0,
                          const double* norm1, int pd0, int pd1, double* dq, double* da, double* dW, double* dbias,
                          void* ws, size_t ws_bytes, hipStream_t s);
int simmatrix_forward_f64(int N, int K1, int K2, const double* q, const double* a, const double* W, double* top,
                          double* scratch, hipStream_t s);
int simmatrix_backward_f64(int N, int K1, int K2, const double* q, const double* a, const double* W,
                           const double* top_diff, int ppd, int pd0, int pd1, double* dq, double* da, double* dW,
                           hipStream_t s);
int pairrank_forward_f64(int count, double margin, const double* a, const double* b, const double* y, double* ordered,
                         double* similar, double* loss, hipStream_t s);
int pairrank_backward_f64(int count, double top_diff, const double* y, const double* ordered, const double* similar,
                          double* da, double* db, hipStream_t s);
}  // namespace mms
#endif  // MMS_INTERNAL_H_
