// csrc/layer_abi.hpp -- what the sources of libmms_caffe.so share on their way into the C ABI of include/mms.h
// (internal: included by the layer sources only, never by a host that compiles against caffe_api.hpp):
//   mms_check      a C-ABI return code as a CHECK
//   abi::          the C ABI by element type, so that one layer template serves Layer<float> and Layer<double>
//   Workspace      the device scratch a C-ABI call is handed, sized in bytes, held as a Blob
//   NO_CPU_MODE    the body of every Forward_cpu / Backward_cpu: this library is the GPU implementation, and a
//                  silent host fallback would void every parity claim
#ifndef MMS_LAYER_ABI_HPP_
#define MMS_LAYER_ABI_HPP_

#include "caffe_api.hpp"
#include "mms.h"

namespace caffe {

inline void mms_check(int rc, const char* what) {
  CHECK_EQ(rc, (int)MMS_OK) << what << ": " << mms_error_string(rc);
}

// `bytes` of device scratch as a Blob<Dtype> of ceil(bytes / sizeof(Dtype)) elements (a Blob never shrinks its
// allocation, so a layer reshaped to and fro does not reallocate).
template <typename Dtype>
class Workspace {
 public:
  // keep_if_zero: a request for no bytes leaves the blob as it is (SimCross, PairRankLoss) instead of emptying it
  void reserve(size_t bytes, bool keep_if_zero = false) {
    if (bytes == 0 && keep_if_zero) return;
    blob_.Reshape(vector<int>{(int)((bytes + sizeof(Dtype) - 1) / sizeof(Dtype))});
  }
  Dtype* data() { return blob_.count() ? blob_.mutable_gpu_data() : nullptr; }
  size_t bytes() const { return (size_t)blob_.count() * sizeof(Dtype); }
 private:
  Blob<Dtype> blob_;
};

// The C ABI by element type: what lets one layer template serve Layer<float> and Layer<double>.
namespace abi {
inline size_t simcross_ws(float, int mode, int N, int W1, int W2, int D, int M) { return mms_simcross_workspace_bytes(mode, N, W1, W2, D, M); }
inline size_t simcross_ws(double, int mode, int N, int W1, int W2, int D, int M) { return mms_simcross_workspace_bytes_f64(mode, N, W1, W2, D, M); }
inline int simcross_forward(int mode, int N, int W1, int W2, int D, int M, const float* q, const float* a, const float* W,
                            const float* bias, float* top, float* n0, float* n1, void* ws, size_t wsb) {
  return mms_simcross_forward_f32(mode, N, W1, W2, D, M, q, a, W, bias, top, n0, n1, ws, wsb, nullptr);
}
inline int simcross_forward(int mode, int N, int W1, int W2, int D, int M, const double* q, const double* a, const double* W,
                            const double* bias, double* top, double* n0, double* n1, void* ws, size_t wsb) {
  return mms_simcross_forward_f64(mode, N, W1, W2, D, M, q, a, W, bias, top, n0, n1, ws, wsb, nullptr);
}
inline int simcross_backward(int mode, int N, int W1, int W2, int D, int M, const float* q, const float* a, const float* W,
                             int bias_term, const float* top, const float* dT, const float* n0, const float* n1, int pd0,
                             int pd1, float* dq, float* da, float* dW, float* db, void* ws, size_t wsb) {
  return mms_simcross_backward_f32(mode, N, W1, W2, D, M, q, a, W, bias_term, top, dT, n0, n1, pd0, pd1, dq, da, dW, db, ws,
                                   wsb, nullptr);
}
inline int simcross_backward(int mode, int N, int W1, int W2, int D, int M, const double* q, const double* a, const double* W,
                             int bias_term, const double* top, const double* dT, const double* n0, const double* n1, int pd0,
                             int pd1, double* dq, double* da, double* dW, double* db, void* ws, size_t wsb) {
  return mms_simcross_backward_f64(mode, N, W1, W2, D, M, q, a, W, bias_term, top, dT, n0, n1, pd0, pd1, dq, da, dW, db, ws,
                                   wsb, nullptr);
}
inline size_t simmatrix_ws(float, int N, int K1, int K2) { return mms_simmatrix_workspace_bytes(N, K1, K2); }
inline size_t simmatrix_ws(double, int, int, int) { return 0; }
inline int simmatrix_forward(int N, int K1, int K2, const float* q, const float* a, const float* W, float* top, float* scr,
                             void* ws, size_t wsb) {
  if (ws) return mms_simmatrix_forward_ws_f32(N, K1, K2, q, a, W, top, scr, ws, wsb, nullptr);   // the layer's own workspace
  return mms_simmatrix_forward_f32(N, K1, K2, q, a, W, top, scr, nullptr);
}
inline int simmatrix_forward(int N, int K1, int K2, const double* q, const double* a, const double* W, double* top, double* scr,
                             void*, size_t) {
  return mms_simmatrix_forward_f64(N, K1, K2, q, a, W, top, scr, nullptr);
}
inline int simmatrix_backward_cached(int N, int K1, int K2, const float* q, const float* a, const float* W, const float* qw,
                                     const float* dT, int ppd, int pd0, int pd1, float* dq, float* da, float* dW, void* ws, size_t wsb) {
  return mms_simmatrix_backward_cached_f32(N, K1, K2, q, a, W, qw, dT, ppd, pd0, pd1, dq, da, dW, ws, wsb, nullptr);
}
inline int simmatrix_backward_cached(int N, int K1, int K2, const double* q, const double* a, const double* W, const double*,
                                     const double* dT, int ppd, int pd0, int pd1, double* dq, double* da, double* dW, void*, size_t) {
  return mms_simmatrix_backward_f64(N, K1, K2, q, a, W, dT, ppd, pd0, pd1, dq, da, dW, nullptr);   // functional path: recomputes
}
inline int simmatrix_backward(int N, int K1, int K2, const float* q, const float* a, const float* W, const float* dT, int ppd,
                              int pd0, int pd1, float* dq, float* da, float* dW, void* ws, size_t wsb) {
  return mms_simmatrix_backward_f32(N, K1, K2, q, a, W, dT, ppd, pd0, pd1, dq, da, dW, ws, wsb, nullptr);
}
inline int simmatrix_backward(int N, int K1, int K2, const double* q, const double* a, const double* W, const double* dT,
                              int ppd, int pd0, int pd1, double* dq, double* da, double* dW, void*, size_t) {
  return mms_simmatrix_backward_f64(N, K1, K2, q, a, W, dT, ppd, pd0, pd1, dq, da, dW, nullptr);
}
inline size_t pairrank_ws(float, int count) { return mms_pairrank_workspace_bytes(count); }
inline size_t pairrank_ws(double, int) { return 0; }
inline int pairrank_forward(int count, float margin, const float* a, const float* b, const float* y, float* o, float* s,
                            float* loss, void* ws, size_t wsb) {
  return mms_pairrank_forward_f32(count, margin, a, b, y, o, s, loss, ws, wsb, nullptr);
}
inline int pairrank_forward(int count, double margin, const double* a, const double* b, const double* y, double* o, double* s,
                            double* loss, void*, size_t) {
  return mms_pairrank_forward_f64(count, margin, a, b, y, o, s, loss, nullptr);
}
inline int pairrank_backward(int count, float td, const float* y, const float* o, const float* s, int pd0, int pd1, float* da,
                             float* db) {
  return mms_pairrank_backward_f32(count, td, y, o, s, pd0, pd1, da, db, nullptr);
}
inline int pairrank_backward(int count, double td, const double* y, const double* o, const double* s, int pd0, int pd1,
                             double* da, double* db) {
  return mms_pairrank_backward_f64(count, td, y, o, s, pd0, pd1, da, db, nullptr);
}
inline size_t embed_ws(float, int M, int N) { return mms_embed_workspace_bytes(M, N); }
inline size_t embed_ws(double, int M, int N) { return mms_embed_workspace_bytes_f64(M, N); }
inline int embed_forward(int M, int N, int K, const float* index, const float* weight, const float* bias, float* top) {
  return mms_embed_forward_f32(M, N, K, index, weight, bias, top, nullptr);
}
inline int embed_forward(int M, int N, int K, const double* index, const double* weight, const double* bias, double* top) {
  return mms_embed_forward_f64(M, N, K, index, weight, bias, top, nullptr);
}
inline int embed_backward(int M, int N, int K, const float* index, const float* dT, float* dW, float* db, void* ws, size_t wsb) {
  return mms_embed_backward_f32(M, N, K, index, dT, dW, db, ws, wsb, nullptr);
}
inline int embed_backward(int M, int N, int K, const double* index, const double* dT, double* dW, double* db, void* ws,
                          size_t wsb) {
  return mms_embed_backward_f64(M, N, K, index, dT, dW, db, ws, wsb, nullptr);
}
inline size_t rank_ws(float, int n) { return mms_rank_workspace_bytes(n); }
inline size_t rank_ws(double, int n) { return mms_rank_workspace_bytes_f64(n); }
inline int rank_map_mrr(int n, int fixed_axis, const float* prob, const float* label, const float* group, float* map,
                        float* mrr, void* ws, size_t wsb) {
  return mms_rank_map_mrr_f32(n, fixed_axis, prob, label, group, map, mrr, nullptr, ws, wsb, nullptr);
}
inline int rank_map_mrr(int n, int fixed_axis, const double* prob, const double* label, const double* group, double* map,
                        double* mrr, void* ws, size_t wsb) {
  return mms_rank_map_mrr_f64(n, fixed_axis, prob, label, group, map, mrr, nullptr, ws, wsb, nullptr);
}
inline int rank_auc_nd(int outer, int channels, int inner, int fixed_axis, const float* prob, const float* label,
                       int has_ignore, int ignore_label, float* auc, void* ws, size_t wsb) {
  return mms_rank_auc_nd_f32(outer, channels, inner, fixed_axis, prob, label, has_ignore, ignore_label, auc, ws, wsb, nullptr);
}
inline int rank_auc_nd(int outer, int channels, int inner, int fixed_axis, const double* prob, const double* label,
                       int has_ignore, int ignore_label, double* auc, void* ws, size_t wsb) {
  return mms_rank_auc_nd_f64(outer, channels, inner, fixed_axis, prob, label, has_ignore, ignore_label, auc, ws, wsb, nullptr);
}
inline int rank_accuracy(int count, const float* a, const float* b, const float* label, float* acc, void* ws, size_t wsb) {
  return mms_rank_accuracy_f32(count, a, b, label, acc, ws, wsb, nullptr);
}
inline int rank_accuracy(int count, const double* a, const double* b, const double* label, double* acc, void* ws, size_t wsb) {
  return mms_rank_accuracy_f64(count, a, b, label, acc, ws, wsb, nullptr);
}
}  // namespace abi

}  // namespace caffe

#define NO_CPU_MODE MMS_FATAL("") << this->type() << " Layer: libmms is the GPU (HIP) implementation; " \
  "CPU mode is served by the reference's own Forward_cpu/Backward_cpu, not by this library."
#endif  // MMS_LAYER_ABI_HPP_
