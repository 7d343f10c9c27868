// csrc/layers_scoring.cpp -- the layers of the scoring path: SimCross, SimMatrix, and PairRankLoss on its
// LossLayer base, for float and double.  Layer set-up, shape rules, parameter blob order and every
// reference-visible quirk follow the reference sources cited next to each method; the compute bodies are not
// restated here at all -- they are calls into the C ABI (layer_abi.hpp).
#include <type_traits>

#include "layer_abi.hpp"
#include "path_net.hpp"

namespace caffe {

// ===================================== SimCross ==============================
// Reference: include/caffe/layers/sim_cross_layer.hpp, src/caffe/layers/sim_cross_layer.cpp
template <typename Dtype>
class SimCrossLayer : public Layer<Dtype> {
 public:
  explicit SimCrossLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  const char* type() const override { return "SimCross"; }
  int ExactNumBottomBlobs() const override { return 2; }
  int ExactNumTopBlobs() const override { return 1; }

  // sim_cross_layer.cpp:10-47.  Quirks kept: pre-loaded blobs_ are NOT honoured
  // (no "Skipping parameter initialization" branch) and param_propagate_down_
  // is never sized.
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK(bottom.size() == 2);
    CHECK(bottom[0]->num() == bottom[1]->num());
    CHECK(bottom[0]->height() == bottom[1]->height());
    const SimCrossParameter& p = this->layer_param_.sim_cross_param();
    dist_mode_ = p.dist_mode();
    CHECK(dist_mode_ >= 0 && dist_mode_ <= 2) << "dist_mode must be 0 (cosine), 1 (euclid) or 2 (bilinear)";
    if (dist_mode_ == 2) {
      const bool bias_term = p.bias_term();
      this->blobs_.resize(bias_term ? 2 : 1);
      this->blobs_[0].reset(new Blob<Dtype>(vector<int>{p.mesure_count(), bottom[0]->height(), bottom[1]->height()}));
      shared_ptr<Filler<Dtype> > wf(GetFiller<Dtype>(p.weight_filler()));
      wf->Fill(this->blobs_[0].get());
      if (bias_term) {
        this->blobs_[1].reset(new Blob<Dtype>(vector<int>{p.mesure_count(), bottom[0]->channels(), bottom[1]->channels()}));
        shared_ptr<Filler<Dtype> > bf(GetFiller<Dtype>(p.bias_filler()));
        bf->Fill(this->blobs_[1].get());
      }
    }
  }

  // sim_cross_layer.cpp:50-80.  top = (N, M|1, W1, W2); data{0,1}_norm_ for mode 0.
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    const int M = dist_mode_ == 2 ? this->layer_param_.sim_cross_param().mesure_count() : 1;
    top[0]->Reshape(vector<int>{bottom[0]->num(), M, bottom[0]->channels(), bottom[1]->channels()});
    if (dist_mode_ == 0) {
      data0_norm_.Reshape(vector<int>{bottom[0]->num(), bottom[0]->channels()});
      data1_norm_.Reshape(vector<int>{bottom[1]->num(), bottom[1]->channels()});
    }
    const size_t ws = abi::simcross_ws(Dtype(0), dist_mode_, bottom[0]->num(), bottom[0]->channels(),
                                       bottom[1]->channels(), bottom[0]->height(), M);
    workspace_.reserve(ws, /*keep_if_zero=*/true);
  }

  // "euclid_backward_mode": MMS_EUCLID_BWD_FP32 (0) / MMS_EUCLID_BWD_REFERENCE (1) for THIS layer; -1 = the thread's
  bool SetOption(const std::string& key, int value) override {
    if (key != "euclid_backward_mode" || value < -1 || value > 1) return false;
    euclid_bwd_mode_ = value;
    return true;
  }

  // Scoring straight from word ids (PathNet's "fuse_embed_scoring"): top = this layer applied to
  // (Embed(ids_q), Embed(ids_a)) with the Embed layers' shared table and bias, the gather done by the forward
  // kernels' own loads (include/mms.h: mms_embed_simcross_forward_f32 / _bilinear_forward_f32).  `bottom` are the
  // layer's ordinary bottoms -- shapes only, their data is neither read nor written.  Returns false when the
  // geometry has no fused kernel (the caller then runs the Embed layers and Forward as usual).
  bool ForwardFromWordIds(const Blob<Dtype>& ids_q, const Blob<Dtype>& ids_a, const Blob<Dtype>& table,
                          const Blob<Dtype>* embed_bias, const vector<Blob<Dtype>*>& bottom,
                          const vector<Blob<Dtype>*>& top) {
    if constexpr (std::is_same<Dtype, float>::value) {
      this->Reshape(bottom, top);
      const int N = bottom[0]->num(), W1 = bottom[0]->channels(), W2 = bottom[1]->channels(), D = bottom[0]->height();
      if (ids_q.count() != N * W1 || ids_a.count() != N * W2 || table.num_axes() != 2 || table.shape(1) != D) return false;
      const int K = table.shape(0), M = top[0]->channels();
      const float* eb = embed_bias ? embed_bias->gpu_data() : nullptr;
      int rc;
      if (dist_mode_ == 2)
        rc = mms_embed_simcross_bilinear_forward_f32(N, W1, W2, D, M, K, ids_q.gpu_data(), ids_a.gpu_data(),
                                                     table.gpu_data(), eb, this->blobs_[0]->gpu_data(),
                                                     this->blobs_.size() > 1 ? this->blobs_[1]->gpu_data() : nullptr,
                                                     top[0]->mutable_gpu_data(), nullptr);
      else
        rc = mms_embed_simcross_forward_f32(dist_mode_, N, W1, W2, D, K, ids_q.gpu_data(), ids_a.gpu_data(),
                                            table.gpu_data(), eb, top[0]->mutable_gpu_data(),
                                            dist_mode_ == 0 ? data0_norm_.mutable_gpu_data() : nullptr,
                                            dist_mode_ == 0 ? data1_norm_.mutable_gpu_data() : nullptr, nullptr);
      if (rc == MMS_ERR_UNSUPPORTED) return false;
      mms_check(rc, "mms_embed_simcross_forward");
      return true;
    } else {
      return false;                                    // the fused entry points are fp32
    }
  }

 protected:
  void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }
  void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }

  // replaces sim_cross_layer.cpp:83-163 / sim_cross_layer.cu:128-194
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    const int M = top[0]->channels();
    const bool mode2 = dist_mode_ == 2, mode0 = dist_mode_ == 0;
    mms_check(abi::simcross_forward(
                  dist_mode_, bottom[0]->num(), bottom[0]->channels(), bottom[1]->channels(),
                  bottom[0]->height(), M, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                  mode2 ? this->blobs_[0]->gpu_data() : nullptr,
                  (mode2 && this->blobs_.size() > 1) ? this->blobs_[1]->gpu_data() : nullptr,
                  top[0]->mutable_gpu_data(), mode0 ? data0_norm_.mutable_gpu_data() : nullptr,
                  mode0 ? data1_norm_.mutable_gpu_data() : nullptr,
                  workspace_.data(), workspace_.bytes()),
              "mms_simcross_forward");
  }

  // replaces sim_cross_layer.cpp:166-307 / sim_cross_layer.cu:197-243
  void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down,
                    const vector<Blob<Dtype>*>& bottom) override {
    const int M = top[0]->channels();
    const bool mode2 = dist_mode_ == 2, mode0 = dist_mode_ == 0;
    const bool bias_term = mode2 && this->blobs_.size() > 1;
    // this layer's arithmetic of the Euclidean backward term, if one was pinned (SetOption): the C ABI's mode
    // belongs to the calling thread, so it is set for the duration of this call and put back
    struct ModeGuard {
      int saved;
      explicit ModeGuard(int m) : saved(-1) {
        if (m >= 0) { saved = mms_get_euclid_backward_mode(); mms_set_euclid_backward_mode(m); }
      }
      ~ModeGuard() { if (saved >= 0) mms_set_euclid_backward_mode(saved); }
    } guard(euclid_bwd_mode_);
    mms_check(abi::simcross_backward(
                  dist_mode_, bottom[0]->num(), bottom[0]->channels(), bottom[1]->channels(),
                  bottom[0]->height(), M, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                  mode2 ? this->blobs_[0]->gpu_data() : nullptr, bias_term, top[0]->gpu_data(),
                  top[0]->gpu_diff(), mode0 ? data0_norm_.gpu_data() : nullptr,
                  mode0 ? data1_norm_.gpu_data() : nullptr, propagate_down[0], propagate_down[1],
                  bottom[0]->mutable_gpu_diff(), bottom[1]->mutable_gpu_diff(),
                  mode2 ? this->blobs_[0]->mutable_gpu_diff() : nullptr,
                  bias_term ? this->blobs_[1]->mutable_gpu_diff() : nullptr,
                  workspace_.data(), workspace_.bytes()),
              "mms_simcross_backward");
  }

  int dist_mode_ = 1;  // 1 euclid, 0 cosine, 2 bilinear (sim_cross_layer.hpp:36)
  int euclid_bwd_mode_ = -1;  // -1: the calling thread's mode; else MMS_EUCLID_BWD_FP32 / _REFERENCE for this layer
  Blob<Dtype> data0_norm_, data1_norm_;
  Workspace<Dtype> workspace_;  // replaces measure_temp{0,1}_
};
INSTANTIATE_CLASS_FD(SimCrossLayer);
REGISTER_LAYER_CLASS_FD(SimCross);

bool SimCrossForwardFromWordIds(Layer<float>& sim, const Blob<float>& ids_q, const Blob<float>& ids_a,
                                const Blob<float>& table, const Blob<float>* embed_bias,
                                const vector<Blob<float>*>& bottom, const vector<Blob<float>*>& top) {
  return static_cast<SimCrossLayer<float>&>(sim).ForwardFromWordIds(ids_q, ids_a, table, embed_bias, bottom, top);
}

// ===================================== SimMatrix =============================
// Reference: include/caffe/layers/sim_matrix_layer.hpp, src/caffe/layers/sim_matrix_layer.cpp
template <typename Dtype>
class SimMatrixLayer : public Layer<Dtype> {
 public:
  explicit SimMatrixLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  const char* type() const override { return "SimMatrix"; }
  int ExactNumBottomBlobs() const override { return 2; }
  int ExactNumTopBlobs() const override { return 1; }

  // sim_matrix_layer.cpp:10-34 (honours pre-loaded blobs)
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_EQ(bottom[0]->num(), bottom[1]->num());
    K1_ = bottom[0]->count(1);
    K2_ = bottom[1]->count(1);
    if (this->blobs_.size() > 0) {
      LOG_INFO << "Skipping parameter initialization";
    } else {
      this->blobs_.resize(1);
      this->blobs_[0].reset(new Blob<Dtype>(vector<int>{K1_, K2_}));
      shared_ptr<Filler<Dtype> > wf(GetFiller<Dtype>(this->layer_param_.sim_matrix_param().weight_filler()));
      wf->Fill(this->blobs_[0].get());
    }
    this->param_propagate_down_.resize(this->blobs_.size(), true);
  }

  // sim_matrix_layer.cpp:37-50
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_EQ(K1_, bottom[0]->count(1)) << "Input size incompatible with inner product parameters.";
    CHECK_EQ(K2_, bottom[1]->count(1)) << "Input size incompatible with inner product parameters.";
    M_ = bottom[0]->count(0, 1);
    top[0]->Reshape(vector<int>{bottom[0]->shape(0), 1});
    const size_t ws = abi::simmatrix_ws(Dtype(0), M_, K1_, K2_);
    workspace_.reserve(ws);
    if (qw_elems_ != M_ * K2_) { qw_valid_ = false; qw_elems_ = M_ * K2_; }
    if (private_qw_) qw_.Reshape(vector<int>{M_, K2_});
  }

 protected:
  void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }
  void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }

  // replaces sim_matrix_layer.cpp:53-65.  Like the reference, Forward leaves Q*W in bottom[1]'s DIFF buffer
  // (:58 takes bottom[1]->mutable_cpu_diff() as its scratch) -- an observable side effect, kept by default.
  // Backward then finds the product where the reference's forward left it and scales it in place into
  // da_j = dT_j * (W^T q_j) (:88) instead of running the same GEMM again: nothing in a Caffe net writes a
  // bottom's diff between a layer's Forward and its own Backward.  A host that does touch that buffer in
  // between can switch the layer to a private copy: SetOption("private_qw", 1) (then Forward leaves
  // bottom[1]'s diff alone, which is the only difference).
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    Dtype* qw = private_qw_ ? qw_.mutable_gpu_data() : bottom[1]->mutable_gpu_diff();
    mms_check(abi::simmatrix_forward(M_, K1_, K2_, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                                     this->blobs_[0]->gpu_data(), top[0]->mutable_gpu_data(), qw,
                                     workspace_.data(), workspace_.bytes()),
              "mms_simmatrix_forward");
    qw_valid_ = true;
  }
  // replaces sim_matrix_layer.cpp:68-95
  void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down,
                    const vector<Blob<Dtype>*>& bottom) override {
    const bool ppd = this->param_propagate_down_[0];
    if (qw_valid_) {
      const Dtype* qw = private_qw_ ? qw_.gpu_data() : bottom[1]->gpu_diff();   // in place when it is the diff
      mms_check(abi::simmatrix_backward_cached(
                    M_, K1_, K2_, bottom[0]->gpu_data(), bottom[1]->gpu_data(), this->blobs_[0]->gpu_data(),
                    qw, top[0]->gpu_diff(), ppd, propagate_down[0], propagate_down[1],
                    propagate_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
                    propagate_down[1] ? bottom[1]->mutable_gpu_diff() : nullptr,
                    ppd ? this->blobs_[0]->mutable_gpu_diff() : nullptr,
                    workspace_.data(), workspace_.bytes()),
                "mms_simmatrix_backward_cached");
      if (!private_qw_ && propagate_down[1]) qw_valid_ = false;   // the diff now holds da, not Q*W
      return;
    }
    mms_check(abi::simmatrix_backward(
                  M_, K1_, K2_, bottom[0]->gpu_data(), bottom[1]->gpu_data(), this->blobs_[0]->gpu_data(),
                  top[0]->gpu_diff(), ppd, propagate_down[0], propagate_down[1],
                  propagate_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
                  propagate_down[1] ? bottom[1]->mutable_gpu_diff() : nullptr,
                  ppd ? this->blobs_[0]->mutable_gpu_diff() : nullptr,
                  workspace_.data(), workspace_.bytes()),
              "mms_simmatrix_backward");
  }
 public:
  bool SetOption(const std::string& key, int value) override {
    if (key != "private_qw") return false;
    private_qw_ = value != 0;
    qw_valid_ = false;
    return true;
  }
 protected:
  int K1_ = 0, K2_ = 0, M_ = 0;
  Workspace<Dtype> workspace_;
  Blob<Dtype> qw_;             // private_qw: Q*W of the last Forward (M_, K2_)
  bool qw_valid_ = false;
  bool private_qw_ = false;
  int qw_elems_ = 0;
};
INSTANTIATE_CLASS_FD(SimMatrixLayer);
REGISTER_LAYER_CLASS_FD(SimMatrix);

// ================================ LossLayer / PairRankLoss ===================
// Reference: include/caffe/layers/loss_layer.hpp:22-49, src/caffe/layers/loss_layer.cpp:8-23
template <typename Dtype>
class LossLayer : public Layer<Dtype> {
 public:
  explicit LossLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    if (this->layer_param_.loss_weight_size() == 0) this->layer_param_.add_loss_weight(Dtype(1));
  }
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_EQ(bottom[0]->num(), bottom[1]->num()) << "The data and label should have the same number.";
    top[0]->Reshape(vector<int>());  // scalar, 0 axes
  }
  int ExactNumBottomBlobs() const override { return 2; }
  bool AutoTopBlobs() const override { return true; }
  int ExactNumTopBlobs() const override { return 1; }
  bool AllowForceBackward(int bottom_index) const override { return bottom_index != 1; }
};

// Reference: include/caffe/layers/pair_rank_loss_layer.hpp, src/caffe/layers/pair_rank_loss_layer.cpp
template <typename Dtype>
class PairRankLossLayer : public LossLayer<Dtype> {
 public:
  explicit PairRankLossLayer(const LayerParameter& param) : LossLayer<Dtype>(param) {}
  const char* type() const override { return "PairRankLoss"; }
  int ExactNumBottomBlobs() const override { return 3; }
  int ExactNumTopBlobs() const override { return -1; }
  int MinTopBlobs() const override { return 1; }
  int MaxTopBlobs() const override { return 2; }  // declared; only top[0] is ever written

  // pair_rank_loss_layer.cpp:10-23.  The caches are shaped ONCE here (there is no
  // Reshape override), so the batch must not grow after SetUp -- as in the reference.
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    LossLayer<Dtype>::LayerSetUp(bottom, top);
    CHECK_EQ(bottom[0]->num(), bottom[1]->num());
    CHECK_EQ(bottom[0]->num(), bottom[2]->num());
    CHECK_EQ(bottom[0]->count(1), bottom[2]->count(1));
    CHECK_EQ(bottom[0]->count(1), bottom[1]->count(1));
    margin_ = (Dtype)this->layer_param_.pair_rank_loss_param().margin();
    ordered_diff_.Reshape(bottom[0]->num(), bottom[0]->channels(), 1, 1);
    similar_diff_.Reshape(bottom[0]->num(), bottom[0]->channels(), 1, 1);
    const size_t ws = abi::pairrank_ws(Dtype(0), ordered_diff_.count());
    workspace_.reserve(ws, /*keep_if_zero=*/true);
  }

 protected:
  void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }
  void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }

  // replaces pair_rank_loss_layer.cpp:26-52 / .cu:10-43
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    const int count = bottom[0]->count();
    CHECK_LE(count, ordered_diff_.count()) << "PairRankLoss caches are sized in LayerSetUp; batch grew";
    mms_check(abi::pairrank_forward(count, margin_, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                                    bottom[2]->gpu_data(), ordered_diff_.mutable_gpu_data(),
                                    similar_diff_.mutable_gpu_data(), top[0]->mutable_gpu_data(),
                                    workspace_.data(), workspace_.bytes()),
              "mms_pairrank_forward");
  }
  // replaces pair_rank_loss_layer.cpp:55-84 (CPU semantics: strict '>')
  void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down,
                    const vector<Blob<Dtype>*>& bottom) override {
    if (propagate_down[2]) LOG_FATAL << this->type() << " Layer cannot backpropagate to label inputs.";
    if (!propagate_down[0] && !propagate_down[1]) return;
    mms_check(abi::pairrank_backward(bottom[0]->count(), top[0]->cpu_diff()[0], bottom[2]->gpu_data(),
                                     ordered_diff_.gpu_data(), similar_diff_.gpu_data(),
                                     propagate_down[0], propagate_down[1],
                                     propagate_down[0] ? bottom[0]->mutable_gpu_diff() : nullptr,
                                     propagate_down[1] ? bottom[1]->mutable_gpu_diff() : nullptr),
              "mms_pairrank_backward");
  }
  Dtype margin_ = 1;
  Blob<Dtype> ordered_diff_, similar_diff_;
  Workspace<Dtype> workspace_;
};
INSTANTIATE_CLASS_FD(PairRankLossLayer);
REGISTER_LAYER_CLASS_FD(PairRankLoss);

}  // namespace caffe
