// csrc/layers_metrics.cpp -- the ranking-metric layers MAP, MRR, AUC and RankAccuracy (forward only) on their
// common base, each one call into the ranking kernels of the C ABI.  MAP is registered for float, the other
// three for float and double.
#include "layer_abi.hpp"

namespace caffe {

// ===================== MAP / MRR / AUC / RankAccuracy (forward only) =========
// Reference: src/caffe/layers/{map,mrr,auc,rank_accuracy}_layer.cpp and their headers.
// The reference has no GPU code for these (Forward_gpu falls back to Forward_cpu through
// the base class, i.e. a D2H copy of the whole score blob); here they run on the device.
template <typename Dtype>
class RankMetricLayerBase : public Layer<Dtype> {
 public:
  explicit RankMetricLayerBase(const LayerParameter& param) : Layer<Dtype>(param) {}
  int ExactNumTopBlobs() const override { return 1; }
 protected:
  void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }
  // map_layer.cpp / mrr_layer.cpp / auc_layer.cpp: Backward is a no-op for metric layers
  void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override {}
  void Backward_gpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override {}
  void size_workspace(int n) {
    const size_t ws = abi::rank_ws(Dtype(), n);
    workspace_.reserve(ws);
  }
  Workspace<Dtype> workspace_;
};

// MAP and MRR are one walk (abi::rank_map_mrr yields both figures): a Metric says which of the two this layer writes,
// under which type string, and which parameter message holds its fixed_axis.
struct MAPMetric {
  static constexpr bool kIsMAP = true;
  static const char* type() { return "MAP"; }
  static int fixed_axis(const LayerParameter& p) { return p.map_param().fixed_axis(); }           // map_layer.cpp:13
};
struct MRRMetric {
  static constexpr bool kIsMAP = false;
  static const char* type() { return "MRR"; }
  static int fixed_axis(const LayerParameter& p) { return p.mrr_param().fixed_axis(); }           // mrr_layer.cpp:13
};
template <typename Dtype, typename Metric>
class MapMrrLayer : public RankMetricLayerBase<Dtype> {
 public:
  explicit MapMrrLayer(const LayerParameter& param) : RankMetricLayerBase<Dtype>(param) {}
  const char* type() const override { return Metric::type(); }
  int ExactNumBottomBlobs() const override { return 3; }
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    fixed_axis_ = Metric::fixed_axis(this->layer_param_);
  }
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_LE(fixed_axis_, bottom[0]->count() / bottom[1]->count())
        << "top_k must be less than or equal to the number of classes.";
    const int outer = bottom[0]->count(0, 1), inner = bottom[0]->count(2);
    CHECK_EQ(outer * inner, bottom[1]->count()) << "Number of labels must match number of predictions";
    CHECK_EQ(outer * inner, bottom[2]->count());
    top[0]->Reshape(vector<int>());
    this->size_workspace(bottom[0]->num());
  }
 protected:
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    Dtype* const out = top[0]->mutable_gpu_data();
    Dtype* const none = nullptr;
    mms_check(abi::rank_map_mrr(bottom[0]->num(), fixed_axis_, bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                                bottom[2]->gpu_data(), Metric::kIsMAP ? out : none, Metric::kIsMAP ? none : out,
                                this->workspace_.data(), this->workspace_.bytes()),
              "mms_rank_map_mrr");
  }
  int fixed_axis_ = 1;
};
template <typename Dtype> using MAPLayer = MapMrrLayer<Dtype, MAPMetric>;
template <typename Dtype> using MRRLayer = MapMrrLayer<Dtype, MRRMetric>;
// MAP for float only, although the body above serves double as well: tests/test_layers_f64_gpu.py pins that
// mms_layer_run_f64 answers "no Layer<double> registered" for MAP.  MRR is the same walk for double.
template class MapMrrLayer<float, MAPMetric>;
REGISTER_LAYER_CLASS(MAP);
template class MapMrrLayer<float, MRRMetric>;
template class MapMrrLayer<double, MRRMetric>;
REGISTER_LAYER_CLASS_FD(MRR);

template <typename Dtype>
class AUCLayer : public RankMetricLayerBase<Dtype> {
 public:
  explicit AUCLayer(const LayerParameter& param) : RankMetricLayerBase<Dtype>(param) {}
  const char* type() const override { return "AUC"; }
  int ExactNumBottomBlobs() const override { return 2; }
  int ExactNumTopBlobs() const override { return -1; }
  int MinTopBlobs() const override { return 1; }
  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    const AUCParameter& p = this->layer_param_.auc_param();               // auc_layer.cpp:14-20
    fixed_axis_ = p.fixed_axis();
    has_ignore_label_ = p.has_ignore_label();
    if (has_ignore_label_) ignore_label_ = p.ignore_label();
  }
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_LE(fixed_axis_, bottom[0]->count() / bottom[1]->count())
        << "top_k must be less than or equal to the number of classes.";
    label_axis_ = bottom[0]->CanonicalAxisIndex(this->layer_param_.auc_param().axis());
    outer_num_ = bottom[0]->count(0, label_axis_);
    inner_num_ = bottom[0]->count(label_axis_ + 1);
    CHECK_EQ(outer_num_ * inner_num_, bottom[1]->count()) << "Number of labels must match number of predictions";
    top[0]->Reshape(vector<int>());
    this->size_workspace(outer_num_ * inner_num_);
  }
 protected:
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    mms_check(abi::rank_auc_nd(outer_num_, bottom[0]->shape(label_axis_), inner_num_, fixed_axis_,
                               bottom[0]->gpu_data(), bottom[1]->gpu_data(), has_ignore_label_,
                               ignore_label_, top[0]->mutable_gpu_data(),
                               this->workspace_.data(), this->workspace_.bytes()),
              "mms_rank_auc_nd");
  }
  int fixed_axis_ = 1, label_axis_ = 1, outer_num_ = 0, inner_num_ = 1, ignore_label_ = 0;
  bool has_ignore_label_ = false;
};
INSTANTIATE_CLASS_FD(AUCLayer);
REGISTER_LAYER_CLASS_FD(AUC);

template <typename Dtype>
class RankAccuracyLayer : public RankMetricLayerBase<Dtype> {
 public:
  explicit RankAccuracyLayer(const LayerParameter& param) : RankMetricLayerBase<Dtype>(param) {}
  const char* type() const override { return "RankAccuracy"; }
  int ExactNumBottomBlobs() const override { return 3; }
  int ExactNumTopBlobs() const override { return -1; }
  int MinTopBlobs() const override { return 1; }
  void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK_EQ(bottom[0]->count(), bottom[1]->count()) << "two pairs have the same dimension!.";
    CHECK_EQ(bottom[0]->count(), bottom[2]->count()) << "pair should have the same dimension with the label!.";
    top[0]->Reshape(vector<int>());
    this->size_workspace(1);
  }
 protected:
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    mms_check(abi::rank_accuracy(bottom[0]->count(), bottom[0]->gpu_data(), bottom[1]->gpu_data(),
                                 bottom[2]->gpu_data(), top[0]->mutable_gpu_data(),
                                 this->workspace_.data(), this->workspace_.bytes()),
              "mms_rank_accuracy");
  }
};
INSTANTIATE_CLASS_FD(RankAccuracyLayer);
REGISTER_LAYER_CLASS_FD(RankAccuracy);

}  // namespace caffe
