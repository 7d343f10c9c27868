// csrc/caffe_runtime.cpp -- the free functions caffe_api.hpp declares and every layer leans on: caffe_rng /
// caffe_set_random_seed, the four fillers behind GetFiller (constant, uniform, gaussian, xavier), caffe_gpu_dot,
// and the check, made once when libmms_caffe.so is loaded, that libmms_hip.so speaks the ABI version this library
// was compiled against.
#include "layer_abi.hpp"

namespace caffe {

// --------------------------------- RNG + fillers -----------------------------
std::mt19937& caffe_rng() {
  static std::mt19937 g(std::random_device{}());
  return g;
}
void caffe_set_random_seed(unsigned seed) { caffe_rng().seed(seed); }

template <typename Dtype>
class ConstantFiller : public Filler<Dtype> {
 public:
  using Filler<Dtype>::Filler;
  void Fill(Blob<Dtype>* blob) override {
    Dtype* data = blob->mutable_cpu_data();
    const Dtype v = this->filler_param_.value();
    for (int i = 0; i < blob->count(); ++i) data[i] = v;
  }
};
template <typename Dtype>
class UniformFiller : public Filler<Dtype> {
 public:
  using Filler<Dtype>::Filler;
  void Fill(Blob<Dtype>* blob) override {
    CHECK(blob->count());
    std::uniform_real_distribution<Dtype> d(this->filler_param_.min(), this->filler_param_.max());
    Dtype* data = blob->mutable_cpu_data();
    for (int i = 0; i < blob->count(); ++i) data[i] = d(caffe_rng());
  }
};
template <typename Dtype>
class GaussianFiller : public Filler<Dtype> {
 public:
  using Filler<Dtype>::Filler;
  void Fill(Blob<Dtype>* blob) override {
    CHECK(blob->count());
    std::normal_distribution<Dtype> d(this->filler_param_.mean(), this->filler_param_.std());
    Dtype* data = blob->mutable_cpu_data();
    for (int i = 0; i < blob->count(); ++i) data[i] = d(caffe_rng());
  }
};
template <typename Dtype>
class XavierFiller : public Filler<Dtype> {  // fan-in variance norm
 public:
  using Filler<Dtype>::Filler;
  void Fill(Blob<Dtype>* blob) override {
    CHECK(blob->count());
    const int fan_in = blob->count() / blob->num();
    const Dtype scale = std::sqrt(Dtype(3) / fan_in);
    std::uniform_real_distribution<Dtype> d(-scale, scale);
    Dtype* data = blob->mutable_cpu_data();
    for (int i = 0; i < blob->count(); ++i) data[i] = d(caffe_rng());
  }
};
template <typename Dtype>
Filler<Dtype>* GetFiller(const FillerParameter& param) {
  const string& type = param.type();
  if (type == "constant") return new ConstantFiller<Dtype>(param);
  if (type == "uniform") return new UniformFiller<Dtype>(param);
  if (type == "gaussian") return new GaussianFiller<Dtype>(param);
  if (type == "xavier") return new XavierFiller<Dtype>(param);
  CHECK(false) << "Unknown filler name: " << type;
  return nullptr;
}
template Filler<float>* GetFiller<float>(const FillerParameter&);
template Filler<double>* GetFiller<double>(const FillerParameter&);

// A Layer host built against one include/mms.h must not run on a libmms_hip.so built from another (argument lists
// changed between ABI versions): checked once when this library is loaded, fatal like every other CHECK here.
namespace {
struct AbiVersionCheck {
  AbiVersionCheck() {
    CHECK_EQ(mms_version(), (int)MMS_VERSION) << "libmms_hip.so ABI version differs from the include/mms.h this "
                                                 "Layer library was compiled against; rebuild both";
  }
} g_abi_version_check;
}  // namespace

// caffe_gpu_dot (src/caffe/util/math_functions.cu): the product is formed on the device, one scalar comes back
template <typename T, typename F>
static T gpu_dot_impl(int n, const T* x, const T* y, F fn) {
  static thread_local T* dev = nullptr;
  if (!dev && hipMalloc(reinterpret_cast<void**>(&dev), sizeof(T)) != hipSuccess) MMS_FATAL("") << "hipMalloc failed";
  mms_check(fn(n, x, y, dev, nullptr), "mms_dot");
  T host = 0;
  if (hipMemcpy(&host, dev, sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) MMS_FATAL("") << "hipMemcpy failed";
  return host;
}
float caffe_gpu_dot(int n, const float* x, const float* y) { return gpu_dot_impl<float>(n, x, y, mms_dot_f32); }
double caffe_gpu_dot(int n, const double* x, const double* y) { return gpu_dot_impl<double>(n, x, y, mms_dot_f64); }

}  // namespace caffe
