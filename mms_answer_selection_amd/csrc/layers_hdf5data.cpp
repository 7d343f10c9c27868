// csrc/layers_hdf5data.cpp -- the HDF5Data layer (float): the files of a source list decoded by hdf5_io.cpp, held
// in device memory, and dealt out a batch at a time by a gather kernel of the C ABI.
#include <algorithm>
#include <fstream>

#include "hdf5_io.hpp"
#include "layer_abi.hpp"

namespace caffe {

// ===================================== HDF5Data ==============================
// Reference: include/caffe/layers/hdf5_data_layer.hpp, src/caffe/layers/hdf5_data_layer.cpp
// :27-151 and .cu:19-51.  `source` lists one .h5 file per line; every top is the dataset of
// the same name, loaded whole and converted to float (util/hdf5.cpp:10-73); a batch is the
// next batch_size rows, moving on to the next file (and wrapping) when a file is used up,
// so a batch can straddle two files.  No libhdf5 here: csrc/hdf5_io.cpp decodes the files.
//
// MI355X shape of it: the reference keeps the file's blobs on the host and issues batch_size
// x top_size small copies per Forward (H2D in its GPU path).  Here a file's datasets are
// uploaded to HBM once, when the file is opened, and a batch is one gather launch per top
// and per contiguous run of rows (mms_feed_gather_rows_f32): no per-step PCIe traffic.
//
// shuffle: the reference uses std::random_shuffle, i.e. libstdc++'s `rand() % (i+1)` swaps
// driven by the C library's rand() state, which nothing in Caffe seeds.  The same loop and
// the same rand() are used here, so a process with the same rand() history shuffles alike.
template <typename Dtype>
class HDF5DataLayer : public Layer<Dtype> {
 public:
  explicit HDF5DataLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  const char* type() const override { return "HDF5Data"; }
  int ExactNumBottomBlobs() const override { return 0; }
  int MinTopBlobs() const override { return 1; }

  void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    CHECK(!this->layer_param_.has_transform_param()) << this->type() << " does not transform data.";
    const string& source = this->layer_param_.hdf5_data_param().source();
    LOG_INFO << "Loading list of HDF5 filenames from: " << source;
    hdf_filenames_.clear();
    std::ifstream source_file(source.c_str());
    CHECK(source_file.is_open()) << "Failed to open source file: " << source;
    string line;
    while (source_file >> line) hdf_filenames_.push_back(line);
    source_file.close();
    num_files_ = (int)hdf_filenames_.size();
    current_file_ = 0;
    CHECK_GE(num_files_, 1) << "Must have at least 1 HDF5 filename listed in " << source;
    file_permutation_.resize(num_files_);
    for (int i = 0; i < num_files_; ++i) file_permutation_[i] = i;
    if (this->layer_param_.hdf5_data_param().shuffle()) RandomShuffle(&file_permutation_);
    LoadHDF5FileData(hdf_filenames_[file_permutation_[current_file_]].c_str());
    current_row_ = 0;
    const int batch_size = this->layer_param_.hdf5_data_param().batch_size();
    for (size_t i = 0; i < top.size(); ++i) {
      vector<int> top_shape = hdf_blobs_[i]->shape();
      top_shape[0] = batch_size;
      top[i]->Reshape(top_shape);
    }
  }
  void Reshape(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override {}

 protected:
  // libstdc++'s std::random_shuffle(first, last) (removed in C++17), spelled out.
  static void RandomShuffle(vector<int>* v) {
    for (size_t i = 1; i < v->size(); ++i) {
      const size_t j = (size_t)std::rand() % (i + 1);
      if (i != j) std::swap((*v)[i], (*v)[j]);
    }
  }
  void UploadPermutation() {
    const int n = (int)data_permutation_.size();
    perm_mem_.reset(new SyncedMemory((size_t)n * sizeof(int)));
    std::memcpy(perm_mem_->mutable_cpu_data(), data_permutation_.data(), (size_t)n * sizeof(int));
  }
  void LoadHDF5FileData(const char* filename) {
    mms_h5::File file;
    string err;
    CHECK(file.Open(filename, &err)) << err;
    const int top_size = this->layer_param_.top_size();
    hdf_blobs_.resize(top_size);
    for (int i = 0; i < top_size; ++i) {
      const string& name = this->layer_param_.top(i);
      CHECK(file.Find(name)) << "Failed to find HDF5 dataset " << name;
      mms_h5::DatasetInfo info;
      std::vector<float> values;
      CHECK(file.ReadFloat(name, &info, &values, &err)) << "Failed to read float dataset " << name << ": " << err;
      CHECK_GE((int)info.dims.size(), 1) << "Input must have at least 1 axis.";
      vector<int> shape;
      for (int64_t d : info.dims) shape.push_back((int)d);
      hdf_blobs_[i].reset(new Blob<Dtype>(shape));
      std::memcpy(hdf_blobs_[i]->mutable_cpu_data(), values.data(), values.size() * sizeof(float));
    }
    const int num = hdf_blobs_[0]->shape(0);
    for (int i = 1; i < top_size; ++i) CHECK_EQ(hdf_blobs_[i]->shape(0), num);
    data_permutation_.resize(num);
    for (int i = 0; i < num; ++i) data_permutation_[i] = i;
    if (this->layer_param_.hdf5_data_param().shuffle()) RandomShuffle(&data_permutation_);
    UploadPermutation();
  }
  void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) override { NO_CPU_MODE; }
  void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override {}
  void Backward_gpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) override {}

  // Same row/file walk as hdf5_data_layer.cpp:124-151, taken a run of rows at a time.
  void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) override {
    const int batch_size = this->layer_param_.hdf5_data_param().batch_size();
    const bool shuffle = this->layer_param_.hdf5_data_param().shuffle();
    int i = 0;
    while (i < batch_size) {
      if (current_row_ == hdf_blobs_[0]->shape(0)) {
        if (num_files_ > 1) {
          ++current_file_;
          if (current_file_ == num_files_) {
            current_file_ = 0;
            if (shuffle) RandomShuffle(&file_permutation_);
          }
          // launches reading the old file's buffers are on the null stream; hipFree in
          // ~SyncedMemory synchronises with them before the memory goes away
          LoadHDF5FileData(hdf_filenames_[file_permutation_[current_file_]].c_str());
        }
        current_row_ = 0;
        if (shuffle) { RandomShuffle(&data_permutation_); HIP_CHECK(hipDeviceSynchronize()); UploadPermutation(); }
      }
      const int rows = hdf_blobs_[0]->shape(0);
      CHECK_GT(rows, 0) << "HDF5 file with no rows";
      const int run = std::min(batch_size - i, rows - current_row_);
      for (size_t j = 0; j < top.size(); ++j) {
        const int data_dim = top[j]->count() / top[j]->shape(0);
        mms_check(mms_feed_gather_rows_f32(run, data_dim, rows, hdf_blobs_[j]->gpu_data(),
                                           shuffle ? static_cast<const int*>(perm_mem_->gpu_data()) : nullptr,
                                           current_row_, top[j]->mutable_gpu_data() + (size_t)i * data_dim, nullptr),
                  "mms_feed_gather_rows_f32");
      }
      i += run;
      current_row_ += run;
    }
  }

  vector<string> hdf_filenames_;
  int num_files_ = 0, current_file_ = 0, current_row_ = 0;
  vector<shared_ptr<Blob<Dtype> > > hdf_blobs_;
  vector<int> data_permutation_, file_permutation_;
  std::unique_ptr<SyncedMemory> perm_mem_;
};
INSTANTIATE_CLASS(HDF5DataLayer);
REGISTER_LAYER_CLASS(HDF5Data);

}  // namespace caffe
