// csrc/layer_handles.cpp -- the C handle API of include/mms_layer.h over the C++ mirror: mms_blob / mms_layer /
// mms_net handles and their calls, mms_caffe_set_mode / mms_caffe_set_random_seed, mms_layer_registry_types, and
// mms_layer_run_f64 (the one entry point that drives Layer<double>).  The mms_snapshot_* and mms_h5_* calls sit
// beside their implementations in caffemodel_io.cpp and hdf5_io.cpp.
#include <algorithm>

#include "capi_err.hpp"
#include "mms_layer.h"
#include "path_net.hpp"

struct mms_blob {
  caffe::Blob<float>* b;
  std::shared_ptr<caffe::Blob<float> > keep;  // set for borrowed parameter blobs
  bool owned;
};
struct mms_layer {
  std::shared_ptr<caffe::Layer<float> > l;
  std::vector<std::unique_ptr<mms_blob> > param_handles;
};
struct mms_net {
  std::unique_ptr<caffe::PathNet> net;
  std::map<std::string, std::unique_ptr<mms_blob> > blob_handles;
  std::vector<std::unique_ptr<mms_layer> > layer_handles;
};

namespace {
std::vector<caffe::Blob<float>*> unwrap(mms_blob_t* const* v, int n) {
  std::vector<caffe::Blob<float>*> out(n);
  for (int i = 0; i < n; ++i) out[i] = v[i]->b;
  return out;
}
std::vector<int> shape_vec(const int* shape, int n) { return std::vector<int>(shape, shape + n); }
}  // namespace

extern "C" {

mms_blob_t* mms_blob_create(const int* shape, int num_axes) {
  // no axes = the default constructor (count 0, nothing allocated: blob.hpp:26-27), as `new Blob<Dtype>()`
  mms_blob_t* h = new mms_blob{num_axes > 0 ? new caffe::Blob<float>(shape_vec(shape, num_axes)) : new caffe::Blob<float>(), nullptr, true};
  return h;
}
void mms_blob_destroy(mms_blob_t* b) {
  if (!b) return;
  if (b->owned) delete b->b;
  delete b;
}
void mms_blob_reshape(mms_blob_t* b, const int* shape, int num_axes) { b->b->Reshape(shape_vec(shape, num_axes)); }
int mms_blob_num_axes(const mms_blob_t* b) { return b->b->num_axes(); }
int mms_blob_shape(const mms_blob_t* b, int axis) { return b->b->shape(axis); }
int mms_blob_count(const mms_blob_t* b) { return b->b->count(); }
const float* mms_blob_cpu(mms_blob_t* b, int which) { return which ? b->b->cpu_diff() : b->b->cpu_data(); }
float* mms_blob_mutable_cpu(mms_blob_t* b, int which) { return which ? b->b->mutable_cpu_diff() : b->b->mutable_cpu_data(); }
const float* mms_blob_gpu(mms_blob_t* b, int which) { return which ? b->b->gpu_diff() : b->b->gpu_data(); }
float* mms_blob_mutable_gpu(mms_blob_t* b, int which) { return which ? b->b->mutable_gpu_diff() : b->b->mutable_gpu_data(); }

mms_layer_t* mms_layer_create(const char* prototxt, char* err, int err_len) {
  caffe::LayerParameter lp;
  std::string e;
  if (!caffe::ReadLayerParameterFromText(prototxt ? prototxt : "", &lp, &e)) {
    set_err(err, err_len, e);
    return nullptr;
  }
  mms_layer_t* h = new mms_layer;
  h->l = caffe::LayerRegistry<float>::CreateLayer(lp);
  return h;
}
void mms_layer_destroy(mms_layer_t* l) { delete l; }
const char* mms_layer_type(const mms_layer_t* l) { return l->l->type(); }
void mms_layer_setup(mms_layer_t* l, mms_blob_t* const* bottom, int nbottom, mms_blob_t* const* top, int ntop) {
  l->l->SetUp(unwrap(bottom, nbottom), unwrap(top, ntop));
}
float mms_layer_forward(mms_layer_t* l, mms_blob_t* const* bottom, int nbottom, mms_blob_t* const* top, int ntop) {
  return l->l->Forward(unwrap(bottom, nbottom), unwrap(top, ntop));
}
void mms_layer_backward(mms_layer_t* l, mms_blob_t* const* top, int ntop, const int* propagate_down,
                        mms_blob_t* const* bottom, int nbottom) {
  std::vector<bool> pd(nbottom);
  for (int i = 0; i < nbottom; ++i) pd[i] = propagate_down[i] != 0;
  l->l->Backward(unwrap(top, ntop), pd, unwrap(bottom, nbottom));
}
int mms_layer_num_param_blobs(mms_layer_t* l) { return (int)l->l->blobs().size(); }
mms_blob_t* mms_layer_param_blob(mms_layer_t* l, int i) {
  auto& blobs = l->l->blobs();
  if (i < 0 || i >= (int)blobs.size()) return nullptr;
  if ((int)l->param_handles.size() < (int)blobs.size()) l->param_handles.resize(blobs.size());
  if (!l->param_handles[i] || l->param_handles[i]->b != blobs[i].get())
    l->param_handles[i].reset(new mms_blob{blobs[i].get(), blobs[i], false});
  return l->param_handles[i].get();
}
void mms_layer_set_param_propagate_down(mms_layer_t* l, int i, int v) { l->l->set_param_propagate_down(i, v != 0); }
int mms_layer_set_option(mms_layer_t* l, const char* key, int value) { return (key && l->l->SetOption(key, value)) ? 0 : 1; }
// ---- whole nets ----
mms_net_t* mms_net_create(const char* prototxt, int phase, char* err, int err_len) {
  caffe::NetParameter np;
  std::string e;
  if (!caffe::ReadNetParameterFromText(prototxt ? prototxt : "", &np, &e)) {
    set_err(err, err_len, e);
    return nullptr;
  }
  mms_net_t* h = new mms_net;
  h->net.reset(new caffe::PathNet(np, phase ? 1 : 0));
  h->layer_handles.resize(h->net->layers().size());
  return h;
}
void mms_net_destroy(mms_net_t* n) { delete n; }
int mms_net_set_option(mms_net_t* n, const char* key, int value) { return (key && n->net->SetOption(key, value)) ? 0 : 1; }
int mms_net_num_fused(const mms_net_t* n) { return n->net->num_fused(); }
int mms_net_num_splits(const mms_net_t* n) { return n->net->num_splits(); }
const char* mms_net_name(const mms_net_t* n) { return n->net->name().c_str(); }
int mms_net_num_layers(const mms_net_t* n) { return (int)n->net->layers().size(); }
const char* mms_net_layer_name(const mms_net_t* n, int i) { return n->net->layers()[i].param.name().c_str(); }
const char* mms_net_layer_type(const mms_net_t* n, int i) { return n->net->layers()[i].param.type().c_str(); }
int mms_net_layer_supported(const mms_net_t* n, int i) { return n->net->layers()[i].layer ? 1 : 0; }
int mms_net_layer_runnable(const mms_net_t* n, int i) { return n->net->layers()[i].runnable ? 1 : 0; }
const char* mms_net_layer_why_not(const mms_net_t* n, int i) { return n->net->layers()[i].why_not.c_str(); }
mms_layer_t* mms_net_layer(mms_net_t* n, int i) {
  if (i < 0 || i >= (int)n->net->layers().size() || !n->net->layers()[i].layer) return nullptr;
  if (!n->layer_handles[i]) { n->layer_handles[i].reset(new mms_layer); n->layer_handles[i]->l = n->net->layers()[i].layer; }
  return n->layer_handles[i].get();
}
int mms_net_num_blobs(const mms_net_t* n) { return (int)n->net->blob_names().size(); }
const char* mms_net_blob_name(const mms_net_t* n, int i) { return n->net->blob_names()[i].c_str(); }
mms_blob_t* mms_net_blob(mms_net_t* n, const char* name) {
  caffe::Blob<float>* b = name ? n->net->find_blob(name) : nullptr;
  if (!b) return nullptr;
  auto& h = n->blob_handles[name];
  if (!h) h.reset(new mms_blob{b, nullptr, false});
  return h.get();
}
int mms_net_setup(mms_net_t* n) { return n->net->SetUp(); }
float mms_net_forward(mms_net_t* n) { return n->net->Forward(); }
void mms_net_backward(mms_net_t* n) { n->net->Backward(); }

void mms_caffe_set_mode(int gpu) { caffe::Caffe::set_mode(gpu ? caffe::Caffe::GPU : caffe::Caffe::CPU); }
void mms_caffe_set_random_seed(unsigned seed) { caffe::caffe_set_random_seed(seed); }
const char* mms_layer_registry_types(void) {
  static std::string s;
  s.clear();
  for (auto& t : caffe::LayerRegistry<float>::LayerTypeList()) s += (s.empty() ? "" : ",") + t;
  return s.c_str();
}

// ---- Layer<double>: one-shot run (create by type string, SetUp, Forward, Backward) ----
// The handle API above is float; this single entry point drives the double instantiation of the layers registered
// for double (the three path layers, Embed, MRR / AUC / RankAccuracy) end to end so that it can be checked
// against the oracle's double code.  The layer gets as many tops as its prototxt names (at least one); top 0 is
// the one returned.
int mms_layer_run_f64(const char* prototxt, int nbottom, const int* bottom_axes, const int* bottom_dims,
                      const double* const* bottom_data, int nparam, const double* const* param_data,
                      const double* top_diff, const int* propagate_down, double* top_out, long long top_capacity,
                      int* top_dims_out, int* top_axes_out, double* const* bottom_diff_out,
                      double* const* param_diff_out, char* err, int err_len) {
  caffe::LayerParameter lp;
  std::string e;
  if (!prototxt || !caffe::ReadLayerParameterFromText(prototxt, &lp, &e)) { set_err(err, err_len, e); return 1; }
  if (caffe::LayerRegistry<double>::Registry().count(lp.type()) == 0) {
    set_err(err, err_len, "no Layer<double> registered for type " + lp.type());
    return 2;
  }
  std::shared_ptr<caffe::Layer<double> > layer = caffe::LayerRegistry<double>::CreateLayer(lp);
  std::vector<std::unique_ptr<caffe::Blob<double> > > bots;
  std::vector<caffe::Blob<double>*> bottom, top;
  int at = 0;
  for (int b = 0; b < nbottom; ++b) {
    std::vector<int> shape(bottom_dims + at, bottom_dims + at + bottom_axes[b]);
    at += bottom_axes[b];
    bots.emplace_back(new caffe::Blob<double>(shape));
    std::memcpy(bots.back()->mutable_cpu_data(), bottom_data[b], sizeof(double) * bots.back()->count());
    bottom.push_back(bots.back().get());
  }
  std::vector<std::unique_ptr<caffe::Blob<double> > > tops;
  for (int t = 0; t < std::max(1, lp.top_size()); ++t) {
    tops.emplace_back(new caffe::Blob<double>());
    top.push_back(tops.back().get());
  }
  caffe::Blob<double>& top0 = *tops[0];
  layer->SetUp(bottom, top);
  if ((int)layer->blobs().size() != nparam && nparam != 0) { set_err(err, err_len, "parameter blob count mismatch"); return 3; }
  for (int i = 0; i < nparam; ++i)
    if (param_data && param_data[i])
      std::memcpy(layer->blobs()[i]->mutable_cpu_data(), param_data[i], sizeof(double) * layer->blobs()[i]->count());
  layer->Forward(bottom, top);
  if (top0.count() > top_capacity) { set_err(err, err_len, "top buffer too small"); return 4; }
  std::memcpy(top_out, top0.cpu_data(), sizeof(double) * top0.count());
  *top_axes_out = top0.num_axes();
  for (int a = 0; a < top0.num_axes() && a < 8; ++a) top_dims_out[a] = top0.shape(a);
  if (top_diff) std::memcpy(top0.mutable_cpu_diff(), top_diff, sizeof(double) * top0.count());
  else top0.mutable_cpu_diff()[0] = 1.0;                        // a loss layer's loss_weight
  std::vector<bool> pd(nbottom);
  for (int b = 0; b < nbottom; ++b) pd[b] = propagate_down ? propagate_down[b] != 0 : true;
  for (int i = 0; i < nparam; ++i)                                // start the parameter diffs from the caller's values
    if (param_diff_out && param_diff_out[i])
      std::memcpy(layer->blobs()[i]->mutable_cpu_diff(), param_diff_out[i], sizeof(double) * layer->blobs()[i]->count());
  layer->Backward(top, pd, bottom);
  for (int b = 0; b < nbottom; ++b)
    if (bottom_diff_out && bottom_diff_out[b])
      std::memcpy(bottom_diff_out[b], bottom[b]->cpu_diff(), sizeof(double) * bottom[b]->count());
  for (int i = 0; i < nparam; ++i)
    if (param_diff_out && param_diff_out[i])
      std::memcpy(param_diff_out[i], layer->blobs()[i]->cpu_diff(), sizeof(double) * layer->blobs()[i]->count());
  return 0;
}

}  // extern "C"
