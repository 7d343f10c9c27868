// csrc/path_net.hpp -- PathNet, the layers of a whole net file that this library implements, wired and run in
// file order (path_net.cpp), and the three calls by which it reaches past the Layer interface into SimCross and
// Embed.  Those are defined beside their classes (layers_scoring.cpp, layers_embed.cpp), so that no layer class
// has to be visible here.
#ifndef MMS_PATH_NET_HPP_
#define MMS_PATH_NET_HPP_

#include <map>
#include <set>

#include "layer_abi.hpp"

namespace caffe {

// SimCrossLayer<float>::ForwardFromWordIds of `sim`, which must be a SimCross layer.
bool SimCrossForwardFromWordIds(Layer<float>& sim, const Blob<float>& ids_q, const Blob<float>& ids_a,
                                const Blob<float>& table, const Blob<float>* embed_bias,
                                const vector<Blob<float>*>& bottom, const vector<Blob<float>*>& top);
// Two Embed layers over one table, run as a pair; both must be Embed layers (layers_embed.cpp says what bl .. te are).
bool EmbedPairForward(Layer<float>& later, Layer<float>& earlier, const vector<Blob<float>*>& bl,
                      const vector<Blob<float>*>& tl, const vector<Blob<float>*>& be, const vector<Blob<float>*>& te,
                      Workspace<float>* index_ws, bool* indexed);
void EmbedPairBackward(Layer<float>& later, Layer<float>& earlier, const vector<Blob<float>*>& bl,
                       const vector<Blob<float>*>& tl, const vector<Blob<float>*>& be, const vector<Blob<float>*>& te,
                       Workspace<float>* index_ws, bool indexed);

struct PathNetLayer {
  LayerParameter param;
  shared_ptr<Layer<float> > layer;        // null: the type is outside this library
  vector<Blob<float>*> bottom, top;
  vector<string> bottom_names, top_names;
  bool runnable = false;
  string why_not;                          // for a supported layer that cannot run: what is missing
};

class PathNet {
 public:
  PathNet(const NetParameter& np, int phase);
  int SetUp();
  // "pair_embed", "fuse_embed_scoring" (path_net.cpp); false for any other key
  bool SetOption(const string& key, int value);
  int num_fused() const { return (int)fused_.size(); }
  float Forward();
  void Backward();
  int num_splits() const { return (int)splits_.size(); }
  Blob<float>* find_blob(const string& n) { auto it = blobs_.find(n); return it == blobs_.end() ? nullptr : it->second; }
  vector<PathNetLayer>& layers() { return layers_; }
  const vector<string>& blob_names() const { return blob_order_; }
  const string& name() const { return name_; }

 private:
  struct Split {
    Blob<float>* orig;
    int producer;                                                  // layer index, -1: a net input
    vector<std::pair<size_t, size_t> > consumers;                  // (layer, bottom index), file order
    vector<Blob<float>*> alias;
  };
  struct EmbedPairState { Workspace<float> index_ws; bool indexed = false, ran = false; };

  bool included(const LayerParameter& lp) const;
  Blob<float>* blob(const string& n, bool create);
  void share_params(PathNetLayer& L);
  static bool has_backward(const PathNetLayer& L);
  bool propagates(const PathNetLayer& L, size_t b) const;
  void insert_splits();
  void split_backward(Split& sp);
  void plan_embed_pairs();
  void plan_fusion();

  string name_;
  int phase_;
  bool fuse_embed_ = false, ran_fused_ = false, pair_embed_ = true;
  std::map<size_t, size_t> embed_pairs_;                 // earlier Embed layer -> the later one over the same table
  std::map<size_t, EmbedPairState> pair_state_;
  std::set<size_t> pair_done_;                           // later layers of pairs that ran as pairs in this Forward
  std::map<size_t, std::pair<size_t, size_t> > fused_;   // SimCross layer -> its two Embed producers
  std::set<size_t> skipped_;
  vector<PathNetLayer> layers_;
  std::map<string, Blob<float>*> blobs_;
  vector<string> blob_order_;
  vector<std::unique_ptr<Blob<float> > > owned_;
  std::map<string, shared_ptr<Blob<float> > > shared_params_;
  std::set<string> produced_by_data_;
  vector<Split> splits_;
};

}  // namespace caffe
#endif  // MMS_PATH_NET_HPP_
