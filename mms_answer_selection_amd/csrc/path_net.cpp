// csrc/path_net.cpp -- PathNet: name wiring, phase filter, parameter sharing, split insertion, Embed pairing and
// embed-scoring fusion for the layers of a net file.
//
// What Net::Init / ForwardFromTo / BackwardFromTo (src/caffe/net.cpp:40-270, 535-591) do for the layers of a
// generated net file that THIS library implements: phase filtering (net.cpp:272-330 StateMeetsRule, phase
// only), blobs wired by name with in-place tops sharing their bottom's blob (net.cpp:385-420), parameters
// shared by `param { name }` (net.cpp:450-530 AppendParam), layers run in file order.  Layers of other types
// are listed and skipped; a blob only they produce is an input the host fills before SetUp.
#include "path_net.hpp"

#include <algorithm>

namespace caffe {

PathNet::PathNet(const NetParameter& np, int phase) : name_(np.name_), phase_(phase) {
  for (size_t i = 0; i < np.input_.size(); ++i) {
    Blob<float>* b = blob(np.input_[i], true);
    if (i < np.input_shape_.size() && !np.input_shape_[i].empty()) b->Reshape(np.input_shape_[i]);
  }
  for (const LayerParameter& lp : np.layer_) {
    if (!included(lp)) continue;
    PathNetLayer L;
    L.param = lp;
    for (const string& bn : lp.bottom_) { L.bottom.push_back(blob(bn, true)); L.bottom_names.push_back(bn); }
    for (const string& tn : lp.top_) { L.top.push_back(blob(tn, true)); L.top_names.push_back(tn); }   // same name = same blob (in place)
    if (LayerRegistry<float>::Registry().count(lp.type())) L.layer = LayerRegistry<float>::CreateLayer(lp);
    layers_.push_back(L);
  }
}
// SetUp of every supported layer whose bottoms have a shape, in file order; returns the number that can run
int PathNet::SetUp() {
  int n = 0;
  for (PathNetLayer& L : layers_) {
    L.runnable = false;
    L.why_not.clear();
    if (!L.layer) { L.why_not = "layer type '" + L.param.type() + "' is not implemented by this library"; continue; }
    for (size_t b = 0; b < L.bottom.size(); ++b)
      if (L.bottom[b]->count() == 0 && L.why_not.empty()) L.why_not = "bottom '" + L.bottom_names[b] + "' has no shape (fill it before SetUp)";
    if (!L.why_not.empty()) continue;
    // AutoTopBlobs (layer.hpp:67-74 / net.cpp:150-166): anonymous tops up to the layer's need
    if (L.layer->AutoTopBlobs()) {
      const int need = std::max(L.layer->MinTopBlobs(), L.layer->ExactNumTopBlobs());
      while ((int)L.top.size() < need) {
        owned_.emplace_back(new Blob<float>());
        L.top.push_back(owned_.back().get());
        L.top_names.push_back("(automatic)");
      }
    }
    L.layer->SetUp(L.bottom, L.top);
    share_params(L);
    L.runnable = true;
    ++n;
  }
  insert_splits();
  plan_fusion();
  return n;
}
// "fuse_embed_scoring" (forward-only nets: evaluation, do_trec_qa_clean.py:617-650): a SimCross layer whose two
// bottoms come from Embed layers that read ONE table (shared by parameter name, as network_v4's do) and feed
// nothing else is run straight from the word ids -- the (N, W, D) blobs are never written.
bool PathNet::SetOption(const string& key, int value) {
  if (key == "pair_embed") { pair_embed_ = value != 0; return true; }
  if (key != "fuse_embed_scoring") return false;
  fuse_embed_ = value != 0;
  plan_fusion();
  return true;
}
float PathNet::Forward() {
  float loss = 0;
  pair_done_.clear();
  for (auto& kv : pair_state_) kv.second.ran = false;
  for (size_t i = 0; i < layers_.size(); ++i) {
    PathNetLayer& L = layers_[i];
    if (!L.runnable || skipped_.count(i)) continue;
    for (Split& sp : splits_)                                    // SplitLayer::Reshape: the tops share the bottom's data
      for (size_t c = 0; c < sp.consumers.size(); ++c)
        if (sp.consumers[c].first == i) { sp.alias[c]->ReshapeLike(*sp.orig); sp.alias[c]->ShareData(*sp.orig); }
    if (pair_done_.count(i)) continue;                 // the later Embed of a pair: written with the earlier one
    auto ep = embed_pairs_.find(i);
    if (ep != embed_pairs_.end() && pair_embed_) {
      // two Embed layers over one table: both gathers in one launch, the backward's inverted index built beside them
      PathNetLayer& Lj = layers_[ep->second];
      EmbedPairState& st = pair_state_[i];
      if (EmbedPairForward(*Lj.layer, *L.layer, Lj.bottom, Lj.top, L.bottom, L.top, &st.index_ws, &st.indexed)) {
        st.ran = true;
        pair_done_.insert(ep->second);
        continue;
      }
      st.ran = false;
    }
    auto f = fused_.find(i);
    if (f != fused_.end()) {
      PathNetLayer& Eq = layers_[f->second.first];
      PathNetLayer& Ea = layers_[f->second.second];
      auto& eb = Eq.layer->blobs();
      if (SimCrossForwardFromWordIds(*L.layer, *Eq.bottom[0], *Ea.bottom[0], *eb[0], eb.size() > 1 ? eb[1].get() : nullptr,
                                     L.bottom, L.top))
        continue;
      Eq.layer->Forward(Eq.bottom, Eq.top);            // no fused kernel for this geometry: the usual three
      Ea.layer->Forward(Ea.bottom, Ea.top);
    }
    loss += L.layer->Forward(L.bottom, L.top);
  }
  ran_fused_ = !fused_.empty();
  return loss;
}
void PathNet::Backward() {
  CHECK(!ran_fused_) << "Backward on a net whose last Forward scored from word ids (fuse_embed_scoring): the "
                        "Embed tops were never written";
  for (size_t i = layers_.size(); i-- > 0;) {
    PathNetLayer& L = layers_[i];
    for (Split& sp : splits_) if (sp.producer == (int)i) split_backward(sp);     // every consumer has run by now
    if (!L.runnable) continue;
    if (!has_backward(L)) continue;
    if (pair_done_.count(i)) continue;                 // the later Embed of a pair: its Backward runs with the earlier one's,
    auto ep = embed_pairs_.find(i);                    // when every consumer of BOTH tops has run
    if (ep != embed_pairs_.end() && pair_state_[i].ran) {
      PathNetLayer& Lj = layers_[ep->second];
      EmbedPairBackward(*Lj.layer, *L.layer, Lj.bottom, Lj.top, L.bottom, L.top, &pair_state_[i].index_ws,
                        pair_state_[i].indexed);
      continue;
    }
    vector<bool> pd(L.bottom.size(), true);
    for (size_t b = 0; b < L.bottom.size(); ++b) pd[b] = propagates(L, b);
    L.layer->Backward(L.top, pd, L.bottom);
  }
  for (Split& sp : splits_) if (sp.producer < 0) split_backward(sp);             // net inputs
}
bool PathNet::included(const LayerParameter& lp) const {
  // net.cpp:272-296 FilterNet: no include rules = included unless an exclude rule matches; with include
  // rules, included iff one matches
  auto matches = [&](int rule) { return rule < 0 || rule == phase_; };
  if (lp.include_phase_.empty()) {
    for (int r : lp.exclude_phase_) if (matches(r)) return false;
    return true;
  }
  for (int r : lp.include_phase_) if (matches(r)) return true;
  return false;
}
Blob<float>* PathNet::blob(const string& n, bool create) {
  auto it = blobs_.find(n);
  if (it != blobs_.end()) return it->second;
  if (!create) return nullptr;
  owned_.emplace_back(new Blob<float>());
  blobs_[n] = owned_.back().get();
  blob_order_.push_back(n);
  return owned_.back().get();
}
void PathNet::share_params(PathNetLayer& L) {
  const string t = L.param.type();
  if (t == "HDF5Data") for (const string& tn : L.top_names) produced_by_data_.insert(tn);
  auto& blobs = L.layer->blobs();
  for (size_t i = 0; i < L.param.param_.size() && i < blobs.size(); ++i) {
    const string& pn = L.param.param_[i].name;
    if (pn.empty()) continue;
    auto it = shared_params_.find(pn);
    if (it == shared_params_.end()) { shared_params_[pn] = blobs[i]; continue; }
    CHECK_EQ(it->second->count(), blobs[i]->count()) << "Shared parameter '" << pn << "' has mismatched sizes";
    blobs[i] = it->second;                                         // ShareData + ShareDiff with the owner
  }
}
bool PathNet::has_backward(const PathNetLayer& L) {
  const string t = L.param.type();
  return !(t == "HDF5Data" || t == "MAP" || t == "MRR" || t == "AUC" || t == "RankAccuracy");
}
bool PathNet::propagates(const PathNetLayer& L, size_t b) const {
  const string t = L.param.type();
  if (t == "Embed") return false;                                // indices (embed_layer.cpp:156)
  if (t == "PairRankLoss" && b == 2) return false;               // labels (pair_rank_loss_layer.cpp:58-61)
  if (produced_by_data_.count(L.bottom_names[b])) return false;
  return true;
}
// What Net::Init's InsertSplits does (src/caffe/util/insert_splits.cpp:13-88, net.cpp:57): a blob that feeds more
// than one layer gets a Split layer, whose tops share its data and own their diffs, and whose Backward SUMS those
// diffs into the blob's (split_layer.cpp:38-57).  Without it each consumer's Backward overwrites the blob's diff
// and the last one wins.  Here: every consumer that propagates down into such a blob reads it through a blob of
// its own (data shared, diff private) and the sum is taken -- in consumer order, like the reference -- right
// before the producing layer's Backward.  This also gives SimMatrix's bottom[1] a diff no sibling touches: its
// Forward parks Q.W there (sim_matrix_layer.cpp:58).
void PathNet::insert_splits() {
  if (!splits_.empty()) return;                                  // SetUp may run again; the wiring is done once
  for (const string& name : blob_order_) {
    Blob<float>* b = blobs_[name];
    Split sp;
    sp.orig = b;
    sp.producer = -1;
    bool in_place = false;
    for (size_t i = 0; i < layers_.size(); ++i) {
      const PathNetLayer& L = layers_[i];
      for (size_t k = 0; k < L.top.size(); ++k) if (L.top[k] == b) sp.producer = (int)i;
      if (!L.runnable || !has_backward(L)) continue;
      for (size_t k = 0; k < L.bottom.size(); ++k) {
        if (L.bottom[k] != b || !propagates(L, k)) continue;
        sp.consumers.emplace_back(i, k);
        for (Blob<float>* t : L.top) if (t == b) in_place = true;
      }
    }
    if (sp.consumers.size() < 2 || in_place || b->count() == 0) continue;
    for (auto& c : sp.consumers) {
      owned_.emplace_back(new Blob<float>());
      Blob<float>* a = owned_.back().get();
      a->ReshapeLike(*b);
      a->ShareData(*b);
      sp.alias.push_back(a);
      layers_[c.first].bottom[c.second] = a;
    }
    splits_.push_back(sp);
  }
}
void PathNet::split_backward(Split& sp) {
  vector<const float*> tops;
  for (Blob<float>* a : sp.alias) tops.push_back(a->gpu_diff());
  mms_check(mms_split_backward_f32(sp.orig->count(), (int)tops.size(), tops.data(), sp.orig->mutable_gpu_diff(), nullptr),
            "mms_split_backward_f32");
}
// Pairs of Embed layers that read ONE table (and bias) by parameter name, the later one's word ids available when
// the earlier one runs: forward as one launch, backward as one pass (EmbedPairForward / EmbedPairBackward; option
// "pair_embed", on by default -- the results are the two layers' bits, so nothing observable changes but the time).
void PathNet::plan_embed_pairs() {
  embed_pairs_.clear();
  pair_state_.clear();
  std::set<size_t> taken;
  for (size_t i = 0; i < layers_.size(); ++i) {
    PathNetLayer& Li = layers_[i];
    if (!Li.runnable || Li.param.type() != "Embed" || taken.count(i) || Li.bottom.size() != 1 || Li.top.size() != 1) continue;
    for (size_t j = i + 1; j < layers_.size(); ++j) {
      PathNetLayer& Lj = layers_[j];
      if (!Lj.runnable || Lj.param.type() != "Embed" || taken.count(j) || Lj.bottom.size() != 1 || Lj.top.size() != 1) continue;
      auto &bi = Li.layer->blobs(), &bj = Lj.layer->blobs();
      if (bi.empty() || bi.size() != bj.size() || bi[0].get() != bj[0].get()) continue;
      if (bi.size() > 1 && bi[1].get() != bj[1].get()) continue;
      bool ready = true;                               // the later layer's ids must exist when the earlier layer runs
      for (size_t k = i; k < layers_.size() && ready; ++k)
        for (Blob<float>* t : layers_[k].top) if (t == Lj.bottom[0]) ready = false;
      if (!ready) continue;
      embed_pairs_[i] = j;
      pair_state_[i];
      taken.insert(i); taken.insert(j);
      break;
    }
  }
}
void PathNet::plan_fusion() {
  plan_embed_pairs();
  fused_.clear();
  skipped_.clear();
  if (!fuse_embed_) return;
  auto producer = [&](size_t before, Blob<float>* b) -> int {
    for (size_t i = before; i-- > 0;)
      for (Blob<float>* t : layers_[i].top) if (t == b) return (int)i;
    return -1;
  };
  auto consumers = [&](Blob<float>* b) {
    int c = 0;
    for (const PathNetLayer& L : layers_) for (Blob<float>* x : L.bottom) if (x == b) ++c;
    return c;
  };
  for (size_t i = 0; i < layers_.size(); ++i) {
    PathNetLayer& L = layers_[i];
    if (!L.runnable || L.param.type() != "SimCross" || L.bottom.size() != 2) continue;
    const int eq = producer(i, L.bottom[0]), ea = producer(i, L.bottom[1]);
    if (eq < 0 || ea < 0 || eq == ea) continue;
    const PathNetLayer &Eq = layers_[eq], &Ea = layers_[ea];
    if (!Eq.runnable || !Ea.runnable || Eq.param.type() != "Embed" || Ea.param.type() != "Embed") continue;
    if (Eq.top.size() != 1 || Ea.top.size() != 1 || Eq.bottom.size() != 1 || Ea.bottom.size() != 1) continue;
    if (consumers(L.bottom[0]) != 1 || consumers(L.bottom[1]) != 1) continue;        // someone else reads q or a
    auto &bq = Eq.layer->blobs(), &ba = Ea.layer->blobs();
    if (bq.empty() || bq.size() != ba.size() || bq[0].get() != ba[0].get()) continue;  // two tables
    if (bq.size() > 1 && bq[1].get() != ba[1].get()) continue;                          // two biases
    fused_[i] = std::make_pair((size_t)eq, (size_t)ea);
    skipped_.insert((size_t)eq);
    skipped_.insert((size_t)ea);
  }
}

}  // namespace caffe
