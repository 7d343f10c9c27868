// csrc/prototxt_reader.cpp -- the subset of protobuf's text format that the net files hold: a lexer, a
// recursive-descent parser that fills the parameter structs of caffe_api.hpp, and the two entry points
// ReadNetParameterFromText / ReadLayerParameterFromText.  Host code only: nothing here touches the device or
// the C ABI.
#include <cctype>
#include <cstdlib>

#include "caffe_api.hpp"

namespace caffe {

namespace {
struct Tok {
  enum Kind { END, IDENT, STRING, NUMBER, LBRACE, RBRACE, COLON } kind;
  string text;
};
class Lexer {
 public:
  explicit Lexer(const string& s) : s_(s) {}
  bool next(Tok* t, string* err) {
    while (i_ < s_.size()) {
      const char c = s_[i_];
      if (std::isspace((unsigned char)c) || c == ',' || c == ';') { ++i_; continue; }
      if (c == '#') { while (i_ < s_.size() && s_[i_] != '\n') ++i_; continue; }
      break;
    }
    if (i_ >= s_.size()) { t->kind = Tok::END; return true; }
    const char c = s_[i_];
    if (c == '{' || c == '<') { ++i_; t->kind = Tok::LBRACE; return true; }
    if (c == '}' || c == '>') { ++i_; t->kind = Tok::RBRACE; return true; }
    if (c == ':') { ++i_; t->kind = Tok::COLON; return true; }
    if (c == '"' || c == '\'') {
      const char q = c;
      size_t j = ++i_;
      string out;
      while (j < s_.size() && s_[j] != q) {
        if (s_[j] == '\\' && j + 1 < s_.size()) ++j;
        out += s_[j++];
      }
      if (j >= s_.size()) { *err = "unterminated string"; return false; }
      i_ = j + 1;
      t->kind = Tok::STRING; t->text = out;
      return true;
    }
    if (std::isalpha((unsigned char)c) || c == '_') {
      size_t j = i_;
      while (j < s_.size() && (std::isalnum((unsigned char)s_[j]) || s_[j] == '_')) ++j;
      t->kind = Tok::IDENT; t->text = s_.substr(i_, j - i_); i_ = j;
      return true;
    }
    if (std::isdigit((unsigned char)c) || c == '-' || c == '+' || c == '.') {
      size_t j = i_ + 1;
      while (j < s_.size() && (std::isalnum((unsigned char)s_[j]) || s_[j] == '.' || s_[j] == '-' || s_[j] == '+')) ++j;
      t->kind = Tok::NUMBER; t->text = s_.substr(i_, j - i_); i_ = j;
      return true;
    }
    *err = string("unexpected character '") + c + "'";
    return false;
  }
 private:
  const string& s_;
  size_t i_ = 0;
};

class Parser {
 public:
  explicit Parser(const string& s) : lex_(s) {}
  bool fail(const string& m) { if (err_.empty()) err_ = m; return false; }
  const string& err() const { return err_; }
  bool advance() { return lex_.next(&cur_, &err_); }
  Tok cur_;

  // after a field name: scalar value
  bool scalar(Tok* v) {
    if (cur_.kind != Tok::COLON) return fail("expected ':'");
    if (!advance()) return false;
    if (cur_.kind != Tok::STRING && cur_.kind != Tok::NUMBER && cur_.kind != Tok::IDENT) return fail("expected a value");
    *v = cur_;
    return advance();
  }
  bool as_float(const Tok& t, float* f) {
    char* end = nullptr;
    *f = std::strtof(t.text.c_str(), &end);
    if (t.kind != Tok::NUMBER || end == t.text.c_str()) return fail("expected a number, got '" + t.text + "'");
    return true;
  }
  bool as_int(const Tok& t, int* i) {
    char* end = nullptr;
    const long v = std::strtol(t.text.c_str(), &end, 0);
    if (t.kind != Tok::NUMBER || *end != '\0') return fail("expected an integer, got '" + t.text + "'");
    *i = (int)v;
    return true;
  }
  bool as_bool(const Tok& t, bool* b) {
    if (t.text == "true" || t.text == "1") { *b = true; return true; }
    if (t.text == "false" || t.text == "0") { *b = false; return true; }
    return fail("expected a bool, got '" + t.text + "'");
  }
  // after a field name: `{ ... }` or `: { ... }`, body handled by f(field_name)
  template <typename F>
  bool message(F f) {
    if (cur_.kind == Tok::COLON && !advance()) return false;
    if (cur_.kind != Tok::LBRACE) return fail("expected '{'");
    if (!advance()) return false;
    while (cur_.kind == Tok::IDENT) {
      const string name = cur_.text;
      if (!advance()) return false;
      if (!f(name)) return fail("unknown or malformed field '" + name + "'");
    }
    if (cur_.kind != Tok::RBRACE) return fail("expected '}'");
    return advance();
  }
  bool skip_message() { return message([&](const string&) { return skip_value(); }); }
  bool skip_value() {
    if (cur_.kind == Tok::LBRACE) return skip_message();
    if (cur_.kind != Tok::COLON) return fail("expected ':' or '{'");
    if (!advance()) return false;
    if (cur_.kind == Tok::LBRACE) return skip_message();
    return advance();
  }
  bool filler(FillerParameter* fp) {
    return message([&](const string& n) {
      Tok v;
      if (!scalar(&v)) return false;
      if (n == "type") { fp->type_ = v.text; return true; }
      if (n == "value") return as_float(v, &fp->value_);
      if (n == "min") return as_float(v, &fp->min_);
      if (n == "max") return as_float(v, &fp->max_);
      if (n == "mean") return as_float(v, &fp->mean_);
      if (n == "std") return as_float(v, &fp->std_);
      if (n == "sparse" || n == "variance_norm") return true;
      return false;
    });
  }
  bool layer_field(const string& n, LayerParameter* lp) {
    Tok v;
    if (n == "name") { if (!scalar(&v)) return false; lp->name_ = v.text; return true; }
    if (n == "type") { if (!scalar(&v)) return false; lp->type_ = v.text; return true; }
    if (n == "bottom") { if (!scalar(&v)) return false; lp->bottom_.push_back(v.text); return true; }
    if (n == "top") { if (!scalar(&v)) return false; lp->top_.push_back(v.text); return true; }
    if (n == "loss_weight") { float f; if (!scalar(&v) || !as_float(v, &f)) return false; lp->loss_weight_.push_back(f); return true; }
    if (n == "propagate_down") { return scalar(&v); }
    if (n == "phase") { if (!scalar(&v)) return false; lp->phase_ = (v.text == "TEST" || v.text == "1") ? 1 : 0; return true; }
    if (n == "include" || n == "exclude") {
      vector<int>* dst = n == "include" ? &lp->include_phase_ : &lp->exclude_phase_;
      bool saw_phase = false;
      if (!message([&](const string& m) {
            if (m == "phase") {
              Tok w;
              if (!scalar(&w)) return false;
              dst->push_back((w.text == "TEST" || w.text == "1") ? 1 : 0);
              saw_phase = true;
              return true;
            }
            return skip_value();                      // min_level / max_level / stage / not_stage: not interpreted
          })) return false;
      if (!saw_phase) dst->push_back(-1);              // a rule without a phase matches every phase
      return true;
    }
    if (n == "param") {
      ParamSpec ps;
      if (!message([&](const string& m) {
            Tok w;
            if (!scalar(&w)) return false;
            if (m == "name") { ps.name = w.text; return true; }
            if (m == "lr_mult") return as_float(w, &ps.lr_mult);
            if (m == "decay_mult") return as_float(w, &ps.decay_mult);
            if (m == "share_mode") return true;
            return false;
          })) return false;
      lp->param_.push_back(ps);
      return true;
    }
    if (n == "sim_cross_param") {
      SimCrossParameter* p = &lp->sim_cross_param_;
      return message([&](const string& m) {
        if (m == "weight_filler") return filler(&p->weight_filler_);
        if (m == "bias_filler") return filler(&p->bias_filler_);
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "dist_mode") return as_int(w, &p->dist_mode_);
        if (m == "mesure_count") return as_int(w, &p->mesure_count_);
        if (m == "bias_term") return as_bool(w, &p->bias_term_);
        return false;
      });
    }
    if (n == "sim_matrix_param") {
      return message([&](const string& m) {
        if (m == "weight_filler") return filler(&lp->sim_matrix_param_.weight_filler_);
        return false;
      });
    }
    if (n == "embed_param") {
      EmbedParameter* p = &lp->embed_param_;
      return message([&](const string& m) {
        if (m == "weight_filler") return filler(&p->weight_filler_);
        if (m == "bias_filler") return filler(&p->bias_filler_);
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "num_output") return as_int(w, &p->num_output_);
        if (m == "input_dim") return as_int(w, &p->input_dim_);
        if (m == "bias_term") return as_bool(w, &p->bias_term_);
        if (m == "weight_source") { p->weight_source_ = w.text; return true; }
        return false;
      });
    }
    if (n == "hdf5_data_param") {
      HDF5DataParameter* p = &lp->hdf5_data_param_;
      return message([&](const string& m) {
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "source") { p->source_ = w.text; return true; }
        if (m == "batch_size") return as_int(w, &p->batch_size_);
        if (m == "shuffle") return as_bool(w, &p->shuffle_);
        return false;
      });
    }
    if (n == "transform_param") { lp->has_transform_param_ = true; return skip_value(); }
    if (n == "map_param" || n == "mrr_param") {
      int* fa = n == "map_param" ? &lp->map_param_.fixed_axis_ : &lp->mrr_param_.fixed_axis_;
      return message([&](const string& m) {
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "fixed_axis") return as_int(w, fa);
        return false;
      });
    }
    if (n == "auc_param") {
      AUCParameter* p = &lp->auc_param_;
      return message([&](const string& m) {
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "fixed_axis") return as_int(w, &p->fixed_axis_);
        if (m == "axis") return as_int(w, &p->axis_);
        if (m == "ignore_label") { p->has_ignore_label_ = true; return as_int(w, &p->ignore_label_); }
        return false;
      });
    }
    if (n == "pair_rank_loss_param") {
      return message([&](const string& m) {
        Tok w;
        if (!scalar(&w)) return false;
        if (m == "margin") return as_float(w, &lp->pair_rank_loss_param_.margin_);
        return false;
      });
    }
    // parameter messages of layer types this library does not implement (whole-net files only)
    if (tolerant_ && n.size() > 6 && n.compare(n.size() - 6, 6, "_param") == 0) {
      lp->skipped_fields_.push_back(n);
      return skip_value();
    }
    if (tolerant_ && (n == "blobs" || n == "blobs_lr" || n == "weight_decay")) return skip_value();   // V1 leftovers
    return false;
  }
  bool tolerant_ = false;
 private:
  Lexer lex_;
  string err_;
};
}  // namespace

bool ReadNetParameterFromText(const string& text, NetParameter* out, string* err) {
  Parser p(text);
  p.tolerant_ = true;
  *out = NetParameter();
  bool ok = p.advance();
  while (ok && p.cur_.kind == Tok::IDENT) {
    const string name = p.cur_.text;
    ok = p.advance();
    if (!ok) break;
    Tok v;
    if (name == "layer" || name == "layers") {
      LayerParameter lp;
      ok = p.message([&](const string& n) { return p.layer_field(n, &lp); });
      if (ok && lp.type_.empty()) ok = p.fail("layer '" + lp.name_ + "' has no type");
      if (ok) out->layer_.push_back(lp);
    } else if (name == "name") {
      ok = p.scalar(&v);
      if (ok) out->name_ = v.text;
    } else if (name == "input") {
      ok = p.scalar(&v);
      if (ok) out->input_.push_back(v.text);
    } else if (name == "input_shape") {
      vector<int> shape;
      ok = p.message([&](const string& m) {
        Tok w;
        int d;
        if (m != "dim" || !p.scalar(&w) || !p.as_int(w, &d)) return false;
        shape.push_back(d);
        return true;
      });
      if (ok) out->input_shape_.push_back(shape);
    } else if (name == "input_dim") {
      int d;
      ok = p.scalar(&v) && p.as_int(v, &d);
      if (ok) {
        if (out->input_shape_.empty() || out->input_shape_.back().size() == 4) out->input_shape_.push_back(vector<int>());
        out->input_shape_.back().push_back(d);
      }
    } else if (name == "force_backward") {
      ok = p.scalar(&v) && p.as_bool(v, &out->force_backward_);
    } else if (name == "state" || name == "debug_info") {
      ok = p.skip_value();
    } else {
      ok = p.fail("unknown net field '" + name + "'");
    }
  }
  if (ok && p.cur_.kind != Tok::END) ok = p.fail("trailing input after the net");
  if (!ok && err) *err = p.err().empty() ? "parse error" : p.err();
  return ok;
}

bool ReadLayerParameterFromText(const string& text, LayerParameter* out, string* err) {
  Parser p(text);
  *out = LayerParameter();
  bool ok = p.advance();
  if (ok && p.cur_.kind == Tok::IDENT && (p.cur_.text == "layer" || p.cur_.text == "layers")) {
    ok = p.advance() && p.message([&](const string& n) { return p.layer_field(n, out); });
  } else if (ok) {
    while (ok && p.cur_.kind == Tok::IDENT) {
      const string name = p.cur_.text;
      ok = p.advance() && (p.layer_field(name, out) || p.fail("unknown or malformed field '" + name + "'"));
    }
  }
  if (ok && p.cur_.kind != Tok::END) ok = p.fail("trailing input after the layer message");
  if (ok && out->type_.empty()) ok = p.fail("layer has no type");
  if (!ok && err) *err = p.err().empty() ? "parse error" : p.err();
  return ok;
}

}  // namespace caffe
