// include/klstm_nnet.hpp -- minimal nnet1 container around the hot path: the `Nnet` the reference trainer
// drives (google/nnet/nnet-nnet.h:36-150, only the declaration is vendored), the components that appear
// in the reference topologies (google/nnet.proto, standard/nnet.proto, README.md:24-45), the masked
// cross-entropy (google/nnet/nnet-loss.cc:76-164, 293-307) and a workalike of the training loop of
// google/nnetbin/bd-nnet-train-lstm-streams.cc (:143-304) on in-memory utterances.
// Header-only C++ over the C-ABI (klstm.h); no HIP or Kaldi headers needed.
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>

#include "klstm_component.hpp"
#include "klstm_trainer.hpp"

namespace klstm_kaldi {

inline void KCheck(klstm_status st) { if (st != KLSTM_OK) KLSTM_ERR("klstm: " << klstm_last_error() << " (status " << (int)st << ")"); }

// CuMatrix stand-in: owning, pitched device matrix (cu-matrix.cc:51-84: rows are pitched; here the stride is the
// column count rounded up to 64 floats = 256 B).
class DeviceMatrix {
 public:
  DeviceMatrix() : data_(nullptr), rows_(0), cols_(0), stride_(0), cap_(0) {}
  ~DeviceMatrix() { if (data_) klstm_free(data_); }
  DeviceMatrix(const DeviceMatrix &) = delete;
  DeviceMatrix &operator=(const DeviceMatrix &) = delete;
  void Resize(int32 rows, int32 cols, bool set_zero = true) {     // no realloc when the shape is unchanged (cu-matrix.cc:56-59)
    const int32 stride = (cols + 63) / 64 * 64;
    const size_t need = (size_t)rows * stride;
    if (need > cap_) {
      if (data_) KCheck(klstm_free(data_));
      void *p = nullptr;
      KCheck(klstm_malloc(&p, need * sizeof(BaseFloat)));
      data_ = (BaseFloat *)p; cap_ = need;
    }
    rows_ = rows; cols_ = cols; stride_ = stride;
    if (set_zero && need) KCheck(klstm_memset_zero(data_, need * sizeof(BaseFloat), nullptr));
  }
  int32 NumRows() const { return rows_; }
  int32 NumCols() const { return cols_; }
  int32 Stride() const { return stride_; }
  MatrixView View() const { return MatrixView(data_, rows_, cols_, stride_); }
  void CopyFromHost(const BaseFloat *src, int32 rows, int32 cols) {          // CuMatrix(const Matrix&), cu-matrix.cc:287-311
    Resize(rows, cols, false);
    std::vector<BaseFloat> tmp((size_t)rows * stride_, 0.f);
    for (int32 r = 0; r < rows; r++) std::memcpy(&tmp[(size_t)r * stride_], src + (size_t)r * cols, cols * sizeof(BaseFloat));
    if (!tmp.empty()) KCheck(klstm_memcpy_h2d(data_, tmp.data(), tmp.size() * sizeof(BaseFloat), nullptr));
  }
  void CopyToHost(std::vector<BaseFloat> *dst) const {
    std::vector<BaseFloat> tmp((size_t)rows_ * stride_);
    if (!tmp.empty()) KCheck(klstm_memcpy_d2h(tmp.data(), data_, tmp.size() * sizeof(BaseFloat), nullptr));
    dst->resize((size_t)rows_ * cols_);
    for (int32 r = 0; r < rows_; r++) std::memcpy(&(*dst)[(size_t)r * cols_], &tmp[(size_t)r * stride_], cols_ * sizeof(BaseFloat));
  }
 private:
  BaseFloat *data_;
  int32 rows_, cols_, stride_;
  size_t cap_;
};

// Polymorphic view of one nnet1 component (Component / UpdatableComponent, [UPSTREAM-unvendored] nnet-component.h).
class Layer {
 public:
  virtual ~Layer() {}
  virtual const char *Marker() const = 0;
  virtual int32 InputDim() const = 0;
  virtual int32 OutputDim() const = 0;
  virtual bool IsUpdatable() const { return false; }
  virtual void ReadData(std::istream &, bool) {}
  virtual void WriteData(std::ostream &, bool) const {}
  virtual void PropagateFnc(const MatrixView &in, MatrixView *out) = 0;
  virtual void BackpropagateFnc(const MatrixView &in, const MatrixView &out, const MatrixView &out_diff, MatrixView *in_diff) = 0;
  virtual void Update(const MatrixView &, const MatrixView &) {}
  virtual void SetUpdateFollows(bool) {}                     // Nnet::Backpropagate: Update comes right behind BackpropagateFnc
  virtual void SetTrainOptions(const NnetTrainOptions &) {}
  virtual void Reset(std::vector<int> &) {}                  // the overlay adds Reset to every Component (nnet-nnet.h:133-137)
  virtual void SetSeqLengths(const std::vector<int32> &) {}   // per-utterance lengths (nnet1's name; the bidirectional layer, klstm_blstm.hpp)
  virtual int32 NumParams() const { return 0; }
  virtual void GetParams(std::vector<BaseFloat> *p) const { p->clear(); }
  void Write(std::ostream &os, bool binary) const {
    WriteToken(os, binary, Marker());
    WriteBasicType(os, binary, OutputDim());
    WriteBasicType(os, binary, InputDim());
    const std::streampos before = os.tellp();
    WriteData(os, binary);
    if (!binary && os.tellp() == before) os << "\n";
  }
};

class LstmLayer : public Layer {            // LstmProjectedStreams / LstmProjected
 public:
  explicit LstmLayer(LstmProjectedStreams *c) : c_(c) {}
  const char *Marker() const override { return c_->Marker(); }
  int32 InputDim() const override { return c_->InputDim(); }
  int32 OutputDim() const override { return c_->OutputDim(); }
  bool IsUpdatable() const override { return true; }
  void ReadData(std::istream &is, bool b) override { c_->ReadData(is, b); }
  void WriteData(std::ostream &os, bool b) const override { c_->WriteData(os, b); }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override { c_->PropagateFnc(in, out); }
  void BackpropagateFnc(const MatrixView &in, const MatrixView &out, const MatrixView &od, MatrixView *id) override { c_->BackpropagateFnc(in, out, od, id); }
  void Update(const MatrixView &a, const MatrixView &b) override { c_->Update(a, b); }
  void SetUpdateFollows(bool v) override { c_->SetUpdateFollows(v); }
  void SetTrainOptions(const NnetTrainOptions &o) override { c_->SetTrainOptions(o); }
  void Reset(std::vector<int> &f) override { if (std::string(c_->Marker()) == "<LstmProjectedStreams>") c_->Reset(f); }
  int32 NumParams() const override { return c_->NumParams(); }
  void GetParams(std::vector<BaseFloat> *p) const override { c_->GetParams(p); }
  LstmProjectedStreams *Impl() { return c_.get(); }
  const LstmProjectedStreams *Impl() const { return c_.get(); }
 private:
  std::unique_ptr<LstmProjectedStreams> c_;
};

class TimeShiftLayer : public Layer {
 public:
  TimeShiftLayer(int32 i, int32 o) : c_(i, o) {}
  const char *Marker() const override { return c_.Marker(); }
  int32 InputDim() const override { return c_.InputDim(); }
  int32 OutputDim() const override { return c_.OutputDim(); }
  void ReadData(std::istream &is, bool b) override { c_.ReadData(is, b); }
  void WriteData(std::ostream &os, bool b) const override { c_.WriteData(os, b); }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override { c_.PropagateFnc(in, out); }
  void BackpropagateFnc(const MatrixView &a, const MatrixView &b, const MatrixView &c, MatrixView *d) override { c_.BackpropagateFnc(a, b, c, d); }
  int32 Shift() const { return c_.Shift(); }
 private:
  TimeShift c_;
};

class TransmitLayer : public Layer {
 public:
  TransmitLayer(int32 i, int32 o) : c_(i, o) {}
  const char *Marker() const override { return c_.Marker(); }
  int32 InputDim() const override { return c_.InputDim(); }
  int32 OutputDim() const override { return c_.OutputDim(); }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override { c_.PropagateFnc(in, out); }
  void BackpropagateFnc(const MatrixView &a, const MatrixView &b, const MatrixView &c, MatrixView *d) override { c_.BackpropagateFnc(a, b, c, d); }
 private:
  TransmitComponent c_;
};

// [UPSTREAM-unvendored nnet-affine-transform.h] AffineTransform: out = in * linearity^T + bias; model line
// "<AffineTransform> 16624 512 <LearnRateCoef> 1 <BiasLearnRateCoef> 1 <MaxNorm> 0  [ ..." (README.md:27).
class AffineLayer : public Layer {
 public:
  AffineLayer(int32 in, int32 out) : in_(in), out_(out), lr_coef_(1.f), bias_lr_coef_(1.f), max_norm_(0.f),
                                     W_(nullptr), b_(nullptr), Wc_(nullptr), bc_(nullptr) {}
  ~AffineLayer() override { klstm_free(W_); klstm_free(b_); klstm_free(Wc_); klstm_free(bc_); }
  const char *Marker() const override { return "<AffineTransform>"; }
  int32 InputDim() const override { return in_; }
  int32 OutputDim() const override { return out_; }
  bool IsUpdatable() const override { return true; }
  void ReadData(std::istream &is, bool binary) override {
    while ('<' == Peek(is, binary)) {                     // optional learning-rate tokens
      std::string tok;
      ReadToken(is, binary, &tok);
      if (tok == "<LearnRateCoef>") ReadBasicType(is, binary, &lr_coef_);
      else if (tok == "<BiasLearnRateCoef>") ReadBasicType(is, binary, &bias_lr_coef_);
      else if (tok == "<MaxNorm>") ReadBasicType(is, binary, &max_norm_);
      else KLSTM_ERR("Unknown token " << tok);
    }
    std::vector<BaseFloat> w, b;
    int32 r, c;
    ReadMatrix(is, binary, &w, &r, &c);
    ReadVector(is, binary, &b);
    if (r != out_ || c != in_ || (int32)b.size() != out_) KLSTM_ERR("AffineTransform: dimension mismatch");
    SetParams(w, b);
  }
  void WriteData(std::ostream &os, bool binary) const override {
    std::vector<BaseFloat> w, b;
    HostParams(&w, &b);
    WriteToken(os, binary, "<LearnRateCoef>"); WriteBasicType(os, binary, lr_coef_);
    WriteToken(os, binary, "<BiasLearnRateCoef>"); WriteBasicType(os, binary, bias_lr_coef_);
    WriteToken(os, binary, "<MaxNorm>"); WriteBasicType(os, binary, max_norm_);
    WriteMatrix(os, binary, w.data(), out_, in_, in_);
    WriteVector(os, binary, b.data(), out_);
  }
  // parameters keep a host shadow so model files can be read / converted without a GPU; the device copy is
  // created at the first PropagateFnc
  void SetParams(const std::vector<BaseFloat> &w, const std::vector<BaseFloat> &b) {
    KLSTM_ASSERT((int32)w.size() == out_ * in_ && (int32)b.size() == out_);
    hw_ = w; hb_ = b; host_fresh_ = true;
    if (W_) Upload();
  }
  void HostParams(std::vector<BaseFloat> *w, std::vector<BaseFloat> *b) const {
    if (W_ && !host_fresh_) {
      hw_.resize((size_t)out_ * in_); hb_.resize(out_);
      KCheck(klstm_memcpy_d2h(hw_.data(), W_, hw_.size() * sizeof(BaseFloat), nullptr));
      KCheck(klstm_memcpy_d2h(hb_.data(), b_, hb_.size() * sizeof(BaseFloat), nullptr));
      host_fresh_ = true;
    }
    *w = hw_; *b = hb_;
  }
  int32 NumParams() const override { return out_ * in_ + out_; }
  void GetParams(std::vector<BaseFloat> *p) const override {
    std::vector<BaseFloat> w, b; HostParams(&w, &b); *p = w; p->insert(p->end(), b.begin(), b.end());
  }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    Alloc();
    KCheck(klstm_affine_propagate(in.Data(), in.NumRows(), in_, in.Stride(), W_, b_, out->Data(), out_, out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(klstm_affine_backpropagate(od.Data(), od.NumRows(), out_, od.Stride(), W_, in_, id->Data(), id->Stride(), nullptr));
  }
  void Update(const MatrixView &input, const MatrixView &diff) override {
    if (opts_.l2_penalty != 0.f || opts_.l1_penalty != 0.f) KLSTM_ERR("AffineTransform: l1/l2 penalties are not implemented");
    KCheck(klstm_affine_update(input.Data(), input.Stride(), diff.Data(), diff.Stride(), input.NumRows(), in_, out_, W_, b_, Wc_, bc_,
                               opts_.learn_rate * lr_coef_, opts_.learn_rate * bias_lr_coef_, opts_.momentum, nullptr));
    host_fresh_ = false;
  }
  void SetTrainOptions(const NnetTrainOptions &o) override { opts_ = o; }
 private:
  void Alloc() {
    if (W_) return;
    void *p;
    KCheck(klstm_malloc(&p, (size_t)out_ * in_ * 4)); W_ = (BaseFloat *)p;
    KCheck(klstm_malloc(&p, (size_t)out_ * 4)); b_ = (BaseFloat *)p;
    KCheck(klstm_malloc(&p, (size_t)out_ * in_ * 4)); Wc_ = (BaseFloat *)p;
    KCheck(klstm_malloc(&p, (size_t)out_ * 4)); bc_ = (BaseFloat *)p;
    KCheck(klstm_memset_zero(Wc_, (size_t)out_ * in_ * 4, nullptr));
    KCheck(klstm_memset_zero(bc_, (size_t)out_ * 4, nullptr));
    Upload();
  }
  void Upload() {
    KLSTM_ASSERT((int32)hw_.size() == out_ * in_ && (int32)hb_.size() == out_);
    KCheck(klstm_memcpy_h2d(W_, hw_.data(), hw_.size() * sizeof(BaseFloat), nullptr));
    KCheck(klstm_memcpy_h2d(b_, hb_.data(), hb_.size() * sizeof(BaseFloat), nullptr));
  }
  int32 in_, out_;
  BaseFloat lr_coef_, bias_lr_coef_, max_norm_;
  NnetTrainOptions opts_;
  BaseFloat *W_, *b_, *Wc_, *bc_;
  mutable std::vector<BaseFloat> hw_, hb_;
  mutable bool host_fresh_ = true;
};

// [UPSTREAM-unvendored nnet-activation.h] Softmax: row softmax forward; backward passes the diff through, because
// Xent's diff (y - t) is already the derivative w.r.t. the softmax input.
class SoftmaxLayer : public Layer {
 public:
  SoftmaxLayer(int32 i, int32 o) : in_(i), out_(o) {}
  const char *Marker() const override { return "<Softmax>"; }
  int32 InputDim() const override { return in_; }
  int32 OutputDim() const override { return out_; }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    KCheck(klstm_softmax(in.Data(), in.NumRows(), in.NumCols(), in.Stride(), out->Data(), out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(klstm_time_shift(od.Data(), od.NumRows(), od.NumCols(), od.Stride(), id->Data(), id->Stride(), 0, nullptr));
  }
 private:
  int32 in_, out_;
};

class Nnet {                                  // google/nnet/nnet-nnet.h:36-150
 public:
  Nnet() {}
  int32 NumComponents() const { return (int32)layers_.size(); }
  Layer &GetComponent(int32 i) { return *layers_[i]; }
  const Layer &GetComponent(int32 i) const { return *layers_[i]; }
  int32 InputDim() const { KLSTM_ASSERT(!layers_.empty()); return layers_.front()->InputDim(); }
  int32 OutputDim() const { KLSTM_ASSERT(!layers_.empty()); return layers_.back()->OutputDim(); }
  void AppendComponent(Layer *l) {
    if (!layers_.empty() && layers_.back()->OutputDim() != l->InputDim()) KLSTM_ERR("Nnet: dimension mismatch between components");
    layers_.emplace_back(l);
  }

  void Read(std::istream &is, bool binary) {      // "<Nnet>" components "</Nnet>"
    layers_.clear();
    std::string token;
    ReadToken(is, binary, &token);
    if (token != "<Nnet>") KLSTM_ERR("Expected <Nnet>, got " << token);
    while (true) {
      ReadToken(is, binary, &token);
      if (token == "</Nnet>") break;
      int32 dim_out, dim_in;
      ReadBasicType(is, binary, &dim_out);
      ReadBasicType(is, binary, &dim_in);
      Layer *l = nullptr;
      if (token == "<LstmProjectedStreams>") l = new LstmLayer(new LstmProjectedStreams(dim_in, dim_out));
      else if (token == "<LstmProjected>") l = new LstmLayer(new LstmProjected(dim_in, dim_out));
      else if (token == "<TimeShift>") l = new TimeShiftLayer(dim_in, dim_out);
      else if (token == "<Transmit>") l = new TransmitLayer(dim_in, dim_out);
      else if (token == "<AffineTransform>") l = new AffineLayer(dim_in, dim_out);
      else if (token == "<Softmax>") l = new SoftmaxLayer(dim_in, dim_out);
      else KLSTM_ERR("Unknown component marker " << token);
      std::unique_ptr<Layer> guard(l);
      l->ReadData(is, binary);
      AppendComponent(guard.release());
    }
  }
  void Read(const std::string &file) {
    std::ifstream f(file, std::ios::binary);
    if (!f) KLSTM_ERR("cannot open " << file);
    Read(f, InitKaldiInputStream(f));
  }
  void Write(std::ostream &os, bool binary) const {
    WriteToken(os, binary, "<Nnet>");
    if (!binary) os << "\n";
    for (const auto &l : layers_) l->Write(os, binary);
    WriteToken(os, binary, "</Nnet>");
    if (!binary) os << "\n";
  }
  void Write(const std::string &file, bool binary) const {
    std::ofstream f(file, std::ios::binary);
    InitKaldiOutputStream(f, binary);
    Write(f, binary);
  }

  void SetTrainOptions(const NnetTrainOptions &o) { opts_ = o; for (auto &l : layers_) l->SetTrainOptions(o); }
  void Reset(std::vector<int> &stream_reset_flag) {          // nnet-nnet.h:132-138: fan out to EVERY component
    for (auto &l : layers_) l->Reset(stream_reset_flag);
  }
  void SetSeqLengths(const std::vector<int32> &lens) {       // fan out to every component (a no-op for all but the bidirectional layer)
    for (auto &l : layers_) l->SetSeqLengths(lens);
  }

  // Nnet::Propagate [UPSTREAM]: each component's output buffer is (re)sized, then PropagateFnc.
  void Propagate(const MatrixView &in, DeviceMatrix *out) {
    const int32 n = NumComponents();
    if ((int32)prop_.size() != n + 1) { prop_.clear(); for (int32 i = 0; i <= n; i++) prop_.emplace_back(new DeviceMatrix()); }
    in0_ = in;
    for (int32 i = 0; i < n; i++) {
      prop_[i + 1]->Resize(in.NumRows(), layers_[i]->OutputDim(), false);
      MatrixView o = prop_[i + 1]->View();
      layers_[i]->PropagateFnc(i == 0 ? in : prop_[i]->View(), &o);
    }
    out->Resize(in.NumRows(), OutputDim(), false);
    MatrixView ov = out->View();
    KCheck(klstm_time_shift(prop_[n]->View().Data(), in.NumRows(), OutputDim(), prop_[n]->Stride(), ov.Data(), ov.Stride(), 0, nullptr));
  }
  void Feedforward(const MatrixView &in, DeviceMatrix *out) { Propagate(in, out); }

  // Nnet::Backpropagate(out_diff, NULL) [UPSTREAM]: components last -> first: Backpropagate, then Update if updatable.
  // The first component gets no in_diff (the stated reason for the dummy <Transmit>, README.md:49).
  void Backpropagate(const MatrixView &out_diff, MatrixView *in_diff) {
    const int32 n = NumComponents();
    KLSTM_ASSERT((int32)prop_.size() == n + 1);
    if ((int32)bprop_.size() != n + 1) { bprop_.clear(); for (int32 i = 0; i <= n; i++) bprop_.emplace_back(new DeviceMatrix()); }
    for (int32 i = n - 1; i >= 0; i--) {
      const MatrixView in = i == 0 ? in0_ : prop_[i]->View();
      const MatrixView out = prop_[i + 1]->View();
      const MatrixView od = i == n - 1 ? out_diff : bprop_[i + 1]->View();
      MatrixView idv, *idp = nullptr;
      if (i > 0) { bprop_[i]->Resize(in.NumRows(), layers_[i]->InputDim(), false); idv = bprop_[i]->View(); idp = &idv; }
      else if (in_diff) { idp = in_diff; }
      const bool upd = layers_[i]->IsUpdatable();
      layers_[i]->SetUpdateFollows(upd);
      layers_[i]->BackpropagateFnc(in, out, od, idp);
      if (upd) layers_[i]->Update(in, od);
      layers_[i]->SetUpdateFollows(false);
    }
  }
 private:
  std::vector<std::unique_ptr<Layer> > layers_;
  std::vector<std::unique_ptr<DeviceMatrix> > prop_, bprop_;
  MatrixView in0_;
  NnetTrainOptions opts_;
};

// Kaldi's Posterior (hmm/posterior.h [UPSTREAM-unvendored]; used as such in nnet-loss.cc:78): per frame a list of (pdf-id, weight)
typedef std::vector<std::vector<std::pair<int32, BaseFloat> > > Posterior;

// Xent with the overlay's EvalMasked (google/nnet/nnet-loss.h:33-80, nnet-loss.cc:76-164, Report :293-307).
class Xent {
 public:
  Xent() : frames_(0), correct_(0), loss_(0), entropy_(0), tgt_(nullptr), mask_(nullptr), rx_(nullptr), rc_(nullptr), cap_(0),
           poff_(nullptr), ppdf_(nullptr), pw_(nullptr), re_(nullptr), pcap_(0), ecap_(0) {}
  ~Xent() { klstm_free(tgt_); klstm_free(mask_); klstm_free(rx_); klstm_free(rc_); klstm_free(poff_); klstm_free(ppdf_); klstm_free(pw_); klstm_free(re_); }
  // EvalMasked with the reference's signature (nnet-loss.cc:76-79): general posteriors.  The (pdf, weight) lists go to the
  // device as CSR arrays (a few KB) instead of the reference's dense num_frames x num_pdf host matrix (:85-97).
  void EvalMasked(const std::vector<BaseFloat> &frame_mask, const DeviceMatrix &net_out, const Posterior &post, DeviceMatrix *diff) {
    const int32 n = net_out.NumRows(), d = net_out.NumCols();
    KLSTM_ASSERT(n == (int32)post.size() && n == (int32)frame_mask.size());              // :82
    std::vector<int32> off(1, 0), pdf;
    std::vector<BaseFloat> w;
    for (int32 t = 0; t < n; t++) {
      for (size_t i = 0; i < post[t].size(); i++) {
        const int32 id = post[t][i].first;
        if (id >= d || id < 0) KLSTM_ERR("Posterior pdf-id out of NN-output dimension, please check number of pdfs by 'hmm-info'." << " nn-outputs : " << d << ", posterior pdf-id : " << id);   // :89-92
        pdf.push_back(id); w.push_back(post[t][i].second);
      }
      off.push_back((int32)pdf.size());
    }
    void *p;
    if ((size_t)n > pcap_) {
      klstm_free(poff_); klstm_free(mask_); klstm_free(rx_); klstm_free(rc_); klstm_free(re_); klstm_free(tgt_);
      KCheck(klstm_malloc(&p, (size_t)(n + 1) * 4)); poff_ = (int32 *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); mask_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); rx_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); rc_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); re_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); tgt_ = (int32 *)p;
      pcap_ = n; cap_ = n;
    }
    if (pdf.size() + 1 > ecap_) {
      klstm_free(ppdf_); klstm_free(pw_);
      ecap_ = pdf.size() + 1;
      KCheck(klstm_malloc(&p, ecap_ * 4)); ppdf_ = (int32 *)p;
      KCheck(klstm_malloc(&p, ecap_ * 4)); pw_ = (BaseFloat *)p;
    }
    KCheck(klstm_memcpy_h2d(poff_, off.data(), off.size() * 4, nullptr));
    if (!pdf.empty()) { KCheck(klstm_memcpy_h2d(ppdf_, pdf.data(), pdf.size() * 4, nullptr)); KCheck(klstm_memcpy_h2d(pw_, w.data(), w.size() * 4, nullptr)); }
    KCheck(klstm_memcpy_h2d(mask_, frame_mask.data(), (size_t)n * 4, nullptr));
    diff->Resize(n, d, false);                                                            // :103
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_xent_eval_masked_post(y.Data(), n, d, y.Stride(), poff_, ppdf_, pw_, mask_, dv.Data(), dv.Stride(), rx_, re_, rc_, nullptr));
    std::vector<BaseFloat> rx(n), rc(n), re(n);
    KCheck(klstm_memcpy_d2h(rx.data(), rx_, (size_t)n * 4, nullptr));
    KCheck(klstm_memcpy_d2h(rc.data(), rc_, (size_t)n * 4, nullptr));
    KCheck(klstm_memcpy_d2h(re.data(), re_, (size_t)n * 4, nullptr));
    double xe = 0, ent = 0; int32 correct = 0, valid = 0;
    for (int32 i = 0; i < n; i++) { xe += rx[i]; ent += re[i]; correct += (rc[i] == 1.f); valid += (frame_mask[i] == 1.f); }
    loss_ += xe; entropy_ += ent; correct_ += correct; frames_ += valid;                  // :138-142
  }
  // frame_mask: 1 valid / 0 padded per row; target: pdf-id per row (one-hot posterior)
  void EvalMasked(const std::vector<BaseFloat> &frame_mask, const DeviceMatrix &net_out, const std::vector<int32> &target,
                  DeviceMatrix *diff) {
    const int32 n = net_out.NumRows(), d = net_out.NumCols();
    KLSTM_ASSERT(n == (int32)target.size() && n == (int32)frame_mask.size());          // :82
    for (int32 t : target) if (t >= d || t < 0) KLSTM_ERR("Posterior pdf-id out of NN-output dimension, please check number of pdfs by 'hmm-info'." << " nn-outputs : " << d << ", posterior pdf-id : " << t);   // :89-92
    if ((size_t)n > cap_) {
      klstm_free(tgt_); klstm_free(mask_); klstm_free(rx_); klstm_free(rc_);
      void *p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); tgt_ = (int32 *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); mask_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); rx_ = (BaseFloat *)p;
      KCheck(klstm_malloc(&p, (size_t)n * 4)); rc_ = (BaseFloat *)p;
      cap_ = n;
    }
    KCheck(klstm_memcpy_h2d(tgt_, target.data(), (size_t)n * 4, nullptr));
    KCheck(klstm_memcpy_h2d(mask_, frame_mask.data(), (size_t)n * 4, nullptr));
    diff->Resize(n, d, false);                                                            // :103
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_xent_eval_masked(y.Data(), n, d, y.Stride(), tgt_, mask_, dv.Data(), dv.Stride(), rx_, rc_, nullptr));
    std::vector<BaseFloat> rx(n), rc(n);
    KCheck(klstm_memcpy_d2h(rx.data(), rx_, (size_t)n * 4, nullptr));
    KCheck(klstm_memcpy_d2h(rc.data(), rc_, (size_t)n * 4, nullptr));
    double xe = 0; int32 correct = 0, valid = 0;
    for (int32 i = 0; i < n; i++) { xe += rx[i]; correct += (rc[i] == 1.f); valid += (frame_mask[i] == 1.f); }
    loss_ += xe; correct_ += correct; frames_ += valid;                                   // :138-142 (entropy of one-hot targets is 0)
  }
  std::string Report() const {                                                            // :293-307
    std::ostringstream oss;
    oss << "AvgLoss: " << (loss_ - entropy_) / frames_ << " (Xent), " << "[AvgXent: " << loss_ / frames_
        << ", AvgTargetEnt: " << entropy_ / frames_ << "]" << std::endl;
    oss << "\nFRAME_ACCURACY >> " << 100.0 * correct_ / frames_ << "% <<";
    return oss.str();
  }
  double AvgLoss() const { return (loss_ - entropy_) / frames_; }
  double FrameAccuracy() const { return (double)correct_ / frames_; }
  double Frames() const { return frames_; }
 private:
  double frames_, correct_, loss_, entropy_;
  int32 *tgt_; BaseFloat *mask_, *rx_, *rc_;
  size_t cap_;
  int32 *poff_, *ppdf_; BaseFloat *pw_, *re_;      // CSR posterior and per-row target entropy of the general EvalMasked
  size_t pcap_, ecap_;
};

struct TrainLstmStreamsOptions {              // bd-nnet-train-lstm-streams.cc:27-71 (the options that matter)
  NnetTrainOptions trn_opts;
  int32 targets_delay = 5, batch_size = 20, num_stream = 4;
  bool crossvalidate = false;
};
struct TrainLstmStreamsStats { int32 num_done = 0; double total_frames = 0, seconds = 0, avg_loss = 0, frame_accuracy = 0; int32 num_minibatches = 0; };

// The while(1) loop of bd-nnet-train-lstm-streams.cc:143-282 on in-memory utterances.
inline TrainLstmStreamsStats TrainLstmStreams(Nnet *nnet, const std::vector<Utterance> &utts, const TrainLstmStreamsOptions &o,
                                              std::string *report = nullptr) {
  nnet->SetTrainOptions(o.trn_opts);                                                  // :104
  MultiStreamBatcher batcher(&utts, o.num_stream, o.batch_size, o.targets_delay);
  Xent xent;
  StreamBatch b;
  DeviceMatrix feat_dev, nnet_out, obj_diff;
  TrainLstmStreamsStats st;
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->Reset(b.new_utt_flags);                                                     // :209
    feat_dev.CopyFromHost(b.feat.data(), o.batch_size * o.num_stream, b.dim);         // :212 CuMatrix(feat)  (no feature transform)
    nnet->Propagate(feat_dev.View(), &nnet_out);                                      // :215
    xent.EvalMasked(b.frame_mask, nnet_out, b.target, &obj_diff);                     // :219
    if (!o.crossvalidate) nnet->Backpropagate(obj_diff.View(), nullptr);              // :227-229
    st.total_frames += b.NumValidFrames();                                            // :241
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.avg_loss = xent.AvgLoss();
  st.frame_accuracy = xent.FrameAccuracy();
  if (report) *report = xent.Report();
  return st;
}

// Connectionist temporal classification on whole utterances (klstm_ctc_eval, klstm.h; not in the reference, whose only objective is
// the frame-level Xent above).  diff is the derivative with respect to the Softmax INPUT, like Xent's (SoftmaxLayer passes it on).
// The statistics stay on the device (four doubles that every Eval adds to) and are read when somebody asks: once per Report().
class Ctc {
 public:
  explicit Ctc(int32 blank = 0) : blank_(blank) {}
  ~Ctc() { klstm_free(ws_); klstm_free(lens_); klstm_free(lab_); klstm_free(off_); klstm_free(loss_); klstm_free(tot_); }
  Ctc(const Ctc &) = delete;
  Ctc &operator=(const Ctc &) = delete;

  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle), labels: per stream.  Utterances that
  // cannot be aligned (klstm.h: too short for their labels, a label outside [0, K) or equal to the blank) get zero diff rows and are
  // counted as rejected, on the device.  Only the shape is checked here.
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    KLSTM_ASSERT((int32)lens.size() == num_stream);
    Grow(&lens_, &lens_cap_, (size_t)num_stream * sizeof(int32));
    KCheck(klstm_memcpy_h2d(lens_, lens.data(), (size_t)num_stream * sizeof(int32), nullptr));
    Eval(net_out, num_stream, (const int32 *)lens_, labels, diff);
  }
  // the same with the lengths already on the device (the array SetSeqLengths was given)
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    const int32 rows = net_out.NumRows(), K = net_out.NumCols();
    KLSTM_ASSERT(num_stream > 0 && rows > 0 && rows % num_stream == 0 && (int32)labels.size() == num_stream && lens_dev);
    const int32 T = rows / num_stream;
    std::vector<int32> off(1, 0), flat;
    size_t longest = 0;
    for (const auto &l : labels) { flat.insert(flat.end(), l.begin(), l.end()); off.push_back((int32)flat.size()); longest = std::max(longest, l.size()); }
    if (flat.empty()) flat.push_back(0);
    const size_t need = klstm_ctc_workspace_bytes(T, num_stream, (int)longest);
    if (need == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    Grow(&ws_, &ws_cap_, need);
    Grow(&lab_, &lab_cap_, flat.size() * sizeof(int32));
    Grow(&off_, &off_cap_, off.size() * sizeof(int32));
    Grow(&loss_, &loss_cap_, (size_t)num_stream * sizeof(BaseFloat));
    if (!tot_) { void *p; KCheck(klstm_malloc(&p, 4 * sizeof(double))); tot_ = (double *)p; KCheck(klstm_memset_zero(tot_, 4 * sizeof(double), nullptr)); }
    KCheck(klstm_memcpy_h2d(lab_, flat.data(), flat.size() * sizeof(int32), nullptr));
    KCheck(klstm_memcpy_h2d(off_, off.data(), off.size() * sizeof(int32), nullptr));
    diff->Resize(rows, K, false);
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_ctc_eval(y.Data(), T, num_stream, K, y.Stride(), lens_dev, (const int32 *)lab_, (const int32 *)off_, blank_, dv.Data(),
                          dv.Stride(), (BaseFloat *)loss_, tot_, ws_, need, nullptr));
    num_stream_ = num_stream;
  }
  // -log p(labels | x) of the streams of the last Eval (+inf: rejected, 0: idle).  Synchronises.
  void UttLoss(std::vector<BaseFloat> *loss) const {
    loss->assign(num_stream_, 0.f);
    if (num_stream_) KCheck(klstm_memcpy_d2h(loss->data(), loss_, (size_t)num_stream_ * sizeof(BaseFloat), nullptr));
  }
  double AvgLoss() const { Fetch(); return h_[0] / h_[1]; }                // per utterance counted
  double AvgLossPerFrame() const { Fetch(); return h_[0] / h_[3]; }
  double NumUtterances() const { Fetch(); return h_[1]; }
  double NumRejected() const { Fetch(); return h_[2]; }
  double Frames() const { Fetch(); return h_[3]; }
  std::string Report() const {
    Fetch();
    std::ostringstream oss;
    oss << "AvgLoss: " << h_[0] / h_[1] << " (Ctc) per utterance, " << h_[0] / h_[3] << " per frame, [" << h_[1] << " utterances, " << h_[3]
        << " frames, " << h_[2] << " rejected]" << std::endl;
    return oss.str();
  }
 private:
  static void Grow(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return;
    klstm_free(*p); *p = nullptr; *cap = 0;
    KCheck(klstm_malloc(p, need));
    *cap = need;
  }
  void Fetch() const {                                                      // one small copy per question, none per minibatch
    h_[0] = h_[1] = h_[2] = h_[3] = 0;
    if (tot_) KCheck(klstm_memcpy_d2h(h_, tot_, 4 * sizeof(double), nullptr));
  }
  int32 blank_, num_stream_ = 0;
  void *ws_ = nullptr, *lens_ = nullptr, *lab_ = nullptr, *off_ = nullptr, *loss_ = nullptr;
  size_t ws_cap_ = 0, lens_cap_ = 0, lab_cap_ = 0, off_cap_ = 0, loss_cap_ = 0;
  double *tot_ = nullptr;
  mutable double h_[4] = {0, 0, 0, 0};
};

struct TrainCtcOptions {
  NnetTrainOptions trn_opts;
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, crossvalidate = false;
};
struct TrainCtcStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double num_rejected = 0, total_frames = 0, seconds = 0, avg_loss = 0, avg_loss_per_frame = 0;
};

// One pass over the utterances, num_stream whole utterances per minibatch, for unidirectional and bidirectional stacks alike: the
// lengths go to every component (the bidirectional layer needs them), every stream starts from zero state (a unidirectional
// <LstmProjectedStreams> stack through Reset; the bidirectional layer resets itself), and a unidirectional layer simply runs on
// through the padding: padding follows every valid frame and its diff rows are zero.  every_batch (optional) sees each minibatch
// after Ctc::Eval: (batch, net_out, obj_diff, ctc).
template <class F>
inline TrainCtcStats TrainCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainCtcOptions &o, std::string *report,
                                             F every_batch) {
  nnet->SetTrainOptions(o.trn_opts);
  WholeUtteranceBatcher batcher(&utts, o.num_stream, o.sort_by_length, o.max_frames);
  Ctc ctc(o.blank);
  UtteranceBatch b;
  DeviceMatrix feat_dev, nnet_out, obj_diff;
  TrainCtcStats st;
  std::vector<int> all(o.num_stream, 1);
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->SetSeqLengths(b.lens);
    nnet->Reset(all);
    feat_dev.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
    nnet->Propagate(feat_dev.View(), &nnet_out);
    ctc.Eval(nnet_out, b.num_stream, b.lens, b.labels, &obj_diff);
    every_batch(b, nnet_out, obj_diff, ctc);
    if (!o.crossvalidate) nnet->Backpropagate(obj_diff.View(), nullptr);
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.num_skipped = batcher.NumSkipped();
  st.num_rejected = ctc.NumRejected();
  st.total_frames = ctc.Frames();
  st.avg_loss = ctc.AvgLoss();
  st.avg_loss_per_frame = ctc.AvgLossPerFrame();
  if (report) *report = ctc.Report();
  return st;
}
inline TrainCtcStats TrainCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainCtcOptions &o,
                                             std::string *report = nullptr) {
  return TrainCtcWholeUtterances(nnet, utts, o, report, [](const UtteranceBatch &, const DeviceMatrix &, const DeviceMatrix &, const Ctc &) {});
}

// CTC best-path decoding of whole utterances and the token error rate against reference label sequences (klstm_ctc_decode, klstm.h;
// INTEGRATION.md 3e).  The five totals stay on the device and are read when somebody asks, like Ctc's.
class CtcGreedyDecoder {
 public:
  explicit CtcGreedyDecoder(int32 blank = 0) : blank_(blank) {}
  ~CtcGreedyDecoder() {
    klstm_free(ws_); klstm_free(lens_); klstm_free(lab_); klstm_free(off_); klstm_free(hyp_); klstm_free(hlen_); klstm_free(score_);
    klstm_free(fc_); klstm_free(err_); klstm_free(w_); klstm_free(tot_);
  }
  CtcGreedyDecoder(const CtcGreedyDecoder &) = delete;
  CtcGreedyDecoder &operator=(const CtcGreedyDecoder &) = delete;

  // One weight per class: the winner of a frame is argmax_k y[k] * w[k] (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  void SetClassWeights(const std::vector<BaseFloat> &w) {
    num_weights_ = (int32)w.size();
    if (w.empty()) return;
    Grow(&w_, &w_cap_, w.size() * sizeof(BaseFloat));
    KCheck(klstm_memcpy_h2d(w_, w.data(), w.size() * sizeof(BaseFloat), nullptr));
  }
  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle); refs: empty (no scoring) or one reference
  // per stream; hyps (optional): the hypothesis of every stream.  Asking for hyps synchronises; the rest stays on the device.
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &refs,
              std::vector<std::vector<int32> > *hyps) {
    KLSTM_ASSERT((int32)lens.size() == num_stream);
    Grow(&lens_, &lens_cap_, (size_t)num_stream * sizeof(int32));
    KCheck(klstm_memcpy_h2d(lens_, lens.data(), (size_t)num_stream * sizeof(int32), nullptr));
    Decode(net_out, num_stream, (const int32 *)lens_, refs, hyps);
  }
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &refs,
              std::vector<std::vector<int32> > *hyps) {
    const int32 rows = net_out.NumRows(), K = net_out.NumCols();
    KLSTM_ASSERT(num_stream > 0 && rows > 0 && rows % num_stream == 0 && lens_dev && (refs.empty() || (int32)refs.size() == num_stream));
    KLSTM_ASSERT(num_weights_ == 0 || num_weights_ == K);
    const int32 T = rows / num_stream;
    const bool scoring = !refs.empty();
    const size_t need = klstm_ctc_decode_workspace_bytes(T, num_stream, 0);
    if (need == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    Grow(&ws_, &ws_cap_, need);
    Grow(&hyp_, &hyp_cap_, (size_t)rows * sizeof(int32));
    Grow(&fc_, &fc_cap_, (size_t)rows * sizeof(int32));
    Grow(&hlen_, &hlen_cap_, (size_t)num_stream * sizeof(int32));
    Grow(&score_, &score_cap_, (size_t)num_stream * sizeof(BaseFloat));
    Grow(&err_, &err_cap_, (size_t)num_stream * sizeof(int32));
    if (scoring) {
      std::vector<int32> off(1, 0), flat;
      for (const auto &l : refs) { flat.insert(flat.end(), l.begin(), l.end()); off.push_back((int32)flat.size()); }
      if (flat.empty()) flat.push_back(0);
      Grow(&lab_, &lab_cap_, flat.size() * sizeof(int32));
      Grow(&off_, &off_cap_, off.size() * sizeof(int32));
      KCheck(klstm_memcpy_h2d(lab_, flat.data(), flat.size() * sizeof(int32), nullptr));
      KCheck(klstm_memcpy_h2d(off_, off.data(), off.size() * sizeof(int32), nullptr));
      if (!tot_) { void *p; KCheck(klstm_malloc(&p, 5 * sizeof(double))); tot_ = (double *)p; KCheck(klstm_memset_zero(tot_, 5 * sizeof(double), nullptr)); }
    }
    MatrixView y = net_out.View();
    KCheck(klstm_ctc_decode(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, num_weights_ ? (const BaseFloat *)w_ : nullptr,
                            (int32 *)hyp_, (int32 *)hlen_, (BaseFloat *)score_, (int32 *)fc_, scoring ? (const int32 *)lab_ : nullptr,
                            scoring ? (const int32 *)off_ : nullptr, scoring ? (int32 *)err_ : nullptr, scoring ? tot_ : nullptr, ws_, need,
                            nullptr));
    num_stream_ = num_stream; rows_ = rows; scored_ = scoring;
    if (!hyps) return;
    std::vector<int32> n(num_stream), h((size_t)rows);
    KCheck(klstm_memcpy_d2h(n.data(), hlen_, n.size() * sizeof(int32), nullptr));
    KCheck(klstm_memcpy_d2h(h.data(), hyp_, h.size() * sizeof(int32), nullptr));
    hyps->assign(num_stream, std::vector<int32>());
    for (int32 s = 0; s < num_stream; s++) (*hyps)[s].assign(h.begin() + (size_t)s * T, h.begin() + (size_t)s * T + n[s]);
  }
  // of the last Decode (each synchronises): path scores, edit distances (-1: not counted; all -1 without references), frame classes
  void UttScores(std::vector<BaseFloat> *v) const { v->assign(num_stream_, 0.f); Get(v->data(), score_, v->size() * sizeof(BaseFloat)); }
  void UttErrors(std::vector<int32> *v) const { v->assign(num_stream_, -1); if (scored_) Get(v->data(), err_, v->size() * sizeof(int32)); }
  void FrameClasses(std::vector<int32> *v) const { v->assign(rows_, -1); Get(v->data(), fc_, v->size() * sizeof(int32)); }

  double TokenErrorRate() const { Fetch(); return h_[0] / h_[1]; }          // edit errors / reference tokens
  double UtteranceErrorRate() const { Fetch(); return h_[4] / h_[3]; }
  double NumUtterances() const { Fetch(); return h_[3]; }
  double NumErrors() const { Fetch(); return h_[0]; }
  double NumRefTokens() const { Fetch(); return h_[1]; }
  double NumHypTokens() const { Fetch(); return h_[2]; }
  std::string Report() const {
    Fetch();
    std::ostringstream oss;
    oss << "UTT_ERROR_RATE: " << 100.0 * h_[4] / h_[3] << "% [" << h_[3] << " utterances, " << h_[0] << " errors, " << h_[1]
        << " reference tokens, " << h_[2] << " hypothesis tokens]" << std::endl;
    oss << "\nTOKEN_ERROR_RATE >> " << 100.0 * h_[0] / h_[1] << "% <<";
    return oss.str();
  }
 private:
  static void Grow(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return;
    klstm_free(*p); *p = nullptr; *cap = 0;
    KCheck(klstm_malloc(p, need));
    *cap = need;
  }
  static void Get(void *dst, const void *src, size_t bytes) { if (bytes) KCheck(klstm_memcpy_d2h(dst, src, bytes, nullptr)); }
  void Fetch() const {
    for (double &v : h_) v = 0;
    if (tot_) KCheck(klstm_memcpy_d2h(h_, tot_, 5 * sizeof(double), nullptr));
  }
  int32 blank_, num_stream_ = 0, rows_ = 0, num_weights_ = 0;
  bool scored_ = false;
  void *ws_ = nullptr, *lens_ = nullptr, *lab_ = nullptr, *off_ = nullptr, *hyp_ = nullptr, *hlen_ = nullptr, *score_ = nullptr, *fc_ = nullptr,
       *err_ = nullptr, *w_ = nullptr;
  size_t ws_cap_ = 0, lens_cap_ = 0, lab_cap_ = 0, off_cap_ = 0, hyp_cap_ = 0, hlen_cap_ = 0, score_cap_ = 0, fc_cap_ = 0, err_cap_ = 0, w_cap_ = 0;
  double *tot_ = nullptr;
  mutable double h_[5] = {0, 0, 0, 0, 0};
};

// CTC prefix beam search of whole utterances: the most probable labellings as n-best lists with scores, the token error rate of the
// 1-best and the oracle error rate of the list (klstm_ctc_beam_decode, klstm.h).  The six totals stay on the device
// and are read when somebody asks, like CtcGreedyDecoder's.
struct CtcHypothesis {
  std::vector<int32> tokens;
  BaseFloat score = 0.f;       // log probability as the search summed it
  int32 errors = -1;           // edit distance to the reference; -1: not counted
};
typedef std::vector<CtcHypothesis> CtcNbestList;     // best first

// A label language model or a lexicon for the beam search (klstm_ctc_beam_decode_lm, klstm.h): a dense deterministic
// weighted automaton over the K classes.  State 0 is the start; label c leads from state q to next[q*K + c] and multiplies the prefix
// probability by weight[q*K + c]; final[q] (empty: none) multiplies a hypothesis that ends in q.  Host tables in, device tables owned.
class CtcLabelLm {
 public:
  CtcLabelLm(int32 num_states, int32 num_classes, const std::vector<int32> &next, const std::vector<BaseFloat> &weight,
             const std::vector<BaseFloat> &final_weight = std::vector<BaseFloat>())
      : states_(num_states), classes_(num_classes) {
    const size_t n = (size_t)num_states * num_classes;
    KLSTM_ASSERT(num_states >= 1 && num_classes >= 2 && next.size() == n && weight.size() == n);
    KLSTM_ASSERT(final_weight.empty() || final_weight.size() == (size_t)num_states);
    try {
      KCheck(klstm_malloc(&next_, n * sizeof(int32)));
      KCheck(klstm_malloc(&weight_, n * sizeof(BaseFloat)));
      KCheck(klstm_memcpy_h2d(next_, next.data(), n * sizeof(int32), nullptr));
      KCheck(klstm_memcpy_h2d(weight_, weight.data(), n * sizeof(BaseFloat), nullptr));
      if (!final_weight.empty()) {
        KCheck(klstm_malloc(&final_, final_weight.size() * sizeof(BaseFloat)));
        KCheck(klstm_memcpy_h2d(final_, final_weight.data(), final_weight.size() * sizeof(BaseFloat), nullptr));
      }
    } catch (...) {                                          // no destructor runs for a half-built object
      Free();
      throw;
    }
  }
  ~CtcLabelLm() { Free(); }
  CtcLabelLm(const CtcLabelLm &) = delete;
  CtcLabelLm &operator=(const CtcLabelLm &) = delete;
  int32 NumStates() const { return states_; }
  int32 NumClasses() const { return classes_; }
  const int32 *Next() const { return (const int32 *)next_; }
  const BaseFloat *Weight() const { return (const BaseFloat *)weight_; }
  const BaseFloat *Final() const { return (const BaseFloat *)final_; }       // null: no final weights
 private:
  void Free() { klstm_free(next_); klstm_free(weight_); klstm_free(final_); next_ = weight_ = final_ = nullptr; }
  int32 states_, classes_;
  void *next_ = nullptr, *weight_ = nullptr, *final_ = nullptr;
};

class CtcBeamDecoder {
 public:
  explicit CtcBeamDecoder(int32 blank = 0, int32 beam = 16, int32 cands = 8, int32 nbest = 1) : blank_(blank), beam_(beam), cands_(cands), nbest_(nbest) {}
  ~CtcBeamDecoder() {
    klstm_free(ws_); klstm_free(lens_); klstm_free(lab_); klstm_free(off_); klstm_free(hyp_); klstm_free(hlen_); klstm_free(cnt_);
    klstm_free(score_); klstm_free(err_); klstm_free(w_); klstm_free(tot_);
  }
  CtcBeamDecoder(const CtcBeamDecoder &) = delete;
  CtcBeamDecoder &operator=(const CtcBeamDecoder &) = delete;

  // One weight per class: the emission of a frame is y[k] * w[k] (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  void SetClassWeights(const std::vector<BaseFloat> &w) {
    num_weights_ = (int32)w.size();
    if (w.empty()) return;
    Grow(&w_, &w_cap_, w.size() * sizeof(BaseFloat));
    KCheck(klstm_memcpy_h2d(w_, w.data(), w.size() * sizeof(BaseFloat), nullptr));
  }
  // Fuses a language model into the search: every later Decode goes through klstm_ctc_beam_decode_lm and its scores are the fused
  // ones.  The decoder keeps the pointer, not the tables; null: the search without one, as before.
  void SetLanguageModel(const CtcLabelLm *lm) { lm_ = lm; }
  // net_out, lens, refs as CtcGreedyDecoder::Decode takes them; lists (optional): the n-best list of every stream (empty for an idle
  // one).  Asking for lists synchronises; the rest stays on the device.
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &refs,
              std::vector<CtcNbestList> *lists) {
    KLSTM_ASSERT((int32)lens.size() == num_stream);
    Grow(&lens_, &lens_cap_, (size_t)num_stream * sizeof(int32));
    KCheck(klstm_memcpy_h2d(lens_, lens.data(), (size_t)num_stream * sizeof(int32), nullptr));
    Decode(net_out, num_stream, (const int32 *)lens_, refs, lists);
  }
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &refs,
              std::vector<CtcNbestList> *lists) {
    const int32 rows = net_out.NumRows(), K = net_out.NumCols();
    KLSTM_ASSERT(num_stream > 0 && rows > 0 && rows % num_stream == 0 && lens_dev && (refs.empty() || (int32)refs.size() == num_stream));
    KLSTM_ASSERT(num_weights_ == 0 || num_weights_ == K);
    KLSTM_ASSERT(nbest_ >= 1);
    const int32 T = rows / num_stream, N = nbest_;
    const bool scoring = !refs.empty();
    const size_t need = klstm_ctc_beam_workspace_bytes(T, num_stream, beam_, cands_);
    if (need == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    Grow(&ws_, &ws_cap_, need);
    Grow(&hyp_, &hyp_cap_, (size_t)rows * N * sizeof(int32));
    Grow(&hlen_, &hlen_cap_, (size_t)num_stream * N * sizeof(int32));
    Grow(&cnt_, &cnt_cap_, (size_t)num_stream * sizeof(int32));
    Grow(&score_, &score_cap_, (size_t)num_stream * N * sizeof(BaseFloat));
    Grow(&err_, &err_cap_, (size_t)num_stream * N * sizeof(int32));
    if (scoring) {
      std::vector<int32> off(1, 0), flat;
      for (const auto &l : refs) { flat.insert(flat.end(), l.begin(), l.end()); off.push_back((int32)flat.size()); }
      if (flat.empty()) flat.push_back(0);
      Grow(&lab_, &lab_cap_, flat.size() * sizeof(int32));
      Grow(&off_, &off_cap_, off.size() * sizeof(int32));
      KCheck(klstm_memcpy_h2d(lab_, flat.data(), flat.size() * sizeof(int32), nullptr));
      KCheck(klstm_memcpy_h2d(off_, off.data(), off.size() * sizeof(int32), nullptr));
      if (!tot_) { void *p; KCheck(klstm_malloc(&p, 6 * sizeof(double))); tot_ = (double *)p; KCheck(klstm_memset_zero(tot_, 6 * sizeof(double), nullptr)); }
    }
    MatrixView y = net_out.View();
    if (!lm_) {
      KCheck(klstm_ctc_beam_decode(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, num_weights_ ? (const BaseFloat *)w_ : nullptr,
                                   beam_, cands_, N, (int32 *)hyp_, (int32 *)hlen_, (int32 *)cnt_, (BaseFloat *)score_,
                                   scoring ? (const int32 *)lab_ : nullptr, scoring ? (const int32 *)off_ : nullptr,
                                   scoring ? (int32 *)err_ : nullptr, scoring ? tot_ : nullptr, ws_, need, nullptr));
    } else {
      KLSTM_ASSERT(lm_->NumClasses() == K);
      KCheck(klstm_ctc_beam_decode_lm(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, num_weights_ ? (const BaseFloat *)w_ : nullptr,
                                      beam_, cands_, N, lm_->NumStates(), lm_->Next(), lm_->Weight(), lm_->Final(), (int32 *)hyp_,
                                      (int32 *)hlen_, (int32 *)cnt_, (BaseFloat *)score_, scoring ? (const int32 *)lab_ : nullptr,
                                      scoring ? (const int32 *)off_ : nullptr, scoring ? (int32 *)err_ : nullptr, scoring ? tot_ : nullptr,
                                      ws_, need, nullptr));
    }
    num_stream_ = num_stream; scored_ = scoring;
    if (!lists) return;
    std::vector<int32> c(num_stream), n((size_t)num_stream * N), h((size_t)rows * N), e((size_t)num_stream * N, -1);
    std::vector<BaseFloat> sc((size_t)num_stream * N);
    Get(c.data(), cnt_, c.size() * sizeof(int32));
    Get(n.data(), hlen_, n.size() * sizeof(int32));
    Get(h.data(), hyp_, h.size() * sizeof(int32));
    Get(sc.data(), score_, sc.size() * sizeof(BaseFloat));
    if (scoring) Get(e.data(), err_, e.size() * sizeof(int32));
    lists->assign(num_stream, CtcNbestList());
    for (int32 s = 0; s < num_stream; s++)
      for (int32 q = 0; q < c[s]; q++) {
        const size_t o = (size_t)s * N + q;
        CtcHypothesis hy;
        hy.tokens.assign(h.begin() + o * T, h.begin() + o * T + n[o]);
        hy.score = sc[o];
        hy.errors = e[o];
        (*lists)[s].push_back(hy);
      }
  }
  // of the last Decode (each synchronises), per stream: entries of the list, the 1-best's score (0 for an empty list) and its edit
  // distance (-1: not counted; all -1 without references)
  void NbestCounts(std::vector<int32> *v) const { v->assign(num_stream_, 0); Get(v->data(), cnt_, v->size() * sizeof(int32)); }
  void UttScores(std::vector<BaseFloat> *v) const {
    std::vector<int32> c;
    NbestCounts(&c);
    std::vector<BaseFloat> sc((size_t)num_stream_ * nbest_);
    Get(sc.data(), score_, sc.size() * sizeof(BaseFloat));
    v->assign(num_stream_, 0.f);
    for (int32 s = 0; s < num_stream_; s++) if (c[s] > 0) (*v)[s] = sc[(size_t)s * nbest_];
  }
  void UttErrors(std::vector<int32> *v) const {
    v->assign(num_stream_, -1);
    if (!scored_) return;
    std::vector<int32> e((size_t)num_stream_ * nbest_);
    Get(e.data(), err_, e.size() * sizeof(int32));
    for (int32 s = 0; s < num_stream_; s++) (*v)[s] = e[(size_t)s * nbest_];
  }

  double TokenErrorRate() const { Fetch(); return h_[0] / h_[1]; }          // 1-best edit errors / reference tokens
  double OracleTokenErrorRate() const { Fetch(); return h_[5] / h_[1]; }    // the best of each list
  double UtteranceErrorRate() const { Fetch(); return h_[4] / h_[3]; }
  double NumUtterances() const { Fetch(); return h_[3]; }
  double NumErrors() const { Fetch(); return h_[0]; }
  double NumOracleErrors() const { Fetch(); return h_[5]; }
  double NumRefTokens() const { Fetch(); return h_[1]; }
  double NumHypTokens() const { Fetch(); return h_[2]; }
  std::string Report() const {
    Fetch();
    std::ostringstream oss;
    oss << "UTT_ERROR_RATE: " << 100.0 * h_[4] / h_[3] << "% [" << h_[3] << " utterances, " << h_[0] << " errors, " << h_[1]
        << " reference tokens, " << h_[2] << " hypothesis tokens]" << std::endl;
    oss << "ORACLE_TOKEN_ERROR_RATE: " << 100.0 * h_[5] / h_[1] << "% [" << nbest_ << "-best, beam " << beam_ << ", " << cands_ << " candidates]" << std::endl;
    oss << "\nTOKEN_ERROR_RATE >> " << 100.0 * h_[0] / h_[1] << "% <<";
    return oss.str();
  }
 private:
  static void Grow(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return;
    klstm_free(*p); *p = nullptr; *cap = 0;
    KCheck(klstm_malloc(p, need));
    *cap = need;
  }
  static void Get(void *dst, const void *src, size_t bytes) { if (bytes) KCheck(klstm_memcpy_d2h(dst, src, bytes, nullptr)); }
  void Fetch() const {
    for (double &v : h_) v = 0;
    if (tot_) KCheck(klstm_memcpy_d2h(h_, tot_, 6 * sizeof(double), nullptr));
  }
  int32 blank_, beam_, cands_, nbest_, num_stream_ = 0, num_weights_ = 0;
  bool scored_ = false;
  const CtcLabelLm *lm_ = nullptr;
  void *ws_ = nullptr, *lens_ = nullptr, *lab_ = nullptr, *off_ = nullptr, *hyp_ = nullptr, *hlen_ = nullptr, *cnt_ = nullptr, *score_ = nullptr,
       *err_ = nullptr, *w_ = nullptr;
  size_t ws_cap_ = 0, lens_cap_ = 0, lab_cap_ = 0, off_cap_ = 0, hyp_cap_ = 0, hlen_cap_ = 0, cnt_cap_ = 0, score_cap_ = 0, err_cap_ = 0, w_cap_ = 0;
  double *tot_ = nullptr;
  mutable double h_[6] = {0, 0, 0, 0, 0, 0};
};

struct DecodeCtcOptions {
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, score = true;              // score: the utterances' labels are references
  std::vector<BaseFloat> class_weights;                  // empty: none
  int32 beam = 0, cands = 8, nbest = 1;                  // beam 0: best path (CtcGreedyDecoder); beam > 0: prefix beam search (CtcBeamDecoder)
  const CtcLabelLm *lm = nullptr;                        // beam > 0 only: fused into the search (CtcBeamDecoder::SetLanguageModel); not owned
};
struct DecodeCtcStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double token_error_rate = 0, utt_error_rate = 0, num_scored = 0, num_errors = 0, num_ref_tokens = 0, seconds = 0;
  double oracle_token_error_rate = 0;                    // beam search only: the best hypothesis of every n-best list
};

// per-stream results of one minibatch -> per-utterance results in the order of the utterance list (idle streams carry nothing)
template <class V>
inline void ScatterByUtterance(const UtteranceBatch &b, const std::vector<V> &per_stream, std::vector<V> *per_utt) {
  KLSTM_ASSERT((int32)per_stream.size() == b.num_stream && (int32)b.utt_index.size() == b.num_stream);
  for (int32 s = 0; s < b.num_stream; s++) {
    if (b.utt_index[s] < 0) continue;
    KLSTM_ASSERT((size_t)b.utt_index[s] < per_utt->size());
    (*per_utt)[b.utt_index[s]] = per_stream[s];
  }
}

// The same loop with the prefix beam search (o.beam > 0).  (*hypotheses)[i] is the 1-best of utts[i], (*nbest_lists)[i] its whole list
// with scores and edit distances (either may be null; both empty for a skipped utterance).  every_batch sees (batch, net_out,
// CtcBeamDecoder) after Decode.
template <class F>
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::string *report, F every_batch) {
  KLSTM_ASSERT(o.beam > 0);
  WholeUtteranceBatcher batcher(&utts, o.num_stream, o.sort_by_length, o.max_frames);
  CtcBeamDecoder dec(o.blank, o.beam, o.cands, o.nbest);
  dec.SetClassWeights(o.class_weights);
  dec.SetLanguageModel(o.lm);
  UtteranceBatch b;
  DeviceMatrix feat_dev, nnet_out;
  DecodeCtcStats st;
  std::vector<int> all(o.num_stream, 1);
  std::vector<CtcNbestList> lists;
  const std::vector<std::vector<int32> > none;
  const bool want = hypotheses || nbest_lists;
  if (hypotheses) hypotheses->assign(utts.size(), std::vector<int32>());
  if (nbest_lists) nbest_lists->assign(utts.size(), CtcNbestList());
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->SetSeqLengths(b.lens);
    nnet->Reset(all);
    feat_dev.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
    nnet->Propagate(feat_dev.View(), &nnet_out);
    dec.Decode(nnet_out, b.num_stream, b.lens, o.score ? b.labels : none, want ? &lists : nullptr);
    if (nbest_lists) ScatterByUtterance(b, lists, nbest_lists);
    if (hypotheses) {
      std::vector<std::vector<int32> > best(b.num_stream);
      for (int32 s = 0; s < b.num_stream; s++) if (!lists[s].empty()) best[s] = lists[s][0].tokens;
      ScatterByUtterance(b, best, hypotheses);
    }
    every_batch(b, nnet_out, dec);
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.num_skipped = batcher.NumSkipped();
  st.num_scored = dec.NumUtterances();
  st.num_errors = dec.NumErrors();
  st.num_ref_tokens = dec.NumRefTokens();
  st.token_error_rate = dec.TokenErrorRate();
  st.utt_error_rate = dec.UtteranceErrorRate();
  st.oracle_token_error_rate = dec.OracleTokenErrorRate();
  if (report) *report = dec.Report();
  return st;
}
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::string *report = nullptr) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, nbest_lists, report, [](const UtteranceBatch &, const DeviceMatrix &, const CtcBeamDecoder &) {});
}

// The loop of TrainCtcWholeUtterances without the objective and the backward pass: SetSeqLengths, Reset, Propagate, Decode.
// (*hypotheses)[i] belongs to utts[i] whatever order the batcher handed them out in; an utterance the batcher skipped (empty, or
// longer than max_frames) keeps an empty hypothesis and is counted in num_skipped.  every_batch (optional) sees each minibatch after
// Decode: (batch, net_out, decoder).  With o.beam > 0 the prefix beam search decodes instead (the overload above; hypotheses are its
// 1-best) and every_batch, which expects the best-path decoder, is not called.
template <class F>
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::string *report, F every_batch) {
  if (o.beam > 0) return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, (std::vector<CtcNbestList> *)nullptr, report);
  WholeUtteranceBatcher batcher(&utts, o.num_stream, o.sort_by_length, o.max_frames);
  CtcGreedyDecoder dec(o.blank);
  dec.SetClassWeights(o.class_weights);
  UtteranceBatch b;
  DeviceMatrix feat_dev, nnet_out;
  DecodeCtcStats st;
  std::vector<int> all(o.num_stream, 1);
  std::vector<std::vector<int32> > hyps;
  const std::vector<std::vector<int32> > none;
  if (hypotheses) hypotheses->assign(utts.size(), std::vector<int32>());
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->SetSeqLengths(b.lens);
    nnet->Reset(all);
    feat_dev.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
    nnet->Propagate(feat_dev.View(), &nnet_out);
    dec.Decode(nnet_out, b.num_stream, b.lens, o.score ? b.labels : none, hypotheses ? &hyps : nullptr);
    if (hypotheses) ScatterByUtterance(b, hyps, hypotheses);
    every_batch(b, nnet_out, dec);
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.num_skipped = batcher.NumSkipped();
  st.num_scored = dec.NumUtterances();
  st.num_errors = dec.NumErrors();
  st.num_ref_tokens = dec.NumRefTokens();
  st.token_error_rate = dec.TokenErrorRate();
  st.utt_error_rate = dec.UtteranceErrorRate();
  if (report) *report = dec.Report();
  return st;
}
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::string *report = nullptr) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, report, [](const UtteranceBatch &, const DeviceMatrix &, const CtcGreedyDecoder &) {});
}

// CTC forced alignment of whole utterances: the most probable alignment of each stream's labels to its frames (klstm_ctc_align,
// klstm.h).  The five totals stay on the device and are read when somebody asks, like Ctc's.
class CtcAligner {
 public:
  explicit CtcAligner(int32 blank = 0) : blank_(blank) {}
  ~CtcAligner() {
    klstm_free(ws_); klstm_free(lens_); klstm_free(lab_); klstm_free(off_); klstm_free(fc_); klstm_free(fp_); klstm_free(tb_); klstm_free(te_);
    klstm_free(score_); klstm_free(w_); klstm_free(tot_);
  }
  CtcAligner(const CtcAligner &) = delete;
  CtcAligner &operator=(const CtcAligner &) = delete;

  // One weight per class: the emission of a frame becomes log(y[k] * w[k]) (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  void SetClassWeights(const std::vector<BaseFloat> &w) {
    num_weights_ = (int32)w.size();
    if (w.empty()) return;
    Grow(&w_, &w_cap_, w.size() * sizeof(BaseFloat));
    KCheck(klstm_memcpy_h2d(w_, w.data(), w.size() * sizeof(BaseFloat), nullptr));
  }
  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle); labels: per stream.  Utterances that
  // cannot be aligned (klstm.h) are rejected on the device.  Nothing synchronises.
  void Align(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &labels) {
    KLSTM_ASSERT((int32)lens.size() == num_stream);
    Grow(&lens_, &lens_cap_, (size_t)num_stream * sizeof(int32));
    KCheck(klstm_memcpy_h2d(lens_, lens.data(), (size_t)num_stream * sizeof(int32), nullptr));
    Align(net_out, num_stream, (const int32 *)lens_, labels);
  }
  void Align(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &labels) {
    const int32 rows = net_out.NumRows(), K = net_out.NumCols();
    KLSTM_ASSERT(num_stream > 0 && rows > 0 && rows % num_stream == 0 && (int32)labels.size() == num_stream && lens_dev);
    KLSTM_ASSERT(num_weights_ == 0 || num_weights_ == K);
    const int32 T = rows / num_stream;
    std::vector<int32> flat;
    off_h_.assign(1, 0);
    size_t longest = 0;
    for (const auto &l : labels) { flat.insert(flat.end(), l.begin(), l.end()); off_h_.push_back((int32)flat.size()); longest = std::max(longest, l.size()); }
    num_labels_ = flat.size();
    if (flat.empty()) flat.push_back(0);
    const size_t need = klstm_ctc_align_workspace_bytes(T, num_stream, (int)std::min(longest, (size_t)1023));   // longer: the device's to reject
    if (need == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    Grow(&ws_, &ws_cap_, need);
    Grow(&lab_, &lab_cap_, flat.size() * sizeof(int32));
    Grow(&off_, &off_cap_, off_h_.size() * sizeof(int32));
    Grow(&fc_, &fc_cap_, (size_t)rows * sizeof(int32));
    Grow(&fp_, &fp_cap_, (size_t)rows * sizeof(int32));
    Grow(&tb_, &tb_cap_, flat.size() * sizeof(int32));
    Grow(&te_, &te_cap_, flat.size() * sizeof(int32));
    Grow(&score_, &score_cap_, (size_t)num_stream * sizeof(BaseFloat));
    if (!tot_) { void *p; KCheck(klstm_malloc(&p, 5 * sizeof(double))); tot_ = (double *)p; KCheck(klstm_memset_zero(tot_, 5 * sizeof(double), nullptr)); }
    KCheck(klstm_memcpy_h2d(lab_, flat.data(), flat.size() * sizeof(int32), nullptr));
    KCheck(klstm_memcpy_h2d(off_, off_h_.data(), off_h_.size() * sizeof(int32), nullptr));
    MatrixView y = net_out.View();
    KCheck(klstm_ctc_align(y.Data(), T, num_stream, K, y.Stride(), lens_dev, (const int32 *)lab_, (const int32 *)off_, blank_,
                           num_weights_ ? (const BaseFloat *)w_ : nullptr, (int32 *)fc_, (int32 *)fp_, (int32 *)tb_, (int32 *)te_,
                           (BaseFloat *)score_, tot_, ws_, need, nullptr));
    num_stream_ = num_stream; rows_ = rows;
  }
  // of the last Align (each synchronises).  Frame classes and positions [T*num_stream], row t*S + s; -1 where there is no path
  void FrameClasses(std::vector<int32> *v) const { v->assign(rows_, -1); Get(v->data(), fc_, v->size() * sizeof(int32)); }
  void FramePositions(std::vector<int32> *v) const { v->assign(rows_, -1); Get(v->data(), fp_, v->size() * sizeof(int32)); }
  // per stream: first frame of every token and one past its last (empty for a stream without labels; -1 where not aligned)
  void TokenBounds(std::vector<std::vector<int32> > *begin, std::vector<std::vector<int32> > *end) const {
    std::vector<int32> b(num_labels_), e(num_labels_);
    Get(b.data(), tb_, b.size() * sizeof(int32));
    Get(e.data(), te_, e.size() * sizeof(int32));
    begin->assign(num_stream_, std::vector<int32>());
    end->assign(num_stream_, std::vector<int32>());
    for (int32 s = 0; s < num_stream_; s++) {
      (*begin)[s].assign(b.begin() + off_h_[s], b.begin() + off_h_[s + 1]);
      (*end)[s].assign(e.begin() + off_h_[s], e.begin() + off_h_[s + 1]);
    }
  }
  // log probability of the path (0: idle, -inf: rejected)
  void UttScores(std::vector<BaseFloat> *v) const { v->assign(num_stream_, 0.f); Get(v->data(), score_, v->size() * sizeof(BaseFloat)); }

  double AvgScorePerFrame() const { Fetch(); return h_[0] / h_[3]; }
  double BlankRatio() const { Fetch(); return h_[4] / h_[3]; }
  double NumAligned() const { Fetch(); return h_[1]; }
  double NumRejected() const { Fetch(); return h_[2]; }
  double Frames() const { Fetch(); return h_[3]; }
  std::string Report() const {
    Fetch();
    std::ostringstream oss;
    oss << "AvgPathScore: " << h_[0] / h_[3] << " (CtcAligner) per frame, blank ratio " << h_[4] / h_[3] << " [" << h_[1] << " utterances, " << h_[3]
        << " frames, " << h_[2] << " rejected]" << std::endl;
    return oss.str();
  }
 private:
  static void Grow(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return;
    klstm_free(*p); *p = nullptr; *cap = 0;
    KCheck(klstm_malloc(p, need));
    *cap = need;
  }
  static void Get(void *dst, const void *src, size_t bytes) { if (bytes) KCheck(klstm_memcpy_d2h(dst, src, bytes, nullptr)); }
  void Fetch() const {
    for (double &v : h_) v = 0;
    if (tot_) KCheck(klstm_memcpy_d2h(h_, tot_, 5 * sizeof(double), nullptr));
  }
  int32 blank_, num_stream_ = 0, rows_ = 0, num_weights_ = 0;
  size_t num_labels_ = 0;
  std::vector<int32> off_h_;
  void *ws_ = nullptr, *lens_ = nullptr, *lab_ = nullptr, *off_ = nullptr, *fc_ = nullptr, *fp_ = nullptr, *tb_ = nullptr, *te_ = nullptr,
       *score_ = nullptr, *w_ = nullptr;
  size_t ws_cap_ = 0, lens_cap_ = 0, lab_cap_ = 0, off_cap_ = 0, fc_cap_ = 0, fp_cap_ = 0, tb_cap_ = 0, te_cap_ = 0, score_cap_ = 0, w_cap_ = 0;
  double *tot_ = nullptr;
  mutable double h_[5] = {0, 0, 0, 0, 0};
};

struct AlignCtcOptions {
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true;
  std::vector<BaseFloat> class_weights;                  // empty: none
};
struct CtcAlignment {                                     // of one utterance; everything empty and aligned = false where there is none
  bool aligned = false;
  int32 blank = 0;                                        // the blank's index among frame_class
  BaseFloat score = 0.f;
  std::vector<int32> frame_class, token_begin, token_end;
};
struct AlignCtcStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double num_aligned = 0, num_rejected = 0, total_frames = 0, avg_score_per_frame = 0, blank_ratio = 0, seconds = 0;
};

// The loop of DecodeCtcWholeUtterances with the aligner in place of the decoder.  (*alignments)[i] belongs to utts[i] whatever
// order the batcher handed them out in; an utterance the batcher skipped or the device rejected keeps an empty alignment.
// every_batch (optional) sees each minibatch after Align: (batch, net_out, aligner).
template <class F>
inline AlignCtcStats AlignCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const AlignCtcOptions &o,
                                             std::vector<CtcAlignment> *alignments, std::string *report, F every_batch) {
  WholeUtteranceBatcher batcher(&utts, o.num_stream, o.sort_by_length, o.max_frames);
  CtcAligner al(o.blank);
  al.SetClassWeights(o.class_weights);
  UtteranceBatch b;
  DeviceMatrix feat_dev, nnet_out;
  AlignCtcStats st;
  std::vector<int> all(o.num_stream, 1);
  std::vector<int32> fc;
  std::vector<BaseFloat> score;
  std::vector<std::vector<int32> > tb, te;
  std::vector<CtcAlignment> per_stream;
  if (alignments) alignments->assign(utts.size(), CtcAlignment());
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->SetSeqLengths(b.lens);
    nnet->Reset(all);
    feat_dev.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
    nnet->Propagate(feat_dev.View(), &nnet_out);
    al.Align(nnet_out, b.num_stream, b.lens, b.labels);
    if (alignments) {
      al.FrameClasses(&fc); al.UttScores(&score); al.TokenBounds(&tb, &te);
      per_stream.assign(b.num_stream, CtcAlignment());
      for (int32 s = 0; s < b.num_stream; s++) {
        if (b.lens[s] <= 0 || fc[s] < 0) continue;                       // idle, or rejected: frame 0 carries -1
        CtcAlignment &a = per_stream[s];
        a.aligned = true; a.blank = o.blank; a.score = score[s]; a.token_begin = tb[s]; a.token_end = te[s];
        a.frame_class.resize(b.lens[s]);
        for (int32 t = 0; t < b.lens[s]; t++) a.frame_class[t] = fc[(size_t)t * b.num_stream + s];
      }
      ScatterByUtterance(b, per_stream, alignments);
    }
    every_batch(b, nnet_out, al);
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.num_skipped = batcher.NumSkipped();
  st.num_aligned = al.NumAligned();
  st.num_rejected = al.NumRejected();
  st.total_frames = al.Frames();
  st.avg_score_per_frame = al.AvgScorePerFrame();
  st.blank_ratio = al.BlankRatio();
  if (report) *report = al.Report();
  return st;
}
inline AlignCtcStats AlignCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const AlignCtcOptions &o,
                                             std::vector<CtcAlignment> *alignments, std::string *report = nullptr) {
  return AlignCtcWholeUtterances(nnet, utts, o, alignments, report, [](const UtteranceBatch &, const DeviceMatrix &, const CtcAligner &) {});
}

// The bridge to the frame-level trainer (TrainLstmStreams): targets = the class of every frame on the alignment, the blank's frames
// as blank_target (negative: the blank's own index).  Utterances without an alignment keep their targets.  Returns how many were
// filled.
inline int32 SetTargetsFromAlignment(std::vector<Utterance> *utts, const std::vector<CtcAlignment> &alignments, int32 blank_target = -1) {
  KLSTM_ASSERT(utts->size() == alignments.size());
  int32 filled = 0;
  for (size_t i = 0; i < utts->size(); i++) {
    const CtcAlignment &a = alignments[i];
    if (!a.aligned) continue;
    KLSTM_ASSERT((int32)a.frame_class.size() == (*utts)[i].num_frames);
    (*utts)[i].targets = a.frame_class;
    if (blank_target >= 0 && blank_target != a.blank)
      for (int32 &c : (*utts)[i].targets) if (c == a.blank) c = blank_target;
    filled++;
  }
  return filled;
}

}  // namespace klstm_kaldi
