// include/klstm_nnet.hpp -- minimal nnet1 container around the hot path: the `Nnet` the reference trainer
// drives (google/nnet/nnet-nnet.h:36-150, only the declaration is vendored), the components that appear
// in the reference topologies (google/nnet.proto, standard/nnet.proto, README.md:24-45), the masked
// cross-entropy (google/nnet/nnet-loss.cc:76-164, 293-307) and a workalike of the training loop of
// google/nnetbin/bd-nnet-train-lstm-streams.cc (:143-304) on in-memory utterances.
// Header-only C++ over the C-ABI (klstm.h); no HIP or Kaldi headers needed.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <istream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>

#include "klstm_cnn.h"
#include "klstm_component.hpp"
#include "klstm_dropout.h"
#include "klstm_nlm.h"
#include "klstm_trainer.hpp"

namespace klstm_kaldi {

inline void KCheck(klstm_status st) { if (st != KLSTM_OK) KLSTM_ERR("klstm: " << klstm_last_error() << " (status " << (int)st << ")"); }

// Owning device memory, move-only and grow-only: the one place in the headers that calls klstm_malloc.  Grow frees before it
// allocates and forgets the old block first, so a klstm_malloc that fails (KCheck throws) leaves an empty buffer behind.
class DeviceBuffer {
 public:
  DeviceBuffer() {}
  ~DeviceBuffer() { klstm_free(p_); }
  DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) { klstm_free(p_); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  void Grow(size_t bytes) {                                   // contents are not kept
    if (bytes <= cap_) return;
    klstm_free(p_); p_ = nullptr; cap_ = 0;
    KCheck(klstm_malloc(&p_, bytes));
    cap_ = bytes;
  }
  size_t Capacity() const { return cap_; }                    // bytes
  template <class T> T *As() const { return static_cast<T *>(p_); }       // null while nothing was ever needed
  template <class T> void Upload(const std::vector<T> &v, void *hip_stream = nullptr) {
    Grow(v.size() * sizeof(T));
    if (!v.empty()) KCheck(klstm_memcpy_h2d(p_, v.data(), v.size() * sizeof(T), hip_stream));
  }
  template <class T> void Download(T *dst, size_t n) const { if (n) KCheck(klstm_memcpy_d2h(dst, p_, n * sizeof(T), nullptr)); }
 private:
  void *p_ = nullptr;
  size_t cap_ = 0;
};

// N running sums that kernels add to: allocated and zeroed at the first Dev(), copied back once per Read() (all zeros before that).
template <int N>
class DeviceTotals {
 public:
  double *Dev() {
    if (!zeroed_) {
      buf_.Grow(N * sizeof(double));
      KCheck(klstm_memset_zero(buf_.As<double>(), N * sizeof(double), nullptr));
      zeroed_ = true;
    }
    return buf_.As<double>();
  }
  const double *Read() const {                                // synchronises; valid until the next Read
    for (double &v : h_) v = 0;
    buf_.Download(h_, zeroed_ ? N : 0);
    return h_;
  }
 private:
  DeviceBuffer buf_;
  bool zeroed_ = false;
  mutable double h_[N];
};

// CuMatrix stand-in: owning, pitched device matrix (cu-matrix.cc:51-84: rows are pitched; here the stride is the
// column count rounded up to 64 floats = 256 B).
class DeviceMatrix {
 public:
  DeviceMatrix() : rows_(0), cols_(0), stride_(0) {}
  DeviceMatrix(const DeviceMatrix &) = delete;
  DeviceMatrix &operator=(const DeviceMatrix &) = delete;
  void Resize(int32 rows, int32 cols, bool set_zero = true) {     // no realloc when the shape is unchanged (cu-matrix.cc:56-59)
    const int32 stride = (cols + 63) / 64 * 64;
    const size_t need = (size_t)rows * stride;
    buf_.Grow(need * sizeof(BaseFloat));
    rows_ = rows; cols_ = cols; stride_ = stride;
    if (set_zero && need) KCheck(klstm_memset_zero(Data(), need * sizeof(BaseFloat), nullptr));
  }
  int32 NumRows() const { return rows_; }
  int32 NumCols() const { return cols_; }
  int32 Stride() const { return stride_; }
  MatrixView View() const { return MatrixView(Data(), rows_, cols_, stride_); }
  void CopyFromHost(const BaseFloat *src, int32 rows, int32 cols) {          // CuMatrix(const Matrix&), cu-matrix.cc:287-311
    Resize(rows, cols, false);
    std::vector<BaseFloat> tmp((size_t)rows * stride_, 0.f);
    for (int32 r = 0; r < rows; r++) std::memcpy(&tmp[(size_t)r * stride_], src + (size_t)r * cols, cols * sizeof(BaseFloat));
    buf_.Upload(tmp);
  }
  void CopyToHost(std::vector<BaseFloat> *dst) const {
    std::vector<BaseFloat> tmp((size_t)rows_ * stride_);
    buf_.Download(tmp.data(), tmp.size());
    dst->resize((size_t)rows_ * cols_);
    for (int32 r = 0; r < rows_; r++) std::memcpy(&(*dst)[(size_t)r * cols_], &tmp[(size_t)r * stride_], cols_ * sizeof(BaseFloat));
  }
 private:
  BaseFloat *Data() const { return buf_.As<BaseFloat>(); }
  DeviceBuffer buf_;
  int32 rows_, cols_, stride_;
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
  AffineLayer(int32 in, int32 out) : in_(in), out_(out), lr_coef_(1.f), bias_lr_coef_(1.f), max_norm_(0.f) {}
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
    if (on_device_) Upload();
  }
  void HostParams(std::vector<BaseFloat> *w, std::vector<BaseFloat> *b) const {
    if (on_device_ && !host_fresh_) {
      hw_.resize((size_t)out_ * in_); hb_.resize(out_);
      W_.Download(hw_.data(), hw_.size());
      b_.Download(hb_.data(), hb_.size());
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
    KCheck(klstm_affine_propagate(in.Data(), in.NumRows(), in_, in.Stride(), W(), b(), out->Data(), out_, out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(klstm_affine_backpropagate(od.Data(), od.NumRows(), out_, od.Stride(), W(), in_, id->Data(), id->Stride(), nullptr));
  }
  void Update(const MatrixView &input, const MatrixView &diff) override {
    if (opts_.l2_penalty != 0.f || opts_.l1_penalty != 0.f) KLSTM_ERR("AffineTransform: l1/l2 penalties are not implemented");
    KCheck(klstm_affine_update(input.Data(), input.Stride(), diff.Data(), diff.Stride(), input.NumRows(), in_, out_, W(), b(),
                               Wc_.As<BaseFloat>(), bc_.As<BaseFloat>(), opts_.learn_rate * lr_coef_, opts_.learn_rate * bias_lr_coef_,
                               opts_.momentum, nullptr));
    host_fresh_ = false;
  }
  void SetTrainOptions(const NnetTrainOptions &o) override { opts_ = o; }
 private:
  void Alloc() {                          // on_device_ only once everything is there: a failure half way is tried again in full
    if (on_device_) return;
    Wc_.Grow((size_t)out_ * in_ * 4);
    bc_.Grow((size_t)out_ * 4);
    KCheck(klstm_memset_zero(Wc_.As<BaseFloat>(), (size_t)out_ * in_ * 4, nullptr));
    KCheck(klstm_memset_zero(bc_.As<BaseFloat>(), (size_t)out_ * 4, nullptr));
    Upload();
    on_device_ = true;
  }
  void Upload() {
    KLSTM_ASSERT((int32)hw_.size() == out_ * in_ && (int32)hb_.size() == out_);
    W_.Upload(hw_);
    b_.Upload(hb_);
  }
  BaseFloat *W() const { return W_.As<BaseFloat>(); }
  BaseFloat *b() const { return b_.As<BaseFloat>(); }
  int32 in_, out_;
  BaseFloat lr_coef_, bias_lr_coef_, max_norm_;
  NnetTrainOptions opts_;
  DeviceBuffer W_, b_, Wc_, bc_;
  bool on_device_ = false;
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

// [UPSTREAM-unvendored nnet-various.h] Dropout, the component the reference points at (nnet-nnet.h:98-99 declares
// Nnet::SetDropoutRetention; its own "LSTM forward dropout" is commented out, bd-nnet-lstm-projected-streams.h:247-256): model line
// "<Dropout> 512 512 <DropoutRetention> 0.8 ".  It stands BETWEEN layers -- the operator acts on what goes up, never on what goes
// through time -- and runs kdrop_apply (klstm_dropout.h: the definition).  Only the retention is in the model file; the rest is
// run-time state:
//   active     OFF by default: the layer is a copy for every caller of Propagate that is not training (decoders, aligner, scorers)
//   seed, salt the key and the layer's own word of the counter (Nnet::SetDropoutSeed gives component i salt i); SetSeed also winds
//              the step and the sequence counter back to 0, so the same seed and the same calls replay the same masks bit for bit
//   step       advances with every active PropagateFnc; BackpropagateFnc replays the counters of the last PropagateFnc
//   per-sequence mode: one mask per (stream, sequence) for all its frames: a stream gets the next id of the layer's counter whenever
//              Reset(flags) flags it; the ids go to the device only when they changed
class DropoutLayer : public Layer {
 public:
  DropoutLayer(int32 i, int32 o) : dim_(i) { if (i != o) KLSTM_ERR("<Dropout>: input dim " << i << " != output dim " << o); }
  const char *Marker() const override { return "<Dropout>"; }
  int32 InputDim() const override { return dim_; }
  int32 OutputDim() const override { return dim_; }
  void ReadData(std::istream &is, bool binary) override {
    ExpectToken(is, binary, "<DropoutRetention>");
    BaseFloat r = 0;
    ReadBasicType(is, binary, &r);
    SetRetention(r);
  }
  void WriteData(std::ostream &os, bool binary) const override {
    WriteToken(os, binary, "<DropoutRetention>");
    WriteBasicType(os, binary, retention_);
    if (!binary) os << "\n";
  }
  void SetRetention(BaseFloat r) {
    unsigned thr; BaseFloat scale;
    if (!(r > 0.f && r <= 1.f) || kdrop_threshold(r, &thr, &scale) != KLSTM_OK) KLSTM_ERR("<Dropout>: retention " << r << " outside (0, 1]");
    retention_ = r;
  }
  BaseFloat Retention() const { return retention_; }
  void SetActive(bool on) { active_ = on; }
  bool Active() const { return active_; }
  void SetSeed(uint64_t seed, uint32_t salt) {
    if (salt >= 0x80000000u) KLSTM_ERR("<Dropout>: salt " << salt << " is not below 2^31");
    seed_ = seed; salt_ = salt; step_ = last_step_ = 0; next_seq_ = 0; seq_ids_.clear(); ids_fresh_ = false;
  }
  void SetPerSequence(bool on) { per_sequence_ = on; }
  bool PerSequence() const { return per_sequence_; }
  uint32_t Step() const { return step_; }
  void Reset(std::vector<int> &flags) override {
    if (seq_ids_.size() != flags.size()) {                       // a new stream count: every stream starts a sequence
      seq_ids_.resize(flags.size());
      for (unsigned &id : seq_ids_) id = next_seq_++;
      ids_fresh_ = false;
      return;
    }
    for (size_t s = 0; s < flags.size(); s++) if (flags[s]) { seq_ids_[s] = next_seq_++; ids_fresh_ = false; }
  }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    if (active_) last_step_ = step_++;
    Apply(in, out);
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &, const MatrixView &od, MatrixView *id) override { if (id) Apply(od, id); }
 private:
  void Apply(const MatrixView &in, MatrixView *out) {
    const bool seq = active_ && per_sequence_ && retention_ != 1.f;
    if (seq) {
      if (seq_ids_.empty()) KLSTM_ERR("<Dropout>: per-sequence masks need a Reset(flags) before the first Propagate");
      if (!ids_fresh_) { ids_.Upload(seq_ids_); ids_fresh_ = true; }
    }
    KCheck(kdrop_apply(in.Data(), in.Stride(), in.NumRows(), dim_, out->Data(), out->Stride(), active_ ? retention_ : 1.f, seed_, last_step_,
                       salt_, seq ? KDROP_SEQUENCE : KDROP_ELEMENT, seq ? (int)seq_ids_.size() : 1, seq ? ids_.As<unsigned>() : nullptr, nullptr));
  }
  int32 dim_;
  BaseFloat retention_ = 1.f;
  bool active_ = false, per_sequence_ = false, ids_fresh_ = false;
  uint64_t seed_ = 0;
  uint32_t salt_ = 0, step_ = 0, last_step_ = 0, next_seq_ = 0;
  std::vector<unsigned> seq_ids_;
  DeviceBuffer ids_;
};

// [UPSTREAM-unvendored nnet-convolutional-component.h] ConvolutionalComponent: the filters slide along the frequency axis of n spliced
// blocks of st values (klstm_cnn.h: THE DEFINITION and the kcnn_conv_* entries; no im2col matrix exists at any point).  Model line
// "<ConvolutionalComponent> 4224 440 <PatchDim> 8 <PatchStep> 1 <PatchStride> 40 <LearnRateCoef> 1 <BiasLearnRateCoef> 1 <MaxNorm> 0
// <Filters>  [ F x K ] <Bias>  [ F ]": the tokens before <Filters> are read in any order and written in this one; <MaxNorm> is read,
// kept and written as AffineLayer does.  Parameters keep a host shadow (files are read, written and converted without a GPU); the device
// copy is created at the first PropagateFnc.  The update is the affine rule (klstm_affine_update): at momentum 0 what upstream does.
class ConvolutionalLayer : public Layer {
 public:
  ConvolutionalLayer(int32 in, int32 out) : in_(in), out_(out) {}
  ConvolutionalLayer(int32 in, int32 out, int32 patch_dim, int32 patch_step, int32 patch_stride) : in_(in), out_(out) { SetGeometry(patch_dim, patch_step, patch_stride); }
  const char *Marker() const override { return "<ConvolutionalComponent>"; }
  int32 InputDim() const override { return in_; }
  int32 OutputDim() const override { return out_; }
  bool IsUpdatable() const override { return true; }
  int32 PatchDim() const { return pd_; }
  int32 PatchStep() const { return ps_; }
  int32 PatchStride() const { return st_; }
  int32 NumPatches() const { return P_; }
  int32 NumFilters() const { return F_; }
  int32 FilterDim() const { return K_; }
  void ReadData(std::istream &is, bool binary) override {
    int32 pd = 0, ps = 0, st = 0;
    while (true) {
      std::string tok;
      ReadToken(is, binary, &tok);
      if (tok == "<Filters>") break;
      if (tok == "<PatchDim>") ReadBasicType(is, binary, &pd);
      else if (tok == "<PatchStep>") ReadBasicType(is, binary, &ps);
      else if (tok == "<PatchStride>") ReadBasicType(is, binary, &st);
      else if (tok == "<LearnRateCoef>") ReadBasicType(is, binary, &lr_coef_);
      else if (tok == "<BiasLearnRateCoef>") ReadBasicType(is, binary, &bias_lr_coef_);
      else if (tok == "<MaxNorm>") ReadBasicType(is, binary, &max_norm_);
      else KLSTM_ERR("ConvolutionalComponent: unknown token " << tok);
    }
    SetGeometry(pd, ps, st);
    std::vector<BaseFloat> w, b;
    int32 r, c;
    ReadMatrix(is, binary, &w, &r, &c);
    ExpectToken(is, binary, "<Bias>");
    ReadVector(is, binary, &b);
    if (r != F_ || c != K_ || (int32)b.size() != F_)
      KLSTM_ERR("ConvolutionalComponent: <Filters> " << r << " x " << c << ", <Bias> " << b.size() << " where " << F_ << " x " << K_ << " and " << F_ << " belong");
    SetParams(w, b);
  }
  void WriteData(std::ostream &os, bool binary) const override {
    std::vector<BaseFloat> w, b;
    HostParams(&w, &b);
    WriteToken(os, binary, "<PatchDim>"); WriteBasicType(os, binary, pd_);
    WriteToken(os, binary, "<PatchStep>"); WriteBasicType(os, binary, ps_);
    WriteToken(os, binary, "<PatchStride>"); WriteBasicType(os, binary, st_);
    WriteToken(os, binary, "<LearnRateCoef>"); WriteBasicType(os, binary, lr_coef_);
    WriteToken(os, binary, "<BiasLearnRateCoef>"); WriteBasicType(os, binary, bias_lr_coef_);
    WriteToken(os, binary, "<MaxNorm>"); WriteBasicType(os, binary, max_norm_);
    WriteToken(os, binary, "<Filters>");
    WriteMatrix(os, binary, w.data(), F_, K_, K_);
    WriteToken(os, binary, "<Bias>");
    WriteVector(os, binary, b.data(), F_);
  }
  void SetParams(const std::vector<BaseFloat> &w, const std::vector<BaseFloat> &b) {       // filters F x K row-major, bias F
    KLSTM_ASSERT(K_ > 0 && (int32)w.size() == F_ * K_ && (int32)b.size() == F_);
    hw_ = w; hb_ = b; host_fresh_ = true;
    if (on_device_) Upload();
  }
  void HostParams(std::vector<BaseFloat> *w, std::vector<BaseFloat> *b) const {
    if (on_device_ && !host_fresh_) {
      hw_.resize((size_t)F_ * K_); hb_.resize(F_);
      W_.Download(hw_.data(), hw_.size());
      b_.Download(hb_.data(), hb_.size());
      host_fresh_ = true;
    }
    *w = hw_; *b = hb_;
  }
  int32 NumParams() const override { return F_ * K_ + F_; }
  void GetParams(std::vector<BaseFloat> *p) const override {                                // filters, then bias
    std::vector<BaseFloat> w, b; HostParams(&w, &b); *p = w; p->insert(p->end(), b.begin(), b.end());
  }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    Alloc();
    KCheck(kcnn_conv_propagate(in.Data(), in.Stride(), in.NumRows(), in_, out_, pd_, ps_, st_, W(), b(), out->Data(), out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(kcnn_conv_backpropagate(od.Data(), od.Stride(), od.NumRows(), in_, out_, pd_, ps_, st_, W(), id->Data(), id->Stride(), nullptr));
  }
  void Update(const MatrixView &input, const MatrixView &diff) override {
    if (opts_.l2_penalty != 0.f || opts_.l1_penalty != 0.f) KLSTM_ERR("ConvolutionalComponent: l1/l2 penalties are not implemented");
    const size_t need = kcnn_conv_workspace_floats(input.NumRows(), in_, out_, pd_, ps_, st_);
    ws_.Grow(need * sizeof(BaseFloat));
    KCheck(kcnn_conv_update(input.Data(), input.Stride(), diff.Data(), diff.Stride(), input.NumRows(), in_, out_, pd_, ps_, st_, W(), b(),
                            Wc_.As<BaseFloat>(), bc_.As<BaseFloat>(), opts_.learn_rate * lr_coef_, opts_.learn_rate * bias_lr_coef_,
                            opts_.momentum, ws_.As<BaseFloat>(), ws_.Capacity() / sizeof(BaseFloat), nullptr));
    host_fresh_ = false;
  }
  void SetTrainOptions(const NnetTrainOptions &o) override { opts_ = o; }
 private:
  void SetGeometry(int32 pd, int32 ps, int32 st) {
    int n, P, K, F;
    if (kcnn_conv_plan(in_, out_, pd, ps, st, &n, &P, &K, &F) != KLSTM_OK) KLSTM_ERR("ConvolutionalComponent: " << klstm_last_error());
    pd_ = pd; ps_ = ps; st_ = st; P_ = P; K_ = K; F_ = F;
  }
  void Alloc() {                          // on_device_ only once everything is there: a failure half way is tried again in full
    if (on_device_) return;
    Wc_.Grow((size_t)F_ * K_ * 4);
    bc_.Grow((size_t)F_ * 4);
    KCheck(klstm_memset_zero(Wc_.As<BaseFloat>(), (size_t)F_ * K_ * 4, nullptr));
    KCheck(klstm_memset_zero(bc_.As<BaseFloat>(), (size_t)F_ * 4, nullptr));
    Upload();
    on_device_ = true;
  }
  void Upload() {
    KLSTM_ASSERT((int32)hw_.size() == F_ * K_ && (int32)hb_.size() == F_);
    W_.Upload(hw_);
    b_.Upload(hb_);
  }
  BaseFloat *W() const { return W_.As<BaseFloat>(); }
  BaseFloat *b() const { return b_.As<BaseFloat>(); }
  int32 in_, out_, pd_ = 0, ps_ = 0, st_ = 0, P_ = 0, K_ = 0, F_ = 0;
  BaseFloat lr_coef_ = 1.f, bias_lr_coef_ = 1.f, max_norm_ = 0.f;
  NnetTrainOptions opts_;
  DeviceBuffer W_, b_, Wc_, bc_, ws_;
  bool on_device_ = false;
  mutable std::vector<BaseFloat> hw_, hb_;
  mutable bool host_fresh_ = true;
};

// [UPSTREAM-unvendored nnet-max-pooling-component.h] MaxPoolingComponent: the maximum over z neighbouring patches of w values (w = the
// number of filters below), every g patches; model line "<MaxPoolingComponent> 1408 4224 <PoolSize> 3 <PoolStep> 3 <PoolStride> 128 ".
// The backward pass is nnet1's rule (klstm_cnn.h): with overlapping pools it is not the true gradient of the maximum.
class MaxPoolingLayer : public Layer {
 public:
  MaxPoolingLayer(int32 in, int32 out) : in_(in), out_(out) {}
  MaxPoolingLayer(int32 in, int32 out, int32 size, int32 step, int32 stride) : in_(in), out_(out) { SetGeometry(size, step, stride); }
  const char *Marker() const override { return "<MaxPoolingComponent>"; }
  int32 InputDim() const override { return in_; }
  int32 OutputDim() const override { return out_; }
  int32 PoolSize() const { return z_; }
  int32 PoolStep() const { return g_; }
  int32 PoolStride() const { return w_; }
  void ReadData(std::istream &is, bool binary) override {
    int32 z = 0, g = 0, w = 0;
    ExpectToken(is, binary, "<PoolSize>"); ReadBasicType(is, binary, &z);
    ExpectToken(is, binary, "<PoolStep>"); ReadBasicType(is, binary, &g);
    ExpectToken(is, binary, "<PoolStride>"); ReadBasicType(is, binary, &w);
    SetGeometry(z, g, w);
  }
  void WriteData(std::ostream &os, bool binary) const override {
    WriteToken(os, binary, "<PoolSize>"); WriteBasicType(os, binary, z_);
    WriteToken(os, binary, "<PoolStep>"); WriteBasicType(os, binary, g_);
    WriteToken(os, binary, "<PoolStride>"); WriteBasicType(os, binary, w_);
    if (!binary) os << "\n";
  }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    KCheck(kcnn_pool_propagate(in.Data(), in.Stride(), in.NumRows(), in_, out_, z_, g_, w_, out->Data(), out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &in, const MatrixView &out, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(kcnn_pool_backpropagate(in.Data(), in.Stride(), out.Data(), out.Stride(), od.Data(), od.Stride(), in.NumRows(), in_, out_, z_, g_, w_,
                                           id->Data(), id->Stride(), nullptr));
  }
 private:
  void SetGeometry(int32 z, int32 g, int32 w) {
    const bool ok = z >= 1 && g >= 1 && w >= 1 && in_ % w == 0 && z <= in_ / w && (int64_t)(1 + (in_ / w - z) / g) * w == out_;
    if (!ok) KLSTM_ERR("MaxPoolingComponent: inconsistent numbers (in " << in_ << ", out " << out_ << ", pool size " << z << ", step " << g << ", stride " << w << ")");
    z_ = z; g_ = g; w_ = w;
  }
  int32 in_, out_, z_ = 0, g_ = 0, w_ = 0;
};

// [UPSTREAM-unvendored nnet-activation.h] Sigmoid / Tanh between the layers: no data; the backward pass works from the OUTPUT
// (in_diff = out_diff y (1 - y) or out_diff (1 - y y)); the forms of the LSTM cell (klstm_cnn.h).
template <int KIND>
class ActivationLayer : public Layer {
 public:
  ActivationLayer(int32 i, int32 o) : dim_(i) { if (i != o) KLSTM_ERR(Marker() << ": input dim " << i << " != output dim " << o); }
  const char *Marker() const override { return KIND == KCNN_SIGMOID ? "<Sigmoid>" : "<Tanh>"; }
  int32 InputDim() const override { return dim_; }
  int32 OutputDim() const override { return dim_; }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override {
    KCheck(kcnn_activation(KIND, in.Data(), in.Stride(), in.NumRows(), dim_, out->Data(), out->Stride(), nullptr));
  }
  void BackpropagateFnc(const MatrixView &, const MatrixView &out, const MatrixView &od, MatrixView *id) override {
    if (id) KCheck(kcnn_activation_diff(KIND, out.Data(), out.Stride(), od.Data(), od.Stride(), out.NumRows(), dim_, id->Data(), id->Stride(), nullptr));
  }
 private:
  int32 dim_;
};
typedef ActivationLayer<KCNN_SIGMOID> SigmoidLayer;
typedef ActivationLayer<KCNN_TANH> TanhLayer;

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
      else if (token == "<Dropout>") l = new DropoutLayer(dim_in, dim_out);
      else if (token == "<ConvolutionalComponent>") l = new ConvolutionalLayer(dim_in, dim_out);
      else if (token == "<MaxPoolingComponent>") l = new MaxPoolingLayer(dim_in, dim_out);
      else if (token == "<Sigmoid>") l = new SigmoidLayer(dim_in, dim_out);
      else if (token == "<Tanh>") l = new TanhLayer(dim_in, dim_out);
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

  // The <Dropout> components (klstm_dropout.h).  SetDropoutRetention is the reference's declared method (nnet-nnet.h:98-99): every
  // <Dropout> takes r.  They are OFF until SetDropoutActive(true); SetDropoutSeed gives component i the salt i and winds the
  // counters back (same seed, same calls: the same masks); SetDropoutPerSequence: one mask per (stream, sequence).
  int32 NumDropout() const { int32 n = 0; for (const auto &l : layers_) n += Dropout(l.get()) != nullptr; return n; }
  void SetDropoutRetention(BaseFloat r) { for (auto &l : layers_) if (DropoutLayer *d = Dropout(l.get())) d->SetRetention(r); }
  void SetDropoutActive(bool on) { for (auto &l : layers_) if (DropoutLayer *d = Dropout(l.get())) d->SetActive(on); }
  void SetDropoutSeed(uint64_t seed) { for (size_t i = 0; i < layers_.size(); i++) if (DropoutLayer *d = Dropout(layers_[i].get())) d->SetSeed(seed, (uint32_t)i); }
  void SetDropoutPerSequence(bool on) { for (auto &l : layers_) if (DropoutLayer *d = Dropout(l.get())) d->SetPerSequence(on); }
  std::vector<bool> DropoutActive() const {                 // of the <Dropout> components, in order
    std::vector<bool> v;
    for (const auto &l : layers_) if (const DropoutLayer *d = Dropout(l.get())) v.push_back(d->Active());
    return v;
  }
  void SetDropoutActive(const std::vector<bool> &v) {
    size_t k = 0;
    for (auto &l : layers_) if (DropoutLayer *d = Dropout(l.get())) { if (k < v.size()) d->SetActive(v[k]); k++; }
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
  static DropoutLayer *Dropout(Layer *l) { return std::string(l->Marker()) == "<Dropout>" ? static_cast<DropoutLayer *>(l) : nullptr; }
  static const DropoutLayer *Dropout(const Layer *l) { return std::string(l->Marker()) == "<Dropout>" ? static_cast<const DropoutLayer *>(l) : nullptr; }
  std::vector<std::unique_ptr<Layer> > layers_;
  std::vector<std::unique_ptr<DeviceMatrix> > prop_, bprop_;
  MatrixView in0_;
  NnetTrainOptions opts_;
};

// The model as inference sees it: the <Dropout> components removed, the rest through the binary form (the result is what Nnet::Read
// makes of that file).  A <Dropout> that is off is a copy, so both models compute the same; this one has the contiguous run of LSTM
// layers that BatchScorer and CtcNeuralRescorer ask for.  Host only.
inline void WithoutDropout(const Nnet &in, Nnet *out) {
  std::stringstream ss;
  WriteToken(ss, true, "<Nnet>");
  for (int32 i = 0; i < in.NumComponents(); i++)
    if (std::string(in.GetComponent(i).Marker()) != "<Dropout>") in.GetComponent(i).Write(ss, true);
  WriteToken(ss, true, "</Nnet>");
  out->Read(ss, true);
}

// What the four trainers do about dropout: for the scope's duration, and only when it trains (not under crossvalidate), the
// <Dropout> components are switched on with the options' seed and mode (and retention, unless 0: the model's own); every exit path,
// an exception included, puts the active flags back as they were.
class DropoutTrainingScope {
 public:
  DropoutTrainingScope(Nnet *nnet, bool crossvalidate, BaseFloat retention, uint64_t seed, bool per_sequence)
      : nnet_(nnet), on_(!crossvalidate && nnet->NumDropout() > 0) {
    if (!on_) return;
    was_ = nnet->DropoutActive();
    if (retention != 0.f) nnet->SetDropoutRetention(retention);
    nnet->SetDropoutSeed(seed);
    nnet->SetDropoutPerSequence(per_sequence);
    nnet->SetDropoutActive(true);
  }
  ~DropoutTrainingScope() { if (on_) nnet_->SetDropoutActive(was_); }
  DropoutTrainingScope(const DropoutTrainingScope &) = delete;
  DropoutTrainingScope &operator=(const DropoutTrainingScope &) = delete;
 private:
  Nnet *nnet_;
  bool on_;
  std::vector<bool> was_;
};

// Kaldi's Posterior (hmm/posterior.h [UPSTREAM-unvendored]; used as such in nnet-loss.cc:78): per frame a list of (pdf-id, weight)
typedef std::vector<std::vector<std::pair<int32, BaseFloat> > > Posterior;

// Xent with the overlay's EvalMasked (google/nnet/nnet-loss.h:33-80, nnet-loss.cc:76-164, Report :293-307).
class Xent {                                    // (not copyable: its buffers are not)
 public:
  Xent() : frames_(0), correct_(0), loss_(0), entropy_(0) {}
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
    poff_.Upload(off);
    ppdf_.Upload(pdf);
    pw_.Upload(w);
    mask_.Upload(frame_mask);
    rx_.Grow((size_t)n * 4); rc_.Grow((size_t)n * 4); re_.Grow((size_t)n * 4);
    diff->Resize(n, d, false);                                                            // :103
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_xent_eval_masked_post(y.Data(), n, d, y.Stride(), poff_.As<int32>(), ppdf_.As<int32>(), pw_.As<BaseFloat>(),
                                       mask_.As<BaseFloat>(), dv.Data(), dv.Stride(), rx_.As<BaseFloat>(), re_.As<BaseFloat>(),
                                       rc_.As<BaseFloat>(), nullptr));
    std::vector<BaseFloat> rx(n), rc(n), re(n);
    rx_.Download(rx.data(), n);
    rc_.Download(rc.data(), n);
    re_.Download(re.data(), n);
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
    tgt_.Upload(target);
    mask_.Upload(frame_mask);
    rx_.Grow((size_t)n * 4); rc_.Grow((size_t)n * 4);
    diff->Resize(n, d, false);                                                            // :103
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_xent_eval_masked(y.Data(), n, d, y.Stride(), tgt_.As<int32>(), mask_.As<BaseFloat>(), dv.Data(), dv.Stride(),
                                  rx_.As<BaseFloat>(), rc_.As<BaseFloat>(), nullptr));
    std::vector<BaseFloat> rx(n), rc(n);
    rx_.Download(rx.data(), n);
    rc_.Download(rc.data(), n);
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
  DeviceBuffer tgt_, mask_, rx_, rc_;
  DeviceBuffer poff_, ppdf_, pw_, re_;             // CSR posterior and per-row target entropy of the general EvalMasked
};

struct TrainLstmStreamsOptions {              // bd-nnet-train-lstm-streams.cc:27-71 (the options that matter)
  NnetTrainOptions trn_opts;
  int32 targets_delay = 5, batch_size = 20, num_stream = 4;
  bool crossvalidate = false;
  BaseFloat dropout_retention = 0.f;                     // the <Dropout> components while training (klstm_dropout.h): 0: the model's own retention
  uint64_t dropout_seed = 0;                             // same seed, same data: the same masks, bit for bit; give every epoch its own
  bool dropout_per_sequence = false;                     // one mask per (stream, sequence) instead of one per element and step
};
struct TrainLstmStreamsStats { int32 num_done = 0; double total_frames = 0, seconds = 0, avg_loss = 0, frame_accuracy = 0; int32 num_minibatches = 0; };

// The while(1) loop of bd-nnet-train-lstm-streams.cc:143-282 on in-memory utterances.
inline TrainLstmStreamsStats TrainLstmStreams(Nnet *nnet, const std::vector<Utterance> &utts, const TrainLstmStreamsOptions &o,
                                              std::string *report = nullptr) {
  nnet->SetTrainOptions(o.trn_opts);                                                  // :104
  DropoutTrainingScope dropout(nnet, o.crossvalidate, o.dropout_retention, o.dropout_seed, o.dropout_per_sequence);
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

// What Ctc, CtcGreedyDecoder, CtcBeamDecoder and CtcAligner do before their C call: the device copy of the lengths, the shape of the
// call, the class weights and the workspace.  (A base for its members only: nothing virtual, and nobody holds a pointer to it.)
class CtcCallBase {
 protected:
  explicit CtcCallBase(int32 blank) : blank_(blank) {}
  void SetClassWeights(const std::vector<BaseFloat> &w) { num_weights_ = (int32)w.size(); w_.Upload(w); }
  const int32 *UploadLens(int32 num_stream, const std::vector<int32> &lens) {      // for the overload that takes them on the device
    KLSTM_ASSERT((int32)lens.size() == num_stream);
    lens_.Upload(lens);
    return lens_.As<int32>();
  }
  // T of net_out [T*num_stream x K].  num_lists: the label or reference lists given, one per stream (or_none: or none at all)
  int32 NumFrames(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, size_t num_lists, bool or_none) const {
    const int32 rows = net_out.NumRows();
    KLSTM_ASSERT(num_stream > 0 && rows > 0 && rows % num_stream == 0 && lens_dev);
    KLSTM_ASSERT((or_none && num_lists == 0) || (int32)num_lists == num_stream);
    KLSTM_ASSERT(num_weights_ == 0 || num_weights_ == net_out.NumCols());
    return rows / num_stream;
  }
  void *Workspace(size_t need) {                     // need: the answer of the call's klstm_ctc_*_workspace_bytes (0: it refused)
    if (need == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    ws_.Grow(need);
    return ws_.As<void>();
  }
  const BaseFloat *Weights() const { return num_weights_ ? w_.As<BaseFloat>() : nullptr; }
  int32 blank_, num_stream_ = 0, rows_ = 0, num_weights_ = 0;      // num_stream_, rows_: of the last call that succeeded
 private:
  DeviceBuffer ws_, lens_, w_;
};

// Label lists as the CSR arrays of the C-ABI on the device: the labels back to back (one 0 where there are none at all, so that the
// array exists) and one offset per list plus the end.  The host keeps the offsets, the number of labels and the longest list.
class PackedLabels {
 public:
  void Upload(const std::vector<std::vector<int32> > &lists) {
    std::vector<int32> flat;
    offsets.assign(1, 0);
    longest = 0;
    for (const auto &l : lists) { flat.insert(flat.end(), l.begin(), l.end()); offsets.push_back((int32)flat.size()); longest = std::max(longest, l.size()); }
    num_labels = flat.size();
    if (flat.empty()) flat.push_back(0);
    lab_.Upload(flat);
    off_.Upload(offsets);
  }
  const int32 *Labels() const { return lab_.As<int32>(); }
  const int32 *Offsets() const { return off_.As<int32>(); }
  std::vector<int32> offsets;
  size_t num_labels = 0, longest = 0;
 private:
  DeviceBuffer lab_, off_;
};

// Connectionist temporal classification on whole utterances (klstm_ctc_eval, klstm.h; not in the reference, whose only objective is
// the frame-level Xent above).  diff is the derivative with respect to the Softmax INPUT, like Xent's (SoftmaxLayer passes it on).
// The statistics stay on the device (four doubles that every Eval adds to) and are read when somebody asks: once per Report().
class Ctc : private CtcCallBase {
 public:
  explicit Ctc(int32 blank = 0) : CtcCallBase(blank) {}

  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle), labels: per stream.  Utterances that
  // cannot be aligned (klstm.h: too short for their labels, a label outside [0, K) or equal to the blank) get zero diff rows and are
  // counted as rejected, on the device.  Only the shape is checked here.
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    Eval(net_out, num_stream, UploadLens(num_stream, lens), labels, diff);
  }
  // the same with the lengths already on the device (the array SetSeqLengths was given)
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    const int32 T = NumFrames(net_out, num_stream, lens_dev, labels.size(), false), K = net_out.NumCols();
    lab_.Upload(labels);
    const size_t need = klstm_ctc_workspace_bytes(T, num_stream, (int)lab_.longest);
    void *ws = Workspace(need);
    loss_.Grow((size_t)num_stream * sizeof(BaseFloat));
    diff->Resize(net_out.NumRows(), K, false);
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_ctc_eval(y.Data(), T, num_stream, K, y.Stride(), lens_dev, lab_.Labels(), lab_.Offsets(), blank_, dv.Data(), dv.Stride(),
                          loss_.As<BaseFloat>(), tot_.Dev(), ws, need, nullptr));
    num_stream_ = num_stream;
  }
  // -log p(labels | x) of the streams of the last Eval (+inf: rejected, 0: idle).  Synchronises.
  void UttLoss(std::vector<BaseFloat> *loss) const { loss->assign(num_stream_, 0.f); loss_.Download(loss->data(), loss->size()); }
  double AvgLoss() const { const double *h = tot_.Read(); return h[0] / h[1]; }                // per utterance counted
  double AvgLossPerFrame() const { const double *h = tot_.Read(); return h[0] / h[3]; }
  double NumUtterances() const { return tot_.Read()[1]; }
  double NumRejected() const { return tot_.Read()[2]; }
  double Frames() const { return tot_.Read()[3]; }
  std::string Report() const {
    const double *h = tot_.Read();                                          // one small copy per question, none per minibatch
    std::ostringstream oss;
    oss << "AvgLoss: " << h[0] / h[1] << " (Ctc) per utterance, " << h[0] / h[3] << " per frame, [" << h[1] << " utterances, " << h[3]
        << " frames, " << h[2] << " rejected]" << std::endl;
    return oss.str();
  }
 private:
  PackedLabels lab_;
  DeviceBuffer loss_;
  DeviceTotals<4> tot_;
};

struct TrainCtcOptions {
  NnetTrainOptions trn_opts;
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, crossvalidate = false;
  BaseFloat dropout_retention = 0.f;                     // the <Dropout> components while training (klstm_dropout.h): 0: the model's own retention
  uint64_t dropout_seed = 0;                             // same seed, same data: the same masks, bit for bit; give every epoch its own
  bool dropout_per_sequence = false;                     // one mask per (stream, sequence) instead of one per element and step
};
struct TrainCtcStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double num_rejected = 0, total_frames = 0, seconds = 0, avg_loss = 0, avg_loss_per_frame = 0;
};

// One pass over the utterances, num_stream whole utterances per minibatch, for unidirectional and bidirectional stacks alike: the
// lengths go to every component (the bidirectional layer needs them), every stream starts from zero state (a unidirectional
// <LstmProjectedStreams> stack through Reset; the bidirectional layer resets itself), and a unidirectional layer simply runs on
// through the padding: padding follows every valid frame.  body sees each minibatch after Propagate: (batch, net_out).  Returns a
// Stats (one of the four below) with num_minibatches, seconds, num_done and num_skipped filled in.
template <class Stats, class Body>
inline Stats ForEachWholeUtteranceBatch(Nnet *nnet, const std::vector<Utterance> &utts, int32 num_stream, bool sort_by_length,
                                        int32 max_frames, Body body) {
  WholeUtteranceBatcher batcher(&utts, num_stream, sort_by_length, max_frames);
  UtteranceBatch b;
  DeviceMatrix feat_dev, nnet_out;
  Stats st;
  std::vector<int> all(num_stream, 1);
  const auto t0 = std::chrono::steady_clock::now();
  while (batcher.Next(&b)) {
    nnet->SetSeqLengths(b.lens);
    nnet->Reset(all);
    feat_dev.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
    nnet->Propagate(feat_dev.View(), &nnet_out);
    body(b, nnet_out);
    st.num_minibatches++;
  }
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.num_done = batcher.NumDone();
  st.num_skipped = batcher.NumSkipped();
  return st;
}

// CTC training: the diff rows of the padding are zero.  every_batch (optional) sees each minibatch after Ctc::Eval: (batch, net_out,
// obj_diff, ctc).
template <class F>
inline TrainCtcStats TrainCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainCtcOptions &o, std::string *report,
                                             F every_batch) {
  nnet->SetTrainOptions(o.trn_opts);
  DropoutTrainingScope dropout(nnet, o.crossvalidate, o.dropout_retention, o.dropout_seed, o.dropout_per_sequence);
  Ctc ctc(o.blank);
  DeviceMatrix obj_diff;
  TrainCtcStats st = ForEachWholeUtteranceBatch<TrainCtcStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
        ctc.Eval(nnet_out, b.num_stream, b.lens, b.labels, &obj_diff);
        every_batch(b, nnet_out, obj_diff, ctc);
        if (!o.crossvalidate) nnet->Backpropagate(obj_diff.View(), nullptr);
      });
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
class CtcGreedyDecoder : private CtcCallBase {
 public:
  explicit CtcGreedyDecoder(int32 blank = 0) : CtcCallBase(blank) {}

  // One weight per class: the winner of a frame is argmax_k y[k] * w[k] (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  using CtcCallBase::SetClassWeights;
  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle); refs: empty (no scoring) or one reference
  // per stream; hyps (optional): the hypothesis of every stream.  Asking for hyps synchronises; the rest stays on the device.
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &refs,
              std::vector<std::vector<int32> > *hyps) {
    Decode(net_out, num_stream, UploadLens(num_stream, lens), refs, hyps);
  }
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &refs,
              std::vector<std::vector<int32> > *hyps) {
    const int32 T = NumFrames(net_out, num_stream, lens_dev, refs.size(), true), rows = net_out.NumRows(), K = net_out.NumCols();
    const bool scoring = !refs.empty();
    const size_t need = klstm_ctc_decode_workspace_bytes(T, num_stream, 0);
    void *ws = Workspace(need);
    hyp_.Grow((size_t)rows * sizeof(int32));
    fc_.Grow((size_t)rows * sizeof(int32));
    hlen_.Grow((size_t)num_stream * sizeof(int32));
    score_.Grow((size_t)num_stream * sizeof(BaseFloat));
    err_.Grow((size_t)num_stream * sizeof(int32));
    if (scoring) refs_.Upload(refs);
    MatrixView y = net_out.View();
    KCheck(klstm_ctc_decode(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, Weights(), hyp_.As<int32>(), hlen_.As<int32>(),
                            score_.As<BaseFloat>(), fc_.As<int32>(), scoring ? refs_.Labels() : nullptr, scoring ? refs_.Offsets() : nullptr,
                            scoring ? err_.As<int32>() : nullptr, scoring ? tot_.Dev() : nullptr, ws, need, nullptr));
    num_stream_ = num_stream; rows_ = rows; scored_ = scoring;
    if (!hyps) return;
    std::vector<int32> n(num_stream), h((size_t)rows);
    hlen_.Download(n.data(), n.size());
    hyp_.Download(h.data(), h.size());
    hyps->assign(num_stream, std::vector<int32>());
    for (int32 s = 0; s < num_stream; s++) (*hyps)[s].assign(h.begin() + (size_t)s * T, h.begin() + (size_t)s * T + n[s]);
  }
  // of the last Decode (each synchronises): path scores, edit distances (-1: not counted; all -1 without references), frame classes
  void UttScores(std::vector<BaseFloat> *v) const { v->assign(num_stream_, 0.f); score_.Download(v->data(), v->size()); }
  void UttErrors(std::vector<int32> *v) const { v->assign(num_stream_, -1); if (scored_) err_.Download(v->data(), v->size()); }
  void FrameClasses(std::vector<int32> *v) const { v->assign(rows_, -1); fc_.Download(v->data(), v->size()); }

  double TokenErrorRate() const { const double *h = tot_.Read(); return h[0] / h[1]; }          // edit errors / reference tokens
  double UtteranceErrorRate() const { const double *h = tot_.Read(); return h[4] / h[3]; }
  double NumUtterances() const { return tot_.Read()[3]; }
  double NumErrors() const { return tot_.Read()[0]; }
  double NumRefTokens() const { return tot_.Read()[1]; }
  double NumHypTokens() const { return tot_.Read()[2]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "UTT_ERROR_RATE: " << 100.0 * h[4] / h[3] << "% [" << h[3] << " utterances, " << h[0] << " errors, " << h[1]
        << " reference tokens, " << h[2] << " hypothesis tokens]" << std::endl;
    oss << "\nTOKEN_ERROR_RATE >> " << 100.0 * h[0] / h[1] << "% <<";
    return oss.str();
  }
 private:
  bool scored_ = false;
  PackedLabels refs_;
  DeviceBuffer hyp_, hlen_, score_, fc_, err_;
  DeviceTotals<5> tot_;
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
    next_.Upload(next);
    weight_.Upload(weight);
    final_.Upload(final_weight);
  }
  int32 NumStates() const { return states_; }
  int32 NumClasses() const { return classes_; }
  const int32 *Next() const { return next_.As<int32>(); }
  const BaseFloat *Weight() const { return weight_.As<BaseFloat>(); }
  const BaseFloat *Final() const { return final_.As<BaseFloat>(); }          // null: no final weights
 private:
  int32 states_, classes_;
  DeviceBuffer next_, weight_, final_;
};

// The host arrays of a sparse back-off language model (klstm_ctc_slm_build, klstm.h): the arcs of the states in CSR
// form with strictly ascending labels, per state a back-off state (-1: none) and its weight, final dense (empty: none).  What
// SparseLm of kaldi-lstm_amd/lm.py holds; ReadArpaLabelLm below fills one from an ARPA file.
struct SparseLabelLm {
  int32 num_classes = 0;
  std::vector<int32> arc_offsets, arc_labels, arc_next, backoff;
  std::vector<BaseFloat> arc_weight, backoff_weight, final_weight;
  int32 NumStates() const { return (int32)backoff.size(); }
};

// A sparse back-off model on the device for CtcBeamDecoder / CtcStreamDecoder::SetLanguageModel: the arrays go up, the build
// validates them there and writes the blob the search walks; Status() (synchronises) is what it dropped or cut, as klstm.h lists it.
class CtcSparseLabelLm {
 public:
  CtcSparseLabelLm(const SparseLabelLm &m, int32 blank) : states_(m.NumStates()), classes_(m.num_classes) {
    const int32 arcs = (int32)m.arc_labels.size();
    KLSTM_ASSERT(states_ >= 1 && arcs >= 1 && m.arc_offsets.size() == (size_t)states_ + 1 && m.arc_next.size() == (size_t)arcs);
    KLSTM_ASSERT(m.arc_weight.size() == (size_t)arcs && m.backoff_weight.size() == (size_t)states_);
    KLSTM_ASSERT(m.final_weight.empty() || m.final_weight.size() == (size_t)states_);
    bytes_ = klstm_ctc_slm_bytes(states_, arcs, classes_);
    if (bytes_ == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    DeviceBuffer off, lab, nxt, wt, bo, bow;
    off.Upload(m.arc_offsets); lab.Upload(m.arc_labels); nxt.Upload(m.arc_next); wt.Upload(m.arc_weight);
    bo.Upload(m.backoff); bow.Upload(m.backoff_weight);
    final_.Upload(m.final_weight);
    blob_.Grow(bytes_);
    status_.Grow(8 * sizeof(int32));
    KCheck(klstm_ctc_slm_build(states_, arcs, classes_, blank, off.As<int32>(), lab.As<int32>(), nxt.As<int32>(), wt.As<BaseFloat>(),
                               bo.As<int32>(), bow.As<BaseFloat>(), blob_.As<void>(), bytes_, status_.As<int32>(), nullptr));
    status_.Download(host_status_, 8);                              // the build has run: the arrays may go
  }
  int32 NumStates() const { return states_; }
  int32 NumClasses() const { return classes_; }
  const void *Blob() const { return blob_.As<void>(); }
  size_t Bytes() const { return bytes_; }
  const BaseFloat *Final() const { return final_.As<BaseFloat>(); }          // null: no final weights
  const int32 *Status() const { return host_status_; }
 private:
  int32 states_, classes_;
  size_t bytes_ = 0;
  DeviceBuffer blob_, final_, status_;
  int32 host_status_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Reads a back-off n-gram in ARPA format into the arrays of a sparse model, as arpa_label_lm of kaldi-lstm_amd/lm.py does from the
// same file: symbols maps a token to its class; n-grams with a token that maps to no class other than the blank are skipped, as are
// those with <s> anywhere but first or </s> anywhere but last.  States are the histories -- every listed n-gram below the highest
// order and every context -- with the <s> history state 0, the empty history state 1 and the others by length, then content; the next
// state is the longest suffix of history + label that is a state; arc weight 10^(alpha logp) e^beta, back-off weight 10^(alpha
// logbow), final = P(</s> | history)^alpha with back-off applied, in double.  Orders up to 9.
inline SparseLabelLm ReadArpaLabelLm(std::istream &is, const std::map<std::string, int32> &symbols, int32 num_classes, int32 blank,
                                     double alpha = 1.0, double beta = 0.0) {
  typedef std::vector<int32> Gram;                                  // -1: <s>, -2: </s>
  std::map<Gram, double> logp, logbow;
  int32 order = 0, n = 0;
  std::string line;
  while (std::getline(is, line)) {
    std::istringstream ls(line);
    std::vector<std::string> f;
    for (std::string tok; ls >> tok;) f.push_back(tok);
    if (f.empty()) continue;
    if (f[0][0] == '\\') {
      const size_t dash = f[0].find('-');
      n = (f[0].size() > 7 && f[0].compare(f[0].size() - 7, 7, "-grams:") == 0) ? std::atoi(f[0].substr(1, dash - 1).c_str()) : 0;
      order = std::max(order, n);
      continue;
    }
    if (n == 0 || (int32)f.size() < n + 1) continue;
    Gram gram;
    bool ok = true;
    for (int32 i = 0; i < n; i++) {
      const std::string &tok = f[1 + i];
      if (tok == "<s>") { ok = ok && i == 0; gram.push_back(-1); }
      else if (tok == "</s>") { ok = ok && i == n - 1; gram.push_back(-2); }
      else {
        const auto it = symbols.find(tok);
        ok = ok && it != symbols.end() && it->second >= 0 && it->second < num_classes && it->second != blank;
        gram.push_back(it != symbols.end() ? it->second : 0);
      }
    }
    if (!ok) continue;
    logp[gram] = std::strtod(f[0].c_str(), nullptr);
    if ((int32)f.size() > n + 1) logbow[gram] = std::strtod(f[n + 1].c_str(), nullptr);
  }
  if (order < 1 || order > 9) KLSTM_ERR("ReadArpaLabelLm: order " << order << " outside 1 to 9");
  auto by_len = [](const Gram &a, const Gram &b) { return a.size() != b.size() ? a.size() < b.size() : a < b; };
  std::set<Gram, decltype(by_len)> hist(by_len);
  hist.insert(Gram());
  for (const auto &kv : logp) {
    const Gram &g = kv.first;
    hist.insert(Gram(g.begin(), g.end() - 1));
    if ((int32)g.size() < order && g.back() != -2) hist.insert(g);
  }
  const Gram start = order > 1 ? Gram(1, -1) : Gram();
  std::vector<Gram> states(1, start);
  if (order > 1) states.push_back(Gram());
  for (const Gram &h : hist)
    if (h != start && !h.empty()) states.push_back(h);
  std::map<Gram, int32> index;
  for (size_t i = 0; i < states.size(); i++) index[states[i]] = (int32)i;
  auto longest = [&](Gram h) {
    while (!index.count(h)) h.erase(h.begin());
    return index[h];
  };
  auto bow_log = [&](const Gram &h) {
    const auto it = logbow.find(h);
    return it == logbow.end() ? 0.0 : it->second;
  };
  std::map<Gram, std::map<int32, double> > arcs;                    // history -> label -> weight
  for (const auto &kv : logp)
    if (kv.first.back() >= 0) arcs[Gram(kv.first.begin(), kv.first.end() - 1)][kv.first.back()] = std::pow(10.0, alpha * kv.second) * std::exp(beta);
  SparseLabelLm m;
  m.num_classes = num_classes;
  m.arc_offsets.push_back(0);
  for (const Gram &h : states) {
    const auto it = arcs.find(h);
    if (it != arcs.end())
      for (const auto &a : it->second) {
        Gram to(h);
        to.push_back(a.first);
        if ((int32)to.size() > order - 1) to.erase(to.begin(), to.end() - (order - 1));
        m.arc_labels.push_back(a.first);
        m.arc_weight.push_back((BaseFloat)a.second);
        m.arc_next.push_back(longest(to));
      }
    m.arc_offsets.push_back((int32)m.arc_labels.size());
    m.backoff.push_back(h.empty() ? -1 : longest(Gram(h.begin() + 1, h.end())));
    m.backoff_weight.push_back(h.empty() ? 1.f : (BaseFloat)std::pow(10.0, alpha * bow_log(h)));
    double acc = 0.0;                                               // log10 P(</s> | h) with back-off applied
    bool found = false;
    for (Gram g(h);; g.erase(g.begin())) {
      Gram e(g);
      e.push_back(-2);
      const auto ep = logp.find(e);
      if (ep != logp.end()) { acc += ep->second; found = true; break; }
      if (g.empty()) break;
      acc += bow_log(g);
    }
    m.final_weight.push_back(found ? (BaseFloat)std::pow(10.0, alpha * acc) : 0.f);
  }
  return m;
}

// What a CtcBeamDecoder's last Decode left on the device: hypotheses [num_stream][nbest][stride], their lengths [num_stream][nbest],
// the entries listed per stream, their edit distances [num_stream][nbest] (null when it had no references), the search's scores
// [num_stream][nbest]
struct CtcNbestDevice { const int32 *hyp, *hyp_len, *count, *errors; int32 num_stream, nbest, stride; const BaseFloat *score; };

// What CtcBeamDecoder and CtcStreamDecoder share on top of CtcCallBase: the sizes of the search, the language model in use, and the
// six totals with their accessors and the report.  (A base for its members only, like CtcCallBase.)
class CtcBeamBase : protected CtcCallBase {
 public:
  // One weight per class: the emission of a frame is y[k] * w[k] (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  using CtcCallBase::SetClassWeights;
  // Fuses a language model into the search: every later call goes through the C call that takes one (klstm_ctc_beam_decode_lm,
  // klstm_ctc_beam_stream_step with its tables) and its scores are the fused ones.  The decoder keeps the pointer, not the tables;
  // null: the search without one, as before.
  void SetLanguageModel(const CtcLabelLm *lm) { lm_ = lm; slm_ = nullptr; }
  // The same with a sparse back-off model (klstm_ctc_beam_decode_slm, klstm_ctc_beam_stream_step_slm); the later of the two calls
  // decides, null: none
  void SetLanguageModel(const CtcSparseLabelLm *slm) { slm_ = slm; lm_ = nullptr; }
  void SetLanguageModel(std::nullptr_t) { lm_ = nullptr; slm_ = nullptr; }

  // over the utterances counted so far (CtcStreamDecoder: emitted with mode 2 and a reference)
  double TokenErrorRate() const { const double *h = tot_.Read(); return h[0] / h[1]; }          // 1-best edit errors / reference tokens
  double OracleTokenErrorRate() const { const double *h = tot_.Read(); return h[5] / h[1]; }    // the best of each list
  double UtteranceErrorRate() const { const double *h = tot_.Read(); return h[4] / h[3]; }
  double NumUtterances() const { return tot_.Read()[3]; }
  double NumErrors() const { return tot_.Read()[0]; }
  double NumOracleErrors() const { return tot_.Read()[5]; }
  double NumRefTokens() const { return tot_.Read()[1]; }
  double NumHypTokens() const { return tot_.Read()[2]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "UTT_ERROR_RATE: " << 100.0 * h[4] / h[3] << "% [" << h[3] << " utterances, " << h[0] << " errors, " << h[1]
        << " reference tokens, " << h[2] << " hypothesis tokens]" << std::endl;
    oss << "ORACLE_TOKEN_ERROR_RATE: " << 100.0 * h[5] / h[1] << "% [" << nbest_ << "-best, beam " << beam_ << ", " << cands_ << " candidates" << how_
        << "]" << std::endl;
    oss << "\nTOKEN_ERROR_RATE >> " << 100.0 * h[0] / h[1] << "% <<";
    return oss.str();
  }
 protected:
  // how: what the report says behind the sizes ("" or ", streaming")
  CtcBeamBase(int32 blank, int32 beam, int32 cands, int32 nbest, const char *how)
      : CtcCallBase(blank), beam_(beam), cands_(cands), nbest_(nbest), how_(how) {}
  int32 beam_, cands_, nbest_;
  const CtcLabelLm *lm_ = nullptr;
  const CtcSparseLabelLm *slm_ = nullptr;
  DeviceTotals<6> tot_;
 private:
  const char *how_;
};

// SetClassWeights, SetLanguageModel, the error rates and Report(): CtcBeamBase
class CtcBeamDecoder : public CtcBeamBase {
 public:
  explicit CtcBeamDecoder(int32 blank = 0, int32 beam = 16, int32 cands = 8, int32 nbest = 1) : CtcBeamBase(blank, beam, cands, nbest, "") {}

  // net_out, lens, refs as CtcGreedyDecoder::Decode takes them; lists (optional): the n-best list of every stream (empty for an idle
  // one).  Asking for lists synchronises; the rest stays on the device.
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &refs,
              std::vector<CtcNbestList> *lists) {
    Decode(net_out, num_stream, UploadLens(num_stream, lens), refs, lists);
  }
  void Decode(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &refs,
              std::vector<CtcNbestList> *lists) {
    const int32 T = NumFrames(net_out, num_stream, lens_dev, refs.size(), true), rows = net_out.NumRows(), K = net_out.NumCols(), N = nbest_;
    KLSTM_ASSERT(nbest_ >= 1);
    const bool scoring = !refs.empty();
    const size_t need = klstm_ctc_beam_workspace_bytes(T, num_stream, beam_, cands_);
    void *ws = Workspace(need);
    hyp_.Grow((size_t)rows * N * sizeof(int32));
    hlen_.Grow((size_t)num_stream * N * sizeof(int32));
    cnt_.Grow((size_t)num_stream * sizeof(int32));
    score_.Grow((size_t)num_stream * N * sizeof(BaseFloat));
    err_.Grow((size_t)num_stream * N * sizeof(int32));
    if (scoring) refs_.Upload(refs);
    const int32 *rl = scoring ? refs_.Labels() : nullptr, *ro = scoring ? refs_.Offsets() : nullptr;
    int32 *er = scoring ? err_.As<int32>() : nullptr;
    double *tot = scoring ? tot_.Dev() : nullptr;
    MatrixView y = net_out.View();
    if (slm_) {
      KLSTM_ASSERT(slm_->NumClasses() == K);
      KCheck(klstm_ctc_beam_decode_slm(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, Weights(), beam_, cands_, N, slm_->Blob(),
                                       slm_->Bytes(), slm_->NumStates(), slm_->Final(), hyp_.As<int32>(), hlen_.As<int32>(), cnt_.As<int32>(),
                                       score_.As<BaseFloat>(), rl, ro, er, tot, ws, need, nullptr));
    } else if (!lm_) {
      KCheck(klstm_ctc_beam_decode(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, Weights(), beam_, cands_, N, hyp_.As<int32>(),
                                   hlen_.As<int32>(), cnt_.As<int32>(), score_.As<BaseFloat>(), rl, ro, er, tot, ws, need, nullptr));
    } else {
      KLSTM_ASSERT(lm_->NumClasses() == K);
      KCheck(klstm_ctc_beam_decode_lm(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, Weights(), beam_, cands_, N, lm_->NumStates(),
                                      lm_->Next(), lm_->Weight(), lm_->Final(), hyp_.As<int32>(), hlen_.As<int32>(), cnt_.As<int32>(),
                                      score_.As<BaseFloat>(), rl, ro, er, tot, ws, need, nullptr));
    }
    num_stream_ = num_stream; scored_ = scoring; frames_ = T;
    if (!lists) return;
    std::vector<int32> c(num_stream), n((size_t)num_stream * N), h((size_t)rows * N), e((size_t)num_stream * N, -1);
    std::vector<BaseFloat> sc((size_t)num_stream * N);
    cnt_.Download(c.data(), c.size());
    hlen_.Download(n.data(), n.size());
    hyp_.Download(h.data(), h.size());
    score_.Download(sc.data(), sc.size());
    if (scoring) err_.Download(e.data(), e.size());
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
  void NbestCounts(std::vector<int32> *v) const { v->assign(num_stream_, 0); cnt_.Download(v->data(), v->size()); }
  void UttScores(std::vector<BaseFloat> *v) const {
    std::vector<int32> c;
    NbestCounts(&c);
    std::vector<BaseFloat> sc((size_t)num_stream_ * nbest_);
    score_.Download(sc.data(), sc.size());
    v->assign(num_stream_, 0.f);
    for (int32 s = 0; s < num_stream_; s++) if (c[s] > 0) (*v)[s] = sc[(size_t)s * nbest_];
  }
  void UttErrors(std::vector<int32> *v) const {
    v->assign(num_stream_, -1);
    if (!scored_) return;
    std::vector<int32> e((size_t)num_stream_ * nbest_);
    err_.Download(e.data(), e.size());
    for (int32 s = 0; s < num_stream_; s++) (*v)[s] = e[(size_t)s * nbest_];
  }

  // the device arrays of the last Decode as klstm_ctc_mbr_eval and klstm_ctc_consensus take them (CtcMbr::Eval, CtcConsensus::Eval), with
  // the shape they were written for
  CtcNbestDevice DeviceLists() const {
    return CtcNbestDevice{hyp_.As<int32>(), hlen_.As<int32>(), cnt_.As<int32>(), scored_ ? err_.As<int32>() : nullptr, num_stream_, nbest_, frames_,
                          score_.As<BaseFloat>()};
  }
 private:
  int32 frames_ = 0;
  bool scored_ = false;
  PackedLabels refs_;
  DeviceBuffer hyp_, hlen_, cnt_, score_, err_;
};

// The prefix beam search fed chunk by chunk (klstm_ctc_beam_stream_step / _emit, klstm.h): num_stream searches whose
// beams live on the device between the calls, for utterances of at most max_frames frames.  Step consumes a chunk of posteriors where
// the scorer leaves it (include/klstm_scorer.hpp BatchScorer::ForEachChunk); Emit reads the current n-best lists and changes nothing,
// so partial results cost one small launch.  For any chunking the lists are CtcBeamDecoder's on the frames consumed so far, bit for
// bit.  The six totals cover the streams emitted with mode 2 and references; they stay on the device and are read when somebody asks.
// SetClassWeights, SetLanguageModel, the error rates and Report(): CtcBeamBase.
class CtcStreamDecoder : public CtcBeamBase {
 public:
  CtcStreamDecoder(int32 blank, int32 beam, int32 cands, int32 nbest, int32 num_stream, int32 max_frames)
      : CtcBeamBase(blank, beam, cands, nbest, ", streaming"), max_frames_(max_frames) {
    num_stream_ = num_stream;
    KLSTM_ASSERT(nbest >= 1);
    state_bytes_ = klstm_ctc_beam_stream_state_bytes(max_frames, num_stream, beam);      // host only: a refused shape needs no GPU
    if (state_bytes_ == 0) KLSTM_ERR("klstm: " << klstm_last_error());
  }
  int32 NumStream() const { return num_stream_; }
  int32 MaxFrames() const { return max_frames_; }

  // chunk [T*num_stream x K], rows t * num_stream + s; lens[s]: the frames of THIS chunk for stream s (0: idle, its state is not
  // touched); start[s] != 0: a new utterance begins in stream s with this chunk (empty: no stream starts).  A stream whose utterance
  // would pass max_frames is rejected for the call and Emit reports frames = -1 - frames.  Asynchronous.
  void Step(const DeviceMatrix &chunk, const std::vector<int32> &lens, const std::vector<int32> &start) {
    const int32 S = num_stream_;
    KLSTM_ASSERT(start.empty() || (int32)start.size() == S);
    const int32 *lens_dev = UploadLens(S, lens);
    const int32 T = NumFrames(chunk, S, lens_dev, 0, true), K = chunk.NumCols();
    KLSTM_ASSERT(!lm_ || lm_->NumClasses() == K);
    if (!start.empty()) start_.Upload(start);
    const size_t need = klstm_ctc_beam_stream_workspace_bytes(T, S, cands_, nbest_);
    void *ws = Workspace(need);
    MatrixView y = chunk.View();
    if (slm_) {
      KLSTM_ASSERT(slm_->NumClasses() == K);
      KCheck(klstm_ctc_beam_stream_step_slm(y.Data(), T, S, K, y.Stride(), lens_dev, start.empty() ? nullptr : start_.As<int32>(), blank_, Weights(),
                                            beam_, cands_, slm_->Blob(), slm_->Bytes(), slm_->NumStates(), State(), state_bytes_, max_frames_, ws,
                                            need, nullptr));
      classes_ = K;
      return;
    }
    KCheck(klstm_ctc_beam_stream_step(y.Data(), T, S, K, y.Stride(), lens_dev, start.empty() ? nullptr : start_.As<int32>(), blank_, Weights(),
                                      beam_, cands_, lm_ ? lm_->NumStates() : 0, lm_ ? lm_->Next() : nullptr, lm_ ? lm_->Weight() : nullptr,
                                      State(), state_bytes_, max_frames_, ws, need, nullptr));
    classes_ = K;
  }
  // mode[s]: 0 skip stream s, 1 its list without the language model's final weights, 2 with them (the list CtcBeamDecoder makes).
  // refs: empty, or one reference per stream (those of the streams emitted with mode 2 are counted).  lists / frames / stable_len
  // (each optional; asking synchronises): per stream the n-best list (empty where skipped), the frames consumed (-1 - frames after
  // an overflow) and the number of leading tokens of the 1-best that can no longer change.  Changes nothing in the state.
  void Emit(const std::vector<int32> &mode, const std::vector<std::vector<int32> > &refs, std::vector<CtcNbestList> *lists,
            std::vector<int32> *frames, std::vector<int32> *stable_len) {
    const int32 S = num_stream_, N = nbest_;
    KLSTM_ASSERT((int32)mode.size() == S && (refs.empty() || (int32)refs.size() == S));
    if (classes_ == 0) KLSTM_ERR("CtcStreamDecoder::Emit before the first Step");
    const bool scoring = !refs.empty();
    mode_.Upload(mode);
    const size_t need = klstm_ctc_beam_stream_workspace_bytes(1, S, 1, N);
    void *ws = Workspace(need);
    hyp_.Grow((size_t)S * N * max_frames_ * sizeof(int32));
    hlen_.Grow((size_t)S * N * sizeof(int32));
    cnt_.Grow((size_t)S * sizeof(int32));
    score_.Grow((size_t)S * N * sizeof(BaseFloat));
    err_.Grow((size_t)S * N * sizeof(int32));
    fr_.Grow((size_t)S * sizeof(int32));
    stab_.Grow((size_t)S * sizeof(int32));
    KCheck(klstm_memset_zero(stab_.As<int32>(), (size_t)S * sizeof(int32), nullptr));     // a skipped stream's is not written
    if (scoring) refs_.Upload(refs);
    KCheck(klstm_ctc_beam_stream_emit(S, classes_, blank_, beam_, N, mode_.As<int32>(), slm_ ? 1 : lm_ ? lm_->NumStates() : 0,
                                      slm_ ? slm_->Final() : lm_ ? lm_->Final() : nullptr,            // (emit reads the final weights alone)
                                      State(), state_bytes_, max_frames_, hyp_.As<int32>(), max_frames_, hlen_.As<int32>(), cnt_.As<int32>(),
                                      score_.As<BaseFloat>(), fr_.As<int32>(), stab_.As<int32>(), scoring ? refs_.Labels() : nullptr,
                                      scoring ? refs_.Offsets() : nullptr, scoring ? err_.As<int32>() : nullptr,
                                      scoring ? tot_.Dev() : nullptr, ws, need, nullptr));
    if (frames) { frames->assign(S, 0); fr_.Download(frames->data(), frames->size()); }
    if (stable_len) { stable_len->assign(S, 0); stab_.Download(stable_len->data(), stable_len->size()); }
    if (!lists) return;
    std::vector<int32> c(S), n((size_t)S * N), e((size_t)S * N, -1), h((size_t)S * N * max_frames_);
    std::vector<BaseFloat> sc((size_t)S * N);
    cnt_.Download(c.data(), c.size());
    hlen_.Download(n.data(), n.size());
    hyp_.Download(h.data(), h.size());
    score_.Download(sc.data(), sc.size());
    if (scoring) err_.Download(e.data(), e.size());
    lists->assign(S, CtcNbestList());
    for (int32 s = 0; s < S; s++)
      for (int32 q = 0; q < c[s]; q++) {
        const size_t o = (size_t)s * N + q;
        CtcHypothesis hy;
        hy.tokens.assign(h.begin() + o * max_frames_, h.begin() + o * max_frames_ + n[o]);
        hy.score = sc[o];
        hy.errors = e[o];
        (*lists)[s].push_back(hy);
      }
  }
 private:
  void *State() {                                       // zero-filled: "nothing yet" in every stream
    if (!state_.As<void>()) {
      state_.Grow(state_bytes_);
      KCheck(klstm_memset_zero(state_.As<void>(), state_bytes_, nullptr));
    }
    return state_.As<void>();
  }
  int32 max_frames_, classes_ = 0;
  size_t state_bytes_ = 0;
  PackedLabels refs_;
  DeviceBuffer state_, start_, mode_, hyp_, hlen_, cnt_, score_, err_, fr_, stab_;
};

// Minimum expected token error over the n-best lists of a CtcBeamDecoder (klstm_ctc_mbr_eval, klstm.h): the
// sequence-discriminative objective that follows CTC training.  With P = softmax over a stream's list of risk_scale * log p(h | y)
// and R = sum P errors, diff is the derivative of R + ctc_weight * (-log p(ref | y)) with respect to the Softmax INPUT, like Ctc's.
// The six totals stay on the device and are read when somebody asks.
class CtcMbr : private CtcCallBase {
 public:
  // max_hyp_len: the longest labelling the workspace serves (longer list entries are dropped); 0: min(1023, 2 * longest reference + 8)
  explicit CtcMbr(int32 blank = 0, BaseFloat risk_scale = 1.f, BaseFloat ctc_weight = 0.f, int32 max_hyp_len = 0)
      : CtcCallBase(blank), risk_scale_(risk_scale), ctc_weight_(ctc_weight), max_hyp_len_(max_hyp_len) {}

  // net_out, lens as Ctc::Eval takes them, and the SAME as the last lists.Decode(net_out, ..., refs, ...) took, which must have had
  // the references (its edit distances are the costs); refs: one list per stream.  Everything is decided on the device (klstm.h):
  // dropped entries, idle / rejected / skipped streams get zero diff rows.
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const CtcBeamDecoder &lists,
            const std::vector<std::vector<int32> > &refs, DeviceMatrix *diff) {
    Eval(net_out, num_stream, UploadLens(num_stream, lens), lists, refs, diff);
  }
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const CtcBeamDecoder &lists,
            const std::vector<std::vector<int32> > &refs, DeviceMatrix *diff) {
    const CtcNbestDevice nb = lists.DeviceLists();
    const int32 T = NumFrames(net_out, num_stream, lens_dev, refs.size(), false), K = net_out.NumCols(), N = nb.nbest;
    KLSTM_ASSERT(nb.num_stream == num_stream && nb.stride == T && nb.errors);
    refs_.Upload(refs);
    const bool with_ref = ctc_weight_ > 0.f;
    const int32 max_len = max_hyp_len_ > 0 ? max_hyp_len_ : (int32)std::min<size_t>(1023, 2 * refs_.longest + 8);
    const size_t need = klstm_ctc_mbr_workspace_bytes(T, num_stream, N, max_len, with_ref);
    void *ws = Workspace(need);
    risk_.Grow((size_t)num_stream * sizeof(BaseFloat));
    logp_.Grow((size_t)num_stream * N * sizeof(BaseFloat));
    diff->Resize(net_out.NumRows(), K, false);
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_ctc_mbr_eval(y.Data(), T, num_stream, K, y.Stride(), lens_dev, blank_, nb.hyp, nb.stride, nb.hyp_len, nb.count, nb.errors, N, with_ref ? refs_.Labels() : nullptr,
                              with_ref ? refs_.Offsets() : nullptr, risk_scale_, ctc_weight_, dv.Data(), dv.Stride(), risk_.As<BaseFloat>(),
                              logp_.As<BaseFloat>(), nullptr, nullptr, tot_.Dev(), ws, need, nullptr));
    num_stream_ = num_stream; nbest_ = N;
  }
  // of the last Eval (each synchronises): the expected errors per stream (0: idle, -1: rejected or skipped); log p(h_q | y) per
  // stream and list slot, [S][N] (-inf: dropped or not listed)
  void UttRisk(std::vector<BaseFloat> *v) const { v->assign(num_stream_, 0.f); risk_.Download(v->data(), v->size()); }
  void HypLogp(std::vector<BaseFloat> *v) const { v->assign((size_t)num_stream_ * nbest_, 0.f); logp_.Download(v->data(), v->size()); }
  double AvgRisk() const { const double *h = tot_.Read(); return h[0] / h[2]; }                 // expected errors per utterance counted
  double AvgFirstBestErrors() const { const double *h = tot_.Read(); return h[1] / h[2]; }
  double NumUtterances() const { return tot_.Read()[2]; }
  double NumRejectedOrSkipped() const { return tot_.Read()[3]; }
  double Frames() const { return tot_.Read()[4]; }
  double AvgRefLoss() const { const double *h = tot_.Read(); return h[5] / h[2]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "AvgRisk: " << h[0] / h[2] << " expected errors per utterance (1-best: " << h[1] / h[2] << "), reference loss " << h[5] / h[2]
        << " per utterance, [" << h[2] << " utterances, " << h[4] << " frames, " << h[3] << " rejected or skipped]" << std::endl;
    return oss.str();
  }
 private:
  BaseFloat risk_scale_, ctc_weight_;
  int32 max_hyp_len_, nbest_ = 0;
  PackedLabels refs_;
  DeviceBuffer risk_, logp_;
  DeviceTotals<6> tot_;
};

inline int32 CtcNbestMaxLen(int32 max_len, int32 stride) { return max_len > 0 ? max_len : std::min<int32>(1023, stride); }      // the token capacity of CtcConsensus, CtcRescorer
// Minimum Bayes risk decoding and unit confidences over the n-best lists of a CtcBeamDecoder (klstm_ctc_consensus, klstm.h, which
// defines every quantity): per stream the entry of the list with the smallest expected unit errors under the
// list's own posterior (or the most probable one), and for each of its tokens or words the posterior mass of the entries that agree
// with it.  Reads the lists where Decode left them; the ten totals stay on the device and are read when somebody asks.
class CtcConsensus : private CtcCallBase {
 public:
  // mbr_pivot: answer with the MBR entry (false: the MAP entry, with confidences); scale multiplies the log weights; separator: -1
  // for token units, otherwise the class that separates words; max_len: the token capacity, 0: min(1023, the lists' stride)
  explicit CtcConsensus(bool mbr_pivot = true, BaseFloat scale = 1.f, int32 separator = -1, int32 max_len = 0)
      : CtcCallBase(0), mbr_pivot_(mbr_pivot), scale_(scale), separator_(separator), max_len_(max_len) {}

  // over the lists of the last lists.Decode; logp_dev: [num_stream][nbest] natural-log weights on the device (CtcMbr's log p(h | y),
  // say), null: the search's scores.  Nothing synchronises.
  void Eval(const CtcBeamDecoder &lists, const BaseFloat *logp_dev = nullptr) { Eval(lists.DeviceLists(), logp_dev); }
  // ... over any lists in that layout: CtcRescorer::DeviceLists(), the re-ranked ones
  void Eval(const CtcNbestDevice &nb, const BaseFloat *logp_dev = nullptr) {
    const int32 S = nb.num_stream, N = nb.nbest;
    KLSTM_ASSERT(S > 0 && N > 0 && nb.stride > 0);
    const int32 max_len = CtcNbestMaxLen(max_len_, nb.stride);
    const size_t need = klstm_ctc_consensus_workspace_bytes(S, N, max_len, separator_ >= 0);
    void *ws = Workspace(need);
    idx_.Grow((size_t)S * 3 * sizeof(int32));
    post_.Grow((size_t)S * N * sizeof(BaseFloat));
    risk_.Grow((size_t)S * N * sizeof(BaseFloat));
    ulen_.Grow((size_t)S * N * sizeof(int32));
    conf_.Grow((size_t)S * nb.stride * sizeof(BaseFloat));
    int32 *idx = idx_.As<int32>();
    KCheck(klstm_ctc_consensus(nb.hyp, nb.stride, nb.hyp_len, nb.count, logp_dev ? logp_dev : nb.score, nb.errors, S, N, max_len, scale_,
                               separator_, mbr_pivot_ ? 1 : 0, idx, idx + S, idx + 2 * S, post_.As<BaseFloat>(), risk_.As<BaseFloat>(),
                               ulen_.As<int32>(), conf_.As<BaseFloat>(), nb.stride, nullptr, tot_.Dev(), ws, need, nullptr));
    num_stream_ = S; nbest_ = N; stride_ = nb.stride;
  }
  // of the last Eval (each synchronises), per stream: the entry answered with, the MAP and the MBR entry (-1: idle or rejected)
  void Picks(std::vector<int32> *pick, std::vector<int32> *map = nullptr, std::vector<int32> *mbr = nullptr) const {
    std::vector<int32> v((size_t)3 * num_stream_);
    idx_.Download(v.data(), v.size());
    pick->assign(v.begin(), v.begin() + num_stream_);
    if (map) map->assign(v.begin() + num_stream_, v.begin() + 2 * num_stream_);
    if (mbr) mbr->assign(v.begin() + 2 * num_stream_, v.end());
  }
  // ... the confidence of every unit of the entry answered with (empty: none), and its expected unit errors (-1: none)
  void Confidences(std::vector<std::vector<BaseFloat> > *conf, std::vector<BaseFloat> *pick_risk = nullptr) const {
    std::vector<int32> pick, ulen((size_t)num_stream_ * nbest_);
    Picks(&pick);
    ulen_.Download(ulen.data(), ulen.size());
    std::vector<BaseFloat> c((size_t)num_stream_ * stride_), r((size_t)num_stream_ * nbest_);
    conf_.Download(c.data(), c.size());
    risk_.Download(r.data(), r.size());
    conf->assign(num_stream_, std::vector<BaseFloat>());
    if (pick_risk) pick_risk->assign(num_stream_, -1.f);
    for (int32 s = 0; s < num_stream_; s++) {
      if (pick[s] < 0) continue;
      const size_t o = (size_t)s * nbest_ + pick[s];
      (*conf)[s].assign(c.begin() + (size_t)s * stride_, c.begin() + (size_t)s * stride_ + ulen[o]);
      if (pick_risk) (*pick_risk)[s] = r[o];
    }
  }
  // over the streams done so far
  double ExpectedErrors() const { const double *h = tot_.Read(); return h[2] / h[0]; }          // of the entry answered with, per utterance
  double MapExpectedErrors() const { const double *h = tot_.Read(); return h[3] / h[0]; }       // of the most probable entry
  double MeanConfidence() const { const double *h = tot_.Read(); return h[6] / h[5]; }          // over the units answered with
  double NumUtterances() const { return tot_.Read()[0]; }
  double NumPickErrors() const { return tot_.Read()[8]; }                                       // edit errors of the entries answered with (lists decoded with references)
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "EXPECTED_ERRORS: " << h[2] / h[0] << " per utterance (" << (mbr_pivot_ ? "MBR" : "MAP") << " entry; MAP entry: " << h[3] / h[0] << "), "
        << (separator_ >= 0 ? "words" : "tokens") << ", mean confidence " << h[6] / h[5] << " [" << h[0] << " utterances, " << h[1]
        << " idle or rejected, " << h[4] << " where the MBR entry is not the MAP entry, " << h[5] << " units, " << h[7] << " entries dropped, "
        << h[8] << " errors (MAP entry: " << h[9] << ")]" << std::endl;
    return oss.str();
  }
 private:
  bool mbr_pivot_;
  BaseFloat scale_;
  int32 separator_, max_len_, nbest_ = 0, stride_ = 0;
  DeviceBuffer idx_, post_, risk_, ulen_, conf_;
  DeviceTotals<10> tot_;
};

// The key a word is known by on the device (klstm_ctc_consensus, klstm_ctc_nbest_rescore; word_key of kaldi-lstm_amd/lm.py): the hash the
// beam search knows its prefixes by, folded over the word's tokens.
inline uint64_t CtcWordKey(const std::vector<int32> &tokens) {
  uint64_t h = KLSTM_CTC_HASH_START;
  for (int32 c : tokens) {
    const uint64_t x = (h ^ (uint64_t)(uint32_t)(c + 1)) * KLSTM_CTC_HASH_MUL;
    h = x ^ (x >> 29);
  }
  return h;
}

// The word table of a CtcRescorer on the device (klstm_ctc_nbest_rescore, klstm.h): the words of a vocabulary, each a
// non-empty run of token classes other than the separator, with the class of each in the word model (empty ids: its position), sorted
// by key.  unk_id: the class an unknown word takes (negative: it forbids the entry).  Two words that share a key are an error.
class CtcWordTable {
 public:
  CtcWordTable(const std::vector<std::vector<int32> > &words, int32 separator, int32 unk_id, const std::vector<int32> &ids = std::vector<int32>())
      : unk_id_(unk_id), separator_(separator) {
    KLSTM_ASSERT(!words.empty() && separator >= 0 && (ids.empty() || ids.size() == words.size()));
    std::map<uint64_t, int32> by_key;
    for (size_t i = 0; i < words.size(); i++) {
      KLSTM_ASSERT(!words[i].empty());
      for (int32 c : words[i]) KLSTM_ASSERT(c >= 0 && c != separator);
      if (!by_key.insert(std::make_pair(CtcWordKey(words[i]), ids.empty() ? (int32)i : ids[i])).second)
        KLSTM_ERR("CtcWordTable: word " << i << " shares its key with an earlier word");
    }
    for (const auto &kv : by_key) { keys_.push_back(kv.first); ids_.push_back(kv.second); }
    dkeys_.Upload(keys_);
    dids_.Upload(ids_);
  }
  int32 NumWords() const { return (int32)keys_.size(); }
  int32 UnkId() const { return unk_id_; }
  int32 Separator() const { return separator_; }
  const std::vector<uint64_t> &Keys() const { return keys_; }        // ascending
  const std::vector<int32> &Ids() const { return ids_; }
  const unsigned long long *KeysDev() const { return dkeys_.As<unsigned long long>(); }
  const int32 *IdsDev() const { return dids_.As<int32>(); }
 private:
  int32 unk_id_, separator_;
  std::vector<uint64_t> keys_;
  std::vector<int32> ids_;
  DeviceBuffer dkeys_, dids_;
};

// Second-pass rescoring of the n-best lists of a CtcBeamDecoder (klstm_ctc_nbest_rescore, klstm.h, which defines every quantity;
// INTEGRATION.md 3n): the score of `sub`, the token model the first pass fused, is taken out and the score of `add` is put in -- a
// token model, or with a word table a model over word classes whose reserved class is add_reserved, the blank it was built with.  The
// re-ranked lists stay on the device in the layout of the search's (DeviceLists(): CtcConsensus::Eval and CtcMbr take them); the eight
// totals stay there too and are read when somebody asks.  The models and the table are not owned.
class CtcRescorer : private CtcCallBase {
 public:
  // num_classes: the token classes K; either model may be null, not both; max_len: the token capacity, 0: min(1023, the lists' stride)
  CtcRescorer(int32 num_classes, const CtcSparseLabelLm *add, const CtcSparseLabelLm *sub, const CtcWordTable *words = nullptr,
              int32 add_reserved = -1, BaseFloat am_scale = 1.f, BaseFloat add_scale = 1.f, BaseFloat unit_bonus = 0.f, int32 max_len = 0)
      : CtcCallBase(0), classes_(num_classes), add_(add), sub_(sub), words_(words), add_reserved_(add_reserved), am_scale_(am_scale),
        add_scale_(add_scale), unit_bonus_(unit_bonus), max_len_(max_len) {
    KLSTM_ASSERT((add || sub) && (!words || add));
  }
  // over the lists of the last lists.Decode.  Nothing synchronises.
  void Eval(const CtcBeamDecoder &lists) { Eval(lists.DeviceLists()); }
  void Eval(const CtcNbestDevice &nb) {
    const int32 S = nb.num_stream, N = nb.nbest;
    KLSTM_ASSERT(S > 0 && N > 0 && nb.stride > 0 && nb.score);
    const int32 max_len = CtcNbestMaxLen(max_len_, nb.stride);
    const size_t need = klstm_ctc_rescore_workspace_bytes(S, N, max_len, words_ ? 1 : 0);
    void *ws = Workspace(need);
    const size_t SN = (size_t)S * N;
    order_.Grow(SN * sizeof(int32)); live_.Grow((size_t)S * sizeof(int32)); score_.Grow(SN * sizeof(BaseFloat));
    addlp_.Grow(SN * sizeof(BaseFloat)); sublp_.Grow(SN * sizeof(BaseFloat)); units_.Grow(SN * sizeof(int32)); oov_.Grow(SN * sizeof(int32));
    ohyp_.Grow(SN * nb.stride * sizeof(int32)); olen_.Grow(SN * sizeof(int32)); ocnt_.Grow((size_t)S * sizeof(int32));
    oscore_.Grow(SN * sizeof(BaseFloat)); oerr_.Grow(SN * sizeof(int32));
    KCheck(klstm_ctc_nbest_rescore(nb.hyp, nb.stride, nb.hyp_len, nb.count, nb.score, nb.errors, S, N, max_len, classes_,
                                   sub_ ? sub_->Blob() : nullptr, sub_ ? sub_->Bytes() : 0, sub_ ? sub_->NumStates() : 0, sub_ ? sub_->Final() : nullptr,
                                   add_ ? add_->Blob() : nullptr, add_ ? add_->Bytes() : 0, add_ ? add_->NumStates() : 0,
                                   add_ ? add_->NumClasses() : 0, add_ ? add_->Final() : nullptr, words_ ? words_->KeysDev() : nullptr,
                                   words_ ? words_->IdsDev() : nullptr, words_ ? words_->NumWords() : 0, words_ ? words_->UnkId() : -1,
                                   words_ ? words_->Separator() : -1, words_ ? add_reserved_ : -1, am_scale_, add_scale_, unit_bonus_,
                                   order_.As<int32>(), live_.As<int32>(), score_.As<BaseFloat>(), addlp_.As<BaseFloat>(), sublp_.As<BaseFloat>(),
                                   units_.As<int32>(), oov_.As<int32>(), N, ohyp_.As<int32>(), nb.stride, olen_.As<int32>(), ocnt_.As<int32>(),
                                   oscore_.As<BaseFloat>(), nb.errors ? oerr_.As<int32>() : nullptr, tot_.Dev(), ws, need, nullptr));
    num_stream_ = S; nbest_ = N; stride_ = nb.stride; scored_ = nb.errors != nullptr;
  }
  // the re-ranked lists of the last Eval on the device, in the layout of CtcBeamDecoder::DeviceLists(); slots beyond a stream's count
  // hold nothing
  CtcNbestDevice DeviceLists() const {
    return CtcNbestDevice{ohyp_.As<int32>(), olen_.As<int32>(), ocnt_.As<int32>(), scored_ ? oerr_.As<int32>() : nullptr, num_stream_, nbest_, stride_,
                          oscore_.As<BaseFloat>()};
  }
  // of the last Eval (each synchronises): the re-ranked list of every stream, best first, with the new scores
  void Lists(std::vector<CtcNbestList> *lists) const {
    const size_t SN = (size_t)num_stream_ * nbest_;
    std::vector<int32> c(num_stream_), n(SN), h(SN * stride_), e(SN, -1);
    std::vector<BaseFloat> sc(SN);
    ocnt_.Download(c.data(), c.size()); olen_.Download(n.data(), n.size()); ohyp_.Download(h.data(), h.size());
    oscore_.Download(sc.data(), sc.size());
    if (scored_) oerr_.Download(e.data(), e.size());
    lists->assign(num_stream_, CtcNbestList());
    for (int32 s = 0; s < num_stream_; s++)
      for (int32 q = 0; q < c[s]; q++) {
        const size_t o = (size_t)s * nbest_ + q;
        CtcHypothesis hy;
        hy.tokens.assign(h.begin() + o * stride_, h.begin() + o * stride_ + n[o]);
        hy.score = sc[o];
        hy.errors = e[o];
        (*lists)[s].push_back(hy);
      }
  }
  // ... the entry of the search's list at every rank [num_stream][nbest] (-1 beyond the entries ranked) and how many were ranked
  void Order(std::vector<int32> *order, std::vector<int32> *live = nullptr) const {
    order->assign((size_t)num_stream_ * nbest_, -1);
    order_.Download(order->data(), order->size());
    if (live) { live->assign(num_stream_, 0); live_.Download(live->data(), live->size()); }
  }
  // ... per entry of the search's list [num_stream][nbest]: the new score (-inf: dropped, forbidden or unlisted), the log weights of
  // `add` and `sub`, the units and the words out of vocabulary (any may be null)
  void Entries(std::vector<BaseFloat> *score, std::vector<BaseFloat> *add_logp = nullptr, std::vector<BaseFloat> *sub_logp = nullptr,
               std::vector<int32> *units = nullptr, std::vector<int32> *oov = nullptr) const {
    const size_t SN = (size_t)num_stream_ * nbest_;
    if (score) { score->assign(SN, 0.f); score_.Download(score->data(), SN); }
    if (add_logp) { add_logp->assign(SN, 0.f); addlp_.Download(add_logp->data(), SN); }
    if (sub_logp) { sub_logp->assign(SN, 0.f); sublp_.Download(sub_logp->data(), SN); }
    if (units) { units->assign(SN, 0); units_.Download(units->data(), SN); }
    if (oov) { oov->assign(SN, 0); oov_.Download(oov->data(), SN); }
  }
  // over the streams rescored so far
  double NumUtterances() const { return tot_.Read()[0]; }
  double NumChanged() const { return tot_.Read()[4]; }                 // streams whose 1-best is no longer the search's
  double NumFirstPassErrors() const { return tot_.Read()[5]; }         // edit errors of the search's 1-best (lists decoded with references)
  double NumRescoredErrors() const { return tot_.Read()[6]; }          // ... of the new 1-best
  double NumDropped() const { return tot_.Read()[2]; }
  double NumForbidden() const { return tot_.Read()[3]; }
  double NumOovWords() const { return tot_.Read()[7]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "RESCORED: " << h[4] << " of " << h[0] << " 1-bests changed, errors " << h[5] << " -> " << h[6] << " [" << (words_ ? "words" : "tokens")
        << ", " << h[1] << " idle or rejected, " << h[2] << " entries dropped, " << h[3] << " forbidden, " << h[7] << " words out of vocabulary]"
        << std::endl;
    return oss.str();
  }
 private:
  int32 classes_;
  const CtcSparseLabelLm *add_, *sub_;
  const CtcWordTable *words_;
  int32 add_reserved_;
  BaseFloat am_scale_, add_scale_, unit_bonus_;
  int32 max_len_, nbest_ = 0, stride_ = 0;
  bool scored_ = false;
  DeviceBuffer order_, live_, score_, addlp_, sublp_, units_, oov_, ohyp_, olen_, ocnt_, oscore_, oerr_;
  DeviceTotals<8> tot_;
};

// Rescoring of the same lists with an LSTM language model (the knlm_* entries, klstm_nlm.h, which defines every quantity; INTEGRATION.md
// 3o).  The LM is an Nnet over V >= K classes, of which 0 .. num_classes - 1 are the CTC model's tokens:
//   [<AffineTransform> D x V]  <LstmProjectedStreams | LstmProjected>...  <AffineTransform> V x R  [<Softmax>]
// the leading Affine an embedding (gathered, never multiplied), a Softmax folded into the scoring.  The model is only read: the rescorer
// builds engines of its own with NumStream = num_stream from the model's current parameters, as BatchScorer does.
struct CtcNeuralRescorerOptions {
  int32 num_stream = 16, chunk = 20;     // E entries are scored at a time, in chunks of T positions
  int32 num_classes = 0;                 // the token classes K; 0: all V classes of the LM
  int32 bos = 0, eos = 0;                // classes of the LM; eos < 0: no end term.  bos = eos = blank with V = K is the economical choice
  BaseFloat am_scale = 1.f, nlm_scale = 1.f, unit_bonus = 0.f;
  int32 out_n = 0;                       // entries the re-ranked list keeps; 0: all
  int32 max_len = 0;                     // the token capacity the plan is laid out for; 0: min(1023, the lists' stride)
  int device = 0;
};
class CtcNeuralRescorer {
 public:
  CtcNeuralRescorer(const Nnet &lm, const CtcNeuralRescorerOptions &o) : o_(o) {
    int32 i0 = 0, i1 = 0;
    CheckTopology(lm, o, &i0, &i1);                   // (before anything touches a device: a refused model needs no GPU)
    const AffineLayer &aff = static_cast<const AffineLayer &>(lm.GetComponent(i1));
    V_ = aff.OutputDim(); aff_in_ = aff.InputDim();
    K_ = o.num_classes > 0 ? o.num_classes : V_;
    cols_ = lm.GetComponent(i0).InputDim();
    for (int32 i = i0; i < i1; i++) {
      const LstmProjectedStreams *c = static_cast<const LstmLayer &>(lm.GetComponent(i)).Impl();
      std::vector<BaseFloat> p;
      c->GetParams(&p);
      klstm_engine *e = nullptr;
      KCheck(klstm_create(c->InputDim(), c->CellDim(), c->OutputDim(), o.num_stream, o.device, nullptr, &e));
      engines_.emplace_back(e);
      KCheck(klstm_set_params_host(e, p.data()));
      KCheck(klstm_set_option(e, "persist_verify", 1));   // a persistent launch that gives up is run again inside its call: the buffers are reused
      dims_.push_back(c->OutputDim());
    }
    std::vector<BaseFloat> w, b;
    aff.HostParams(&w, &b);
    W_.Upload(w); b_.Upload(b);
    if (i0 == 1) {
      static_cast<const AffineLayer &>(lm.GetComponent(0)).HostParams(&w, &b);
      We_.Upload(w); be_.Upload(b);
    }
    embed_ = i0 == 1;
    const size_t rows = (size_t)o.num_stream * o.chunk;       // tight rows, as kaldi_lstm_amd.nlm lays them out: the same kernels, the same bits
    x_.Grow(rows * cols_ * sizeof(BaseFloat));
    for (int32 d : dims_) { h_.emplace_back(); h_.back().Grow(rows * d * sizeof(BaseFloat)); }
    a_.Grow(rows * V_ * sizeof(BaseFloat));
    ws_bytes_ = knlm_workspace_bytes(o.num_stream, o.chunk);
    if (!ws_bytes_) KLSTM_ERR("klstm: " << klstm_last_error());
    ws_.Grow(ws_bytes_);
  }
  // The checks of the constructor, host only; [*lstm_begin, *lstm_end) are the LSTM components, *lstm_end the last <AffineTransform>,
  // *lstm_begin == 1 with an embedding.  Raises (KLSTM_ERR) on a topology or an option the rescorer does not take.
  static void CheckTopology(const Nnet &lm, const CtcNeuralRescorerOptions &o, int32 *lstm_begin = nullptr, int32 *lstm_end = nullptr) {
    if (o.num_stream < 1 || o.num_stream > 32 || o.chunk < 1) KLSTM_ERR("CtcNeuralRescorer: num_stream must be 1..32 and chunk >= 1");
    const int32 n = lm.NumComponents();
    auto marker = [&](int32 i) { return i < n ? std::string(lm.GetComponent(i).Marker()) : std::string("(end of the model)"); };
    auto hint = [&](int32 i) { return marker(i) == "<Dropout>" ? " (pass the model through WithoutDropout first)" : ""; };
    int32 i = marker(0) == "<AffineTransform>" ? 1 : 0;
    const int32 b = i;
    while (marker(i) == "<LstmProjectedStreams>" || marker(i) == "<LstmProjected>") i++;
    if (i == b) KLSTM_ERR("CtcNeuralRescorer: " << marker(i) << " at component " << i << " where an <LstmProjectedStreams> / <LstmProjected> belongs" << hint(i));
    if (marker(i) != "<AffineTransform>") KLSTM_ERR("CtcNeuralRescorer: " << marker(i) << " at component " << i << " where the <AffineTransform> belongs" << hint(i));
    const int32 e = i++;
    if (marker(i) == "<Softmax>") i++;
    if (i != n) KLSTM_ERR("CtcNeuralRescorer: " << marker(i) << " at component " << i << " is not supported (accepted: "
                          "[<AffineTransform>] <LstmProjected[Streams]>... <AffineTransform> [<Softmax>])" << hint(i));
    const int32 V = lm.GetComponent(e).OutputDim(), K = o.num_classes > 0 ? o.num_classes : V;
    if (lm.GetComponent(0).InputDim() != V) KLSTM_ERR("CtcNeuralRescorer: the model reads " << lm.GetComponent(0).InputDim() << " classes and writes " << V);
    if (K < 2 || K > V || V > 32768 || o.bos < 0 || o.bos >= V || o.eos >= V)
      KLSTM_ERR("CtcNeuralRescorer: " << K << " token classes, bos " << o.bos << ", eos " << o.eos << " with " << V << " classes");
    if (!std::isfinite(o.am_scale) || !std::isfinite(o.nlm_scale) || !std::isfinite(o.unit_bonus)) KLSTM_ERR("CtcNeuralRescorer: the scales must be finite");
    if (lstm_begin) *lstm_begin = b;
    if (lstm_end) *lstm_end = e;
  }
  CtcNeuralRescorer(const CtcNeuralRescorer &) = delete;
  CtcNeuralRescorer &operator=(const CtcNeuralRescorer &) = delete;

  // over the lists of the last lists.Decode, or any lists in that layout (CtcRescorer::DeviceLists()).  Nothing synchronises.
  void Rescore(const CtcBeamDecoder &lists) { Rescore(lists.DeviceLists()); }
  void Rescore(const CtcNbestDevice &nb) {
    const int32 S = nb.num_stream, N = nb.nbest, E = o_.num_stream, T = o_.chunk, rows = E * T;
    KLSTM_ASSERT(S > 0 && N > 0 && nb.stride > 0 && nb.score);
    const int32 max_len = CtcNbestMaxLen(o_.max_len, nb.stride), out_n = o_.out_n > 0 ? std::min(o_.out_n, N) : N;
    const size_t SN = (size_t)S * N;
    acc_.Grow(SN * sizeof(double)); pos_.Grow(SN * sizeof(int32));       // (set by every group's first chunk: max_len >= 1, so there is one)
    order_.Grow(SN * sizeof(int32)); live_.Grow((size_t)S * sizeof(int32)); score_.Grow(SN * sizeof(BaseFloat));
    nlmlp_.Grow(SN * sizeof(BaseFloat)); units_.Grow(SN * sizeof(int32));
    ohyp_.Grow(SN * nb.stride * sizeof(int32)); olen_.Grow(SN * sizeof(int32)); ocnt_.Grow((size_t)S * sizeof(int32));
    oscore_.Grow(SN * sizeof(BaseFloat)); oerr_.Grow(SN * sizeof(int32));
    const int32 chunks = (max_len + (o_.eos >= 0 ? 1 : 0) + T - 1) / T;
    std::vector<int> flags(E, 1);
    for (int32 first = 0; first < S * N; first += E) {
      for (auto &eng : engines_) KCheck(klstm_reset(eng.get(), flags.data(), E));       // every group starts from zero state
      for (int32 c = 0; c < chunks; c++) {
        KCheck(knlm_pack(nb.hyp, nb.stride, nb.hyp_len, nb.count, nb.score, S, N, max_len, K_, V_, o_.bos, o_.eos, first, E, T, c * T,
                         embed_ ? We_.As<BaseFloat>() : nullptr, embed_ ? be_.As<BaseFloat>() : nullptr, embed_ ? cols_ : 0, x_.As<BaseFloat>(), cols_,
                         nullptr));
        const BaseFloat *in = x_.As<BaseFloat>();
        int32 in_stride = cols_;
        for (size_t l = 0; l < engines_.size(); l++) {
          KCheck(klstm_propagate_inference(engines_[l].get(), in, rows, in_stride, h_[l].As<BaseFloat>(), dims_[l]));
          in = h_[l].As<BaseFloat>();
          in_stride = dims_[l];
        }
        KCheck(klstm_affine_propagate(in, rows, aff_in_, in_stride, W_.As<BaseFloat>(), b_.As<BaseFloat>(), a_.As<BaseFloat>(), V_, V_, nullptr));
        KCheck(knlm_score_rows(a_.As<BaseFloat>(), V_, nb.hyp, nb.stride, nb.hyp_len, nb.count, nb.score, S, N, max_len, K_, V_, o_.eos, first, E, T,
                               c * T, acc_.As<double>(), pos_.As<int32>(), ws_.As<void>(), ws_bytes_, nullptr));
      }
    }
    KCheck(knlm_rank(nb.hyp, nb.stride, nb.hyp_len, nb.count, nb.score, nb.errors, S, N, max_len, K_, acc_.As<double>(), o_.am_scale, o_.nlm_scale,
                     o_.unit_bonus, o_.eos >= 0 ? 1 : 0, order_.As<int32>(), live_.As<int32>(), score_.As<BaseFloat>(), nlmlp_.As<BaseFloat>(),
                     units_.As<int32>(), out_n, ohyp_.As<int32>(), nb.stride, olen_.As<int32>(), ocnt_.As<int32>(), oscore_.As<BaseFloat>(),
                     nb.errors ? oerr_.As<int32>() : nullptr, tot_.Dev(), nullptr));
    num_stream_ = S; nbest_ = N; out_nbest_ = out_n; stride_ = nb.stride; scored_ = nb.errors != nullptr;
  }
  // the re-ranked lists of the last Rescore on the device, in the layout of CtcBeamDecoder::DeviceLists() (CtcConsensus::Eval and CtcMbr
  // take them); slots beyond a stream's count hold nothing
  CtcNbestDevice DeviceLists() const {
    return CtcNbestDevice{ohyp_.As<int32>(), olen_.As<int32>(), ocnt_.As<int32>(), scored_ ? oerr_.As<int32>() : nullptr, num_stream_, out_nbest_, stride_,
                          oscore_.As<BaseFloat>()};
  }
  // of the last Rescore (each synchronises): the re-ranked list of every stream, best first, with the new scores
  void Lists(std::vector<CtcNbestList> *lists) const {
    const size_t SN = (size_t)num_stream_ * out_nbest_;
    std::vector<int32> c(num_stream_), n(SN), h(SN * stride_), e(SN, -1);
    std::vector<BaseFloat> sc(SN);
    ocnt_.Download(c.data(), c.size()); olen_.Download(n.data(), n.size()); ohyp_.Download(h.data(), h.size());
    oscore_.Download(sc.data(), sc.size());
    if (scored_) oerr_.Download(e.data(), e.size());
    lists->assign(num_stream_, CtcNbestList());
    for (int32 s = 0; s < num_stream_; s++)
      for (int32 q = 0; q < c[s]; q++) {
        const size_t o = (size_t)s * out_nbest_ + q;
        CtcHypothesis hy;
        hy.tokens.assign(h.begin() + o * stride_, h.begin() + o * stride_ + n[o]);
        hy.score = sc[o];
        hy.errors = e[o];
        (*lists)[s].push_back(hy);
      }
  }
  // ... the entry of the given list at every rank [num_stream][nbest] (-1 beyond the entries ranked) and how many were ranked
  void Order(std::vector<int32> *order, std::vector<int32> *live = nullptr) const {
    order->assign((size_t)num_stream_ * nbest_, -1);
    order_.Download(order->data(), order->size());
    if (live) { live->assign(num_stream_, 0); live_.Download(live->data(), live->size()); }
  }
  // ... per entry of the given list [num_stream][nbest]: the new score and the LM's log probability (-inf: dropped, forbidden or
  // unlisted), the units (any may be null)
  void Entries(std::vector<BaseFloat> *score, std::vector<BaseFloat> *nlm_logp = nullptr, std::vector<int32> *units = nullptr) const {
    const size_t SN = (size_t)num_stream_ * nbest_;
    if (score) { score->assign(SN, 0.f); score_.Download(score->data(), SN); }
    if (nlm_logp) { nlm_logp->assign(SN, 0.f); nlmlp_.Download(nlm_logp->data(), SN); }
    if (units) { units->assign(SN, 0); units_.Download(units->data(), SN); }
  }
  // over the streams rescored so far
  double NumUtterances() const { return tot_.Read()[0]; }
  double NumChanged() const { return tot_.Read()[4]; }                 // streams whose 1-best is no longer the given list's
  double NumFirstPassErrors() const { return tot_.Read()[5]; }         // edit errors of the given list's 1-best (lists decoded with references)
  double NumRescoredErrors() const { return tot_.Read()[6]; }          // ... of the new 1-best
  double NumDropped() const { return tot_.Read()[2]; }
  double NumForbidden() const { return tot_.Read()[3]; }
  double NumPositions() const { return tot_.Read()[7]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "NEURAL RESCORED: " << h[4] << " of " << h[0] << " 1-bests changed, errors " << h[5] << " -> " << h[6] << " [" << h[1]
        << " idle or rejected, " << h[2] << " entries dropped, " << h[3] << " forbidden, " << h[7] << " positions scored]" << std::endl;
    return oss.str();
  }
 private:
  struct EngineDel { void operator()(klstm_engine *e) const { klstm_destroy(e); } };
  CtcNeuralRescorerOptions o_;
  std::vector<std::unique_ptr<klstm_engine, EngineDel> > engines_;
  std::vector<int32> dims_;
  int32 V_ = 0, K_ = 0, cols_ = 0, aff_in_ = 0, num_stream_ = 0, nbest_ = 0, out_nbest_ = 0, stride_ = 0;
  bool embed_ = false, scored_ = false;
  size_t ws_bytes_ = 0;
  DeviceBuffer W_, b_, We_, be_, x_, a_, ws_, acc_, pos_;
  std::vector<DeviceBuffer> h_;
  DeviceBuffer order_, live_, score_, nlmlp_, units_, ohyp_, olen_, ocnt_, oscore_, oerr_;
  DeviceTotals<8> tot_;
};

// The training data of such an LM: per token sequence one Utterance of one-hot feature rows [bos, y_0, ...] over V classes with the
// next-token targets [y_0, ..., eos], which TrainLstmStreams trains on.  eos < 0: no end term (one row fewer; a sequence that leaves no
// row is skipped).
inline std::vector<Utterance> LmTrainingUtterances(const std::vector<std::vector<int32> > &sequences, int32 V, int32 bos, int32 eos) {
  KLSTM_ASSERT(V >= 2 && bos >= 0 && bos < V && eos < V);
  std::vector<Utterance> out;
  for (const auto &y : sequences) {
    for (int32 t : y) KLSTM_ASSERT(t >= 0 && t < V);
    std::vector<int32> x(1, bos), tgt(y);
    x.insert(x.end(), y.begin(), y.end());
    if (eos >= 0) tgt.push_back(eos); else x.pop_back();
    if (x.empty()) continue;
    Utterance u;
    u.num_frames = (int32)x.size(); u.dim = V;
    u.feats.assign((size_t)u.num_frames * V, 0.f);
    for (int32 p = 0; p < u.num_frames; p++) u.feats[(size_t)p * V + x[p]] = 1.f;
    u.targets = tgt;
    out.push_back(u);
  }
  return out;
}

struct TrainMbrOptions {
  NnetTrainOptions trn_opts;
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, crossvalidate = false;
  int32 beam = 16, cands = 8, nbest = 8;                 // the search that makes the lists (CtcBeamDecoder)
  BaseFloat risk_scale = 1.f, ctc_weight = 0.f;
  const CtcLabelLm *lm = nullptr;                        // fused into the search; not owned
  std::vector<BaseFloat> class_weights;                  // empty: none
  int32 max_hyp_len = 0;                                 // 0: min(1023, 2 * longest reference + 8)
  BaseFloat dropout_retention = 0.f;                     // the <Dropout> components while training (klstm_dropout.h): 0: the model's own retention
  uint64_t dropout_seed = 0;                             // same seed, same data: the same masks, bit for bit; give every epoch its own
  bool dropout_per_sequence = false;                     // one mask per (stream, sequence) instead of one per element and step
};
struct TrainMbrStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double num_rejected = 0, total_frames = 0, seconds = 0, avg_loss = 0, avg_loss_per_frame = 0;     // the reference's CTC loss (0 without ctc_weight)
  double avg_risk = 0, token_error_rate = 0;             // expected errors per utterance; 1-best token error rate of the lists
};

// Minimum expected token error training over the model's own n-best lists: Propagate, beam search against the labels, CtcMbr::Eval,
// Backpropagate (not under crossvalidate).  every_batch (optional) sees each minibatch after the Eval: (batch, net_out, obj_diff,
// decoder, mbr).
template <class F>
inline TrainMbrStats TrainMbrWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainMbrOptions &o, std::string *report,
                                             F every_batch) {
  nnet->SetTrainOptions(o.trn_opts);
  DropoutTrainingScope dropout(nnet, o.crossvalidate, o.dropout_retention, o.dropout_seed, o.dropout_per_sequence);
  CtcBeamDecoder dec(o.blank, o.beam, o.cands, o.nbest);
  if (!o.class_weights.empty()) dec.SetClassWeights(o.class_weights);
  dec.SetLanguageModel(o.lm);
  CtcMbr mbr(o.blank, o.risk_scale, o.ctc_weight, o.max_hyp_len);
  DeviceMatrix obj_diff;
  TrainMbrStats st = ForEachWholeUtteranceBatch<TrainMbrStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
        dec.Decode(nnet_out, b.num_stream, b.lens, b.labels, nullptr);
        mbr.Eval(nnet_out, b.num_stream, b.lens, dec, b.labels, &obj_diff);
        every_batch(b, nnet_out, obj_diff, dec, mbr);
        if (!o.crossvalidate) nnet->Backpropagate(obj_diff.View(), nullptr);
      });
  st.num_rejected = mbr.NumRejectedOrSkipped();
  st.total_frames = mbr.Frames();
  st.avg_loss = mbr.AvgRefLoss();
  st.avg_loss_per_frame = mbr.Frames() > 0 ? mbr.AvgRefLoss() * mbr.NumUtterances() / mbr.Frames() : 0;
  st.avg_risk = mbr.AvgRisk();
  st.token_error_rate = dec.TokenErrorRate();
  if (report) *report = mbr.Report() + dec.Report();
  return st;
}
inline TrainMbrStats TrainMbrWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainMbrOptions &o,
                                             std::string *report = nullptr) {
  return TrainMbrWholeUtterances(nnet, utts, o, report,
                                 [](const UtteranceBatch &, const DeviceMatrix &, const DeviceMatrix &, const CtcBeamDecoder &, const CtcMbr &) {});
}

// MMI (CTC-CRF) against a label language model (klstm_ctc_mmi_eval, klstm.h): loss = -log p(ref | y) - log W(ref) +
// log Z with Z summed over every labelling the model accepts -- the model CtcBeamDecoder::SetLanguageModel fuses into the search.  diff
// is the derivative of loss + ctc_weight * (-log p(ref | y)) with respect to the Softmax INPUT, like Ctc's.  The denominator graph is
// built on the device when the model is set and serves every Eval after it; the five totals stay on the device.  The model is the
// DENSE one: a sparse back-off model (CtcSparseLabelLm) serves the search only.
class CtcMmi : private CtcCallBase {
 public:
  explicit CtcMmi(int32 blank = 0, BaseFloat ctc_weight = 0.f) : CtcCallBase(blank), ctc_weight_(ctc_weight) {}

  // the model is read here and not needed afterwards; setting another one rebuilds the graph
  void SetLanguageModel(const CtcLabelLm *lm) {
    KLSTM_ASSERT(lm);
    states_ = lm->NumStates(); classes_ = lm->NumClasses();
    graph_bytes_ = klstm_ctc_mmi_graph_bytes(states_, classes_);
    if (graph_bytes_ == 0) KLSTM_ERR("klstm: " << klstm_last_error());
    graph_.Grow(graph_bytes_);
    KCheck(klstm_ctc_mmi_graph_build(states_, classes_, blank_, lm->Next(), lm->Weight(), lm->Final(), graph_.As<void>(), graph_bytes_, nullptr));
  }
  // net_out, lens, labels as Ctc::Eval takes them.  Everything is decided on the device (klstm.h): idle and rejected streams (what
  // Ctc rejects, and labels the model does not accept) get zero diff rows.
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    Eval(net_out, num_stream, UploadLens(num_stream, lens), labels, diff);
  }
  void Eval(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &labels,
            DeviceMatrix *diff) {
    const int32 T = NumFrames(net_out, num_stream, lens_dev, labels.size(), false), K = net_out.NumCols();
    KLSTM_ASSERT(graph_bytes_ > 0 && K == classes_);
    lab_.Upload(labels);
    const size_t need = klstm_ctc_mmi_workspace_bytes(T, num_stream, K, states_, (int)std::min(lab_.longest, (size_t)1023));   // longer: the device's to reject
    void *ws = Workspace(need);
    loss_.Grow((size_t)num_stream * sizeof(BaseFloat));
    diff->Resize(net_out.NumRows(), K, false);
    MatrixView y = net_out.View(), dv = diff->View();
    KCheck(klstm_ctc_mmi_eval(y.Data(), T, num_stream, K, y.Stride(), lens_dev, lab_.Labels(), lab_.Offsets(), blank_, graph_.As<void>(),
                              graph_bytes_, states_, ctc_weight_, dv.Data(), dv.Stride(), loss_.As<BaseFloat>(), nullptr, nullptr, nullptr,
                              tot_.Dev(), ws, need, nullptr));
    num_stream_ = num_stream;
  }
  // the loss of the streams of the last Eval (+inf: rejected, 0: idle).  Synchronises.
  void UttLoss(std::vector<BaseFloat> *loss) const { loss->assign(num_stream_, 0.f); loss_.Download(loss->data(), loss->size()); }
  double AvgLoss() const { const double *h = tot_.Read(); return h[0] / h[1]; }                // per utterance counted
  double AvgLossPerFrame() const { const double *h = tot_.Read(); return h[0] / h[3]; }
  double NumUtterances() const { return tot_.Read()[1]; }
  double NumRejected() const { return tot_.Read()[2]; }
  double Frames() const { return tot_.Read()[3]; }
  double AvgRefLoss() const { const double *h = tot_.Read(); return h[4] / h[1]; }             // the CTC loss of the references
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "AvgLoss: " << h[0] / h[1] << " (CtcMmi) per utterance, " << h[0] / h[3] << " per frame, reference CTC loss " << h[4] / h[1]
        << " per utterance, [" << h[1] << " utterances, " << h[3] << " frames, " << h[2] << " rejected]" << std::endl;
    return oss.str();
  }
 private:
  BaseFloat ctc_weight_;
  int32 states_ = 0, classes_ = 0;
  size_t graph_bytes_ = 0;
  PackedLabels lab_;
  DeviceBuffer graph_, loss_;
  DeviceTotals<5> tot_;
};

struct TrainMmiOptions {
  NnetTrainOptions trn_opts;                             // learning rate, momentum
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, crossvalidate = false;
  BaseFloat ctc_weight = 0.f;
  const CtcLabelLm *lm = nullptr;                        // the denominator's model (required); not owned
  BaseFloat dropout_retention = 0.f;                     // the <Dropout> components while training (klstm_dropout.h): 0: the model's own retention
  uint64_t dropout_seed = 0;                             // same seed, same data: the same masks, bit for bit; give every epoch its own
  bool dropout_per_sequence = false;                     // one mask per (stream, sequence) instead of one per element and step
};
struct TrainMmiStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double num_rejected = 0, total_frames = 0, seconds = 0, avg_loss = 0, avg_loss_per_frame = 0;     // the MMI loss
  double avg_ref_loss = 0;                               // the CTC loss of the references, per utterance
};

// MMI training: Propagate, CtcMmi::Eval against the labels, Backpropagate (not under crossvalidate).  every_batch (optional) sees each
// minibatch after the Eval: (batch, net_out, obj_diff, mmi).
template <class F>
inline TrainMmiStats TrainMmiWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainMmiOptions &o, std::string *report,
                                             F every_batch) {
  KLSTM_ASSERT(o.lm);
  nnet->SetTrainOptions(o.trn_opts);
  DropoutTrainingScope dropout(nnet, o.crossvalidate, o.dropout_retention, o.dropout_seed, o.dropout_per_sequence);
  CtcMmi mmi(o.blank, o.ctc_weight);
  mmi.SetLanguageModel(o.lm);
  DeviceMatrix obj_diff;
  TrainMmiStats st = ForEachWholeUtteranceBatch<TrainMmiStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
        mmi.Eval(nnet_out, b.num_stream, b.lens, b.labels, &obj_diff);
        every_batch(b, nnet_out, obj_diff, mmi);
        if (!o.crossvalidate) nnet->Backpropagate(obj_diff.View(), nullptr);
      });
  st.num_rejected = mmi.NumRejected();
  st.total_frames = mmi.Frames();
  st.avg_loss = mmi.AvgLoss();
  st.avg_loss_per_frame = mmi.AvgLossPerFrame();
  st.avg_ref_loss = mmi.AvgRefLoss();
  if (report) *report = mmi.Report();
  return st;
}
inline TrainMmiStats TrainMmiWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const TrainMmiOptions &o,
                                             std::string *report = nullptr) {
  return TrainMmiWholeUtterances(nnet, utts, o, report, [](const UtteranceBatch &, const DeviceMatrix &, const DeviceMatrix &, const CtcMmi &) {});
}

struct DecodeCtcOptions {
  int32 num_stream = 4, blank = 0, max_frames = 0;       // max_frames 0: 65535 / num_stream
  bool sort_by_length = true, score = true;              // score: the utterances' labels are references
  std::vector<BaseFloat> class_weights;                  // empty: none
  int32 beam = 0, cands = 8, nbest = 1;                  // beam 0: best path (CtcGreedyDecoder); beam > 0: prefix beam search (CtcBeamDecoder)
  const CtcLabelLm *lm = nullptr;                        // beam > 0 only: fused into the search (CtcBeamDecoder::SetLanguageModel); not owned
  const CtcSparseLabelLm *slm = nullptr;                 // beam > 0 only: a sparse back-off model in its place (at most one of the two); not owned
  int32 consensus = 0;                                   // beam > 0 only (CtcConsensus over each minibatch's lists): 0 off, 1 the MAP entry with
                                                         // confidences, 2 the MBR entry is the hypothesis
  BaseFloat consensus_scale = 1.f;                       // multiplies the search's scores under the lists' posterior
  int32 separator = -1;                                  // -1: errors and confidences per token; otherwise the class that separates words
  CtcRescorer *rescorer = nullptr;                       // beam > 0 only: runs on each minibatch's lists before the consensus step, which then
                                                         // sees the re-ranked lists, as do hypotheses and nbest_lists; not owned; null: none
  CtcNeuralRescorer *neural_rescorer = nullptr;          // beam > 0 only: an LSTM language model over the lists, behind `rescorer` (whose re-ranked
                                                         // lists it then reads) and before the consensus step; not owned; null: none
};
struct DecodeCtcStats {
  int32 num_done = 0, num_skipped = 0, num_minibatches = 0;
  double token_error_rate = 0, utt_error_rate = 0, num_scored = 0, num_errors = 0, num_ref_tokens = 0, seconds = 0;
  double oracle_token_error_rate = 0;                    // beam search only: the best hypothesis of every n-best list
  // with o.consensus only: expected unit errors per utterance of the hypotheses returned and of the MAP entries under the lists'
  // posteriors, the mean confidence of the units returned, the edit errors of the hypotheses returned (scored passes)
  double expected_errors = 0, map_expected_errors = 0, mean_confidence = 0, num_pick_errors = 0;
  // with o.rescorer only, over this pass: the token error rates of the search's 1-bests and of the rescored ones (scored passes) and
  // the utterances whose 1-best changed
  double first_pass_token_error_rate = 0, rescored_token_error_rate = 0, num_changed_1best = 0;
  // with o.neural_rescorer only, over this pass: the token error rates of the 1-bests it was given and of its own (scored passes) and
  // the utterances whose 1-best it changed
  double neural_first_pass_token_error_rate = 0, neural_rescored_token_error_rate = 0, num_neural_changed_1best = 0;
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
// what both decoders know at the end of a pass
template <class Decoder>
inline void FillDecodeCtcStats(const Decoder &dec, DecodeCtcStats *st, std::string *report) {
  st->num_scored = dec.NumUtterances();
  st->num_errors = dec.NumErrors();
  st->num_ref_tokens = dec.NumRefTokens();
  st->token_error_rate = dec.TokenErrorRate();
  st->utt_error_rate = dec.UtteranceErrorRate();
  if (report) *report = dec.Report();
}

// The loop of DecodeCtcWholeUtterances below with the prefix beam search (o.beam > 0).  (*hypotheses)[i] is the 1-best of utts[i],
// (*nbest_lists)[i] its whole list with scores and edit distances (either may be null; both empty for a skipped utterance).
// every_batch sees (batch, net_out, CtcBeamDecoder) after Decode.  With o.consensus (1 or 2) a CtcConsensus runs over the lists of
// every minibatch: (*hypotheses)[i] is then the entry it answers with (the MAP or the MBR one), (*confidences)[i] (may be null) holds
// one confidence per token or word of it, and the statistics and the report carry the expected errors.  With o.rescorer the lists of
// every minibatch are re-ranked first (CtcRescorer::Eval): hypotheses, nbest_lists and the consensus then see the re-ranked lists, and
// the statistics carry the error rates before and after; null leaves the loop as it was.  With o.neural_rescorer an LSTM language
// model re-ranks the lists next (CtcNeuralRescorer::Rescore, over the rescorer's lists where there is one): search -> rescorer ->
// neural_rescorer -> consensus, each stage reading the previous one's lists; null leaves the loop as it was.
template <class F>
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::vector<std::vector<BaseFloat> > *confidences, std::string *report, F every_batch) {
  KLSTM_ASSERT(o.beam > 0 && o.consensus >= 0 && o.consensus <= 2);
  CtcBeamDecoder dec(o.blank, o.beam, o.cands, o.nbest);
  CtcConsensus cons(o.consensus == 2, o.consensus_scale, o.separator);
  dec.SetClassWeights(o.class_weights);
  KLSTM_ASSERT(!o.lm || !o.slm);
  if (o.slm) dec.SetLanguageModel(o.slm); else dec.SetLanguageModel(o.lm);
  std::vector<CtcNbestList> lists;
  const std::vector<std::vector<int32> > none;
  const bool want = hypotheses || nbest_lists;
  if (hypotheses) hypotheses->assign(utts.size(), std::vector<int32>());
  if (nbest_lists) nbest_lists->assign(utts.size(), CtcNbestList());
  if (confidences) confidences->assign(utts.size(), std::vector<BaseFloat>());
  const double resc0[3] = {o.rescorer ? o.rescorer->NumChanged() : 0, o.rescorer ? o.rescorer->NumFirstPassErrors() : 0,
                           o.rescorer ? o.rescorer->NumRescoredErrors() : 0};          // the rescorer may have seen other passes
  CtcNeuralRescorer *const nr = o.neural_rescorer;
  const double nresc0[3] = {nr ? nr->NumChanged() : 0, nr ? nr->NumFirstPassErrors() : 0, nr ? nr->NumRescoredErrors() : 0};
  DecodeCtcStats st = ForEachWholeUtteranceBatch<DecodeCtcStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
        dec.Decode(nnet_out, b.num_stream, b.lens, o.score ? b.labels : none, want && !o.rescorer && !nr ? &lists : nullptr);
        if (o.rescorer) {
          o.rescorer->Eval(dec);
          if (want && !nr) o.rescorer->Lists(&lists);
        }
        if (nr) {
          if (o.rescorer) nr->Rescore(o.rescorer->DeviceLists()); else nr->Rescore(dec);
          if (want) nr->Lists(&lists);
        }
        std::vector<int32> pick(b.num_stream, 0);          // without a consensus: the head of the list
        if (o.consensus) {
          if (nr) cons.Eval(nr->DeviceLists()); else if (o.rescorer) cons.Eval(o.rescorer->DeviceLists()); else cons.Eval(dec);
          if (hypotheses) cons.Picks(&pick);
          if (confidences) {
            std::vector<std::vector<BaseFloat> > conf;
            cons.Confidences(&conf);
            ScatterByUtterance(b, conf, confidences);
          }
        }
        if (nbest_lists) ScatterByUtterance(b, lists, nbest_lists);
        if (hypotheses) {
          std::vector<std::vector<int32> > best(b.num_stream);
          for (int32 s = 0; s < b.num_stream; s++)
            if (pick[s] >= 0 && (size_t)pick[s] < lists[s].size()) best[s] = lists[s][pick[s]].tokens;
          ScatterByUtterance(b, best, hypotheses);
        }
        every_batch(b, nnet_out, dec);
      });
  st.oracle_token_error_rate = dec.OracleTokenErrorRate();
  FillDecodeCtcStats(dec, &st, report);
  if (o.consensus) {
    st.expected_errors = cons.ExpectedErrors();
    st.map_expected_errors = cons.MapExpectedErrors();
    st.mean_confidence = cons.MeanConfidence();
    st.num_pick_errors = cons.NumPickErrors();
    if (report) *report += "\n" + cons.Report();
  }
  if (o.rescorer) {
    st.num_changed_1best = o.rescorer->NumChanged() - resc0[0];
    if (st.num_ref_tokens > 0) {
      st.first_pass_token_error_rate = (o.rescorer->NumFirstPassErrors() - resc0[1]) / st.num_ref_tokens;
      st.rescored_token_error_rate = (o.rescorer->NumRescoredErrors() - resc0[2]) / st.num_ref_tokens;
    }
    if (report) *report += "\n" + o.rescorer->Report();
  }
  if (nr) {
    st.num_neural_changed_1best = nr->NumChanged() - nresc0[0];
    if (st.num_ref_tokens > 0) {
      st.neural_first_pass_token_error_rate = (nr->NumFirstPassErrors() - nresc0[1]) / st.num_ref_tokens;
      st.neural_rescored_token_error_rate = (nr->NumRescoredErrors() - nresc0[2]) / st.num_ref_tokens;
    }
    if (report) *report += "\n" + nr->Report();
  }
  return st;
}
template <class F>
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::string *report, F every_batch) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, nbest_lists, (std::vector<std::vector<BaseFloat> > *)nullptr, report, every_batch);
}
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::string *report = nullptr) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, nbest_lists, report, [](const UtteranceBatch &, const DeviceMatrix &, const CtcBeamDecoder &) {});
}
// ... with the confidences of the hypotheses (o.consensus 1 or 2; empty vectors without)
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::vector<CtcNbestList> *nbest_lists,
                                               std::vector<std::vector<BaseFloat> > *confidences, std::string *report) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, nbest_lists, confidences, report,
                                  [](const UtteranceBatch &, const DeviceMatrix &, const CtcBeamDecoder &) {});
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
  CtcGreedyDecoder dec(o.blank);
  dec.SetClassWeights(o.class_weights);
  std::vector<std::vector<int32> > hyps;
  const std::vector<std::vector<int32> > none;
  if (hypotheses) hypotheses->assign(utts.size(), std::vector<int32>());
  DecodeCtcStats st = ForEachWholeUtteranceBatch<DecodeCtcStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
        dec.Decode(nnet_out, b.num_stream, b.lens, o.score ? b.labels : none, hypotheses ? &hyps : nullptr);
        if (hypotheses) ScatterByUtterance(b, hyps, hypotheses);
        every_batch(b, nnet_out, dec);
      });
  FillDecodeCtcStats(dec, &st, report);
  return st;
}
inline DecodeCtcStats DecodeCtcWholeUtterances(Nnet *nnet, const std::vector<Utterance> &utts, const DecodeCtcOptions &o,
                                               std::vector<std::vector<int32> > *hypotheses, std::string *report = nullptr) {
  return DecodeCtcWholeUtterances(nnet, utts, o, hypotheses, report, [](const UtteranceBatch &, const DeviceMatrix &, const CtcGreedyDecoder &) {});
}

// CTC forced alignment of whole utterances: the most probable alignment of each stream's labels to its frames (klstm_ctc_align,
// klstm.h).  The five totals stay on the device and are read when somebody asks, like Ctc's.
class CtcAligner : private CtcCallBase {
 public:
  explicit CtcAligner(int32 blank = 0) : CtcCallBase(blank) {}

  // One weight per class: the emission of a frame becomes log(y[k] * w[k]) (label priors: w[k] = prior[k]^-alpha).  Empty: none.
  using CtcCallBase::SetClassWeights;
  // net_out [T*num_stream x K] posteriors (row t*S + s); lens: frames per stream (0 = idle); labels: per stream.  Utterances that
  // cannot be aligned (klstm.h) are rejected on the device.  Nothing synchronises.
  void Align(const DeviceMatrix &net_out, int32 num_stream, const std::vector<int32> &lens, const std::vector<std::vector<int32> > &labels) {
    Align(net_out, num_stream, UploadLens(num_stream, lens), labels);
  }
  void Align(const DeviceMatrix &net_out, int32 num_stream, const int32 *lens_dev, const std::vector<std::vector<int32> > &labels) {
    const int32 T = NumFrames(net_out, num_stream, lens_dev, labels.size(), false), rows = net_out.NumRows(), K = net_out.NumCols();
    lab_.Upload(labels);
    const size_t need = klstm_ctc_align_workspace_bytes(T, num_stream, (int)std::min(lab_.longest, (size_t)1023));   // longer: the device's to reject
    void *ws = Workspace(need);
    const size_t tokens = std::max(lab_.num_labels, (size_t)1);         // (as many as the label array has)
    fc_.Grow((size_t)rows * sizeof(int32));
    fp_.Grow((size_t)rows * sizeof(int32));
    tb_.Grow(tokens * sizeof(int32));
    te_.Grow(tokens * sizeof(int32));
    score_.Grow((size_t)num_stream * sizeof(BaseFloat));
    MatrixView y = net_out.View();
    KCheck(klstm_ctc_align(y.Data(), T, num_stream, K, y.Stride(), lens_dev, lab_.Labels(), lab_.Offsets(), blank_, Weights(),
                           fc_.As<int32>(), fp_.As<int32>(), tb_.As<int32>(), te_.As<int32>(), score_.As<BaseFloat>(), tot_.Dev(), ws, need,
                           nullptr));
    num_stream_ = num_stream; rows_ = rows;
  }
  // of the last Align (each synchronises).  Frame classes and positions [T*num_stream], row t*S + s; -1 where there is no path
  void FrameClasses(std::vector<int32> *v) const { v->assign(rows_, -1); fc_.Download(v->data(), v->size()); }
  void FramePositions(std::vector<int32> *v) const { v->assign(rows_, -1); fp_.Download(v->data(), v->size()); }
  // per stream: first frame of every token and one past its last (empty for a stream without labels; -1 where not aligned)
  void TokenBounds(std::vector<std::vector<int32> > *begin, std::vector<std::vector<int32> > *end) const {
    const std::vector<int32> &off = lab_.offsets;
    std::vector<int32> b(lab_.num_labels), e(lab_.num_labels);
    tb_.Download(b.data(), b.size());
    te_.Download(e.data(), e.size());
    begin->assign(num_stream_, std::vector<int32>());
    end->assign(num_stream_, std::vector<int32>());
    for (int32 s = 0; s < num_stream_; s++) {
      (*begin)[s].assign(b.begin() + off[s], b.begin() + off[s + 1]);
      (*end)[s].assign(e.begin() + off[s], e.begin() + off[s + 1]);
    }
  }
  // log probability of the path (0: idle, -inf: rejected)
  void UttScores(std::vector<BaseFloat> *v) const { v->assign(num_stream_, 0.f); score_.Download(v->data(), v->size()); }

  double AvgScorePerFrame() const { const double *h = tot_.Read(); return h[0] / h[3]; }
  double BlankRatio() const { const double *h = tot_.Read(); return h[4] / h[3]; }
  double NumAligned() const { return tot_.Read()[1]; }
  double NumRejected() const { return tot_.Read()[2]; }
  double Frames() const { return tot_.Read()[3]; }
  std::string Report() const {
    const double *h = tot_.Read();
    std::ostringstream oss;
    oss << "AvgPathScore: " << h[0] / h[3] << " (CtcAligner) per frame, blank ratio " << h[4] / h[3] << " [" << h[1] << " utterances, " << h[3]
        << " frames, " << h[2] << " rejected]" << std::endl;
    return oss.str();
  }
 private:
  PackedLabels lab_;
  DeviceBuffer fc_, fp_, tb_, te_, score_;
  DeviceTotals<5> tot_;
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
  CtcAligner al(o.blank);
  al.SetClassWeights(o.class_weights);
  std::vector<int32> fc;
  std::vector<BaseFloat> score;
  std::vector<std::vector<int32> > tb, te;
  std::vector<CtcAlignment> per_stream;
  if (alignments) alignments->assign(utts.size(), CtcAlignment());
  AlignCtcStats st = ForEachWholeUtteranceBatch<AlignCtcStats>(nnet, utts, o.num_stream, o.sort_by_length, o.max_frames,
      [&](const UtteranceBatch &b, const DeviceMatrix &nnet_out) {
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
      });
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
