// include/klstm_blstm.hpp -- a bidirectional LSTMP layer over whole utterances (Kaldi nnet1's later BLstmProjectedStreams, which was
// written from the same LstmProjectedStreams code), built from two unmodified engines.
//
//   in  [T*S x I]   time-major (row t*S + s); stream s holds ONE whole utterance of lens[s] frames starting at t = 0, rows
//                   t >= lens[s] are padding, lens[s] = 0 marks an idle stream (SetSeqLengths, nnet1's name).
//   out [T*S x 2R]  columns [0, R): the forward engine on `in` from zero state (klstm_reset of every stream + klstm_propagate);
//                   columns [R, 2R): the backward engine on the per-stream time reversal of `in` (row t of stream s is input row
//                   lens[s]-1-t), from zero state, reversed back.  nnet1's column order.  Padding rows of out are zero in both halves.
//   backward        the forward engine gets columns [0, R) of out_diff, the backward engine the reversal of columns [R, 2R);
//                   in_diff = in_diff_f + reverse(in_diff_b), padding rows zero.  in_diff may be NULL.  Update / momentum per
//                   direction through the engines' own calls; KLSTM_BPTT_FUSE_UPDATE (SetUpdateFollows) is passed through.
//
// Why padding is exact in both directions: padding frames come AFTER every valid frame of their stream, in both time orders (the
// reversal maps the valid prefix onto a valid prefix), so the recurrence carries nothing from a padding frame into a valid one.  In the
// backward pass the only way in is out_diff, and this layer zeroes out_diff's padding rows itself before either engine sees them (the
// masked Xent, klstm_softmax_xent_masked, leaves them zero anyway): every derivative of a padding frame is then exactly zero, so padding
// reaches no valid output, no gradient and no in_diff, whatever finite values the padding rows of `in` hold.
//
// Both engines run on ONE HIP stream, one after the other.  Do not split the directions over two streams: the persistent chains hold
// most or all of the chip (the fp32 chain 200 + 50 of 256 CUs, the per-XCD bf16 chain all 256), and two of them side by side would
// make each other give up (INTEGRATION.md "A shared GPU").  The reversal kernels (klstm_reverse_streams) read what the engines wrote,
// so both engines run with "persist_verify" on (the default of the LstmProjectedStreams mirror): a persistent launch that gives up is
// answered inside the engine's call, before the reversal reads its output.  With KLSTM_BPTT_FUSE_UPDATE an engine's in_diff is valid
// when its klstm_update has returned: the two halves of in_diff are then summed in Update.
//
// Header-only C++ over the C-ABI (klstm.h), like klstm_scorer.hpp.  There is no model-file form of this layer: it is built from two
// reference-format <LstmProjectedStreams> components, which read and write the reference's format as they are.
#pragma once
#include <memory>
#include <vector>

#include "klstm_nnet.hpp"

namespace klstm_kaldi {

class BLstmProjectedStreams {
 public:
  enum Direction { kForward = 0, kBackward = 1 };
  // Takes ownership of the two directions (e.g. ReadLstmComponent of two <LstmProjectedStreams>), also when it throws: same input,
  // cell and output dimensions and the same number of streams.
  BLstmProjectedStreams(LstmProjectedStreams *fwd, LstmProjectedStreams *bwd) : f_(fwd), b_(bwd) {
    KLSTM_ASSERT(f_ && b_);
    if (std::string(f_->Marker()) != "<LstmProjectedStreams>" || std::string(b_->Marker()) != "<LstmProjectedStreams>")
      KLSTM_ERR("BLstmProjectedStreams: both directions must be <LstmProjectedStreams> components (got " << f_->Marker() << ", "
                << b_->Marker() << ")");
    if (f_->InputDim() != b_->InputDim() || f_->OutputDim() != b_->OutputDim() || f_->CellDim() != b_->CellDim() ||
        f_->NumStream() != b_->NumStream() || f_->NumStream() <= 0)
      KLSTM_ERR("BLstmProjectedStreams: the two directions differ in shape (I " << f_->InputDim() << "/" << b_->InputDim() << ", C "
                << f_->CellDim() << "/" << b_->CellDim() << ", R " << f_->OutputDim() << "/" << b_->OutputDim() << ", streams "
                << f_->NumStream() << "/" << b_->NumStream() << ")");
    f_->SetPersistVerify(true);
    b_->SetPersistVerify(true);
  }
  BLstmProjectedStreams(const BLstmProjectedStreams &) = delete;
  BLstmProjectedStreams &operator=(const BLstmProjectedStreams &) = delete;

  int32 InputDim() const { return f_->InputDim(); }
  int32 OutputDim() const { return 2 * f_->OutputDim(); }
  int32 CellDim() const { return f_->CellDim(); }
  int32 NumStream() const { return f_->NumStream(); }
  LstmProjectedStreams &Dir(Direction d) { return d == kForward ? *f_ : *b_; }
  const LstmProjectedStreams &Dir(Direction d) const { return d == kForward ? *f_ : *b_; }

  // both engines and the reversal kernels on `hip_stream` (nullptr: the library's per-device stream for the engines and the legacy
  // default stream, which is ordered with it, for the reversals -- as the other stateless calls of klstm_nnet.hpp)
  void SetDevice(int device, void *hip_stream = nullptr) { f_->SetDevice(device, hip_stream); b_->SetDevice(device, hip_stream); stream_ = hip_stream; }
  void SetTrainOptions(const NnetTrainOptions &o) { f_->SetTrainOptions(o); b_->SetTrainOptions(o); }
  void SetUpdateFollows(bool v) { f_->SetUpdateFollows(v); b_->SetUpdateFollows(v); update_follows_ = v; }

  int32 NumParams() const { return f_->NumParams() + b_->NumParams(); }
  void GetParams(std::vector<BaseFloat> *p) const {                 // forward block, then backward block
    std::vector<BaseFloat> q;
    f_->GetParams(p);
    b_->GetParams(&q);
    p->insert(p->end(), q.begin(), q.end());
  }
  void SetParams(Direction d, const std::vector<BaseFloat> &p) { Dir(d).SetParams(p); }

  // Per-utterance lengths of the next minibatches, one per stream, 0 <= lens[s] <= T (T is checked at PropagateFnc).  Copied to the
  // device here.
  void SetSeqLengths(const std::vector<int32> &lens) {
    if ((int32)lens.size() != NumStream()) KLSTM_ERR("SetSeqLengths: " << lens.size() << " lengths for " << NumStream() << " streams");
    for (int32 v : lens) if (v < 0) KLSTM_ERR("SetSeqLengths: negative length " << v);
    lens_own_.Upload(lens, stream_);
    lens_host_ = lens;
    lens_dev_ = lens_own_.As<int32>();
  }
  // The same from S ints the caller keeps on the device (they must stay there, unchanged, until the Update of the minibatch).  The
  // kernels clamp them to [0, T]; nothing is checked on the host.
  void SetSeqLengths(const int32 *lens_dev) {
    KLSTM_ASSERT(lens_dev);
    lens_host_.clear();
    lens_dev_ = lens_dev;
  }

  void PropagateFnc(const MatrixView &in, MatrixView *out) {
    const int32 S = NumStream(), R = f_->OutputDim(), rows = in.NumRows();
    KLSTM_ASSERT(rows % S == 0);
    KLSTM_ASSERT(in.NumCols() == InputDim() && out->NumCols() == OutputDim() && out->NumRows() == rows);
    if (!lens_dev_) KLSTM_ERR("BLstmProjectedStreams: SetSeqLengths before PropagateFnc");
    const int32 T = rows / S;
    for (int32 v : lens_host_) if (v > T) KLSTM_ERR("BLstmProjectedStreams: utterance length " << v << " > " << T << " frames per stream");
    if (rows > 0) {
      KLSTM_ASSERT(klstm_pointer_on_device(f_->Engine(), in.Data()) == 1 && klstm_pointer_on_device(f_->Engine(), out->Data()) == 1);
    }
    xb_.Resize(rows, InputDim(), false);
    ob_.Resize(rows, R, false);
    std::vector<int> all(S, 1);
    f_->Reset(all);
    b_->Reset(all);
    MatrixView of(out->Data(), rows, R, out->Stride()), obv = ob_.View(), xbv = xb_.View();
    f_->PropagateFnc(in, &of);
    KCheck(klstm_reverse_streams(in.Data(), in.Stride(), S, T, InputDim(), lens_dev_, xbv.Data(), xbv.Stride(), KLSTM_REVERSE_SET, stream_));
    b_->PropagateFnc(xbv, &obv);
    KCheck(klstm_reverse_streams(obv.Data(), obv.Stride(), S, T, R, lens_dev_, out->Data() + R, out->Stride(), KLSTM_REVERSE_SET, stream_));
    KCheck(klstm_reverse_streams(nullptr, 0, S, T, R, lens_dev_, out->Data(), out->Stride(), KLSTM_REVERSE_ZERO_PAD, stream_));
    T_ = T;
  }

  // for the minibatch of the immediately preceding PropagateFnc (same `in`, same lengths)
  void BackpropagateFnc(const MatrixView &in, const MatrixView &out, const MatrixView &out_diff, MatrixView *in_diff) {
    const int32 S = NumStream(), R = f_->OutputDim(), rows = in.NumRows();
    KLSTM_ASSERT(rows == xb_.NumRows() && rows / S == T_);
    KLSTM_ASSERT(out_diff.NumRows() == rows && out_diff.NumCols() == OutputDim());
    KLSTM_ASSERT(!in_diff || (in_diff->NumRows() == rows && in_diff->NumCols() == InputDim()));
    odf_.Resize(rows, R, false);
    odb_.Resize(rows, R, false);
    MatrixView odfv = odf_.View(), odbv = odb_.View();
    KCheck(klstm_reverse_streams(out_diff.Data(), out_diff.Stride(), S, T_, R, lens_dev_, odfv.Data(), odfv.Stride(), KLSTM_REVERSE_MASK_COPY,
                                 stream_));
    f_->BackpropagateFnc(in, MatrixView(const_cast<BaseFloat *>(out.Data()), rows, R, out.Stride()), odfv, in_diff);
    KCheck(klstm_reverse_streams(out_diff.Data() + R, out_diff.Stride(), S, T_, R, lens_dev_, odbv.Data(), odbv.Stride(), KLSTM_REVERSE_SET,
                                 stream_));
    MatrixView idbv;
    if (in_diff) { idb_.Resize(rows, InputDim(), false); idbv = idb_.View(); }
    b_->BackpropagateFnc(xb_.View(), ob_.View(), odbv, in_diff ? &idbv : nullptr);
    pending_ = in_diff ? *in_diff : MatrixView();
    has_pending_ = in_diff != nullptr;
    if (!update_follows_) CombineInDiff();
  }

  void Update(const MatrixView &input, const MatrixView &diff) {
    f_->Update(input, diff);
    b_->Update(xb_.View(), odb_.View());
    CombineInDiff();
  }

 private:
  // in_diff (the forward engine's) += reverse(in_diff of the backward engine); padding rows zero
  void CombineInDiff() {
    if (!has_pending_) return;
    has_pending_ = false;
    const int32 S = NumStream();
    KCheck(klstm_reverse_streams(idb_.View().Data(), idb_.Stride(), S, T_, InputDim(), lens_dev_, pending_.Data(), pending_.Stride(),
                                 KLSTM_REVERSE_ADD, stream_));
    KCheck(klstm_reverse_streams(nullptr, 0, S, T_, InputDim(), lens_dev_, pending_.Data(), pending_.Stride(), KLSTM_REVERSE_ZERO_PAD,
                                 stream_));
  }

  std::unique_ptr<LstmProjectedStreams> f_, b_;
  void *stream_ = nullptr;
  bool update_follows_ = false;
  DeviceBuffer lens_own_;                     // device copy of SetSeqLengths(vector)
  const int32 *lens_dev_ = nullptr;           // the lengths the kernels read
  std::vector<int32> lens_host_;              // (empty with the device-pointer form)
  int32 T_ = 0;
  DeviceMatrix xb_, ob_, odf_, odb_, idb_;    // reversed in, the backward engine's out, the two out_diff halves, its in_diff
  MatrixView pending_;                        // in_diff whose backward half is still to be added (KLSTM_BPTT_FUSE_UPDATE: in Update)
  bool has_pending_ = false;
};

// The Nnet wrapper.  Its marker names the layer in messages only: this project defines no model-file form for it (see above).
class BLstmLayer : public Layer {
 public:
  explicit BLstmLayer(BLstmProjectedStreams *c) : c_(c) {}
  BLstmLayer(LstmProjectedStreams *fwd, LstmProjectedStreams *bwd) : c_(new BLstmProjectedStreams(fwd, bwd)) {}
  const char *Marker() const override { return "<BLstmProjectedStreams>"; }
  int32 InputDim() const override { return c_->InputDim(); }
  int32 OutputDim() const override { return c_->OutputDim(); }
  bool IsUpdatable() const override { return true; }
  void WriteData(std::ostream &, bool) const override {
    KLSTM_ERR("BLstmProjectedStreams has no model-file form: write its two directions (Dir(kForward), Dir(kBackward)) as "
              "<LstmProjectedStreams> components");
  }
  void PropagateFnc(const MatrixView &in, MatrixView *out) override { c_->PropagateFnc(in, out); }
  void BackpropagateFnc(const MatrixView &in, const MatrixView &out, const MatrixView &od, MatrixView *id) override { c_->BackpropagateFnc(in, out, od, id); }
  void Update(const MatrixView &a, const MatrixView &b) override { c_->Update(a, b); }
  void SetUpdateFollows(bool v) override { c_->SetUpdateFollows(v); }
  void SetTrainOptions(const NnetTrainOptions &o) override { c_->SetTrainOptions(o); }
  void SetSeqLengths(const std::vector<int32> &lens) override { c_->SetSeqLengths(lens); }
  int32 NumParams() const override { return c_->NumParams(); }
  void GetParams(std::vector<BaseFloat> *p) const override { c_->GetParams(p); }
  BLstmProjectedStreams *Impl() { return c_.get(); }
 private:
  std::unique_ptr<BLstmProjectedStreams> c_;
};

}  // namespace klstm_kaldi
