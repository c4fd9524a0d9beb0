// include/klstm_scorer.hpp -- batched forward-only scoring of many utterances through a klstm::Nnet, and the FAQ's google -> standard
// model conversion as code (README.md of the reference, Q1).
//
// The per-utterance way to score a model is the nnet-forward workalike (klstm_nnet.hpp Nnet::Feedforward) on the standard form:
// LstmProjected with ONE stream, the slowest row of the dispatch table (a latency-bound chain), activation planes written for a
// BPTT that never comes, a Softmax launch of its own.  BatchScorer packs the utterances into the S streams of engines of its own
// instead, runs the LSTM stack forward only (klstm_propagate_inference) chunk by chunk, and writes each utterance's rows through
// one fused output kernel (klstm_log_softmax_scatter).  An utterance starts at a chunk boundary with its stream reset -- the
// trainer's scheme (bd-nnet-train-lstm-streams.cc:146-209) -- and the state carries across chunks, so the chunk length does not
// change the result.
// Header-only C++ over the C-ABI (klstm.h); no HIP or Kaldi headers needed.
#pragma once
#include <algorithm>
#include <climits>
#include <memory>
#include <sstream>

#include "klstm_nnet.hpp"

namespace klstm_kaldi {

// ---- FAQ Q1 as code: <Transmit> -> <TimeShift> <Shift> shift, <LstmProjectedStreams> -> <LstmProjected> (no <NumStream>),
// parameters unchanged.  A model that does not begin with the <Transmit> (the shift would have nowhere to go), a <TimeShift> already in
// the model, or a component other than these and <AffineTransform> / <Softmax>, is refused; a <Dropout> is left out (WithoutDropout).  (The model is read through its binary form: the result is what Nnet::Read makes of the converted file.)
inline void ConvertToStandard(const Nnet &in, int32 shift, Nnet *out) {
  if (in.NumComponents() == 0 || std::string(in.GetComponent(0).Marker()) != "<Transmit>")
    KLSTM_ERR("ConvertToStandard: the first component is " << (in.NumComponents() ? in.GetComponent(0).Marker() : "missing")
              << ", not the <Transmit> that becomes <TimeShift> <Shift> " << shift << " (the shift would be lost)");
  std::stringstream ss;
  WriteToken(ss, true, "<Nnet>");
  for (int32 i = 0; i < in.NumComponents(); i++) {
    const Layer &l = in.GetComponent(i);
    const std::string m = l.Marker();
    if (m == "<Transmit>") {
      if (i != 0) KLSTM_ERR("ConvertToStandard: <Transmit> at position " << i << " (only the first component may be one)");
      WriteToken(ss, true, "<TimeShift>"); WriteBasicType(ss, true, l.OutputDim()); WriteBasicType(ss, true, l.InputDim());
      WriteToken(ss, true, "<Shift>"); WriteBasicType(ss, true, shift); ss << "\n";
    } else if (m == "<LstmProjectedStreams>" || m == "<LstmProjected>") {
      const LstmProjectedStreams *c = static_cast<const LstmLayer &>(l).Impl();
      const int32 I = c->InputDim(), R = c->OutputDim(), C = c->CellDim();
      std::vector<BaseFloat> p;
      c->GetParams(&p);
      WriteToken(ss, true, "<LstmProjected>"); WriteBasicType(ss, true, R); WriteBasicType(ss, true, I);
      WriteToken(ss, true, "<CellDim>"); WriteBasicType(ss, true, C);
      const BaseFloat *q = p.data();
      WriteMatrix(ss, true, q, 4 * C, I, I); q += (size_t)4 * C * I;
      WriteMatrix(ss, true, q, 4 * C, R, R); q += (size_t)4 * C * R;
      WriteVector(ss, true, q, 4 * C); q += 4 * C;
      for (int k = 0; k < 3; k++) { WriteVector(ss, true, q, C); q += C; }
      WriteMatrix(ss, true, q, R, C, C);
    } else if (m == "<AffineTransform>" || m == "<Softmax>") {
      l.Write(ss, true);
    } else if (m == "<Dropout>") {                          // a copy at inference: dropped, as WithoutDropout drops it
    } else {
      KLSTM_ERR("ConvertToStandard: " << m << " at position " << i << " has no standard form here (the google model is "
                "<Transmit> <LstmProjectedStreams>... <AffineTransform> <Softmax>)");
    }
  }
  WriteToken(ss, true, "</Nnet>");
  out->Read(ss, true);
}

// ---- the chunk plan: which utterance frame every row of every chunk carries (a pure host function) ----
// Utterances go to streams greedily and back to back, in order: at every chunk boundary each stream whose utterance is finished takes
// the next one (streams in order 0..S-1), as the trainer's batcher does (bd-nnet-train-lstm-streams.cc:146-174).  Zero-length
// utterances are skipped.  Per chunk and stream: desc = {row offset of the utterance in the concatenated input, its length, the
// frame the chunk starts at} ({0, 0, 0}: idle), reset = 1 where an utterance starts (or the stream is idle); per row t*S + s of the
// chunk: dst = off + start + t while that frame exists, else -1 (padding).  Output rows are laid out like the input rows.
struct ScorePlan {
  int32 S = 0, T = 0, num_chunks = 0;
  std::vector<int32> desc;    // [num_chunks][S][3]
  std::vector<int32> reset;   // [num_chunks][S]
  std::vector<int32> dst;     // [num_chunks][T * S]
};
inline ScorePlan PlanChunks(const std::vector<int32> &lens, int32 S, int32 T) {
  if (S <= 0 || T <= 0) KLSTM_ERR("PlanChunks: num_stream (" << S << ") and chunk length (" << T << ") must be positive");
  ScorePlan p;
  p.S = S; p.T = T;
  std::vector<long> off(lens.size() + 1, 0);
  for (size_t u = 0; u < lens.size(); u++) {
    if (lens[u] < 0) KLSTM_ERR("PlanChunks: negative utterance length");
    off[u + 1] = off[u] + lens[u];
  }
  if (off.back() > INT_MAX) KLSTM_ERR("PlanChunks: more than 2^31 rows");
  std::vector<int32> utt(S, -1), cur(S, 0);
  size_t next = 0;
  while (true) {
    for (int32 s = 0; s < S; s++) {
      if (utt[s] >= 0 && cur[s] < lens[utt[s]]) continue;
      utt[s] = -1;
      while (next < lens.size() && lens[next] == 0) next++;
      if (next < lens.size()) { utt[s] = (int32)next++; cur[s] = 0; }
    }
    bool any = false;
    for (int32 s = 0; s < S; s++) any |= utt[s] >= 0;
    if (!any) break;
    for (int32 s = 0; s < S; s++) {
      const bool on = utt[s] >= 0;
      p.desc.push_back(on ? (int32)off[utt[s]] : 0);
      p.desc.push_back(on ? lens[utt[s]] : 0);
      p.desc.push_back(on ? cur[s] : 0);
      p.reset.push_back(!on || cur[s] == 0 ? 1 : 0);
    }
    const size_t d0 = p.dst.size();
    p.dst.resize(d0 + (size_t)T * S);
    for (int32 t = 0; t < T; t++)
      for (int32 s = 0; s < S; s++) {
        const bool on = utt[s] >= 0 && cur[s] + t < lens[utt[s]];
        p.dst[d0 + (size_t)t * S + s] = on ? (int32)off[utt[s]] + cur[s] + t : -1;
      }
    for (int32 s = 0; s < S; s++) if (utt[s] >= 0) cur[s] += T;
    p.num_chunks++;
  }
  return p;
}

struct BatchScorerOptions {
  int32 num_stream = 16;                // (a stack with 512-input layers scores faster at 8 today: DESIGN.md 3, "Batched scoring")
  int32 chunk = 50;                     // frames per stream and chunk: the fastest of 20 / 50 / 100 at 16 streams (tools/score_bench.py)
  int32 targets_delay = INT_MIN;        // the shift of a <Transmit> (google) model; INT_MIN: not given (0 for such a model)
  int mode = KLSTM_SCORE_POSTERIOR;     // KLSTM_SCORE_POSTERIOR / _LOGPOST / _LOGLIKE (klstm.h klstm_log_softmax_scatter)
  std::vector<BaseFloat> log_prior;     // KLSTM_SCORE_LOGLIKE: one log prior per output column
  BaseFloat prior_scale = 1.f;
  int device = 0;
};

// Accepted topologies (what Nnet::Read reads): [<Transmit> | <TimeShift>] <LstmProjectedStreams | LstmProjected>... <AffineTransform>
// [<Softmax>].  The first component's shift goes into the pack; the Softmax, if any, into the output kernel (KLSTM_SCORE_POSTERIOR
// gives what the model outputs; the log forms are computed from the Affine rows directly).  The model is only read: the scorer
// builds engines of its own with NumStream = num_stream from the model's current parameters.
class BatchScorer {
 public:
  BatchScorer(const Nnet &nnet, const BatchScorerOptions &o) : o_(o) {
    int32 i0 = 0, i1 = 0;
    shift_ = CheckTopology(nnet, o, &i0, &i1);       // (before anything touches a device: a refused model needs no GPU)
    in_dim_ = nnet.GetComponent(0).InputDim();
    for (int32 i = i0; i < i1; i++) {
      const LstmProjectedStreams *c = static_cast<const LstmLayer &>(nnet.GetComponent(i)).Impl();
      std::vector<BaseFloat> p;
      c->GetParams(&p);
      klstm_engine *e = nullptr;
      KCheck(klstm_create(c->InputDim(), c->CellDim(), c->OutputDim(), o.num_stream, o.device, nullptr, &e));
      engines_.emplace_back(e);
      KCheck(klstm_set_params_host(e, p.data()));
      KCheck(klstm_set_option(e, "persist_verify", 1));   // a persistent launch that gives up is run again inside its call (klstm.h "persist")
      dims_.push_back(c->OutputDim());
    }
    const AffineLayer &aff = static_cast<const AffineLayer &>(nnet.GetComponent(i1));
    std::vector<BaseFloat> w, b;
    aff.HostParams(&w, &b);
    aff_in_ = aff.InputDim(); out_dim_ = aff.OutputDim();
    W_.Upload(w); b_.Upload(b);
    if (o.mode == KLSTM_SCORE_LOGLIKE) lp_.Upload(o.log_prior);
    const int32 rows = o.num_stream * o.chunk;
    int32 wmax = in_dim_;
    for (int32 d : dims_) wmax = std::max(wmax, d);
    for (int k = 0; k < 2; k++) act_[k].Resize(rows, wmax, false);
    aout_.Resize(rows, out_dim_, false);
  }
  // The checks of the constructor, host only: returns the shift of the pack; [*lstm_begin, *lstm_end) are the LSTM components and
  // *lstm_end the <AffineTransform>.  Raises (KLSTM_ERR) on a topology or an option the scorer does not take.
  static int32 CheckTopology(const Nnet &nnet, const BatchScorerOptions &o, int32 *lstm_begin = nullptr, int32 *lstm_end = nullptr) {
    if (o.num_stream < 1 || o.num_stream > 256 || o.chunk < 1) KLSTM_ERR("BatchScorer: num_stream must be 1..256 and chunk >= 1");
    if ((long)o.num_stream * o.chunk > 65535) KLSTM_ERR("BatchScorer: num_stream * chunk > 65535");
    if (o.mode != KLSTM_SCORE_POSTERIOR && o.mode != KLSTM_SCORE_LOGPOST && o.mode != KLSTM_SCORE_LOGLIKE) KLSTM_ERR("BatchScorer: unknown mode");
    const int32 n = nnet.NumComponents();
    auto marker = [&](int32 i) { return i < n ? std::string(nnet.GetComponent(i).Marker()) : std::string("(end of the model)"); };
    auto hint = [&](int32 i) { return marker(i) == "<Dropout>" ? " (pass the model through WithoutDropout first)" : ""; };
    int32 i = 0, shift = 0;
    if (marker(0) == "<TimeShift>") {
      shift = static_cast<const TimeShiftLayer &>(nnet.GetComponent(0)).Shift();
      if (o.targets_delay != INT_MIN)
        KLSTM_ERR("BatchScorer: the model has a <TimeShift> (shift " << shift << "): a targets_delay as well is ambiguous");
      i = 1;
    } else {
      if (o.targets_delay != INT_MIN) shift = o.targets_delay;
      if (marker(0) == "<Transmit>") i = 1;
    }
    const int32 b = i;
    while (marker(i) == "<LstmProjectedStreams>" || marker(i) == "<LstmProjected>") i++;
    if (i == b) KLSTM_ERR("BatchScorer: " << marker(i) << " at component " << i << " where an <LstmProjectedStreams> / <LstmProjected> belongs" << hint(i));
    if (marker(i) != "<AffineTransform>") KLSTM_ERR("BatchScorer: " << marker(i) << " at component " << i << " where the <AffineTransform> belongs" << hint(i));
    const int32 e = i++;
    if (marker(i) == "<Softmax>") i++;
    if (i != n) KLSTM_ERR("BatchScorer: " << marker(i) << " at component " << i << " is not supported (accepted: "
                          "[<Transmit>|<TimeShift>] <LstmProjected[Streams]>... <AffineTransform> [<Softmax>])" << hint(i));
    if (o.mode == KLSTM_SCORE_LOGLIKE && (int32)o.log_prior.size() != nnet.GetComponent(e).OutputDim())
      KLSTM_ERR("BatchScorer: log_prior needs " << nnet.GetComponent(e).OutputDim() << " values");
    if (lstm_begin) *lstm_begin = b;
    if (lstm_end) *lstm_end = e;
    return shift;
  }
  BatchScorer(const BatchScorer &) = delete;
  BatchScorer &operator=(const BatchScorer &) = delete;

  int32 InputDim() const { return in_dim_; }
  int32 OutputDim() const { return out_dim_; }
  int32 Shift() const { return shift_; }

  // Device API: feats_dev = the utterances' rows concatenated (row stride feat_stride), lens = their lengths; out_dev receives the
  // scores in the same row layout (row stride out_stride >= OutputDim()).  Asynchronous on the library's stream (klstm_create with a
  // NULL stream); klstm_stream_synchronize(nullptr) waits for it.
  void ScoreDevice(const BaseFloat *feats_dev, int32 feat_stride, const std::vector<int32> &lens, BaseFloat *out_dev, int32 out_stride) {
    const int32 S = o_.num_stream, T = o_.chunk, rows = S * T;
    const ScorePlan p = PlanChunks(lens, S, T);
    if (!p.num_chunks) return;
    if (feat_stride < in_dim_ || out_stride < out_dim_) KLSTM_ERR("BatchScorer: stride smaller than the row");
    KCheck(klstm_stream_synchronize(nullptr));        // (the plan arrays may still be read by an earlier call's kernels)
    pdesc_.Upload(p.desc);
    pdst_.Upload(p.dst);
    std::vector<int> flags(S);
    for (int32 c = 0; c < p.num_chunks; c++) {
      KCheck(klstm_pack_streams(feats_dev, in_dim_, feat_stride, pdesc_.As<int32>() + (size_t)c * 3 * S, S, T, shift_, act_[0].View().Data(),
                                act_[0].Stride(), nullptr, nullptr));
      for (int32 s = 0; s < S; s++) flags[s] = p.reset[(size_t)c * S + s];
      int k = 0;
      for (auto &eng : engines_) {
        klstm_engine *e = eng.get();
        KCheck(klstm_reset(e, flags.data(), S));
        KCheck(klstm_propagate_inference(e, act_[k].View().Data(), rows, act_[k].Stride(), act_[k ^ 1].View().Data(), act_[k ^ 1].Stride()));
        k ^= 1;
      }
      KCheck(klstm_affine_propagate(act_[k].View().Data(), rows, aff_in_, act_[k].Stride(), W_.As<BaseFloat>(), b_.As<BaseFloat>(),
                                    aout_.View().Data(), out_dim_, aout_.Stride(), nullptr));
      KCheck(klstm_log_softmax_scatter(aout_.View().Data(), rows, out_dim_, aout_.Stride(), pdst_.As<int32>() + (size_t)c * rows, out_dev,
                                       out_stride, o_.mode, lp_.As<BaseFloat>(), o_.prior_scale, nullptr));
    }
  }
  // The loop of ScoreDevice for a consumer that works chunk by chunk (CtcStreamDecoder::Step): every chunk's scores go to fn in CHUNK
  // layout, a [chunk * num_stream x OutputDim()] matrix with rows t * num_stream + s, instead of the utterances' rows.  fn(scores,
  // info) also learns per stream how many frames of the chunk are the utterance's (rows behind them are padding), whether its
  // utterance starts and whether it ends with this chunk, and the utterance's index in lens (-1: idle).  Asynchronous like
  // ScoreDevice: fn queues its own work on the library's stream.
  struct ChunkInfo { std::vector<int32> frames, start, end, utt; };
  template <class F>
  void ForEachChunk(const BaseFloat *feats_dev, int32 feat_stride, const std::vector<int32> &lens, F fn) {
    const int32 S = o_.num_stream, T = o_.chunk, rows = S * T;
    const ScorePlan p = PlanChunks(lens, S, T);
    if (!p.num_chunks) return;
    if (feat_stride < in_dim_) KLSTM_ERR("BatchScorer: stride smaller than the row");
    std::vector<std::pair<int32, int32> > by_off;     // (row offset, index) of the utterances with frames: offsets ascend
    for (size_t u = 0, off = 0; u < lens.size(); off += lens[u++])
      if (lens[u] > 0) by_off.emplace_back((int32)off, (int32)u);
    KCheck(klstm_stream_synchronize(nullptr));
    pdesc_.Upload(p.desc);
    std::vector<int32> ident(rows);
    for (int32 r = 0; r < rows; r++) ident[r] = r;
    pdst_.Upload(ident);
    cpost_.Resize(rows, out_dim_, false);
    std::vector<int> flags(S);
    ChunkInfo info;
    for (int32 c = 0; c < p.num_chunks; c++) {
      KCheck(klstm_pack_streams(feats_dev, in_dim_, feat_stride, pdesc_.As<int32>() + (size_t)c * 3 * S, S, T, shift_, act_[0].View().Data(),
                                act_[0].Stride(), nullptr, nullptr));
      for (int32 s = 0; s < S; s++) flags[s] = p.reset[(size_t)c * S + s];
      int k = 0;
      for (auto &eng : engines_) {
        klstm_engine *e = eng.get();
        KCheck(klstm_reset(e, flags.data(), S));
        KCheck(klstm_propagate_inference(e, act_[k].View().Data(), rows, act_[k].Stride(), act_[k ^ 1].View().Data(), act_[k ^ 1].Stride()));
        k ^= 1;
      }
      KCheck(klstm_affine_propagate(act_[k].View().Data(), rows, aff_in_, act_[k].Stride(), W_.As<BaseFloat>(), b_.As<BaseFloat>(),
                                    aout_.View().Data(), out_dim_, aout_.Stride(), nullptr));
      KCheck(klstm_log_softmax_scatter(aout_.View().Data(), rows, out_dim_, aout_.Stride(), pdst_.As<int32>(), cpost_.View().Data(),
                                       cpost_.Stride(), o_.mode, lp_.As<BaseFloat>(), o_.prior_scale, nullptr));
      info.frames.assign(S, 0); info.start.assign(S, 0); info.end.assign(S, 0); info.utt.assign(S, -1);
      for (int32 s = 0; s < S; s++) {
        const int32 *d = &p.desc[((size_t)c * S + s) * 3];
        if (d[1] <= 0) continue;
        info.frames[s] = std::min(T, d[1] - d[2]);
        info.start[s] = d[2] == 0;
        info.end[s] = d[2] + T >= d[1];
        info.utt[s] = std::lower_bound(by_off.begin(), by_off.end(), std::make_pair(d[0], (int32)-1))->second;
      }
      fn(static_cast<const DeviceMatrix &>(cpost_), static_cast<const ChunkInfo &>(info));
    }
  }
  // Host API: one [len x InputDim()] row-major matrix per utterance in, one [len x OutputDim()] matrix per utterance out.
  void Score(const std::vector<std::vector<BaseFloat> > &utts, std::vector<std::vector<BaseFloat> > *out) {
    std::vector<int32> lens;
    long total = 0;
    for (const auto &u : utts) {
      if (u.size() % (size_t)in_dim_) KLSTM_ERR("BatchScorer::Score: an utterance is not a whole number of " << in_dim_ << "-wide rows");
      lens.push_back((int32)(u.size() / in_dim_)); total += lens.back();
    }
    out->assign(utts.size(), std::vector<BaseFloat>());
    if (!total) return;
    std::vector<BaseFloat> cat((size_t)total * in_dim_);
    size_t o = 0;
    for (const auto &u : utts) { std::copy(u.begin(), u.end(), cat.begin() + o); o += u.size(); }
    DeviceMatrix fin, fout;
    fin.CopyFromHost(cat.data(), (int32)total, in_dim_);
    fout.Resize((int32)total, out_dim_, false);
    ScoreDevice(fin.View().Data(), fin.Stride(), lens, fout.View().Data(), fout.Stride());
    KCheck(klstm_stream_synchronize(nullptr));
    std::vector<BaseFloat> all;
    fout.CopyToHost(&all);
    o = 0;
    for (size_t u = 0; u < utts.size(); u++) {
      (*out)[u].assign(all.begin() + o, all.begin() + o + (size_t)lens[u] * out_dim_);
      o += (size_t)lens[u] * out_dim_;
    }
  }

 private:
  BatchScorerOptions o_;
  int32 shift_ = 0, in_dim_ = 0, aff_in_ = 0, out_dim_ = 0;
  struct EngineDel { void operator()(klstm_engine *e) const { klstm_destroy(e); } };
  std::vector<std::unique_ptr<klstm_engine, EngineDel> > engines_;
  std::vector<int32> dims_;
  DeviceBuffer W_, b_, lp_;                   // lp_ stays empty (null) unless the mode is KLSTM_SCORE_LOGLIKE
  DeviceBuffer pdesc_, pdst_;                 // the plan of the ScoreDevice call in flight
  DeviceMatrix act_[2], aout_, cpost_;        // cpost_: the chunk ForEachChunk hands out
};

// Streaming CTC decoding of a unidirectional model: the scorer's chunk loop with a CtcStreamDecoder behind it.  The forward pass and
// the search advance together chunk by chunk, nothing of an utterance but its beam is kept, and an utterance may be as long as the
// state is sized for (max_frames = the longest one): the limit of DecodeCtcWholeUtterances (65535 / num_stream frames) does not
// apply.  so: num_stream <= 32 and the chunk length; o: blank, beam > 0, cands, nbest, class weights, lm, score as
// DecodeCtcWholeUtterances takes them; o.max_frames > 0 skips longer utterances as the batcher there does.  (*hypotheses)[i] is the
// 1-best of utts[i], (*nbest_lists)[i] its list (either may be null; both empty for a skipped utterance).  A bidirectional model
// needs the whole utterance before its first output row exists and is refused, before any device work.
inline DecodeCtcStats DecodeCtcStreaming(const Nnet &nnet, const std::vector<Utterance> &utts, const BatchScorerOptions &so,
                                         const DecodeCtcOptions &o, std::vector<std::vector<int32> > *hypotheses,
                                         std::vector<CtcNbestList> *nbest_lists, std::string *report = nullptr) {
  for (int32 i = 0; i < nnet.NumComponents(); i++)
    if (std::string(nnet.GetComponent(i).Marker()).find("<BLstm") == 0)
      KLSTM_ERR("DecodeCtcStreaming: " << nnet.GetComponent(i).Marker() << " at component " << i << " is bidirectional: its first output row "
                "needs the last input row, so there is nothing to stream (use DecodeCtcWholeUtterances)");
  if (o.beam <= 0) KLSTM_ERR("DecodeCtcStreaming: beam must be positive (the best path needs no carried beam)");
  if (so.mode != KLSTM_SCORE_POSTERIOR) KLSTM_ERR("DecodeCtcStreaming: the search reads posteriors (BatchScorerOptions::mode KLSTM_SCORE_POSTERIOR)");
  if (so.num_stream > 32) KLSTM_ERR("DecodeCtcStreaming: num_stream " << so.num_stream << " > 32");
  BatchScorer::CheckTopology(nnet, so);
  if (hypotheses) hypotheses->assign(utts.size(), std::vector<int32>());
  if (nbest_lists) nbest_lists->assign(utts.size(), CtcNbestList());
  DecodeCtcStats st;
  const int32 dim = nnet.GetComponent(0).InputDim();
  std::vector<int32> lens(utts.size(), 0);
  long total = 0;
  int32 longest = 0;
  for (size_t u = 0; u < utts.size(); u++) {
    const Utterance &ut = utts[u];
    if (ut.num_frames <= 0 || (o.max_frames > 0 && ut.num_frames > o.max_frames)) { st.num_skipped++; continue; }
    if (ut.dim != dim || ut.feats.size() != (size_t)ut.num_frames * dim) KLSTM_ERR("DecodeCtcStreaming: utterance " << u << " is not [frames x " << dim << "]");
    lens[u] = ut.num_frames; total += ut.num_frames; longest = std::max(longest, ut.num_frames); st.num_done++;
  }
  if (!total) return st;
  if (total > INT_MAX) KLSTM_ERR("DecodeCtcStreaming: more than 2^31 rows");
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<BaseFloat> cat((size_t)total * dim);
  size_t at = 0;
  for (size_t u = 0; u < utts.size(); u++)
    if (lens[u]) { std::copy(utts[u].feats.begin(), utts[u].feats.end(), cat.begin() + at); at += utts[u].feats.size(); }
  DeviceMatrix feats;
  feats.CopyFromHost(cat.data(), (int32)total, dim);
  BatchScorer scorer(nnet, so);
  CtcStreamDecoder dec(o.blank, o.beam, o.cands, o.nbest, so.num_stream, longest);
  dec.SetClassWeights(o.class_weights);
  KLSTM_ASSERT(!o.lm || !o.slm);
  if (o.slm) dec.SetLanguageModel(o.slm); else dec.SetLanguageModel(o.lm);
  const int32 S = so.num_stream;
  std::vector<CtcNbestList> lists;
  std::vector<int32> mode(S);
  std::vector<std::vector<int32> > refs(S);
  const std::vector<std::vector<int32> > none;
  scorer.ForEachChunk(feats.View().Data(), feats.Stride(), lens, [&](const DeviceMatrix &post, const BatchScorer::ChunkInfo &info) {
    dec.Step(post, info.frames, info.start);
    st.num_minibatches++;
    bool any = false;
    for (int32 s = 0; s < S; s++) {
      mode[s] = info.frames[s] > 0 && info.end[s] ? 2 : 0;
      refs[s] = mode[s] && o.score ? utts[info.utt[s]].labels : std::vector<int32>();
      any |= mode[s] != 0;
    }
    if (!any) return;
    dec.Emit(mode, o.score ? refs : none, hypotheses || nbest_lists ? &lists : nullptr, nullptr, nullptr);
    for (int32 s = 0; s < S && (hypotheses || nbest_lists); s++) {
      if (!mode[s]) continue;
      if (hypotheses && !lists[s].empty()) (*hypotheses)[info.utt[s]] = lists[s][0].tokens;
      if (nbest_lists) (*nbest_lists)[info.utt[s]] = lists[s];
    }
  });
  KCheck(klstm_stream_synchronize(nullptr));
  st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  st.oracle_token_error_rate = dec.OracleTokenErrorRate();
  FillDecodeCtcStats(dec, &st, report);
  return st;
}

}  // namespace klstm_kaldi
