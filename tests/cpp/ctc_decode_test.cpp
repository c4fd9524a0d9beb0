// tests/cpp/ctc_decode_test.cpp -- drives CtcGreedyDecoder / DecodeCtcWholeUtterances (include/klstm_nnet.hpp) for
// tests/test_ctc_decode.py (host only: the reordering into utterance order) and tests/test_ctc_decode_gpu.py (train, decode, cross-check).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

static std::vector<int32> parse_ints(const std::string &csv) {
  std::vector<int32> v;
  std::stringstream ss(csv);
  std::string tok;
  while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(atoi(tok.c_str()));
  return v;
}
template <class T>
static void put(std::ofstream &f, const std::vector<T> &v) { f.write(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T)); }
static void put(std::ofstream &f, int32 v) { f.write(reinterpret_cast<const char *>(&v), sizeof(v)); }

// utterance i of the reordering check (tests/test_ctc.plain_utts): dim 3, feats(t, d) = 1000 i + t + d / 4, labels i, i + 1, ... (i % 5)
static Utterance plain_utt(int32 i, int32 frames) {
  Utterance u;
  u.num_frames = frames; u.dim = 3;
  u.feats.resize((size_t)frames * 3);
  for (int32 t = 0; t < frames; t++) for (int32 d = 0; d < 3; d++) u.feats[(size_t)t * 3 + d] = 1000.f * i + t + 0.25f * d;
  for (int32 j = 0; j < i % 5; j++) u.labels.push_back(i + j);
  return u;
}

// the memorisable pattern task of tests/cpp/ctc_test.cpp: `classes` - 1 labels, each a run of 3..6 frames whose features are a noisy
// one-hot pattern of the label (dim 16) -- the label sequence is a deterministic function of the features
static unsigned lcg(unsigned *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }
static Utterance pattern_utt(unsigned seed, int32 nlabels, int32 classes) {
  Utterance u;
  u.dim = 16;
  unsigned s = seed * 2654435761u + 12345u;
  for (int32 j = 0; j < nlabels; j++) {
    const int32 c = 1 + (int32)(lcg(&s) % (unsigned)(classes - 1)), run = 3 + (int32)(lcg(&s) % 4u);
    u.labels.push_back(c);
    for (int32 t = 0; t < run; t++)
      for (int32 d = 0; d < 16; d++)
        u.feats.push_back((d % (classes - 1) == c - 1 ? 1.f : 0.f) + 0.1f * ((float)(lcg(&s) % 1000u) / 1000.f - 0.5f));
    u.num_frames += run;
  }
  return u;
}
static LstmProjectedStreams *new_lstm(int32 in, int32 cell, int32 out, int32 streams) {
  std::unique_ptr<LstmProjectedStreams> c(new LstmProjectedStreams(in, out));
  std::ostringstream cfg;
  cfg << "<CellDim> " << cell << " <NumStream> " << streams << " <ParamScale> 0.1";
  std::istringstream is(cfg.str());
  c->InitData(is);
  return c.release();
}
static std::string join(const std::vector<int32> &v) {
  std::ostringstream o;
  for (size_t i = 0; i < v.size(); i++) o << (i ? "," : "") << v[i];
  return o.str();
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "order" && argc == 6) {
      // order <streams> <sort 0/1> <max_frames> <len,len,...>      host only.  The batcher's minibatches, a per-stream result made of
      // what the stream carries (frames, first feature, labels), scattered into utterance order as DecodeCtcWholeUtterances does it.
      // Prints "OK <skipped>" and one line per utterance: its result, comma separated (empty: skipped)
      const int32 S = atoi(argv[2]);
      std::vector<Utterance> utts;
      const std::vector<int32> lens = parse_ints(argv[5]);
      for (size_t i = 0; i < lens.size(); i++) utts.push_back(plain_utt((int32)i, lens[i]));
      WholeUtteranceBatcher batcher(&utts, S, atoi(argv[3]) != 0, atoi(argv[4]));
      std::vector<std::vector<int32> > per_utt(utts.size());
      UtteranceBatch b;
      while (batcher.Next(&b)) {
        std::vector<std::vector<int32> > per_stream(S);
        for (int32 s = 0; s < S; s++) {
          if (b.lens[s] == 0) continue;
          per_stream[s].push_back(b.lens[s]);
          per_stream[s].push_back((int32)b.feat[(size_t)s * b.dim]);
          per_stream[s].insert(per_stream[s].end(), b.labels[s].begin(), b.labels[s].end());
        }
        ScatterByUtterance(b, per_stream, &per_utt);
      }
      std::cout << "OK " << batcher.NumSkipped() << "\n";
      for (const auto &v : per_utt) std::cout << join(v) << "\n";
    } else if (mode == "train" && (argc == 4 || argc == 7)) {
      // train <blstm|lstm> <dump> [<epochs> <learn rate> <momentum>]      GPU.  The nets of ctc_test's train mode on a dozen pattern
      // utterances, plus one utterance beyond max_frames (skipped).  Decoded before training, trained, decoded after; a
      // cross-validation pass of TrainCtcWholeUtterances whose every_batch hook feeds a CtcGreedyDecoder (the recipe of
      // INTEGRATION.md 3e); the first minibatch of the last decode is dumped (T, S, K, labels; lens, offsets, labels, posteriors,
      // hyp_len, hyp [S*T], errors, scores, frame classes).
      // Measured: at learn rate 0.01, momentum 0.9 the bidirectional net has left the all-blank phase after 60 epochs (token error
      // rate 0), the unidirectional one still sits in it at 60 (1.0) and is at 0 after 150; learn rates of 0.02 and more diverge.
      const bool bi = std::string(argv[2]) == "blstm";
      const int32 S = 4, K = 6, epochs = argc == 7 ? atoi(argv[4]) : bi ? 60 : 150;
      std::srand(7);
      std::vector<Utterance> utts;
      for (int32 i = 0; i < 12; i++) utts.push_back(pattern_utt(100 + i, 4 + i % 7, K));
      utts.insert(utts.begin() + 5, pattern_utt(56, 40, K));        // >= 120 frames: skipped, in the middle of the list
      TrainCtcOptions o;
      o.num_stream = S;
      o.max_frames = 100;
      o.trn_opts.learn_rate = argc == 7 ? (float)atof(argv[5]) : 0.01f;
      o.trn_opts.momentum = argc == 7 ? (float)atof(argv[6]) : 0.9f;
      Nnet nnet;
      nnet.AppendComponent(new TransmitLayer(16, 16));
      if (bi) {
        std::unique_ptr<LstmProjectedStreams> f(new_lstm(16, 32, 16, S)), b(new_lstm(16, 32, 16, S));
        LstmProjectedStreams *fp = f.release(), *bp = b.release();
        nnet.AppendComponent(new BLstmLayer(fp, bp));
      } else {
        nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
        nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      }
      const int32 H = bi ? 32 : 16;
      AffineLayer *aff = new AffineLayer(H, K);
      std::vector<BaseFloat> w((size_t)K * H), bias(K, 0.f);
      for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
      aff->SetParams(w, bias);
      nnet.AppendComponent(aff);
      nnet.AppendComponent(new SoftmaxLayer(K, K));

      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      std::vector<std::vector<int32> > hyp0, hyp1;
      const DecodeCtcStats before = DecodeCtcWholeUtterances(&nnet, utts, d, &hyp0);
      double last = 0;
      for (int32 e = 0; e < epochs; e++) {
        const TrainCtcStats st = TrainCtcWholeUtterances(&nnet, utts, o);
        last = st.avg_loss_per_frame;
        if (e % 10 == 0 || e == epochs - 1) std::cerr << "epoch " << e << " loss/frame " << st.avg_loss_per_frame << "\n";
      }
      int32 mb = 0;
      std::string report;
      const DecodeCtcStats after = DecodeCtcWholeUtterances(&nnet, utts, d, &hyp1, &report,
          [&](const UtteranceBatch &b, const DeviceMatrix &y, const CtcGreedyDecoder &dec) {
            if (mb++ != 0) return;
            std::vector<BaseFloat> post, score;
            std::vector<int32> err, fc;
            y.CopyToHost(&post); dec.UttScores(&score); dec.UttErrors(&err); dec.FrameClasses(&fc);
            std::vector<int32> off(1, 0), flat, hlen, hyp((size_t)b.num_frames * b.num_stream, -1);
            for (const auto &l : b.labels) { flat.insert(flat.end(), l.begin(), l.end()); off.push_back((int32)flat.size()); }
            for (int32 s = 0; s < b.num_stream; s++) {
              const std::vector<int32> &h = b.utt_index[s] >= 0 ? hyp1[b.utt_index[s]] : std::vector<int32>();
              hlen.push_back((int32)h.size());
              std::copy(h.begin(), h.end(), hyp.begin() + (size_t)s * b.num_frames);
            }
            std::ofstream f(argv[3], std::ios::binary);
            put(f, b.num_frames); put(f, b.num_stream); put(f, K); put(f, (int32)flat.size());
            put(f, b.lens); put(f, off); put(f, flat); put(f, post); put(f, hlen); put(f, hyp); put(f, err); put(f, score); put(f, fc);
          });
      // the token error rate of a cross-validation pass through the existing every_batch hook
      TrainCtcOptions cv = o;
      cv.crossvalidate = true;
      CtcGreedyDecoder cvdec(cv.blank);
      TrainCtcWholeUtterances(&nnet, utts, cv, nullptr,
          [&](const UtteranceBatch &b, const DeviceMatrix &y, const DeviceMatrix &, const Ctc &) { cvdec.Decode(y, b.num_stream, b.lens, b.labels, nullptr); });
      // hypotheses in the order of utts: an utterance decoded ALONE gives the same hypothesis (the net sees whole utterances from zero state)
      bool in_order = hyp1.size() == utts.size() && hyp1[5].empty();
      for (size_t i = 0; i < utts.size() && in_order; i += 4) {
        if (i == 5) continue;
        std::vector<Utterance> one(1, utts[i]);
        std::vector<std::vector<int32> > h;
        DecodeCtcWholeUtterances(&nnet, one, d, &h);
        in_order = h.size() == 1 && h[0] == hyp1[i];
      }
      std::cerr << report << "\n";
      for (size_t i = 0; i < utts.size(); i++) std::cerr << "utt " << i << " ref " << join(utts[i].labels) << " hyp " << join(hyp1[i]) << "\n";
      std::cout << "OK ter_before=" << before.token_error_rate << " ter_after=" << after.token_error_rate << " uer_after=" << after.utt_error_rate
                << " ter_crossvalidate=" << cvdec.TokenErrorRate() << " scored=" << (int)after.num_scored << " cv_scored=" << (int)cvdec.NumUtterances()
                << " skipped=" << after.num_skipped << " in_order=" << (int)in_order << " last_epoch_loss_per_frame=" << last
                << " errors_after=" << (int)after.num_errors << " ref_tokens=" << (int)after.num_ref_tokens << "\n";
    } else {
      std::cerr << "usage: ctc_decode_test order <streams> <sort> <max_frames> <lens> | train <blstm|lstm> <dump> [<epochs> <learn rate> <momentum>]\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
