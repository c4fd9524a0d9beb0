// tests/cpp/ctc_beam_test.cpp -- drives CtcBeamDecoder / DecodeCtcWholeUtterances with beam > 0 (include/klstm_nnet.hpp) for
// tests/test_ctc_beam_gpu.py: train the pattern task, decode greedily and with the prefix beam search, cross-check.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

template <class T>
static void put(std::ofstream &f, const std::vector<T> &v) { f.write(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T)); }
static void put(std::ofstream &f, int32 v) { f.write(reinterpret_cast<const char *>(&v), sizeof(v)); }

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

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "train" && argc == 4) {
      // train <blstm|lstm> <dump>      GPU.  The nets and the schedule of ctc_decode_test's train mode.  After training: the greedy
      // decode (beam = 0), the beam decode (beam 8, 5 candidates, 4-best) with its lists, and a cross-validation pass of
      // TrainCtcWholeUtterances whose every_batch hook feeds a CtcBeamDecoder (the recipe of INTEGRATION.md 3g).  The first minibatch
      // of the beam decode is dumped (T, S, K, N; lens, posteriors, count [S], hyp_len [S*N], scores [S*N], hyp [S*N*T]).
      const bool bi = std::string(argv[2]) == "blstm";
      const int32 S = 4, K = 6, epochs = bi ? 60 : 150, N = 4;
      std::srand(7);
      std::vector<Utterance> utts;
      for (int32 i = 0; i < 12; i++) utts.push_back(pattern_utt(100 + i, 4 + i % 7, K));
      utts.insert(utts.begin() + 5, pattern_utt(56, 40, K));        // >= 120 frames: skipped, in the middle of the list
      TrainCtcOptions o;
      o.num_stream = S;
      o.max_frames = 100;
      o.trn_opts.learn_rate = 0.01f;
      o.trn_opts.momentum = 0.9f;
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
      for (int32 e = 0; e < epochs; e++) TrainCtcWholeUtterances(&nnet, utts, o);

      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      std::vector<std::vector<int32> > greedy, greedy0, best;
      const DecodeCtcStats g = DecodeCtcWholeUtterances(&nnet, utts, d, &greedy);
      int32 calls = 0;
      const DecodeCtcStats g0 = DecodeCtcWholeUtterances(&nnet, utts, d, &greedy0, nullptr,
          [&](const UtteranceBatch &, const DeviceMatrix &, const CtcGreedyDecoder &) { calls++; });      // beam = 0: the loop as it was
      DecodeCtcOptions bo = d;
      bo.beam = 8; bo.cands = 5; bo.nbest = N;
      std::vector<CtcNbestList> lists;
      std::string report;
      int32 mb = 0;
      const DecodeCtcStats bs = DecodeCtcWholeUtterances(&nnet, utts, bo, &best, &lists, &report,
          [&](const UtteranceBatch &b, const DeviceMatrix &y, const CtcBeamDecoder &) {
            if (mb++ != 0) return;
            std::vector<BaseFloat> post, score((size_t)b.num_stream * N, 0.f);
            y.CopyToHost(&post);
            std::vector<int32> cnt, hlen((size_t)b.num_stream * N, 0), hyp((size_t)b.num_stream * N * b.num_frames, -1);
            for (int32 s = 0; s < b.num_stream; s++) {
              const CtcNbestList &l = b.utt_index[s] >= 0 ? lists[b.utt_index[s]] : CtcNbestList();
              cnt.push_back((int32)l.size());
              for (size_t q = 0; q < l.size(); q++) {
                hlen[(size_t)s * N + q] = (int32)l[q].tokens.size();
                score[(size_t)s * N + q] = l[q].score;
                std::copy(l[q].tokens.begin(), l[q].tokens.end(), hyp.begin() + ((size_t)s * N + q) * b.num_frames);
              }
            }
            std::ofstream f(argv[3], std::ios::binary);
            put(f, b.num_frames); put(f, b.num_stream); put(f, K); put(f, N);
            put(f, b.lens); put(f, post); put(f, cnt); put(f, hlen); put(f, score); put(f, hyp);
          });
      // the 1-best overload: hypotheses only
      std::vector<std::vector<int32> > best1;
      const DecodeCtcStats b1 = DecodeCtcWholeUtterances(&nnet, utts, bo, &best1);
      // the error rates of a cross-validation pass through the existing every_batch hook
      TrainCtcOptions cv = o;
      cv.crossvalidate = true;
      CtcBeamDecoder cvdec(cv.blank, bo.beam, bo.cands, bo.nbest);
      TrainCtcWholeUtterances(&nnet, utts, cv, nullptr,
          [&](const UtteranceBatch &b, const DeviceMatrix &y, const DeviceMatrix &, const Ctc &) { cvdec.Decode(y, b.num_stream, b.lens, b.labels, nullptr); });
      bool lists_ok = lists.size() == utts.size() && lists[5].empty() && best[5].empty();
      int32 oracle = 0;
      for (size_t i = 0; i < utts.size() && lists_ok; i++) {
        if (i == 5) continue;
        lists_ok = !lists[i].empty() && (int32)lists[i].size() <= N && lists[i][0].tokens == best[i];
        int32 m = 1 << 30;
        for (size_t q = 0; q < lists[i].size(); q++) {
          m = std::min(m, lists[i][q].errors);
          if (q > 0) lists_ok = lists_ok && lists[i][q].score <= lists[i][q - 1].score && lists[i][q].tokens != lists[i][0].tokens;
        }
        oracle += m;
      }
      std::cerr << report << "\n";
      std::cout << "OK ter_greedy=" << g.token_error_rate << " ter_beam=" << bs.token_error_rate << " oracle_beam=" << bs.oracle_token_error_rate
                << " uer_beam=" << bs.utt_error_rate << " ter_crossvalidate=" << cvdec.TokenErrorRate() << " oracle_crossvalidate=" << cvdec.OracleTokenErrorRate()
                << " scored=" << (int)bs.num_scored << " cv_scored=" << (int)cvdec.NumUtterances() << " skipped=" << bs.num_skipped
                << " beam0_same=" << (int)(greedy0 == greedy && g0.num_errors == g.num_errors && calls == g.num_minibatches)
                << " best1_same=" << (int)(best1 == best && b1.num_errors == bs.num_errors) << " lists_ok=" << (int)lists_ok
                << " oracle_errors=" << oracle << " ref_tokens=" << (int)bs.num_ref_tokens << " errors_beam=" << (int)bs.num_errors << "\n";
    } else {
      std::cerr << "usage: ctc_beam_test train <blstm|lstm> <dump>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
