// tests/cpp/ctc_mbr_test.cpp -- drives CtcMbr / TrainMbrWholeUtterances (include/klstm_nnet.hpp) for tests/test_ctc_mbr_gpu.py: train the
// pattern task with CTC for a few epochs only, then minimise the expected token errors over the model's own n-best lists.
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


static TrainMbrStats crossvalidate(Nnet *nnet, const std::vector<Utterance> &utts, TrainMbrOptions o, const char *dump, int32 K) {
  o.crossvalidate = true;
  int32 mb = 0;
  return TrainMbrWholeUtterances(nnet, utts, o, nullptr,
      [&](const UtteranceBatch &b, const DeviceMatrix &y, const DeviceMatrix &diff, const CtcBeamDecoder &dec, const CtcMbr &mbr) {
        if (mb++ != 1 || !dump) return;          // the SECOND minibatch: the objects have been through another shape by then
        const int32 T = b.num_frames, S = b.num_stream, N = o.nbest;
        std::vector<BaseFloat> post, d, risk, logp;
        y.CopyToHost(&post);
        diff.CopyToHost(&d);
        mbr.UttRisk(&risk);
        mbr.HypLogp(&logp);
        std::vector<CtcNbestList> lists;
        CtcBeamDecoder again(o.blank, o.beam, o.cands, o.nbest);
        again.Decode(y, S, b.lens, b.labels, &lists);
        std::vector<int32> cnt, hlen((size_t)S * N, 0), err((size_t)S * N, -1), hyp((size_t)S * N * T, -1), off(1, 0), flat;
        for (int32 s = 0; s < S; s++) {
          cnt.push_back((int32)lists[s].size());
          for (size_t q = 0; q < lists[s].size(); q++) {
            hlen[(size_t)s * N + q] = (int32)lists[s][q].tokens.size();
            err[(size_t)s * N + q] = lists[s][q].errors;
            std::copy(lists[s][q].tokens.begin(), lists[s][q].tokens.end(), hyp.begin() + ((size_t)s * N + q) * T);
          }
          flat.insert(flat.end(), b.labels[s].begin(), b.labels[s].end());
          off.push_back((int32)flat.size());
        }
        std::ofstream f(dump, std::ios::binary);
        put(f, T); put(f, S); put(f, K); put(f, N); put(f, (int32)flat.size());
        put(f, b.lens); put(f, off); put(f, flat); put(f, cnt); put(f, hlen); put(f, err); put(f, hyp);
        put(f, post); put(f, d); put(f, risk); put(f, logp);
      });
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "train" && argc == 6) {
      // train <blstm|lstm> <dump> <ctc epochs> <mbr learning rate>      GPU.  The nets of ctc_beam_test's train mode, trained with CTC
      // for <ctc epochs> only; a cross-validation pass of TrainMbrWholeUtterances (beam 8, 5 candidates, 4-best, risk scale 1, CTC
      // weight 0.1), whose second minibatch is dumped; three epochs of it; the cross-validation pass again.
      const bool bi = std::string(argv[2]) == "blstm";
      const int32 S = 4, K = 6, ctc_epochs = std::atoi(argv[4]), mbr_epochs = 3;
      const float mbr_lr = (float)std::atof(argv[5]);
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
      for (int32 e = 0; e < ctc_epochs; e++) TrainCtcWholeUtterances(&nnet, utts, o);

      TrainMbrOptions m;
      m.num_stream = S;
      m.max_frames = o.max_frames;
      m.trn_opts = o.trn_opts;
      m.trn_opts.learn_rate = mbr_lr;
      m.beam = 8; m.cands = 5; m.nbest = 4;
      m.risk_scale = 1.f; m.ctc_weight = 0.1f;
      const TrainMbrStats before = crossvalidate(&nnet, utts, m, argv[3], K);
      std::vector<double> epoch_risk;
      std::string report;
      for (int32 e = 0; e < mbr_epochs; e++) epoch_risk.push_back(TrainMbrWholeUtterances(&nnet, utts, m, &report).avg_risk);
      const TrainMbrStats after = crossvalidate(&nnet, utts, m, nullptr, K);
      std::cerr << report << "\n";
      std::cout << "OK ctc_epochs=" << ctc_epochs << " mbr_epochs=" << mbr_epochs << " mbr_learn_rate=" << mbr_lr << " risk_before=" << before.avg_risk
                << " ter_before=" << before.token_error_rate << " risk_epoch0=" << epoch_risk[0] << " risk_epoch1=" << epoch_risk[1]
                << " risk_epoch2=" << epoch_risk[2] << " risk_after=" << after.avg_risk << " ter_after=" << after.token_error_rate
                << " ref_loss_before=" << before.avg_loss << " ref_loss_after=" << after.avg_loss << " done=" << after.num_done
                << " skipped=" << after.num_skipped << " rejected_or_skipped=" << (int)after.num_rejected << " minibatches=" << after.num_minibatches
                << "\n";
    } else {
      std::cerr << "usage: ctc_mbr_test train <blstm|lstm> <dump> <ctc epochs> <mbr learning rate>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
