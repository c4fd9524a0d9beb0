// tests/cpp/ctc_mmi_test.cpp -- drives CtcMmi / TrainMmiWholeUtterances (include/klstm_nnet.hpp) for tests/test_ctc_mmi_gpu.py: train the
// pattern task with CTC for a few epochs, then MMI against a bigram estimated from the training labels.
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


// the bigram of lm.py's ngram_label_lm(order 2) without smoothing: state 0 the start, state 1 + c after label c; what the training
// labels never did is forbidden (weight 0)
struct Bigram { int32 Q, K; std::vector<int32> next; std::vector<BaseFloat> weight, fin; };
static Bigram estimate_bigram(const std::vector<Utterance> &utts, int32 K, int32 max_frames) {
  Bigram g;
  g.Q = K + 1; g.K = K;
  std::vector<double> cnt((size_t)g.Q * K, 0.0), end(g.Q, 0.0);
  for (const Utterance &u : utts) {
    if (u.num_frames > max_frames) continue;
    int32 q = 0;
    for (int32 c : u.labels) { cnt[(size_t)q * K + c] += 1; q = 1 + c; }
    end[q] += 1;
  }
  g.next.assign((size_t)g.Q * K, 0); g.weight.assign((size_t)g.Q * K, 0.f); g.fin.assign(g.Q, 0.f);
  for (int32 q = 0; q < g.Q; q++) {
    double den = end[q];
    for (int32 c = 0; c < K; c++) den += cnt[(size_t)q * K + c];
    for (int32 c = 1; c < K; c++) {
      g.next[(size_t)q * K + c] = 1 + c;
      if (den > 0) g.weight[(size_t)q * K + c] = (BaseFloat)(cnt[(size_t)q * K + c] / den);
    }
    if (den > 0) g.fin[q] = (BaseFloat)(end[q] / den);
  }
  return g;
}
static bool accepts(const Bigram &g, const std::vector<int32> &labels) {
  int32 q = 0;
  for (int32 c : labels) { if (!(g.weight[(size_t)q * g.K + c] > 0.f)) return false; q = g.next[(size_t)q * g.K + c]; }
  return g.fin[q] > 0.f;
}

static TrainMmiStats crossvalidate(Nnet *nnet, const std::vector<Utterance> &utts, TrainMmiOptions o, const char *dump, const Bigram &g) {
  o.crossvalidate = true;
  int32 mb = 0;
  return TrainMmiWholeUtterances(nnet, utts, o, nullptr,
      [&](const UtteranceBatch &b, const DeviceMatrix &y, const DeviceMatrix &diff, const CtcMmi &mmi) {
        if (mb++ != 1 || !dump) return;          // the SECOND minibatch: the objects have been through another shape by then
        const int32 T = b.num_frames, S = b.num_stream;
        std::vector<BaseFloat> post, d, loss;
        y.CopyToHost(&post);
        diff.CopyToHost(&d);
        mmi.UttLoss(&loss);
        std::vector<int32> off(1, 0), flat;
        for (int32 s = 0; s < S; s++) { flat.insert(flat.end(), b.labels[s].begin(), b.labels[s].end()); off.push_back((int32)flat.size()); }
        std::ofstream f(dump, std::ios::binary);
        put(f, T); put(f, S); put(f, g.K); put(f, g.Q); put(f, (int32)flat.size());
        put(f, b.lens); put(f, off); put(f, flat); put(f, g.next); put(f, g.weight); put(f, g.fin);
        put(f, post); put(f, d); put(f, loss);
      });
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "train" && argc == 6) {
      // train <blstm|lstm> <dump> <ctc epochs> <mmi learning rate>      GPU.  The nets and the CTC schedule of ctc_mbr_test's train mode; a
      // bigram estimated from the training labels without smoothing; a cross-validation pass of TrainMmiWholeUtterances (CTC weight
      // 0.1) over the training utterances and ONE more whose labels the bigram does not accept, whose second minibatch is dumped;
      // three epochs of MMI on the training utterances; the cross-validation pass again.
      const bool bi = std::string(argv[2]) == "blstm";
      const int32 S = 4, K = 6, ctc_epochs = std::atoi(argv[4]);
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


      const Bigram g = estimate_bigram(utts, K, o.max_frames);
      const CtcLabelLm lm(g.Q, g.K, g.next, g.weight, g.fin);
      std::vector<Utterance> cv = utts;
      for (const Utterance &u : utts) if (u.num_frames <= o.max_frames && !accepts(g, u.labels)) KLSTM_ERR("a training utterance is not accepted");
      bool found = false;
      for (unsigned seed = 1000; seed < 2000 && !found; seed++) {
        const Utterance u = pattern_utt(seed, 6, K);
        if (!accepts(g, u.labels)) { cv.push_back(u); found = true; }
      }
      if (!found) KLSTM_ERR("no utterance that the bigram rejects");

      TrainMmiOptions m;
      m.num_stream = S;
      m.max_frames = o.max_frames;
      m.trn_opts = o.trn_opts;
      m.trn_opts.learn_rate = (float)std::atof(argv[5]);
      m.ctc_weight = 0.1f;
      m.lm = &lm;
      const int32 mmi_epochs = 3;
      const TrainMmiStats before = crossvalidate(&nnet, cv, m, argv[3], g);
      std::vector<double> epoch_loss;
      std::string report;
      for (int32 e = 0; e < mmi_epochs; e++) epoch_loss.push_back(TrainMmiWholeUtterances(&nnet, utts, m, &report).avg_loss);
      const TrainMmiStats after = crossvalidate(&nnet, cv, m, nullptr, g);
      std::cerr << report << "\n";
      std::cout << "OK ctc_epochs=" << ctc_epochs << " mmi_epochs=" << mmi_epochs << " mmi_learn_rate=" << m.trn_opts.learn_rate
                << " loss_before=" << before.avg_loss << " loss_epoch0=" << epoch_loss[0] << " loss_epoch1=" << epoch_loss[1]
                << " loss_epoch2=" << epoch_loss[2] << " loss_after=" << after.avg_loss << " loss_per_frame_after=" << after.avg_loss_per_frame
                << " ref_loss_before=" << before.avg_ref_loss << " ref_loss_after=" << after.avg_ref_loss << " done=" << after.num_done
                << " skipped=" << after.num_skipped << " rejected=" << (int)after.num_rejected << " frames=" << (long)after.total_frames
                << " minibatches=" << after.num_minibatches << "\n";
    } else {
      std::cerr << "usage: ctc_mmi_test train <blstm|lstm> <dump> <ctc epochs> <mmi learning rate>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
