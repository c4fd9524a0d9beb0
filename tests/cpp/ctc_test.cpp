// tests/cpp/ctc_test.cpp -- drives WholeUtteranceBatcher (include/klstm_trainer.hpp; host only) and Ctc / TrainCtcWholeUtterances
// (include/klstm_nnet.hpp; GPU) for tests/test_ctc.py and tests/test_ctc_gpu.py.
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

// utterance i of the batcher check: dim 3, feats(t, d) = 1000 i + t + d / 4, labels i, i + 1, ... (i % 5 of them)
static Utterance plain_utt(int32 i, int32 frames) {
  Utterance u;
  u.num_frames = frames; u.dim = 3;
  u.feats.resize((size_t)frames * 3);
  for (int32 t = 0; t < frames; t++) for (int32 d = 0; d < 3; d++) u.feats[(size_t)t * 3 + d] = 1000.f * i + t + 0.25f * d;
  for (int32 j = 0; j < i % 5; j++) u.labels.push_back(i + j);
  return u;
}

// utterances of the training check: `classes` - 1 labels, each a run of 3..6 frames whose features are a noisy one-hot pattern of the
// label (dim 16) -- the label sequence is a deterministic function of the features
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
    if (mode == "batcher" && argc == 7) {
      // batcher <streams> <sort 0/1> <max_frames> <len,len,...> <out>     host only.  Writes per minibatch: T, lens[S], utt_index[S],
      // per stream (L, labels), then feat [T*S x 3]; prints "OK <minibatches> <done> <skipped>"
      const int32 S = atoi(argv[2]);
      std::vector<Utterance> utts;
      const std::vector<int32> lens = parse_ints(argv[5]);
      for (size_t i = 0; i < lens.size(); i++) utts.push_back(plain_utt((int32)i, lens[i]));
      WholeUtteranceBatcher batcher(&utts, S, atoi(argv[3]) != 0, atoi(argv[4]));
      std::ofstream f(argv[6], std::ios::binary);
      UtteranceBatch b;
      int32 n = 0;
      while (batcher.Next(&b)) {
        KLSTM_ASSERT(b.num_stream == S && b.dim == 3 && b.feat.size() == (size_t)b.num_frames * S * 3);
        put(f, b.num_frames); put(f, b.lens); put(f, b.utt_index);
        for (int32 s = 0; s < S; s++) { put(f, (int32)b.labels[s].size()); put(f, b.labels[s]); }
        put(f, b.feat);
        n++;
      }
      std::cout << "OK " << n << " " << batcher.NumDone() << " " << batcher.NumSkipped() << "\n";
    } else if (mode == "train" && argc == 4) {
      // train <blstm|lstm> <dump>      GPU.  Transmit - (BLstm 16/32/16 | two LstmProjectedStreams 16/32/16) - Affine - Softmax, 4 streams,
      // a dozen pattern utterances, 10 epochs of TrainCtcWholeUtterances.  blstm: the first minibatch of the last epoch is dumped
      // (T, S, K, labels; lens, offsets, labels, posteriors, diff, losses).  lstm: one utterance too short for its labels and one
      // beyond max_frames are planted.
      const bool bi = std::string(argv[2]) == "blstm";
      const int32 S = 4, K = 6, epochs = 10;
      std::srand(7);
      std::vector<Utterance> utts;
      for (int32 i = 0; i < 12; i++) utts.push_back(pattern_utt(100 + i, 4 + i % 7, K));
      int32 planted_rejected = 0, planted_skipped = 0;
      TrainCtcOptions o;
      o.num_stream = S;
      o.trn_opts.learn_rate = 0.002f;
      o.trn_opts.momentum = 0.f;
      if (!bi) {
        Utterance shorty = pattern_utt(55, 1, K);            // 3..6 frames, then nine labels: cannot be aligned
        shorty.labels.assign(9, 2);
        utts.push_back(shorty); planted_rejected = 1;
        utts.push_back(pattern_utt(56, 40, K));               // >= 120 frames
        o.max_frames = 100; planted_skipped = 1;
      }
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
      double first = 0, last = 0, rejected = 0;
      int32 skipped = 0;
      for (int32 e = 0; e < epochs; e++) {
        int32 mb = 0;
        const bool dump = bi && e == epochs - 1;
        const TrainCtcStats st = TrainCtcWholeUtterances(&nnet, utts, o, nullptr,
            [&](const UtteranceBatch &b, const DeviceMatrix &y, const DeviceMatrix &d, const Ctc &ctc) {
              if (!dump || mb++ != 0) return;
              std::vector<BaseFloat> post, diff, loss;
              y.CopyToHost(&post); d.CopyToHost(&diff); ctc.UttLoss(&loss);
              std::vector<int32> off(1, 0), flat;
              for (const auto &l : b.labels) { flat.insert(flat.end(), l.begin(), l.end()); off.push_back((int32)flat.size()); }
              std::ofstream f(argv[3], std::ios::binary);
              put(f, b.num_frames); put(f, b.num_stream); put(f, K); put(f, (int32)flat.size());
              put(f, b.lens); put(f, off); put(f, flat); put(f, post); put(f, diff); put(f, loss);
            });
        if (e == 0) first = st.avg_loss_per_frame;
        last = st.avg_loss_per_frame; rejected = st.num_rejected; skipped = st.num_skipped;
        std::cerr << "epoch " << e << " loss/frame " << st.avg_loss_per_frame << " loss/utt " << st.avg_loss << " frames " << st.total_frames
                  << " minibatches " << st.num_minibatches << "\n";
      }
      std::cout << "OK first_epoch_loss_per_frame=" << first << " last_epoch_loss_per_frame=" << last << " rejected=" << (int)rejected
                << " planted_rejected=" << planted_rejected << " skipped=" << skipped << " planted_skipped=" << planted_skipped << "\n";
    } else {
      std::cerr << "usage: ctc_test batcher <streams> <sort> <max_frames> <lens> <out> | train <blstm|lstm> <dump>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
