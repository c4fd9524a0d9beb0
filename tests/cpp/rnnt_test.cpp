// tests/cpp/rnnt_test.cpp -- drives TransducerJoint, Transducer and TrainTransducerWholeUtterances (include/klstm_nnet.hpp) for
// tests/test_rnnt_gpu.py.  `train <epochs>`: encoder <LstmProjectedStreams> 8 -> 16 / 8 + <AffineTransform> to J = 16; predictor
// <AffineTransform> 5 -> 8 (the embedding of the one-hot rows) + <LstmProjectedStreams> 8 -> 16 / 8 + <AffineTransform> to 16; V = 5; four
// utterances of 6 .. 12 frames with 1 .. 4 labels, two streams: two minibatches per epoch, from a fixed seed.  The first minibatch of the
// first epoch is evaluated again by krnnt_eval called directly on the same activations.  Prints
//   OK <bit-identical 0/1> <all finite 0/1> <minibatches> | the average loss of every epoch
// `io` (host only): the joint written and read back in text and in binary; prints OK <1 when both round trips keep every bit>.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

static LstmProjectedStreams *new_lstm(int32 in, int32 cell, int32 out, int32 streams) {
  std::unique_ptr<LstmProjectedStreams> c(new LstmProjectedStreams(in, out));
  std::ostringstream cfg;
  cfg << "<CellDim> " << cell << " <NumStream> " << streams << " <ParamScale> 0.3";
  std::istringstream is(cfg.str());
  c->InitData(is);
  return c.release();
}
static void random_params(int32 in, int32 out, double scale, std::vector<BaseFloat> *w, std::vector<BaseFloat> *b) {
  w->resize((size_t)out * in); b->assign(out, 0.f);
  for (auto &v : *w) v = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * scale);
}
static AffineLayer *new_affine(int32 in, int32 out, double scale) {
  AffineLayer *aff = new AffineLayer(in, out);
  std::vector<BaseFloat> w, b;
  random_params(in, out, scale, &w, &b);
  aff->SetParams(w, b);
  return aff;
}
template <class T>
static std::vector<T> down(const T *dev, size_t n) {
  std::vector<T> v(n);
  KCheck(klstm_memcpy_d2h(v.data(), dev, n * sizeof(T), nullptr));
  return v;
}

int main(int argc, char **argv) {
  try {
    const int32 V = 5, J = 16, S = 2;
    std::srand(7);
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "io") {
      TransducerJoint joint(J, V);
      std::vector<BaseFloat> w, b, w2, b2;
      random_params(J, V, 1.0, &w, &b);
      for (auto &v : b) v = (BaseFloat)(std::rand() % 1000) / 3000.f;
      joint.SetParams(w, b);
      bool same = true;
      for (int binary = 0; binary < 2; binary++) {
        std::stringstream ss;
        joint.Write(ss, binary != 0);
        TransducerJoint back(1, 1);
        back.Read(ss, binary != 0);
        back.HostParams(&w2, &b2);
        same = same && back.JointDim() == J && back.NumClasses() == V && w2.size() == w.size() && b2.size() == b.size() &&
               std::memcmp(w.data(), w2.data(), w.size() * 4) == 0 && std::memcmp(b.data(), b2.data(), b.size() * 4) == 0;
      }
      std::printf("OK %d\n", (int)same);
      return 0;
    }
    if (mode != "train" || argc < 3) KLSTM_ERR("usage: rnnt_test train <epochs> | io");
    const int epochs = std::atoi(argv[2]);
    Nnet enc, pred;
    enc.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, S)));
    enc.AppendComponent(new_affine(8, J, 1.0));
    pred.AppendComponent(new_affine(V, 8, 1.0));
    pred.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, S)));
    pred.AppendComponent(new_affine(8, J, 1.0));
    TransducerJoint joint(J, V);
    std::vector<BaseFloat> w, b;
    random_params(J, V, 0.6, &w, &b);
    joint.SetParams(w, b);
    const int32 frames[4] = {12, 9, 7, 6}, nlab[4] = {4, 2, 3, 1};
    std::vector<Utterance> utts(4);
    for (int i = 0; i < 4; i++) {
      utts[i].num_frames = frames[i]; utts[i].dim = 8;
      for (int k = 0; k < frames[i] * 8; k++) utts[i].feats.push_back((BaseFloat)((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 2.f);
      for (int k = 0; k < nlab[i]; k++) utts[i].labels.push_back(1 + std::rand() % (V - 1));
    }
    TrainTransducerOptions o;
    o.num_stream = S; o.blank = 0;
    o.trn_opts.learn_rate = 0.01f; o.trn_opts.momentum = 0.5f;
    bool identical = false, finite = true;
    int minibatches = 0;
    std::vector<double> avg;
    for (int ep = 0; ep < epochs; ep++) {
      TrainTransducerStats st = TrainTransducerWholeUtterances(&enc, &pred, &joint, utts, o, nullptr,
          [&](const UtteranceBatch &bt, const DeviceMatrix &eo, const DeviceMatrix &po, const Transducer &tr) {
            std::vector<BaseFloat> loss;
            tr.UttLoss(&loss);
            for (BaseFloat v : loss) finite = finite && std::isfinite(v);
            if (minibatches++ != 0) return;
            // the same activations through krnnt_eval directly
            PackedLabels lab;
            lab.Upload(bt.labels);
            const int32 T = bt.num_frames, Umax = (int32)lab.longest;
            DeviceBuffer lens, ws, l2, de, dp, wg, bg;
            lens.Upload(bt.lens);
            const size_t need = krnnt_workspace_bytes(T, S, Umax, J, V);
            ws.Grow(need); l2.Grow(S * 4); de.Grow((size_t)T * S * J * 4); dp.Grow((size_t)(Umax + 1) * S * J * 4); wg.Grow(V * J * 4); bg.Grow(V * 4);
            MatrixView e = eo.View(), p = po.View();
            KCheck(krnnt_eval(e.Data(), e.Stride(), p.Data(), p.Stride(), joint.W(), joint.b(), T, S, Umax, J, V, lens.As<int32>(), lab.Labels(),
                              lab.Offsets(), 0, de.As<float>(), J, dp.As<float>(), J, wg.As<float>(), bg.As<float>(), l2.As<float>(), nullptr,
                              ws.As<void>(), need, nullptr));
            const std::vector<float> a = down(l2.As<float>(), S), g1 = down(wg.As<float>(), V * J), g2 = down((const float *)joint.WGrad(), V * J);
            identical = std::memcmp(a.data(), loss.data(), S * 4) == 0 && std::memcmp(g1.data(), g2.data(), V * J * 4) == 0;
          });
      finite = finite && std::isfinite(st.avg_loss) && st.num_done == 4 && st.num_rejected == 0;
      avg.push_back(st.avg_loss);
    }
    std::printf("OK %d %d %d |", (int)identical, (int)finite, minibatches);
    for (double v : avg) std::printf(" %.9g", v);
    std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
