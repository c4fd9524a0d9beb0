// tests/cpp/rnnt_band_test.cpp -- drives Transducer::BandFromFrames / EvalBanded and the band option of TrainTransducerWholeUtterances
// (include/klstm_nnet.hpp) for tests/test_rnnt_band_gpu.py.
// `eval`: T = 21, Umax = 6, V = 7, J = 32, S = 2, R = 4; enc, pred, W, b in that order from the generator x <- 1664525 x + 1013904223
// (mod 2^32, from 12345), value ((x >> 8) & 0xffff) / 65536 - 0.5, which the test repeats.  Prints
//   OK <the two losses as bit patterns> <the sums of the bit patterns of d_enc, d_pred, W_grad, b_grad>
// `train`: the networks and utterances of rnnt_test.cpp.  Two passes with band = 4 (the second utterance with label frames, the others
// along the straight line), then on fresh copies two passes with band = 0 whose every minibatch is evaluated again by krnnt_eval called
// directly on the same activations.  Prints
//   OK <band 0 bit-identical 0/1> | the average loss of the two banded passes
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
static unsigned long long bit_sum(const std::vector<float> &v) {
  unsigned long long sum = 0;
  for (float x : v) { uint32_t u; std::memcpy(&u, &x, 4); sum += u; }
  return sum;
}

static int eval_mode() {
  const int32 T = 21, Umax = 6, V = 7, J = 32, S = 2, R = 4;
  uint32_t x = 12345;
  auto gen = [&](size_t n) {
    std::vector<BaseFloat> v(n);
    for (auto &e : v) { x = x * 1664525u + 1013904223u; e = (BaseFloat)((x >> 8) & 0xffff) / 65536.f - 0.5f; }
    return v;
  };
  DeviceMatrix enc, pred, d_enc, d_pred;
  const std::vector<BaseFloat> eh = gen((size_t)T * S * J), ph = gen((size_t)(Umax + 1) * S * J), w = gen((size_t)V * J), b = gen(V);
  enc.CopyFromHost(eh.data(), T * S, J);
  pred.CopyFromHost(ph.data(), (Umax + 1) * S, J);
  TransducerJoint joint(J, V);
  joint.SetParams(w, b);
  const std::vector<int32> lens = {T, T - 4};
  const std::vector<std::vector<int32> > labels = {{1, 2, 2, 3, 4, 6}, {5, 1, 3}}, frames = {{1, 4, 5, 9, 14, 18}, {0, 7, 11}};
  Transducer tr(0);
  const int32 *band = tr.BandFromFrames(T, S, lens, labels, &frames, R);
  tr.EvalBanded(enc, pred, S, lens, labels, band, R, &joint, &d_enc, &d_pred);
  std::vector<BaseFloat> loss, de, dp;
  tr.UttLoss(&loss);
  d_enc.CopyToHost(&de);
  d_pred.CopyToHost(&dp);
  std::printf("OK");
  for (float v : loss) { uint32_t u; std::memcpy(&u, &v, 4); std::printf(" %u", u); }
  std::printf(" %llu %llu %llu %llu\n", bit_sum(de), bit_sum(dp), bit_sum(down((const float *)joint.WGrad(), (size_t)V * J)),
              bit_sum(down((const float *)joint.bGrad(), V)));
  return 0;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval") return eval_mode();
    if (mode != "train") KLSTM_ERR("usage: rnnt_band_test eval | train");
    const int32 V = 5, J = 16, S = 2;
    const int32 frames[4] = {12, 9, 7, 6}, nlab[4] = {4, 2, 3, 1};
    std::vector<double> avg;
    bool identical = true;
    for (int band = 4; band >= 0; band -= 4) {
      std::srand(7);
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
      std::vector<Utterance> utts(4);
      for (int i = 0; i < 4; i++) {
        utts[i].num_frames = frames[i]; utts[i].dim = 8;
        for (int k = 0; k < frames[i] * 8; k++) utts[i].feats.push_back((BaseFloat)((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 2.f);
        for (int k = 0; k < nlab[i]; k++) utts[i].labels.push_back(1 + std::rand() % (V - 1));
      }
      const std::vector<std::vector<int32> > label_frames = {{}, {2, 6}};
      TrainTransducerOptions o;
      o.num_stream = S; o.blank = 0; o.band = band; o.label_frames = &label_frames;
      o.trn_opts.learn_rate = 0.01f; o.trn_opts.momentum = 0.5f;
      for (int ep = 0; ep < 2; ep++) {
        TrainTransducerStats st = TrainTransducerWholeUtterances(&enc, &pred, &joint, utts, o, nullptr,
            [&](const UtteranceBatch &bt, const DeviceMatrix &eo, const DeviceMatrix &po, const Transducer &tr) {
              if (band != 0) return;
              std::vector<BaseFloat> loss;
              tr.UttLoss(&loss);
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
              identical = identical && std::memcmp(a.data(), loss.data(), S * 4) == 0 && std::memcmp(g1.data(), g2.data(), V * J * 4) == 0;
            });
        if (st.num_done != 4 || st.num_rejected != 0 || !std::isfinite(st.avg_loss)) KLSTM_ERR("pass " << ep << " with band " << band << " did not finish");
        if (band != 0) avg.push_back(st.avg_loss);
      }
    }
    std::printf("OK %d |", (int)identical);
    for (double v : avg) std::printf(" %.9g", v);
    std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
