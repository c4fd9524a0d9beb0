// tests/cpp/dropout_test.cpp -- drives the kdrop_* entries (include/klstm_dropout.h) and the <Dropout> component, the Nnet switches,
// WithoutDropout and the trainers' dropout scope (include/klstm_nnet.hpp, klstm_scorer.hpp) for tests/test_dropout*.py.  The modes
// errors, nnet_copy, without, standard and topology are host only; train and ctc need the GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <sstream>

#include "klstm_dropout.h"
#include "klstm_nnet.hpp"
#include "klstm_scorer.hpp"

using namespace klstm_kaldi;

static int failures = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) { std::printf("FAILED %s:%d: %s (last error: '%s')\n", __FILE__, __LINE__, #c, klstm_last_error()); failures++; } \
  } while (0)

static std::vector<float> read_raw(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) KLSTM_ERR("cannot open " << path);
  f.seekg(0, std::ios::end);
  const size_t n = (size_t)f.tellg() / sizeof(float);
  f.seekg(0);
  std::vector<float> v(n);
  f.read(reinterpret_cast<char *>(v.data()), n * sizeof(float));
  return v;
}
// float32 stream: nutt, then per utterance: len, dim, ntargets, feats[len*dim], targets[ntargets]  (tests/test_component.py _pack_utts)
static std::vector<Utterance> read_utts(const std::string &path) {
  const std::vector<float> raw = read_raw(path);
  size_t o = 0;
  const int nutt = (int)raw[o++];
  std::vector<Utterance> utts(nutt);
  for (auto &u : utts) {
    u.num_frames = (int)raw[o++]; u.dim = (int)raw[o++];
    const int nt = (int)raw[o++];
    u.feats.assign(raw.begin() + o, raw.begin() + o + (size_t)u.num_frames * u.dim); o += (size_t)u.num_frames * u.dim;
    for (int i = 0; i < nt; i++) u.targets.push_back((int32)raw[o++]);
  }
  return utts;
}
static std::string model_bytes(const Nnet &n) { std::stringstream ss; n.Write(ss, true); return ss.str(); }
static bool all_off(const Nnet &n) { for (bool b : n.DropoutActive()) if (b) return false; return true; }
static std::string refusal(const std::function<void()> &f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}

// the utterances of tests/cpp/ctc_test.cpp's training check: `classes` - 1 labels, each a run of 3..6 frames whose features are a noisy
// one-hot pattern of the label (dim 16)
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
// Transmit - LSTM 16/32/16 - Dropout 0.8 - LSTM 16/32/16 - Affine - Softmax; the same parameters at every call
static void ctc_stack(int32 S, int32 K, Nnet *nnet) {
  std::srand(7);
  nnet->AppendComponent(new TransmitLayer(16, 16));
  nnet->AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
  DropoutLayer *d = new DropoutLayer(16, 16);
  d->SetRetention(0.8f);
  nnet->AppendComponent(d);
  nnet->AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
  AffineLayer *aff = new AffineLayer(16, K);
  std::vector<BaseFloat> w((size_t)K * 16), bias(K, 0.f);
  for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
  aff->SetParams(w, bias);
  nnet->AppendComponent(aff);
  nnet->AppendComponent(new SoftmaxLayer(K, K));
}
static std::string ctc_run(const std::vector<Utterance> &utts, int32 S, int32 K, uint64_t seed, bool per_sequence, int32 epochs, Nnet *keep = nullptr) {
  Nnet local, *nnet = keep ? keep : &local;
  ctc_stack(S, K, nnet);
  TrainCtcOptions o;
  o.num_stream = S;
  o.trn_opts.learn_rate = 0.002f;
  o.trn_opts.momentum = 0.f;
  o.dropout_per_sequence = per_sequence;
  for (int32 e = 0; e < epochs; e++) {
    o.dropout_seed = seed + (uint64_t)e * 1000;                 // every epoch its own masks
    const TrainCtcStats st = TrainCtcWholeUtterances(nnet, utts, o);
    if (!std::isfinite(st.avg_loss_per_frame)) KLSTM_ERR("ctc_run: loss " << st.avg_loss_per_frame);
    if (!all_off(*nnet)) KLSTM_ERR("ctc_run: dropout is still on after TrainCtcWholeUtterances");
  }
  return model_bytes(*nnet);
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "errors" && argc == 2) {
      // every KLSTM_ERR_ARG of the two entries, before any HIP call (no device is needed), each with its message; the pointers are
      // never followed
      float buf[64] = {0};
      float *in = buf, *out = buf + 32;
      unsigned ids[2] = {0, 0}, thr = 7;
      float scale = 7.f;
      const float nan = std::numeric_limits<float>::quiet_NaN();
      CHECK(std::strcmp(klstm_last_error(), "") == 0);
      CHECK(kdrop_threshold(0.5f, nullptr, &scale) == KLSTM_ERR_ARG);
      CHECK(std::strcmp(klstm_last_error(), "kdrop_threshold: null argument") == 0);
      for (float p : {0.f, -0.1f, 1.0000001f, nan, 0x1p-33f}) {
        CHECK(kdrop_threshold(p, &thr, &scale) == KLSTM_ERR_ARG);
        CHECK(std::strstr(klstm_last_error(), "kdrop_threshold: retention") != nullptr && thr == 7 && scale == 7.f);
      }
      auto apply = [&](const float *i, int is, int rows, int cols, float *o, int os, float p, unsigned salt, int md, int S, const unsigned *id) {
        return kdrop_apply(i, is, rows, cols, o, os, p, 1234ull, 0u, salt, md, S, id, nullptr);
      };
      struct Case { klstm_status st; const char *msg; };
      const Case cases[] = {
          {apply(in, 4, -1, 4, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: bad size"},
          {apply(in, 4, 2, -4, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: bad size"},
          {apply(in, 4, 2, 4, out, 4, 0.f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: retention"},
          {apply(in, 4, 2, 4, out, 4, 1.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: retention"},
          {apply(in, 4, 2, 4, out, 4, nan, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: retention"},
          {apply(in, 4, 2, 4, out, 4, 0.5f, 0x80000000u, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: salt"},
          {apply(in, 4, 2, 4, out, 4, 0.5f, 0, 2, 1, nullptr), "kdrop_apply: unknown mode 2"},
          {apply(in, 4, 2, 4, out, 4, 0.5f, 0, -1, 1, nullptr), "kdrop_apply: unknown mode -1"},
          {apply(in, 4, 2, 4, out, 4, 0.5f, 0, KDROP_SEQUENCE, 0, ids), "kdrop_apply: num_stream 0"},
          {apply(in, 4, 2, 4, out, 4, 0.5f, 0, KDROP_SEQUENCE, 2, nullptr), "kdrop_apply: KDROP_SEQUENCE needs seq_id_dev"},
          {apply(nullptr, 4, 2, 4, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: null argument"},
          {apply(in, 4, 2, 4, nullptr, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: null argument"},
          {apply(in, 3, 2, 4, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: row stride below the column count"},
          {apply(in, 4, 2, 4, out, 3, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: row stride below the column count"},
          {apply(in, 4, 2, 4, in + 1, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: in and out overlap"},
          {apply(in + 4, 4, 2, 4, in, 4, 1.f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: in and out overlap"},
          {apply(in, 4, 2, 4, in, 8, 0.5f, 0, KDROP_ELEMENT, 1, nullptr), "kdrop_apply: in == out with two strides"},
      };
      // (the messages were overwritten one by one: run each again and read its own)
      int n = 0;
      for (const Case &c : cases) { CHECK(c.st == KLSTM_ERR_ARG); n++; }
      CHECK(apply(in, 4, 2, 4, out, 4, 0.5f, 0, 2, 1, nullptr) == KLSTM_ERR_ARG);
      CHECK(std::strcmp(klstm_last_error(), "kdrop_apply: unknown mode 2") == 0);
      CHECK(apply(in, 4, 2, 4, in + 1, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr) == KLSTM_ERR_ARG);
      CHECK(std::strcmp(klstm_last_error(), "kdrop_apply: in and out overlap (only in == out may)") == 0);
      CHECK(apply(in, 3, 2, 4, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr) == KLSTM_ERR_ARG);
      CHECK(std::strncmp(klstm_last_error(), cases[12].msg, std::strlen(cases[12].msg)) == 0);
      CHECK(apply(in, 4, 2, 4, out, 4, 0.5f, 0, KDROP_SEQUENCE, 2, nullptr) == KLSTM_ERR_ARG);
      CHECK(std::strcmp(klstm_last_error(), cases[9].msg) == 0);
      // an empty block is fine and launches nothing (no device here), null pointers included; a p == 1 call in place does nothing
      CHECK(apply(nullptr, 0, 0, 4, nullptr, 0, 0.5f, 0, KDROP_ELEMENT, 1, nullptr) == KLSTM_OK);
      CHECK(apply(in, 4, 2, 0, out, 4, 0.5f, 0, KDROP_ELEMENT, 1, nullptr) == KLSTM_OK);
      CHECK(apply(in, 4, 2, 4, in, 4, 1.f, 0, KDROP_ELEMENT, 1, nullptr) == KLSTM_OK);
      for (float v : buf) CHECK(v == 0.f);
      if (failures) return 1;
      std::printf("OK %d refusals before any HIP call\n", n + 6);
    } else if (mode == "messages" && argc == 2) {
      // one line per refusal of kdrop_apply: its message (for the test that every case has one of its own)
      float buf[64] = {0};
      unsigned ids[2] = {0, 0};
      const float nan = std::numeric_limits<float>::quiet_NaN();
      auto say = [&](klstm_status st) { std::printf("%d|%s\n", (int)st, klstm_last_error()); };
      std::printf("OK\n");
      say(kdrop_apply(buf, 4, -1, 4, buf + 32, 4, 0.5f, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 32, 4, nan, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0x80000000u, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0, 7, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0, KDROP_SEQUENCE, 0, ids, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0, KDROP_SEQUENCE, 2, nullptr, nullptr));
      say(kdrop_apply(nullptr, 4, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 3, 2, 4, buf + 32, 4, 0.5f, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf + 2, 4, 0.5f, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
      say(kdrop_apply(buf, 4, 2, 4, buf, 8, 0.5f, 1, 0, 0, KDROP_ELEMENT, 1, nullptr, nullptr));
    } else if (mode == "nnet_copy" && argc == 5) {
      // nnet_copy <nnet_in> <binary> <nnet_out>
      Nnet nnet; nnet.Read(argv[2]);
      nnet.Write(argv[4], atoi(argv[3]) != 0);
      std::cout << "OK " << nnet.NumComponents() << " " << nnet.NumDropout();
      for (int i = 0; i < nnet.NumComponents(); i++) std::cout << " " << nnet.GetComponent(i).Marker();
      std::cout << "\n";
    } else if (mode == "without" && argc == 4) {
      // without <nnet_in> <nnet_out (binary)>
      Nnet nnet, plain; nnet.Read(argv[2]);
      WithoutDropout(nnet, &plain);
      plain.Write(argv[3], true);
      std::cout << "OK " << plain.NumComponents() << " " << plain.NumDropout() << "\n";
    } else if (mode == "standard" && argc == 5) {
      // standard <nnet_in> <shift> <nnet_out (binary)>
      Nnet nnet, std_; nnet.Read(argv[2]);
      ConvertToStandard(nnet, atoi(argv[3]), &std_);
      std_.Write(argv[4], true);
      std::cout << "OK " << std_.NumComponents() << " " << std_.NumDropout() << "\n";
    } else if (mode == "retention" && argc == 5) {
      // retention <nnet_in> <r> <nnet_out (text)>     SetDropoutRetention, the reference's declared method
      Nnet nnet; nnet.Read(argv[2]);
      nnet.SetDropoutRetention((float)atof(argv[3]));
      nnet.Write(argv[4], false);
      std::cout << "OK " << nnet.NumDropout() << " " << (all_off(nnet) ? "off" : "on") << "\n";
    } else if (mode == "topology" && argc == 4) {
      // topology <nnet_in> <lm_in>: what BatchScorer says to the model as it is and to its WithoutDropout form, and CtcNeuralRescorer to the LM
      Nnet nnet, plain, lm; nnet.Read(argv[2]); lm.Read(argv[3]);
      WithoutDropout(nnet, &plain);
      BatchScorerOptions so;
      CtcNeuralRescorerOptions ro;
      std::cout << "OK\n";
      std::cout << "scorer: " << refusal([&] { BatchScorer::CheckTopology(nnet, so); }) << "\n";
      std::cout << "scorer_plain: " << refusal([&] { BatchScorer::CheckTopology(plain, so); }) << "\n";
      std::cout << "rescorer: " << refusal([&] { CtcNeuralRescorer::CheckTopology(lm, ro); }) << "\n";
    } else if (mode == "layer" && argc == 8) {
      // layer <x_raw> <rows> <cols> <seed> <per_sequence> <out_raw>      GPU.  Transmit -> Dropout 0.8 (component 1: salt 1) through
      // Nnet::Propagate / Backpropagate: one pass switched off, then three minibatches switched on (4 streams; Reset flags all, then
      // stream 1 alone, then none).  Dumps out and in_diff (of out_diff = x) of each of the four passes.
      const std::vector<float> x = read_raw(argv[2]);
      const int rows = atoi(argv[3]), cols = atoi(argv[4]);
      Nnet nnet;
      nnet.AppendComponent(new TransmitLayer(cols, cols));
      nnet.AppendComponent(new DropoutLayer(cols, cols));
      nnet.SetDropoutRetention(0.8f);
      nnet.SetDropoutSeed(strtoull(argv[5], nullptr, 0));
      nnet.SetDropoutPerSequence(atoi(argv[6]) != 0);
      DeviceMatrix in, out, in_diff;
      in.CopyFromHost(x.data(), rows, cols);
      in_diff.Resize(rows, cols);
      std::vector<float> all, h;
      std::ofstream f(argv[7], std::ios::binary);
      const int flags[4][4] = {{1, 1, 1, 1}, {1, 1, 1, 1}, {0, 1, 0, 0}, {0, 0, 0, 0}};
      for (int pass = 0; pass < 4; pass++) {
        if (pass == 1) nnet.SetDropoutActive(true);
        if (pass >= 1) { std::vector<int> fl(flags[pass], flags[pass] + 4); nnet.Reset(fl); }
        nnet.Propagate(in.View(), &out);
        MatrixView idv = in_diff.View();
        nnet.Backpropagate(in.View(), &idv);
        out.CopyToHost(&h); f.write(reinterpret_cast<const char *>(h.data()), h.size() * sizeof(float));
        in_diff.CopyToHost(&h); f.write(reinterpret_cast<const char *>(h.data()), h.size() * sizeof(float));
      }
      std::cout << "OK " << static_cast<DropoutLayer &>(nnet.GetComponent(1)).Step() << "\n";
    } else if (mode == "train" && argc == 13) {
      // train <nnet_in> <utts_raw> <S> <T> <delay> <lr> <momentum> <crossvalidate> <retention (0: the model's)> <seed> <nnet_out>   GPU
      // TrainLstmStreams with the dropout options.  Under crossvalidate the same pass runs over the WithoutDropout form as well and
      // both losses are printed as hexadecimal floats.
      Nnet nnet; nnet.Read(argv[2]);
      std::vector<Utterance> utts = read_utts(argv[3]);
      TrainLstmStreamsOptions o;
      o.num_stream = atoi(argv[4]); o.batch_size = atoi(argv[5]); o.targets_delay = atoi(argv[6]);
      o.trn_opts.learn_rate = (float)atof(argv[7]); o.trn_opts.momentum = (float)atof(argv[8]);
      o.crossvalidate = atoi(argv[9]) != 0;
      o.dropout_retention = (float)atof(argv[10]);
      o.dropout_seed = strtoull(argv[11], nullptr, 0);
      if (!all_off(nnet)) KLSTM_ERR("a model that was just read has its dropout on");
      std::string report;
      const TrainLstmStreamsStats st = TrainLstmStreams(&nnet, utts, o, &report);
      const bool restored = all_off(nnet);
      if (!o.crossvalidate) nnet.Write(argv[12], true);
      std::cout.precision(10);
      std::cout << "OK " << st.num_done << " " << st.num_minibatches << " " << st.total_frames << " " << st.avg_loss << " "
                << st.frame_accuracy << " " << (restored ? "restored" : "LEFT_ON") << " " << nnet.NumDropout() << "\n";
      if (o.crossvalidate) {
        Nnet plain;
        WithoutDropout(nnet, &plain);
        const TrainLstmStreamsStats sp = TrainLstmStreams(&plain, utts, o);
        std::printf("CV %a %a %a %a\n", st.avg_loss, sp.avg_loss, st.frame_accuracy, sp.frame_accuracy);
      }
    } else if (mode == "ctc" && argc == 2) {
      // ctc      GPU.  The two-layer stack with a <Dropout> between the layers, 3 streams, a dozen pattern utterances, two epochs of
      // TrainCtcWholeUtterances with dropout_per_sequence: two runs with one seed, one with another seed, one per element; then
      // DecodeCtcWholeUtterances on the trained model and on its WithoutDropout form.
      const int32 S = 3, K = 6, epochs = 2;
      std::vector<Utterance> utts;
      for (int32 i = 0; i < 12; i++) utts.push_back(pattern_utt(100 + i, 4 + i % 7, K));
      Nnet trained;
      const std::string a = ctc_run(utts, S, K, 11, true, epochs, &trained), b = ctc_run(utts, S, K, 11, true, epochs);
      const std::string c = ctc_run(utts, S, K, 12, true, epochs), d = ctc_run(utts, S, K, 11, false, epochs);
      Nnet untouched;
      ctc_stack(S, K, &untouched);
      CHECK(a == b);                                   // one seed: bit-identical models
      CHECK(a != c);                                   // another seed: another model
      CHECK(a != d);                                   // one mask per sequence is not one per element
      CHECK(a != model_bytes(untouched));              // (and it trained at all)
      Nnet plain;
      WithoutDropout(trained, &plain);
      CHECK(trained.NumDropout() == 1 && plain.NumDropout() == 0 && plain.NumComponents() == trained.NumComponents() - 1);
      DecodeCtcOptions dopt;
      dopt.num_stream = S;
      std::vector<std::vector<int32> > h1, h2;
      const DecodeCtcStats s1 = DecodeCtcWholeUtterances(&trained, utts, dopt, &h1), s2 = DecodeCtcWholeUtterances(&plain, utts, dopt, &h2);
      CHECK(h1.size() == utts.size() && h1 == h2);
      CHECK(s1.num_errors == s2.num_errors && s1.token_error_rate == s2.token_error_rate);
      size_t tokens = 0;
      for (const auto &h : h1) tokens += h.size();
      if (failures) return 1;
      std::cout << "OK models " << a.size() << " bytes, " << h1.size() << " hypotheses, " << tokens << " tokens, token error rate " << s1.token_error_rate << "\n";
    } else {
      std::cerr << "usage: dropout_test errors|messages|nnet_copy|without|standard|retention|topology|layer|train|ctc ...\n";
      return 2;
    }
    return 0;
  } catch (const std::exception &e) {
    std::cout << "EXCEPTION: " << e.what() << "\n";
    return 3;
  }
}
