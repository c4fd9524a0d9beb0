// tests/cpp/cnn_test.cpp -- drives the kcnn_* entries (include/klstm_cnn.h) and the <ConvolutionalComponent>, <MaxPoolingComponent>,
// <Sigmoid> and <Tanh> components of include/klstm_nnet.hpp for tests/test_cnn*.py.  The modes errors and nnet_copy are host only;
// layers and train need the GPU.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "klstm_cnn.h"
#include "klstm_nnet.hpp"

using namespace klstm_kaldi;

static int failures = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) { std::printf("FAILED %s:%d: %s (last error: '%s')\n", __FILE__, __LINE__, #c, klstm_last_error()); failures++; } \
  } while (0)
#define REFUSED(call, msg)                                                       \
  do {                                                                           \
    CHECK((call) == KLSTM_ERR_ARG);                                              \
    CHECK(std::strstr(klstm_last_error(), msg) != nullptr);                      \
    refusals++;                                                                  \
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
// GetParams of every component, one after the other
static void dump_params(const Nnet &nnet, const char *path) {
  std::ofstream f(path, std::ios::binary);
  std::vector<BaseFloat> p;
  for (int i = 0; i < nnet.NumComponents(); i++) {
    nnet.GetComponent(i).GetParams(&p);
    f.write(reinterpret_cast<const char *>(p.data()), p.size() * sizeof(BaseFloat));
  }
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "errors" && argc == 2) {
      // every KLSTM_ERR_ARG of the entries, before any HIP call (no device is needed); the pointers are never followed and the
      // outputs stay as they were
      float buf[256] = {0};
      float *a = buf, *b = buf + 64, *c = buf + 128, *d = buf + 192;
      int refusals = 0, n = 7, P = 7, K = 7, F = 7;
      CHECK(std::strcmp(klstm_last_error(), "") == 0);
      // kcnn_conv_plan: in 12 = 1 block of 12, patches of 4 every 4: P = 3, K = 4; out 6: F = 2
      CHECK(kcnn_conv_plan(12, 6, 4, 4, 12, &n, &P, &K, &F) == KLSTM_OK && n == 1 && P == 3 && K == 4 && F == 2);
      CHECK(kcnn_conv_plan(440, 4224, 8, 1, 40, &n, &P, &K, &F) == KLSTM_OK && n == 11 && P == 33 && K == 88 && F == 128);
      n = P = K = F = 7;
      REFUSED(kcnn_conv_plan(12, 6, 4, 4, 12, nullptr, &P, &K, &F), "null argument");
      REFUSED(kcnn_conv_plan(0, 6, 4, 4, 12, &n, &P, &K, &F), "a number below 1");
      REFUSED(kcnn_conv_plan(12, 6, 4, 0, 12, &n, &P, &K, &F), "a number below 1");
      REFUSED(kcnn_conv_plan(12, 6, 4, 4, 5, &n, &P, &K, &F), "does not divide the input dim");
      REFUSED(kcnn_conv_plan(12, 6, 13, 1, 12, &n, &P, &K, &F), "above the patch stride");
      REFUSED(kcnn_conv_plan(12, 6, 4, 3, 12, &n, &P, &K, &F), "does not divide stride - dim");
      REFUSED(kcnn_conv_plan(12, 7, 4, 4, 12, &n, &P, &K, &F), "do not divide the output dim");
      CHECK(n == 7 && P == 7 && K == 7 && F == 7);
      CHECK(kcnn_conv_workspace_floats(65, 12, 6, 4, 4, 12) == 2 * (2 * 4 + 2 * 2) && kcnn_conv_workspace_floats(0, 12, 6, 4, 4, 12) == 0);
      CHECK(kcnn_conv_workspace_floats(65, 12, 7, 4, 4, 12) == 0);
      // the four convolution entries: geometry (12, 6, 4, 4, 12)
      REFUSED(kcnn_conv_propagate(a, 12, 2, 12, 7, 4, 4, 12, b, c, d, 6, nullptr), "kcnn_conv_propagate: inconsistent numbers");
      REFUSED(kcnn_conv_propagate(a, 12, -1, 12, 6, 4, 4, 12, b, c, d, 6, nullptr), "kcnn_conv_propagate: rows");
      REFUSED(kcnn_conv_propagate(nullptr, 12, 2, 12, 6, 4, 4, 12, b, c, d, 6, nullptr), "kcnn_conv_propagate: null argument");
      REFUSED(kcnn_conv_propagate(a, 12, 2, 12, 6, 4, 4, 12, b, nullptr, d, 6, nullptr), "kcnn_conv_propagate: null argument");
      REFUSED(kcnn_conv_propagate(a, 11, 2, 12, 6, 4, 4, 12, b, c, d, 6, nullptr), "kcnn_conv_propagate: row stride");
      REFUSED(kcnn_conv_propagate(a, 12, 2, 12, 6, 4, 4, 12, b, c, d, 5, nullptr), "kcnn_conv_propagate: row stride");
      REFUSED(kcnn_conv_backpropagate(a, 6, 2, 12, 6, 5, 4, 12, b, d, 12, nullptr), "kcnn_conv_backpropagate: inconsistent numbers");
      REFUSED(kcnn_conv_backpropagate(a, 6, -2, 12, 6, 4, 4, 12, b, d, 12, nullptr), "kcnn_conv_backpropagate: rows");
      REFUSED(kcnn_conv_backpropagate(a, 6, 2, 12, 6, 4, 4, 12, nullptr, d, 12, nullptr), "kcnn_conv_backpropagate: null argument");
      REFUSED(kcnn_conv_backpropagate(a, 5, 2, 12, 6, 4, 4, 12, b, d, 12, nullptr), "kcnn_conv_backpropagate: row stride");
      REFUSED(kcnn_conv_backpropagate(a, 6, 2, 12, 6, 4, 4, 12, b, d, 11, nullptr), "kcnn_conv_backpropagate: row stride");
      REFUSED(kcnn_conv_gradient(a, 12, b, 6, 2, 12, 6, 4, 4, 24, c, d, d, 64, nullptr), "kcnn_conv_gradient: inconsistent numbers");
      REFUSED(kcnn_conv_gradient(a, 12, b, 6, -1, 12, 6, 4, 4, 12, c, d, d, 64, nullptr), "kcnn_conv_gradient: rows");
      REFUSED(kcnn_conv_gradient(a, 12, b, 6, 2, 12, 6, 4, 4, 12, c, nullptr, d, 64, nullptr), "kcnn_conv_gradient: null argument");
      REFUSED(kcnn_conv_gradient(a, 12, b, 5, 2, 12, 6, 4, 4, 12, c, d, d, 64, nullptr), "kcnn_conv_gradient: row stride");
      REFUSED(kcnn_conv_gradient(a, 12, b, 6, 2, 12, 6, 4, 4, 12, c, d, d, 11, nullptr), "kcnn_conv_gradient: workspace of 11 floats, 12 needed");
      REFUSED(kcnn_conv_gradient(a, 12, b, 6, 2, 12, 6, 4, 4, 12, c, d, nullptr, 64, nullptr), "kcnn_conv_gradient: workspace of 0 floats");
      REFUSED(kcnn_conv_update(a, 12, b, 6, 2, 12, 6, 4, 4, 12, c, d, c, nullptr, 0.1f, 0.1f, 0.f, d, 64, nullptr), "kcnn_conv_update: null argument");
      REFUSED(kcnn_conv_update(a, 12, b, 6, 2, 12, 6, 4, 4, 12, c, d, c, d, 0.1f, 0.1f, 0.f, d, 9, nullptr), "kcnn_conv_update: workspace");
      REFUSED(kcnn_conv_update(a, 12, b, 6, 2, 12, 5, 4, 4, 12, c, d, c, d, 0.1f, 0.1f, 0.f, d, 64, nullptr), "kcnn_conv_update: inconsistent numbers");
      // pooling: 5 patches of 3, pools of 3 every 1: Q = 3
      REFUSED(kcnn_pool_propagate(a, 15, 2, 15, 9, 3, 1, 4, b, 9, nullptr), "kcnn_pool_propagate: inconsistent numbers");
      REFUSED(kcnn_pool_propagate(a, 15, 2, 15, 9, 6, 1, 3, b, 9, nullptr), "kcnn_pool_propagate: inconsistent numbers");
      REFUSED(kcnn_pool_propagate(a, 15, 2, 15, 9, 2, 2, 3, b, 9, nullptr), "kcnn_pool_propagate: inconsistent numbers");
      REFUSED(kcnn_pool_propagate(a, 15, 2, 15, 6, 3, 1, 3, b, 9, nullptr), "kcnn_pool_propagate: inconsistent numbers");
      REFUSED(kcnn_pool_propagate(a, 15, -1, 15, 9, 3, 1, 3, b, 9, nullptr), "kcnn_pool_propagate: rows");
      REFUSED(kcnn_pool_propagate(a, 15, 2, 15, 9, 3, 1, 3, nullptr, 9, nullptr), "kcnn_pool_propagate: null argument");
      REFUSED(kcnn_pool_propagate(a, 14, 2, 15, 9, 3, 1, 3, b, 9, nullptr), "kcnn_pool_propagate: row stride");
      REFUSED(kcnn_pool_backpropagate(a, 15, b, 9, c, 9, 2, 15, 9, 3, 0, 3, d, 15, nullptr), "kcnn_pool_backpropagate: inconsistent numbers");
      REFUSED(kcnn_pool_backpropagate(a, 15, b, 9, c, 9, -1, 15, 9, 3, 1, 3, d, 15, nullptr), "kcnn_pool_backpropagate: rows");
      REFUSED(kcnn_pool_backpropagate(a, 15, nullptr, 9, c, 9, 2, 15, 9, 3, 1, 3, d, 15, nullptr), "kcnn_pool_backpropagate: null argument");
      REFUSED(kcnn_pool_backpropagate(a, 15, b, 9, c, 8, 2, 15, 9, 3, 1, 3, d, 15, nullptr), "kcnn_pool_backpropagate: row stride");
      REFUSED(kcnn_pool_backpropagate(a, 15, b, 9, c, 9, 2, 15, 9, 3, 1, 3, d, 14, nullptr), "kcnn_pool_backpropagate: row stride");
      // activations
      REFUSED(kcnn_activation(2, a, 8, 2, 8, b, 8, nullptr), "kcnn_activation: unknown kind");
      REFUSED(kcnn_activation(KCNN_TANH, a, 8, -2, 8, b, 8, nullptr), "kcnn_activation: bad size");
      REFUSED(kcnn_activation(KCNN_TANH, a, 8, 2, 8, nullptr, 8, nullptr), "kcnn_activation: null argument");
      REFUSED(kcnn_activation(KCNN_SIGMOID, a, 7, 2, 8, b, 8, nullptr), "kcnn_activation: row stride");
      REFUSED(kcnn_activation(KCNN_SIGMOID, a, 8, 2, 8, a, 16, nullptr), "kcnn_activation: in == out with two strides");
      REFUSED(kcnn_activation_diff(-1, a, 8, b, 8, 2, 8, c, 8, nullptr), "kcnn_activation_diff: unknown kind");
      REFUSED(kcnn_activation_diff(KCNN_TANH, a, 8, b, 8, 2, -8, c, 8, nullptr), "kcnn_activation_diff: bad size");
      REFUSED(kcnn_activation_diff(KCNN_TANH, nullptr, 8, b, 8, 2, 8, c, 8, nullptr), "kcnn_activation_diff: null argument");
      REFUSED(kcnn_activation_diff(KCNN_TANH, a, 8, b, 8, 2, 8, c, 7, nullptr), "kcnn_activation_diff: row stride");
      REFUSED(kcnn_activation_diff(KCNN_TANH, a, 8, b, 8, 2, 8, b, 16, nullptr), "kcnn_activation_diff: in_diff == out_diff with two strides");
      // zero rows and an unwanted in_diff are fine and launch nothing (no device here), null pointers included
      CHECK(kcnn_conv_propagate(nullptr, 0, 0, 12, 6, 4, 4, 12, nullptr, nullptr, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_conv_backpropagate(nullptr, 0, 0, 12, 6, 4, 4, 12, nullptr, d, 12, nullptr) == KLSTM_OK);
      CHECK(kcnn_conv_backpropagate(a, 6, 2, 12, 6, 4, 4, 12, b, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_conv_gradient(nullptr, 0, nullptr, 0, 0, 12, 6, 4, 4, 12, nullptr, nullptr, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_conv_update(nullptr, 0, nullptr, 0, 0, 12, 6, 4, 4, 12, nullptr, nullptr, nullptr, nullptr, 0.1f, 0.1f, 0.9f, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_pool_propagate(nullptr, 0, 0, 15, 9, 3, 1, 3, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_pool_backpropagate(a, 15, b, 9, c, 9, 2, 15, 9, 3, 1, 3, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_activation(KCNN_SIGMOID, nullptr, 0, 0, 8, nullptr, 0, nullptr) == KLSTM_OK);
      CHECK(kcnn_activation_diff(KCNN_SIGMOID, a, 8, b, 8, 2, 8, nullptr, 0, nullptr) == KLSTM_OK);
      for (float v : buf) CHECK(v == 0.f);
      if (failures) return 1;
      std::printf("OK %d refusals before any HIP call\n", refusals);
    } else if (mode == "nnet_copy" && argc == 5) {
      // nnet_copy <nnet_in> <binary> <nnet_out>
      Nnet nnet; nnet.Read(argv[2]);
      nnet.Write(argv[4], atoi(argv[3]) != 0);
      int32 params = 0;
      for (int i = 0; i < nnet.NumComponents(); i++) params += nnet.GetComponent(i).NumParams();
      std::cout << "OK " << nnet.NumComponents() << " " << params;
      for (int i = 0; i < nnet.NumComponents(); i++) std::cout << " " << nnet.GetComponent(i).Marker();
      std::cout << "\n";
    } else if (mode == "layers" && argc == 11) {
      // layers <nnet_in> <x_raw> <out_diff_raw> <rows> <lr> <momentum> <steps> <dump_raw> <nnet_out>        GPU.  `steps` times
      // Nnet::Propagate and Nnet::Backpropagate (with Update, as a trainer drives them) on one input and one out_diff; dumps out and
      // the in_diff of the first component of every step, then writes the trained model in binary.
      Nnet nnet; nnet.Read(argv[2]);
      const std::vector<float> x = read_raw(argv[3]), od = read_raw(argv[4]);
      const int rows = atoi(argv[5]), steps = atoi(argv[8]);
      NnetTrainOptions opts;
      opts.learn_rate = (float)atof(argv[6]); opts.momentum = (float)atof(argv[7]);
      nnet.SetTrainOptions(opts);
      if ((int)x.size() != rows * nnet.InputDim() || (int)od.size() != rows * nnet.OutputDim()) KLSTM_ERR("layers: sizes of the raw files");
      DeviceMatrix in, out, out_diff, in_diff;
      in.CopyFromHost(x.data(), rows, nnet.InputDim());
      out_diff.CopyFromHost(od.data(), rows, nnet.OutputDim());
      in_diff.Resize(rows, nnet.InputDim());
      std::ofstream dump(argv[9], std::ios::binary);
      std::vector<float> h;
      for (int step = 0; step < steps; step++) {
        nnet.Propagate(in.View(), &out);
        MatrixView idv = in_diff.View();
        nnet.Backpropagate(out_diff.View(), &idv);
        out.CopyToHost(&h); dump.write(reinterpret_cast<const char *>(h.data()), h.size() * sizeof(float));
        in_diff.CopyToHost(&h); dump.write(reinterpret_cast<const char *>(h.data()), h.size() * sizeof(float));
      }
      nnet.Write(argv[10], true);
      std::cout << "OK " << nnet.NumComponents() << " " << steps << "\n";
    } else if (mode == "train" && argc == 14) {
      // train <nnet_in> <utts_raw> <ctc_utts_raw> <S> <T> <delay> <lr> <momentum> <params_before_raw> <params_after_streams_raw>
      //       <params_after_ctc_raw> <frame_classes_raw>        GPU.  TrainLstmStreams over the first utterances, then one pass of
      // TrainCtcWholeUtterances over the second (their targets are the label sequences; one minibatch of S), then the same minibatch
      // through Nnet::Propagate and CtcGreedyDecoder.  GetParams of every component at the three points; the decoder's frame classes
      // [T x S] as int32; the hypotheses on the output line.
      Nnet nnet; nnet.Read(argv[2]);
      std::vector<Utterance> utts = read_utts(argv[3]), cutts = read_utts(argv[4]);
      for (auto &u : cutts) { u.labels = u.targets; u.targets.clear(); }
      const int32 S = atoi(argv[5]);
      TrainLstmStreamsOptions o;
      o.num_stream = S; o.batch_size = atoi(argv[6]); o.targets_delay = atoi(argv[7]);
      o.trn_opts.learn_rate = (float)atof(argv[8]); o.trn_opts.momentum = (float)atof(argv[9]);
      dump_params(nnet, argv[10]);
      const TrainLstmStreamsStats st = TrainLstmStreams(&nnet, utts, o);
      dump_params(nnet, argv[11]);
      TrainCtcOptions co;
      co.trn_opts = o.trn_opts; co.num_stream = S;
      const TrainCtcStats cs = TrainCtcWholeUtterances(&nnet, cutts, co);
      dump_params(nnet, argv[12]);
      WholeUtteranceBatcher batcher(&cutts, S, true, 0);
      UtteranceBatch b;
      if (!batcher.Next(&b)) KLSTM_ERR("train: no CTC minibatch");
      DeviceMatrix feat, out;
      std::vector<int> all(S, 1);
      nnet.SetSeqLengths(b.lens);
      nnet.Reset(all);
      feat.CopyFromHost(b.feat.data(), b.num_frames * b.num_stream, b.dim);
      nnet.Propagate(feat.View(), &out);
      CtcGreedyDecoder dec(0);
      std::vector<std::vector<int32> > hyps;
      dec.Decode(out, S, b.lens, b.labels, &hyps);
      std::vector<int32> fc;
      dec.FrameClasses(&fc);
      std::ofstream f(argv[13], std::ios::binary);
      f.write(reinterpret_cast<const char *>(fc.data()), fc.size() * sizeof(int32));
      std::cout.precision(10);
      std::cout << "OK " << st.num_done << " " << st.num_minibatches << " " << cs.num_done << " " << cs.num_minibatches << " " << cs.num_rejected << " "
                << b.num_frames << " " << cs.avg_loss;
      for (const auto &h : hyps) { std::cout << " |"; for (int32 c : h) std::cout << " " << c; }
      std::cout << "\n";
    } else {
      std::cerr << "usage: cnn_test errors|nnet_copy|layers|train ...\n";
      return 2;
    }
    return 0;
  } catch (const std::exception &e) {
    std::cout << "EXCEPTION: " << e.what() << "\n";
    return 3;
  }
}
