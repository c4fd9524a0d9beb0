// tests/cpp/ctc_nlm_test.cpp -- drives CtcNeuralRescorer and DecodeCtcOptions::neural_rescorer (include/klstm_nnet.hpp) for
// tests/test_ctc_nlm_gpu.py.  `rescore`: an LM read from a model file that Nnet::Write wrote rescores lists given in a file, and what it
// made of them is dumped for the comparison with the Python call.  `decode`: the pattern task of tests/cpp/ctc_rescore_test.cpp decoded
// without the option, with an LM that cannot change an order (nlm_scale 0), and with an LM behind an n-gram rescorer and before the
// consensus.  `utterances` (host only): what LmTrainingUtterances makes of three sequences, for tests/test_ctc_nlm.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

template <class T>
static void put(std::ofstream &f, const std::vector<T> &v) { f.write(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T)); }
template <class T>
static std::vector<T> get(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  f.read(reinterpret_cast<char *>(v.data()), n * sizeof(T));
  if (!f) KLSTM_ERR("the lists file is too short");
  return v;
}
template <class T>
static std::vector<T> down(const T *dev, size_t n) {
  std::vector<T> v(n);
  if (n) KCheck(klstm_memcpy_d2h(v.data(), dev, n * sizeof(T), nullptr));
  return v;
}

// the memorisable pattern task of tests/cpp/ctc_test.cpp
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
static LstmProjectedStreams *new_lstm(int32 in, int32 cell, int32 out, int32 streams, const char *scale) {
  std::unique_ptr<LstmProjectedStreams> c(new LstmProjectedStreams(in, out));
  std::ostringstream cfg;
  cfg << "<CellDim> " << cell << " <NumStream> " << streams << " <ParamScale> " << scale;
  std::istringstream is(cfg.str());
  c->InitData(is);
  return c.release();
}
static AffineLayer *new_affine(int32 in, int32 out, double scale) {
  AffineLayer *aff = new AffineLayer(in, out);
  std::vector<BaseFloat> w((size_t)out * in), bias(out, 0.f);
  for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * scale);
  aff->SetParams(w, bias);
  return aff;
}
// everything of the statistics but the wall clock and the neural rescorer's own three
static bool same_stats(const DecodeCtcStats &a, const DecodeCtcStats &b) {
  const double x[] = {a.token_error_rate, a.utt_error_rate, a.num_scored, a.num_errors, a.num_ref_tokens, a.oracle_token_error_rate,
                      a.expected_errors, a.map_expected_errors, a.mean_confidence, a.num_pick_errors, a.first_pass_token_error_rate,
                      a.rescored_token_error_rate, a.num_changed_1best};
  const double y[] = {b.token_error_rate, b.utt_error_rate, b.num_scored, b.num_errors, b.num_ref_tokens, b.oracle_token_error_rate,
                      b.expected_errors, b.map_expected_errors, b.mean_confidence, b.num_pick_errors, b.first_pass_token_error_rate,
                      b.rescored_token_error_rate, b.num_changed_1best};
  return a.num_done == b.num_done && a.num_skipped == b.num_skipped && a.num_minibatches == b.num_minibatches &&
         std::memcmp(x, y, sizeof(x)) == 0;
}
static bool same_lists(const std::vector<CtcNbestList> &a, const std::vector<CtcNbestList> &b) {
  bool same = a.size() == b.size();
  for (size_t i = 0; i < a.size() && same; i++) {
    same = a[i].size() == b[i].size();
    for (size_t q = 0; q < a[i].size() && same; q++) same = a[i][q].tokens == b[i][q].tokens && a[i][q].errors == b[i][q].errors;
  }
  return same;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rescore" && argc == 13) {
      // rescore <model> <lists> <dump> <E> <T> <K> <bos> <eos> <am_scale> <nlm_scale> <unit_bonus>      GPU.
      // <lists>, in 4-byte words: S, N, stride, count [S], hyp_len [S*N], logp [S*N] (floats), errors [S*N], hyp [S*N*stride].
      // <dump>: order [S*N], live [S], score, nlm_logp (floats), units [S*N], then of the re-ranked list count [S], len, score, errors
      // [S*N], hyp [S*N*stride].
      Nnet given, lm;
      given.Read(argv[2]);
      const std::string rewritten = std::string(argv[2]) + ".written";
      given.Write(rewritten, true);                                  // the rescorer reads what Nnet::Write wrote
      lm.Read(rewritten);
      std::ifstream f(argv[3], std::ios::binary);
      const std::vector<int32> head = get<int32>(f, 3);
      const int32 S = head[0], N = head[1], stride = head[2];
      const size_t SN = (size_t)S * N;
      const std::vector<int32> count = get<int32>(f, S), hyp_len = get<int32>(f, SN);
      const std::vector<BaseFloat> logp = get<BaseFloat>(f, SN);
      const std::vector<int32> errors = get<int32>(f, SN), hyp = get<int32>(f, SN * stride);
      DeviceBuffer dc, dl, dp, de, dh;
      dc.Upload(count); dl.Upload(hyp_len); dp.Upload(logp); de.Upload(errors); dh.Upload(hyp);
      CtcNeuralRescorerOptions o;
      o.num_stream = std::atoi(argv[5]); o.chunk = std::atoi(argv[6]); o.num_classes = std::atoi(argv[7]);
      o.bos = std::atoi(argv[8]); o.eos = std::atoi(argv[9]);
      o.am_scale = (BaseFloat)std::atof(argv[10]); o.nlm_scale = (BaseFloat)std::atof(argv[11]); o.unit_bonus = (BaseFloat)std::atof(argv[12]);
      CtcNeuralRescorer r(lm, o);
      const CtcNbestDevice nb{dh.As<int32>(), dl.As<int32>(), dc.As<int32>(), de.As<int32>(), S, N, stride, dp.As<BaseFloat>()};
      r.Rescore(nb);
      r.Rescore(nb);                                                  // twice: the second call's answers are the first's
      std::vector<int32> order, live, units;
      std::vector<BaseFloat> score, nlp;
      r.Order(&order, &live);
      r.Entries(&score, &nlp, &units);
      const CtcNbestDevice out = r.DeviceLists();
      std::ofstream g(argv[4], std::ios::binary);
      put(g, order); put(g, live); put(g, score); put(g, nlp); put(g, units);
      put(g, down(out.count, S)); put(g, down(out.hyp_len, SN)); put(g, down(out.score, SN)); put(g, down(out.errors, SN));
      put(g, down(out.hyp, SN * stride));
      std::vector<CtcNbestList> lists;
      r.Lists(&lists);
      std::cout << "OK utterances=" << r.NumUtterances() << " positions=" << r.NumPositions() << " lists=" << lists.size() << "\n";
    } else if (mode == "decode" && argc == 3) {
      // decode <epochs>      GPU
      const int32 S = 4, K = 6, N = 4, epochs = std::atoi(argv[2]);
      std::srand(7);
      std::vector<Utterance> utts;
      for (int32 i = 0; i < 8; i++) utts.push_back(pattern_utt(100 + i, 4 + i % 7, K));
      TrainCtcOptions o;
      o.num_stream = S;
      o.max_frames = 100;
      o.trn_opts.learn_rate = 0.01f;
      o.trn_opts.momentum = 0.9f;
      Nnet nnet;
      nnet.AppendComponent(new TransmitLayer(16, 16));
      nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S, "0.1")));
      nnet.AppendComponent(new_affine(16, K, 0.2));
      nnet.AppendComponent(new SoftmaxLayer(K, K));
      for (int32 e = 0; e < epochs; e++) TrainCtcWholeUtterances(&nnet, utts, o);
      // the LM: untrained, over the K classes, the blank its bos and eos
      Nnet lm;
      lm.AppendComponent(new LstmLayer(new_lstm(K, 16, 8, 1, "0.5")));
      lm.AppendComponent(new_affine(8, K, 2.0));
      lm.AppendComponent(new SoftmaxLayer(K, K));

      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      d.beam = 8; d.cands = 5; d.nbest = N;
      std::vector<std::vector<int32> > best, best_zero, best_nlm;
      std::vector<CtcNbestList> lists, lists_zero, lists_nlm;
      std::string rep, rep_zero, rep_nlm;
      // without the option: what the loop reports today
      const DecodeCtcStats plain = DecodeCtcWholeUtterances(&nnet, utts, d, &best, &lists, &rep);
      const bool off_zero = plain.neural_first_pass_token_error_rate == 0 && plain.neural_rescored_token_error_rate == 0 &&
                            plain.num_neural_changed_1best == 0 && rep.find("NEURAL") == std::string::npos;
      // an LM that cannot move an entry: the same answers
      CtcNeuralRescorerOptions oz;
      oz.num_stream = 4; oz.chunk = 5; oz.nlm_scale = 0.f;
      CtcNeuralRescorer zero(lm, oz);
      DecodeCtcOptions dz = d;
      dz.neural_rescorer = &zero;
      const DecodeCtcStats sz = DecodeCtcWholeUtterances(&nnet, utts, dz, &best_zero, &lists_zero, &rep_zero);
      const bool zero_same = best_zero == best && same_lists(lists, lists_zero) && same_stats(sz, plain) && sz.num_neural_changed_1best == 0 &&
                             sz.neural_first_pass_token_error_rate == plain.token_error_rate &&
                             sz.neural_rescored_token_error_rate == plain.token_error_rate && zero.NumForbidden() == 0;
      // search -> n-gram rescorer -> LM -> consensus
      SparseLabelLm h;
      h.num_classes = K;
      unsigned sd = 11u;
      h.arc_offsets.push_back(0);
      for (int32 c = 1; c < K; c++) { h.arc_labels.push_back(c); h.arc_next.push_back(0); h.arc_weight.push_back(0.05f + 0.9f * (float)(lcg(&sd) % 1000u) / 1000.f); }
      h.arc_offsets.push_back((int32)h.arc_labels.size());
      h.backoff.push_back(-1); h.backoff_weight.push_back(1.f); h.final_weight.push_back(0.5f);
      const CtcSparseLabelLm uni(h, 0);
      CtcRescorer ngram(K, &uni, nullptr);
      CtcNeuralRescorerOptions on;
      on.num_stream = 4; on.chunk = 5; on.nlm_scale = 1.5f; on.unit_bonus = 0.5f;
      CtcNeuralRescorer nlm(lm, on);
      DecodeCtcOptions dn = d;
      dn.rescorer = &ngram; dn.neural_rescorer = &nlm; dn.consensus = 1;
      std::vector<std::vector<BaseFloat> > conf;
      const DecodeCtcStats sn = DecodeCtcWholeUtterances(&nnet, utts, dn, &best_nlm, &lists_nlm, &conf, &rep_nlm);
      bool heads = best_nlm.size() == utts.size(), conf_ok = true;
      double new_errors = 0;
      for (size_t i = 0; i < utts.size(); i++) {
        heads = heads && !lists_nlm[i].empty() && best_nlm[i] == lists_nlm[i][0].tokens;           // consensus 1: the head of the re-ranked list
        conf_ok = conf_ok && conf[i].size() == best_nlm[i].size();
        new_errors += lists_nlm[i].empty() ? 0 : lists_nlm[i][0].errors;
      }
      const bool staged = sn.neural_first_pass_token_error_rate == sn.rescored_token_error_rate &&      // it read the n-gram stage's lists
                          sn.neural_rescored_token_error_rate == new_errors / plain.num_ref_tokens && sn.first_pass_token_error_rate == plain.token_error_rate &&
                          sn.num_neural_changed_1best == nlm.NumChanged();
      std::cerr << rep_nlm;
      std::cout.precision(17);
      std::cout << "OK off_zero=" << (int)off_zero << " zero_same=" << (int)zero_same << " heads=" << (int)heads << " conf_ok=" << (int)conf_ok
                << " staged=" << (int)staged << " changed=" << sn.num_neural_changed_1best << " utterances=" << nlm.NumUtterances()
                << " has_report=" << (int)(rep_nlm.find("NEURAL RESCORED") != std::string::npos && rep_nlm.find("RESCORED") < rep_nlm.find("NEURAL RESCORED"))
                << "\n";
    } else if (mode == "utterances" && argc == 5) {
      // utterances <V> <bos> <eos>      host only.  LmTrainingUtterances of the sequences {3, 1, 2}, {}, {5}: per utterance a line
      // "frames dim : the column of the 1 in every row (-1: the row is not one-hot) : the targets"
      const std::vector<Utterance> u = LmTrainingUtterances({{3, 1, 2}, {}, {5}}, std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
      std::cout << "OK " << u.size() << "\n";
      for (const Utterance &x : u) {
        std::cout << x.num_frames << " " << x.dim << " :";
        for (int32 p = 0; p < x.num_frames; p++) {
          int32 hot = -1, ones = 0, others = 0;
          for (int32 c = 0; c < x.dim; c++) {
            const BaseFloat v = x.feats[(size_t)p * x.dim + c];
            if (v == 1.f) { hot = c; ones++; } else if (v != 0.f) others++;
          }
          std::cout << " " << (ones == 1 && others == 0 ? hot : -1);
        }
        std::cout << " :";
        for (int32 t : x.targets) std::cout << " " << t;
        std::cout << " : " << x.feats.size() << " " << x.labels.size() << "\n";
      }
    } else {
      std::cerr << "usage: ctc_nlm_test rescore <model> <lists> <dump> <E> <T> <K> <bos> <eos> <am_scale> <nlm_scale> <unit_bonus> | decode <epochs> | utterances <V> <bos> <eos>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
