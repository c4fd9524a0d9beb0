// tests/cpp/ctc_rescore_test.cpp -- drives CtcRescorer and CtcWordTable behind a CtcBeamDecoder and DecodeCtcWholeUtterances with
// DecodeCtcOptions::rescorer (include/klstm_nnet.hpp) for tests/test_ctc_rescore_gpu.py: train the pattern task briefly (the lists are
// to differ), decode with a fused bigram, rescore every minibatch over tokens and over words, cross-check the loop with and without
// the option, and dump the models, the table and per minibatch the search's device arrays with what the two rescorers made of them.
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
static void put(std::ofstream &f, int32 v) { f.write(reinterpret_cast<const char *>(&v), sizeof(v)); }
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
static LstmProjectedStreams *new_lstm(int32 in, int32 cell, int32 out, int32 streams) {
  std::unique_ptr<LstmProjectedStreams> c(new LstmProjectedStreams(in, out));
  std::ostringstream cfg;
  cfg << "<CellDim> " << cell << " <NumStream> " << streams << " <ParamScale> 0.1";
  std::istringstream is(cfg.str());
  c->InitData(is);
  return c.release();
}
// a full bigram without back-offs over the classes other than `blank`: state 0 the start, state c after the class c; weights and
// final weights seeded.  With one state: a unigram.
static SparseLabelLm seeded_lm(int32 classes, int32 blank, bool bigram, unsigned seed) {
  SparseLabelLm m;
  m.num_classes = classes;
  const int32 Q = bigram ? classes : 1;
  unsigned s = seed;
  m.arc_offsets.push_back(0);
  for (int32 q = 0; q < Q; q++) {
    for (int32 c = 0; c < classes; c++) {
      if (c == blank) continue;
      m.arc_labels.push_back(c);
      m.arc_next.push_back(bigram ? c : 0);
      m.arc_weight.push_back(0.02f + 0.9f * (float)(lcg(&s) % 1000u) / 1000.f);
    }
    m.arc_offsets.push_back((int32)m.arc_labels.size());
    m.backoff.push_back(-1);
    m.backoff_weight.push_back(1.f);
    m.final_weight.push_back(0.1f + 0.8f * (float)(lcg(&s) % 1000u) / 1000.f);
  }
  return m;
}
static void put_lm(std::ofstream &f, const SparseLabelLm &m, int32 blank) {
  put(f, m.NumStates()); put(f, (int32)m.arc_labels.size()); put(f, m.num_classes); put(f, blank);
  put(f, m.arc_offsets); put(f, m.arc_labels); put(f, m.arc_next); put(f, m.arc_weight); put(f, m.backoff); put(f, m.backoff_weight);
  put(f, m.final_weight);
}
static void put_rescorer(std::ofstream &f, const CtcRescorer &r, int32 S, int32 N, int32 T) {
  std::vector<int32> order, live, units, oov;
  std::vector<BaseFloat> score, alp, slp;
  r.Order(&order, &live);
  r.Entries(&score, &alp, &slp, &units, &oov);
  const CtcNbestDevice o = r.DeviceLists();
  put(f, order); put(f, live); put(f, score); put(f, alp); put(f, slp); put(f, units); put(f, oov);
  put(f, down(o.count, S)); put(f, down(o.hyp_len, (size_t)S * N)); put(f, down(o.score, (size_t)S * N)); put(f, down(o.errors, (size_t)S * N));
  put(f, down(o.hyp, (size_t)S * N * T));
}
// everything of the statistics but the wall clock
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

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "run" && argc == 4) {
      // run <epochs> <dump>      GPU.  The dump, in 4-byte words: K; the models sub, add, word (states, arcs, classes, blank, offsets,
      // labels, next, weight, back-off, back-off weight, final); the table (W, keys as pairs of words, ids, unk, separator); then per
      // minibatch T, S, N, the search's count [S], hyp_len, score, errors [S*N], hyp [S*N*T], and for the token and the word rescorer
      // order [S*N], live [S], score, add_logp, sub_logp, units, oov [S*N], out count [S], len, score, errors [S*N], hyp [S*N*T].
      const int32 S = 4, K = 6, N = 4, sep = 1, epochs = std::atoi(argv[2]);
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
      nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      AffineLayer *aff = new AffineLayer(16, K);
      std::vector<BaseFloat> w((size_t)K * 16), bias(K, 0.f);
      for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
      aff->SetParams(w, bias);
      nnet.AppendComponent(aff);
      nnet.AppendComponent(new SoftmaxLayer(K, K));
      for (int32 e = 0; e < epochs; e++) TrainCtcWholeUtterances(&nnet, utts, o);

      // the models: a token bigram fused into the search, another one for the second pass, and a word unigram over a vocabulary of
      // four words (class 4 for unknown words, class 5 reserved)
      const int32 V = 6, unk = 4, reserved = 5;
      const SparseLabelLm h_sub = seeded_lm(K, 0, true, 11u), h_add = seeded_lm(K, 0, true, 23u), h_word = seeded_lm(V, reserved, false, 37u);
      const CtcSparseLabelLm sub(h_sub, 0), add(h_add, 0), word(h_word, reserved);
      const std::vector<std::vector<int32> > vocab = {{2}, {3}, {2, 3}, {4, 5}};
      const CtcWordTable table(vocab, sep, unk);

      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      d.beam = 8; d.cands = 5; d.nbest = N;
      d.slm = &sub;
      // the loop without the option; then with a rescorer that puts back what it takes out: the same answers
      std::vector<std::vector<int32> > best, best_id, best_tok;
      std::vector<CtcNbestList> lists, lists_id, lists_tok;
      std::string rep, rep_id, rep_tok;
      const DecodeCtcStats plain = DecodeCtcWholeUtterances(&nnet, utts, d, &best, &lists, &rep);
      const bool off_zero = plain.first_pass_token_error_rate == 0 && plain.rescored_token_error_rate == 0 && plain.num_changed_1best == 0 &&
                            rep.find("RESCORED") == std::string::npos;
      bool heads = best.size() == utts.size();
      for (size_t i = 0; i < utts.size() && heads; i++) heads = !lists[i].empty() && best[i] == lists[i][0].tokens;
      CtcRescorer identity(K, &sub, &sub);
      DecodeCtcOptions did = d;
      did.rescorer = &identity;
      const DecodeCtcStats sid = DecodeCtcWholeUtterances(&nnet, utts, did, &best_id, &lists_id, &rep_id);
      DecodeCtcStats tid = sid;
      tid.first_pass_token_error_rate = tid.rescored_token_error_rate = tid.num_changed_1best = 0;
      bool identity_same = best_id == best && same_stats(tid, plain) && sid.num_changed_1best == 0 &&
                           sid.first_pass_token_error_rate == plain.token_error_rate && sid.rescored_token_error_rate == plain.token_error_rate;
      for (size_t i = 0; i < lists.size() && identity_same; i++) {
        identity_same = lists[i].size() == lists_id[i].size();
        for (size_t q = 0; q < lists[i].size() && identity_same; q++)
          identity_same = lists[i][q].tokens == lists_id[i][q].tokens && lists[i][q].errors == lists_id[i][q].errors;
      }

      // the second pass proper: tokens in the loop, with a consensus behind it; words by a rescorer of our own in every_batch
      std::ofstream f(argv[3], std::ios::binary);
      put(f, K);
      put_lm(f, h_sub, 0); put_lm(f, h_add, 0); put_lm(f, h_word, reserved);
      put(f, table.NumWords());
      f.write(reinterpret_cast<const char *>(table.Keys().data()), table.Keys().size() * sizeof(uint64_t));
      put(f, table.Ids()); put(f, unk); put(f, sep);
      CtcRescorer tok(K, &add, &sub, nullptr, -1, 1.f, 0.8f, 0.25f), wrd(K, &word, &sub, &table, reserved, 1.f, 0.5f, 0.f);
      DecodeCtcOptions dt = d;
      dt.rescorer = &tok;
      dt.consensus = 1;
      int32 mb = 0;
      bool lists_match = true;
      std::vector<std::vector<BaseFloat> > conf;
      const DecodeCtcStats st = DecodeCtcWholeUtterances(&nnet, utts, dt, &best_tok, &lists_tok, &conf, &rep_tok,
          [&](const UtteranceBatch &b, const DeviceMatrix &, const CtcBeamDecoder &dec) {
            wrd.Eval(dec);
            mb++;
            const CtcNbestDevice nb = dec.DeviceLists();
            const int32 T = nb.stride;
            put(f, T); put(f, b.num_stream); put(f, N);
            put(f, down(nb.count, b.num_stream)); put(f, down(nb.hyp_len, (size_t)b.num_stream * N)); put(f, down(nb.score, (size_t)b.num_stream * N));
            put(f, down(nb.errors, (size_t)b.num_stream * N)); put(f, down(nb.hyp, (size_t)b.num_stream * N * T));
            put_rescorer(f, tok, b.num_stream, N, T);
            put_rescorer(f, wrd, b.num_stream, N, T);
            std::vector<CtcNbestList> mine;
            tok.Lists(&mine);
            for (int32 s = 0; s < b.num_stream; s++) {
              if (b.utt_index[s] < 0) continue;
              const CtcNbestList &l = lists_tok[b.utt_index[s]];
              lists_match = lists_match && l.size() == mine[s].size();
              for (size_t q = 0; q < l.size() && lists_match; q++) lists_match = l[q].tokens == mine[s][q].tokens;
            }
          });
      f.close();
      bool heads_tok = best_tok.size() == utts.size(), conf_ok = true;
      for (size_t i = 0; i < utts.size(); i++) {
        heads_tok = heads_tok && !lists_tok[i].empty() && best_tok[i] == lists_tok[i][0].tokens;      // consensus 1: the head of the re-ranked list
        conf_ok = conf_ok && conf[i].size() == best_tok[i].size();
      }
      double new_errors = 0;
      for (size_t i = 0; i < utts.size(); i++) new_errors += lists_tok[i].empty() ? 0 : lists_tok[i][0].errors;
      const bool rates_ok = st.first_pass_token_error_rate == plain.token_error_rate && st.token_error_rate == plain.token_error_rate &&
                            st.rescored_token_error_rate == new_errors / plain.num_ref_tokens && st.num_changed_1best == tok.NumChanged();
      std::cerr << rep_tok << "\n" << wrd.Report();
      std::cout.precision(17);
      std::cout << "OK off_zero=" << (int)off_zero << " heads=" << (int)heads << " identity_same=" << (int)identity_same
                << " lists_match=" << (int)lists_match << " heads_tok=" << (int)heads_tok << " conf_ok=" << (int)conf_ok << " rates_ok=" << (int)rates_ok
                << " minibatches=" << mb << " changed=" << st.num_changed_1best << " first_ter=" << st.first_pass_token_error_rate
                << " rescored_ter=" << st.rescored_token_error_rate << " tok_utts=" << (int)tok.NumUtterances() << " wrd_utts=" << (int)wrd.NumUtterances()
                << " wrd_oov=" << (int)wrd.NumOovWords() << " tok_first_errors=" << tok.NumFirstPassErrors() << " tok_rescored_errors=" << tok.NumRescoredErrors()
                << " wrd_changed=" << wrd.NumChanged()
                << " has_report=" << (int)(rep_tok.find("RESCORED") != std::string::npos && rep_tok.find("EXPECTED_ERRORS") != std::string::npos) << "\n";
    } else {
      std::cerr << "usage: ctc_rescore_test run <epochs> <dump>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
