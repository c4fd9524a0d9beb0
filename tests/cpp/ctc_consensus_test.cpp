// tests/cpp/ctc_consensus_test.cpp -- drives CtcConsensus behind a CtcBeamDecoder and DecodeCtcWholeUtterances with
// DecodeCtcOptions::consensus in {0, 1, 2} (include/klstm_nnet.hpp) for tests/test_ctc_consensus_gpu.py: train the pattern task
// briefly (the lists are to differ), decode, cross-check, and dump two minibatches' lists with what the consensus made of them.
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
// everything of the statistics but the wall clock
static bool same_stats(const DecodeCtcStats &a, const DecodeCtcStats &b) {
  const double x[] = {a.token_error_rate, a.utt_error_rate, a.num_scored, a.num_errors, a.num_ref_tokens, a.oracle_token_error_rate,
                      a.expected_errors, a.map_expected_errors, a.mean_confidence, a.num_pick_errors};
  const double y[] = {b.token_error_rate, b.utt_error_rate, b.num_scored, b.num_errors, b.num_ref_tokens, b.oracle_token_error_rate,
                      b.expected_errors, b.map_expected_errors, b.mean_confidence, b.num_pick_errors};
  return a.num_done == b.num_done && a.num_skipped == b.num_skipped && a.num_minibatches == b.num_minibatches &&
         std::memcmp(x, y, sizeof(x)) == 0;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "run" && argc == 4) {
      // run <epochs> <dump>      GPU.  Per dumped minibatch: T, S, N; count [S], hyp_len [S*N], score [S*N], errors [S*N], hyp [S*N*T],
      // then pick, map, mbr [S], the number of confidences per stream [S] and the confidences back to back, the risk of the pick [S].
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
      nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      AffineLayer *aff = new AffineLayer(16, K);
      std::vector<BaseFloat> w((size_t)K * 16), bias(K, 0.f);
      for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
      aff->SetParams(w, bias);
      nnet.AppendComponent(aff);
      nnet.AppendComponent(new SoftmaxLayer(K, K));
      for (int32 e = 0; e < epochs; e++) TrainCtcWholeUtterances(&nnet, utts, o);

      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      d.beam = 8; d.cands = 5; d.nbest = N;
      // the search as it was: the overload without confidences, and consensus = 0 through the one with them
      std::vector<std::vector<int32> > best, best0, hyp1, hyp2;
      std::vector<CtcNbestList> lists, lists0, lists2;
      std::vector<std::vector<BaseFloat> > conf0, conf1, conf2;
      std::string rep, rep0, rep1, rep2;
      const DecodeCtcStats plain = DecodeCtcWholeUtterances(&nnet, utts, d, &best, &lists, &rep);
      const DecodeCtcStats s0 = DecodeCtcWholeUtterances(&nnet, utts, d, &best0, &lists0, &conf0, &rep0);
      bool off_same = best0 == best && same_stats(s0, plain) && rep0 == rep && lists0.size() == lists.size();
      for (size_t i = 0; i < lists.size() && off_same; i++) {
        off_same = lists[i].size() == lists0[i].size() && conf0[i].empty();
        for (size_t q = 0; q < lists[i].size() && off_same; q++)
          off_same = lists[i][q].tokens == lists0[i][q].tokens && std::memcmp(&lists[i][q].score, &lists0[i][q].score, sizeof(BaseFloat)) == 0 &&
                     lists[i][q].errors == lists0[i][q].errors;
      }
      // the MAP entry with confidences, then the MBR entry; a CtcConsensus of our own behind the decoder of the second pass, dumped
      DecodeCtcOptions d1 = d, d2 = d;
      d1.consensus = 1;
      d2.consensus = 2;
      const DecodeCtcStats s1 = DecodeCtcWholeUtterances(&nnet, utts, d1, &hyp1, nullptr, &conf1, &rep1);
      CtcConsensus cons(true);
      std::ofstream f(argv[3], std::ios::binary);
      int32 mb = 0;
      const DecodeCtcStats s2 = DecodeCtcWholeUtterances(&nnet, utts, d2, &hyp2, &lists2, &conf2, &rep2,
          [&](const UtteranceBatch &b, const DeviceMatrix &, const CtcBeamDecoder &dec) {
            cons.Eval(dec);
            mb++;
            const int32 T = b.num_frames;
            std::vector<BaseFloat> score((size_t)b.num_stream * N, 0.f);
            std::vector<int32> cnt, hlen((size_t)b.num_stream * N, 0), err((size_t)b.num_stream * N, -1), hyp((size_t)b.num_stream * N * T, -1);
            for (int32 s = 0; s < b.num_stream; s++) {
              const CtcNbestList &l = b.utt_index[s] >= 0 ? lists2[b.utt_index[s]] : CtcNbestList();
              cnt.push_back((int32)l.size());
              for (size_t q = 0; q < l.size(); q++) {
                hlen[(size_t)s * N + q] = (int32)l[q].tokens.size();
                score[(size_t)s * N + q] = l[q].score;
                err[(size_t)s * N + q] = l[q].errors;
                std::copy(l[q].tokens.begin(), l[q].tokens.end(), hyp.begin() + ((size_t)s * N + q) * T);
              }
            }
            std::vector<int32> pick, map, mbr, nconf;
            std::vector<std::vector<BaseFloat> > conf;
            std::vector<BaseFloat> flat, risk;
            cons.Picks(&pick, &map, &mbr);
            cons.Confidences(&conf, &risk);
            for (const auto &c : conf) { nconf.push_back((int32)c.size()); flat.insert(flat.end(), c.begin(), c.end()); }
            put(f, T); put(f, b.num_stream); put(f, N);
            put(f, cnt); put(f, hlen); put(f, score); put(f, err); put(f, hyp);
            put(f, pick); put(f, map); put(f, mbr); put(f, nconf); put(f, (int32)flat.size()); put(f, flat); put(f, risk);
          });
      f.close();
      bool map_ok = hyp1.size() == utts.size(), mbr_ok = hyp2.size() == utts.size(), conf_ok = true;
      for (size_t i = 0; i < utts.size(); i++) {
        map_ok = map_ok && !lists[i].empty() && hyp1[i] == lists[i][0].tokens;          // the scores descend: the MAP entry is the head
        bool in_list = false;
        for (const auto &h : lists[i]) in_list = in_list || h.tokens == hyp2[i];
        mbr_ok = mbr_ok && in_list;
        conf_ok = conf_ok && conf1[i].size() == hyp1[i].size() && conf2[i].size() == hyp2[i].size();
        for (BaseFloat c : conf1[i]) conf_ok = conf_ok && c > 0.f && c <= 1.f;
        for (BaseFloat c : conf2[i]) conf_ok = conf_ok && c > 0.f && c <= 1.f;
      }
      // the search's own figures do not move with the option; the MAP entry's expected errors are one number however it is reached
      DecodeCtcStats t1 = s1, t2 = s2;
      t1.expected_errors = t1.map_expected_errors = t1.mean_confidence = t1.num_pick_errors = 0;
      t2.expected_errors = t2.map_expected_errors = t2.mean_confidence = t2.num_pick_errors = 0;
      const bool search_same = same_stats(t1, plain) && same_stats(t2, plain);
      const bool map_risk_same = s1.expected_errors == s1.map_expected_errors && s1.map_expected_errors == s2.map_expected_errors &&
                                 s1.num_pick_errors == plain.num_errors;
      std::cerr << rep2 << "\n" << cons.Report();
      std::cout.precision(17);
      std::cout << "OK off_same=" << (int)off_same << " map_ok=" << (int)map_ok << " mbr_ok=" << (int)mbr_ok << " conf_ok=" << (int)conf_ok
                << " search_same=" << (int)search_same << " map_risk_same=" << (int)map_risk_same << " minibatches=" << mb
                << " expected_map=" << s1.expected_errors << " expected_mbr=" << s2.expected_errors << " mean_conf_map=" << s1.mean_confidence
                << " mean_conf_mbr=" << s2.mean_confidence << " own_expected=" << cons.ExpectedErrors() << " own_map_expected=" << cons.MapExpectedErrors()
                << " own_mean_conf=" << cons.MeanConfidence() << " own_utts=" << (int)cons.NumUtterances() << " pick_errors=" << (int)s2.num_pick_errors
                << " ter=" << plain.token_error_rate << " has_report=" << (int)(rep2.find("EXPECTED_ERRORS") != std::string::npos && rep0.find("EXPECTED_ERRORS") == std::string::npos)
                << "\n";
    } else {
      std::cerr << "usage: ctc_consensus_test run <epochs> <dump>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
