// tests/cpp/ctc_beam_stream_test.cpp -- drives CtcStreamDecoder (include/klstm_nnet.hpp), BatchScorer::ForEachChunk and DecodeCtcStreaming
// (include/klstm_scorer.hpp) for tests/test_ctc_beam_stream.py (the refusals, host only) and tests/test_ctc_beam_stream_gpu.py (the
// pattern task of the sibling drivers, streamed at two chunk sizes and compared with the whole-utterance decoders).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>

#include "../../include/klstm_blstm.hpp"
#include "../../include/klstm_scorer.hpp"

using namespace klstm_kaldi;

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
static void add_output(Nnet *nnet, int32 H, int32 K) {
  AffineLayer *aff = new AffineLayer(H, K);
  std::vector<BaseFloat> w((size_t)K * H), bias(K, 0.f);
  for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
  aff->SetParams(w, bias);
  nnet->AppendComponent(aff);
  nnet->AppendComponent(new SoftmaxLayer(K, K));
}
static bool same_lists(const std::vector<CtcNbestList> &a, const std::vector<CtcNbestList> &b, bool scores) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    if (a[i].size() != b[i].size()) return false;
    for (size_t q = 0; q < a[i].size(); q++) {
      if (a[i][q].tokens != b[i][q].tokens || a[i][q].errors != b[i][q].errors) return false;
      if (scores && std::memcmp(&a[i][q].score, &b[i][q].score, sizeof(BaseFloat)) != 0) return false;
    }
  }
  return true;
}
template <class F>
static std::string refusal(F f) {
  try { f(); } catch (const std::exception &e) { return e.what(); }
  return "";
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "refuse" && argc == 2) {
      // refuse      host only: what DecodeCtcStreaming and CtcStreamDecoder turn down before any device work
      const int32 S = 4, K = 6;
      std::vector<Utterance> utts(1, pattern_utt(1, 4, K));
      Nnet bi, uni;
      bi.AppendComponent(new TransmitLayer(16, 16));
      bi.AppendComponent(new BLstmLayer(new_lstm(16, 32, 16, S), new_lstm(16, 32, 16, S)));
      add_output(&bi, 32, K);
      uni.AppendComponent(new TransmitLayer(16, 16));
      uni.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      add_output(&uni, 16, K);
      BatchScorerOptions so;
      so.num_stream = S; so.chunk = 20;
      DecodeCtcOptions o;
      o.beam = 8; o.cands = 5; o.nbest = 4;
      std::vector<std::vector<int32> > hyp;
      auto run = [&](const Nnet &n, const BatchScorerOptions &s, const DecodeCtcOptions &d) {
        return refusal([&] { DecodeCtcStreaming(n, utts, s, d, &hyp, nullptr); });
      };
      const std::string r_bi = run(bi, so, o);
      DecodeCtcOptions greedy = o;
      greedy.beam = 0;
      const std::string r_beam = run(uni, so, greedy);
      BatchScorerOptions logp = so;
      logp.mode = KLSTM_SCORE_LOGPOST;
      const std::string r_mode = run(uni, logp, o);
      BatchScorerOptions wide = so;
      wide.num_stream = 33;
      const std::string r_wide = run(uni, wide, o);
      const std::string r_state = refusal([&] { CtcStreamDecoder d(0, 64, 8, 1, 4, (1 << 25) + 1); });      // frames * beam + 1 >= 2^31
      const std::string r_beam65 = refusal([&] { CtcStreamDecoder d(0, 65, 8, 1, 4, 100); });
      const bool ok = r_bi.find("bidirectional") != std::string::npos && r_beam.find("beam must be positive") != std::string::npos &&
                      r_mode.find("posteriors") != std::string::npos && r_wide.find("> 32") != std::string::npos &&
                      r_state.find("2^31") != std::string::npos && r_beam65.find("beam") != std::string::npos;
      std::cerr << r_bi << "\n" << r_beam << "\n" << r_mode << "\n" << r_wide << "\n" << r_state << "\n" << r_beam65 << "\n";
      std::cout << (ok ? "OK" : "FAILED") << " refused=" << (int)ok << "\n";
      return ok ? 0 : 1;
    } else if (mode == "stream" && argc == 4) {
      // stream <chunk a> <chunk b>      GPU.  Train the unidirectional net of ctc_beam_test's train mode, then decode (beam 8, 5
      // candidates, 4-best): DecodeCtcWholeUtterances; DecodeCtcStreaming at both chunk sizes; and a CtcBeamDecoder on the posteriors
      // that BatchScorer::ForEachChunk hands out, S utterances a call -- the streaming lists must equal those bit for bit.  Between the two
      // chunk sizes, and against DecodeCtcWholeUtterances, the forward pass may round differently (other launch plans): tokens, edit
      // distances and statistics are compared, the score bits only reported (whole_bits, chunkings_bits).
      const int32 S = 4, K = 6, N = 4;
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
      nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      nnet.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      add_output(&nnet, 16, K);
      for (int32 e = 0; e < 150; e++) TrainCtcWholeUtterances(&nnet, utts, o);

      DecodeCtcOptions bo;
      bo.num_stream = S; bo.max_frames = o.max_frames; bo.beam = 8; bo.cands = 5; bo.nbest = N;
      std::vector<std::vector<int32> > best_w;
      std::vector<CtcNbestList> lists_w;
      const DecodeCtcStats sw = DecodeCtcWholeUtterances(&nnet, utts, bo, &best_w, &lists_w);

      bool captured_same = true, stats_same = true, whole_same = true, whole_bits = true, chunkings_same = true, chunkings_bits = true;
      std::vector<CtcNbestList> first;
      int32 chunks = 0;
      for (int a = 2; a < 4; a++) {
        BatchScorerOptions so;
        so.num_stream = S; so.chunk = std::atoi(argv[a]);
        std::vector<std::vector<int32> > best_s;
        std::vector<CtcNbestList> lists_s;
        std::string report;
        const DecodeCtcStats ss = DecodeCtcStreaming(nnet, utts, so, bo, &best_s, &lists_s, &report);
        chunks += ss.num_minibatches;
        // the posteriors the stream decoder saw, per utterance
        std::vector<int32> lens(utts.size(), 0);
        std::vector<BaseFloat> cat;
        for (size_t u = 0; u < utts.size(); u++)
          if (utts[u].num_frames <= o.max_frames) { lens[u] = utts[u].num_frames; cat.insert(cat.end(), utts[u].feats.begin(), utts[u].feats.end()); }
        DeviceMatrix feats;
        feats.CopyFromHost(cat.data(), (int32)(cat.size() / 16), 16);
        std::vector<std::vector<BaseFloat> > post(utts.size());
        BatchScorer scorer(nnet, so);
        scorer.ForEachChunk(feats.View().Data(), feats.Stride(), lens, [&](const DeviceMatrix &y, const BatchScorer::ChunkInfo &info) {
          std::vector<BaseFloat> h;
          y.CopyToHost(&h);
          for (int32 s = 0; s < S; s++)
            for (int32 t = 0; t < info.frames[s]; t++)
              post[info.utt[s]].insert(post[info.utt[s]].end(), h.begin() + ((size_t)t * S + s) * K, h.begin() + ((size_t)t * S + s + 1) * K);
        });
        CtcBeamDecoder dec(bo.blank, bo.beam, bo.cands, N);
        std::vector<CtcNbestList> lists_c(utts.size());
        std::vector<int32> kept;
        for (size_t u = 0; u < utts.size(); u++) if (lens[u]) kept.push_back((int32)u);
        for (size_t g = 0; g < kept.size(); g += S) {
          int32 T = 1;
          std::vector<int32> bl(S, 0);
          std::vector<std::vector<int32> > refs(S);
          for (int32 s = 0; s < S && g + s < kept.size(); s++) { bl[s] = lens[kept[g + s]]; T = std::max(T, bl[s]); refs[s] = utts[kept[g + s]].labels; }
          std::vector<BaseFloat> yb((size_t)T * S * K, 0.f);
          for (int32 s = 0; s < S && g + s < kept.size(); s++)
            for (int32 t = 0; t < bl[s]; t++)
              std::copy(post[kept[g + s]].begin() + (size_t)t * K, post[kept[g + s]].begin() + (size_t)(t + 1) * K, yb.begin() + ((size_t)t * S + s) * K);
          DeviceMatrix y;
          y.CopyFromHost(yb.data(), T * S, K);
          std::vector<CtcNbestList> l;
          dec.Decode(y, S, bl, refs, &l);
          for (int32 s = 0; s < S && g + s < kept.size(); s++) lists_c[kept[g + s]] = l[s];
        }
        captured_same = captured_same && same_lists(lists_s, lists_c, true);
        for (size_t u = 0; u < utts.size(); u++) captured_same = captured_same && best_s[u] == (lists_c[u].empty() ? std::vector<int32>() : lists_c[u][0].tokens);
        stats_same = stats_same && ss.num_errors == dec.NumErrors() && ss.num_ref_tokens == dec.NumRefTokens() && ss.num_scored == dec.NumUtterances() &&
                     ss.token_error_rate == dec.TokenErrorRate() && ss.utt_error_rate == dec.UtteranceErrorRate() &&
                     ss.oracle_token_error_rate == dec.OracleTokenErrorRate() && ss.num_done == sw.num_done && ss.num_skipped == sw.num_skipped;
        whole_same = whole_same && same_lists(lists_s, lists_w, false) && best_s == best_w && ss.num_errors == sw.num_errors &&
                     ss.num_ref_tokens == sw.num_ref_tokens && ss.num_scored == sw.num_scored && ss.oracle_token_error_rate == sw.oracle_token_error_rate;
        whole_bits = whole_bits && same_lists(lists_s, lists_w, true);
        if (a == 2) first = lists_s; else { chunkings_same = same_lists(first, lists_s, false); chunkings_bits = same_lists(first, lists_s, true); }
        if (a == 2) std::cerr << report << "\n";
      }
      std::cout << "OK captured_same=" << (int)captured_same << " stats_same=" << (int)stats_same << " whole_same=" << (int)whole_same
                << " whole_bits=" << (int)whole_bits << " chunkings_same=" << (int)chunkings_same << " chunkings_bits=" << (int)chunkings_bits << " chunks=" << chunks
                << " ter_whole=" << sw.token_error_rate << " scored=" << (int)sw.num_scored << " skipped=" << sw.num_skipped << "\n";
    } else {
      std::cerr << "usage: ctc_beam_stream_test refuse | stream <chunk a> <chunk b>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
