// tests/cpp/ctc_test.cpp -- drives WholeUtteranceBatcher (include/klstm_trainer.hpp; host only) and Ctc / TrainCtcWholeUtterances
// (include/klstm_nnet.hpp; GPU) for tests/test_ctc.py and tests/test_ctc_gpu.py; on the GPU also the pieces the CTC classes are built from
// (DeviceBuffer, DeviceTotals) and one object of each class through calls of changing shape.
#include <cmath>
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

// ---- the reuse check: one call of every CTC class on seeded posteriors, everything a stream gets out of it as raw bytes ----
struct ReuseCase {
  int32 T, S;
  std::vector<int32> lens;
  std::vector<std::vector<int32> > labels;
};
template <class T>
static void append(std::string *bytes, const std::vector<T> &v) { bytes->append(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T)); }
static void append(std::string *bytes, const std::vector<std::vector<int32> > &v) {
  for (const auto &l : v) { const std::vector<int32> n(1, (int32)l.size()); append(bytes, n); append(bytes, l); }
}
// seeded softmax rows [T*S x K]
static void fill_posteriors(unsigned seed, int32 rows, int32 K, DeviceMatrix *y) {
  unsigned s = seed * 2654435761u + 99u;
  std::vector<BaseFloat> h((size_t)rows * K);
  for (int32 r = 0; r < rows; r++) {
    double sum = 0;
    for (int32 k = 0; k < K; k++) sum += h[(size_t)r * K + k] = std::exp(3.f * (float)(lcg(&s) % 1000u) / 1000.f);
    for (int32 k = 0; k < K; k++) h[(size_t)r * K + k] = (BaseFloat)(h[(size_t)r * K + k] / sum);
  }
  y->CopyFromHost(h.data(), rows, K);
}
struct ReuseObjects {
  Ctc ctc;
  CtcGreedyDecoder greedy;
  CtcBeamDecoder beam{0, 4, 2, 2};
  CtcAligner aligner;
};
// sums[]: what the totals of the four objects grow by in this call, from the per-stream outputs
static std::string reuse_call(ReuseObjects *o, const ReuseCase &c, const DeviceMatrix &y, double *sums) {
  std::string out;
  DeviceMatrix diff;
  std::vector<BaseFloat> f, d;
  std::vector<int32> a, b;
  std::vector<std::vector<int32> > u, v;
  o->ctc.Eval(y, c.S, c.lens, c.labels, &diff);
  o->ctc.UttLoss(&f); diff.CopyToHost(&d);
  append(&out, f); append(&out, d);
  for (int32 s = 0; s < c.S; s++) if (c.lens[s] > 0 && std::isfinite(f[s])) sums[0] += (double)f[s];
  o->greedy.Decode(y, c.S, c.lens, c.labels, &u);
  o->greedy.UttScores(&f); o->greedy.UttErrors(&a); o->greedy.FrameClasses(&b);
  append(&out, u); append(&out, f); append(&out, a); append(&out, b);
  for (int32 s = 0; s < c.S; s++) if (a[s] > 0) sums[1] += 1;
  std::vector<CtcNbestList> lists;
  o->beam.Decode(y, c.S, c.lens, c.labels, &lists);
  for (const auto &l : lists)
    for (const auto &h : l) { append(&out, h.tokens); append(&out, std::vector<BaseFloat>(1, h.score)); append(&out, std::vector<int32>(1, h.errors)); }
  o->beam.NbestCounts(&a); append(&out, a);
  o->beam.UttScores(&f); append(&out, f);
  o->beam.UttErrors(&a); append(&out, a);
  for (int32 s = 0; s < c.S; s++) if (a[s] > 0) sums[2] += 1;
  o->aligner.Align(y, c.S, c.lens, c.labels);
  o->aligner.FrameClasses(&a); o->aligner.FramePositions(&b); o->aligner.TokenBounds(&u, &v); o->aligner.UttScores(&f);
  append(&out, a); append(&out, b); append(&out, u); append(&out, v); append(&out, f);
  for (int32 s = 0; s < c.S; s++) {
    if (c.lens[s] <= 0 || !std::isfinite(f[s])) continue;
    sums[3] += (double)f[s];
    for (int32 t = 0; t < c.lens[s]; t++) sums[4] += a[(size_t)t * c.S + s] == 0;
  }
  return out;
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
    } else if (mode == "buffers" && argc == 2) {
      // buffers      GPU.  The contracts of DeviceBuffer and DeviceTotals (include/klstm_nnet.hpp), one key=0/1 each
      DeviceBuffer a;
      a.Grow(100);
      const void *p = a.As<void>();
      a.Grow(50);
      const bool keeps = p && a.As<void>() == p && a.Capacity() >= 100;
      a.Grow(200);
      const bool grows = a.As<void>() && a.Capacity() >= 200;
      const void *q = a.As<void>();
      DeviceBuffer b(std::move(a));
      const bool moved = !a.As<void>() && a.Capacity() == 0 && b.As<void>() == q && b.Capacity() >= 200;
      DeviceBuffer c;
      c.Grow(16);
      c = std::move(b);
      const bool assigned = !b.As<void>() && b.Capacity() == 0 && c.As<void>() == q && c.Capacity() >= 200;
      DeviceBuffer e;
      int32 x = 7;
      e.Upload(std::vector<int32>());
      e.Download(&x, 0);
      const bool empty = !e.As<void>() && e.Capacity() == 0 && x == 7;
      std::vector<int32> five = {1, 2, 3, 4, 5}, back(5, 0);
      c.Upload(five);                                                       // fits: the block stays
      c.Download(back.data(), back.size());
      const bool round_trip = back == five && c.As<void>() == q;
      DeviceTotals<4> t;
      const double *h = t.Read();
      bool untouched = h[0] == 0 && h[1] == 0 && h[2] == 0 && h[3] == 0;
      KLSTM_ASSERT(t.Dev() != nullptr && t.Dev() == t.Dev());
      h = t.Read();
      untouched = untouched && h[0] == 0 && h[1] == 0 && h[2] == 0 && h[3] == 0;
      DeviceMatrix y, diff;                                                 // one call that adds to a totals block, read twice
      fill_posteriors(1, 12, 5, &y);
      Ctc ctc;
      ctc.Eval(y, 2, std::vector<int32>{6, 5}, std::vector<std::vector<int32> >{{1, 2}, {3}}, &diff);
      const double r1[4] = {ctc.AvgLoss(), ctc.NumUtterances(), ctc.NumRejected(), ctc.Frames()};
      const double r2[4] = {ctc.AvgLoss(), ctc.NumUtterances(), ctc.NumRejected(), ctc.Frames()};
      const bool twice = std::memcmp(r1, r2, sizeof(r1)) == 0 && r1[1] == 2 && r1[2] == 0 && r1[3] == 11 && std::isfinite(r1[0]) && r1[0] > 0;
      std::cout << "OK grow_smaller_keeps_pointer=" << keeps << " grow_larger_has_capacity=" << grows << " moved_from_is_empty=" << moved
                << " move_assigned_from_is_empty=" << assigned << " empty_upload_download_do_nothing=" << empty << " round_trip=" << round_trip
                << " untouched_totals_are_zero=" << untouched << " totals_read_twice_agree=" << twice << "\n";
    } else if (mode == "reuse" && argc == 2) {
      // reuse      GPU.  One object each of Ctc, CtcGreedyDecoder, CtcBeamDecoder (beam 4, 2 candidates, 2-best) and CtcAligner through three
      // calls, K = 5, blank 0: (T 6, S 2), (T 12, S 3) with stream 1 idle, (T 6, S 2) again -- the buffers grow, then are larger than
      // needed.  same<i>: every per-stream output of call i has the bits a fresh set of objects gives; totals: the reused objects'
      // totals are the three fresh ones added up.
      const int32 K = 5;
      const ReuseCase cases[3] = {{6, 2, {6, 4}, {{1, 2, 3}, {}}},
                                  {12, 3, {12, 0, 9}, {{4, 4, 1}, {2}, {3, 1}}},
                                  {6, 2, {5, 6}, {{2}, {1, 1, 3}}}};
      ReuseObjects reused;
      double want[5] = {0, 0, 0, 0, 0}, ignore[5];
      bool same[3], fresh_totals = true;
      double ctc_n = 0, ctc_rej = 0, ctc_frames = 0, g[5] = {0, 0, 0, 0, 0}, bm[6] = {0, 0, 0, 0, 0, 0}, al[3] = {0, 0, 0};
      for (int32 i = 0; i < 3; i++) {
        const ReuseCase &c = cases[i];
        DeviceMatrix y;
        fill_posteriors(10 + i, c.T * c.S, K, &y);
        ReuseObjects fresh;
        const std::string a = reuse_call(&reused, c, y, ignore), b = reuse_call(&fresh, c, y, want);
        same[i] = !a.empty() && a == b;
        ctc_n += fresh.ctc.NumUtterances(); ctc_rej += fresh.ctc.NumRejected(); ctc_frames += fresh.ctc.Frames();
        g[0] += fresh.greedy.NumErrors(); g[1] += fresh.greedy.NumRefTokens(); g[2] += fresh.greedy.NumHypTokens(); g[3] += fresh.greedy.NumUtterances();
        bm[0] += fresh.beam.NumErrors(); bm[1] += fresh.beam.NumRefTokens(); bm[2] += fresh.beam.NumHypTokens(); bm[3] += fresh.beam.NumUtterances();
        bm[5] += fresh.beam.NumOracleErrors();
        al[0] += fresh.aligner.NumAligned(); al[1] += fresh.aligner.NumRejected(); al[2] += fresh.aligner.Frames();
        fresh_totals = fresh_totals && fresh.ctc.NumUtterances() > 0 && fresh.greedy.NumRefTokens() > 0 && fresh.aligner.Frames() > 0;
      }
      const bool totals =
          reused.ctc.NumUtterances() == ctc_n && reused.ctc.NumRejected() == ctc_rej && reused.ctc.Frames() == ctc_frames &&
          reused.ctc.AvgLoss() == want[0] / ctc_n && reused.ctc.AvgLossPerFrame() == want[0] / ctc_frames &&
          reused.greedy.NumErrors() == g[0] && reused.greedy.NumRefTokens() == g[1] && reused.greedy.NumHypTokens() == g[2] &&
          reused.greedy.NumUtterances() == g[3] && reused.greedy.UtteranceErrorRate() == want[1] / g[3] &&
          reused.beam.NumErrors() == bm[0] && reused.beam.NumRefTokens() == bm[1] && reused.beam.NumHypTokens() == bm[2] &&
          reused.beam.NumUtterances() == bm[3] && reused.beam.NumOracleErrors() == bm[5] && reused.beam.UtteranceErrorRate() == want[2] / bm[3] &&
          reused.aligner.NumAligned() == al[0] && reused.aligner.NumRejected() == al[1] && reused.aligner.Frames() == al[2] &&
          reused.aligner.AvgScorePerFrame() == want[3] / al[2] && reused.aligner.BlankRatio() == want[4] / al[2];
      std::cout << "OK same0=" << same[0] << " same1=" << same[1] << " same2=" << same[2] << " totals=" << totals << " fresh_totals_counted="
                << fresh_totals << " utterances=" << ctc_n << " frames=" << ctc_frames << " ref_tokens=" << g[1] << " aligned=" << al[0] << "\n";
    } else {
      std::cerr << "usage: ctc_test batcher <streams> <sort> <max_frames> <lens> <out> | train <blstm|lstm> <dump> | buffers | reuse\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
