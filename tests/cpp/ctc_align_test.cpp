// tests/cpp/ctc_align_test.cpp -- drives CtcAligner / AlignCtcWholeUtterances / SetTargetsFromAlignment (include/klstm_nnet.hpp) for
// tests/test_ctc_align.py (host only: alignments in utterance order, the targets bridge) and tests/test_ctc_align_gpu.py (train with
// CTC, align, train a frame-level net on the alignment).
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
// utterance i of the reordering check (tests/test_ctc.plain_utts): dim 3, feats(t, d) = 1000 i + t + d / 4, labels i, i + 1, ... (i % 5)
static Utterance plain_utt(int32 i, int32 frames) {
  Utterance u;
  u.num_frames = frames; u.dim = 3;
  u.feats.resize((size_t)frames * 3);
  for (int32 t = 0; t < frames; t++) for (int32 d = 0; d < 3; d++) u.feats[(size_t)t * 3 + d] = 1000.f * i + t + 0.25f * d;
  for (int32 j = 0; j < i % 5; j++) u.labels.push_back(i + j);
  return u;
}
// the memorisable pattern task of tests/cpp/ctc_decode_test.cpp
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
static AffineLayer *new_affine(int32 in, int32 out) {
  AffineLayer *aff = new AffineLayer(in, out);
  std::vector<BaseFloat> w((size_t)out * in), bias(out, 0.f);
  for (size_t i = 0; i < w.size(); i++) w[i] = (BaseFloat)(((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 0.2);
  aff->SetParams(w, bias);
  return aff;
}
static std::string join(const std::vector<int32> &v) {
  std::ostringstream o;
  for (size_t i = 0; i < v.size(); i++) o << (i ? "," : "") << v[i];
  return o.str();
}
static std::vector<int32> collapse(const std::vector<int32> &path, int32 blank) {
  std::vector<int32> out;
  for (size_t t = 0; t < path.size(); t++)
    if (path[t] != blank && (t == 0 || path[t] != path[t - 1])) out.push_back(path[t]);
  return out;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "order" && argc == 6) {
      // order <streams> <sort 0/1> <max_frames> <len,len,...>      host only.  The batcher's minibatches; every stream gets an alignment
      // made of what it carries (frame 0: 1 + the utterance's number read off its first feature, the other frames blank; token begins:
      // its labels), scattered into utterance order as AlignCtcWholeUtterances does it; then SetTargetsFromAlignment with the blank
      // as 99.  Prints "OK <skipped> <filled>" and per utterance "<targets>;<token begins>" (empty: skipped)
      const int32 S = atoi(argv[2]);
      std::vector<Utterance> utts;
      const std::vector<int32> lens = parse_ints(argv[5]);
      for (size_t i = 0; i < lens.size(); i++) utts.push_back(plain_utt((int32)i, lens[i]));
      WholeUtteranceBatcher batcher(&utts, S, atoi(argv[3]) != 0, atoi(argv[4]));
      std::vector<CtcAlignment> per_utt(utts.size());
      UtteranceBatch b;
      while (batcher.Next(&b)) {
        std::vector<CtcAlignment> per_stream(S);
        for (int32 s = 0; s < S; s++) {
          if (b.lens[s] == 0) continue;
          CtcAlignment &a = per_stream[s];
          a.aligned = true;
          a.frame_class.assign(b.lens[s], 0);
          a.frame_class[0] = 1 + (int32)b.feat[(size_t)s * b.dim] / 1000;
          a.token_begin = b.labels[s];
        }
        ScatterByUtterance(b, per_stream, &per_utt);
      }
      const int32 filled = SetTargetsFromAlignment(&utts, per_utt, 99);
      std::cout << "OK " << batcher.NumSkipped() << " " << filled << "\n";
      for (size_t i = 0; i < utts.size(); i++) std::cout << join(utts[i].targets) << ";" << join(per_utt[i].token_begin) << "\n";
    } else if (mode == "train" && (argc == 2 || argc == 4)) {
      // train [<ctc epochs> <frame-level epochs>]      GPU.  The bidirectional net of ctc_decode_test's train mode on its dozen pattern
      // utterances (plus one beyond max_frames: skipped), trained with CTC until it recognises them; every utterance aligned; the
      // alignment against the labels, against the greedy path and its score; targets from the alignment; a fresh unidirectional
      // <LstmProjectedStreams> net trained on them by the frame-level trainer.
      const int32 S = 4, K = 6, epochs = argc == 4 ? atoi(argv[2]) : 60, fl_epochs = argc == 4 ? atoi(argv[3]) : 30;
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
      {
        std::unique_ptr<LstmProjectedStreams> f(new_lstm(16, 32, 16, S)), b(new_lstm(16, 32, 16, S));
        LstmProjectedStreams *fp = f.release(), *bp = b.release();
        nnet.AppendComponent(new BLstmLayer(fp, bp));
      }
      nnet.AppendComponent(new_affine(32, K));
      nnet.AppendComponent(new SoftmaxLayer(K, K));
      for (int32 e = 0; e < epochs; e++) {
        const TrainCtcStats st = TrainCtcWholeUtterances(&nnet, utts, o);
        if (e % 10 == 0 || e == epochs - 1) std::cerr << "ctc epoch " << e << " loss/frame " << st.avg_loss_per_frame << "\n";
      }
      // the greedy path of every utterance: hypothesis, frame classes, score
      DecodeCtcOptions d;
      d.num_stream = S;
      d.max_frames = o.max_frames;
      std::vector<std::vector<int32> > hyp, greedy_fc(utts.size());
      std::vector<BaseFloat> greedy_score(utts.size(), 0.f);
      const DecodeCtcStats dec = DecodeCtcWholeUtterances(&nnet, utts, d, &hyp, nullptr,
          [&](const UtteranceBatch &b, const DeviceMatrix &, const CtcGreedyDecoder &g) {
            std::vector<int32> fc;
            std::vector<BaseFloat> sc;
            g.FrameClasses(&fc); g.UttScores(&sc);
            std::vector<std::vector<int32> > per_stream(b.num_stream);
            for (int32 s = 0; s < b.num_stream; s++)
              for (int32 t = 0; t < b.lens[s]; t++) per_stream[s].push_back(fc[(size_t)t * b.num_stream + s]);
            ScatterByUtterance(b, per_stream, &greedy_fc);
            ScatterByUtterance(b, sc, &greedy_score);
          });
      AlignCtcOptions a;
      a.num_stream = S;
      a.max_frames = o.max_frames;
      std::vector<CtcAlignment> ali;
      std::string report;
      const AlignCtcStats as = AlignCtcWholeUtterances(&nnet, utts, a, &ali, &report);
      std::cerr << report;
      int32 collapse_ok = 0, score_ok = 0, same_as_greedy = 0, greedy_correct = 0, bounds_ok = 0, naligned = 0;
      for (size_t i = 0; i < utts.size(); i++) {
        const CtcAlignment &al = ali[i];
        if (!al.aligned) continue;
        naligned++;
        collapse_ok += collapse(al.frame_class, 0) == utts[i].labels && (int32)al.frame_class.size() == utts[i].num_frames;
        // the greedy path is the unconstrained optimum: no alignment scores above it, but for the last bit of two different sums
        const float g = greedy_score[i], ulp = std::nextafter(std::fabs(g), INFINITY) - std::fabs(g);
        score_ok += al.score <= g + ulp;
        if (hyp[i] == utts[i].labels) { greedy_correct++; same_as_greedy += al.frame_class == greedy_fc[i]; }
        bool ok = al.token_begin.size() == utts[i].labels.size() && al.token_end.size() == utts[i].labels.size();
        for (size_t j = 0; ok && j < al.token_begin.size(); j++) {
          ok = al.token_begin[j] < al.token_end[j] && (j == 0 || al.token_end[j - 1] <= al.token_begin[j]);
          for (int32 t = al.token_begin[j]; ok && t < al.token_end[j]; t++) ok = al.frame_class[t] == utts[i].labels[j];
        }
        bounds_ok += ok;
        std::cerr << "utt " << i << " score " << al.score << " greedy " << g << " path " << join(al.frame_class) << "\n";
      }
      // the bridge: targets from the alignment, then the frame-level trainer on a fresh unidirectional net
      const int32 filled = SetTargetsFromAlignment(&utts, ali);
      int32 targets_ok = 0;
      double blank_frames = 0, frames = 0;
      for (size_t i = 0; i < utts.size(); i++) {
        if (!ali[i].aligned) continue;
        bool ok = (int32)utts[i].targets.size() == utts[i].num_frames && collapse(utts[i].targets, 0) == utts[i].labels;
        for (int32 c : utts[i].targets) { ok = ok && c >= 0 && c < K; blank_frames += c == 0; frames += 1; }
        targets_ok += ok;
      }
      Nnet uni;
      uni.AppendComponent(new TransmitLayer(16, 16));
      uni.AppendComponent(new LstmLayer(new_lstm(16, 32, 16, S)));
      uni.AppendComponent(new_affine(16, K));
      uni.AppendComponent(new SoftmaxLayer(K, K));
      TrainLstmStreamsOptions fo;
      fo.num_stream = S; fo.batch_size = 20; fo.targets_delay = 2;
      // measured: at learn rate 0.01 and momentum 0.9 (the CTC trainer's) the frame-level loss jumps from epoch to epoch and one run in
      // three ended in NaN; the gradient here is a sum over 80 frames per minibatch
      fo.trn_opts.learn_rate = 0.003f; fo.trn_opts.momentum = 0.5f;
      double first = 0, last = 0, acc = 0;
      int32 fl_done = 0;
      for (int32 e = 0; e < fl_epochs; e++) {
        const TrainLstmStreamsStats st = TrainLstmStreams(&uni, utts, fo);
        if (e == 0) first = st.avg_loss;
        last = st.avg_loss; acc = st.frame_accuracy; fl_done = st.num_done;
        std::cerr << "frame-level epoch " << e << " loss " << st.avg_loss << " frame accuracy " << st.frame_accuracy << " blank share "
                  << blank_frames / frames << "\n";
      }
      std::cout << "OK ter=" << dec.token_error_rate << " aligned=" << naligned << " num_aligned=" << (int)as.num_aligned << " rejected=" << (int)as.num_rejected
                << " skipped=" << as.num_skipped << " collapse_ok=" << collapse_ok << " score_ok=" << score_ok << " greedy_correct=" << greedy_correct
                << " same_as_greedy=" << same_as_greedy << " bounds_ok=" << bounds_ok << " filled=" << filled << " targets_ok=" << targets_ok
                << " fl_done=" << fl_done << " fl_first_loss=" << first << " fl_last_loss=" << last << " fl_frame_accuracy=" << acc
                << " blank_share=" << blank_frames / frames << " blank_ratio=" << as.blank_ratio << " avg_score_per_frame=" << as.avg_score_per_frame << "\n";
    } else {
      std::cerr << "usage: ctc_align_test order <streams> <sort> <max_frames> <lens> | train [<ctc epochs> <frame-level epochs>]\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
