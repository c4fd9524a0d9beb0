// tests/cpp/rnnt_greedy_test.cpp -- drives TransducerGreedy and DecodeTransducerWholeUtterances (include/klstm_nnet.hpp) for
// tests/test_rnnt_greedy_gpu.py.  The small model of rnnt_test.cpp (encoder <LstmProjectedStreams> 8 -> 16 / 8 + <AffineTransform> to
// J = 16; predictor <AffineTransform> 5 -> 8 + <LstmProjectedStreams> 8 -> 16 / 8 + <AffineTransform> to 16; V = 5) decodes three
// utterances of 12, 9 and 7 frames on two streams (the second minibatch has an idle stream), once with poll_every = 1 and once with 0.
// After each minibatch of the first pass the predictor runs teacher-forced over the decoded hypotheses, as the trainer runs it.
// `rnnt_greedy_test <file>` writes JSON to <file>: V, J, blank, bos, max_symbols, max_len, W, b, labels, and per utterance enc, pred (the
// teacher-forced rows 0 .. U), tokens, frames, flags, score.  Prints OK <both passes agree 0/1> <utterances> <labels> <steps of each pass>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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
static void dump(std::ostream &os, const char *name, const T *v, size_t n, const char *end = ",") {
  os << "\"" << name << "\": [";
  os.precision(9);
  for (size_t i = 0; i < n; i++) os << (i ? ", " : "") << v[i];
  os << "]" << end;
}

int main(int argc, char **argv) {
  try {
    if (argc < 2) KLSTM_ERR("usage: rnnt_greedy_test <file>");
    const int32 V = 5, J = 16, S = 2;
    std::srand(7);
    Nnet enc, pred;
    enc.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, S)));
    enc.AppendComponent(new_affine(8, J, 20.0));           // (large last layers: the untrained LSTMs' outputs are a few hundredths, and
    pred.AppendComponent(new_affine(V, 8, 1.0));           // the joint should see inputs of order one, or the bias alone decides)
    pred.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, S)));
    pred.AppendComponent(new_affine(8, J, 20.0));
    TransducerJoint joint(J, V);
    std::vector<BaseFloat> w, b;
    random_params(J, V, 2.0, &w, &b);
    b[0] = 1.f;                                            // the blank: about every other node emits
    joint.SetParams(w, b);
    const int32 frames[3] = {12, 9, 7};
    std::vector<Utterance> utts(3);
    for (int i = 0; i < 3; i++) {
      utts[i].num_frames = frames[i]; utts[i].dim = 8;
      for (int k = 0; k < frames[i] * 8; k++) utts[i].feats.push_back((BaseFloat)((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 2.f);
    }
    DecodeTransducerOptions o;
    o.num_stream = S; o.blank = 0; o.max_symbols = 2; o.max_len = 20; o.poll_every = 1;
    std::vector<TransducerHypothesis> hyp, again;
    std::vector<std::vector<BaseFloat> > enc_rows(3), pred_rows(3);
    std::vector<int> all(S, 1);
    Transducer pack(o.blank);
    DeviceMatrix pred_in, pred_out;
    std::string report;
    const DecodeTransducerStats st = DecodeTransducerWholeUtterances(&enc, &pred, &joint, utts, o, &hyp, &report,
        [&](const UtteranceBatch &bt, const DeviceMatrix &eo, const TransducerGreedy &g) {
          std::vector<TransducerHypothesis> h;
          g.Results(&h);
          std::vector<std::vector<int32> > labels;
          for (const auto &x : h) labels.push_back(x.tokens);
          pack.Pack(S, labels, V, o.blank, &pred_in);      // the predictor teacher-forced over the hypotheses, from reset state
          pred.Reset(all);
          pred.Propagate(pred_in.View(), &pred_out);
          std::vector<BaseFloat> e, p;
          eo.CopyToHost(&e); pred_out.CopyToHost(&p);
          for (int32 s = 0; s < S; s++) {
            const int32 i = bt.utt_index[s];
            if (i < 0) continue;
            for (int32 t = 0; t < bt.lens[s]; t++) enc_rows[i].insert(enc_rows[i].end(), &e[((size_t)t * S + s) * J], &e[((size_t)t * S + s) * J] + J);
            for (size_t u = 0; u <= labels[s].size(); u++) pred_rows[i].insert(pred_rows[i].end(), &p[(u * S + s) * J], &p[(u * S + s) * J] + J);
          }
        });
    o.poll_every = 0;
    const DecodeTransducerStats st0 = DecodeTransducerWholeUtterances(&enc, &pred, &joint, utts, o, &again);
    bool same = st.total_labels == st0.total_labels && st.num_utterances == 3 && st0.num_steps == 2 * (o.max_len + 1);
    for (int i = 0; i < 3; i++)
      same = same && hyp[i].tokens == again[i].tokens && hyp[i].frames == again[i].frames && hyp[i].flags == again[i].flags &&
             std::memcmp(&hyp[i].score, &again[i].score, sizeof(BaseFloat)) == 0;
    std::ofstream os(argv[1]);
    os << "{\"V\": " << V << ", \"J\": " << J << ", \"blank\": " << o.blank << ", \"bos\": " << o.blank << ", \"max_symbols\": " << o.max_symbols
       << ", \"max_len\": " << o.max_len << ", \"labels\": " << st.total_labels << ", ";
    dump(os, "W", w.data(), w.size());
    dump(os, "b", b.data(), b.size());
    os << "\"utts\": [";
    for (int i = 0; i < 3; i++) {
      os << (i ? ", {" : "{");
      dump(os, "enc", enc_rows[i].data(), enc_rows[i].size());
      dump(os, "pred", pred_rows[i].data(), pred_rows[i].size());
      dump(os, "tokens", hyp[i].tokens.data(), hyp[i].tokens.size());
      dump(os, "frames", hyp[i].frames.data(), hyp[i].frames.size());
      os << "\"flags\": " << hyp[i].flags << ", \"score\": " << hyp[i].score << "}";
    }
    os << "]}\n";
    os.close();
    std::printf("OK %d %lld %lld %lld %lld\n", (int)same, (long long)st.num_utterances, (long long)st.total_labels, (long long)st.num_steps,
                (long long)st0.num_steps);
    return 0;
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
