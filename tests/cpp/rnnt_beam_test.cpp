// tests/cpp/rnnt_beam_test.cpp -- drives TransducerBeam and DecodeTransducerBeamWholeUtterances (include/klstm_nnet.hpp) for
// tests/test_rnnt_beam_gpu.py.  The small model of rnnt_greedy_test.cpp (V = 5, J = 16, LSTM predictor behind an embedding Affine)
// decodes three utterances of 12, 9 and 7 frames on two streams with beam 3, so the predictor runs six streams and the second
// minibatch has an idle stream; once with poll_every = 1 and once with 0.  Then the predictor runs teacher-forced, from reset state,
// over all 64 label sequences of max_len = 3 labels: the rows of every prefix a search can visit.
// `rnnt_beam_test <file>` writes JSON to <file>: V, J, blank, bos, beam, nbest, max_len, W, b, prefixes [{y, row}], and per utterance
// enc, flags, nbest [{tokens, score}].  Prints OK <both passes agree 0/1> <utterances> <hypotheses> <steps of each pass>.
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
    if (argc < 2) KLSTM_ERR("usage: rnnt_beam_test <file>");
    const int32 V = 5, J = 16, S = 2, B = 3, SB = S * B;
    std::srand(7);
    Nnet enc, pred;
    enc.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, S)));
    enc.AppendComponent(new_affine(8, J, 20.0));
    pred.AppendComponent(new_affine(V, 8, 1.0));
    pred.AppendComponent(new LstmLayer(new_lstm(8, 16, 8, SB)));   // one stream per slot
    pred.AppendComponent(new_affine(8, J, 20.0));
    TransducerJoint joint(J, V);
    std::vector<BaseFloat> w, b;
    random_params(J, V, 2.0, &w, &b);
    b[0] = 3.f;                                            // the blank: a label every few frames, so that lists of <= 3 labels carry weight
    joint.SetParams(w, b);
    const int32 frames[3] = {12, 9, 7};
    std::vector<Utterance> utts(3);
    for (int i = 0; i < 3; i++) {
      utts[i].num_frames = frames[i]; utts[i].dim = 8;
      for (int k = 0; k < frames[i] * 8; k++) utts[i].feats.push_back((BaseFloat)((std::rand() + 1.0) / (RAND_MAX + 2.0) - 0.5) * 2.f);
    }
    DecodeTransducerBeamOptions o;
    o.num_stream = S; o.blank = 0; o.beam = B; o.nbest = 3; o.max_len = 3; o.poll_every = 1;
    std::vector<CtcNbestList> lists, again;
    std::vector<int32> flags, flags_again;
    std::vector<std::vector<BaseFloat> > enc_rows(3);
    std::string report;
    const DecodeTransducerBeamStats st = DecodeTransducerBeamWholeUtterances(&enc, &pred, &joint, utts, o, &lists, &flags, &report,
        [&](const UtteranceBatch &bt, const DeviceMatrix &eo, const TransducerBeam &) {
          std::vector<BaseFloat> e;
          eo.CopyToHost(&e);
          for (int32 s = 0; s < S; s++)
            for (int32 t = 0; bt.utt_index[s] >= 0 && t < bt.lens[s]; t++)
              enc_rows[bt.utt_index[s]].insert(enc_rows[bt.utt_index[s]].end(), &e[((size_t)t * S + s) * J], &e[((size_t)t * S + s) * J] + J);
        });
    o.poll_every = 0;
    const DecodeTransducerBeamStats st0 = DecodeTransducerBeamWholeUtterances(&enc, &pred, &joint, utts, o, &again, &flags_again, nullptr,
        [](const UtteranceBatch &, const DeviceMatrix &, const TransducerBeam &) {});
    bool same = st.total_hypotheses == st0.total_hypotheses && st.num_utterances == 3 && st0.num_steps == 2 * (o.max_len + 1) && flags == flags_again;
    for (int i = 0; i < 3; i++) {
      same = same && lists[i].size() == again[i].size();
      for (size_t q = 0; same && q < lists[i].size(); q++)
        same = lists[i][q].tokens == again[i][q].tokens && std::memcmp(&lists[i][q].score, &again[i][q].score, sizeof(BaseFloat)) == 0;
    }
    // a stream limit the predictor was not built for is refused with a message
    bool refused = false;
    try { o.num_stream = 1; DecodeTransducerBeamWholeUtterances(&enc, &pred, &joint, utts, o, &again); } catch (const std::exception &) { refused = true; }
    same = same && refused;

    std::ofstream os(argv[1]);
    os << "{\"V\": " << V << ", \"J\": " << J << ", \"blank\": " << o.blank << ", \"bos\": " << o.blank << ", \"beam\": " << B << ", \"nbest\": " << o.nbest
       << ", \"max_len\": " << o.max_len << ", ";
    dump(os, "W", w.data(), w.size());
    dump(os, "b", b.data(), b.size());
    os << "\"prefixes\": [";
    Transducer pack(o.blank);
    DeviceMatrix pred_in, pred_out;
    std::vector<int> all(SB, 1);
    std::vector<BaseFloat> p;
    bool first = true;
    for (int32 base = 0; base < 64; base += SB) {          // sequence n: the base-4 digits of n, labels 1 .. 4
      std::vector<std::vector<int32> > labels(SB);
      for (int32 s = 0; s < SB && base + s < 64; s++)
        labels[s] = {1 + (base + s) / 16, 1 + (base + s) / 4 % 4, 1 + (base + s) % 4};
      pack.Pack(SB, labels, V, o.blank, &pred_in);
      pred.Reset(all);
      pred.Propagate(pred_in.View(), &pred_out);
      pred_out.CopyToHost(&p);
      for (int32 s = 0; s < SB && base + s < 64; s++)
        for (size_t u = 0; u <= 3; u++) {
          if (u < 3 && (base + s) % (u == 2 ? 4 : u == 1 ? 16 : 64) != 0) continue;   // each prefix once: from its first extension
          os << (first ? "{" : ", {");
          first = false;
          dump(os, "y", labels[s].data(), u);
          dump(os, "row", &p[(u * SB + s) * J], (size_t)J, "}");
        }
    }
    os << "], \"utts\": [";
    for (int i = 0; i < 3; i++) {
      os << (i ? ", {" : "{");
      dump(os, "enc", enc_rows[i].data(), enc_rows[i].size());
      os << "\"flags\": " << flags[i] << ", \"nbest\": [";
      for (size_t q = 0; q < lists[i].size(); q++) {
        os << (q ? ", {" : "{");
        dump(os, "tokens", lists[i][q].tokens.data(), lists[i][q].tokens.size());
        os << "\"score\": " << lists[i][q].score << "}";
      }
      os << "]}";
    }
    os << "]}\n";
    os.close();
    std::printf("OK %d %lld %lld %lld %lld\n", (int)same, (long long)st.num_utterances, (long long)st.total_hypotheses, (long long)st.num_steps,
                (long long)st0.num_steps);
    return 0;
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
