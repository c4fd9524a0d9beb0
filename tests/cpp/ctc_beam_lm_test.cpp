// tests/cpp/ctc_beam_lm_test.cpp -- drives CtcLabelLm, CtcBeamDecoder::SetLanguageModel and DecodeCtcOptions::lm (include/klstm_nnet.hpp)
// for tests/test_ctc_beam_lm_gpu.py on a minibatch and tables the test wrote, and dumps the lists for it to compare.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

template <class T>
static std::vector<T> get(std::ifstream &f, size_t n) {
  std::vector<T> v(n);
  f.read(reinterpret_cast<char *>(v.data()), n * sizeof(T));
  if (!f) throw std::runtime_error("short input file");
  return v;
}
static void put(std::ofstream &f, int32 v) { f.write(reinterpret_cast<const char *>(&v), sizeof(v)); }
// count, then per hypothesis: length, score bits, tokens
static void put_list(std::ofstream &f, const CtcNbestList &l) {
  put(f, (int32)l.size());
  for (const CtcHypothesis &h : l) {
    int32 bits;
    std::memcpy(&bits, &h.score, sizeof(bits));
    put(f, (int32)h.tokens.size()); put(f, bits);
    for (int32 c : h.tokens) put(f, c);
  }
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "decode" && argc == 4) {
      // decode <in> <out>      GPU.  in: T, S, K, B, C, N, Q, has_final, blank; lens [S]; posteriors [T*S*K]; next [Q*K]; weight [Q*K]; final
      // [Q] if has_final.  out, a list per stream each time: CtcBeamDecoder with SetLanguageModel; DecodeCtcWholeUtterances with
      // DecodeCtcOptions::lm through an identity net (utterance s = the frames of stream s; an idle stream has an empty list); the same
      // decoder after SetLanguageModel(nullptr); a fresh decoder that never saw one.
      std::ifstream in(argv[2], std::ios::binary);
      const std::vector<int32> hd = get<int32>(in, 9);
      const int32 T = hd[0], S = hd[1], K = hd[2], B = hd[3], C = hd[4], N = hd[5], Q = hd[6], blank = hd[8];
      const std::vector<int32> lens = get<int32>(in, S);
      const std::vector<BaseFloat> post = get<BaseFloat>(in, (size_t)T * S * K);
      const std::vector<int32> next = get<int32>(in, (size_t)Q * K);
      const std::vector<BaseFloat> weight = get<BaseFloat>(in, (size_t)Q * K);
      const std::vector<BaseFloat> fin = hd[7] ? get<BaseFloat>(in, Q) : std::vector<BaseFloat>();
      CtcLabelLm lm(Q, K, next, weight, fin);
      std::ofstream out(argv[3], std::ios::binary);
      const std::vector<std::vector<int32> > none;

      DeviceMatrix y;
      y.CopyFromHost(post.data(), T * S, K);
      CtcBeamDecoder dec(blank, B, C, N);
      dec.SetLanguageModel(&lm);
      std::vector<CtcNbestList> lists;
      dec.Decode(y, S, lens, none, &lists);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);

      std::vector<Utterance> utts(S);
      for (int32 s = 0; s < S; s++) {
        Utterance &u = utts[s];
        u.dim = K;
        u.num_frames = lens[s] > 0 && lens[s] <= T ? lens[s] : 0;                // 0 frames: skipped by the batcher
        for (int32 t = 0; t < u.num_frames; t++)
          u.feats.insert(u.feats.end(), post.begin() + ((size_t)t * S + s) * K, post.begin() + ((size_t)t * S + s + 1) * K);
      }
      Nnet nnet;
      nnet.AppendComponent(new TransmitLayer(K, K));
      DecodeCtcOptions o;
      o.num_stream = S; o.blank = blank; o.sort_by_length = false; o.score = false;
      o.beam = B; o.cands = C; o.nbest = N; o.lm = &lm;
      std::vector<std::vector<int32> > best;
      std::vector<CtcNbestList> ulists;
      DecodeCtcWholeUtterances(&nnet, utts, o, &best, &ulists);
      bool best_ok = true;
      for (int32 s = 0; s < S; s++) {
        put_list(out, ulists[s]);
        best_ok = best_ok && (ulists[s].empty() ? best[s].empty() : best[s] == ulists[s][0].tokens);
      }

      dec.SetLanguageModel(nullptr);
      dec.Decode(y, S, lens, none, &lists);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);
      CtcBeamDecoder plain(blank, B, C, N);
      plain.Decode(y, S, lens, none, &lists);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);
      std::cout << "OK best_ok=" << (int)best_ok << " states=" << lm.NumStates() << "\n";
    } else {
      std::cerr << "usage: ctc_beam_lm_test decode <in> <out>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
