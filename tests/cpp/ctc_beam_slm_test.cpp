// tests/cpp/ctc_beam_slm_test.cpp -- drives ReadArpaLabelLm, CtcSparseLabelLm, the SetLanguageModel overloads of CtcBeamDecoder and
// CtcStreamDecoder and DecodeCtcOptions::slm (include/klstm_nnet.hpp) for tests/test_ctc_beam_slm.py and tests/test_ctc_beam_slm_gpu.py
// on an ARPA file and a minibatch the test wrote, and dumps what it made for the test to compare.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
template <class T>
static void put_all(std::ofstream &f, const std::vector<T> &v) {
  put(f, (int32)v.size());
  f.write(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T));
}
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
// lines of "token class"
static std::map<std::string, int32> read_symbols(const char *path) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("cannot open the symbol table");
  std::map<std::string, int32> m;
  std::string tok;
  int32 c;
  while (f >> tok >> c) m[tok] = c;
  return m;
}
static SparseLabelLm read_model(char **a) {                         // <arpa> <symbols> K blank alpha beta
  std::ifstream f(a[0]);
  if (!f) throw std::runtime_error("cannot open the ARPA file");
  return ReadArpaLabelLm(f, read_symbols(a[1]), std::atoi(a[2]), std::atoi(a[3]), std::atof(a[4]), std::atof(a[5]));
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "arpa" && argc == 9) {
      // arpa <arpa> <symbols> K blank alpha beta <out>      host only.  out: the seven arrays, each as a count and its values
      const SparseLabelLm m = read_model(argv + 2);
      std::ofstream out(argv[8], std::ios::binary);
      put_all(out, m.arc_offsets); put_all(out, m.arc_labels); put_all(out, m.arc_next); put_all(out, m.arc_weight);
      put_all(out, m.backoff); put_all(out, m.backoff_weight); put_all(out, m.final_weight);
      std::cout << "OK states=" << m.NumStates() << " arcs=" << m.arc_labels.size() << "\n";
    } else if (mode == "decode" && argc == 11) {
      // decode <arpa> <symbols> K blank alpha beta <in> <out> <chunk>      GPU.  in: T, S, B, C, N; lens [S]; posteriors [T*S*K].  out, a
      // list per stream each time: CtcBeamDecoder with the sparse model; DecodeCtcWholeUtterances with DecodeCtcOptions::slm through an
      // identity net; CtcStreamDecoder fed `chunk` frames a step and emitted with mode 2; the decoder after SetLanguageModel(nullptr)
      const SparseLabelLm m = read_model(argv + 2);
      const int32 K = std::atoi(argv[4]), blank = std::atoi(argv[5]), chunk = std::atoi(argv[10]);
      std::ifstream in(argv[8], std::ios::binary);
      const std::vector<int32> hd = get<int32>(in, 5);
      const int32 T = hd[0], S = hd[1], B = hd[2], C = hd[3], N = hd[4];
      const std::vector<int32> lens = get<int32>(in, S);
      const std::vector<BaseFloat> post = get<BaseFloat>(in, (size_t)T * S * K);
      CtcSparseLabelLm slm(m, blank);
      std::ofstream out(argv[9], std::ios::binary);
      const std::vector<std::vector<int32> > none;

      DeviceMatrix y;
      y.CopyFromHost(post.data(), T * S, K);
      CtcBeamDecoder dec(blank, B, C, N);
      dec.SetLanguageModel(&slm);
      std::vector<CtcNbestList> lists;
      dec.Decode(y, S, lens, none, &lists);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);

      std::vector<Utterance> utts(S);
      int32 longest = 1;
      for (int32 s = 0; s < S; s++) {
        Utterance &u = utts[s];
        u.dim = K;
        u.num_frames = lens[s] > 0 && lens[s] <= T ? lens[s] : 0;                // 0 frames: skipped by the batcher
        longest = std::max(longest, u.num_frames);
        for (int32 t = 0; t < u.num_frames; t++)
          u.feats.insert(u.feats.end(), post.begin() + ((size_t)t * S + s) * K, post.begin() + ((size_t)t * S + s + 1) * K);
      }
      Nnet nnet;
      nnet.AppendComponent(new TransmitLayer(K, K));
      DecodeCtcOptions o;
      o.num_stream = S; o.blank = blank; o.sort_by_length = false; o.score = false;
      o.beam = B; o.cands = C; o.nbest = N; o.slm = &slm;
      std::vector<std::vector<int32> > best;
      std::vector<CtcNbestList> ulists;
      DecodeCtcWholeUtterances(&nnet, utts, o, &best, &ulists);
      bool best_ok = true;
      for (int32 s = 0; s < S; s++) {
        put_list(out, ulists[s]);
        best_ok = best_ok && (ulists[s].empty() ? best[s].empty() : best[s] == ulists[s][0].tokens);
      }

      CtcStreamDecoder sd(blank, B, C, N, S, longest);
      sd.SetLanguageModel(&slm);
      for (int32 t0 = 0; t0 < T; t0 += chunk) {
        const int32 Tc = std::min(chunk, T - t0);
        std::vector<int32> cl(S), start(S, t0 == 0 ? 1 : 0);
        bool any = false;
        for (int32 s = 0; s < S; s++) {
          const int32 n = lens[s] > 0 && lens[s] <= T ? lens[s] : 0;
          cl[s] = std::max(0, std::min(Tc, n - t0));
          any = any || cl[s] > 0;
        }
        if (!any) break;
        DeviceMatrix part;
        part.CopyFromHost(post.data() + (size_t)t0 * S * K, Tc * S, K);
        sd.Step(part, cl, start);
      }
      sd.Emit(std::vector<int32>(S, 2), none, &lists, nullptr, nullptr);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);

      dec.SetLanguageModel(nullptr);
      dec.Decode(y, S, lens, none, &lists);
      for (int32 s = 0; s < S; s++) put_list(out, lists[s]);
      const int32 *st = slm.Status();
      std::cout << "OK best_ok=" << (int)best_ok << " states=" << slm.NumStates() << " dropped=" << st[0] + st[1] + st[2] + st[3]
                << " cut=" << st[4] + st[5] << "\n";
    } else {
      std::cerr << "usage: ctc_beam_slm_test arpa <arpa> <symbols> K blank alpha beta <out> | decode <arpa> <symbols> K blank alpha beta <in> <out> <chunk>\n";
      return 2;
    }
  } catch (const std::exception &e) {
    std::cout << "ERROR " << e.what() << "\n";
    return 1;
  }
  return 0;
}
