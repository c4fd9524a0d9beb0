// tests/cpp/scorer_test.cpp -- drives include/klstm_scorer.hpp (batched scoring, google -> standard conversion) for
// tests/test_scorer.py (host-only modes, no GPU) and tests/test_scorer_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../include/klstm_scorer.hpp"

using namespace klstm_kaldi;

static std::vector<float> read_raw(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) KLSTM_ERR("cannot open " << path);
  f.seekg(0, std::ios::end);
  const size_t n = (size_t)f.tellg() / sizeof(float);
  f.seekg(0);
  std::vector<float> v(n);
  f.read(reinterpret_cast<char *>(v.data()), n * sizeof(float));
  return v;
}
static void write_raw(const std::string &path, const float *p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char *>(p), n * sizeof(float));
}
static std::vector<int32> parse_ints(const std::string &csv) {
  std::vector<int32> v;
  std::stringstream ss(csv);
  std::string tok;
  while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(atoi(tok.c_str()));
  return v;
}
static BatchScorerOptions options(const char *S, const char *T, const char *mode, const char *delay) {
  BatchScorerOptions o;
  o.num_stream = atoi(S); o.chunk = atoi(T);
  const std::string m = mode;
  o.mode = m == "post" ? KLSTM_SCORE_POSTERIOR : m == "logpost" ? KLSTM_SCORE_LOGPOST : m == "loglike" ? KLSTM_SCORE_LOGLIKE : -1;
  if (std::string(delay) != "none") o.targets_delay = atoi(delay);
  return o;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "convert" && argc == 6) {
      // convert <google_nnet> <shift> <binary> <out>          ConvertToStandard, then Nnet::Write (host only)
      Nnet in, out;
      in.Read(argv[2]);
      ConvertToStandard(in, atoi(argv[3]), &out);
      out.Write(argv[5], atoi(argv[4]) != 0);
      std::cout << "OK " << out.NumComponents();
      for (int32 i = 0; i < out.NumComponents(); i++) std::cout << " " << out.GetComponent(i).Marker();
      std::cout << "\n";
    } else if (mode == "check" && argc == 7) {
      // check <nnet> <S> <T> <post|logpost|loglike> <targets_delay|none>     BatchScorer's topology / option checks (host only)
      Nnet nnet;
      nnet.Read(argv[2]);
      BatchScorerOptions o = options(argv[3], argv[4], argv[5], argv[6]);
      if (o.mode == KLSTM_SCORE_LOGLIKE) o.log_prior.assign(nnet.OutputDim(), 0.f);
      std::cout << "OK shift " << BatchScorer::CheckTopology(nnet, o) << "\n";
    } else if (mode == "plan" && argc == 5) {
      // plan <S> <T> <len,len,...>        PlanChunks (host only): "chunks n", then per chunk the desc, reset and dst lines
      const ScorePlan p = PlanChunks(parse_ints(argv[4]), atoi(argv[2]), atoi(argv[3]));
      std::cout << "chunks " << p.num_chunks << "\n";
      for (int32 c = 0; c < p.num_chunks; c++) {
        for (int32 i = 0; i < 3 * p.S; i++) std::cout << (i ? " " : "") << p.desc[(size_t)c * 3 * p.S + i];
        std::cout << "\n";
        for (int32 i = 0; i < p.S; i++) std::cout << (i ? " " : "") << p.reset[(size_t)c * p.S + i];
        std::cout << "\n";
        for (int32 i = 0; i < p.S * p.T; i++) std::cout << (i ? " " : "") << p.dst[(size_t)c * p.S * p.T + i];
        std::cout << "\n";
      }
    } else if (mode == "score" && argc == 12) {
      // score <nnet> <feats_raw> <len,len,...> <S> <T> <post|logpost|loglike> <targets_delay|none> <log_prior_raw|none> <prior_scale> <out_raw>
      // host API: the concatenated feature rows are split into utterances, scored, the outputs concatenated again
      Nnet nnet;
      nnet.Read(argv[2]);
      const std::vector<float> x = read_raw(argv[3]);
      const std::vector<int32> lens = parse_ints(argv[4]);
      BatchScorerOptions o = options(argv[5], argv[6], argv[7], argv[8]);
      if (std::string(argv[9]) != "none") o.log_prior = read_raw(argv[9]);
      o.prior_scale = (float)atof(argv[10]);
      BatchScorer sc(nnet, o);
      std::vector<std::vector<float> > utts, outs;
      size_t off = 0;
      for (int32 n : lens) {
        utts.emplace_back(x.begin() + off, x.begin() + off + (size_t)n * sc.InputDim());
        off += (size_t)n * sc.InputDim();
      }
      if (off != x.size()) KLSTM_ERR("score: " << x.size() << " floats for " << off << " expected");
      sc.Score(utts, &outs);
      std::vector<float> all;
      for (const auto &u : outs) all.insert(all.end(), u.begin(), u.end());
      write_raw(argv[11], all.data(), all.size());
      std::cout << "OK " << outs.size() << " " << sc.OutputDim() << " " << sc.Shift() << "\n";
    } else {
      std::cerr << "usage: scorer_test convert|check|plan|score ...\n";
      return 2;
    }
  } catch (const std::exception &ex) {
    std::cout << "ERROR " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
