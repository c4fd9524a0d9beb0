// tests/cpp/rnnt_simple_test.cpp -- drives Transducer::EvalSimple / BandFromOccupation (include/klstm_nnet.hpp) for
// tests/test_rnnt_simple_gpu.py.  T = 21, Umax = 6, V = 37, S = 2, R = 3; am, lm in that order from the generator
// x <- 1664525 x + 1013904223 (mod 2^32, from 12345), value 4 (((x >> 8) & 0xffff) / 65536 - 0.5), which the test repeats.  Prints
//   OK <the two losses as bit patterns> <the sums of the bit patterns of d_am, d_lm> <the S T band entries>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "../../include/klstm_blstm.hpp"

using namespace klstm_kaldi;

static unsigned long long bit_sum(const std::vector<float> &v) {
  unsigned long long sum = 0;
  for (float x : v) { uint32_t u; std::memcpy(&u, &x, 4); sum += u; }
  return sum;
}

int main() {
  try {
    const int32 T = 21, Umax = 6, V = 37, S = 2, R = 3;
    uint32_t x = 12345;
    auto gen = [&](size_t n) {
      std::vector<BaseFloat> v(n);
      for (auto &e : v) { x = x * 1664525u + 1013904223u; e = 4.f * ((BaseFloat)((x >> 8) & 0xffff) / 65536.f - 0.5f); }
      return v;
    };
    DeviceMatrix am, lm, d_am, d_lm;
    const std::vector<BaseFloat> ah = gen((size_t)T * S * V), lh = gen((size_t)(Umax + 1) * S * V);
    am.CopyFromHost(ah.data(), T * S, V);
    lm.CopyFromHost(lh.data(), (Umax + 1) * S, V);
    const std::vector<int32> lens = {T, T - 4};
    const std::vector<std::vector<int32> > labels = {{1, 2, 2, 3, 4, 36}, {5, 1, 3}};
    Transducer tr(0);
    const BaseFloat *occ = tr.EvalSimple(am, lm, S, lens, labels, &d_am, &d_lm);
    std::vector<BaseFloat> loss, da, dl;
    tr.UttLoss(&loss);
    const int32 *band_dev = tr.BandFromOccupation(occ, T, S, lens, labels, R);
    std::vector<int32> band((size_t)S * T);
    KCheck(klstm_memcpy_d2h(band.data(), band_dev, band.size() * sizeof(int32), nullptr));
    d_am.CopyToHost(&da);
    d_lm.CopyToHost(&dl);
    std::printf("OK");
    for (float v : loss) { uint32_t u; std::memcpy(&u, &v, 4); std::printf(" %u", u); }
    std::printf(" %llu %llu", bit_sum(da), bit_sum(dl));
    for (int32 v : band) std::printf(" %d", v);
    std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
