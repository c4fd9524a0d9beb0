// tests/cpp/ctc_plan_test.cpp -- the host helpers of the CTC lattice losses (csrc/klstm_ctc_host.h: ctc_chain_plan, ctc_chain_dispatch,
// ctc_label_capacity_of, ctc_npad, ctc_up256, CtcCarver) without a device: the plan table at both edges of every plan, the dispatcher's
// pair for every plan and its error for any other, the bisection over a toy byte count and over the loss's formula, which this file
// computes for itself, and the carver of a workspace over a null and over a real base.  Built with -fsanitize=address,undefined and run on the host (tests/test_ctc_plan.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../kaldi-lstm_amd/csrc/klstm_ctc_host.h"

using namespace klstm;

static int failures = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

// the workspace of klstm_ctc_eval, written out here: one status word and two links per label position in a head of
// whole 256 bytes, then the alpha and the beta rows of roundup4(2 L + 1) floats
static size_t loss_bytes(int T, int S, int L) {
  size_t head = (size_t)S * (1 + 2 * (size_t)L) * 4;
  while (head % 256) head++;
  size_t row = 2 * (size_t)L + 1;
  while (row % 4) row++;
  return head + 2 * (size_t)T * S * row * 4;
}

// The capacity is the largest L in [0, 1023] with bytes_at(L) <= bytes (here by a linear scan), -1 below bytes_at(0).  Where bytes_at
// steps up between L and L + 1 that is L itself from bytes_at(L) up to one byte below bytes_at(L + 1); a rounded formula has plateaus
// (the loss's at T = S = 1: L = 0 and 1 cost the same 288 bytes), and there the longer labelling is served by the same bytes.
// Returns how many of the four probed L were such steps.
template <class F>
static int check_capacity(F bytes_at) {
  auto scan = [&](size_t bytes) { int best = -1; for (int L = 0; L <= 1023; L++) if (bytes_at(L) <= bytes) best = L; return best; };
  int steps = 0;
  CHECK(ctc_label_capacity_of(bytes_at(0) - 1, bytes_at) == -1);
  for (int L : {0, 1, 511, 1022}) {
    CHECK(bytes_at(L) <= bytes_at(L + 1));
    const bool step = bytes_at(L) < bytes_at(L + 1);
    steps += step;
    const int lo = ctc_label_capacity_of(bytes_at(L), bytes_at), hi = ctc_label_capacity_of(bytes_at(L + 1) - 1, bytes_at);
    CHECK(lo == scan(bytes_at(L)) && hi == scan(bytes_at(L + 1) - 1));
    if (step) CHECK(lo == L && hi == L);
    else CHECK(lo > L);
  }
  CHECK(ctc_label_capacity_of(bytes_at(1023), bytes_at) == 1023);
  CHECK(ctc_label_capacity_of(bytes_at(1023) + 1, bytes_at) == 1023);
  CHECK(ctc_label_capacity_of(8 * bytes_at(1023), bytes_at) == 1023);
  return steps;
}

// A layout of every kind of region (the shape of cons_layout and mbr_layout: rounded regions of several types, one left out on a flag,
// packed bulk rows at the end), written through so that the sanitizer sees every byte a region owns.
struct Carved { std::vector<std::pair<char *, size_t> > regions; size_t bytes; };
static Carved carve(void *base, size_t n, bool with_keys) {
  CtcCarver c(base);
  Carved out;
  auto note = [&](void *p, size_t bytes) { out.regions.push_back({static_cast<char *>(p), bytes}); };
  note(c.take<unsigned>(64), 64 * sizeof(unsigned));
  note(c.take<int>(n), n * sizeof(int));
  note(c.take<double>(3 * n), 3 * n * sizeof(double));
  note(c.take<unsigned char>(n + 1), n + 1);
  if (with_keys) note(c.take<unsigned long long>(n), n * sizeof(unsigned long long));
  const size_t rounded = out.regions.size();
  note(c.packed<float>(4 * n + 4), (4 * n + 4) * sizeof(float));
  note(c.packed<float>(4 * n + 4), (4 * n + 4) * sizeof(float));
  out.bytes = c.bytes();
  CHECK(rounded == (with_keys ? 5u : 4u));
  return out;
}

static void check_carver() {
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000})
    for (bool with_keys : {false, true}) {
      const Carved count = carve(nullptr, n, with_keys);           // a null base only counts
      for (const auto &r : count.regions) CHECK(r.first == nullptr);
      std::vector<char> raw(count.bytes + 256);
      char *base = raw.data() + (256 - reinterpret_cast<uintptr_t>(raw.data()) % 256) % 256;
      const Carved real = carve(base, n, with_keys);
      CHECK(real.bytes == count.bytes && real.regions.size() == count.regions.size());      // ... what a real base consumes
      const size_t rounded = with_keys ? 5 : 4;
      char *end = base;
      for (size_t i = 0; i < real.regions.size(); i++) {
        const auto &r = real.regions[i];
        CHECK(r.first == end);                                     // in order, disjoint, nothing between them but the rounding
        if (i <= rounded) CHECK(reinterpret_cast<uintptr_t>(r.first) % 256 == 0);           // every take, and the first packed one
        std::memset(r.first, (int)i + 1, r.second);                // inside raw, or the sanitizer says so
        end = r.first + (i < rounded ? ctc_up256(r.second) : r.second);
      }
      CHECK(end == base + real.bytes);
      for (size_t i = 0; i < real.regions.size(); i++)             // nobody wrote into a neighbour
        CHECK(real.regions[i].first[0] == (char)(i + 1) && real.regions[i].first[real.regions[i].second - 1] == (char)(i + 1));
      CHECK(count.bytes == 256 + ctc_up256(4 * n) + ctc_up256(24 * n) + ctc_up256(n + 1) + (with_keys ? ctc_up256(8 * n) : 0) + 2 * (16 * n + 16));
    }
  CtcCarver empty(nullptr);
  CHECK(empty.bytes() == 0 && empty.take<int>(0) == nullptr && empty.bytes() == 0);
}

int main() {
  check_carver();
  // the plan table: 16 * waves + states per thread
  const struct { int N, nw, p; } table[] = {{1, 1, 1},    {63, 1, 1},   {64, 1, 1},    {65, 4, 1},    {255, 4, 1},   {256, 4, 1},  {257, 4, 2},
                                           {511, 4, 2},  {512, 4, 2},  {513, 16, 1},  {1023, 16, 1}, {1024, 16, 1}, {1025, 16, 2}, {2047, 16, 2}};
  for (const auto &e : table) {
    const int plan = ctc_chain_plan(e.N);
    CHECK(plan == 16 * e.nw + e.p);
    CHECK(64 * e.nw * e.p >= e.N);
    int nw = 0, p = 0, calls = 0;
    const int ret = ctc_chain_dispatch(plan, -1, [&](auto w, auto s) { nw = w(); p = s(); calls++; return 7; });
    CHECK(ret == 7 && calls == 1 && nw == e.nw && p == e.p);
  }
  // every other plan is the error, and the callable is not called
  for (int plan = -40; plan < 400; plan++) {
    if (plan == 17 || plan == 65 || plan == 66 || plan == 257 || plan == 258) continue;
    int calls = 0;
    CHECK(ctc_chain_dispatch(plan, -1, [&](auto, auto) { calls++; return 7; }) == -1 && calls == 0);
  }
  CHECK(ctc_chain_dispatch(16 * 8 + 1, -1, [](auto, auto) { return 7; }) == -1);      // the alignment's own plan is none of the five

  // the capacity over a toy byte count, then over the loss's formula
  CHECK(check_capacity([](int L) { return (size_t)1000 + 37 * (size_t)L; }) == 4);
  const int shapes[][2] = {{1, 1}, {50, 32}};
  for (const auto &ts : shapes) {
    const int T = ts[0], S = ts[1];
    CHECK(check_capacity([&](int L) { return loss_bytes(T, S, L); }) == (T == 1 ? 2 : 4));      // T = S = 1: plateaus at L = 0 and 1022
    for (int L : {0, 1, 2, 511, 1022, 1023}) {     // the pieces a layout is made of give the same count
      CHECK(ctc_up256((size_t)S * (1 + 2 * (size_t)L) * 4) + 2 * (size_t)T * S * ctc_npad(L) * 4 == loss_bytes(T, S, L));
      std::printf("loss_bytes %d %d %d %zu\n", T, S, L, loss_bytes(T, S, L));       // for the caller: what the library must answer
    }
  }
  CHECK(ctc_npad(0) == 4 && ctc_npad(1) == 4 && ctc_npad(2) == 8 && ctc_npad(1023) == 2048);
  CHECK(ctc_up256(0) == 0 && ctc_up256(1) == 256 && ctc_up256(256) == 256 && ctc_up256(257) == 512);
  alignas(16) static float row[8];
  CHECK(ctc_al16(row) && !ctc_al16(row + 1) && ctc_al16(row + 4));
  CHECK(ctc_rows_vec(8, 8, 12, row, row + 4) == 1 && ctc_rows_vec(6, 8, 8, row, row) == 0 && ctc_rows_vec(8, 6, 8, row, row) == 0);
  CHECK(ctc_rows_vec(8, 8, 6, row, row) == 0 && ctc_rows_vec(8, 8, 8, row + 1, row) == 0 && ctc_rows_vec(8, 8, 8, row, row + 2) == 0);

  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("ctc_plan: all checks passed\n");
  return 0;
}
