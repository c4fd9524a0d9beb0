// tests/cpp/gran_plan_test.cpp -- the host's bookkeeping of the value-only granule rings (csrc/klstm_kernels.h: gran_plan, gran_advance,
// gran_reset, gran_grow_slots) against a model of the rings themselves.  No device: every slot of the two rings is a flag (poisoned or
// written); a launch checks that every slot it will poll is poisoned, writes its slots and poisons what the plan tells it to.  Built with
// -fsanitize=address,undefined and run on the host (tests/test_gran_plan.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kaldi-lstm_amd/csrc/klstm_kernels.h"

using namespace klstm;

static int failures = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

struct Rings {
  GranState st;
  std::vector<char> dirty[2];                        // per ring and slot: written since it was last poisoned
  int cap;
  long value_launches = 0, tagged_launches = 0, grows = 0;
  explicit Rings(int cap_) : cap(cap_) {}
  void fill() { for (auto &r : dirty) r.assign((size_t)st.slots, 0); }
  void recover() { fill(); gran_reset(st); }
  // one launch of T frames, as the engine issues it (klstm_engine.hip set_gran_args) and the kernels run it
  void launch(int T) {
    const GranPlan p = gran_plan(st.n, T, st.last[1 - (int)(st.n & 1u)], st.slots, cap);
    if (!p.use) { CHECK(T + 2 > cap || T < 1); tagged_launches++; return; }
    CHECK(T + 2 <= cap);
    if (p.grow_to) {
      CHECK(p.grow_to >= T + 2 && p.grow_to <= cap && p.grow_to > st.slots);
      CHECK(p.ring == 0 && p.npoison == 0);
      st.slots = p.grow_to;
      fill(); gran_reset(st);
      grows++;
    } else {
      CHECK(p.ring == (int)(st.n & 1u));
    }
    CHECK(T + 2 <= st.slots);
    CHECK(p.npoison >= 0 && p.npoison <= st.slots - 1);
    std::vector<char> &mine = dirty[p.ring], &other = dirty[1 - p.ring];
    for (int t = 1; t <= T; t++) CHECK(!mine[(size_t)t]);          // every slot this launch polls holds POISON
    for (int t = 1; t <= T; t++) mine[(size_t)t] = 1;              // ... and is written exactly once
    for (int t = 1; t <= p.npoison; t++) other[(size_t)t] = 0;
    for (size_t t = 0; t < other.size(); t++) CHECK(!other[t]);    // the other ring is clean for the next launch
    CHECK(!mine[0] && !mine[(size_t)st.slots - 1]);                // the spare slots at either end stay untouched
    gran_advance(st, p, T);
    value_launches++;
  }
};

int main() {
  // fixed and alternating frame counts, both parities of the launch count
  for (int T : {3, 8, 9, 20, 30}) {
    Rings r(GRAN_CAP_SLOTS);
    for (int i = 0; i < 7; i++) r.launch(T);
    CHECK(r.value_launches == 7 && r.grows == 1 && r.st.slots == 32);
  }
  {
    Rings r(GRAN_CAP_SLOTS);
    const int seq[] = {20, 8, 20, 9, 8, 8, 30, 3, 3, 20};
    for (int T : seq) r.launch(T);
    CHECK(r.grows == 1 && r.value_launches == 10);
  }
  // growth: 32 -> 64 -> 256 slots, then small again (the rings never shrink)
  {
    Rings r(GRAN_CAP_SLOTS);
    const int seq[] = {20, 8, 40, 8, 40, 62, 63, 20, 254, 9, 254, 254, 20};
    for (int T : seq) r.launch(T);
    CHECK(r.grows == 4 && r.st.slots == 256 && r.tagged_launches == 0);
  }
  CHECK(gran_grow_slots(1) == 32 && gran_grow_slots(30) == 32 && gran_grow_slots(31) == 64 && gran_grow_slots(62) == 64);
  CHECK(gran_grow_slots(63) == 128 && gran_grow_slots(254) == 256 && gran_grow_slots(200, 100) == 100);
  // the cap: tagged launches in between leave the state alone
  {
    Rings r(GRAN_CAP_SLOTS);
    const int seq[] = {20, 255, 20, 1000, 255, 9, 20, 255};
    for (int T : seq) r.launch(T);
    CHECK(r.tagged_launches == 4 && r.value_launches == 4 && r.st.n == 4);
  }
  {
    Rings r(40);                                     // a small cap: T <= 38
    const int seq[] = {20, 38, 39, 38, 20, 39, 8};
    for (int T : seq) r.launch(T);
    CHECK(r.tagged_launches == 2 && r.st.slots == 40 && r.grows == 2);
  }
  // recover(): both rings poisoned, the count starts over, whatever the launches in between left
  {
    Rings r(GRAN_CAP_SLOTS);
    for (int T : {20, 9, 20}) r.launch(T);
    r.recover();
    CHECK(r.st.n == 0 && r.st.last[0] == 0 && r.st.last[1] == 0 && r.st.slots == 32);
    for (int T : {8, 20, 9, 20}) r.launch(T);
  }
  // a long pseudo-random run over every frame count up to the cap, with recoveries
  {
    Rings r(GRAN_CAP_SLOTS);
    unsigned x = 12345u;
    for (int i = 0; i < 5000; i++) {
      x = x * 1664525u + 1013904223u;
      const int T = 1 + (int)((x >> 8) % 300u);
      if ((x >> 20) % 97u == 0) r.recover();
      r.launch(T);
    }
    CHECK(r.value_launches > 3000 && r.tagged_launches > 300);
  }
  // arguments out of range
  CHECK(gran_plan(0, 0, 0, 32).use == 0 && gran_plan(0, -5, 0, 32).use == 0);
  CHECK(gran_plan(3, 20, 1000, 32).npoison == 31 && gran_plan(3, 20, -4, 32).npoison == 0);
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("gran_plan: all checks passed\n");
  return 0;
}
