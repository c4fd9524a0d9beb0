// kaldi-lstm_amd/csrc/klstm_ctc_host.h -- host code shared by the CTC launchers (klstm_ctc.hip: the loss; klstm_ctc_mbr.hip: the n-best
// risk; klstm_ctc_mmi.hip: MMI; klstm_ctc_align.hip: the forced alignment; klstm_ctc_consensus.hip, klstm_ctc_rescore.hip: the second
// pass): the plan of the alpha / beta chain and its dispatch, the label capacity of a workspace, the padding and alignment rules, the
// carver of a workspace.  Plain C++17, no HIP: a host program compiles it (tests/cpp/ctc_plan_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace klstm {

inline size_t ctc_up256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t ctc_npad(int Lcap) { return ((size_t)2 * Lcap + 1 + 3) / 4 * 4; }      // floats in a row of 2 Lcap + 1 states
inline bool ctc_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// 1: the rows of y and diff can be read and written 16 bytes at a time
inline int ctc_rows_vec(int K, int stride, int dstride, const void *y, const void *diff) {
  return K % 4 == 0 && stride % 4 == 0 && dstride % 4 == 0 && ctc_al16(y) && ctc_al16(diff);
}

// A workspace handed out region by region, each named once: packed<T>(n) is n elements at the current offset, take<T>(n) the same
// with the offset then rounded up to 256 bytes (the regions that need no rounding, the bulk rows, close a layout).  Over a null base
// every pointer is null and bytes() counts what a real base would have consumed: a layout is one function for both questions.
struct CtcCarver {
  char *base;
  size_t off = 0;
  explicit CtcCarver(void *b) : base(static_cast<char *>(b)) {}
  template <class T> T *packed(size_t n) { const size_t o = off; off += n * sizeof(T); return base ? reinterpret_cast<T *>(base + o) : nullptr; }
  template <class T> T *take(size_t n) { T *p = packed<T>(n); off = ctc_up256(off); return p; }
  size_t bytes() const { return off; }
};

// The geometry of ctc_chain_run for N = 2 Lcap + 1 states, as 16 * waves + states per thread.
// measured: four waves with one state per thread beat one wave with two (391 against 487 us at T = 1000, 101 states)
// -- the step is bound by its exp / log issue slots, which more waves on more SIMDs share, and the workgroup barrier costs less than
// a second state per lane; sixteen waves lose to four with two states each (670 against 633 us at 301 states), so they serve only
// what four cannot hold.
inline int ctc_chain_plan(int N) {
  return N <= 64 ? 16 * 1 + 1 : N <= 256 ? 16 * 4 + 1 : N <= 512 ? 16 * 4 + 2 : N <= 1024 ? 16 * 16 + 1 : 16 * 16 + 2;
}
// f(NW, P) of the plan, both as std::integral_constant (nw(), p() are constant expressions); `bad` for a plan outside the five
template <class R, class F>
R ctc_chain_dispatch(int plan, R bad, F &&f) {
  using std::integral_constant;
  switch (plan) {
    case 16 * 1 + 1: return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
    case 16 * 4 + 1: return f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
    case 16 * 4 + 2: return f(integral_constant<int, 4>{}, integral_constant<int, 2>{});
    case 16 * 16 + 1: return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    case 16 * 16 + 2: return f(integral_constant<int, 16>{}, integral_constant<int, 2>{});
    default: return bad;
  }
}

// The longest label sequence a workspace of `bytes` serves, -1: none.  bytes_at: Lcap -> bytes, not decreasing.
template <class F>
int ctc_label_capacity_of(size_t bytes, F &&bytes_at) {
  if (bytes < bytes_at(0)) return -1;
  int lo = 0, hi = 1023;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (bytes_at(mid) <= bytes) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace klstm
