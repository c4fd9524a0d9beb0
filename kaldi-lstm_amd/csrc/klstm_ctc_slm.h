// kaldi-lstm_amd/csrc/klstm_ctc_slm.h -- the sparse back-off language model on the device, shared by the prefix beam search
// (klstm_ctc_beam.hip: builds the blob and walks it a frame ahead) and the n-best rescoring (klstm_ctc_rescore.hip: walks it along
// finished hypotheses): the one-rounding float helpers, the emission rule, the layout of the blob and slm_lookup, the walk itself.
// Moved here from klstm_ctc_beam.hip unchanged.  Include it BELOW the includer's `#pragma clang fp contract(off)`: hipcc contracts
// a * b + c into an FMA by default, and the pragma governs the operators written below it.  The header sets no pragma of its own: at
// file scope it would reach everything the includer writes after the include.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace klstm {

__device__ __forceinline__ float bmul(float a, float b) { return a * b; }
__device__ __forceinline__ float badd(float a, float b) { return a + b; }
__device__ __forceinline__ double bmul(double a, double b) { return a * b; }
__device__ __forceinline__ double badd(double a, double b) { return a + b; }

constexpr float BEAM_TINY = 0x1p-60f, BEAM_HUGE = 0x1p60f;

// NaN or below 2^-60: exactly 0; above 2^60 (+inf too): 2^60
__device__ __forceinline__ float beam_emit(float v) { return v >= BEAM_TINY ? fminf(v, BEAM_HUGE) : 0.f; }

// The blob of a sparse back-off model, Q states and A arcs (byte offsets, every section 16-byte aligned):
//   int hdr[16]      [0] SLM_MAGIC, [1] Q, [2] A, [3] K, [4..5] direct cells handed out (one 64-bit counter), [6] blank, [8..15] status
//   int4 rec[Q]      x: first cell of the state, y: its arcs (-1: a direct row of K cells), z: back-off state or -1, w: back-off weight bits
//   int raw[Q]       the back-off before the chain check (range-checked only)
//   int labels[A]    the labels of the arcs as given
//   int2 cells[5 A]  x: weight bits, y: next (-1 where it left [0, Q); SLM_MISS in a direct row: no arc).  The first A cells are the
//                    arcs in CSR order; behind them the direct rows, K cells each, of the states with at least K / 4 arcs: at most
//                    4 A cells as long as the states' arc ranges do not overlap, and a state that finds no room keeps its sorted arcs
constexpr int SLM_MAGIC = 0x314D4C53, SLM_MAXBACK = 8, SLM_MISS = -2;
// measured: a state with at least K / 4 arcs gets a direct row (0: no state does, every lookup is a binary search)
#ifndef KLSTM_SLM_DIRECT_DIV
#define KLSTM_SLM_DIRECT_DIV 4
#endif
static_assert(KLSTM_SLM_DIRECT_DIV >= 0 && KLSTM_SLM_DIRECT_DIV <= 4, "the blob holds 4 A cells of direct rows");
struct SlmLayout { size_t rec, raw, labels, cells, bytes; };
__host__ __device__ inline size_t slm_up16(size_t n) { return (n + 15) / 16 * 16; }
__host__ __device__ inline SlmLayout slm_layout(int Q, int A) {
  SlmLayout l;
  l.rec = 64;
  l.raw = l.rec + (size_t)Q * 16;
  l.labels = l.raw + slm_up16((size_t)Q * 4);
  l.cells = l.labels + slm_up16((size_t)A * 4);
  l.bytes = (l.cells + (size_t)A * 40 + 255) / 256 * 256;
  return l;
}
struct SlmView {
  const int4 *rec;
  const int *labels;
  const int2 *cells;
};
__device__ __forceinline__ SlmView slm_view(const void *blob, int Q) {
  const char *p = reinterpret_cast<const char *>(blob);
  const SlmLayout l = slm_layout(Q, reinterpret_cast<const int *>(p)[2]);
  return SlmView{reinterpret_cast<const int4 *>(p + l.rec), reinterpret_cast<const int *>(p + l.labels), reinterpret_cast<const int2 *>(p + l.cells)};
}
// sparse_lm_lookup of lm.py, bit for bit: (q, c) -> (g, n).  q in [0, Q), c in [0, K).  The build checked every index a walk
// follows; the trip count is bounded here whatever the blob holds.
__device__ __forceinline__ void slm_lookup(const SlmView &m, int q, int c, float &g, int &n) {
  float prod = 1.f;
  g = 0.f; n = -1;
  for (int it = 0; it <= SLM_MAXBACK; it++) {
    const int4 r = m.rec[q];
    int at = -1;                                                   // the cell of the arc, if the state has one for c
    if (r.y < 0) at = r.x + c;
    else {
      int lo = 0, hi = r.y;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m.labels[r.x + mid] < c) lo = mid + 1; else hi = mid;
      }
      if (lo < r.y && m.labels[r.x + lo] == c) at = r.x + lo;
    }
    if (at >= 0) {
      const int2 cell = m.cells[at];
      if (cell.y != SLM_MISS) {
        const float wt = __int_as_float(cell.x);
        g = it ? bmul(prod, wt) : wt;
        n = cell.y;
        return;
      }
    }
    if (r.z < 0) return;                                           // a miss without a back-off: forbidden
    prod = beam_emit(bmul(prod, beam_emit(__int_as_float(r.w))));
    q = r.z;
  }
}

}  // namespace klstm
