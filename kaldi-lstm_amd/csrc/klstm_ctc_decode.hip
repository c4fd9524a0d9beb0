// kaldi-lstm_amd/csrc/klstm_ctc_decode.hip -- CTC best-path decoding of whole utterances and the token error rate against reference
// label sequences (klstm_ctc_decode of include/klstm.h).  Two launches:
//   k_ctc_argmax_sub<LPR> / k_ctc_argmax_wg   one row (t, s) of the posterior matrix per group of LPR lanes / per workgroup:
//                  best = argmax_k key(y[k] * w[k]) as a (value, index) pair, reduced inside the wave with DPP and (workgroup per row)
//                  across the four waves through LDS.  Writes frame_class and frame_logp = log(max(y[best], FLT_MIN)).  Padding rows
//                  and the rows of idle / rejected streams are not read and get class -1.
//   k_ctc_collapse grid (S), 256 threads.  Stream s: the kept frames (class != blank and != the class of the frame before) are compacted
//                  in order into hyp[s*T ..) by a flag + prefix sum over chunks of 256 frames; the path score is summed in double
//                  (thread-strided partial sums, then a fixed tree); wave 0 then runs the Levenshtein recurrence against the
//                  reference, one row per hypothesis token, the whole row in the registers of ONE wave (no barrier on the chain).
//                  The workgroup that finishes last adds the minibatch's statistics onto the totals, streams in order.
// DETERMINISM.  No floating-point atomics; ties go to the lowest column by the comparison itself (the pair order is total), every sum is
// a fixed tree over a fixed workgroup size whose shape depends on the utterance's length alone, the edit distance is integer.
#include <cfloat>
#include <climits>
#include <cmath>

#include "../../include/klstm.h"
#include "klstm_ctc_dev.h"
#include "klstm_kernels.h"

namespace klstm {

__device__ __forceinline__ float ctc_key(float v) { return v == v ? v : -INFINITY; }      // a NaN never wins

// One row seen by lane `lane` of `nl` lanes (ctc_for_row of klstm_ctc_dev.h); w (or null): the class weights, indexed by column.
__device__ __forceinline__ Best scan_row(const float *__restrict__ yp, const float *__restrict__ w, int K, int lane, int nl) {
  Best b{-INFINITY, INT_MAX};
  ctc_for_row(yp, w, K, lane, nl, [&](float v, int c) { best_take(b, ctc_key(v), c); });
  return b;
}

__device__ __forceinline__ bool row_valid(int r, int T, int S, const int *__restrict__ lens) {
  const int s = r % S, t = r / S, len = lens[s];
  return len > 0 && len <= T && t < len;
}
__device__ __forceinline__ void put_row(int r, bool valid, int idx, const float *__restrict__ yp, int *__restrict__ fclass,
                                        float *__restrict__ flogp) {
  fclass[r] = valid ? idx : -1;
  flogp[r] = valid ? logf(fmaxf(yp[idx], FLT_MIN)) : 0.f;         // fmaxf(NaN, x) = x: a NaN winner (a row of nothing else) scores FLT_MIN
}

// 256 threads, 256 / LPR rows per workgroup, LPR = 16 or 64 lanes per row.  ticket: zeroed here for k_ctc_collapse.
template <int LPR>
__global__ __launch_bounds__(256) void k_ctc_argmax_sub(const float *__restrict__ y, int T, int S, int K, int stride,
                                                        const int *__restrict__ lens, const float *__restrict__ w, int *__restrict__ fclass,
                                                        float *__restrict__ flogp, unsigned *__restrict__ ticket) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;
  const int r = blockIdx.x * (256 / LPR) + threadIdx.x / LPR, lane = threadIdx.x % LPR;
  const bool inside = r < T * S;
  const bool valid = inside && row_valid(r, T, S, lens);
  const float *yp = y + (size_t)(inside ? r : 0) * stride;
  Best b{-INFINITY, INT_MAX};
  if (valid) b = scan_row(yp, w, K, lane, LPR);
  if (LPR == 16) row16_best(b); else wave_best(b);                // every lane takes part: DPP reads its neighbours' registers
  if (inside && lane == LPR - 1) put_row(r, valid, b.i, yp, fclass, flogp);
}

// one workgroup of four waves per row
__global__ __launch_bounds__(256) void k_ctc_argmax_wg(const float *__restrict__ y, int T, int S, int K, int stride,
                                                       const int *__restrict__ lens, const float *__restrict__ w, int *__restrict__ fclass,
                                                       float *__restrict__ flogp, unsigned *__restrict__ ticket) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r == 0 && tid == 0) *ticket = 0u;
  const float *yp = y + (size_t)r * stride;
  if (!row_valid(r, T, S, lens)) {                                 // uniform over the workgroup
    if (tid == 0) put_row(r, false, 0, yp, fclass, flogp);
    return;
  }
  Best b = scan_row(yp, w, K, tid, 256);
  wave_best(b);
  if ((tid & 63) == 63) { sv[tid >> 6] = b.v; si[tid >> 6] = b.i; }
  __syncthreads();
  if (tid == 0) {
    Best a{sv[0], si[0]};
    best_take(a, sv[1], si[1]); best_take(a, sv[2], si[2]); best_take(a, sv[3], si[3]);
    put_row(r, true, a.i, yp, fclass, flogp);
  }
}

struct CtcDecWs { int *fclass; float *flogp; int *stat; unsigned *ticket; };       // stat [S][4]: errors, ref tokens, hyp tokens, counted

__global__ __launch_bounds__(256) void k_ctc_collapse(const int *__restrict__ fclass, const float *__restrict__ flogp, int T, int S, int K,
                                                      const int *__restrict__ lens, int blank, int *__restrict__ hyp,
                                                      int *__restrict__ hyp_len, float *__restrict__ score, const int *__restrict__ refs,
                                                      const int *__restrict__ roff, int *__restrict__ errors, double *__restrict__ totals,
                                                      int *__restrict__ stat, unsigned *__restrict__ ticket) {
  __shared__ int wcnt[4];
  __shared__ double dsum[256];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int len = lens[s];
  if (len < 0 || len > T) len = 0;                                 // rejected: the outputs of an idle stream
  int H = 0, err = -1, L = 0;

  // collapse: chunks of 256 frames, kept frames written in order
  for (int t0 = 0; t0 < len; t0 += 256) {
    const int t = t0 + tid;
    const int c = t < len ? fclass[(size_t)t * S + s] : blank;
    const int cb = (t > 0 && t < len) ? fclass[(size_t)(t - 1) * S + s] : -1;
    const bool keep = c != blank && c != cb;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int base = H;
    for (int q = 0; q < wv; q++) base += wcnt[q];
    if (keep) hyp[(size_t)s * T + base + __popcll(m & ((1ull << lane) - 1ull))] = c;
    H += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  // path score: thread tid sums frames tid, tid + 256, ... in double, then a fixed tree
  double acc = 0.0;
  for (int t = tid; t < len; t += 256) acc += (double)flogp[(size_t)t * S + s];
  dsum[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) dsum[tid] += dsum[tid + o];
    __syncthreads();
  }
  // the reference: usable iff every label is a class other than the blank and there are at most 1023 of them
  bool scored = false;
  if (refs && len > 0) {
    const int o0 = roff[s];
    L = roff[s + 1] - o0;
    int bad = L < 0 || L > 1023;
    if (!bad)
      for (int j = tid; j < L; j += 256) {
        const int c = refs[o0 + j];
        bad |= (c < 0 || c >= K || c == blank);
      }
    scored = !__syncthreads_or(bad);
    if (scored && wv == 0) {
      const int *ref = refs + o0;
      err = L < 64 ? edit_distance<1>(fclass, S, s, len, blank, ref, L) : L < 256 ? edit_distance<4>(fclass, S, s, len, blank, ref, L)
                                                                                : edit_distance<16>(fclass, S, s, len, blank, ref, L);
    }
  }
  if (tid != 0) return;
  hyp_len[s] = H;
  if (score) score[s] = (float)dsum[0];
  if (errors) errors[s] = err;
  if (!totals) return;
  stat[4 * s] = err; stat[4 * s + 1] = L; stat[4 * s + 2] = H; stat[4 * s + 3] = scored;
  if (!ctc_last_arrival(ticket, S)) return;
  double e = 0, n = 0, h = 0, u = 0, w = 0;
  for (int q = 0; q < S; q++) {
    const int *st = stat + 4 * q;
    if (!__hip_atomic_load(st + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
    const int eq = __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e += eq; w += eq > 0; u += 1;
    n += __hip_atomic_load(st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    h += __hip_atomic_load(st + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  totals[0] += e; totals[1] += n; totals[2] += h; totals[3] += u; totals[4] += w;
}

static size_t dec_rows_bytes(int T, int S) { return ((size_t)T * S * sizeof(int) + 255) / 256 * 256; }

size_t ctc_decode_workspace_bytes(int T, int S) { return 2 * dec_rows_bytes(T, S) + 256 * 3; }    // frame_class, frame_logp, stat [32][4], ticket

hipError_t launch_ctc_decode(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int *hyp,
                             int *hyp_len, float *score, int *frame_class, const int *refs, const int *roff, int *errors, double *totals,
                             void *workspace, hipStream_t st) {
  char *p = reinterpret_cast<char *>(workspace);
  CtcDecWs ws;
  ws.fclass = frame_class ? frame_class : reinterpret_cast<int *>(p);
  ws.flogp = reinterpret_cast<float *>(p + dec_rows_bytes(T, S));
  ws.stat = reinterpret_cast<int *>(p + 2 * dec_rows_bytes(T, S));
  ws.ticket = reinterpret_cast<unsigned *>(p + 2 * dec_rows_bytes(T, S) + 512);
  const int rows = T * S;
  // measured: 16 lanes per row up to 256 classes (16.4 against 19.0 us at 32000 rows, K = 256), a wave per row beyond
  // (K = 2048, 8000 rows: 19.7 us where 16 lanes take 28.8), and a workgroup per row only where rows are too few for a wave each to
  // fill the device (1200 rows, K = 16624: 18.9 against 40.8 us; from 8000 rows on the wave per row is level or ahead)
  const int g = K <= 256 ? 16 : (K > 2048 && rows < 4096) ? 256 : 64;
  hipError_t err;
  if (g == 16)
    err = launch(k_ctc_argmax_sub<16>, dim3((rows + 15) / 16), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, ws.fclass, ws.flogp, ws.ticket);
  else if (g == 64)
    err = launch(k_ctc_argmax_sub<64>, dim3((rows + 3) / 4), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, ws.fclass, ws.flogp, ws.ticket);
  else
    err = launch(k_ctc_argmax_wg, dim3(rows), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, ws.fclass, ws.flogp, ws.ticket);
  if (err != hipSuccess) return err;
  return launch(k_ctc_collapse, dim3(S), dim3(256), 0, st, LaunchProbe{}, (const int *)ws.fclass, (const float *)ws.flogp, T, S, K, lens, blank, hyp,
                hyp_len, score, refs, roff, errors, totals, ws.stat, ws.ticket);
}

}  // namespace klstm
