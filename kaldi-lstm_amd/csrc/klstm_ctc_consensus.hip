// kaldi-lstm_amd/csrc/klstm_ctc_consensus.hip -- minimum Bayes risk decoding and token / word confidences over CTC n-best lists
// (klstm_ctc_consensus of include/klstm.h; the numpy twin: tests/ctc_consensus_ref.py).  For every stream a list of
// hypotheses h_q with log probabilities l_q (the arrays klstm_ctc_beam_decode wrote, or hyp_logp of klstm_ctc_mbr_eval):
//   units of h_q: its tokens, or its words (the maximal runs of tokens other than the separator, known by their 64-bit beam_hash)
//   P_q = softmax_q(scale l_q),  D[q][r] = Levenshtein(units of h_q, units of h_r),  R_q = sum_r P_r D[q][r]
//   map = argmax_q scale l_q,  mbr = argmin_q R_q,  pick = the one the caller asked for
//   conf_u = sum_r P_r [unit u of h_pick is matched in THE alignment of h_pick against h_r]
// Five launches:
//   k_cons_keys   grid (N, S), one wave.  Is the entry live (klstm_ctc_nbest.h: the contract of a list); its unit count; word keys.
//   k_cons_dist   grid (pair blocks, S), four waves, one unordered pair (q <= r) each: the rows of edit_distance of klstm_ctc_dev.h
//                 (KLSTM_ED_ROW_STEP: columns across the lanes, P per lane, prefix minimum by wave_scan_min), the longer sequence across
//                 the lanes, P = 1 / 4 / 16 by its length.  Writes D[q][r] and D[r][q].
//   k_cons_pick   grid (S), one wave.  P, R, map, mbr, pick in double; every sum in index order.
//   k_cons_align  grid (N, S), one wave: the same rows with the pivot's units as rows and the entry's across the lanes, two bits of
//                 back-pointer per cell decided while the old and the new row are in registers.  A lane's bits of a row are one word
//                 that only this lane reads again: in LDS where the table fits CONS_LDS bytes, in the workspace otherwise.  The walk
//                 back fetches CONS_BR rows of words into registers at a time and steps by __shfl.
//   k_cons_conf   grid (S).  conf_u summed over r ascending by the thread of slot u; the stream's statistics; the last workgroup to
//                 arrive (ctc_last_arrival) adds the minibatch onto the totals, streams in order (KLSTM_NBEST_ADD_TOTALS).
// DETERMINISM.  No floating-point atomics, no reduction tree over floating-point values: bit-identical from run to run.
// The products and sums below are the twin's, one rounding each: no contraction into FMAs.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/klstm.h"
#include "klstm_ctc_host.h"
#include "klstm_ctc_nbest.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int CONS_LDS = 16384;        // bytes of back-pointers a wave keeps in LDS (256 rows of 64 bytes; 10 workgroups per CU)
constexpr int CONS_BR = 8;             // rows of back-pointer words the walk back holds in registers

struct ConsIn : NbestIn {};             // the caller's arrays; the ninth member is sep (its own type: the kernels keep their names)
// the workspace.  live [S N]; ulen [S N]; info [S]: 0 idle, 1 done, 2 rejected; pivot [S][4]: pick, map, mbr, entries dropped;
// P, R [S N] double; stat [S][8] double; match [S N][max_len] bytes; keys [S N][max_len] u64 (word mode); table [S N][max_len][64]
// words of 4 bytes (max_len > 255 only: below, every table fits LDS)
struct ConsWs { int *live, *ulen, *info, *pivot, *dist; unsigned *ticket; double *P, *R, *stat; unsigned char *match; u64 *keys; unsigned *table; };

static bool cons_table_in_lds(int max_len) { return max_len <= 255; }

static size_t cons_layout(int S, int N, int max_len, bool words, void *base, ConsWs &ws) {
  const size_t SN = (size_t)S * N, L = (size_t)(max_len > 0 ? max_len : 1);
  CtcCarver c(base);
  ws.ticket = c.take<unsigned>(64);
  ws.info = c.take<int>(S);
  ws.pivot = c.take<int>((size_t)S * 4);
  ws.live = c.take<int>(SN);
  ws.ulen = c.take<int>(SN);
  ws.P = c.take<double>(SN);
  ws.R = c.take<double>(SN);
  ws.stat = c.take<double>((size_t)S * 8);
  ws.dist = c.take<int>(SN * N);
  ws.match = c.take<unsigned char>(SN * L);
  ws.keys = words ? c.take<u64>(SN * L) : nullptr;
  ws.table = cons_table_in_lds(max_len) ? nullptr : c.take<unsigned>(SN * L * 64);
  return c.bytes();
}

size_t ctc_consensus_workspace_bytes(int S, int N, int max_len, int words) { ConsWs ws; return cons_layout(S, N, max_len, words != 0, nullptr, ws); }

// the unit keys of entry (s, q): its tokens, or its words' hashes in the workspace
template <class KT> struct ConsKeys;
template <> struct ConsKeys<int> {
  static __device__ __forceinline__ const int *of(const ConsIn &a, const ConsWs &, int se) { return a.hyp + (size_t)se * a.stride; }
};
template <> struct ConsKeys<u64> {
  static __device__ __forceinline__ const u64 *of(const ConsIn &a, const ConsWs &ws, int se) { return ws.keys + (size_t)se * a.max_len; }
};

// ------------------------------------------------------------------------------------------------------------------------------------
// Is the entry live, how many units has it, what are their keys.  One wave per entry.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cons_keys(ConsIn a, ConsWs ws, int *__restrict__ unit_len) {
  const int q = blockIdx.x, s = blockIdx.y, lane = threadIdx.x, se = s * a.N + q;
  if (se == 0 && lane == 0) *ws.ticket = 0u;                       // for k_cons_conf, three launches later
  KLSTM_NBEST_SHAPE(a, s, q, se, listed, live, len, lp)
  const int *h = a.hyp + (size_t)se * a.stride;
  if (live) KLSTM_NBEST_TOKENS(h, len, lane, v_ < 0, live)         // no K here: a token is a class if it is >= 0
  int units = 0;
  if (live && a.sep < 0) units = len;
  if (live && a.sep >= 0) {
    u64 *keys = ws.keys + (size_t)se * a.max_len;
    for (int t0 = 0; t0 < len; t0 += 64) {
      const int t = t0 + lane;
      const bool start = nbest_word_start(h, len, a.sep, t);
      const unsigned long long mask = __ballot(start);
      if (start) keys[units + nbest_word_slot(mask, lane)] = nbest_word_key(h, len, a.sep, t);     // the lane of a word's first token
      units += __popcll(mask);
    }
  }
  if (lane == 0) { ws.live[se] = live; ws.ulen[se] = units; unit_len[se] = units; }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The Levenshtein rows of one wave: those of edit_distance<P, false> of klstm_ctc_dev.h (KLSTM_ED_ROW_STEP) over unit keys.  Column j (0 .. Lc) of the row sits in
// lane j / P, slot j % P and carries cols[j - 1]; one row per unit of rows[0 .. Lr).  Returns D[Lr][Lc] in every lane.
// TRACE: row i (1 .. Lr) leaves its word of two bits per slot (KLSTM_ED_ROW_STEP) in tab[(i - 1) * 64 + lane].  Columns beyond Lc hold
// values nobody reads.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int P, class KT, bool TRACE, class W>
__device__ __forceinline__ int cons_rows(const KT *__restrict__ cols, int Lc, const KT *__restrict__ rows, int Lr, W *tab) {
  const int lane = threadIdx.x & 63;
  int prev[P];
  KT rl[P];
#pragma unroll
  for (int e = 0; e < P; e++) {
    const int j = lane * P + e;
    prev[e] = j;
    rl[e] = (j >= 1 && j <= Lc) ? cols[j - 1] : (KT)0;
  }
  int row = 0;
  for (int t0 = 0; t0 < Lr; t0 += 64) {
    const KT c = t0 + lane < Lr ? rows[t0 + lane] : (KT)0;
    const int n = Lr - t0 < 64 ? Lr - t0 : 64;
    for (int k = 0; k < n; k++) {
      const KT tok = __shfl(c, k);
      row++;
      KLSTM_ED_ROW_STEP(P, TRACE, prev, rl, tok, row, code)
      if (TRACE) tab[(size_t)(row - 1) * 64 + lane] = (W)code;
    }
  }
  int out = 0;
#pragma unroll
  for (int e = 0; e < P; e++) if (lane * P + e == Lc) out = prev[e];
  return __shfl(out, Lc / P);
}

// pair p of the N (N + 1) / 2 pairs q <= r, row by row
__device__ __forceinline__ void cons_pair(int p, int N, int &q, int &r) {
  q = 0;
  while (p >= N - q) { p -= N - q; q++; }
  r = q + p;
}

template <class KT>
__global__ __launch_bounds__(256) void k_cons_dist(ConsIn a, ConsWs ws, int *__restrict__ dist) {
  const int N = a.N, s = blockIdx.y, lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= N * (N + 1) / 2) return;                                // uniform over the wave
  int q, r;
  cons_pair(p, N, q, r);
  const int sq = s * N + q, sr = s * N + r;
  int d = -1;
  if (ws.live[sq] && ws.live[sr]) {
    d = 0;
    if (q != r) {
      const int lq = ws.ulen[sq], lr = ws.ulen[sr];
      const bool qlong = lq >= lr;                                 // the longer one across the lanes
      const KT *cols = ConsKeys<KT>::of(a, ws, qlong ? sq : sr), *rows = ConsKeys<KT>::of(a, ws, qlong ? sr : sq);
      const int Lc = qlong ? lq : lr, Lr = qlong ? lr : lq;
      if (Lc <= 63) d = cons_rows<1, KT, false, unsigned char>(cols, Lc, rows, Lr, nullptr);
      else if (Lc <= 255) d = cons_rows<4, KT, false, unsigned char>(cols, Lc, rows, Lr, nullptr);
      else d = cons_rows<16, KT, false, unsigned char>(cols, Lc, rows, Lr, nullptr);
    }
  }
  if (lane == 0) { dist[(size_t)sq * N + r] = d; dist[(size_t)sr * N + q] = d; }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Posteriors, risks and the pivot of one stream, in double, every sum in index order.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cons_pick(ConsIn a, ConsWs ws, float scale, int pivot_mode, const int *__restrict__ dist,
                                                  int *__restrict__ pick, int *__restrict__ map, int *__restrict__ mbr,
                                                  float *__restrict__ post, float *__restrict__ risk) {
  __shared__ double sP[64], sR[64];
  __shared__ int sh_st;
  const int s = blockIdx.x, tid = threadIdx.x, N = a.N;
  const int *live = ws.live + s * N;
  if (tid == 0) {
    const int cnt = a.count[s];
    int st = 1, nlive = 0;
    if (cnt < 0 || cnt > N) st = 2;
    else {
      for (int q = 0; q < cnt; q++) nlive += live[q];
      if (nlive == 0) st = 0;
    }
    double m = -INFINITY, Z = 0.0;
    if (st == 1) {
      for (int q = 0; q < N; q++) if (live[q]) m = fmax(m, (double)scale * (double)a.logp[s * N + q]);
      for (int q = 0; q < N; q++) {
        sP[q] = live[q] ? exp((double)scale * (double)a.logp[s * N + q] - m) : 0.0;
        if (live[q]) Z += sP[q];
      }
    }
    for (int q = 0; q < N; q++) {
      const double Pq = (st == 1 && live[q]) ? sP[q] / Z : 0.0;
      sP[q] = Pq;
      ws.P[s * N + q] = Pq;
      post[s * N + q] = (float)Pq;
    }
    ws.info[s] = st;
    ws.pivot[4 * s + 3] = st == 2 ? 0 : cnt - nlive;
    sh_st = st;
  }
  __syncthreads();
  const int st = sh_st;
  if (tid < N) {
    double R = -1.0;
    if (st == 1 && live[tid]) {
      R = 0.0;
      const int *drow = dist + (size_t)(s * N + tid) * N;
      for (int r = 0; r < N; r++) if (live[r]) R += sP[r] * (double)drow[r];
    }
    sR[tid] = R;
    ws.R[s * N + tid] = R;
    risk[s * N + tid] = (float)R;
  }
  __syncthreads();
  if (tid != 0) return;
  int imap = -1, imbr = -1;
  if (st == 1) {
    double zb = 0.0, rb = 0.0;
    for (int q = 0; q < N; q++) {
      if (!live[q]) continue;
      const double z = (double)scale * (double)a.logp[s * N + q];
      if (imap < 0 || z > zb) { imap = q; zb = z; }                // ties: the lowest q
      if (imbr < 0 || sR[q] < rb) { imbr = q; rb = sR[q]; }
    }
  }
  const int ipick = pivot_mode ? imbr : imap;
  map[s] = imap; mbr[s] = imbr; pick[s] = ipick;
  ws.pivot[4 * s] = ipick; ws.pivot[4 * s + 1] = imap; ws.pivot[4 * s + 2] = imbr;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The alignment of the pivot against one live entry by one wave: which of the pivot's slots are matched.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int P, class KT, class W>
__device__ __forceinline__ void cons_align(const KT *__restrict__ piv, int La, const KT *__restrict__ ent, int Lb, W *tab,
                                           unsigned char *__restrict__ match) {
  const int lane = threadIdx.x & 63;
  cons_rows<P, KT, true, W>(ent, Lb, piv, La, tab);
  unsigned m = 0;                                                  // slot u: lane u % 64, bit u / 64
  int i = La, j = Lb;                                              // uniform over the wave
  while (i > 0) {
    const int i0 = i;
    unsigned regs[CONS_BR];
#pragma unroll
    for (int k = 0; k < CONS_BR; k++) regs[k] = i0 - k >= 1 ? (unsigned)tab[(size_t)(i0 - k - 1) * 64 + lane] : 0u;
#pragma unroll
    for (int k = 0; k < CONS_BR; k++) {
      if (i != i0 - k || i <= 0) continue;                         // row i0 - k, until the walk leaves it
      for (;;) {
        const unsigned cell = ((unsigned)__shfl((int)regs[k], j / P) >> (2 * (j % P))) & 3u;
        if (cell == 3u && j > 0) { j--; continue; }                // left
        if (cell == 0u && lane == ((i - 1) & 63)) m |= 1u << ((i - 1) >> 6);
        if (cell <= 1u) j--;                                       // diagonal; otherwise up
        i--;
        break;
      }
    }
  }
  for (int u = lane; u < La; u += 64) match[u] = (unsigned char)((m >> (u >> 6)) & 1u);
}

template <class KT>
__global__ __launch_bounds__(64) void k_cons_align(ConsIn a, ConsWs ws) {
  __shared__ unsigned lds[CONS_LDS / 4];
  const int r = blockIdx.x, s = blockIdx.y, N = a.N, sr = s * N + r;
  if (ws.info[s] != 1 || !ws.live[sr]) return;                     // uniform
  const int sp = s * N + ws.pivot[4 * s];
  const int La = ws.ulen[sp], Lb = ws.ulen[sr];
  const KT *piv = ConsKeys<KT>::of(a, ws, sp), *ent = ConsKeys<KT>::of(a, ws, sr);
  unsigned char *match = ws.match + (size_t)sr * a.max_len;
  unsigned *gtab = ws.table ? ws.table + (size_t)sr * a.max_len * 64 : nullptr;      // La <= max_len rows of 64 words
  if (Lb <= 255) {                                                 // a byte per lane and row
    const bool fits = La * 64 <= CONS_LDS;                         // always, where there is no table in the workspace
    unsigned char *tab = fits ? reinterpret_cast<unsigned char *>(lds) : reinterpret_cast<unsigned char *>(gtab);
    if (Lb <= 63) cons_align<1, KT, unsigned char>(piv, La, ent, Lb, tab, match);
    else cons_align<4, KT, unsigned char>(piv, La, ent, Lb, tab, match);
  } else {
    unsigned *tab = La * 256 <= CONS_LDS ? lds : gtab;
    cons_align<16, KT, unsigned>(piv, La, ent, Lb, tab, match);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The confidences of the pivot's slots, the stream's statistics and, by the last workgroup to arrive, the totals.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cons_conf(ConsIn a, ConsWs ws, int S, float *__restrict__ conf, int conf_stride,
                                                   double *__restrict__ totals) {
  __shared__ double cd[1024];
  __shared__ double sP[64];
  __shared__ int slive[64];
  const int s = blockIdx.x, tid = threadIdx.x, N = a.N;
  const int st = ws.info[s];
  int ipick = -1, La = 0;
  if (st == 1) {
    ipick = ws.pivot[4 * s];
    La = ws.ulen[s * N + ipick];
    if (tid < N) { sP[tid] = ws.P[s * N + tid]; slive[tid] = ws.live[s * N + tid]; }
    __syncthreads();
    for (int u = tid; u < La; u += 256) {
      double c = 0.0;
      for (int r = 0; r < N; r++)
        if (slive[r] && ws.match[(size_t)(s * N + r) * a.max_len + u]) c += sP[r];
      cd[u] = c;
      conf[(size_t)s * conf_stride + u] = (float)c;
    }
    __syncthreads();
  }
  if (tid != 0 || !totals) return;
  double *stat = ws.stat + 8 * s;
  double csum = 0.0;
  for (int u = 0; u < La; u++) csum += cd[u];
  const int imap = st == 1 ? ws.pivot[4 * s + 1] : -1, imbr = st == 1 ? ws.pivot[4 * s + 2] : -1;
  stat[0] = st == 1 ? ws.R[s * N + ipick] : 0.0;
  stat[1] = st == 1 ? ws.R[s * N + imap] : 0.0;
  stat[2] = (st == 1 && imbr != imap) ? 1.0 : 0.0;
  stat[3] = (double)La;
  stat[4] = csum;
  stat[5] = (double)ws.pivot[4 * s + 3];
  stat[6] = (st == 1 && a.errors) ? (double)a.errors[s * N + ipick] : 0.0;
  stat[7] = (st == 1 && a.errors) ? (double)a.errors[s * N + imap] : 0.0;
  if (!ctc_last_arrival(ws.ticket, S)) return;
  KLSTM_NBEST_ADD_TOTALS(ws.info, ws.stat, S, 0, totals)
}

template <class KT>
static hipError_t cons_launch(const ConsIn &in, const ConsWs &ws, int S, float scale, int pivot_mode, int *pick, int *map, int *mbr,
                              float *post, float *risk, int *unit_len, float *conf, int conf_stride, int *dist, double *totals,
                              hipStream_t st) {
  const int N = in.N;
  hipError_t err = launch(k_cons_keys, dim3(N, S), dim3(64), 0, st, LaunchProbe{}, in, ws, unit_len);
  if (err != hipSuccess) return err;
  err = launch(k_cons_dist<KT>, dim3((N * (N + 1) / 2 + 3) / 4, S), dim3(256), 0, st, LaunchProbe{}, in, ws, dist);
  if (err != hipSuccess) return err;
  err = launch(k_cons_pick, dim3(S), dim3(64), 0, st, LaunchProbe{}, in, ws, scale, pivot_mode, (const int *)dist, pick, map, mbr, post, risk);
  if (err != hipSuccess) return err;
  err = launch(k_cons_align<KT>, dim3(N, S), dim3(64), 0, st, LaunchProbe{}, in, ws);
  if (err != hipSuccess) return err;
  return launch(k_cons_conf, dim3(S), dim3(256), 0, st, LaunchProbe{}, in, ws, S, conf, conf_stride, totals);
}

hipError_t launch_ctc_consensus(const int *hyp, int hyp_stride, const int *hyp_len, const int *count, const float *logp, const int *errors,
                                int S, int N, int max_len, float scale, int separator, int pivot_mode, int *pick, int *map, int *mbr,
                                float *post, float *risk, int *unit_len, float *conf, int conf_stride, int *dist, double *totals,
                                void *workspace, hipStream_t st) {
  const bool words = separator >= 0;
  ConsWs ws;
  cons_layout(S, N, max_len, words, workspace, ws);
  const ConsIn in{{hyp, hyp_len, count, logp, errors, hyp_stride, N, max_len, {words ? separator : -1}}};
  if (!dist) dist = ws.dist;
  if (words) return cons_launch<u64>(in, ws, S, scale, pivot_mode, pick, map, mbr, post, risk, unit_len, conf, conf_stride, dist, totals, st);
  return cons_launch<int>(in, ws, S, scale, pivot_mode, pick, map, mbr, post, risk, unit_len, conf, conf_stride, dist, totals, st);
}

}  // namespace klstm
