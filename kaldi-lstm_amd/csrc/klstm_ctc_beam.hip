// kaldi-lstm_amd/csrc/klstm_ctc_beam.hip -- CTC prefix beam search over whole utterances with n-best lists, their scores and their edit
// distances (klstm_ctc_beam_decode of include/klstm.h; the definition is tests/ctc_beam_ref.py).  Three launches:
//   k_ctc_topc_sub<LPR> / k_ctc_topc_wg   one valid row (t, s) per group of LPR lanes / per workgroup: the C best non-blank
//                  (emission, column) pairs in descending order (larger value first, then the lower column), found by C rounds of the
//                  decoder's (value, index) reduction, each over the columns that come AFTER the winner of the round before.  The order
//                  is total, so the reduction tree does not matter.  Padding rows and idle / rejected streams are not read.
//   k_ctc_beam     grid (S), 64 to 256 threads: the frame chain of one stream.  Beam entries, the frame's list of up to B (C + 1) entries
//                  and its keys live in LDS.  A total is a non-negative float, so (float bits, ~list position) is ONE 64-bit integer
//                  key and selection is an integer rank: a key's place in the new beam is the number of keys above it.  Prefix-tree nodes (parent, token) go to the workspace, B a frame.
//                  After the last frame the first N live entries are written out: the prefix by walking the parents, the score.
//                  Its storage, lm_fetch, table staging and frame loop are the text of klstm_ctc_beam_frame.h, which the streaming
//                  kernel k_ctc_beam_stream below includes too: ONE frame body in source, compiled into both.
//   k_ctc_beam_tail grid (S), 256 threads, only with references: wave q % 4 runs the one-wave Levenshtein recurrence of
//                  klstm_ctc_dev.h for hypothesis q; the workgroup that finishes last adds the statistics onto the totals, streams in order.
// ARITHMETIC.  Every step on the chain is ONE float32 operation rounded to nearest (bmul / badd below: never contracted into an
// FMA); the per-frame rescale multiplies by a power of two.  Emissions and rescaled values below 2^-60 are exactly 0, so no product
// is ever denormal and the denormal mode of the device cannot matter.  The twin reproduces every bit.
// DETERMINISM.  No floating-point atomics; all state of a stream is its own.
// LANGUAGE MODEL (klstm_ctc_beam_decode_lm; the definition is tests/ctc_beam_lm_ref.py).  k_ctc_beam<LM>: 0 is the search
// without one, compiled to the code it was.  With a dense automaton (next, weight, final) a beam entry carries its state e_lm, and
// the extension of entry i by the candidate c is worth p * f, f = flush(e[c] * flush(weight[state_i][c])), 0 where next[state_i][c]
// leaves [0, Q).  The lookup depends on the beam just selected, so it is issued the moment the new states are in LDS -- right after the
// barrier that ends frame t, for the candidates of frame t + 1 that were prefetched a frame earlier -- and lands in REGISTERS of the
// thread that builds that very extension two barriers later (thread q % nt owns extension q in both places): the stay entries of
// frame t + 1 are computed under its latency.  The one reader of ANOTHER thread's factor would be the stay entry an extension
// merges into; there the roles are swapped: the stay entry leaves its slot number in merged[] and the extension's thread adds its
// value onto it (one extension per stay entry, so no race and the same two roundings).  LM = 1 reads the tables from global memory,
// LM = 2 from a copy staged into dynamic LDS at the start (ctc_beam_lm_resident decides); the two give the same bits.
// SPARSE BACK-OFF MODEL (klstm_ctc_slm_build, klstm_ctc_beam_decode_slm; the definition is sparse_lm_lookup of lm.py).
// LM = 3: the pair (weight, next) of an extension comes from slm_lookup, a walk over a back-off automaton that k_slm_* below built into
// one device blob from CSR arrays -- at most 9 states visited, a direct row or a binary search in each.  It is issued where the dense
// gather is and lands in the same registers; nothing downstream of lm_fetch knows which model it was.
#include <cfloat>
#include <climits>
#include <cmath>

#include "../../include/klstm.h"
#include "klstm_ctc_dev.h"
#include "klstm_kernels.h"

// hipcc contracts a * b + c into an FMA by default, and the header's __fmul_rn / __fadd_rn are plain operators that carry that
// licence with them when they are inlined.  The pragma governs the operators written BELOW it in this file: every product and every
// sum of the chain goes through bmul / badd, which therefore stay two instructions wherever they end up.
#pragma clang fp contract(off)

// bmul / badd, the emission rule beam_emit, the blob of a sparse back-off model and slm_lookup: shared with klstm_ctc_rescore.hip
#include "klstm_ctc_slm.h"

namespace klstm {

constexpr int BEAM_LMK = 8;            // extensions a thread builds at the largest list: 2048 over 256 threads
constexpr int BEAM_KPT = 9;            // keys a thread ranks at the largest list: 2112 entries over 256 threads
constexpr int BEAM_MAXB = 64, BEAM_MAXC = 32, BEAM_MAXLIST = 2114;      // B (C + 1) <= 2112, one more for the pair reads, even

__device__ __forceinline__ float beam_emit_at(const float *__restrict__ yp, const float *__restrict__ w, int k) {
  return beam_emit(w ? bmul(yp[k], w[k]) : yp[k]);
}
__device__ __forceinline__ bool beam_row_valid(int r, int T, int S, const int *__restrict__ lens) {
  const int s = r % S, t = r / S, len = lens[s];
  return len > 0 && len <= T && t < len;
}

// the best pair of the row that comes after `prev` in the order (and is not the blank), over the lanes' shares
__device__ __forceinline__ Best topc_scan(const float *__restrict__ yp, const float *__restrict__ w, int K, int blank, Best prev, int lane, int nl) {
  Best b{0.f, INT_MAX};
  ctc_for_row(yp, w, K, lane, nl, [&](float v, int c) {
    const float e = beam_emit(v);
    if (c != blank && (e < prev.v || (e == prev.v && c > prev.i))) best_take(b, e, c);
  });
  return b;
}

// 256 threads, 256 / LPR rows per workgroup, LPR = 16 or 64 lanes per row.  ticket: zeroed here for k_ctc_beam_tail.
template <int LPR>
__global__ __launch_bounds__(256) void k_ctc_topc_sub(const float *__restrict__ y, int T, int S, int K, int stride, const int *__restrict__ lens,
                                                      const float *__restrict__ w, int blank, int C, float *__restrict__ topv,
                                                      int *__restrict__ topi, unsigned *__restrict__ ticket) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;
  const int r = blockIdx.x * (256 / LPR) + threadIdx.x / LPR, lane = threadIdx.x % LPR;
  const bool inside = r < T * S;
  const bool valid = inside && beam_row_valid(r, T, S, lens);
  const float *yp = y + (size_t)(inside ? r : 0) * stride;
  Best prev{INFINITY, -1};
  for (int j = 0; j < C; j++) {                                     // every lane takes part: DPP reads its neighbours' registers
    Best b{0.f, INT_MAX};
    if (valid && prev.v > 0.f) b = topc_scan(yp, w, K, blank, prev, lane, LPR);
    if (LPR == 16) row16_best(b); else wave_best(b);
    const int src = (threadIdx.x & 63) | (LPR - 1);
    prev.v = __shfl(b.v, src);
    prev.i = __shfl(b.i, src);
    if (!(prev.v > 0.f)) { prev.v = 0.f; prev.i = -1; }
    if (valid && lane == LPR - 1) { topv[(size_t)r * C + j] = prev.v; topi[(size_t)r * C + j] = prev.i; }
  }
}

// one workgroup of four waves per row
__global__ __launch_bounds__(256) void k_ctc_topc_wg(const float *__restrict__ y, int T, int S, int K, int stride, const int *__restrict__ lens,
                                                     const float *__restrict__ w, int blank, int C, float *__restrict__ topv,
                                                     int *__restrict__ topi, unsigned *__restrict__ ticket) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (r == 0 && tid == 0) *ticket = 0u;
  if (!beam_row_valid(r, T, S, lens)) return;                      // uniform over the workgroup
  const float *yp = y + (size_t)r * stride;
  Best prev{INFINITY, -1};
  for (int j = 0; j < C; j++) {
    if (prev.v > 0.f) {                                            // uniform
      Best b = topc_scan(yp, w, K, blank, prev, tid, 256);
      wave_best(b);
      if ((tid & 63) == 63) { sv[tid >> 6] = b.v; si[tid >> 6] = b.i; }
      __syncthreads();
      Best a{sv[0], si[0]};
      best_take(a, sv[1], si[1]); best_take(a, sv[2], si[2]); best_take(a, sv[3], si[3]);
      __syncthreads();
      prev = a;
      if (!(prev.v > 0.f)) { prev.v = 0.f; prev.i = -1; }
    }
    if (tid == 0) { topv[(size_t)r * C + j] = prev.v; topi[(size_t)r * C + j] = prev.i; }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The search.  List position of the stay entry of beam entry i: i; of the extension of entry i by the candidate of rank r: Bc + i C + r.
// ------------------------------------------------------------------------------------------------------------------------------------
struct BeamLm {                         // the label language model: Q states, next / weight [Q][K], fin [Q] or null
  int Q;                                // LM = 3: next is the blob of klstm_ctc_slm_build, weight is not read
  const int *next;
  const float *weight, *fin;
};

// The n-best list of a beam, one wave (B <= 64: it sees the whole beam), under k_ctc_beam's epilogue and k_ctc_beam_emit.  tot: the
// lane's total, or tf = total * flush(final[state]).
// by tf, ties to the earlier beam position: the integer rank of the frame selection (tf >= 0: the bits order as the values do)
__device__ __forceinline__ int beam_tf_rank(float tot, int tid) {
  const unsigned mine = __float_as_uint(tot);
  int rank = 0;
  for (int j = 0; j < 64; j++) {
    const unsigned o = __shfl(mine, j);
    rank += (o > mine) || (o == mine && j < tid);
  }
  return rank;
}
// the lane's place in the list (N: not in it) and the list's length: the first N entries with a total > 0 in beam order, or by tf
// when `ranked` (uniform); none: the first entry alone, dead
__device__ __forceinline__ int beam_list_slot(float tot, bool ranked, int N, int tid, int &cnt) {
  const u64 live = __ballot(tot > 0.f);
  int slot = live ? (tot > 0.f ? __popcll(live & ((1ull << tid) - 1ull)) : N) : (tid == 0 ? 0 : N);
  if (ranked && live) {
    const int rank = beam_tf_rank(tot, tid);
    slot = tot > 0.f ? rank : N;
  }
  cnt = live ? min(N, (int)__popcll(live)) : 1;
  return slot;
}
__device__ __forceinline__ float beam_score(float tot, int E) {
  return tot > 0.f ? (float)badd(log((double)tot), bmul((double)E, 0.6931471805599453)) : -INFINITY;
}

// The frame body -- storage, lm_fetch, the staging of resident tables and the frame loop -- is the text of klstm_ctc_beam_frame.h, included here and in
// k_ctc_beam_stream part by part; KLSTM_BEAM_FRAME and KLSTM_BEAM_NODE are the two places where the kernels differ.
template <int LM>
__global__ __launch_bounds__(256) void k_ctc_beam(const float *__restrict__ y, int T, int S, int K, int stride, const int *__restrict__ lens,
                                                  const float *__restrict__ w, int blank, int B, int C, int N, const float *__restrict__ topv,
                                                  const int *__restrict__ topi, int *npar, int *ntok, int *hyp, int *__restrict__ hyp_len,
                                                  int *__restrict__ count, float *__restrict__ score, BeamLm lm) {
#define KLSTM_BEAM_PART 1
#include "klstm_ctc_beam_frame.h"

  const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  int len = lens[s];
  if (len < 0 || len > T) len = 0;                                 // rejected: the outputs of an idle stream
  if (len == 0) {
    if (tid == 0) count[s] = 0;
    return;
  }
  const size_t nbase = (size_t)s * ((size_t)T * B + 1);            // node 0 of the stream: the empty prefix
  for (int q = tid; q < BEAM_MAXB * BEAM_MAXC; q += nt) merged[q] = 0;
  if (tid == 0) {
    e_node[0] = 0; e_tok[0] = -1; e_len[0] = 0; e_hash[0] = BEAM_H0; e_ph[0] = 0; e_pb[0] = 1.f; e_pnb[0] = 0.f;
    npar[nbase] = -1; ntok[nbase] = -1;
  }
  int Bc = 1, E = 0;
  // the candidates and the blank's emission of a frame are fetched one frame ahead: their latency is off the chain
  float nv = 0.f, neb = beam_emit_at(y + (size_t)s * stride, w, blank);
  int ni = -1;
  if (tid < C) { nv = topv[(size_t)s * C + tid]; ni = topi[(size_t)s * C + tid]; }
#define KLSTM_BEAM_PART 2
#include "klstm_ctc_beam_frame.h"
  if constexpr (LM != 0) {
#define KLSTM_BEAM_PART 3
#include "klstm_ctc_beam_frame.h"
    if (tid == 0) e_lm[0] = 0;
    if (tid < C) { cvs[tid] = nv; cis[tid] = ni; }
    __syncthreads();
    lm_fetch(0, C);
  }

#define KLSTM_BEAM_FRAME t
#define KLSTM_BEAM_NODE(n) nbase + n
#define KLSTM_BEAM_PART 4
#include "klstm_ctc_beam_frame.h"
#undef KLSTM_BEAM_FRAME
#undef KLSTM_BEAM_NODE
  __syncthreads();
  __threadfence_block();                                           // the nodes other threads wrote
  if (tid >= 64) return;
  float tot = tid < Bc ? badd(e_pb[tid], e_pnb[tid]) : 0.f;
  bool ranked = false;
  if constexpr (LM != 0)
    if (lm.fin) {                                                  // uniform.  tot becomes tf = total * flush(final[state])
      if (tid < Bc) tot = bmul(tot, beam_emit(lm.fin[e_lm[(len & 1) * BEAM_MAXB + tid]]));
      ranked = true;
    }
  int cnt;
  const int slot = beam_list_slot(tot, ranked, N, tid, cnt);
  if (tid == 0) count[s] = cnt;
  if (slot >= N) return;
  const size_t o = (size_t)s * N + slot;
  const int ln = e_len[tid];
  hyp_len[o] = ln;
  if (score) score[o] = beam_score(tot, E);
  int node = e_node[tid];
  for (int q = ln - 1; q >= 0; q--) {                              // this launch wrote the nodes
    hyp[o * T + q] = __hip_atomic_load(ntok + nbase + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    node = __hip_atomic_load(npar + nbase + node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// stat [S][8]: 1-best errors, reference tokens, 1-best tokens, counted, oracle errors
__global__ __launch_bounds__(256) void k_ctc_beam_tail(const int *__restrict__ hyp, const int *__restrict__ hyp_len, const int *__restrict__ count,
                                                       int T, int S, int K, int N, int blank, const int *__restrict__ refs,
                                                       const int *__restrict__ roff, int *__restrict__ errors, double *__restrict__ totals,
                                                       int *__restrict__ stat, unsigned *__restrict__ ticket) {
  __shared__ int errs[BEAM_MAXB];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cnt = count[s];
  int L = 0;
  bool scored = false;
  if (cnt > 0) {                                                   // the reference: usable iff every label is a class other than the blank, at most 1023
    const int o0 = roff[s];
    L = roff[s + 1] - o0;
    int bad = L < 0 || L > 1023;
    if (!bad)
      for (int j = tid; j < L; j += 256) {
        const int c = refs[o0 + j];
        bad |= (c < 0 || c >= K || c == blank);
      }
    scored = !__syncthreads_or(bad);
    if (scored) {
      const int *ref = refs + o0;
      for (int q = wv; q < cnt; q += 4) {
        const int *h = hyp + ((size_t)s * N + q) * T;
        const int hl = hyp_len[(size_t)s * N + q];
        const int e = L < 64 ? edit_distance<1, false>(h, 1, 0, hl, -1, ref, L) : L < 256 ? edit_distance<4, false>(h, 1, 0, hl, -1, ref, L)
                                                                                 : edit_distance<16, false>(h, 1, 0, hl, -1, ref, L);
        if (lane == 0) errs[q] = e;
      }
    }
  }
  __syncthreads();
  if (errors)
    for (int q = tid; q < N; q += 256) errors[(size_t)s * N + q] = (scored && q < cnt) ? errs[q] : -1;
  if (tid != 0 || !totals) return;
  int oracle = 0;
  if (scored) {
    oracle = errs[0];
    for (int q = 1; q < cnt; q++) oracle = min(oracle, errs[q]);
  }
  int *st = stat + 8 * s;
  st[0] = scored ? errs[0] : 0; st[1] = L; st[2] = scored ? hyp_len[(size_t)s * N] : 0; st[3] = scored; st[4] = oracle;
  if (!ctc_last_arrival(ticket, S)) return;
  double e = 0, n = 0, h = 0, u = 0, wr = 0, orc = 0;
  for (int q = 0; q < S; q++) {
    const int *sq = stat + 8 * q;
    if (!__hip_atomic_load(sq + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
    const int eq = __hip_atomic_load(sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e += eq; wr += eq > 0; u += 1;
    n += __hip_atomic_load(sq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    h += __hip_atomic_load(sq + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    orc += __hip_atomic_load(sq + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  totals[0] += e; totals[1] += n; totals[2] += h; totals[3] += u; totals[4] += wr; totals[5] += orc;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Building the blob of a sparse back-off model, once per model (klstm_ctc_slm_build): four small launches in stream order.  Every
// index a walk of slm_lookup will follow is checked HERE, against Q, A and K, so that no content of the caller's arrays can send a
// search out of the blob.  status [8]: states dropped (they keep their back-off and lose their arcs) for [0] labels not strictly
// ascending, [1] a label outside [0, K), [2] a blank arc, [3] an arc range outside [0, A]; back-offs cut to -1 for [4] a target
// outside [-1, Q), [5] a chain of more than 8 back-offs (a cycle is one); [6] states that got a direct row.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_slm_arcs(int Q, int A, int K, int blank, const int *__restrict__ labels, const int *__restrict__ nxt,
                                                  const float *__restrict__ wt, void *blob) {
  char *p = reinterpret_cast<char *>(blob);
  const SlmLayout l = slm_layout(Q, A);
  int *hdr = reinterpret_cast<int *>(p);
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    const int t = threadIdx.x;
    hdr[t] = t == 0 ? SLM_MAGIC : t == 1 ? Q : t == 2 ? A : t == 3 ? K : t == 6 ? blank : 0;
  }
  int *lab = reinterpret_cast<int *>(p + l.labels);
  int2 *cells = reinterpret_cast<int2 *>(p + l.cells);
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < (size_t)A; j += (size_t)gridDim.x * 256) {
    const int n = nxt[j];
    lab[j] = labels[j];
    cells[j] = make_int2(__float_as_int(wt[j]), (unsigned)n < (unsigned)Q ? n : -1);
  }
}

// one thread per state: its arcs checked, its record, its direct row
__global__ __launch_bounds__(256) void k_slm_states(int Q, int A, int K, int blank, const int *__restrict__ off, const int *__restrict__ labels,
                                                    const int *__restrict__ backoff, const float *__restrict__ bow, void *blob) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  char *p = reinterpret_cast<char *>(blob);
  const SlmLayout l = slm_layout(Q, A);
  int *hdr = reinterpret_cast<int *>(p), *status = hdr + 8;
  int2 *cells = reinterpret_cast<int2 *>(p + l.cells);
  int b = off[q], e = off[q + 1], why = -1;
  if (b < 0 || e < b || e > A) why = 3;
  else
    for (int j = b, prev = -1; j < e; j++) {                       // ascending inside [0, K): at most K arcs are read
      const int c = labels[j];
      if (c < 0 || c >= K) why = 1;
      else if (c == blank) why = 2;
      else if (c <= prev) why = 0;
      if (why >= 0) break;
      prev = c;
    }
  if (why >= 0) { atomicAdd(status + why, 1); b = e = 0; }
  int deg = e - b, bo = backoff[q];
  if (bo < -1 || bo >= Q) { atomicAdd(status + 4, 1); bo = -1; }
  if (KLSTM_SLM_DIRECT_DIV > 0 && deg > 0 && (long)deg * KLSTM_SLM_DIRECT_DIV >= K) {      // a direct row, if there is room: K <= 4 deg cells
    const u64 at = atomicAdd(reinterpret_cast<u64 *>(hdr + 4), (u64)K);
    if (at + (u64)K <= (u64)4 * (u64)A) {
      int2 *row = cells + (size_t)A + (size_t)at;
      for (int c = 0; c < K; c++) row[c] = make_int2(0, SLM_MISS);
      for (int j = b; j < e; j++) row[labels[j]] = cells[j];       // k_slm_arcs wrote them: an earlier launch
      atomicAdd(status + 6, 1);
      b = A + (int)at; deg = -1;
    }
  }
  reinterpret_cast<int4 *>(p + l.rec)[q] = make_int4(b, deg, bo, __float_as_int(bow[q]));
  reinterpret_cast<int *>(p + l.raw)[q] = bo;
}

// one thread per state: a back-off whose chain does not end within SLM_MAXBACK states is cut.  Decided on the range-checked back-offs
// of k_slm_states alone, so the outcome does not depend on the order the threads run in
__global__ __launch_bounds__(256) void k_slm_chains(int Q, int A, void *blob) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  char *p = reinterpret_cast<char *>(blob);
  const SlmLayout l = slm_layout(Q, A);
  int *status = reinterpret_cast<int *>(p) + 8;
  if (q < Q) {
    const int *raw = reinterpret_cast<const int *>(p + l.raw);
    int d = 0;
    for (int s = raw[q]; s >= 0 && d <= SLM_MAXBACK; s = raw[s]) d++;
    if (d > SLM_MAXBACK) {
      reinterpret_cast<int4 *>(p + l.rec)[q].z = -1;
      atomicAdd(status + 5, 1);
    }
  }
}

__global__ void k_slm_status(const void *blob, int *__restrict__ status_out) {
  if (threadIdx.x < 8) status_out[threadIdx.x] = reinterpret_cast<const int *>(blob)[8 + threadIdx.x];
}

size_t ctc_slm_bytes(int Q, int A) { return slm_layout(Q, A).bytes; }

hipError_t launch_ctc_slm_build(int Q, int A, int K, int blank, const int *off, const int *labels, const int *nxt, const float *wt,
                                const int *backoff, const float *bow, void *blob, int *status, hipStream_t st) {
  const int gq = (Q + 255) / 256, ga = min((A + 255) / 256, 4096);
  hipError_t err = launch(k_slm_arcs, dim3(ga), dim3(256), 0, st, LaunchProbe{}, Q, A, K, blank, labels, nxt, wt, blob);
  if (err != hipSuccess) return err;
  err = launch(k_slm_states, dim3(gq), dim3(256), 0, st, LaunchProbe{}, Q, A, K, blank, off, labels, backoff, bow, blob);
  if (err != hipSuccess) return err;
  err = launch(k_slm_chains, dim3(gq), dim3(256), 0, st, LaunchProbe{}, Q, A, blob);
  if (err != hipSuccess || !status) return err;
  return launch(k_slm_status, dim3(1), dim3(64), 0, st, LaunchProbe{}, (const void *)blob, status);
}

static size_t up256(size_t n) { return (n + 255) / 256 * 256; }
static size_t beam_top_bytes(int T, int S, int C) { return up256((size_t)T * S * C * sizeof(int)); }
static size_t beam_node_bytes(int T, int S, int B) { return up256(((size_t)T * B + 1) * S * sizeof(int)); }

// top values, top columns, node parents, node tokens, stat [32][8], ticket
size_t ctc_beam_workspace_bytes(int T, int S, int B, int C) { return 2 * beam_top_bytes(T, S, C) + 2 * beam_node_bytes(T, S, B) + 1024 + 256; }

// measured (T = 1000, K = 64, tables of 33 to 124 KB): resident tables are level with the gather at beam 4 / 4 and 16 / 8 and
// 0.3 to 0.7 us a frame ahead at 64 / 32 at EVERY size that fits (122.7 against 123.2 at S = 8, 96 KB), so there is no crossover in table
// size: resident whenever the tables fit beside the search's own 31 KB of LDS with room to spare
#ifndef KLSTM_BEAM_LM_RESIDENT_BYTES
#define KLSTM_BEAM_LM_RESIDENT_BYTES (96 * 1024)
#endif
bool ctc_beam_lm_resident(int Q, int K, int B, int C) {
  (void)B; (void)C;
  return (size_t)Q * K * 8 <= (size_t)KLSTM_BEAM_LM_RESIDENT_BYTES;
}

// the row top-C of T * S rows; zeroes the ticket of k_ctc_beam_tail
static hipError_t launch_ctc_topc(const float *y, int T, int S, int K, int stride, const int *lens, const float *w, int blank, int C, float *topv,
                                  int *topi, unsigned *ticket, hipStream_t st) {
  const int rows = T * S;
  // measured (T = 1000, S = 32, C = 32): 16 lanes per row up to 256 classes (level with the others), a wave per row up to
  // 2048 (K = 1024: 11.7 against 11.8 and 12.1 ms a call), a workgroup per row beyond: the C passes over a long row stay in the
  // caches of ONE compute unit (K = 16624: 22.6 against 25.1 ms; 1200 rows: 3.9 against 4.9 ms; level at K = 4096)
  if (K <= 256)
    return launch(k_ctc_topc_sub<16>, dim3((rows + 15) / 16), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, blank, C, topv, topi, ticket);
  if (K <= 2048)
    return launch(k_ctc_topc_sub<64>, dim3((rows + 3) / 4), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, blank, C, topv, topi, ticket);
  return launch(k_ctc_topc_wg, dim3(rows), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, w, blank, C, topv, topi, ticket);
}

// measured: a list that fits one or two waves is served fastest by just those (2.2 against 2.4 us a frame at B = 4,
// C = 4); beyond 128 entries four waves, and BEAM_KPT keys a thread need all 256 threads at the largest list
static int beam_threads(int B, int C) { return B * (C + 1) <= 64 ? 64 : B * (C + 1) <= 128 ? 128 : 256; }

// One of the four instances of a search kernel template, grid (S): without an LM (Q = 0), gathering its tables, with the tables
// resident in dynamic LDS (ctc_beam_lm_resident decides), or walking a sparse back-off model in global memory.  args: the kernel's own.
template <class Kern, class... A>
static hipError_t launch_beam_chain(Kern none, Kern gathered, Kern resident, Kern sparse, bool is_sparse, int S, int K, int B, int C, int Q,
                                    hipStream_t st, A... args) {
  const dim3 grid(S), block(beam_threads(B, C));
  if (is_sparse) return launch(sparse, grid, block, 0, st, LaunchProbe{}, args...);
  if (Q == 0) return launch(none, grid, block, 0, st, LaunchProbe{}, args...);
  if (!ctc_beam_lm_resident(Q, K, B, C)) return launch(gathered, grid, block, 0, st, LaunchProbe{}, args...);
  // about 32 KB of static LDS come on top: past 64 KB in all the kernel needs the opt-in that launch() applies to the dynamic part alone
  const size_t dyn = (size_t)Q * K * 8;
  if (dyn > 32 * 1024 && dyn <= 64 * 1024) {
    const hipError_t err = raise_lds_limit(reinterpret_cast<const void *>(resident), dyn);
    if (err != hipSuccess) return err;
  }
  return launch(resident, grid, block, dyn, st, LaunchProbe{}, args...);
}

static hipError_t launch_ctc_beam_any(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int B, int C,
                                      int N, BeamLm lm, bool sparse, int *hyp, int *hyp_len, int *count, float *score, const int *refs,
                                      const int *roff, int *errors, double *totals, void *workspace, hipStream_t st);

hipError_t launch_ctc_beam(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int B, int C, int N,
                           int *hyp, int *hyp_len, int *count, float *score, const int *refs, const int *roff, int *errors, double *totals,
                           void *workspace, hipStream_t st) {
  return launch_ctc_beam_lm(y, T, S, K, stride, lens, blank, w, B, C, N, 0, nullptr, nullptr, nullptr, hyp, hyp_len, count, score, refs, roff,
                            errors, totals, workspace, st);
}

// Q = 0: no language model
hipError_t launch_ctc_beam_lm(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int B, int C, int N,
                              int Q, const int *lm_next, const float *lm_weight, const float *lm_final, int *hyp, int *hyp_len, int *count,
                              float *score, const int *refs, const int *roff, int *errors, double *totals, void *workspace, hipStream_t st) {
  return launch_ctc_beam_any(y, T, S, K, stride, lens, blank, w, B, C, N, BeamLm{Q, lm_next, lm_weight, lm_final}, false, hyp, hyp_len, count,
                             score, refs, roff, errors, totals, workspace, st);
}

// slm: the blob klstm_ctc_slm_build wrote for Q states
hipError_t launch_ctc_beam_slm(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int B, int C, int N,
                               int Q, const void *slm, const float *lm_final, int *hyp, int *hyp_len, int *count, float *score,
                               const int *refs, const int *roff, int *errors, double *totals, void *workspace, hipStream_t st) {
  return launch_ctc_beam_any(y, T, S, K, stride, lens, blank, w, B, C, N, BeamLm{Q, reinterpret_cast<const int *>(slm), nullptr, lm_final}, true,
                             hyp, hyp_len, count, score, refs, roff, errors, totals, workspace, st);
}

static hipError_t launch_ctc_beam_any(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const float *w, int B, int C,
                                      int N, BeamLm lm, bool sparse, int *hyp, int *hyp_len, int *count, float *score, const int *refs,
                                      const int *roff, int *errors, double *totals, void *workspace, hipStream_t st) {
  char *p = reinterpret_cast<char *>(workspace);
  float *topv = reinterpret_cast<float *>(p);
  int *topi = reinterpret_cast<int *>(p + beam_top_bytes(T, S, C));
  int *npar = reinterpret_cast<int *>(p + 2 * beam_top_bytes(T, S, C));
  int *ntok = reinterpret_cast<int *>(p + 2 * beam_top_bytes(T, S, C) + beam_node_bytes(T, S, B));
  int *stat = reinterpret_cast<int *>(p + 2 * beam_top_bytes(T, S, C) + 2 * beam_node_bytes(T, S, B));
  unsigned *ticket = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(stat) + 1024);
  hipError_t err = launch_ctc_topc(y, T, S, K, stride, lens, w, blank, C, topv, topi, ticket, st);
  if (err != hipSuccess) return err;
  err = launch_beam_chain(k_ctc_beam<0>, k_ctc_beam<1>, k_ctc_beam<2>, k_ctc_beam<3>, sparse, S, K, B, C, lm.Q, st, y, T, S, K, stride, lens, w, blank, B,
                          C, N, (const float *)topv, (const int *)topi, npar, ntok, hyp, hyp_len, count, score, lm);
  if (err != hipSuccess || !refs) return err;
  return launch(k_ctc_beam_tail, dim3(S), dim3(256), 0, st, LaunchProbe{}, (const int *)hyp, (const int *)hyp_len, (const int *)count, T, S, K, N,
                blank, refs, roff, errors, totals, stat, ticket);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// STREAMING (klstm_ctc_beam_stream_step / _emit of include/klstm.h; the definition is tests/ctc_beam_stream_ref.py).  The
// search above is a frame chain whose whole carried state is Bc, E and at most 64 beam entries plus the prefix tree, so it can stop at
// any frame boundary and go on in another launch with the same bits.  k_ctc_beam_stream<LM> is the frame loop of k_ctc_beam over the
// frames of one CHUNK, between a load and a store of that state; k_ctc_beam_emit<LM> is its epilogue as a kernel of its own, which
// only reads the state and shares the list rule (beam_list_slot, beam_score) with it.  The frame body is k_ctc_beam's: the same text,
// klstm_ctc_beam_frame.h, compiled into both kernels, with the frame's index and the place of a node as the two macros each kernel
// sets.  Shared TEXT, not a shared function: one __forceinline__ body under both kernels was built and measured, and missed the
// speed bar in the small-beam LM cells (profiles/ctc_beam_shared_body_ab.json); the included text compiles to the
// instructions the two copies had (profiles/ctc_beam_one_body_isa.txt).  The prologues and epilogues differ and stay here.
// State of stream s at state + s * beam_state_stride(max_frames, B):
//   int hdr[16]          [0] BEAM_STARTED once a step began an utterance here, [1] frames consumed, [2] Bc, [3] E, [4] overflow flag
//   u64 hash[64], ph[64]; int node[64], tok[64], len[64], lm[64]; float pb[64], pnb[64]          the beam entries, Bc of them valid
//   int npar[max_frames B + 1], ntok[max_frames B + 1]                                           the prefix tree, node 0 the empty prefix
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int BEAM_STARTED = 0x4B435442;
constexpr size_t BEAM_STATE_HEAD = 2816;                            // 64 + 2 * 512 + 6 * 256 = 2624, rounded up to 256

struct BeamState {
  int *hdr;
  u64 *hash, *ph;
  int *node, *tok, *len, *lm;
  float *pb, *pnb;
  int *npar, *ntok;
};
__host__ __device__ inline size_t beam_tree_bytes(int max_frames, int B) { return (((size_t)max_frames * B + 1) * sizeof(int) + 255) / 256 * 256; }
__host__ __device__ inline size_t beam_state_stride(int max_frames, int B) { return BEAM_STATE_HEAD + 2 * beam_tree_bytes(max_frames, B); }
__device__ __forceinline__ BeamState beam_state_at(void *state, int s, int max_frames, int B) {
  char *p = reinterpret_cast<char *>(state) + (size_t)s * beam_state_stride(max_frames, B);
  BeamState b;
  b.hdr = reinterpret_cast<int *>(p);
  b.hash = reinterpret_cast<u64 *>(p + 64);
  b.ph = b.hash + BEAM_MAXB;
  b.node = reinterpret_cast<int *>(p + 64 + 1024);
  b.tok = b.node + BEAM_MAXB; b.len = b.tok + BEAM_MAXB; b.lm = b.len + BEAM_MAXB;
  b.pb = reinterpret_cast<float *>(b.lm + BEAM_MAXB);
  b.pnb = b.pb + BEAM_MAXB;
  b.npar = reinterpret_cast<int *>(p + BEAM_STATE_HEAD);
  b.ntok = reinterpret_cast<int *>(p + BEAM_STATE_HEAD + beam_tree_bytes(max_frames, B));
  return b;
}

// T, lens: the frames of this chunk; topv / topi: the candidates of its rows
template <int LM>
__global__ __launch_bounds__(256) void k_ctc_beam_stream(const float *__restrict__ y, int T, int S, int K, int stride, const int *__restrict__ lens,
                                                         const int *__restrict__ start, const float *__restrict__ w, int blank, int B, int C,
                                                         const float *__restrict__ topv, const int *__restrict__ topi, void *state,
                                                         int max_frames, BeamLm lm) {
#define KLSTM_BEAM_PART 1
#include "klstm_ctc_beam_frame.h"

  const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int len = lens[s];
  if (len <= 0 || len > T) return;                                 // idle (or rejected) in this call: the state is not touched
  const BeamState bs = beam_state_at(state, s, max_frames, B);
  const bool fresh = bs.hdr[0] != BEAM_STARTED || (start && start[s] != 0);
  const int t0 = fresh ? 0 : bs.hdr[1];
  if (t0 < 0 || t0 > max_frames || len > max_frames - t0) {        // uniform.  Overflow: the flag alone, which no thread above reads
    if (tid == 0) bs.hdr[4] = 1;
    return;
  }
  int *const npar = bs.npar, *const ntok = bs.ntok;
  int Bc = 1, E = 0;
  for (int q = tid; q < BEAM_MAXB * BEAM_MAXC; q += nt) merged[q] = 0;
  if (fresh) {
    if (tid == 0) {
      e_node[0] = 0; e_tok[0] = -1; e_len[0] = 0; e_hash[0] = BEAM_H0; e_ph[0] = 0; e_pb[0] = 1.f; e_pnb[0] = 0.f;
      npar[0] = -1; ntok[0] = -1;
      if constexpr (LM != 0) e_lm[0] = 0;
    }
  } else {
    Bc = min(max(bs.hdr[2], 1), B);
    E = bs.hdr[3];
    if (tid < Bc) {
      e_node[tid] = bs.node[tid]; e_tok[tid] = bs.tok[tid]; e_len[tid] = bs.len[tid]; e_hash[tid] = bs.hash[tid]; e_ph[tid] = bs.ph[tid];
      e_pb[tid] = bs.pb[tid]; e_pnb[tid] = bs.pnb[tid];
      if constexpr (LM != 0) e_lm[tid] = min(max(bs.lm[tid], 0), lm.Q - 1);
    }
  }
  // the prefetches restart at the chunk's first frame as k_ctc_beam starts at frame 0: a value fetched a frame later is the same value
  float nv = 0.f, neb = beam_emit_at(y + (size_t)s * stride, w, blank);
  int ni = -1;
  if (tid < C) { nv = topv[(size_t)s * C + tid]; ni = topi[(size_t)s * C + tid]; }
#define KLSTM_BEAM_PART 2
#include "klstm_ctc_beam_frame.h"
  if constexpr (LM != 0) {
#define KLSTM_BEAM_PART 3
#include "klstm_ctc_beam_frame.h"
    if (tid < C) { cvs[tid] = nv; cis[tid] = ni; }
    __syncthreads();
    lm_fetch(0, Bc * C);
  }

#define KLSTM_BEAM_FRAME (t0 + t)                                   // t0 + t < max_frames
#define KLSTM_BEAM_NODE(n) n
#define KLSTM_BEAM_PART 4
#include "klstm_ctc_beam_frame.h"
#undef KLSTM_BEAM_FRAME
#undef KLSTM_BEAM_NODE
  __syncthreads();
  if (tid < Bc) {                                                  // the beam goes back where the next step, or an emit, finds it
    bs.node[tid] = e_node[tid]; bs.tok[tid] = e_tok[tid]; bs.len[tid] = e_len[tid]; bs.hash[tid] = e_hash[tid]; bs.ph[tid] = e_ph[tid];
    bs.pb[tid] = e_pb[tid]; bs.pnb[tid] = e_pnb[tid];
    if constexpr (LM != 0) bs.lm[tid] = e_lm[(len & 1) * BEAM_MAXB + tid];
    else bs.lm[tid] = 0;
  }
  if (tid == 0) {
    bs.hdr[0] = BEAM_STARTED; bs.hdr[1] = t0 + len; bs.hdr[2] = Bc; bs.hdr[3] = E;
    if (fresh) bs.hdr[4] = 0;
  }
}

// One wave per stream: the n-best list of the saved beam as k_ctc_beam's epilogue writes it, the frames consumed and the length of
// the prefix all live entries share.  Reads the state, writes none of it.  tcount: the counts k_ctc_beam_tail sees (mode 2 alone).
template <int LM>
__global__ __launch_bounds__(64) void k_ctc_beam_emit(int S, int B, int N, const int *__restrict__ mode, const float *__restrict__ fin,
                                                      void *state, int max_frames, int *__restrict__ hyp, int hyp_stride,
                                                      int *__restrict__ hyp_len, int *__restrict__ count, float *__restrict__ score,
                                                      int *__restrict__ frames, int *__restrict__ stable, int *__restrict__ tcount,
                                                      unsigned *__restrict__ ticket) {
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s == 0 && tid == 0) *ticket = 0u;                            // for k_ctc_beam_tail
  const BeamState bs = beam_state_at(state, s, max_frames, B);
  const bool started = bs.hdr[0] == BEAM_STARTED;
  const int m = mode[s], nfr = started ? bs.hdr[1] : 0;
  if (tid == 0 && frames) frames[s] = bs.hdr[4] ? -1 - nfr : nfr;
  if (m < 1 || m > 2 || !started) {                                // skipped, or nothing yet: no list
    if (tid == 0) {
      count[s] = 0; tcount[s] = 0;
      if (stable && m >= 1 && m <= 2) stable[s] = 0;
    }
    return;
  }
  const int Bc = min(max(bs.hdr[2], 1), B), E = bs.hdr[3];
  const float tot0 = tid < Bc ? badd(bs.pb[tid], bs.pnb[tid]) : 0.f;
  float tot = tot0;
  bool ranked = false;
  if constexpr (LM != 0)
    if (m == 2 && fin) {                                           // uniform.  tot becomes tf = total * flush(final[state])
      if (tid < Bc) tot = bmul(tot, beam_emit(fin[bs.lm[tid]]));
      ranked = true;
    }
  int cnt;
  const int slot = beam_list_slot(tot, ranked, N, tid, cnt);
  if (tid == 0) { count[s] = cnt; tcount[s] = m == 2 ? cnt : 0; }
  const int myln = tid < Bc ? bs.len[tid] : 0, mynode = tid < Bc ? bs.node[tid] : 0;
  if (slot < N) {
    const size_t o = (size_t)s * N + slot;
    hyp_len[o] = myln;
    if (score) score[o] = beam_score(tot, E);
    int node = mynode;
    for (int q = myln - 1; q >= 0; q--) {
      hyp[o * hyp_stride + q] = bs.ntok[node];
      node = bs.npar[node];
    }
  }
  if (!stable) return;
  // the longest common prefix of the entries with a total > 0, token by token: the same prefix can own two nodes (it left the beam
  // and came back), so equal nodes end the walk but unequal ones decide nothing
  const u64 live0 = __ballot(tot0 > 0.f);
  if (!live0) {                                                    // DEAD: the first entry
    if (tid == 0) stable[s] = myln;
    return;
  }
  const bool lv = tot0 > 0.f;
  int d = lv ? myln : INT_MAX;
  for (int off = 32; off > 0; off >>= 1) d = min(d, __shfl_xor(d, off));
  int node = lv ? mynode : 0;
  for (int q = lv ? myln - d : 0; q > 0; q--) node = bs.npar[node];           // every live lane up to the shortest live length
  const int first = __ffsll((long long)live0) - 1;
  int ans = d;
  while (d > 0) {
    const int n0 = __shfl(node, first);
    if (!__ballot(lv && node != n0)) break;                        // one node: one prefix from here up
    const int tk = lv ? bs.ntok[node] : 0, tk0 = __shfl(tk, first);
    if (__ballot(lv && tk != tk0)) ans = d - 1;                     // token d disagrees: at most d - 1 are common
    if (lv) node = bs.npar[node];
    d--;
  }
  if (tid == 0) stable[s] = ans;
}

size_t ctc_beam_stream_state_bytes(int max_frames, int S, int B) { return (size_t)S * beam_state_stride(max_frames, B); }

// statistics [32][8] (1024), ticket (256), the tail's counts [32] (256), then top values, top columns of the chunk's rows
constexpr size_t BEAM_STREAM_WS_HEAD = 1536;
size_t ctc_beam_stream_workspace_bytes(int T, int S, int C, int N) {
  (void)N;
  return BEAM_STREAM_WS_HEAD + 2 * beam_top_bytes(T, S, C);
}
size_t ctc_beam_stream_emit_workspace_bytes() { return BEAM_STREAM_WS_HEAD; }

// sparse: lm_next is the blob klstm_ctc_slm_build wrote for Q states, lm_weight is not read
hipError_t launch_ctc_beam_stream_step(const float *y, int T, int S, int K, int stride, const int *lens, const int *start, int blank,
                                       const float *w, int B, int C, int Q, const int *lm_next, const float *lm_weight, bool sparse, void *state,
                                       int max_frames, void *workspace, hipStream_t st) {
  char *p = reinterpret_cast<char *>(workspace);
  unsigned *ticket = reinterpret_cast<unsigned *>(p + 1024);
  float *topv = reinterpret_cast<float *>(p + BEAM_STREAM_WS_HEAD);
  int *topi = reinterpret_cast<int *>(p + BEAM_STREAM_WS_HEAD + beam_top_bytes(T, S, C));
  const hipError_t err = launch_ctc_topc(y, T, S, K, stride, lens, w, blank, C, topv, topi, ticket, st);
  if (err != hipSuccess) return err;
  return launch_beam_chain(k_ctc_beam_stream<0>, k_ctc_beam_stream<1>, k_ctc_beam_stream<2>, k_ctc_beam_stream<3>, sparse, S, K, B, C, Q, st, y, T, S, K,
                           stride, lens, start, w, blank, B, C, (const float *)topv, (const int *)topi, state, max_frames,
                           BeamLm{Q, lm_next, lm_weight, nullptr});
}

hipError_t launch_ctc_beam_stream_emit(int S, int K, int blank, int B, int N, const int *mode, int Q, const float *lm_final, const void *state,
                                       int max_frames, int *hyp, int hyp_stride, int *hyp_len, int *count, float *score, int *frames,
                                       int *stable, const int *refs, const int *roff, int *errors, double *totals, void *workspace,
                                       hipStream_t st) {
  char *p = reinterpret_cast<char *>(workspace);
  int *stat = reinterpret_cast<int *>(p);
  unsigned *ticket = reinterpret_cast<unsigned *>(p + 1024);
  int *tcount = reinterpret_cast<int *>(p + 1280);
  void *sp = const_cast<void *>(state);
  hipError_t err;
  if (Q > 0 && lm_final)
    err = launch(k_ctc_beam_emit<1>, dim3(S), dim3(64), 0, st, LaunchProbe{}, S, B, N, mode, lm_final, sp, max_frames, hyp, hyp_stride, hyp_len,
                 count, score, frames, stable, tcount, ticket);
  else
    err = launch(k_ctc_beam_emit<0>, dim3(S), dim3(64), 0, st, LaunchProbe{}, S, B, N, mode, (const float *)nullptr, sp, max_frames, hyp,
                 hyp_stride, hyp_len, count, score, frames, stable, tcount, ticket);
  if (err != hipSuccess || !refs) return err;
  return launch(k_ctc_beam_tail, dim3(S), dim3(256), 0, st, LaunchProbe{}, (const int *)hyp, (const int *)hyp_len, (const int *)tcount, hyp_stride,
                S, K, N, blank, refs, roff, errors, totals, stat, ticket);
}

}  // namespace klstm
