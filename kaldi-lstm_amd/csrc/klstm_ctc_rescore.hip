// kaldi-lstm_amd/csrc/klstm_ctc_rescore.hip -- second-pass rescoring of CTC n-best lists with token and word back-off language models
// (klstm_ctc_nbest_rescore of include/klstm.h; the numpy twin: tests/ctc_rescore_ref.py).  For every stream a list of
// hypotheses h_q with log probabilities l_q (the arrays klstm_ctc_beam_decode wrote) and up to two sparse back-off models, blobs of
// klstm_ctc_slm_build: `sub`, over the tokens, whose score is taken out (the model the first pass fused), and `add`, over the tokens or
// over the words -- the maximal runs of tokens other than the separator, known by their 64-bit beam_hash and mapped to the word
// model's classes by a sorted table -- whose score is put in:
//   logw(model, h) = log prod flush(g_i) [* flush(final)],  (g_i, next) = slm_lookup(state, unit_i): the product kept as a double
//                    mantissa in [0.5, 1) and an integer exponent, one IEEE product and one frexp per unit, so it never leaves the
//                    normal range and carries the twin's bits; the one log at the end is the only operation that may differ
//   z_q = am_scale l_q - logw(sub) + add_scale logw(add) + unit_bonus units_q, in double, left to right
//   the entries that are well formed and that no model forbids, ranked by z descending, ties to the lower q
// Two launches:
//   k_resc_walk   grid (N, S), one wave per entry.  The entry check of klstm_ctc_nbest.h (the contract of a list) stages the tokens in
//                 LDS; in word mode the lane of a word's first token folds its key, bisects the table and leaves the class in LDS;
//                 then lane 0 walks `sub` and lane 1 walks `add`, in lockstep: each walk is one chain of dependent loads to which the
//                 other lanes have nothing to add.  Lane 0 writes the entry's score.
//   k_resc_rank   grid (S), one wave per stream (N <= 64: it sees the whole list).  Ranks by integer comparison on an order-preserving
//                 map of the double's bits, writes the order, gathers the re-ranked list (tokens copied by all lanes) and the stream's
//                 statistics; the last workgroup to arrive (ctc_last_arrival) adds the minibatch onto the totals, streams in order.
// DETERMINISM.  No floating-point atomics, no reduction over floating-point values: bit-identical from run to run.
// BOUNDS.  Every loop is bounded by max_len, the table's size, N or SLM_MAXBACK; a token is checked against [0, K) before it is looked
// up, a word's class against [0, V), a next state against [0, Q), and the bisection of the table stays inside [0, W) whatever it holds.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>

#include "../../include/klstm.h"
#include "klstm_ctc_host.h"
#include "klstm_ctc_nbest.h"
#include "klstm_ctc_slm.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int RESC_TOK = 1024, RESC_WORDS = 512;      // max_len <= 1023 tokens make at most 512 words
enum { RESC_UNLISTED = 0, RESC_DROPPED = 1, RESC_FORBIDDEN = 2, RESC_LIVE = 3 };

struct RescIn : NbestIn {};             // the caller's arrays; the ninth member is K (its own type: the kernels keep their names)
// a model: the blob (null: none), its final weights (or null), its states
struct RescLm { const void *blob; const float *fin; int Q; };
// the word table: W sorted keys with their classes (W = 0: token level), the word model's V classes, its reserved class, the class of
// an unknown word (< 0: it forbids the entry), the separator
struct RescWords { const u64 *keys; const int *ids; int W, V, reserved, unk, sep; };
// the workspace.  state [S N]: RESC_*; oov [S N]; z [S N] double; info [S]: 0 idle, 1 done, 2 rejected; stat [S][8] double
struct RescWs { unsigned *ticket; int *info, *state, *oov; double *z, *stat; };
struct RescOut {
  int *order, *live_count;
  int out_n, out_stride;
  int *out_hyp, *out_len, *out_count;
  float *out_score;
  int *out_errors;
  double *totals;
};

static size_t resc_layout(int S, int N, void *base, RescWs &ws) {
  const size_t SN = (size_t)S * N;
  CtcCarver c(base);
  ws.ticket = c.take<unsigned>(64);
  ws.info = c.take<int>(S);
  ws.state = c.take<int>(SN);
  ws.oov = c.take<int>(SN);
  ws.z = c.take<double>(SN);
  ws.stat = c.take<double>((size_t)S * 8);
  return c.bytes();
}

// the same bytes with and without a word table: the words' classes live in LDS
size_t ctc_rescore_workspace_bytes(int S, int N, int /*max_len*/, int /*words*/) { RescWs ws; return resc_layout(S, N, nullptr, ws); }

// ------------------------------------------------------------------------------------------------------------------------------------
// One entry: is it well formed, its units, the two walks, its score.  One wave.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_resc_walk(RescIn a, RescLm sub, RescLm add, RescWords w, float am_scale, float add_scale,
                                                  float unit_bonus, RescWs ws, float *__restrict__ score, float *__restrict__ add_logp,
                                                  float *__restrict__ sub_logp, int *__restrict__ units_out, int *__restrict__ oov_out) {
  __shared__ int lds[RESC_TOK + RESC_WORDS];                       // the tokens, behind them the words' classes
  int *tok = lds, *wid = lds + RESC_TOK;
  const int q = blockIdx.x, s = blockIdx.y, lane = threadIdx.x, se = s * a.N + q;
  if (se == 0 && lane == 0) *ws.ticket = 0u;                       // for k_resc_rank, the next launch
  KLSTM_NBEST_SHAPE(a, s, q, se, listed, ok, len, lp)              // max_len <= 1023: the tokens fit
  if (ok) {                                                        // uniform over the wave
    const int *h = a.hyp + (size_t)se * a.stride;
    KLSTM_NBEST_TOKENS(h, len, lane, (tok[t_] = v_, v_ < 0 || v_ >= a.K), ok)
  }
  __syncthreads();
  int nunits = 0, noov = 0;
  if (ok && w.W == 0) nunits = len;
  if (ok && w.W > 0) {
    for (int t0 = 0; t0 < len; t0 += 64) {
      const int t = t0 + lane;
      const bool start = nbest_word_start(tok, len, w.sep, t);
      const unsigned long long mask = __ballot(start);
      bool isoov = false;
      if (start) {                                                 // the lane of a word's first token folds the word and looks it up
        const u64 hs = nbest_word_key(tok, len, w.sep, t);
        int lo = 0, hi = w.W;
        for (int it = 0; it < 32 && lo < hi; it++) {               // W <= 2^24: 25 halvings at most; lo, hi, mid stay in [0, W]
          const int mid = (lo + hi) >> 1;
          if (w.keys[mid] < hs) lo = mid + 1; else hi = mid;
        }
        int id = -1;
        if (lo < w.W && w.keys[lo] == hs) id = w.ids[lo];
        isoov = id < 0 || id >= w.V || id == w.reserved;
        if (isoov) id = w.unk >= 0 ? w.unk : -1;                   // -1: the walk stops here
        wid[nunits + nbest_word_slot(mask, lane)] = id;
      }
      noov += __popcll(__ballot(isoov));
      nunits += __popcll(mask);
    }
  }
  __syncthreads();
  // the two walks: lane 0 over the tokens for `sub`, lane 1 over the tokens or the words' classes for `add`, the same instructions
  double logw = 0.0;
  int forb = 0;
  if (ok && lane < 2) {
    const void *blob = lane ? add.blob : sub.blob;
    const float *fin = lane ? add.fin : sub.fin;
    const int Q = lane ? add.Q : sub.Q;
    const bool by_word = lane == 1 && w.W > 0;
    const int base = by_word ? RESC_TOK : 0, n = by_word ? nunits : len;
    if (blob) {
      const SlmView view = slm_view(blob, Q);
      double m = 1.0;
      int e = 0, st = 0;
      for (int i = 0; i < n; i++) {
        const int u = lds[base + i];
        if (u < 0) { forb = 1; break; }                            // an unknown word without a class for it
        float g;
        int nx;
        slm_lookup(view, st, u, g, nx);
        const float gf = beam_emit(g);
        if (gf == 0.f || nx < 0 || nx >= Q) { forb = 1; break; }
        int de;
        m = frexp(bmul(m, (double)gf), &de);
        e += de;
        st = nx;
      }
      if (!forb && fin) {
        const float gf = beam_emit(fin[st]);
        if (gf == 0.f) forb = 1;
        else {
          int de;
          m = frexp(bmul(m, (double)gf), &de);
          e += de;
        }
      }
      logw = forb ? -(double)INFINITY : badd(log(m), bmul((double)e, 0.6931471805599453));
    }
  }
  const double sub_lw = __shfl(logw, 0), add_lw = __shfl(logw, 1);
  const int forbidden = __shfl(forb, 0) | __shfl(forb, 1);
  if (lane != 0) return;
  const int state = !listed ? RESC_UNLISTED : !ok ? RESC_DROPPED : forbidden ? RESC_FORBIDDEN : RESC_LIVE;
  double z = bmul((double)am_scale, (double)lp);
  if (sub.blob) z = z - sub_lw;
  if (add.blob) z = badd(z, bmul((double)add_scale, add_lw));
  z = badd(z, bmul((double)unit_bonus, (double)nunits));
  z = z + 0.0;                                                     // -0 becomes +0: one key per value
  ws.state[se] = state;
  ws.z[se] = z;
  ws.oov[se] = noov;
  score[se] = state == RESC_LIVE ? (float)z : -INFINITY;
  if (add_logp) add_logp[se] = ok ? (float)add_lw : -INFINITY;
  if (sub_logp) sub_logp[se] = ok ? (float)sub_lw : -INFINITY;
  if (units_out) units_out[se] = nunits;
  if (oov_out) oov_out[se] = noov;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The ranking of one stream, its re-ranked list, its statistics and, by the last workgroup to arrive, the totals.  One wave.
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_resc_rank(RescIn a, RescWs ws, int S, RescOut o) {
  __shared__ int ord[64];
  __shared__ double sz[64];
  const int s = blockIdx.x, lane = threadIdx.x, N = a.N;
  const int cnt = a.count[s];
  const bool rejected = cnt < 0 || cnt > N;
  int state = RESC_UNLISTED, oov = 0;
  double z = 0.0;
  if (lane < N) { state = ws.state[s * N + lane]; z = ws.z[s * N + lane]; oov = ws.oov[s * N + lane]; }
  const int live = state == RESC_LIVE;
  // by z descending, ties to the lower q: the bits of a double order as the values do once the sign is folded in
  const u64 bits = (u64)__double_as_longlong(z);
  const u64 key = bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));
  const unsigned khi = (unsigned)(key >> 32), klo = (unsigned)key;
  int rank = 0;
  for (int j = 0; j < N; j++) {
    const u64 kj = ((u64)(unsigned)__shfl((int)khi, j) << 32) | (u64)(unsigned)__shfl((int)klo, j);
    const int lj = __shfl(live, j);
    rank += lj && (kj > key || (kj == key && j < lane));
  }
  const int nlive = __popcll(__ballot(live));
  const int ndropped = __popcll(__ballot(state == RESC_DROPPED)), nforbidden = __popcll(__ballot(state == RESC_FORBIDDEN));
  for (int d = 32; d > 0; d >>= 1) oov += __shfl_xor(oov, d);       // integers: any order
  ord[lane] = -1;
  sz[lane] = z;
  __syncthreads();
  if (live) ord[rank] = lane;                                      // the ranks of the live entries are 0 .. nlive - 1, each once
  __syncthreads();
  if (lane < N) o.order[s * N + lane] = ord[lane];
  const int st = rejected ? 2 : nlive == 0 ? 0 : 1;
  if (o.out_n >= 1) {
    const int oc = nlive < o.out_n ? nlive : o.out_n;
    if (lane == 0) o.out_count[s] = oc;
    for (int r = 0; r < oc; r++) {
      const int src = s * N + ord[r];
      const size_t dst = (size_t)s * o.out_n + r;
      const int len = a.hyp_len[src];                              // a live entry: 0 <= len <= min(stride, max_len) <= out_stride
      for (int t = lane; t < len; t += 64) o.out_hyp[dst * o.out_stride + t] = a.hyp[(size_t)src * a.stride + t];
      if (lane == 0) {
        o.out_len[dst] = len;
        o.out_score[dst] = (float)sz[ord[r]];
        if (o.out_errors) o.out_errors[dst] = a.errors ? a.errors[src] : -1;
      }
    }
  }
  if (lane != 0) return;
  o.live_count[s] = nlive;
  ws.info[s] = st;
  if (!o.totals) return;
  double *stat = ws.stat + 8 * s;
  const int best = st == 1 ? ord[0] : -1;
  stat[2] = (double)ndropped;
  stat[3] = (double)nforbidden;
  stat[4] = (st == 1 && best != 0) ? 1.0 : 0.0;
  stat[5] = (st == 1 && a.errors) ? (double)a.errors[s * N] : 0.0;
  stat[6] = (st == 1 && a.errors) ? (double)a.errors[s * N + best] : 0.0;
  stat[7] = (double)oov;
  if (!ctc_last_arrival(ws.ticket, S)) return;
  KLSTM_NBEST_ADD_TOTALS(ws.info, ws.stat, S, 2, o.totals)
}

hipError_t launch_ctc_rescore(const int *hyp, int hyp_stride, const int *hyp_len, const int *count, const float *logp, const int *errors,
                              int S, int N, int max_len, int K, const void *sub, int sub_states, const float *sub_final, const void *add,
                              int add_states, int add_classes, const float *add_final, const unsigned long long *word_keys,
                              const int *word_ids, int num_words, int unk_id, int separator, int add_reserved, float am_scale,
                              float add_scale, float unit_bonus, int *order, int *live_count, float *score, float *add_logp,
                              float *sub_logp, int *units, int *oov, int out_n, int *out_hyp, int out_stride, int *out_len,
                              int *out_count, float *out_score, int *out_errors, double *totals, void *workspace, hipStream_t st) {
  RescWs ws;
  resc_layout(S, N, workspace, ws);
  const RescIn in{{hyp, hyp_len, count, logp, errors, hyp_stride, N, max_len, {K}}};
  const RescLm lsub{sub, sub ? sub_final : nullptr, sub_states}, ladd{add, add ? add_final : nullptr, add_states};
  const RescWords w{word_keys, word_ids, num_words, add_classes, add_reserved, unk_id, separator};
  const RescOut o{order, live_count, out_n, out_stride, out_hyp, out_len, out_count, out_score, out_errors, totals};
  hipError_t err = launch(k_resc_walk, dim3(N, S), dim3(64), 0, st, LaunchProbe{}, in, lsub, ladd, w, am_scale, add_scale, unit_bonus, ws,
                          score, add_logp, sub_logp, units, oov);
  if (err != hipSuccess) return err;
  return launch(k_resc_rank, dim3(S), dim3(64), 0, st, LaunchProbe{}, in, ws, S, o);
}

}  // namespace klstm
