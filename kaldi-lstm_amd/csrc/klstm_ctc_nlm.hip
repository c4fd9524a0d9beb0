// kaldi-lstm_amd/csrc/klstm_ctc_nlm.hip -- rescoring of CTC n-best lists with an LSTM language model: the three stateless knlm_*
// entries of include/klstm_nlm.h (which defines every quantity; the numpy twin: tests/ctc_nlm_ref.py) and their kernels.
// The net itself runs through the engines and klstm_affine_propagate; this file is the glue that keeps the lists on the device:
//   k_nlm_pack     grid (T E), 256 threads: row t E + e of the chunk's engine input, the one-hot of the entry's token at that position or
//                  the token's column of the embedding plus its bias (a gather: the rows x V one-hot block and its product never exist).
//   k_nlm_rows<NW> the rows of the last Affine -> lp of every row that has a target, ONE sweep over the row: every lane keeps the
//                  maximum and the sum of exp(a - maximum) of its columns (rescaled when the maximum moves), the lanes are combined by
//                  a fixed tree.  NW = 1: one wave per row, four rows per workgroup (narrow rows leave no wave idle); NW = 4: one
//                  workgroup per row (V >= NLM_WIDE).  T E rows: the chip is filled by rows, not by entries.
//   k_nlm_sum      one thread per engine stream adds the chunk's row values onto the entry's double, t ascending: the fixed order.
//                  A launch of its own: a stateless call has nobody to zero a ticket for it.
//   k_nlm_rank     ONE workgroup of 16 waves, a wave per stream (S <= 32: two rounds): the entry check, z, the ranking by integer
//                  comparison on an order-preserving map of the double's bits, the order, the re-ranked list, the stream's
//                  statistics in LDS; after one barrier thread 0 adds the minibatch onto the totals, streams in order.  The ranking
//                  is k_resc_rank's (klstm_ctc_rescore.hip), kept as a copy: that kernel reads the states its walk left in a workspace and
//                  hands its statistics over by a ticket; here there is neither.
// DETERMINISM.  No floating-point atomics; every sum over floating-point values has a fixed order: bit-identical from run to run.
// BOUNDS.  An entry is checked under the contract of klstm_ctc_nbest.h (tokens in [0, K)) by one wave of every workgroup before a token is used
// (once per row: the rows of an entry sit in different workgroups, which share nothing, and a check is len / 64 loads a lane), so a
// token indexes V >= K columns safely; rows and entries beyond T E and S N are not touched; every loop is bounded by max_len, V, T or N.
#pragma clang fp contract(off)
#include <cmath>
#include <cstdint>

#include "../../include/klstm_nlm.h"
#include "klstm_ctc_host.h"
#include "klstm_ctc_nbest.h"
#include "klstm_ctc_slm.h"
#include "klstm_host.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int NLM_WIDE = 1024;          // from this many classes a row takes a whole workgroup
enum { NLM_UNLISTED = 0, NLM_DROPPED = 1, NLM_FORBIDDEN = 2, NLM_LIVE = 3 };

// the workspace of knlm_score_rows: lp [T E] and whether the row has one
struct NlmWs { float *lp; int *has; };
static size_t nlm_layout(int E, int T, void *base, NlmWs &ws) {
  CtcCarver c(base);
  ws.lp = c.take<float>((size_t)E * T);
  ws.has = c.take<int>((size_t)E * T);
  return c.bytes();
}

// Entry se by one wave: well formed?  len and lp as KLSTM_NBEST_SHAPE leaves them.  Uniform over the wave.
__device__ __forceinline__ bool nlm_entry(const NbestIn &a, int se, int lane, int &len_out, float &lp_out, bool &listed_out) {
  const int s = se / a.N, q = se - s * a.N;
  KLSTM_NBEST_SHAPE(a, s, q, se, listed, ok, len, lp)
  if (ok) {
    const int *h = a.hyp + (size_t)se * a.stride;
    KLSTM_NBEST_TOKENS(h, len, lane, (v_ < 0 || v_ >= a.K), ok)
  }
  len_out = len;
  lp_out = lp;
  listed_out = listed;
  return ok;
}

__global__ __launch_bounds__(256) void k_nlm_pack(NbestIn a, int SN, int bos, int has_eos, int first, int E, int t0,
                                                  const float *__restrict__ embW, const float *__restrict__ embB, int V, int cols,
                                                  float *__restrict__ out, int out_stride) {
  __shared__ int sx;
  const int row = blockIdx.x, t = row / E, e = row - t * E, lane = threadIdx.x & 63;
  const int se = first + e, p = t0 + t;
  if (threadIdx.x < 64) {                                          // the first wave checks the entry for the workgroup
    int x = -1;                                                    // the class that goes in; -1: a row of zeros
    if (se < SN) {
      int len;
      float lp;
      bool listed;
      if (nlm_entry(a, se, lane, len, lp, listed) && p < len + has_eos) x = p == 0 ? bos : a.hyp[(size_t)se * a.stride + p - 1];
    }
    if (lane == 0) sx = x;
  }
  __syncthreads();
  const int x = sx;
  float *op = out + (size_t)row * out_stride;
  if (x < 0) {
    for (int c = threadIdx.x; c < cols; c += 256) op[c] = 0.f;
  } else if (!embW) {
    for (int c = threadIdx.x; c < cols; c += 256) op[c] = c == x ? 1.f : 0.f;
  } else {
    // a column of [D x V]: neighbouring threads read V floats apart, one cache line each.  D loads a row, microseconds a chunk next to
    // the engines' hundreds; a transposed copy [V x D] kept by the caller would make it one contiguous row
    for (int c = threadIdx.x; c < cols; c += 256) op[c] = embW[(size_t)c * V + x] + embB[c];
  }
}

template <int NW>
__global__ __launch_bounds__(256) void k_nlm_rows(const float *__restrict__ y, int y_stride, NbestIn a, int SN, int V, int eos, int first,
                                                  int E, int rows, int t0, NlmWs ws) {
  __shared__ float sm[4];
  __shared__ int stgt;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = NW == 1 ? blockIdx.x * 4 + wave : blockIdx.x, tid = NW == 1 ? lane : threadIdx.x;
  if (row >= rows) return;                                         // NW = 1: this wave alone, it meets no barrier below
  const int t = row / E, e = row - t * E, se = first + e, p = t0 + t;
  int tgt = -1;                                                    // uniform over the row's threads
  if (NW == 1 || wave == 0) {                                      // NW = 4: the first wave checks the entry for the workgroup
    if (se < SN) {
      int len;
      float lp;
      bool listed;
      if (nlm_entry(a, se, lane, len, lp, listed)) {
        if (p < len) tgt = a.hyp[(size_t)se * a.stride + p];
        else if (p == len && eos >= 0) tgt = eos;
      }
    }
    if (NW != 1 && lane == 0) stgt = tgt;
  }
  if (NW != 1) {
    __syncthreads();
    tgt = stgt;
  }
  if (tgt < 0) {
    if (tid == 0) ws.has[row] = 0;
    return;
  }
  const float *yp = y + (size_t)row * y_stride;
  float m = -3.4e38f, sum = 0.f;                                   // of this thread's columns: their maximum, sum of exp(a - m)
  ctc_for_row(yp, nullptr, V, tid, 64 * NW, [&](float v, int) {
    const bool up = v > m;                                         // (a NaN: not up, and it poisons the sum)
    const float ex = expf(up ? m - v : v - m);
    sum = up ? sum * ex + 1.f : sum + ex;
    m = up ? v : m;
  });
  float mx, tot;
  if (NW == 1) {
    mx = m;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    tot = sum * expf(m - mx);
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
  } else {
    mx = ctc_block_reduce(m, sm, true);
    tot = ctc_block_reduce(sum * expf(m - mx), sm, false);
  }
  if (tid == 0) {
    ws.lp[row] = (yp[tgt] - mx) - logf(tot);
    ws.has[row] = 1;
  }
}

__global__ __launch_bounds__(64) void k_nlm_sum(NlmWs ws, int SN, int first, int E, int T, int t0, double *__restrict__ acc,
                                                int *__restrict__ positions) {
  const int e = threadIdx.x, se = first + e;
  if (e >= E || se >= SN) return;
  double v = t0 == 0 ? 0.0 : acc[se];
  int n = (t0 == 0 || !positions) ? 0 : positions[se];
  for (int t = 0; t < T; t++) {
    if (!ws.has[t * E + e]) continue;
    v += (double)ws.lp[t * E + e];
    n++;
  }
  acc[se] = v;
  if (positions) positions[se] = n;
}

struct NlmOut {
  int *order, *live_count;
  float *score, *nlm_logp;
  int *units;
  int out_n, out_stride;
  int *out_hyp, *out_len, *out_count;
  float *out_score;
  int *out_errors;
  double *totals;
};

__global__ __launch_bounds__(1024) void k_nlm_rank(NbestIn a, int S, const double *__restrict__ acc, float am_scale, float nlm_scale,
                                                   float unit_bonus, int has_eos, NlmOut o) {
  __shared__ double stat[32][8];
  __shared__ int info[32];                                         // 0 idle, 1 done, 2 rejected
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, N = a.N;
  for (int s = wave; s < S; s += 16) {
    const int cnt = a.count[s];
    const bool rejected = cnt < 0 || cnt > N;
    int state = NLM_UNLISTED, mylen = 0;
    float mylp = 0.f;
    for (int q = 0; q < N; q++) {                                  // the wave checks the entries one after the other, lane q keeps entry q
      int len;
      float lp;
      bool listed;
      const bool ok = nlm_entry(a, s * N + q, lane, len, lp, listed);
      if (!listed) break;                                          // uniform: q >= count, or the stream is rejected
      if (lane == q) { state = ok ? NLM_LIVE : NLM_DROPPED; mylen = ok ? len : 0; mylp = lp; }
    }
    const bool formed = state == NLM_LIVE;
    double lw = 0.0, z = 0.0;
    if (formed) {
      lw = acc[s * N + lane];
      if (!isfinite(lw)) state = NLM_FORBIDDEN;
      z = bmul((double)am_scale, (double)mylp);
      z = badd(z, bmul((double)nlm_scale, lw));
      z = badd(z, bmul((double)unit_bonus, (double)mylen));
      z = z + 0.0;                                                 // -0 becomes +0: one key per value
    }
    const int live = state == NLM_LIVE;
    if (lane < N) {
      o.score[s * N + lane] = live ? (float)z : -INFINITY;
      if (o.nlm_logp) o.nlm_logp[s * N + lane] = live ? (float)lw : -INFINITY;
      if (o.units) o.units[s * N + lane] = mylen;
    }
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
    const int ndropped = __popcll(__ballot(state == NLM_DROPPED)), nforbidden = __popcll(__ballot(state == NLM_FORBIDDEN));
    int npos = formed ? mylen + (has_eos ? 1 : 0) : 0;
    for (int d = 32; d > 0; d >>= 1) npos += __shfl_xor(npos, d);   // integers: any order
    int ord = -1;                                                  // the entry of rank `lane`: the ranks of the live entries are 0 .. nlive - 1, each once
    for (int j = 0; j < N; j++) {
      const int rj = __shfl(rank, j), lj = __shfl(live, j);
      if (lj && rj == lane) ord = j;
    }
    if (lane < N) o.order[s * N + lane] = ord;
    const int st = rejected ? 2 : nlive == 0 ? 0 : 1;
    const int best = __shfl(ord, 0);
    if (o.out_n >= 1) {
      const int oc = nlive < o.out_n ? nlive : o.out_n;
      if (lane == 0) o.out_count[s] = oc;
      for (int r = 0; r < oc; r++) {
        const int q = __shfl(ord, r), src = s * N + q;
        const double zq = __shfl(z, q);
        const size_t dst = (size_t)s * o.out_n + r;
        const int len = a.hyp_len[src];                            // a live entry: 0 <= len <= min(stride, max_len) <= out_stride
        for (int t = lane; t < len; t += 64) o.out_hyp[dst * o.out_stride + t] = a.hyp[(size_t)src * a.stride + t];
        if (lane == 0) {
          o.out_len[dst] = len;
          o.out_score[dst] = (float)zq;
          if (o.out_errors) o.out_errors[dst] = a.errors ? a.errors[src] : -1;
        }
      }
    }
    if (lane == 0) {
      o.live_count[s] = nlive;
      info[s] = st;
      stat[s][2] = (double)ndropped;
      stat[s][3] = (double)nforbidden;
      stat[s][4] = (st == 1 && best != 0) ? 1.0 : 0.0;
      stat[s][5] = (st == 1 && a.errors) ? (double)a.errors[s * N] : 0.0;
      stat[s][6] = (st == 1 && a.errors) ? (double)a.errors[s * N + best] : 0.0;
      stat[s][7] = (double)npos;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0 || !o.totals) return;
  double t[8] = {};
  for (int s = 0; s < S; s++) {                                    // the streams in order
    t[info[s] == 1 ? 0 : 1] += 1.0;
    for (int i = 2; i < 8; i++) t[i] += stat[s][i];
  }
  for (int i = 0; i < 8; i++) o.totals[i] += t[i];
}

}  // namespace klstm

using namespace klstm;

// ---- the checks, every one before the first HIP call; fn is the entry's name, which every message begins with ----
static klstm_status nlm_list_check(const char *fn, int S, int list_n, int max_len, int K, int V) {
  if (S < 1 || S > 32 || list_n < 1 || list_n > 64 || max_len < 0 || max_len > 1023)
    return fail(KLSTM_ERR_SHAPE, "%s: streams %d, list of %d, length %d outside 1 <= S <= 32, 1 <= list <= 64, 0 <= L <= 1023", fn, S, list_n, max_len);
  if (K < 2 || V < K || V > 32768) return fail(KLSTM_ERR_SHAPE, "%s: %d token classes, %d classes outside 2 <= K <= V <= 32768", fn, K, V);
  return KLSTM_OK;
}
static klstm_status nlm_chunk_shape(const char *fn, int E, int T) {
  if (E < 1 || E > 32 || T < 1 || (long)T * E > (1L << 24))
    return fail(KLSTM_ERR_SHAPE, "%s: %d engine streams, chunks of %d outside 1 <= E <= 32, 1 <= T, T * E <= 2^24", fn, E, T);
  return KLSTM_OK;
}
static klstm_status nlm_chunk_args(const char *fn, int S, int list_n, int hyp_stride, int first_entry, int t0) {
  if (hyp_stride < 1) return fail(KLSTM_ERR_ARG, "%s: hypothesis stride %d", fn, hyp_stride);
  if (first_entry < 0 || first_entry >= S * list_n) return fail(KLSTM_ERR_ARG, "%s: first entry %d outside [0, %d)", fn, first_entry, S * list_n);
  if (t0 < 0) return fail(KLSTM_ERR_ARG, "%s: first position %d below 0", fn, t0);
  return KLSTM_OK;
}

extern "C" {

klstm_status knlm_pack(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                       int S, int list_n, int max_len, int K, int V, int bos, int eos, int first_entry, int E, int T, int t0,
                       const float *embed_W_dev, const float *embed_bias_dev, int D, float *out_dev, int out_stride, void *hip_stream) {
  const char *fn = "knlm_pack";
  if (klstm_status st = nlm_list_check(fn, S, list_n, max_len, K, V); st != KLSTM_OK) return st;
  if (klstm_status st = nlm_chunk_shape(fn, E, T); st != KLSTM_OK) return st;
  if (embed_W_dev && (D < 1 || D > 32768)) return fail(KLSTM_ERR_SHAPE, "%s: an embedding of %d rows outside 1 <= D <= 32768", fn, D);
  if (!hyp_dev || !hyp_len_dev || !nbest_count_dev || !logp_dev || !out_dev) return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (embed_W_dev && !embed_bias_dev) return fail(KLSTM_ERR_ARG, "%s: an embedding without its bias", fn);
  if (bos < 0 || bos >= V) return fail(KLSTM_ERR_ARG, "%s: bos %d outside [0, %d)", fn, bos, V);
  if (eos >= V) return fail(KLSTM_ERR_ARG, "%s: eos %d outside [0, %d)", fn, eos, V);
  if (klstm_status st = nlm_chunk_args(fn, S, list_n, hyp_stride, first_entry, t0); st != KLSTM_OK) return st;
  const int cols = embed_W_dev ? D : V;
  if (out_stride < cols) return fail(KLSTM_ERR_ARG, "%s: row stride below the row (%d < %d)", fn, out_stride, cols);
  const NbestIn in{hyp_dev, hyp_len_dev, nbest_count_dev, logp_dev, nullptr, hyp_stride, list_n, max_len, {K}};
  HIPCHK(launch(k_nlm_pack, dim3(T * E), dim3(256), 0, (hipStream_t)hip_stream, LaunchProbe{}, in, S * list_n, bos, eos >= 0 ? 1 : 0,
                first_entry, E, t0, embed_W_dev, embed_bias_dev, V, cols, out_dev, out_stride));
  return KLSTM_OK;
}

size_t knlm_workspace_bytes(int E, int T) {
  if (nlm_chunk_shape("knlm_workspace_bytes", E, T) != KLSTM_OK) return 0;
  NlmWs ws;
  return nlm_layout(E, T, nullptr, ws);
}

klstm_status knlm_score_rows(const float *a_dev, int a_stride, const int *hyp_dev, int hyp_stride, const int *hyp_len_dev,
                             const int *nbest_count_dev, const float *logp_dev, int S, int list_n, int max_len, int K, int V, int eos,
                             int first_entry, int E, int T, int t0, double *acc_dev, int *positions_dev, void *workspace,
                             size_t workspace_bytes, void *hip_stream) {
  const char *fn = "knlm_score_rows";
  if (klstm_status st = nlm_list_check(fn, S, list_n, max_len, K, V); st != KLSTM_OK) return st;
  if (klstm_status st = nlm_chunk_shape(fn, E, T); st != KLSTM_OK) return st;
  if (!a_dev || !hyp_dev || !hyp_len_dev || !nbest_count_dev || !logp_dev || !acc_dev || !workspace) return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (eos >= V) return fail(KLSTM_ERR_ARG, "%s: eos %d outside [0, %d)", fn, eos, V);
  if (klstm_status st = nlm_chunk_args(fn, S, list_n, hyp_stride, first_entry, t0); st != KLSTM_OK) return st;
  if (a_stride < V) return fail(KLSTM_ERR_ARG, "%s: row stride below V (%d < %d)", fn, a_stride, V);
  if (!ctc_al16(workspace)) return fail(KLSTM_ERR_ARG, "%s: workspace must be 16-byte aligned", fn);
  NlmWs ws;
  const size_t need = nlm_layout(E, T, workspace, ws);
  if (workspace_bytes < need)
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below knlm_workspace_bytes(%d, %d) = %zu", fn, workspace_bytes, E, T, need);
  const NbestIn in{hyp_dev, hyp_len_dev, nbest_count_dev, logp_dev, nullptr, hyp_stride, list_n, max_len, {K}};
  const int rows = T * E, SN = S * list_n;
  hipStream_t st = (hipStream_t)hip_stream;
  if (V >= NLM_WIDE)
    HIPCHK(launch(k_nlm_rows<4>, dim3(rows), dim3(256), 0, st, LaunchProbe{}, a_dev, a_stride, in, SN, V, eos, first_entry, E, rows, t0, ws));
  else
    HIPCHK(launch(k_nlm_rows<1>, dim3((rows + 3) / 4), dim3(256), 0, st, LaunchProbe{}, a_dev, a_stride, in, SN, V, eos, first_entry, E, rows, t0, ws));
  HIPCHK(launch(k_nlm_sum, dim3(1), dim3(64), 0, st, LaunchProbe{}, ws, SN, first_entry, E, T, t0, acc_dev, positions_dev));
  return KLSTM_OK;
}

klstm_status knlm_rank(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                       const int *errors_dev, int S, int list_n, int max_len, int K, const double *acc_dev, float am_scale,
                       float nlm_scale, float unit_bonus, int has_eos, int *order_dev, int *live_count_dev, float *score_dev,
                       float *nlm_logp_dev, int *units_dev, int out_n, int *out_hyp_dev, int out_stride, int *out_len_dev,
                       int *out_count_dev, float *out_score_dev, int *out_errors_dev, double *totals_dev, void *hip_stream) {
  const char *fn = "knlm_rank";
  if (klstm_status st = nlm_list_check(fn, S, list_n, max_len, K, K); st != KLSTM_OK) return st;
  if (out_n < 0 || out_n > list_n) return fail(KLSTM_ERR_SHAPE, "%s: a list of %d out of a list of %d", fn, out_n, list_n);
  if (!hyp_dev || !hyp_len_dev || !nbest_count_dev || !logp_dev || !acc_dev || !order_dev || !live_count_dev || !score_dev)
    return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (out_n >= 1 && (!out_hyp_dev || !out_len_dev || !out_count_dev || !out_score_dev))
    return fail(KLSTM_ERR_ARG, "%s: null list output with out_n %d", fn, out_n);
  if (hyp_stride < 1 || (out_n >= 1 && out_stride < (hyp_stride < max_len ? hyp_stride : max_len)))
    return fail(KLSTM_ERR_ARG, "%s: hypothesis stride %d, output stride %d (at least min(hypothesis stride, length %d))", fn, hyp_stride, out_stride, max_len);
  if (!std::isfinite(am_scale) || !std::isfinite(nlm_scale) || !std::isfinite(unit_bonus))
    return fail(KLSTM_ERR_ARG, "%s: scales %g, %g and bonus %g must be finite", fn, (double)am_scale, (double)nlm_scale, (double)unit_bonus);
  const NbestIn in{hyp_dev, hyp_len_dev, nbest_count_dev, logp_dev, errors_dev, hyp_stride, list_n, max_len, {K}};
  const NlmOut o{order_dev, live_count_dev, score_dev, nlm_logp_dev, units_dev, out_n, out_stride, out_hyp_dev, out_len_dev, out_count_dev,
                 out_score_dev, out_errors_dev, totals_dev};
  HIPCHK(launch(k_nlm_rank, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, LaunchProbe{}, in, S, acc_dev, am_scale, nlm_scale, unit_bonus,
                has_eos, o));
  return KLSTM_OK;
}

}  // extern "C"
