// kaldi-lstm_amd/csrc/klstm_ctc_nbest.h -- the contract of an n-best list, for the kernels that read the arrays the prefix beam search
// wrote (klstm_ctc_consensus.hip, klstm_ctc_rescore.hip): the caller's arrays, which entries count, what a word is, how
// a minibatch goes onto the caller's totals.  The Levenshtein row step and the ticket are in klstm_ctc_dev.h, with the decoders.
#pragma once
#include "klstm_ctc_dev.h"

namespace klstm {

// hyp [S][N][stride], hyp_len [S][N], count [S], logp [S][N], errors [S][N] or null; max_len: the token capacity of the call.  The
// ninth member is the call's own: the consensus's separator (-1: token units), the rescoring's token classes.
struct NbestIn { const int *hyp, *hyp_len, *count; const float *logp; const int *errors; int stride, N, max_len; union { int sep, K; }; };

// Entry (s, q), se = s N + q.  listed: the stream's count lies in [0, N] and q < count; the slots beyond the count are never read.
// ok: listed and well formed, that is a finite logp, 0 <= len <= min(stride, max_len) (KLSTM_NBEST_SHAPE, which declares listed, ok,
// len, lp under the caller's names) and no token that BAD objects to (KLSTM_NBEST_TOKENS, under `if (ok)`, h the entry's tokens; BAD:
// an expression over position t_ and token v_, met once per token, token t by lane t % 64; it may keep the token).  Listed and not
// ok is DROPPED.  Uniform over the wave.  THE TWO CALLERS DIFFER in BAD: the rescoring looks tokens up in models of K classes and
// demands [0, K); the consensus has no K, compares tokens only with each other, and objects to negative ones alone.
// TEXT: as one function k_resc_walk has two pairs of instructions swapped, k_cons_keys another control flow (ctc_nbest_shared_isa.txt).
#define KLSTM_NBEST_SHAPE(a, s, q, se, listed, ok, len, lp)                                                                          \
  const bool listed = (a).count[s] >= 0 && (a).count[s] <= (a).N && (q) < (a).count[s];                                              \
  bool ok = listed;                                                                                                                  \
  int len = 0;                                                                                                                       \
  float lp = 0.f;                                                                                                                    \
  if (ok) {                                                                                                                          \
    len = (a).hyp_len[se];                                                                                                           \
    lp = (a).logp[se];                                                                                                               \
    ok = isfinite(lp) && len >= 0 && len <= (a).stride && len <= (a).max_len;                                                        \
  }
#define KLSTM_NBEST_TOKENS(h, len, lane, BAD, ok)                                                                                    \
  {                                                                                                                                  \
    bool bad_ = false;                                                                                                               \
    for (int t_ = (lane); t_ < (len); t_ += 64) {                                                                                    \
      const int v_ = (h)[t_];                                                                                                        \
      bad_ |= BAD;                                                                                                                   \
    }                                                                                                                                \
    ok = !__any(bad_);                                                                                                               \
  }

// The words of tok[0 .. len): the maximal runs of tokens other than `sep` (leading, trailing, repeated separators make no empty word),
// each known by its key, beam_hash folded over its tokens from BEAM_H0.  A wave takes 64 tokens at a time: the ballot of
// nbest_word_start counts the words, nbest_word_slot(ballot, lane) places this lane's among them, the lane of a start folds the key.
__device__ __forceinline__ bool nbest_word_start(const int *tok, int len, int sep, int t) {
  return t < len && tok[t] != sep && (t == 0 || tok[t - 1] == sep);
}
__device__ __forceinline__ unsigned nbest_word_slot(unsigned long long starts, int lane) { return __popcll(starts & ((1ull << lane) - 1ull)); }
__device__ __forceinline__ u64 nbest_word_key(const int *tok, int len, int sep, int t) {
  u64 hs = BEAM_H0;
  for (int i = t; i < len && tok[i] != sep; i++) hs = beam_hash(hs, tok[i]);
  return hs;
}

// The totals of a minibatch, by the thread ctc_last_arrival chose: over the S streams in order, info[q] == 1 counts into t[0], anything
// else into t[1]; stat[8 q + i], FIRST <= i < 8, goes into t[i + 2 - FIRST]; then t onto totals.  TEXT: as a function k_cons_conf
// is scheduled differently (ctc_nbest_shared_isa.txt).
#define KLSTM_NBEST_ADD_TOTALS(info, stat, S, FIRST, totals)                                                                         \
  {                                                                                                                                  \
    double t_[10 - (FIRST)] = {};                                                                                                    \
    for (int q = 0; q < (S); q++) {                                                                                                  \
      const int sq = __hip_atomic_load((info) + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                                      \
      t_[sq == 1 ? 0 : 1] += 1.0;                                                                                                    \
      for (int i = (FIRST); i < 8; i++)                                                                                              \
        t_[i + 2 - (FIRST)] += __hip_atomic_load((stat) + 8 * q + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                    \
    }                                                                                                                                \
    for (int i = 0; i < 10 - (FIRST); i++) (totals)[i] += t_[i];                                                                     \
  }

}  // namespace klstm
