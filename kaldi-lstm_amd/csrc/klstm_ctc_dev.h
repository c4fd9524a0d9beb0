// kaldi-lstm_amd/csrc/klstm_ctc_dev.h -- device code shared by the CTC kernels (klstm_ctc.hip: the loss; klstm_ctc_align.hip: the forced
// alignment; klstm_ctc_decode.hip: best path; klstm_ctc_beam.hip: prefix beam search; klstm_ctc_mbr.hip: the n-best risk;
// klstm_ctc_mmi.hip: MMI; through klstm_ctc_nbest.h, the contract of an n-best list, klstm_ctc_consensus.hip and klstm_ctc_rescore.hip):
// the prefix hash, the status of an utterance, the maximum over a wave, the fixed-tree reduction over a workgroup, the links, the zero
// row and the gamma row of the three lattice losses, (value, index) reductions, the row reader, the ticket of the last workgroup, the
// Levenshtein row step with the one-wave distance on it, the alpha / beta chain of the loss (ctc_chain_run).  Host side: klstm_ctc_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/klstm.h"

namespace klstm {

constexpr float CTC_NEG = -1e30f;      // "log 0": absorbs every offset (ulp 7e22), exp(CTC_NEG - m) = 0

// The 64-bit hash of a label sequence: beam_hash folded over its labels from BEAM_H0, the hash of the empty prefix.  The prefix beam
// search (klstm_ctc_beam.hip) knows its prefixes by it; the second pass (klstm_ctc_nbest.h) and CtcWordKey of klstm_nnet.hpp know words by it.
typedef unsigned long long u64;
constexpr u64 BEAM_H0 = KLSTM_CTC_HASH_START, BEAM_HMUL = KLSTM_CTC_HASH_MUL;
__device__ __forceinline__ u64 beam_hash(u64 h, int c) {
  const u64 x = (h ^ (u64)(unsigned)(c + 1)) * BEAM_HMUL;
  return x ^ (x >> 29);
}

// 0 idle (len 0), 1 feasible, 2 rejected.  Uniform over the workgroup; sm: 2 ints of LDS.
__device__ __forceinline__ int ctc_status(int len, int T, int L, int Lcap, const int *__restrict__ lab, int K, int blank, int *sm) {
  if (len == 0) return 0;
  if (len < 0 || len > T || L < 0 || L > Lcap) return 2;
  if (threadIdx.x == 0) { sm[0] = 0; sm[1] = 0; }
  __syncthreads();
  int rep = 0, bad = 0;
  for (int j = threadIdx.x; j < L; j += blockDim.x) {
    const int c = lab[j];
    bad |= (c < 0 || c >= K || c == blank);
    rep += (j > 0 && lab[j - 1] == c);
  }
  if (rep) atomicAdd(&sm[0], rep);       // integer: the order of arrival does not matter
  if (bad) atomicOr(&sm[1], 1);
  __syncthreads();
  const int r = sm[0], b = sm[1];
  __syncthreads();
  return (b || len < L + r) ? 2 : 1;
}

// Maximum over the wave, the same value in every lane.  DPP row shifts and row broadcasts (the data path of the VALU, a few cycles
// each) instead of six trips through the LDS crossbar (__shfl_xor = ds_bpermute): this reduction sits on the dependent chain of
// every step.  max is idempotent, so the inclusive-scan form needs no bank masks; lanes without a source keep their own value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return fmaxf(v, __int_as_float(o));
}
__device__ __forceinline__ float wave_max(float v) {
  v = dpp_max<0x111, 0xf>(v);      // row_shr:1
  v = dpp_max<0x112, 0xf>(v);      // row_shr:2
  v = dpp_max<0x114, 0xf>(v);      // row_shr:4
  v = dpp_max<0x118, 0xf>(v);      // row_shr:8   lane 15 of every row of 16: the row's maximum
  v = dpp_max<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
  v = dpp_max<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3: lane 63 holds the maximum of the wave
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Maximum or sum over a workgroup of 256 threads by a fixed tree, the same value in every thread; sm: 4 floats of LDS.
__device__ __forceinline__ float ctc_block_reduce(float v, float *sm, bool is_max) {
  for (int o = 32; o > 0; o >>= 1) { const float x = __shfl_xor(v, o); v = is_max ? fmaxf(v, x) : v + x; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])) : (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__device__ __forceinline__ float ctc_block_sum(float v, float *sm) { return ctc_block_reduce(v, sm, false); }

// ------------------------------------------------------------------------------------------------------------------------------------
// The pieces around ctc_chain_run that the loss (klstm_ctc.hip), the n-best risk (klstm_ctc_mbr.hip) and MMI (klstm_ctc_mmi.hip) share
// ("One copy"): the links of a labelling, the zero row of diff and the gamma row of a frame.
// ------------------------------------------------------------------------------------------------------------------------------------
// The links of lab[0 .. L) by a workgroup of nt threads: next[j] = the next position that carries the class of position j (-1: none),
// first[j] = 1 where no earlier position carries it.  The thread of a first position then sums its class along next, in order.
__device__ __forceinline__ void ctc_links(const int *__restrict__ lab, int L, int *next, int *first, int nt) {
  const int tid = threadIdx.x;
  for (int j = tid; j < L; j += nt) first[j] = 1;
  __syncthreads();
  for (int j = tid; j < L; j += nt) {
    const int c = lab[j];
    int q = j + 1;
    while (q < L && lab[q] != c) q++;
    next[j] = q < L ? q : -1;
    if (q < L) first[q] = 0;                   // position q has exactly one predecessor: one writer
  }
}

// A row of K zeros by a workgroup of 256 threads; vec: 16 bytes at a time (ctc_rows_vec of klstm_ctc_host.h)
__device__ __forceinline__ void ctc_zero_row(float *dp, int K, int vec) {
  const int tid = threadIdx.x;
  if (vec) for (int c = tid * 4; c < K; c += 1024) *reinterpret_cast<float4 *>(dp + c) = make_float4(0.f, 0.f, 0.f, 0.f);
  else for (int c = tid; c < K; c += 256) dp[c] = 0.f;
}

// The gamma row of one frame by a workgroup of 256 threads: g[i] = exp(a[i] + bt[i] - their maximum) for the N states, `sall` their
// sum and `seven` the sum over the even (blank) states, both declared here as ACC and summed by SUM(value, SMS) (float:
// ctc_block_sum and the 4 floats of LDS; MMI: double).  Expects `tid` and `float sm[4]` (LDS) in scope.  TEXT, not a function: as a
// function the same instructions come out in another order (profiles/ctc_shared_pieces_isa.txt).
#define KLSTM_CTC_GAMMA_ROW(ACC, SUM, SMS, a, bt, N, g, sall, seven)                                                                 \
  ACC sall = 0, seven = 0;                                                                                                           \
  {                                                                                                                                  \
    float mx_ = CTC_NEG;                                                                                                             \
    for (int i = tid; i < (N); i += 256) { const float v = (a)[i] + (bt)[i]; (g)[i] = v; mx_ = fmaxf(mx_, v); }                      \
    mx_ = ctc_block_reduce(mx_, sm, true);                                                                                           \
    for (int i = tid; i < (N); i += 256) {     /* 256 is even: a thread's states are all even or all odd */                          \
      const float ex_ = expf((g)[i] - mx_);                                                                                          \
      (g)[i] = ex_;                                                                                                                  \
      sall += (ACC)ex_;                                                                                                              \
      seven += (i & 1) ? (ACC)0 : (ACC)ex_;                                                                                          \
    }                                                                                                                                \
    sall = SUM(sall, SMS);                                                                                                           \
    seven = SUM(seven, SMS);                                                                                                         \
  }

// ------------------------------------------------------------------------------------------------------------------------------------
// (value, index) pairs.  a beats b iff a.v > b.v, or a.v == b.v and a.i < b.i: a total order on (non-NaN value, distinct index), so
// any reduction tree gives the same winner.  The neutral element is (-inf, INT_MAX): it loses to every real column.
// ------------------------------------------------------------------------------------------------------------------------------------
struct Best { float v; int i; };
__device__ __forceinline__ void best_take(Best &b, float v, int i) {
  const bool t = v > b.v || (v == b.v && i < b.i);
  b.v = t ? v : b.v;
  b.i = t ? i : b.i;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void dpp_best(Best &b) {        // lanes without a source (or outside the row mask) see themselves
  const int ov = __builtin_amdgcn_update_dpp(__float_as_int(b.v), __float_as_int(b.v), CTRL, ROW_MASK, 0xf, false);
  const int oi = __builtin_amdgcn_update_dpp(b.i, b.i, CTRL, ROW_MASK, 0xf, false);
  best_take(b, __int_as_float(ov), oi);
}
// after this, lane 15 of every row of 16 lanes holds the best of its row
__device__ __forceinline__ void row16_best(Best &b) {
  dpp_best<0x111, 0xf>(b);      // row_shr:1
  dpp_best<0x112, 0xf>(b);      // row_shr:2
  dpp_best<0x114, 0xf>(b);      // row_shr:4
  dpp_best<0x118, 0xf>(b);      // row_shr:8
}
// ... and after this, lane 63 holds the best of the wave
__device__ __forceinline__ void wave_best(Best &b) {
  row16_best(b);
  dpp_best<0x142, 0xa>(b);      // row_bcast:15 into rows 1 and 3
  dpp_best<0x143, 0xc>(b);      // row_bcast:31 into rows 2 and 3
}

// One row of K columns seen by lane `lane` of `nl` lanes: a scalar head up to the first 16-byte boundary of the row, float4 body,
// scalar tail.  A lane meets its columns in ascending order and hands f(value, column) the ONE fp32 product y[k] * w[k] (y[k] itself
// without weights).  w (or null): the class weights, indexed by column.
template <class F>
__device__ __forceinline__ void ctc_for_row(const float *__restrict__ yp, const float *__restrict__ w, int K, int lane, int nl, F f) {
  int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(yp) & 15u)) & 15u) >> 2);
  head = head < K ? head : K;
  const int n4 = (K - head) >> 2, tail0 = head + 4 * n4;
  if (lane < head) f(w ? yp[lane] * w[lane] : yp[lane], lane);
  const float4 *y4 = reinterpret_cast<const float4 *>(yp + head);
  if (!w) {
#pragma unroll 4
    for (int q = lane; q < n4; q += nl) {
      const float4 a = y4[q];
      const int c = head + 4 * q;
      f(a.x, c); f(a.y, c + 1); f(a.z, c + 2); f(a.w, c + 3);
    }
  } else if ((reinterpret_cast<uintptr_t>(w + head) & 15u) == 0) {
    const float4 *w4 = reinterpret_cast<const float4 *>(w + head);
#pragma unroll 4
    for (int q = lane; q < n4; q += nl) {
      const float4 a = y4[q], m = w4[q];
      const int c = head + 4 * q;
      f(a.x * m.x, c); f(a.y * m.y, c + 1); f(a.z * m.z, c + 2); f(a.w * m.w, c + 3);
    }
  } else {
#pragma unroll 2
    for (int q = lane; q < n4; q += nl) {
      const float4 a = y4[q];
      const int c = head + 4 * q;
      f(a.x * w[c], c); f(a.y * w[c + 1], c + 1); f(a.z * w[c + 2], c + 2); f(a.w * w[c + 3], c + 3);
    }
  }
  const int c = tail0 + lane;
  if (c < K) f(w ? yp[c] * w[c] : yp[c], c);
}

// The ticket of the kernels that add their minibatch onto the caller's totals (k_ctc_collapse, k_ctc_beam_tail, k_cons_conf, k_resc_rank):
// thread 0 of a stream's workgroup, its statistics written; true for the last of S to arrive, who reads everybody's (agent scope).
__device__ __forceinline__ bool ctc_last_arrival(unsigned *ticket, int S) {
  __threadfence();                                                 // the stream's statistics before its ticket
  if (atomicAdd(ticket, 1u) != (unsigned)(S - 1)) return false;
  __threadfence();                                                 // the last workgroup: everybody's statistics are visible
  return true;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Levenshtein distance between the collapsed best path of stream s and ref[0 .. L), by ONE wave.  Column j of the row (0 .. L) sits in
// lane j / P, slot j % P.  For every hypothesis token:  tmp[j] = min(D'[j] + 1, D'[j-1] + (ref[j-1] != token)),  tmp[0] = row number,
// D[j] = j + min_{k <= j}(tmp[k] - k): a prefix minimum, in the lane's own slots first, then across the lanes by the DPP scan.
// The tokens come straight from frame_class (the launch before wrote it), 64 frames at a time, the kept ones picked off a ballot.
// COLLAPSE = false (klstm_ctc_beam.hip): fclass holds a finished hypothesis, every entry other than `blank` is a token.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min(int v) {
  return min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ int wave_scan_min(int v) {              // inclusive prefix minimum over the lanes (min is idempotent: no bank masks)
  v = dpp_min<0x111, 0xf>(v);
  v = dpp_min<0x112, 0xf>(v);
  v = dpp_min<0x114, 0xf>(v);
  v = dpp_min<0x118, 0xf>(v);
  v = dpp_min<0x142, 0xa>(v);
  v = dpp_min<0x143, 0xc>(v);
  return v;
}
constexpr int ED_BIG = 1 << 29;

// One row of the table, for the hypothesis token `tok` of row number `row` (1 ..): prev[P] holds D' on entry and D on return, rl[P] the
// keys of the lane's columns (int classes, or u64 word keys: klstm_ctc_consensus.hip).  TRACE (a constant): `code`, declared here, gets
// two bits per slot, the step the fixed walk back takes out of cell (row, j): 0 diagonal with equal keys, 1 diagonal with a substitution,
// 2 up, 3 left.  Expects `lane`.  TEXT: as a function edit_distance<16> comes out with other registers (ctc_nbest_shared_isa.txt).
#define KLSTM_ED_ROW_STEP(P, TRACE, prev, rl, tok, row, code)                                                                        \
  unsigned code = 0;                                                                                                                 \
  {                                                                                                                                  \
    const int up_ = __shfl_up((prev)[(P) - 1], 1);                 /* D'[j - 1] of the lane's first slot */                          \
    int run_ = ED_BIG, v_[P];                                                                                                        \
    _Pragma("unroll") for (int e = 0; e < (P); e++) {                                                                                \
      const int j = lane * (P) + e, diag = e ? (prev)[e - 1] : up_;                                                                  \
      int tmp = min((prev)[e] + 1, diag + ((rl)[e] != (tok)));                                                                       \
      if (j == 0) tmp = (row);                                                                                                       \
      run_ = min(run_, tmp - j);                                                                                                     \
      v_[e] = run_;                                                                                                                  \
    }                                                                                                                                \
    int excl_ = __shfl_up(wave_scan_min(run_), 1), diag_ = up_;                                                                      \
    if (lane == 0) excl_ = ED_BIG;                                                                                                   \
    _Pragma("unroll") for (int e = 0; e < (P); e++) {                                                                                \
      const int j = lane * (P) + e, nw = j + min(v_[e], excl_);                                                                      \
      if (TRACE) {                                                 /* the old row is still in prev */                                \
        const int ne = (rl)[e] != (tok);                                                                                             \
        const unsigned c2 = j == 0 ? 2u : nw == diag_ + ne ? (unsigned)ne : nw == (prev)[e] + 1 ? 2u : 3u;                           \
        code |= c2 << (2 * e);                                                                                                       \
        diag_ = (prev)[e];                                                                                                           \
      }                                                                                                                              \
      (prev)[e] = nw;                                                                                                                \
    }                                                                                                                                \
  }

template <int P, bool COLLAPSE = true>
__device__ int edit_distance(const int *__restrict__ fclass, int S, int s, int len, int blank, const int *__restrict__ ref, int L) {
  const int lane = threadIdx.x & 63;
  int prev[P], rl[P];
#pragma unroll
  for (int e = 0; e < P; e++) {
    const int j = lane * P + e;
    prev[e] = j;
    rl[e] = (j >= 1 && j <= L) ? ref[j - 1] : -2;                  // -2: no class, never equal to a token
  }
  int row = 0;
  for (int t0 = 0; t0 < len; t0 += 64) {
    const int t = t0 + lane;
    const int c = t < len ? fclass[(size_t)t * S + s] : blank;
    const int cb = (COLLAPSE && t > 0 && t < len) ? fclass[(size_t)(t - 1) * S + s] : -1;
    unsigned long long mask = __ballot(c != blank && (!COLLAPSE || c != cb));
    while (mask) {
      const int k = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int tok = __shfl(c, k);
      row++;
      KLSTM_ED_ROW_STEP(P, false, prev, rl, tok, row, code) (void)code;
    }
  }
  int out = 0;
#pragma unroll
  for (int e = 0; e < P; e++) if (lane * P + e == L) out = prev[e];
  return __shfl(out, L / P);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// One chain of the CTC lattice of `lab[0 .. L)` over the `len` frames of one stream, by the whole workgroup of 64 NW threads with P
// states per thread: dir 0 alpha (forwards, the frame's emission included), dir 1 beta (backwards, without it).  ys:
// the stream's row 0 of the posteriors, tstride: elements between its frames.  The normalised row of frame t goes to gout[t * Npad +
// state].  Returns log p(lab | y) = the offsets summed in double plus the last row's tail (valid on thread 0 of an alpha chain).  The
// caller has established that the labelling is feasible (ctc_status 1) and that 2 L + 1 <= 64 NW P.  Shared by klstm_ctc.hip (the loss)
// and klstm_ctc_mbr.hip (the n-best risk), whose log probabilities therefore carry the same bits.
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int CTC_DEPTH = 4;           // steps the emission gather runs ahead of the chain

template <int NW, int P>
__device__ __forceinline__ double ctc_chain_run(const float *__restrict__ ys, size_t tstride, int len, const int *__restrict__ lab, int L,
                                                int blank, int dir, float *__restrict__ gout, int Npad) {
  constexpr int NT = 64 * NW, CAP = NT * P;
  __shared__ float row[2][CAP + 4];           // state i at [i + 2]; two cells of CTC_NEG on either side
  __shared__ float pmax[2][NW];
  const int tid = threadIdx.x;
  const int N = 2 * L + 1;
  const int sgn = dir ? 1 : -1;                // neighbours i + sgn, i + 2 sgn
  const float *yp[P];
  bool act[P], allow2[P];
  float w[P], base0[P];
#pragma unroll
  for (int k = 0; k < P; k++) {
    const int i = tid + k * NT;
    act[k] = i < N;
    const int cls = (act[k] && (i & 1)) ? lab[i >> 1] : blank;
    yp[k] = ys + cls;
    const int j = dir ? i + 2 : i;             // the state a skip would arrive at
    allow2[k] = act[k] && (j & 1) && j >= 3 && j < N && lab[j >> 1] != lab[(j >> 1) - 1];
    base0[k] = !act[k] ? CTC_NEG : dir ? (i >= N - 2 ? 0.f : CTC_NEG) : (i <= 1 ? 0.f : CTC_NEG);
    w[k] = CTC_NEG;
  }
  if (tid < 2) {
    row[0][tid] = CTC_NEG; row[1][tid] = CTC_NEG;
    row[0][CAP + 2 + tid] = CTC_NEG; row[1][CAP + 2 + tid] = CTC_NEG;
  }

  float en[CTC_DEPTH][P];
#pragma unroll
  for (int d = 0; d < CTC_DEPTH; d++)
#pragma unroll
    for (int k = 0; k < P; k++) en[d][k] = d < len ? yp[k][(size_t)(dir ? len - 1 - d : d) * tstride] : 1.f;

  double csum = 0.0;                           // sum of the offsets taken out so far (the loss needs it; alpha only)
  float M = 0.f;
  for (int u0 = 0; u0 < len; u0 += CTC_DEPTH) {
    float ec[CTC_DEPTH][P];
#pragma unroll
    for (int d = 0; d < CTC_DEPTH; d++)
#pragma unroll
      for (int k = 0; k < P; k++) {
        ec[d][k] = en[d][k];
        const int un = u0 + CTC_DEPTH + d;
        en[d][k] = un < len ? yp[k][(size_t)(dir ? len - 1 - un : un) * tstride] : 1.f;
      }
#pragma unroll
    for (int d = 0; d < CTC_DEPTH; d++) {
      const int u = u0 + d;
      if (u >= len) break;
      const int b = u & 1, tt = dir ? len - 1 - u : u;
      float lmax = CTC_NEG;
      if (u > 0) csum += (double)M;
#pragma unroll
      for (int k = 0; k < P; k++) {
        const int i = tid + k * NT;
        float base = base0[k];
        if (u > 0) {
          const float x0 = w[k], x1 = row[b ^ 1][i + 2 + sgn];
          const float x2 = allow2[k] ? row[b ^ 1][i + 2 + 2 * sgn] : CTC_NEG;
          const float m = fmaxf(x0, fmaxf(x1, x2));
          base = m + __logf(__expf(x0 - m) + __expf(x1 - m) + __expf(x2 - m)) - M;
        }
        const float em = logf(fmaxf(ec[d][k], FLT_MIN));    // off the chain: the accurate one
        const float wk = act[k] ? base + em : CTC_NEG;
        if (act[k]) gout[(size_t)tt * Npad + i] = dir ? base : wk;
        w[k] = wk;
        lmax = fmaxf(lmax, wk);
      }
#pragma unroll
      for (int k = 0; k < P; k++) row[b][tid + k * NT + 2] = w[k];
      lmax = wave_max(lmax);
      if (NW > 1) {
        if ((tid & 63) == 0) pmax[b][tid >> 6] = lmax;
      }
      __syncthreads();
      if (NW > 1) {
        lmax = pmax[b][0];
#pragma unroll
        for (int q = 1; q < NW; q++) lmax = fmaxf(lmax, pmax[b][q]);
      }
      M = lmax;
    }
  }
  double lp = 0.0;
  if (dir == 0 && tid == 0) {
    const int b = (len - 1) & 1;
    const float a1 = row[b][N - 1 + 2], a2 = N > 1 ? row[b][N - 2 + 2] : CTC_NEG;
    const float m = fmaxf(a1, a2);
    const float tail = m + logf(expf(a1 - m) + expf(a2 - m));
    lp = csum + (double)tail;
  }
  return lp;
}

}  // namespace klstm
