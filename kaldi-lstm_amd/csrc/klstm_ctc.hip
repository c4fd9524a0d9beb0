// kaldi-lstm_amd/csrc/klstm_ctc.hip -- connectionist temporal classification on whole utterances (klstm_ctc_eval of include/klstm.h;
// DESIGN.md 4h).  Two launches:
//   k_ctc_chain    grid (S, 3).  y = 0: the alpha chain of stream s, y = 1: its beta chain, y = 2: the label bookkeeping of stream s
//                  (feasibility word, and for every label position the next position that carries the same class).  The 2L+1 states
//                  of an utterance are spread over the threads of ONE workgroup (state i on thread i % threads), the previous row
//                  lives in LDS (double-buffered: one barrier per step, none at all when the workgroup is a single wave).
//   k_ctc_combine  grid (T*S).  One row each: gamma from alpha + beta, diff = y - gamma, zero rows for padding / idle / rejected
//                  streams; row 0 also adds the minibatch's statistics onto the totals, streams in order.
// NUMBERS.  Both recursions stay in the log domain but NORMALISED: the row written at step u is taken relative to the maximum of the
// row before it, so the stored values are of the size of one frame's log posteriors (not of log alpha ~ -1e3, whose ulp of 1e-4 is what
// costs stock fp32 CTC its gradient digits).  gamma is normalised per frame, so the offsets cancel there; the loss needs their sum,
// which the alpha chain keeps in double.  alpha includes the frame's emission, beta does not (gamma ~ exp(alpha + beta)).
// DETERMINISM.  No floating-point atomics.  Every reduction is a fixed tree over a fixed workgroup size; a class that appears several
// times in a label sequence is summed by the thread of its FIRST position, walking the positions in order; the blank's L+1 states are a
// tree over the even states.
#include <cfloat>
#include <cmath>

#include "../../include/klstm.h"
#include "klstm_ctc_dev.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int CTC_DEPTH = 4;           // steps the emission gather runs ahead of the chain

template <int NW, int P>
__global__ __launch_bounds__(64 * NW) void k_ctc_chain(const float *__restrict__ y, int T, int S, int K, int stride,
                                                       const int *__restrict__ lens, const int *__restrict__ labels,
                                                       const int *__restrict__ loff, int blank, float *__restrict__ utt_loss, CtcWs ws) {
  constexpr int NT = 64 * NW, CAP = NT * P;
  __shared__ float row[2][CAP + 4];           // state i at [i + 2]; two cells of CTC_NEG on either side
  __shared__ float pmax[2][NW];
  __shared__ int sm[2];
  const int s = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int L = loff[s + 1] - loff[s], len = lens[s];
  const int *lab = labels + loff[s];
  const int st = ctc_status(len, T, L, ws.Lcap, lab, K, blank, sm);

  if (dir == 2) {                              // bookkeeping for k_ctc_combine
    if (tid == 0) ws.info[s] = st;
    if (st != 1) return;
    int *next = ws.link + (size_t)s * 2 * ws.Lcap, *first = next + ws.Lcap;
    for (int j = tid; j < L; j += NT) first[j] = 1;
    __syncthreads();
    for (int j = tid; j < L; j += NT) {
      const int c = lab[j];
      int q = j + 1;
      while (q < L && lab[q] != c) q++;
      next[j] = q < L ? q : -1;
      if (q < L) first[q] = 0;                 // position q has exactly one predecessor: one writer
    }
    return;
  }
  if (st != 1) {
    if (dir == 0 && tid == 0) utt_loss[s] = st == 2 ? INFINITY : 0.f;
    return;
  }

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
    yp[k] = y + (size_t)s * stride + cls;
    const int j = dir ? i + 2 : i;             // the state a skip would arrive at
    allow2[k] = act[k] && (j & 1) && j >= 3 && j < N && lab[j >> 1] != lab[(j >> 1) - 1];
    base0[k] = !act[k] ? CTC_NEG : dir ? (i >= N - 2 ? 0.f : CTC_NEG) : (i <= 1 ? 0.f : CTC_NEG);
    w[k] = CTC_NEG;
  }
  if (tid < 2) {
    row[0][tid] = CTC_NEG; row[1][tid] = CTC_NEG;
    row[0][CAP + 2 + tid] = CTC_NEG; row[1][CAP + 2 + tid] = CTC_NEG;
  }
  const size_t tstride = (size_t)S * stride;
  float *gout = (dir ? ws.B : ws.A) + (size_t)s * T * ws.Npad;

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
        if (act[k]) gout[(size_t)tt * ws.Npad + i] = dir ? base : wk;
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
  if (dir == 0 && tid == 0) {
    const int b = (len - 1) & 1;
    const float a1 = row[b][N - 1 + 2], a2 = N > 1 ? row[b][N - 2 + 2] : CTC_NEG;
    const float m = fmaxf(a1, a2);
    const float tail = m + logf(expf(a1 - m) + expf(a2 - m));
    utt_loss[s] = (float)(-(csum + (double)tail));
  }
}

__device__ __forceinline__ float ctc_block_reduce(float v, float *sm, bool is_max) {     // 256 threads, fixed tree
  for (int o = 32; o > 0; o >>= 1) { const float x = __shfl_xor(v, o); v = is_max ? fmaxf(v, x) : v + x; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return is_max ? fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])) : (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(256) void k_ctc_combine(const float *__restrict__ y, int T, int S, int K, int stride,
                                                     const int *__restrict__ lens, const int *__restrict__ labels,
                                                     const int *__restrict__ loff, int blank, float *__restrict__ diff, int dstride,
                                                     const float *__restrict__ utt_loss, double *__restrict__ totals, CtcWs ws, int vec) {
  __shared__ float g[2048];
  __shared__ float sm[4];
  const int r = blockIdx.x, s = r % S, t = r / S, tid = threadIdx.x;
  if (r == 0 && totals && tid == 0) {          // the minibatch's statistics, streams in order
    double loss = 0, cnt = 0, rej = 0, frames = 0;
    for (int q = 0; q < S; q++) {
      const int st = ws.info[q];
      if (st == 1) { loss += (double)utt_loss[q]; cnt += 1; frames += lens[q]; }
      else if (st == 2) rej += 1;
    }
    totals[0] += loss; totals[1] += cnt; totals[2] += rej; totals[3] += frames;
  }
  float *dp = diff + (size_t)r * dstride;
  const float *yp = y + (size_t)r * stride;
  if (ws.info[s] != 1 || t >= lens[s]) {
    if (vec) for (int c = tid * 4; c < K; c += 1024) *reinterpret_cast<float4 *>(dp + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    else for (int c = tid; c < K; c += 256) dp[c] = 0.f;
    return;
  }
  const int L = loff[s + 1] - loff[s], N = 2 * L + 1;
  const int *lab = labels + loff[s];
  const float *a = ws.A + ((size_t)s * T + t) * ws.Npad, *bt = ws.B + ((size_t)s * T + t) * ws.Npad;
  float mx = CTC_NEG;
  for (int i = tid; i < N; i += 256) { const float v = a[i] + bt[i]; g[i] = v; mx = fmaxf(mx, v); }
  mx = ctc_block_reduce(mx, sm, true);
  float sall = 0.f, seven = 0.f;
  for (int i = tid; i < N; i += 256) {         // 256 is even: a thread's states are all even or all odd
    const float e = expf(g[i] - mx);
    g[i] = e;
    sall += e;
    seven += (i & 1) ? 0.f : e;
  }
  sall = ctc_block_reduce(sall, sm, false);
  seven = ctc_block_reduce(seven, sm, false);
  const float inv = 1.f / sall;
  if (vec) for (int c = tid * 4; c < K; c += 1024) *reinterpret_cast<float4 *>(dp + c) = *reinterpret_cast<const float4 *>(yp + c);
  else for (int c = tid; c < K; c += 256) dp[c] = yp[c];
  __syncthreads();                             // g complete, the copied row visible to the threads that correct it
  if (tid == 0) dp[blank] = yp[blank] - seven * inv;
  const int *next = ws.link + (size_t)s * 2 * ws.Lcap, *first = next + ws.Lcap;
  for (int j = tid; j < L; j += 256) {
    if (!first[j]) continue;
    float acc = g[2 * j + 1];
    for (int q = next[j]; q >= 0; q = next[q]) acc += g[2 * q + 1];
    const int c = lab[j];
    dp[c] = yp[c] - acc * inv;
  }
}

size_t ctc_workspace_bytes(int T, int S, int Lcap) {
  const size_t npad = ((size_t)2 * Lcap + 1 + 3) / 4 * 4;
  const size_t head = ((size_t)S * (1 + 2 * (size_t)Lcap) * sizeof(int) + 255) / 256 * 256;
  return head + 2 * (size_t)T * S * npad * sizeof(float);
}

int ctc_label_capacity(int T, int S, size_t bytes) {        // the longest label sequence a workspace of `bytes` serves; -1: none
  if (bytes < ctc_workspace_bytes(T, S, 0)) return -1;
  int lo = 0, hi = 1023;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (ctc_workspace_bytes(T, S, mid) <= bytes) lo = mid; else hi = mid - 1;
  }
  return lo;
}

static bool ctc_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t launch_ctc(const float *y, int T, int S, int K, int stride, const int *lens, const int *labels, const int *loff, int blank,
                      float *diff, int dstride, float *utt_loss, double *totals, void *workspace, int Lcap, hipStream_t st) {
  CtcWs ws;
  ws.Lcap = Lcap;
  ws.Npad = (2 * Lcap + 1 + 3) / 4 * 4;
  const size_t head = ((size_t)S * (1 + 2 * (size_t)Lcap) * sizeof(int) + 255) / 256 * 256;
  ws.info = reinterpret_cast<int *>(workspace);
  ws.link = ws.info + S;
  ws.A = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + head);
  ws.B = ws.A + (size_t)T * S * ws.Npad;
  const int N = 2 * Lcap + 1;
  // measured: four waves with one state per thread beat one wave with two (391 against 487 us at T = 1000, 101 states)
  // -- the step is bound by its exp / log issue slots, which more waves on more SIMDs share, and the workgroup barrier costs less than
  // a second state per lane; sixteen waves lose to four with two states each (670 against 633 us at 301 states), so they serve only
  // what four cannot hold.  16 * waves + states per thread:
  const int plan = N <= 64 ? 16 * 1 + 1 : N <= 256 ? 16 * 4 + 1 : N <= 512 ? 16 * 4 + 2 : N <= 1024 ? 16 * 16 + 1 : 16 * 16 + 2;
  const dim3 grid(S, 3);
  hipError_t err;
#define CTC_CASE(NW, P)                                                                                                              \
  case 16 * NW + P:                                                                                                                  \
    err = launch(k_ctc_chain<NW, P>, grid, dim3(64 * NW), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, labels, loff, blank, utt_loss, ws); \
    break;
  switch (plan) {
    CTC_CASE(1, 1) CTC_CASE(4, 1) CTC_CASE(4, 2) CTC_CASE(16, 1) CTC_CASE(16, 2)
    default: return hipErrorInvalidValue;
  }
#undef CTC_CASE
  if (err != hipSuccess) return err;
  const int vec = K % 4 == 0 && stride % 4 == 0 && dstride % 4 == 0 && ctc_al16(y) && ctc_al16(diff);
  return launch(k_ctc_combine, dim3(T * S), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, labels, loff, blank, diff, dstride,
                (const float *)utt_loss, totals, ws, vec);
}

}  // namespace klstm
