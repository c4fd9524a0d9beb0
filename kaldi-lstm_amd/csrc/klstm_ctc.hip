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
#include "klstm_ctc_host.h"
#include "klstm_kernels.h"

namespace klstm {

template <int NW, int P>
__global__ __launch_bounds__(64 * NW) void k_ctc_chain(const float *__restrict__ y, int T, int S, int K, int stride,
                                                       const int *__restrict__ lens, const int *__restrict__ labels,
                                                       const int *__restrict__ loff, int blank, float *__restrict__ utt_loss, CtcWs ws) {
  constexpr int NT = 64 * NW;
  __shared__ int sm[2];
  const int s = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int L = loff[s + 1] - loff[s], len = lens[s];
  const int *lab = labels + loff[s];
  const int st = ctc_status(len, T, L, ws.Lcap, lab, K, blank, sm);

  if (dir == 2) {                              // bookkeeping for k_ctc_combine
    if (tid == 0) ws.info[s] = st;
    if (st != 1) return;
    int *next = ws.link + (size_t)s * 2 * ws.Lcap, *first = next + ws.Lcap;
    ctc_links(lab, L, next, first, NT);
    return;
  }
  if (st != 1) {
    if (dir == 0 && tid == 0) utt_loss[s] = st == 2 ? INFINITY : 0.f;
    return;
  }

  float *gout = (dir ? ws.B : ws.A) + (size_t)s * T * ws.Npad;
  const double lp = ctc_chain_run<NW, P>(y + (size_t)s * stride, (size_t)S * stride, len, lab, L, blank, dir, gout, ws.Npad);
  if (dir == 0 && tid == 0) utt_loss[s] = (float)(-lp);
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
    ctc_zero_row(dp, K, vec);
    return;
  }
  const int L = loff[s + 1] - loff[s], N = 2 * L + 1;
  const int *lab = labels + loff[s];
  const float *a = ws.A + ((size_t)s * T + t) * ws.Npad, *bt = ws.B + ((size_t)s * T + t) * ws.Npad;
  KLSTM_CTC_GAMMA_ROW(float, ctc_block_sum, sm, a, bt, N, g, sall, seven)
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

static size_t ctc_layout(int T, int S, int Lcap, void *base, CtcWs *ws) {
  const size_t npad = ctc_npad(Lcap), head = ctc_up256((size_t)S * (1 + 2 * (size_t)Lcap) * sizeof(int));
  if (ws) {
    ws->info = reinterpret_cast<int *>(base);
    ws->link = ws->info + S;
    ws->A = reinterpret_cast<float *>(reinterpret_cast<char *>(base) + head);
    ws->B = ws->A + (size_t)T * S * npad;
    ws->Npad = (int)npad;
    ws->Lcap = Lcap;
  }
  return head + 2 * (size_t)T * S * npad * sizeof(float);
}

size_t ctc_workspace_bytes(int T, int S, int Lcap) { return ctc_layout(T, S, Lcap, nullptr, nullptr); }

int ctc_label_capacity(int T, int S, size_t bytes) {
  return ctc_label_capacity_of(bytes, [&](int Lcap) { return ctc_workspace_bytes(T, S, Lcap); });
}

hipError_t launch_ctc(const float *y, int T, int S, int K, int stride, const int *lens, const int *labels, const int *loff, int blank,
                      float *diff, int dstride, float *utt_loss, double *totals, void *workspace, int Lcap, hipStream_t st) {
  CtcWs ws;
  ctc_layout(T, S, Lcap, workspace, &ws);
  const hipError_t err = ctc_chain_dispatch(ctc_chain_plan(2 * Lcap + 1), hipErrorInvalidValue, [&](auto nw, auto p) {
    return launch(k_ctc_chain<nw(), p()>, dim3(S, 3), dim3(64 * nw()), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, labels, loff, blank,
                  utt_loss, ws);
  });
  if (err != hipSuccess) return err;
  return launch(k_ctc_combine, dim3(T * S), dim3(256), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, labels, loff, blank, diff, dstride,
                (const float *)utt_loss, totals, ws, ctc_rows_vec(K, stride, dstride, y, diff));
}

}  // namespace klstm
