// kaldi-lstm_amd/csrc/klstm_ctc_mbr.hip -- minimum expected token error over CTC n-best lists (klstm_ctc_mbr_eval of include/klstm.h;
// DESIGN.md 4n).  For every stream a list of labellings h_q with integer costs W_q (the arrays klstm_ctc_beam_decode wrote):
//   l_q = log p(h_q | y),  P_q = softmax_q(kappa l_q),  R = sum_q P_q W_q,  c_q = P_q (W_q - R),
//   diff = kappa sum_q c_q gamma_q + lambda (y - gamma_ref)          (with respect to the softmax input, as klstm_ctc_eval)
// Three launches, E = list slots (+ 1 for the reference when lambda > 0) entries per stream:
//   k_mbr_chain    grid (S E, 3).  y = 0 / 1: the alpha / beta chain of ONE entry (ctc_chain_run of klstm_ctc_dev.h, the step of
//                  klstm_ctc_eval: the log probabilities carry its bits), y = 2: the entry's status and its next / first links
//                  (ctc_links).  The plan is the loss's (ctc_chain_plan of klstm_ctc_host.h, from the same capacity).  All
//                  S E chains run side by side.
//   k_mbr_weights  grid (S).  The stream's status; P, R, c in double by one thread, q ascending; the slot of every class that occurs
//                  in the stream's list (an accumulator index for the third launch).
//   k_mbr_combine  grid (T S).  One row each: per entry in order gamma from alpha + beta by the text k_ctc_combine expands, c_q gamma_q added
//                  into an LDS accumulator (one slot per class of the list, the blank's in a register), then the row written ONCE:
//                  lambda y (or zero) coalesced, the slots scattered on top.  Row 0 adds the statistics onto the totals.
// DETERMINISM.  No floating-point atomics.  Within a labelling a class is summed by the thread of its first position, so no two threads
// of one pass share a slot; a barrier separates the labellings, which are taken q ascending, the reference last.  WHICH slot a class
// gets is decided by an integer atomic and may differ from run to run; no value depends on it.
#include <cfloat>
#include <cmath>

#include "../../include/klstm.h"
#include "klstm_ctc_dev.h"
#include "klstm_ctc_host.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int MBR_KMAX = 32768;        // the class map of the workspace is sized for the largest K the entry takes

// the caller's arrays.  N list slots per stream; entry N (where E == N + 1) is the reference
struct MbrIn { const int *lens, *hyp, *hyp_len, *count, *errors, *ref, *roff; int hyp_stride, N, T, K, blank; };
// the workspace.  info [S]: 0 idle, 1 counted, 2 rejected, 3 skipped; einfo [S E]: 1 = the entry is feasible; link [S E][3 Lcap]: next
// position of the same class, first-of-its-class flag, accumulator slot; cmap [S][K]: class -> slot; sclass [S][E Lcap]: slot -> class
struct MbrWs { int *info, *einfo, *nslot, *link, *cmap, *sclass; double *logp; float *coef, *A, *B; int Npad, Lcap, E, slotcap; };

static size_t mbr_layout(int T, int S, int N, int Lcap, int with_ref, void *base, MbrWs &ws) {
  const size_t E = (size_t)N + (with_ref ? 1 : 0), npad = ctc_npad(Lcap), SE = (size_t)S * E;
  CtcCarver c(base);
  ws.logp = c.take<double>(SE);
  ws.coef = c.take<float>(SE);
  ws.info = c.take<int>(S);
  ws.nslot = c.take<int>(S);
  ws.einfo = c.take<int>(SE);
  ws.cmap = c.take<int>((size_t)S * MBR_KMAX);
  ws.sclass = c.take<int>(SE * (size_t)Lcap);
  ws.link = c.take<int>(SE * 3 * (size_t)Lcap);
  ws.A = c.packed<float>((size_t)T * SE * npad);
  ws.B = c.packed<float>((size_t)T * SE * npad);
  ws.Npad = (int)npad;
  ws.Lcap = Lcap;
  ws.E = (int)E;
  ws.slotcap = (int)E * Lcap;
  return c.bytes();
}

size_t ctc_mbr_workspace_bytes(int T, int S, int N, int Lcap, int with_ref) {
  MbrWs ws;
  return mbr_layout(T, S, N, Lcap, with_ref, nullptr, ws);
}

int ctc_mbr_label_capacity(int T, int S, int N, int with_ref, size_t bytes) {
  return ctc_label_capacity_of(bytes, [&](int Lcap) { return ctc_mbr_workspace_bytes(T, S, N, Lcap, with_ref); });
}

// the labels of entry e of stream s and their number
__device__ __forceinline__ const int *mbr_entry(const MbrIn &a, int s, int e, int &L) {
  if (e == a.N) { L = a.roff[s + 1] - a.roff[s]; return a.ref + a.roff[s]; }
  L = a.hyp_len[s * a.N + e];
  return a.hyp + (size_t)(s * a.N + e) * a.hyp_stride;
}
// what a stream needs before any of its entries is looked at: a valid length, a non-empty list, every listed cost counted
__device__ __forceinline__ bool mbr_stream_open(const MbrIn &a, int s) {
  const int len = a.lens[s], cnt = a.count[s];
  if (len <= 0 || len > a.T || cnt <= 0 || cnt > a.N) return false;
  for (int q = 0; q < cnt; q++) if (a.errors[s * a.N + q] < 0) return false;
  return true;
}
// 1: entry e of stream s is listed and feasible (klstm_ctc_eval's rule, and no longer than its row).  Uniform; sm: 2 ints of LDS
__device__ __forceinline__ int mbr_entry_ok(const MbrIn &a, int s, int e, int Lcap, int *sm, const int *&lab, int &L) {
  if (e < a.N && e >= a.count[s]) return 0;
  lab = mbr_entry(a, s, e, L);
  if (e < a.N && L > a.hyp_stride) return 0;
  return ctc_status(a.lens[s], a.T, L, Lcap, lab, a.K, a.blank, sm) == 1;
}

template <int NW, int P>
__global__ __launch_bounds__(64 * NW) void k_mbr_chain(const float *__restrict__ y, int S, int stride, MbrIn a, MbrWs ws) {
  constexpr int NT = 64 * NW;
  __shared__ int sm[2];
  const int s = blockIdx.x / ws.E, e = blockIdx.x % ws.E, dir = blockIdx.y, tid = threadIdx.x;
  const int se = s * ws.E + e;
  const bool with_ref = ws.E > a.N;
  const int *lab = nullptr;
  int L = 0, ref_ok = 1, ok = 0;
  const int len = a.lens[s];
  if (with_ref && len > 0 && len <= a.T) ref_ok = mbr_entry_ok(a, s, a.N, ws.Lcap, sm, lab, L);
  const bool open = ref_ok && mbr_stream_open(a, s);
  if (open && e == a.N) {                      // the reference's chains are needed only where a list entry is feasible
    const int cnt = a.count[s];
    for (int q = 0; q < cnt && !ok; q++) ok = mbr_entry_ok(a, s, q, ws.Lcap, sm, lab, L);
  }
  if (open && (e < a.N || ok)) ok = mbr_entry_ok(a, s, e, ws.Lcap, sm, lab, L);

  if (dir == 2) {                              // bookkeeping for the launches that follow
    if (tid == 0) ws.einfo[se] = e == a.N ? ref_ok : ok;       // the reference: its own status, whatever the list's
    if (!ok) return;
    int *next = ws.link + (size_t)se * 3 * ws.Lcap, *first = next + ws.Lcap;
    ctc_links(lab, L, next, first, NT);
    return;
  }
  if (!ok) return;
  float *gout = (dir ? ws.B : ws.A) + (size_t)se * a.T * ws.Npad;
  const double lp = ctc_chain_run<NW, P>(y + (size_t)s * stride, (size_t)S * stride, len, lab, L, a.blank, dir, gout, ws.Npad);
  if (dir == 0 && tid == 0) ws.logp[se] = lp;
}

__global__ __launch_bounds__(256) void k_mbr_weights(int S, MbrIn a, float kappa, float lam, float *__restrict__ risk,
                                                     float *__restrict__ hyp_logp, float *__restrict__ hyp_post,
                                                     float *__restrict__ ref_loss, MbrWs ws) {
  __shared__ int sh_st, sh_slots;
  __shared__ double wexp[16];                  // exp(kappa l_q - max) of the listed entries (list_n <= 16)
  const int s = blockIdx.x, tid = threadIdx.x, N = a.N, E = ws.E;
  const bool with_ref = E > N;
  if (tid == 0) {
    const int len = a.lens[s], cnt = a.count[s];
    int st = 1;
    if (len == 0) st = 0;
    else if (len < 0 || len > a.T || cnt < 0 || cnt > N || (with_ref && !ws.einfo[s * E + N])) st = 2;
    else {
      int feasible = 0;
      bool uncounted = false;
      for (int q = 0; q < cnt; q++) { uncounted |= a.errors[s * N + q] < 0; feasible += ws.einfo[s * E + q]; }
      if (cnt == 0 || uncounted || feasible == 0) st = 3;
    }
    double R = 0.0, inv = 0.0, m = -INFINITY;
    if (st == 1) {
      for (int q = 0; q < cnt; q++) if (ws.einfo[s * E + q]) m = fmax(m, (double)kappa * ws.logp[s * E + q]);
      double Z = 0.0;
      for (int q = 0; q < cnt; q++) {
        wexp[q] = ws.einfo[s * E + q] ? exp((double)kappa * ws.logp[s * E + q] - m) : 0.0;
        Z += wexp[q];
      }
      inv = 1.0 / Z;
      for (int q = 0; q < cnt; q++) if (ws.einfo[s * E + q]) R += wexp[q] * inv * (double)a.errors[s * N + q];
    }
    for (int q = 0; q < N; q++) {
      const bool live = st == 1 && q < cnt && ws.einfo[s * E + q];
      const double Pq = live ? wexp[q] * inv : 0.0;
      ws.coef[s * E + q] = live ? (float)((double)kappa * (Pq * ((double)a.errors[s * N + q] - R))) : 0.f;
      if (hyp_logp) hyp_logp[s * N + q] = live ? (float)ws.logp[s * E + q] : -INFINITY;
      if (hyp_post) hyp_post[s * N + q] = (float)Pq;
    }
    if (with_ref) ws.coef[s * E + N] = -lam;
    risk[s] = st == 1 ? (float)R : st == 0 ? 0.f : -1.f;
    if (ref_loss) ref_loss[s] = (st == 1 && with_ref) ? (float)(-ws.logp[s * E + N]) : 0.f;
    ws.info[s] = st;
    sh_st = st;
    sh_slots = 0;
  }
  __syncthreads();
  if (sh_st != 1) return;
  // the accumulator slot of every class that occurs in a feasible entry of the stream
  int *cmap = ws.cmap + (size_t)s * a.K, *sclass = ws.sclass + (size_t)s * ws.slotcap;
  for (int c = tid; c < a.K; c += 256) cmap[c] = -1;
  __syncthreads();
  for (int e = 0; e < E; e++) {
    if (!ws.einfo[s * E + e] || (e < N && e >= a.count[s])) continue;
    int L;
    const int *lab = mbr_entry(a, s, e, L);
    for (int j = tid; j < L; j += 256) cmap[lab[j]] = -2;       // several writers, one value
  }
  __syncthreads();
  for (int c = tid; c < a.K; c += 256)
    if (cmap[c] == -2) {
      const int id = atomicAdd(&sh_slots, 1);                   // integer: which slot a class gets changes no value
      cmap[c] = id;
      sclass[id] = c;
    }
  __syncthreads();
  for (int e = 0; e < E; e++) {
    if (!ws.einfo[s * E + e] || (e < N && e >= a.count[s])) continue;
    int L;
    const int *lab = mbr_entry(a, s, e, L);
    int *slot = ws.link + ((size_t)(s * E + e) * 3 + 2) * ws.Lcap;
    for (int j = tid; j < L; j += 256) slot[j] = cmap[lab[j]];
  }
  if (tid == 0) ws.nslot[s] = sh_slots;
}

__global__ __launch_bounds__(256) void k_mbr_combine(const float *__restrict__ y, int S, int stride, MbrIn a, float lam,
                                                     float *__restrict__ diff, int dstride, const float *__restrict__ risk,
                                                     double *__restrict__ totals, MbrWs ws, int vec) {
  extern __shared__ float acc[];               // one slot per class of the stream's list
  __shared__ float g[2048];
  __shared__ float sm[4];
  const int r = blockIdx.x, s = r % S, t = r / S, tid = threadIdx.x, K = a.K, N = a.N, E = ws.E;
  if (r == 0 && totals && tid == 0) {          // the minibatch's statistics, streams in order
    double R = 0, first = 0, cnt = 0, out = 0, frames = 0, rl = 0;
    for (int q = 0; q < S; q++) {
      const int st = ws.info[q];
      if (st == 1) {
        R += (double)risk[q]; first += (double)a.errors[q * N]; cnt += 1; frames += a.lens[q];
        if (E > N) rl += (double)(float)(-ws.logp[q * E + N]);
      } else if (st >= 2) out += 1;
    }
    totals[0] += R; totals[1] += first; totals[2] += cnt; totals[3] += out; totals[4] += frames; totals[5] += rl;
  }
  float *dp = diff + (size_t)r * dstride;
  const float *yp = y + (size_t)r * stride;
  if (ws.info[s] != 1 || t >= a.lens[s]) {
    ctc_zero_row(dp, K, vec);
    return;
  }
  const int nsl = ws.nslot[s], cnt = a.count[s];
  for (int i = tid; i < nsl; i += 256) acc[i] = 0.f;
  float bacc = 0.f;                            // the blank's column (the same in every thread)
  for (int e = 0; e < E; e++) {
    if ((e < N && e >= cnt) || !ws.einfo[s * E + e]) continue;
    const float cf = ws.coef[s * E + e];
    int L;
    mbr_entry(a, s, e, L);
    const int NS = 2 * L + 1;
    const size_t rowoff = ((size_t)(s * E + e) * a.T + t) * ws.Npad;
    const float *al = ws.A + rowoff, *bt = ws.B + rowoff;
    __syncthreads();                           // the pass before is done with g; its slots are final
    KLSTM_CTC_GAMMA_ROW(float, ctc_block_sum, sm, al, bt, NS, g, sall, seven)
    const float inv = 1.f / sall;
    bacc += cf * (seven * inv);
    __syncthreads();                           // g complete
    const int *next = ws.link + (size_t)(s * E + e) * 3 * ws.Lcap, *first = next + ws.Lcap, *slot = first + ws.Lcap;
    for (int j = tid; j < L; j += 256) {
      if (!first[j]) continue;
      float sum = g[2 * j + 1];
      for (int q = next[j]; q >= 0; q = next[q]) sum += g[2 * q + 1];
      acc[slot[j]] += cf * (sum * inv);        // the only thread of this pass on that slot
    }
  }
  if (lam > 0.f) {
    if (vec) for (int c = tid * 4; c < K; c += 1024) {
      const float4 v = *reinterpret_cast<const float4 *>(yp + c);
      *reinterpret_cast<float4 *>(dp + c) = make_float4(lam * v.x, lam * v.y, lam * v.z, lam * v.w);
    } else for (int c = tid; c < K; c += 256) dp[c] = lam * yp[c];
  } else ctc_zero_row(dp, K, vec);
  __syncthreads();                             // the slots are final, the row is visible to the threads that correct it
  if (tid == 0) dp[a.blank] = (lam > 0.f ? lam * yp[a.blank] : 0.f) + bacc;
  const int *sclass = ws.sclass + (size_t)s * ws.slotcap;
  for (int i = tid; i < nsl; i += 256) {
    const int c = sclass[i];
    dp[c] = (lam > 0.f ? lam * yp[c] : 0.f) + acc[i];
  }
}

hipError_t launch_ctc_mbr(const float *y, int T, int S, int K, int stride, const int *lens, int blank, const int *hyp, int hyp_stride,
                          const int *hyp_len, const int *count, const int *errors, int N, const int *ref, const int *roff, float kappa,
                          float lam, float *diff, int dstride, float *risk, float *hyp_logp, float *hyp_post, float *ref_loss,
                          double *totals, void *workspace, int Lcap, hipStream_t st) {
  MbrWs ws;
  mbr_layout(T, S, N, Lcap, ref != nullptr, workspace, ws);
  const MbrIn in{lens, hyp, hyp_len, count, errors, ref, roff, hyp_stride, N, T, K, blank};
  hipError_t err = ctc_chain_dispatch(ctc_chain_plan(2 * Lcap + 1), hipErrorInvalidValue, [&](auto nw, auto p) {
    return launch(k_mbr_chain<nw(), p()>, dim3(S * ws.E, 3), dim3(64 * nw()), 0, st, LaunchProbe{}, y, S, stride, in, ws);
  });
  if (err != hipSuccess) return err;
  err = launch(k_mbr_weights, dim3(S), dim3(256), 0, st, LaunchProbe{}, S, in, kappa, lam, risk, hyp_logp, hyp_post, ref_loss, ws);
  if (err != hipSuccess) return err;
  const int vec = ctc_rows_vec(K, stride, dstride, y, diff);
  const int slots = ws.slotcap < K ? ws.slotcap : K;
  const size_t shm = (size_t)(slots > 0 ? slots : 1) * sizeof(float);
  return launch(k_mbr_combine, dim3(T * S), dim3(256), shm, st, LaunchProbe{}, y, S, stride, in, lam, diff, dstride, (const float *)risk,
                totals, ws, vec);
}

}  // namespace klstm
