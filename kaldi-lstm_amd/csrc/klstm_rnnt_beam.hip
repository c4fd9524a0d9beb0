// kaldi-lstm_amd/csrc/klstm_rnnt_beam.hip -- transducer beam search with n-best lists: the krnnt_beam_* entries of include/klstm_rnnt.h
// (which states the search and every score; the torch yardstick: tests/rnnt_beam_ref.py) and their kernels.  The search is
// label-synchronous like the greedy one: in step u every live slot (s, b) holds a prefix of u labels, its predictor row is fixed, and
// all its frames are met against that one row (joint_logits() of klstm_rnnt_dev.h, 16 frames per M-tile).  What a slot needs from its
// parent is one column, e(t) = alpha_parent(t) + lpy_parent(t, label): the state's E [S B][T] in double.
//   k_rnnt_beam_begin    grid S: the stream's status, slot 0 live with E = (0, log 0, ...), the bos row, parents -1, an empty list.
//   k_rnnt_beam_scan     grid (ceil(T / FB), S B), 4 waves, FB = 64 frames (wave w: frames 16 w ..; 32 for J > 512, where waves 2 and 3
//                        only help to load the W panels).  Sweep 1 over the class passes: per frame the running max and sum and the
//                        blank's logit -> lse(t) as (max, log sum), lpb(t).  Then wave 0, lane = frame, in double: Bl (an exclusive prefix sum, shuffles in
//                        a fixed order), Cl (an inclusive logadd scan of e - Bl), the per-frame records and the chunk's (Bl(f1),
//                        Cl(f1-1), offY); the weights wx(t) = Bl(t) and wy(t) = Bl(t) + Cl(t) - offY go to LDS as floats.  Sweep 2 over
//                        the class passes: per class X_k = logsumexp_t (wx + lpy), Y_k likewise with wy -- a lane of the C layout holds
//                        four frames of one class as (max, sum), the lanes of a column merge by a butterfly over xor 16, 32, the waves
//                        through LDS (the W panel's, free between two products) in wave order.  V <= 128: the accumulators of sweep 1
//                        are still in registers and sweep 2 runs no product; V > 128: sweep 2 forms the logits again (same code, same
//                        bits), twice the joint work.  A chunk needs no other chunk: 2 V floats per (slot, chunk) leave the workgroup.
//   k_rnnt_beam_combine  grid S, 256 threads: per live slot the chunk chain in double (A_in, kept for the entry kernel; the last A_out is
//                        complete(y)); prefix(y + k) for all (slot, class) into the candidate array (a double maximum, float exps around
//                        it: these scores only order candidates); the completes are offered to the list in slot order (rows shifted by
//                        the whole workgroup); B + 1 rounds of argmax over the candidates above thr (ties to the lower (slot, class);
//                        round B + 1 only sets the pruned bit); parents, labels, tokens (copied from the parent's row of the other
//                        generation), next_in rows, the list's arrays, the flags.
//   k_rnnt_beam_entry    grid (ceil(T / 64), S B) over the NEW slots: alpha_parent(t) = Bl(t) + logadd(A_in, Cl(t)) from the parent's
//                        records, the one class logit W_k . tanh(enc[t] + pred_parent) + b_k by a wave per frame (lanes over j, a
//                        fixed butterfly), E_new(t) = alpha + a_k - lse_parent(t).  Workgroup (0, 0) adds up the live slots.
// BOUNDS.  enc rows and the per-frame records are indexed under t < T_s <= T (begin rejects anything else); LDS rows behind T_s are
// zero-filled and their weights are log 0; classes >= V are masked at the panel load, in both epilogues and never written; records are
// indexed by (slot, blockIdx.x) with gridDim.x = nchunk; token rows hold 1024 ints and a label is written only at u < max_len <= 1023;
// list rows are indexed under q < N.  No floating-point atomics, no atomics at all.
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_ctc_host.h"
#include "klstm_host.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_dev.h"

namespace klstm {

enum { BF_FINISHED = 1, BF_TRUNCATED = 2, BF_REJECTED = 4, BF_IDLE = 8, BF_PRUNED = 16, BF_STOP = 15 };
constexpr int BEAM_MAXB = 32, BEAM_TOK = 1024, BEAM_EF = 64;      // beam and list limit, ints of a token row, frames of an entry workgroup
constexpr double DLOG0 = -1e30, DNONE = -1e29;                    // log 0 and the line below which a value counts as log 0

static int beam_fb(int J) { return J <= 512 ? 64 : 32; }

struct BeamState {
  int *flags, *Ts, *step, *nlive, *count;      // per stream
  double *lscore;                              // [S][32] the list's scores
  int *llen;                                   // [S][32]
  int *live, *par, *lab;                       // per slot: live; of a new slot: the parent's row and the label
  int *tok;                                    // [2][S B][1024]
  double *E, *Bl, *Cl;                         // [S B][T]
  float *lse, *lsl;                            // [S B][T] lse(t) as the maximum and the log of the sum
  double *Ain, *BlEnd, *ClEnd, *offY;          // [S B][nchunk]
  float *XY;                                   // [S B][nchunk][2][V]
  double *cand;                                // [S B][V]
};

static BeamState beam_carve(void *base, int T, int S, int B, int J, int V, size_t *bytes) {
  CtcCarver c(base);
  BeamState g;
  const size_t SB = (size_t)S * B, nrec = SB * ((T + beam_fb(J) - 1) / beam_fb(J));
  g.flags = c.take<int>(S); g.Ts = c.take<int>(S); g.step = c.take<int>(S); g.nlive = c.take<int>(S); g.count = c.take<int>(S);
  g.lscore = c.take<double>((size_t)S * BEAM_MAXB); g.llen = c.take<int>((size_t)S * BEAM_MAXB);
  g.live = c.take<int>(SB); g.par = c.take<int>(SB); g.lab = c.take<int>(SB);
  g.tok = c.take<int>(2 * SB * BEAM_TOK);
  g.E = c.take<double>(SB * T); g.Bl = c.take<double>(SB * T); g.Cl = c.take<double>(SB * T);
  g.lse = c.take<float>(SB * T); g.lsl = c.take<float>(SB * T);
  g.Ain = c.take<double>(nrec); g.BlEnd = c.take<double>(nrec); g.ClEnd = c.take<double>(nrec); g.offY = c.take<double>(nrec);
  g.XY = c.take<float>(nrec * 2 * V);
  g.cand = c.take<double>(SB * V);
  *bytes = c.bytes();
  return g;
}

struct BeamArgs {
  const float *enc, *pred, *W, *b;
  int enc_stride, pred_stride, T, S, B, N, J, V, blank, max_len, fb, nchunk;
  const float *embed, *embed_bias;
  int width;
  float *next_in;
  int next_in_stride;
  int *parent, *hyp, *hyp_len;
  float *score_out;
  int *count_out, *flags_out, *live;
  BeamState g;
};

__device__ __forceinline__ double dlogadd(double x, double y) {
  if (x < DNONE) return y < DNONE ? DLOG0 : y;
  if (y < DNONE) return x;
  const double m = fmax(x, y);
  return m + log1p(exp(fmin(x, y) - m));
}

// rows s B .. s B + B - 1 of next_in from x[0 .. B) (-1: zeros), by the whole workgroup
__device__ __forceinline__ void beam_rows(const int *x, int s, int B, int V, const float *embed, const float *bias, int width, float *out, int stride) {
  for (int bq = 0; bq < B; bq++) {
    const int xs = x[bq];
    for (int c = threadIdx.x; c < width; c += blockDim.x) {
      float v = 0.f;
      if (xs >= 0 && xs < V) v = embed ? embed[(size_t)c * V + xs] + (bias ? bias[c] : 0.f) : (c == xs ? 1.f : 0.f);
      out[((size_t)s * B + bq) * stride + c] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_rnnt_beam_begin(BeamState g, const int *lens, int T, int B, int V, int bos, const float *embed,
                                                         const float *bias, int width, float *next_in, int stride, int *parent) {
  __shared__ int x[BEAM_MAXB];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int Ts = lens[s];
  const int f = Ts == 0 ? BF_IDLE : (Ts < 0 || Ts > T) ? BF_REJECTED : 0;
  if (tid == 0) { g.flags[s] = f; g.Ts[s] = f ? 0 : Ts; g.step[s] = 0; g.nlive[s] = f ? 0 : 1; g.count[s] = 0; }
  if (tid < B) {
    const size_t sb = (size_t)s * B + tid;
    g.live[sb] = !f && tid == 0; g.par[sb] = -1; g.lab[sb] = -1;
    parent[sb] = -1;
    x[tid] = (!f && tid == 0) ? bos : -1;
  }
  if (!f)
    for (int t = tid; t < Ts; t += 256) g.E[(size_t)s * B * T + t] = t == 0 ? 0.0 : DLOG0;      // the empty prefix enters at frame 0 only
  __syncthreads();
  beam_rows(x, s, B, V, embed, bias, width, next_in, stride);
}

// (max, sum) of a set of exponents merged with another set's
__device__ __forceinline__ void ms_merge(float &m, float &s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = s * expf(m - nm) + os * expf(om - nm);
  m = nm;
}

__global__ __launch_bounds__(256) void k_rnnt_beam_scan(BeamArgs a) {
  extern __shared__ float lds[];
  __shared__ float f_max[64], f_ls[64], f_lpb[64], f_wx[64], f_wy[64];
  const int J = a.J, V = a.V, Jp = J + 2, FB = a.fb, T = a.T;
  float *encL = lds, *predL = encL + FB * Jp, *Wp = predL + Jp;
  const int sb = blockIdx.y, s = sb / a.B, c = blockIdx.x, t0 = c * FB, tid = threadIdx.x;
  if (!a.g.live[sb]) return;
  const int Ts = a.g.Ts[s];
  if (t0 >= Ts) return;
  const int hi = min(FB, Ts - t0);
  rnnt_stage(encL, Jp, a.enc, a.enc_stride, t0, FB, hi, a.S, s, J);
  rnnt_stage(predL, Jp, a.pred, a.pred_stride, 0, 1, 1, 0, sb, J);        // row sb of pred_rows
  const int lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const bool owns = wave * RT < FB;                    // FB = 32: waves 2 and 3 run the product of tiles 0 and 1 again and drop it
  const int fbase = (owns ? wave : wave & 1) * RT;
  const float *encW = encL + fbase * Jp;
  const float *const pl[1] = {predL};
  const bool one = V <= VP;
  f32x4 acc[1][NVT];
  // sweep 1: the statistics of every frame
  float mrun[4], srun[4], ab[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { mrun[j] = RLOG0; srun[j] = 0.f; ab[j] = 0.f; }
  for (int v0 = 0; v0 < V; v0 += VP) {
    const int nvt = (min(VP, V - v0) + 15) / 16;
    joint_logits<1>(encW, Jp, pl, a.W, J, V, v0, nvt, Wp, acc);
    float bias[NVT];
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) {
      const int v = v0 + vt * 16 + i16;
      bias[vt] = (vt < nvt && v < V) ? a.b[v] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float x[NVT], pb = 0.f, lv = RLOG0;
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) {
        const int v = v0 + vt * 16 + i16;
        x[vt] = (vt < nvt && v < V) ? acc[0][vt][j] + bias[vt] : RLOG0;
        pb += v == a.blank ? x[vt] : 0.f;
        lv = fmaxf(lv, x[vt]);
      }
      lv = red16_max(lv);
      const float nm = fmaxf(mrun[j], lv);
      float sum = 0.f;
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) sum += expf(x[vt] - nm);
      sum = red16_sum(sum);
      srun[j] = srun[j] * expf(mrun[j] - nm) + sum;
      mrun[j] = nm;
      ab[j] += red16_sum(pb);
    }
  }
  if (owns) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (i16 == j) {
        const int f = fbase + 4 * kg + j;
        const float ls = logf(srun[j]);                // lse = max + ls is never formed: a - max is exact near the top, where it matters
        f_max[f] = mrun[j]; f_ls[f] = ls; f_lpb[f] = (ab[j] - mrun[j]) - ls;
      }
  }
  __syncthreads();
  // wave 0, lane = frame: the chunk's Bl and Cl in double, its records, the float weights of sweep 2
  if (wave == 0) {
    const bool val = lane < hi;
    const size_t row = (size_t)sb * T + t0 + (val ? lane : 0);
    const double lpb = val ? (double)f_lpb[lane] : 0.0;
    double incl = lpb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    const double before = __shfl_up(incl, 1);
    const double Bl = lane == 0 ? 0.0 : before;
    const double e = val ? a.g.E[row] : DLOG0;
    double Cl = e < DNONE ? DLOG0 : e - Bl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(Cl, o);
      if (lane >= o) Cl = dlogadd(up, Cl);
    }
    const double w = (val && !(Cl < DNONE)) ? Bl + Cl : DLOG0;
    double off = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) off = fmax(off, __shfl_xor(off, o));
    if (off < DNONE) off = 0.0;
    f_wx[lane] = val ? (float)Bl : RLOG0;
    f_wy[lane] = w < DNONE ? RLOG0 : (float)(w - off);
    if (val) { a.g.Bl[row] = Bl; a.g.Cl[row] = Cl; a.g.lse[row] = f_max[lane]; a.g.lsl[row] = f_ls[lane]; }
    const double bl_end = __shfl(incl, hi - 1), cl_end = __shfl(Cl, hi - 1);
    if (lane == 0) {
      const size_t r = (size_t)sb * a.nchunk + c;
      a.g.BlEnd[r] = bl_end; a.g.ClEnd[r] = cl_end; a.g.offY[r] = off;
    }
  }
  __syncthreads();
  // sweep 2: X_k and Y_k of every class
  float maxf[4], lsf[4], wx[4], wy[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { const int f = fbase + 4 * kg + j; maxf[j] = f_max[f]; lsf[j] = f_ls[f]; wx[j] = f_wx[f]; wy[j] = f_wy[f]; }
  const int nw = FB / RT;
  float *xy = a.g.XY + ((size_t)sb * a.nchunk + c) * 2 * V;
  for (int v0 = 0; v0 < V; v0 += VP) {
    const int nvt = (min(VP, V - v0) + 15) / 16;
    if (!one) joint_logits<1>(encW, Jp, pl, a.W, J, V, v0, nvt, Wp, acc);
    __syncthreads();                                   // the last panel is done with: its LDS takes the waves' partials
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) {
      const int v = v0 + vt * 16 + i16;
      if (vt < nvt && v < V) {
        const float bias = a.b[v];
        float mx = RLOG0, my = RLOG0, lp[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          lp[j] = ((acc[0][vt][j] + bias) - maxf[j]) - lsf[j];
          mx = fmaxf(mx, lp[j] + wx[j]); my = fmaxf(my, lp[j] + wy[j]);
        }
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) { sx += expf(lp[j] + wx[j] - mx); sy += expf(lp[j] + wy[j] - my); }
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          ms_merge(mx, sx, __shfl_xor(mx, o), __shfl_xor(sx, o));
          ms_merge(my, sy, __shfl_xor(my, o), __shfl_xor(sy, o));
        }
        if (kg == 0 && owns) {
          float *p = Wp + ((size_t)wave * VP + vt * 16 + i16) * 4;
          p[0] = mx; p[1] = sx; p[2] = my; p[3] = sy;
        }
      }
    }
    __syncthreads();
    if (tid < VP && v0 + tid < V) {
      float mx = Wp[tid * 4], sx = Wp[tid * 4 + 1], my = Wp[tid * 4 + 2], sy = Wp[tid * 4 + 3];
      for (int w = 1; w < nw; w++) {
        const float *p = Wp + ((size_t)w * VP + tid) * 4;
        ms_merge(mx, sx, p[0], p[1]);
        ms_merge(my, sy, p[2], p[3]);
      }
      xy[v0 + tid] = mx + logf(sx); xy[V + v0 + tid] = my + logf(sy);
    }
  }
}

__global__ __launch_bounds__(256) void k_rnnt_beam_combine(BeamArgs a) {
  __shared__ double comp[BEAM_MAXB], w_sc[4];
  __shared__ int lv[BEAM_MAXB], x[BEAM_MAXB], sel[BEAM_MAXB], w_ix[4], best_ix, sh_p, sh_cnt;
  const int s = blockIdx.x, tid = threadIdx.x, B = a.B, N = a.N, V = a.V, lane = tid & 63, wave = tid >> 6;
  const size_t sb0 = (size_t)s * B, SB = (size_t)a.S * B;
  const int u = a.g.step[s];
  int f = a.g.flags[s];
  double *ls = a.g.lscore + (size_t)s * BEAM_MAXB;
  int *ll = a.g.llen + (size_t)s * BEAM_MAXB;
  if (tid < BEAM_MAXB) { x[tid] = -1; lv[tid] = (tid < B && !(f & BF_STOP)) ? a.g.live[sb0 + tid] : 0; }
  __syncthreads();
  int nsel = 0;
  if (!(f & BF_STOP)) {
    const int Ts = a.g.Ts[s], nc = (Ts + a.fb - 1) / a.fb, gen = u & 1;
    // the chunk chain of every live slot
    if (tid < B && lv[tid]) {
      const size_t r0 = (sb0 + tid) * a.nchunk;
      double A = DLOG0;
      for (int c = 0; c < nc; c++) { a.g.Ain[r0 + c] = A; A = a.g.BlEnd[r0 + c] + dlogadd(A, a.g.ClEnd[r0 + c]); }
      comp[tid] = A;
    }
    __syncthreads();
    // prefix(y + k) of every (slot, class)
    for (int idx = tid; idx < B * V; idx += 256) {
      const int bq = idx / V, k = idx - bq * V;
      double sc = DLOG0;
      if (lv[bq] && k != a.blank) {
        const size_t r0 = (sb0 + bq) * a.nchunk;
        double m = DLOG0;
        for (int c = 0; c < nc; c++) {
          const float *xy = a.g.XY + (r0 + c) * 2 * V;
          const double ain = a.g.Ain[r0 + c];
          if (!(ain < DNONE)) m = fmax(m, ain + (double)xy[k]);
          m = fmax(m, a.g.offY[r0 + c] + (double)xy[V + k]);
        }
        if (!(m < DNONE)) {
          float sum = 0.f;
          for (int c = 0; c < nc; c++) {
            const float *xy = a.g.XY + (r0 + c) * 2 * V;
            const double ain = a.g.Ain[r0 + c];
            if (!(ain < DNONE)) sum += expf((float)(ain + (double)xy[k] - m));
            sum += expf((float)(a.g.offY[r0 + c] + (double)xy[V + k] - m));
          }
          sc = m + (double)logf(sum);
        }
      }
      a.g.cand[sb0 * V + idx] = sc;
    }
    __syncthreads();                                     // the selection below reads what other threads wrote
    // the completes go to the list, in slot order
    for (int bq = 0; bq < B; bq++) {
      if (!lv[bq]) continue;
      if (tid == 0) {
        const int cnt = a.g.count[s];
        int p = cnt;
        while (p > 0 && ls[p - 1] < comp[bq]) p--;      // a tie keeps the earlier entry
        sh_p = p < N ? p : -1; sh_cnt = cnt;
      }
      __syncthreads();
      const int p = sh_p, cnt = sh_cnt;
      if (p >= 0) {
        for (int q = min(cnt, N - 1); q > p; q--) {
          const int len = ll[q - 1];
          for (int t = tid; t < len; t += 256) a.hyp[((size_t)s * N + q) * a.max_len + t] = a.hyp[((size_t)s * N + q - 1) * a.max_len + t];
          __syncthreads();
          if (tid == 0) { ll[q] = len; ls[q] = ls[q - 1]; }
        }
        const int *src = a.g.tok + ((size_t)gen * SB + sb0 + bq) * BEAM_TOK;
        for (int t = tid; t < u && t < a.max_len; t += 256) a.hyp[((size_t)s * N + p) * a.max_len + t] = src[t];
        if (tid == 0) { ll[p] = min(u, a.max_len); ls[p] = comp[bq]; a.g.count[s] = min(cnt + 1, N); }
      }
      __syncthreads();
    }
    const int cnt = a.g.count[s];
    const double thr = cnt == N ? ls[N - 1] : DLOG0;
    // the B best candidates above thr; one more round tells whether the beam cut one
    const double *cand = a.g.cand + sb0 * V;
    bool pruned = false;
    for (int r = 0; r <= B; r++) {
      double bs = DLOG0;
      int bi = INT32_MAX;
      for (int idx = tid; idx < B * V; idx += 256) {
        const double v = cand[idx];
        if (v > bs) { bs = v; bi = idx; }
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double ov = __shfl_xor(bs, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bs || (ov == bs && oi < bi)) { bs = ov; bi = oi; }
      }
      if (lane == 0) { w_sc[wave] = bs; w_ix[wave] = bi; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < 4; w++)
          if (w_sc[w] > bs || (w_sc[w] == bs && w_ix[w] < bi)) { bs = w_sc[w]; bi = w_ix[w]; }
        const bool in = bi != INT32_MAX && bs > thr && !(bs < DNONE);
        best_ix = in ? bi : -1;
        if (in && r < B) { sel[r] = bi; a.g.cand[sb0 * V + bi] = DLOG0; }
      }
      __syncthreads();
      if (best_ix < 0) break;
      if (r < B) nsel = r + 1; else pruned = true;
      __syncthreads();
    }
    if (pruned) f |= BF_PRUNED;
    if (nsel == 0) f |= BF_FINISHED;
    else if (u + 1 > a.max_len) { f |= BF_TRUNCATED; nsel = 0; }
    // the new slots: parent, label, tokens
    const int ngen = gen ^ 1;
    for (int j = 0; j < nsel; j++) {
      const int bq = sel[j] / V, k = sel[j] - bq * V;
      const int *src = a.g.tok + ((size_t)gen * SB + sb0 + bq) * BEAM_TOK;
      int *dst = a.g.tok + ((size_t)ngen * SB + sb0 + j) * BEAM_TOK;
      for (int t = tid; t < u; t += 256) dst[t] = src[t];
      if (tid == 0) { dst[u] = k; x[j] = k; a.g.par[sb0 + j] = (int)sb0 + bq; a.g.lab[sb0 + j] = k; }
    }
    __syncthreads();
    if (tid == 0) { a.g.flags[s] = f; a.g.step[s] = u + 1; a.g.nlive[s] = nsel; }
  }
  if (tid < B) {
    a.g.live[sb0 + tid] = tid < nsel;
    a.parent[sb0 + tid] = tid < nsel ? a.g.par[sb0 + tid] : -1;
  }
  if (tid < N) {
    const int cnt = a.g.count[s];
    a.hyp_len[(size_t)s * N + tid] = tid < cnt ? ll[tid] : 0;
    a.score_out[(size_t)s * N + tid] = tid < cnt ? (float)ls[tid] : 0.f;
  }
  if (tid == 0) { a.count_out[s] = a.g.count[s]; a.flags_out[s] = f; if (f & BF_STOP) a.g.nlive[s] = 0; }
  __syncthreads();
  beam_rows(x, s, B, V, a.embed, a.embed_bias, a.width, a.next_in, a.next_in_stride);
}

__global__ __launch_bounds__(256) void k_rnnt_beam_entry(BeamArgs a) {
  const int sb = blockIdx.y, s = sb / a.B, t0 = blockIdx.x * BEAM_EF, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int J = a.J, T = a.T;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    int n = 0;
    for (int q = 0; q < a.S; q++) n += a.g.nlive[q];
    *a.live = n;
  }
  if (!a.g.live[sb]) return;
  const int Ts = a.g.Ts[s];
  if (t0 >= Ts) return;
  const int par = a.g.par[sb], k = a.g.lab[sb];
  float w[16], p[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int j = lane + 64 * i;
    w[i] = j < J ? a.W[(size_t)k * J + j] : 0.f;
    p[i] = j < J ? a.pred[(size_t)par * a.pred_stride + j] : 0.f;
  }
  const float bk = a.b[k];
  for (int fr = wave; fr < BEAM_EF; fr += 4) {
    const int t = t0 + fr;
    if (t >= Ts) break;
    const float *er = a.enc + ((size_t)t * a.S + s) * a.enc_stride;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int j = lane + 64 * i;
      if (j < J) d += w[i] * k_tanh(er[j] + p[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (lane == 0) {
      const size_t prow = (size_t)par * T + t;
      const double alpha = dlogadd(a.g.Ain[(size_t)par * a.nchunk + t / a.fb], a.g.Cl[prow]);
      a.g.E[(size_t)sb * T + t] = alpha < DNONE ? DLOG0 : a.g.Bl[prow] + alpha + (double)(((d + bk) - a.g.lse[prow]) - a.g.lsl[prow]);
    }
  }
}

static bool bal4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

static const char *beam_limits(int T, int S, int B, int J, int V) {
  if (S < 1 || S > 32) return "1 <= S <= 32";
  if (B < 1 || B > BEAM_MAXB) return "1 <= B <= 32";
  if (T < 1 || (long long)T * S > (1ll << 24)) return "1 <= T, T S <= 2^24";
  if (J < 16 || J > 1024 || J % 16 != 0) return "16 <= J <= 1024, J % 16 == 0";
  if (V < 2 || V > 4096) return "2 <= V <= 4096";
  return nullptr;
}

// what begin and step share: the input rows' and the parents' arguments and the state
static klstm_status beam_common(const char *who, int T, int S, int B, int J, int V, const float *embed, const float *embed_bias, int D,
                                const float *next_in, int next_in_stride, const int *parent, const void *state, size_t state_bytes) {
  if (const char *why = beam_limits(T, S, B, J, V)) return fail(KLSTM_ERR_SHAPE, "%s: T %d, S %d, B %d, J %d, V %d: the limit is %s", who, T, S, B, J, V, why);
  if (embed && D < 1) return fail(KLSTM_ERR_SHAPE, "%s: an embedding of %d rows", who, D);
  if (!next_in || !parent || !state) return fail(KLSTM_ERR_ARG, "%s: null argument", who);
  if (next_in_stride < (embed ? D : V)) return fail(KLSTM_ERR_ARG, "%s: row stride %d below the width %d", who, next_in_stride, embed ? D : V);
  if (!bal4(next_in) || !bal4(parent) || !bal4(embed) || !bal4(embed_bias)) return fail(KLSTM_ERR_ARG, "%s: misaligned pointer", who);
  size_t need = 0;
  beam_carve(nullptr, T, S, B, J, V, &need);
  if (state_bytes < need) return fail(KLSTM_ERR_ARG, "%s: state of %zu bytes, %zu needed", who, state_bytes, need);
  if (reinterpret_cast<uintptr_t>(state) & 255) return fail(KLSTM_ERR_ARG, "%s: the state is not 256-byte aligned", who);
  return KLSTM_OK;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_beam_state_bytes(int T, int S, int B, int J, int V) {
  if (const char *why = beam_limits(T, S, B, J, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_beam_state_bytes: T %d, S %d, B %d, J %d, V %d: the limit is %s", T, S, B, J, V, why);
    return 0;
  }
  size_t bytes = 0;
  beam_carve(nullptr, T, S, B, J, V, &bytes);
  return bytes;
}

klstm_status krnnt_beam_begin(int T, int S, int B, int J, int V, int bos, const int *lens_dev, const float *embed, const float *embed_bias, int D,
                              float *next_in, int next_in_stride, int *parent_dev, void *state, size_t state_bytes, void *hip_stream) {
  if (const klstm_status st = beam_common("krnnt_beam_begin", T, S, B, J, V, embed, embed_bias, D, next_in, next_in_stride, parent_dev, state, state_bytes)) return st;
  if (bos < 0 || bos >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_beam_begin: bos %d outside [0, %d)", bos, V);
  if (!lens_dev) return fail(KLSTM_ERR_ARG, "krnnt_beam_begin: null argument");
  size_t need = 0;
  const BeamState g = beam_carve(state, T, S, B, J, V, &need);
  HIPCHK(launch(k_rnnt_beam_begin, dim3(S), dim3(256), 0, (hipStream_t)hip_stream, LaunchProbe(), g, lens_dev, T, B, V, bos, embed, embed_bias,
                embed ? D : V, next_in, next_in_stride, parent_dev));
  return KLSTM_OK;
}

klstm_status krnnt_beam_step(const float *enc, int enc_stride, const float *pred_rows, int pred_stride, const float *W, const float *b, int T,
                             int S, int B, int N, int J, int V, int blank, int max_len, const float *embed, const float *embed_bias, int D,
                             float *next_in, int next_in_stride, int *parent_dev, int *nbest_hyp, int *nbest_len, float *nbest_score,
                             int *nbest_count, int *flags_dev, int *live_dev, void *state, size_t state_bytes, void *hip_stream) {
  if (const klstm_status st = beam_common("krnnt_beam_step", T, S, B, J, V, embed, embed_bias, D, next_in, next_in_stride, parent_dev, state, state_bytes)) return st;
  if (N < 1 || N > B) return fail(KLSTM_ERR_SHAPE, "krnnt_beam_step: a list of %d with a beam of %d: the limit is 1 <= N <= B", N, B);
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_beam_step: blank %d outside [0, %d)", blank, V);
  if (max_len < 1 || max_len > 1023) return fail(KLSTM_ERR_SHAPE, "krnnt_beam_step: max_len %d: the limit is 1 <= max_len <= 1023", max_len);
  if (!enc || !pred_rows || !W || !b || !nbest_hyp || !nbest_len || !nbest_score || !nbest_count || !flags_dev || !live_dev)
    return fail(KLSTM_ERR_ARG, "krnnt_beam_step: null argument");
  if (enc_stride < J || pred_stride < J) return fail(KLSTM_ERR_ARG, "krnnt_beam_step: row stride below the width %d (%d, %d)", J, enc_stride, pred_stride);
  if (!bal4(enc) || !bal4(pred_rows) || !bal4(W) || !bal4(b) || !bal4(nbest_hyp) || !bal4(nbest_len) || !bal4(nbest_score) || !bal4(nbest_count) ||
      !bal4(flags_dev) || !bal4(live_dev))
    return fail(KLSTM_ERR_ARG, "krnnt_beam_step: misaligned pointer");
  BeamArgs a;
  size_t need = 0;
  a.g = beam_carve(state, T, S, B, J, V, &need);
  a.enc = enc; a.pred = pred_rows; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.B = B; a.N = N; a.J = J; a.V = V; a.blank = blank; a.max_len = max_len;
  a.fb = beam_fb(J); a.nchunk = (T + a.fb - 1) / a.fb;
  a.embed = embed; a.embed_bias = embed_bias; a.width = embed ? D : V; a.next_in = next_in; a.next_in_stride = next_in_stride;
  a.parent = parent_dev; a.hyp = nbest_hyp; a.hyp_len = nbest_len; a.score_out = nbest_score; a.count_out = nbest_count;
  a.flags_out = flags_dev; a.live = live_dev;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t shm = ((size_t)(a.fb + 1) * (J + 2) + VP * WPS) * sizeof(float);
  HIPCHK(launch(k_rnnt_beam_scan, dim3(a.nchunk, S * B), dim3(256), shm, st, LaunchProbe(), a));
  HIPCHK(launch(k_rnnt_beam_combine, dim3(S), dim3(256), 0, st, LaunchProbe(), a));
  HIPCHK(launch(k_rnnt_beam_entry, dim3((T + BEAM_EF - 1) / BEAM_EF, S * B), dim3(256), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

}  // extern "C"
