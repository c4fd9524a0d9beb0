// kaldi-lstm_amd/csrc/klstm_rnnt.hip -- RNN-transducer training: the krnnt_* entries of include/klstm_rnnt.h (which defines every
// quantity; the torch yardstick: tests/rnnt_ref.py) and their kernels.  Neither h = tanh(enc[t] + pred[u]) nor the
// logits W h + b of a lattice node ever go to memory: both exist only in registers, in the forward pass and again in the backward pass.
//   k_rnnt_prep       one thread per stream: status (1 runs, 0 idle, -1 rejected), T_s, U_s and the label offset, for every kernel behind it.
//   k_rnnt_joint_fwd  a workgroup (4 waves) owns KRNNT_TILE_T x KRNNT_TILE_U = 16 x 8 nodes of one stream: the 16 enc rows and the 8 pred
//                     rows go to LDS once; a wave owns two M-tiles (16 t at one u each).  joint_logits() (klstm_rnnt_dev.h, shared
//                     with the decoder, klstm_rnnt_decode.hip): h is formed in registers as the A
//                     operand of MFMA16 (lane (i, kg) computes tanh for row i, column k0 + kg: exactly the element it feeds), taken once
//                     per k-step and used against all of the pass's class tiles (up to KRNNT_PASS_V = 128 classes, 8 accumulator tiles per
//                     M-tile); W streams through LDS in panels of 32 k shared by the four waves, stored [class][k] with a row stride of 34
//                     floats: a B read (class = lane & 15, k = lane >> 4) hits bank 2 class + kg, 32 distinct banks per half wave, and
//                     the panel's stores (consecutive k) are conflict-free too.  Every panel is a chain of its own that is added to the
//                     node's sums (short chains round less, as in klstm_cnn.hip).  V > 128 runs in passes with a running max and sum.
//                     The epilogue reduces a node's row over the 16 lanes that hold it with a fixed butterfly and writes three floats.
//   k_rnnt_lattice    grid (S, 2): alpha and beta of a stream side by side, one thread per u, along the anti-diagonals d = t + u, the
//                     previous diagonal double-buffered in LDS, one barrier per diagonal (a wave-level fence when the workgroup is one
//                     wave), the lpb / lpy of the next four diagonals loaded into registers ahead.  Diagonal d is stored minus the maximum
//                     of the stored diagonal before it; thread 0 sums those maxima in double (the offsets) and takes the loss in double.
//                     The recursion itself (the LDS rows, the logadd) runs in double and rounds once, at the store to the float planes:
//                     in float the rounding of every diagonal (an ulp of 1e-6 at |log| = 10) adds up in w_b, w_y and from there in b_grad.
//   k_rnnt_weights    one thread per node: w_b, w_y from alpha, beta, the offsets and the loss, the sum taken in double before the exp;
//                     thread 0 adds to the totals in stream order.
//   k_rnnt_joint_bwd<NJ>  krnnt_grad_splits() persistent workgroups; workgroup c takes the units (stream, block of 16 t) c, c + splits, ..
//                     in order and walks a unit's u four at a time, one M-tile per wave.  Per pass of 128 classes: the logits again
//                     (joint_logits, the same bits as forward), g in registers from lse, w_b, w_y, then through a 64 x 128 LDS tile (the
//                     transposition between the C and the A layout) into two more products: dz += g W (K = classes, W rows from L2, the
//                     J / 16 accumulator tiles of the wave's 16 nodes live in registers: NJ of them) and W_grad partial += g^T h (K = the
//                     workgroup's 64 nodes; wave w owns the column tiles w, w + 4, ..; h is taken again as the B operand), added to the
//                     workgroup's OWN partial in memory (b_grad's partial is kept in double: its terms cancel) by the lane that always owns that element.  dz (1 - h^2) is added to the wave's
//                     own slot of the d_enc partials (4 slots: the waves differ in u) and its sum over the 16 t goes to the d_pred
//                     partial of the t block.
//   k_rnnt_finish     the fixed-order second stage: d_enc = the four slots in order, d_pred = the t blocks in order, W_grad / b_grad =
//                     the splits in order (in double, rounded once); zero rows where the definition says so; rejected streams untouched.
//   k_rnnt_pack       the prediction network's input rows.
// KNOWN SLOW SPOTS (first version): the lattice reads lpb / lpy with a stride of Umax along a diagonal; the backward products read W
// and the partials through L2 instead of LDS panels; with V J > 2^16 fewer than 256 workgroups run the backward pass.
// BOUNDS.  Nodes are touched only under t < T_s and u <= U_s (the workgroups of other tiles leave at once); LDS rows beyond them are
// zero-filled, classes >= V are masked at the panel load and in the epilogues; node and row offsets are size_t products.
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_ctc_host.h"
#include "klstm_host.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_dev.h"

namespace klstm {

constexpr int RU = KRNNT_TILE_U;            // (RT, VP, NVT, KP, WPS and RLOG0: klstm_rnnt_dev.h)
constexpr int BU = 4, GS = VP + 2;          // u per backward step (one per wave), floats per row of the g tile
constexpr int ESLOTS = 4;                   // d_enc partial slots = waves of the backward workgroup

// (RnntWs and RnntArgs: klstm_rnnt_dev.h, shared with klstm_rnnt_simple.hip)

static int rnnt_splits(int J, int V) {
  const long long s = (1ll << 24) / ((long long)V * J);
  return s < 8 ? 8 : s > 256 ? 256 : (int)s;
}

// the layout of the workspace (include/klstm_rnnt.h states the formula); base null: only bytes() counts
RnntWs rnnt_carve(void *base, int T, int S, int U1, int J, int V, bool grads, size_t *bytes) {
  CtcCarver c(base);
  RnntWs w;
  const size_t N = (size_t)S * T * U1, ntb = (size_t)(T + RT - 1) / RT;
  w.meta = c.take<int4>(S);
  w.loss = c.take<double>(S);
  w.offs = c.take<double>((size_t)2 * S * (T + U1));
  w.lpb = c.take<float>(N); w.lpy = c.take<float>(N); w.lse = c.take<float>(N);
  w.A = c.take<float>(N); w.B = c.take<float>(N); w.wb = c.take<float>(N); w.wy = c.take<float>(N);
  w.dep = w.dpp = w.wpart = nullptr; w.bpart = nullptr;
  if (grads) {                                         // the partials' term: a forward-only call needs none of it
    w.dep = c.take<float>((size_t)ESLOTS * S * T * J);
    w.dpp = c.take<float>(ntb * S * U1 * J);
    w.wpart = c.take<float>((size_t)rnnt_splits(J, V) * V * J);
    w.bpart = c.take<double>((size_t)rnnt_splits(J, V) * V);
  }
  *bytes = c.bytes();
  return w;
}

__global__ __launch_bounds__(64) void k_rnnt_prep(RnntArgs a) {
  const int s = threadIdx.x;
  if (s >= a.S) return;
  const int Ts = a.lens[s], o0 = a.loff[s], o1 = a.loff[s + 1], U = o1 - o0;
  int st = 1;
  if (Ts == 0) st = 0;
  else if (Ts < 0 || Ts > a.T || U < 0 || U > a.U1 - 1 || o0 < 0) st = -1;
  else
    for (int i = o0; i < o1; i++) {
      const int y = a.labels[i];
      if (y < 0 || y >= a.V || y == a.blank) { st = -1; break; }
    }
  a.ws.meta[s] = make_int4(st, st == 1 ? Ts : 0, st == 1 ? U : 0, o0);
}

__global__ __launch_bounds__(256) void k_rnnt_joint_fwd(RnntArgs a) {
  extern __shared__ float lds[];
  const int J = a.J, V = a.V, Jp = J + 2;
  float *encL = lds, *predL = encL + RT * Jp, *Wp = predL + RU * Jp;
  const int s = blockIdx.z, t0 = blockIdx.x * RT, u0 = blockIdx.y * RU;
  const int4 me = a.ws.meta[s];
  if (me.x != 1 || t0 >= me.y || u0 > me.z) return;
  const int Ts = me.y, U = me.z;
  rnnt_stage(encL, Jp, a.enc, a.enc_stride, t0, RT, min(RT, Ts - t0), a.S, s, J);
  rnnt_stage(predL, Jp, a.pred, a.pred_stride, u0, RU, min(RU, U + 1 - u0), a.S, s, J);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15, kg = lane >> 4;
  const float *const pl[2] = {predL + (2 * wave) * Jp, predL + (2 * wave + 1) * Jp};
  int lab[2];
#pragma unroll
  for (int m = 0; m < 2; m++) {
    const int u = u0 + 2 * wave + m;
    lab[m] = u < U ? a.labels[me.w + u] : -1;
  }
  float mrun[2][4], srun[2][4], ab[2][4], ay[2][4];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int j = 0; j < 4; j++) { mrun[m][j] = RLOG0; srun[m][j] = 0.f; ab[m][j] = 0.f; ay[m][j] = 0.f; }
  for (int v0 = 0; v0 < V; v0 += VP) {
    const int nvt = (min(VP, V - v0) + 15) / 16;
    f32x4 acc[2][NVT];
    joint_logits<2>(encL, Jp, pl, a.W, J, V, v0, nvt, Wp, acc);
    float bias[NVT];
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) {
      const int v = v0 + vt * 16 + i16;
      bias[vt] = (vt < nvt && v < V) ? a.b[v] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float x[NVT], mx = RLOG0, pb = 0.f, py = 0.f;
#pragma unroll
        for (int vt = 0; vt < NVT; vt++) {
          const int v = v0 + vt * 16 + i16;
          x[vt] = (vt < nvt && v < V) ? acc[m][vt][j] + bias[vt] : RLOG0;
          mx = fmaxf(mx, x[vt]);
          pb += v == a.blank ? x[vt] : 0.f;
          py += v == lab[m] ? x[vt] : 0.f;
        }
        mx = red16_max(mx);
        const float nm = fmaxf(mrun[m][j], mx);
        float sum = 0.f;
#pragma unroll
        for (int vt = 0; vt < NVT; vt++) sum += expf(x[vt] - nm);
        sum = red16_sum(sum);
        srun[m][j] = srun[m][j] * expf(mrun[m][j] - nm) + sum;
        mrun[m][j] = nm;
        ab[m][j] += red16_sum(pb);
        ay[m][j] += red16_sum(py);
      }
  }
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int t = t0 + 4 * kg + j, u = u0 + 2 * wave + m;
      if (i16 == j && t < Ts && u <= U) {
        const size_t n = ((size_t)s * a.T + t) * a.U1 + u;
        const float lse = mrun[m][j] + logf(srun[m][j]);
        a.ws.lpb[n] = ab[m][j] - lse;
        a.ws.lpy[n] = u < U ? ay[m][j] - lse : RLOG0;
        a.ws.lse[n] = lse;
      }
    }
}

__device__ __forceinline__ double rnnt_logadd(double x, double y) {
  const double m = fmax(x, y), d = fmin(x, y) - m;
  if (m <= -1e29) return (double)RLOG0;
  return m + log1p(exp(d));
}

// DIR 0: alpha, forward over the diagonals; DIR 1: beta, backward.  Stored value of diagonal d = true value - offs[d].
template <int DIR>
__device__ __forceinline__ void rnnt_lattice_run(const RnntArgs &a, int s, int Ts, int U, double (*row)[1024 + 2], float (*wmax)[16]) {
  const int u = threadIdx.x, lane = u & 63, wave = u >> 6, nw = blockDim.x >> 6, nd = Ts + U, U1 = a.U1;
  const size_t base = (size_t)s * a.T * U1;
  const float *lpb = a.ws.lpb + base, *lpy = a.ws.lpy + base;
  float *out = (DIR == 0 ? a.ws.A : a.ws.B) + base;
  double *offs = a.ws.offs + (size_t)(2 * s + DIR) * (a.T + U1);
  const bool one = nw == 1;
  for (int e = u; e < 2 * (1024 + 2); e += blockDim.x) (&row[0][0])[e] = (double)RLOG0;
  if (u < 32) (&wmax[0][0])[u] = RLOG0;
  if (one) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
  // what step e (diagonal d = e or nd - 1 - e) needs of thread u: alpha: lpb(t-1, u), lpy(t, u-1); beta: lpb(t, u), lpy(t, u)
  auto fetch = [&](int e, float &fb, float &fy) {
    fb = 0.f; fy = 0.f;
    if (e >= nd || u > U) return;
    const int d = DIR == 0 ? e : nd - 1 - e, t = d - u;
    if (t < 0 || t >= Ts) return;
    if (DIR == 0) {
      if (t > 0) fb = lpb[(size_t)(t - 1) * U1 + u];
      if (u > 0) fy = lpy[(size_t)t * U1 + u - 1];
    } else {
      fb = lpb[(size_t)t * U1 + u];
      if (u < U) fy = lpy[(size_t)t * U1 + u];
    }
  };
  float cb[4], cy[4], nb[4], ny[4];
#pragma unroll
  for (int i = 0; i < 4; i++) fetch(i, cb[i], cy[i]);
  double offacc = 0.0;
  for (int e0 = 0; e0 < nd; e0 += 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) fetch(e0 + 4 + i, nb[i], ny[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int e = e0 + i;
      if (e < nd) {
        const int d = DIR == 0 ? e : nd - 1 - e, t = d - u, cur = e & 1, prv = cur ^ 1;
        float mprev = 0.f;
        if (e > 0) {
          mprev = wmax[prv][0];
          for (int w = 1; w < nw; w++) mprev = fmaxf(mprev, wmax[prv][w]);
        }
        double val = (double)RLOG0;
        if (u <= U && t >= 0 && t < Ts) {
          if (DIR == 0) {
            if (e == 0) val = 0.0;
            else {
              const double x1 = t > 0 ? row[prv][u + 1] + cb[i] : (double)RLOG0, x2 = u > 0 ? row[prv][u] + cy[i] : (double)RLOG0;
              val = rnnt_logadd(x1, x2) - mprev;
            }
          } else {
            if (e == 0) val = cb[i];
            else {
              const double x1 = t + 1 < Ts ? row[prv][u + 1] + cb[i] : (double)RLOG0, x2 = u < U ? row[prv][u + 2] + cy[i] : (double)RLOG0;
              val = rnnt_logadd(x1, x2) - mprev;
            }
          }
          if (val < -1e29) val = (double)RLOG0;
          out[(size_t)t * U1 + u] = (float)val;
        }
        row[cur][u + 1] = val;
        float wm = (float)val;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
        if (lane == 0) wmax[cur][wave] = wm;
        if (u == 0) {
          offacc += (double)mprev;
          offs[d] = offacc;
          if (DIR == 1 && e == nd - 1) {
            const double loss = -(val + offacc);
            a.ws.loss[s] = loss;
            a.utt_loss[s] = (float)loss;
          }
        }
        if (one) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { cb[i] = nb[i]; cy[i] = ny[i]; }
  }
}

__global__ __launch_bounds__(1024) void k_rnnt_lattice(RnntArgs a) {
  __shared__ double row[2][1024 + 2];
  __shared__ float wmax[2][16];
  const int s = blockIdx.x;
  const int4 me = a.ws.meta[s];
  if (me.x != 1) {
    if (blockIdx.y == 1 && threadIdx.x == 0) { a.ws.loss[s] = 0.0; a.utt_loss[s] = 0.f; }
    return;
  }
  if (blockIdx.y == 0) rnnt_lattice_run<0>(a, s, me.y, me.z, row, wmax);
  else rnnt_lattice_run<1>(a, s, me.y, me.z, row, wmax);
}

__global__ __launch_bounds__(256) void k_rnnt_weights(RnntArgs a) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x, N = (size_t)a.S * a.T * a.U1;
  if (n == 0 && a.totals) {
    for (int s = 0; s < a.S; s++) {
      const int4 me = a.ws.meta[s];
      if (me.x == 1) { a.totals[0] += a.ws.loss[s]; a.totals[1] += me.y; a.totals[2] += me.z; a.totals[3] += 1.0; }
      if (me.x == -1) { a.totals[3] += 1.0; a.totals[4] += 1.0; }
    }
  }
  if (n >= N) return;
  const int u = (int)(n % a.U1), t = (int)((n / a.U1) % a.T), s = (int)(n / ((size_t)a.U1 * a.T));
  const int4 me = a.ws.meta[s];
  float wb = 0.f, wy = 0.f;
  if (me.x == 1 && t < me.y && u <= me.z) {
    const int Ts = me.y, U = me.z, d = t + u, L = a.T + a.U1;
    const double *oA = a.ws.offs + (size_t)(2 * s) * L, *oB = oA + L;
    const double loss = a.ws.loss[s], al = (double)a.ws.A[n] + oA[d];
    if (t == Ts - 1) {
      if (u == U) wb = (float)exp(al + (double)a.ws.lpb[n] + loss);
    } else {
      wb = (float)exp(al + (double)a.ws.lpb[n] + ((double)a.ws.B[n + a.U1] + oB[d + 1]) + loss);
    }
    if (u < U) wy = (float)exp(al + (double)a.ws.lpy[n] + ((double)a.ws.B[n + 1] + oB[d + 1]) + loss);
  }
  a.ws.wb[n] = wb;
  a.ws.wy[n] = wy;
}

template <int NJ>
__global__ __launch_bounds__(256) void k_rnnt_joint_bwd(RnntArgs a) {
  extern __shared__ float lds[];
  const int J = a.J, V = a.V, Jp = J + 2, U1 = a.U1, S = a.S;
  float *encL = lds, *predL = encL + RT * Jp, *Wp = predL + BU * Jp, *G = Wp + VP * WPS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const size_t wsz = (size_t)V * J;
  float *wpart = a.ws.wpart + (size_t)blockIdx.x * wsz;
  double *bpart = a.ws.bpart + (size_t)blockIdx.x * V;
  float *dep = a.ws.dep + (size_t)wave * S * a.T * J;
  for (size_t e = tid; e < wsz; e += 256) wpart[e] = 0.f;
  for (int e = tid; e < V; e += 256) bpart[e] = 0.0;
  for (int unit = blockIdx.x; unit < S * a.ntb; unit += gridDim.x) {
    const int s = unit / a.ntb, tb = unit - s * a.ntb, t0 = tb * RT;
    const int4 me = a.ws.meta[s];
    if (me.x != 1 || t0 >= me.y) continue;
    const int Ts = me.y, U = me.z;
    __syncthreads();                                   // the unit before is done with encL (and the zeros above are visible)
    rnnt_stage(encL, Jp, a.enc, a.enc_stride, t0, RT, min(RT, Ts - t0), S, s, J);
    for (int ub = 0; ub <= U; ub += BU) {
      __syncthreads();                                 // the step before is done with predL
      rnnt_stage(predL, Jp, a.pred, a.pred_stride, ub, BU, min(BU, U + 1 - ub), S, s, J);
      const int u = ub + wave;
      const int lab = u < U ? a.labels[me.w + u] : -1;
      bool rv[4];
      float lse[4], wb[4], wy[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int t = t0 + 4 * kg + j;
        rv[j] = u <= U && t < Ts;
        const size_t n = ((size_t)s * a.T + (rv[j] ? t : 0)) * U1 + (rv[j] ? u : 0);
        lse[j] = rv[j] ? a.ws.lse[n] : 0.f;
        wb[j] = rv[j] ? a.ws.wb[n] : 0.f;
        wy[j] = rv[j] ? a.ws.wy[n] : 0.f;
      }
      f32x4 dz[NJ];
#pragma unroll
      for (int nt = 0; nt < NJ; nt++) dz[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float *const pl[1] = {predL + wave * Jp};
      for (int v0 = 0; v0 < V; v0 += VP) {
        const int nvt = (min(VP, V - v0) + 15) / 16, nv = nvt * 16;
        f32x4 acc[1][NVT];
        joint_logits<1>(encL, Jp, pl, a.W, J, V, v0, nvt, Wp, acc);
        // g in registers, then into the tile: row = node (16 wave + t), column = class of the pass
#pragma unroll
        for (int vt = 0; vt < NVT; vt++)
          if (vt < nvt) {
            const int v = v0 + vt * 16 + i16;
            const float bias = v < V ? a.b[v] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              float g = 0.f;
              if (rv[j] && v < V) {
                g = (wb[j] + wy[j]) * expf(acc[0][vt][j] + bias - lse[j]);
                if (v == a.blank) g -= wb[j];
                if (v == lab) g -= wy[j];
              }
              G[(wave * 16 + 4 * kg + j) * GS + vt * 16 + i16] = g;
            }
          }
        __syncthreads();
        // dz += g W: K = the pass's classes
        for (int vs = 0; vs < nv; vs += 4) {
          const float av = G[(wave * 16 + i16) * GS + vs + kg];
          const int vr = v0 + vs + kg;
          const float *wr = a.W + (size_t)(vr < V ? vr : 0) * J;
#pragma unroll
          for (int nt = 0; nt < NJ; nt++)
            if (nt * 16 < J) {
              const float bv = vr < V ? wr[nt * 16 + i16] : 0.f;
              dz[nt] = MFMA16(av, bv, dz[nt]);
            }
        }
        // W_grad partial += g^T h: K = the workgroup's 64 nodes
        for (int nt = wave; nt * 16 < J; nt += 4) {
          const int col = nt * 16 + i16;
          f32x4 dw[NVT];
#pragma unroll
          for (int vt = 0; vt < NVT; vt++) dw[vt] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int q = 0; q < 16; q++) {
            const int node = 4 * q + kg;
            const float hb = k_tanh(encL[(node & 15) * Jp + col] + predL[(node >> 4) * Jp + col]);
#pragma unroll
            for (int vt = 0; vt < NVT; vt++)
              if (vt < nvt) dw[vt] = MFMA16(G[node * GS + vt * 16 + i16], hb, dw[vt]);
          }
#pragma unroll
          for (int vt = 0; vt < NVT; vt++)
            if (vt < nvt) {
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int v = v0 + vt * 16 + 4 * kg + j;
                if (v < V) wpart[(size_t)v * J + col] += dw[vt][j];
              }
            }
        }
        if (tid < nv && v0 + tid < V) {
          double sum = 0.0;
          for (int node = 0; node < 64; node++) sum += (double)G[node * GS + tid];
          bpart[v0 + tid] += sum;
        }
      }
      // dz (1 - h^2): into the wave's slot of the d_enc partials, and its sum over the 16 t into the t block's d_pred partial
#pragma unroll
      for (int nt = 0; nt < NJ; nt++)
        if (nt * 16 < J) {
          const int col = nt * 16 + i16;
          float colsum = 0.f;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int r = 4 * kg + j, t = t0 + r;
            const float h = k_tanh(encL[r * Jp + col] + predL[wave * Jp + col]);
            const float v = dz[nt][j] * (1.f - h * h);
            colsum += v;
            if (t < Ts) {
              float *p = dep + ((size_t)t * S + s) * J + col;
              *p = ub == 0 ? v : *p + v;
            }
          }
          colsum += __shfl_xor(colsum, 16);
          colsum += __shfl_xor(colsum, 32);
          if (kg == 0 && u <= U) a.ws.dpp[((size_t)tb * S * U1 + (size_t)u * S + s) * J + col] = colsum;
        }
    }
  }
}

__global__ __launch_bounds__(256) void k_rnnt_finish(RnntArgs a) {
  const size_t J = a.J, ne = (size_t)a.S * a.T * J, np = (size_t)a.S * a.U1 * J, nw = (size_t)a.V * J + a.V;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < ne + np + nw; e += (size_t)gridDim.x * 256) {
    if (e < ne) {
      const int r = (int)(e / J), c = (int)(e - (size_t)r * J), s = r % a.S, t = r / a.S;
      const int4 me = a.ws.meta[s];
      if (me.x == -1) continue;
      float v = 0.f;
      if (me.x == 1 && t < me.y)
        for (int w = 0; w < ESLOTS; w++) v += a.ws.dep[(size_t)w * ne + e];
      a.d_enc[(size_t)r * a.de_stride + c] = v;
    } else if (e < ne + np) {
      const size_t i = e - ne;
      const int r = (int)(i / J), c = (int)(i - (size_t)r * J), s = r % a.S, u = r / a.S;
      const int4 me = a.ws.meta[s];
      if (me.x == -1) continue;
      float v = 0.f;
      if (me.x == 1 && u <= me.z)
        for (int tb = 0; tb * RT < me.y; tb++) v += a.ws.dpp[(size_t)tb * np + i];
      a.d_pred[(size_t)r * a.dp_stride + c] = v;
    } else {
      const size_t i = e - ne - np;
      double v = 0.0;
      const size_t nwj = (size_t)a.V * J;
      if (i < nwj) {
        for (int c = 0; c < a.splits; c++) v += (double)a.ws.wpart[(size_t)c * nwj + i];
        a.Wg[i] = (float)v;
      } else {
        for (int c = 0; c < a.splits; c++) v += a.ws.bpart[(size_t)c * a.V + (i - nwj)];
        a.bg[i - nwj] = (float)v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_rnnt_pack(const int *labels, const int *loff, int S, int V, int bos, const float *embed, const float *bias,
                                                   int width, float *out, int out_stride) {
  const int r = blockIdx.x, s = r % S, u = r / S, o0 = loff[s], U = loff[s + 1] - o0;
  int x = -1;
  if (u == 0) x = bos;
  else if (u <= U) x = labels[o0 + u - 1];
  if (x < 0 || x >= V) x = -1;
  for (int c = threadIdx.x; c < width; c += 256) {
    float v = 0.f;
    if (x >= 0) v = embed ? embed[(size_t)c * V + x] + (bias ? bias[c] : 0.f) : (c == x ? 1.f : 0.f);
    out[(size_t)r * out_stride + c] = v;
  }
}

hipError_t rnnt_launch_prep(const RnntArgs &a, hipStream_t st) { return launch(k_rnnt_prep, dim3(1), dim3(64), 0, st, LaunchProbe(), a); }

hipError_t rnnt_launch_joint_fwd(const RnntArgs &a, hipStream_t st) {
  return launch(k_rnnt_joint_fwd, dim3((a.T + RT - 1) / RT, (a.U1 + RU - 1) / RU, a.S), dim3(256),
                ((size_t)(RT + RU) * (a.J + 2) + VP * WPS) * sizeof(float), st, LaunchProbe(), a);
}

hipError_t rnnt_launch_lattice(const RnntArgs &a, hipStream_t st) {
  const size_t N = (size_t)a.S * a.T * a.U1;
  const hipError_t e = launch(k_rnnt_lattice, dim3(a.S, 2), dim3((a.U1 + 63) / 64 * 64), 0, st, LaunchProbe(), a);
  if (e != hipSuccess) return e;
  return launch(k_rnnt_weights, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, LaunchProbe(), a);
}

static bool al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

const char *rnnt_limits(int T, int S, int Umax, int J, int V) {
  if (S < 1 || S > 32) return "1 <= S <= 32";
  if (T < 1) return "1 <= T";
  if (Umax < 0 || Umax > 1023) return "0 <= Umax <= 1023";
  if ((long long)T * (Umax + 1) * S > (1ll << 24)) return "T (Umax+1) S <= 2^24";
  if (J < 16 || J > 1024 || J % 16 != 0) return "16 <= J <= 1024, J % 16 == 0";
  if (V < 2 || V > 4096) return "2 <= V <= 4096";
  return nullptr;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

int krnnt_grad_splits(int J, int V) { return (J < 1 || V < 1) ? 0 : rnnt_splits(J, V); }

size_t krnnt_workspace_bytes(int T, int S, int Umax, int J, int V) {
  if (const char *why = rnnt_limits(T, S, Umax, J, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_workspace_bytes: T %d, S %d, Umax %d, J %d, V %d: the limit is %s", T, S, Umax, J, V, why);
    return 0;
  }
  size_t bytes = 0;
  rnnt_carve(nullptr, T, S, Umax + 1, J, V, true, &bytes);
  return bytes;
}

size_t krnnt_forward_workspace_bytes(int T, int S, int Umax) {
  if (const char *why = rnnt_limits(T, S, Umax, 16, 2)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_forward_workspace_bytes: T %d, S %d, Umax %d: the limit is %s", T, S, Umax, why);
    return 0;
  }
  size_t bytes = 0;
  rnnt_carve(nullptr, T, S, Umax + 1, 16, 2, false, &bytes);
  return bytes;
}

klstm_status krnnt_eval(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                        int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                        float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad, float *b_grad,
                        float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  if (const char *why = rnnt_limits(T, S, Umax, J, V))
    return fail(KLSTM_ERR_SHAPE, "krnnt_eval: T %d, S %d, Umax %d, J %d, V %d: the limit is %s", T, S, Umax, J, V, why);
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_eval: blank %d outside [0, %d)", blank, V);
  if (!enc || !pred || !W || !b || !lens_dev || !labels_dev || !label_offsets_dev || !utt_loss_dev || !workspace)
    return fail(KLSTM_ERR_ARG, "krnnt_eval: null argument");
  const int ngrad = (d_enc != nullptr) + (d_pred != nullptr) + (W_grad != nullptr) + (b_grad != nullptr);
  if (ngrad != 0 && ngrad != 4) return fail(KLSTM_ERR_ARG, "krnnt_eval: the four gradient outputs are given together or not at all");
  if (enc_stride < J || pred_stride < J || (ngrad && (d_enc_stride < J || d_pred_stride < J)))
    return fail(KLSTM_ERR_ARG, "krnnt_eval: row stride below the width %d (%d, %d, %d, %d)", J, enc_stride, pred_stride, d_enc_stride, d_pred_stride);
  if (!al4(enc) || !al4(pred) || !al4(W) || !al4(b) || !al4(d_enc) || !al4(d_pred) || !al4(W_grad) || !al4(b_grad) || !al4(utt_loss_dev) ||
      (reinterpret_cast<uintptr_t>(totals_dev) & 7))
    return fail(KLSTM_ERR_ARG, "krnnt_eval: misaligned pointer");
  RnntArgs a;
  size_t need = 0;
  a.ws = rnnt_carve(workspace, T, S, Umax + 1, J, V, ngrad != 0, &need);
  if (workspace_bytes < need) return fail(KLSTM_ERR_ARG, "krnnt_eval: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(KLSTM_ERR_ARG, "krnnt_eval: the workspace is not 256-byte aligned");
  a.enc = enc; a.pred = pred; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.U1 = Umax + 1; a.J = J; a.V = V; a.blank = blank;
  a.lens = lens_dev; a.labels = labels_dev; a.loff = label_offsets_dev;
  a.d_enc = d_enc; a.d_pred = d_pred; a.Wg = W_grad; a.bg = b_grad; a.de_stride = d_enc_stride; a.dp_stride = d_pred_stride;
  a.utt_loss = utt_loss_dev; a.totals = totals_dev;
  a.splits = rnnt_splits(J, V); a.ntb = (T + RT - 1) / RT;
  hipStream_t st = (hipStream_t)hip_stream;
  const int Jp = J + 2, U1 = a.U1;
  HIPCHK(rnnt_launch_prep(a, st));
  HIPCHK(rnnt_launch_joint_fwd(a, st));
  HIPCHK(rnnt_launch_lattice(a, st));
  if (!ngrad) return KLSTM_OK;
  const size_t shm = ((size_t)(RT + BU) * Jp + VP * WPS + 64 * GS) * sizeof(float);
  if (J <= 128) HIPCHK(launch(k_rnnt_joint_bwd<8>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  else if (J <= 512) HIPCHK(launch(k_rnnt_joint_bwd<32>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  else HIPCHK(launch(k_rnnt_joint_bwd<64>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  const size_t nfin = (size_t)S * T * J + (size_t)S * U1 * J + (size_t)V * J + V;
  const size_t gfin = (nfin + 255) / 256;
  HIPCHK(launch(k_rnnt_finish, dim3((unsigned)(gfin < 4096 ? gfin : 4096)), dim3(256), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status krnnt_pack(const int *labels_dev, const int *label_offsets_dev, int S, int Umax, int V, int bos, const float *embed,
                        const float *embed_bias, int D, float *out, int out_stride, void *hip_stream) {
  if (S < 1 || S > 32 || Umax < 0 || Umax > 1023 || V < 1 || (embed && D < 1))
    return fail(KLSTM_ERR_SHAPE, "krnnt_pack: S %d, Umax %d, V %d, D %d beyond the limits", S, Umax, V, D);
  if (bos < 0 || bos >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_pack: bos %d outside [0, %d)", bos, V);
  if (!labels_dev || !label_offsets_dev || !out) return fail(KLSTM_ERR_ARG, "krnnt_pack: null argument");
  const int width = embed ? D : V;
  if (out_stride < width) return fail(KLSTM_ERR_ARG, "krnnt_pack: row stride %d below the width %d", out_stride, width);
  HIPCHK(launch(k_rnnt_pack, dim3((Umax + 1) * S), dim3(256), 0, (hipStream_t)hip_stream, LaunchProbe(), labels_dev, label_offsets_dev, S, V, bos,
                embed, embed_bias, width, out, out_stride));
  return KLSTM_OK;
}

}  // extern "C"
