// kaldi-lstm_amd/csrc/klstm_rnnt_band.hip -- band-pruned RNN-transducer training: krnnt_band_eval, its workspace sizes and
// krnnt_band_from_frames (include/klstm_rnnt.h, BAND-PRUNED TRAINING, states every quantity; the torch yardstick:
// tests/rnnt_band_ref.py).  Only the nodes (t, u0(t) + r), 0 <= r < R, exist: the joint runs on T R nodes per stream instead of
// T (U+1), the planes are band-relative [S][T][R], and as in klstm_rnnt.hip neither h nor the logits ever go to memory.
//   k_rband_prep      one workgroup per stream: labels and band checked by all threads (the band's three conditions, one frame per
//                     thread), status / T_s / U_s / label offset for every kernel behind it.
//   k_rband_joint_fwd a workgroup (4 waves) owns 16 frames x 8 band offsets of one stream; a wave owns two M-tiles (16 frames at one
//                     offset r each).  Lane row i of an M-tile needs pred row u0(t0 + i) + r: a different row per frame, and the rows of
//                     one tile span up to 15 (R-1) + R label positions, so no whole-row staging.  band_joint_logits() gathers the
//                     operand per NODE into LDS in the k-panels of 32 that W streams through: Zp [node][k] = enc[t][k] + pred[u][k],
//                     128 nodes x 32 k per panel, row stride 34 floats like the W panel (an A read of lane (i, kg) hits bank
//                     2 i + kg: 32 distinct banks per half wave; the panel's stores run along k).  h = tanh(Zp) is formed in registers as
//                     the MFMA16 A operand, once per k-step for all class tiles of the pass (128 classes, running max and sum over the
//                     passes), each panel a chain of its own.  The LDS footprint does not depend on J.
//   k_rband_lattice   grid (S, 2), ONE WAVE per (stream, direction), lane = band offset r, no workgroup barrier.  The wave walks the
//                     anti-diagonals d = t + u (T_s + U dependent steps).  t + u0(t) grows strictly with t, so lane r meets at most one
//                     node per diagonal: it keeps its own frame pointer and works when pointer + u0(pointer) + r == d.  The two
//                     predecessors lie on the diagonal before, in other lanes' registers: the label step in lane r -/+ 1, the blank
//                     step in lane r +/- (u0(t) - u0(t-1)) -- the row shift is applied right there, in the lane index of the shuffle.
//                     Every lane carries u0 of its next eight frames and lpb / lpy of its next four in registers, loaded that far ahead
//                     of use.  Values are doubles in registers, stored as floats minus the maximum of the diagonal before; the maxima
//                     are summed in double (the offsets) and the loss is taken in double, as in k_rnnt_lattice.
//   k_rband_weights   one thread per band node: w_b (only if (t+1, u) is in the band, or at the last node), w_y (only if r + 1 < R).
//   k_rband_joint_bwd<NJ>  krnnt_grad_splits() persistent workgroups over the units (stream, 16 frames), a unit's band offsets four at a
//                     time, one M-tile per wave.  The logits again (the same function, the same bits), g through the 64 x 128 LDS tile
//                     into dz += g W and the workgroup's own W_grad / b_grad partial, as k_rnnt_joint_bwd does.  Then dz (1 - h^2) of the
//                     64 nodes goes through the same LDS tile, 128 columns at a time, to COLUMN OWNERS: thread c < 128 owns column c of
//                     d_pred, thread 128 + c column c of d_enc.  The d_enc owner adds the four offsets of a frame in order and adds to
//                     d_enc[t] itself: a unit owns its frames, so d_enc needs no partials at all.  The d_pred owner walks offset by
//                     offset, frame by frame (u0(t) + r does not fall along that walk), sums runs of equal u and adds each run to the
//                     unit's window row u: one thread, one order, although many (t, r) of the tile hit the same u.
//                     The window of unit b covers the label rows u0(16 b) .. u0(last frame of b) + R - 1 and lives at rows u + b R of
//                     a per-stream array: the padded spans u0(16 (b+1)) - u0(16 b) + R telescope, so their prefix sum is u0(16 b) + b R
//                     and no scan is needed; (Umax+1) + tb R rows hold every window.
//   k_rband_finish    d_pred[u] = the windows that hold u, in block order (they are consecutive: a binary search finds the first);
//                     zero rows of d_enc and d_pred where the definition says so; W_grad / b_grad = the splits in order, in double.
//   k_rband_from_frames  one workgroup per stream: c(t) by binary search in the label frames, the clamp, then the suffix maximum of
//                     u0(t) - t (R-1) in chunks of 256 frames from the end (band_close() of klstm_rnnt_dev.h, which
//                     krnnt_band_from_occupation ends with as well).
// BOUNDS.  A node is touched only with t < T_s, r < R and u0(t) + r <= U_s (nodeU[] in LDS holds u or -1 per node of the tile and every
// access goes through it); band entries are read only for t < T_s of a stream whose band the prep kernel accepted; classes >= V are
// masked at the panel load and in the epilogues; offsets are size_t products.
#include <climits>
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_band_dev.h"            // the tile constants, BandWs, BandArgs and the device code shared with klstm_rnnt_band16.hip

namespace klstm {

static int band_splits(int J, int V) {
  const long long s = (1ll << 24) / ((long long)V * J);
  return s < 8 ? 8 : s > 256 ? 256 : (int)s;
}

// the layout of the workspace (include/klstm_rnnt.h states the formula); base null: only bytes() counts
BandWs band_carve(void *base, int T, int S, int U1, int R, int J, int V, bool grads, size_t *bytes) {
  CtcCarver c(base);
  BandWs w;
  const size_t N = (size_t)S * T * R, ntb = (size_t)(T + RT - 1) / RT;
  w.meta = c.take<int4>(S);
  w.loss = c.take<double>(S);
  w.offs = c.take<double>((size_t)2 * S * (T + OFFS_U));
  w.lpb = c.take<float>(N); w.lpy = c.take<float>(N); w.lse = c.take<float>(N);
  w.A = c.take<float>(N); w.B = c.take<float>(N); w.wb = c.take<float>(N); w.wy = c.take<float>(N);
  w.dpp = w.wpart = nullptr; w.bpart = nullptr;
  if (grads) {
    w.dpp = c.take<float>((size_t)S * (U1 + ntb * R) * J);
    w.wpart = c.take<float>((size_t)band_splits(J, V) * V * J);
    w.bpart = c.take<double>((size_t)band_splits(J, V) * V);
  }
  *bytes = c.bytes();
  return w;
}

__global__ __launch_bounds__(256) void k_rband_prep(BandArgs a) {
  __shared__ int bad;
  const int s = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) bad = 0;
  __syncthreads();
  const int Ts = a.lens[s], o0 = a.loff[s], o1 = a.loff[s + 1], U = o1 - o0;
  int st = 1;
  if (Ts == 0) st = 0;
  else if (Ts < 0 || Ts > a.T || U < 0 || U > a.U1 - 1 || o0 < 0) st = -1;
  if (st == 1) {
    int b = 0;
    for (int i = o0 + tid; i < o1; i += 256) {
      const int y = a.labels[i];
      if (y < 0 || y >= a.V || y == a.blank) b = 1;
    }
    const int *u0 = a.band + (size_t)s * a.T;
    for (int t = tid; t < Ts; t += 256) {                // the three conditions of a valid band
      const long long c = u0[t];
      if (t == 0 && c != 0) b = 1;
      if (t + 1 < Ts) {
        const long long dl = (long long)u0[t + 1] - c;
        if (dl < 0 || dl > a.R - 1) b = 1;
      } else if (c > U || c + a.R - 1 < U) b = 1;
    }
    if (b) atomicOr(&bad, 1);                            // an integer flag: the order does not matter
  }
  __syncthreads();
  if (tid == 0) {
    if (st == 1 && bad) st = -1;
    a.ws.meta[s] = make_int4(st, st == 1 ? Ts : 0, st == 1 ? U : 0, o0);
  }
}

// The sibling of joint_logits() (klstm_rnnt_dev.h) for a band: the logits (without bias) of the workgroup's 4 MT M-tiles, M-tile
// wave MT + m of the calling wave; node 16 mtile + i has frame t0 + i and pred row nodeU[node].  Per k-panel the W rows and the nodes'
// enc + pred rows go to LDS (Wp, Zp); a node that does not exist gets zeros (h = 0).  Called by all 256 threads together.
template <int MT>
__device__ __forceinline__ void band_joint_logits(const float *__restrict__ enc, int enc_stride, const float *__restrict__ pred, int pred_stride,
                                                  int S, int s, int t0, const int *nodeU, const float *__restrict__ W, int J, int V, int v0, int nvt,
                                                  float *Wp, float *Zp, f32x4 (&acc)[MT][NVT]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) acc[m][vt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kp = 0; kp < J; kp += KP) {
    const int kw = min(KP, J - kp);
    __syncthreads();                                   // the panel before is done with (and the caller's LDS stores are visible)
    for (int e = tid; e < nvt * 16 * KP; e += 256) {
      const int v = e / KP, k = e - v * KP;
      Wp[v * WPS + k] = (v0 + v < V && k < kw) ? W[(size_t)(v0 + v) * J + kp + k] : 0.f;
    }
    for (int e = tid; e < 4 * MT * 16 * KP; e += 256) {
      const int node = e / KP, k = e - node * KP, u = nodeU[node];
      float z = 0.f;
      if (u >= 0 && k < kw)
        z = enc[((size_t)(t0 + (node & 15)) * S + s) * enc_stride + kp + k] + pred[((size_t)u * S + s) * pred_stride + kp + k];
      Zp[node * WPS + k] = z;
    }
    __syncthreads();
    f32x4 part[MT][NVT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) part[m][vt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < kw; ks += 4) {
      float h[MT];
#pragma unroll
      for (int m = 0; m < MT; m++) h[m] = k_tanh(Zp[((wave * MT + m) * 16 + i16) * WPS + ks + kg]);
#pragma unroll
      for (int vt = 0; vt < NVT; vt++)
        if (vt < nvt) {
          const float bv = Wp[(vt * 16 + i16) * WPS + ks + kg];
#pragma unroll
          for (int m = 0; m < MT; m++) part[m][vt] = MFMA16(h[m], bv, part[m][vt]);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int vt = 0; vt < NVT; vt++)
        if (vt < nvt) acc[m][vt] += part[m][vt];
  }
}

__global__ __launch_bounds__(256) void k_rband_joint_fwd(BandArgs a) {
  __shared__ float Wp[VP * WPS];
  __shared__ float Zp[16 * BR * WPS];
  __shared__ int nodeU[16 * BR];
  const int J = a.J, V = a.V, R = a.R;
  const int s = blockIdx.z, t0 = blockIdx.x * RT, r0 = blockIdx.y * BR;
  const int4 me = a.ws.meta[s];
  if (me.x != 1 || t0 >= me.y) return;
  const int Ts = me.y, U = me.z;
  band_nodes(nodeU, 16 * BR, a.band + (size_t)s * a.T, t0, r0, Ts, U, R);
  __syncthreads();
  if (nodeU[0] < 0) return;                            // u0 does not fall: without node (t0, r0) the tile has none
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15, kg = lane >> 4;
  int nu[2][4], lab[2][4];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      nu[m][j] = nodeU[(2 * wave + m) * 16 + 4 * kg + j];
      lab[m][j] = (nu[m][j] >= 0 && nu[m][j] < U) ? a.labels[me.w + nu[m][j]] : -1;
    }
  float mrun[2][4], srun[2][4], ab[2][4], ay[2][4];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int j = 0; j < 4; j++) { mrun[m][j] = RLOG0; srun[m][j] = 0.f; ab[m][j] = 0.f; ay[m][j] = 0.f; }
  for (int v0 = 0; v0 < V; v0 += VP) {
    const int nvt = (min(VP, V - v0) + 15) / 16;
    f32x4 acc[2][NVT];
    band_joint_logits<2>(a.enc, a.enc_stride, a.pred, a.pred_stride, a.S, s, t0, nodeU, a.W, J, V, v0, nvt, Wp, Zp, acc);
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
          py += v == lab[m][j] ? x[vt] : 0.f;
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
    for (int j = 0; j < 4; j++)
      if (i16 == j && nu[m][j] >= 0) {
        const size_t n = ((size_t)s * a.T + t0 + 4 * kg + j) * R + r0 + 2 * wave + m;
        const float lse = mrun[m][j] + logf(srun[m][j]);
        a.ws.lpb[n] = ab[m][j] - lse;
        a.ws.lpy[n] = nu[m][j] < U ? ay[m][j] - lse : RLOG0;
        a.ws.lse[n] = lse;
      }
}

__device__ __forceinline__ double band_logadd(double x, double y) {
  const double m = fmax(x, y), d = fmin(x, y) - m;
  if (m <= -1e29) return (double)RLOG0;
  return m + log1p(exp(d));
}

// DIR 0: alpha, up the diagonals; DIR 1: beta, down.  Stored value of diagonal d = true value - offs[d].  One wave; lane = band offset.
template <int DIR>
__device__ __forceinline__ void band_lattice_run(const BandArgs &a, int s, int Ts, int U) {
  constexpr int QU = 9, QD = 4, STEP = DIR ? -1 : 1;   // q[i] = u0(t + (i-1) STEP): the row before, the lane's row, seven rows ahead
  const int r = threadIdx.x, R = a.R, nd = Ts + U;
  const int *u0 = a.band + (size_t)s * a.T;
  const size_t base = (size_t)s * a.T * R;
  const float *lpb = a.ws.lpb + base, *lpy = a.ws.lpy + base;
  float *out = (DIR == 0 ? a.ws.A : a.ws.B) + base;
  double *offs = a.ws.offs + (size_t)(2 * s + DIR) * a.L;
  auto band_at = [&](int t) { return u0[min(max(t, 0), Ts - 1)]; };
  // what row tt gives lane r: alpha: lpb(tt-1, u), lpy(tt, u-1); beta: lpb(tt, u), lpy(tt, u); u = ucur + r
  auto fetch = [&](int tt, int uprev, int ucur, float &fb, float &fy) {
    fb = 0.f; fy = 0.f;
    if (r >= R || tt < 0 || tt >= Ts || ucur + r > U) return;
    if (DIR == 0) {
      const int src = r + ucur - uprev;
      if (tt > 0 && src < R) fb = lpb[(size_t)(tt - 1) * R + src];
      if (r > 0) fy = lpy[(size_t)tt * R + r - 1];
    } else {
      fb = lpb[(size_t)tt * R + r];
      fy = lpy[(size_t)tt * R + r];
    }
  };
  int t = DIR ? Ts - 1 : 0, q[QU];
#pragma unroll
  for (int i = 0; i < QU; i++) q[i] = band_at(t + (i - 1) * STEP);
  float cb[QD], cy[QD];
#pragma unroll
  for (int i = 0; i < QD; i++) fetch(t + i * STEP, q[i], q[i + 1], cb[i], cy[i]);
  double prev = (double)RLOG0, offacc = 0.0;
  float mprev = 0.f;
  for (int e = 0; e < nd; e++) {
    const int d = DIR == 0 ? e : nd - 1 - e;
    const bool live = r < R && t >= 0 && t < Ts;
    const int key = t + q[1] + r, u = q[1] + r;
    const bool hit = live && key == d;
    // alpha: key >= d always, the pointer moves on a hit; beta: key > d is a node with u > U, passed over one per step
    const bool adv = live && (DIR == 0 ? key == d : key >= d);
    const int sh = DIR == 0 ? q[1] - q[0] : q[0] - q[1];           // u0(t) - u0(t-1), or u0(t+1) - u0(t): the row shift
    const int src = DIR == 0 ? r + sh : r - sh;
    const double pblank = __shfl(prev, min(max(src, 0), 63));
    const double plabel = __shfl(prev, DIR == 0 ? max(r - 1, 0) : min(r + 1, 63));
    double val = (double)RLOG0;
    if (hit && u <= U) {
      if (DIR == 0) {
        if (e == 0) val = 0.0;
        else {
          const double x1 = (t > 0 && src < R) ? pblank + cb[0] : (double)RLOG0, x2 = r > 0 ? plabel + cy[0] : (double)RLOG0;
          val = band_logadd(x1, x2) - mprev;
        }
      } else {
        if (e == 0) val = cb[0];
        else {
          const double x1 = (t + 1 < Ts && src >= 0) ? pblank + cb[0] : (double)RLOG0;
          const double x2 = (r + 1 < R && u < U) ? plabel + cy[0] : (double)RLOG0;
          val = band_logadd(x1, x2) - mprev;
        }
      }
      if (val < -1e29) val = (double)RLOG0;
      out[(size_t)t * R + r] = (float)val;
    }
    float wm = (float)val;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
    offacc += (double)mprev;
    if (r == 0) {
      offs[d] = offacc;
      if (DIR == 1 && e == nd - 1) {                     // node (0, 0): this lane
        const double loss = -(val + offacc);
        a.ws.loss[s] = loss;
        a.utt_loss[s] = (float)loss;
      }
    }
    if (adv) {
      t += STEP;
#pragma unroll
      for (int i = 0; i + 1 < QU; i++) q[i] = q[i + 1];
      q[QU - 1] = band_at(t + (QU - 2) * STEP);
#pragma unroll
      for (int i = 0; i + 1 < QD; i++) { cb[i] = cb[i + 1]; cy[i] = cy[i + 1]; }
      fetch(t + (QD - 1) * STEP, q[QD - 1], q[QD], cb[QD - 1], cy[QD - 1]);
    }
    prev = val;
    mprev = wm;
  }
}

__global__ __launch_bounds__(64) void k_rband_lattice(BandArgs a) {
  const int s = blockIdx.x;
  const int4 me = a.ws.meta[s];
  if (me.x != 1) {
    if (blockIdx.y == 1 && threadIdx.x == 0) { a.ws.loss[s] = 0.0; a.utt_loss[s] = 0.f; }
    return;
  }
  if (blockIdx.y == 0) band_lattice_run<0>(a, s, me.y, me.z);
  else band_lattice_run<1>(a, s, me.y, me.z);
}

__global__ __launch_bounds__(256) void k_rband_weights(BandArgs a) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x, N = (size_t)a.S * a.T * a.R;
  if (n == 0 && a.totals) {
    for (int s = 0; s < a.S; s++) {
      const int4 me = a.ws.meta[s];
      if (me.x == 1) { a.totals[0] += a.ws.loss[s]; a.totals[1] += me.y; a.totals[2] += me.z; a.totals[3] += 1.0; }
      if (me.x == -1) { a.totals[3] += 1.0; a.totals[4] += 1.0; }
    }
  }
  if (n >= N) return;
  const int R = a.R, r = (int)(n % R), t = (int)((n / R) % a.T), s = (int)(n / ((size_t)R * a.T));
  const int4 me = a.ws.meta[s];
  float wb = 0.f, wy = 0.f;
  if (me.x == 1 && t < me.y) {
    const int Ts = me.y, U = me.z;
    const int *u0 = a.band + (size_t)s * a.T;
    const int u = u0[t] + r;
    if (u <= U) {
      const int d = t + u;
      const double *oA = a.ws.offs + (size_t)(2 * s) * a.L, *oB = oA + a.L;
      const double loss = a.ws.loss[s], al = (double)a.ws.A[n] + oA[d];
      if (t == Ts - 1) {
        if (u == U) wb = (float)exp(al + (double)a.ws.lpb[n] + loss);
      } else {
        const int src = u - u0[t + 1];                   // (t+1, u) is in the band iff src >= 0 (src <= r < R always)
        if (src >= 0) wb = (float)exp(al + (double)a.ws.lpb[n] + ((double)a.ws.B[n - r + R + src] + oB[d + 1]) + loss);
      }
      if (u < U && r + 1 < R) wy = (float)exp(al + (double)a.ws.lpy[n] + ((double)a.ws.B[n + 1] + oB[d + 1]) + loss);
    }
  }
  a.ws.wb[n] = wb;
  a.ws.wy[n] = wy;
}

template <int NJ>
__global__ __launch_bounds__(256) void k_rband_joint_bwd(BandArgs a) {
  extern __shared__ float lds[];
  const int J = a.J, V = a.V, Jp = J + 2, S = a.S, R = a.R;
  float *encL = lds, *Wp = encL + RT * Jp, *Zp = Wp + VP * WPS, *G = Zp + 64 * WPS;
  int *nodeU = reinterpret_cast<int *>(G + 64 * BGS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const size_t wsz = (size_t)V * J;
  float *wpart = a.ws.wpart + (size_t)blockIdx.x * wsz;
  double *bpart = a.ws.bpart + (size_t)blockIdx.x * V;
  for (size_t e = tid; e < wsz; e += 256) wpart[e] = 0.f;
  for (int e = tid; e < V; e += 256) bpart[e] = 0.0;
  for (int unit = blockIdx.x; unit < S * a.ntb; unit += gridDim.x) {
    const int s = unit / a.ntb, tb = unit - s * a.ntb, t0 = tb * RT;
    const int4 me = a.ws.meta[s];
    if (me.x != 1 || t0 >= me.y) continue;
    const int Ts = me.y, U = me.z;
    const int *u0 = a.band + (size_t)s * a.T;
    const int lo = u0[t0], hi = min(U, u0[min(t0 + RT, Ts) - 1] + R - 1);
    float *win = a.ws.dpp + ((size_t)s * a.prow + (size_t)tb * R) * J;     // row u of the unit's window: win + u J
    __syncthreads();                                   // the unit before is done with encL (and the zeros above are visible)
    rnnt_stage(encL, Jp, a.enc, a.enc_stride, t0, RT, min(RT, Ts - t0), S, s, J);
    if (tid < 128)                                     // the column owners clear their columns of the window
      for (int u = lo; u <= hi; u++)
        for (int col = tid; col < J; col += 128) win[(size_t)u * J + col] = 0.f;
    for (int rb = 0; rb < R; rb += BBU) {
      __syncthreads();                                 // the step before is done with nodeU and G
      band_nodes(nodeU, 64, u0, t0, rb, Ts, U, R);
      __syncthreads();
      if (nodeU[0] < 0) break;                         // no node at (t0, rb): none at any later frame or offset
      int nu[4], lab[4];
      float lse[4], wb[4], wy[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        nu[j] = nodeU[wave * 16 + 4 * kg + j];
        const bool rv = nu[j] >= 0;
        const size_t n = rv ? ((size_t)s * a.T + t0 + 4 * kg + j) * R + rb + wave : 0;
        lab[j] = (rv && nu[j] < U) ? a.labels[me.w + nu[j]] : -1;
        lse[j] = rv ? a.ws.lse[n] : 0.f;
        wb[j] = rv ? a.ws.wb[n] : 0.f;
        wy[j] = rv ? a.ws.wy[n] : 0.f;
      }
      f32x4 dz[NJ];
#pragma unroll
      for (int nt = 0; nt < NJ; nt++) dz[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int v0 = 0; v0 < V; v0 += VP) {
        const int nvt = (min(VP, V - v0) + 15) / 16, nv = nvt * 16;
        f32x4 acc[1][NVT];
        band_joint_logits<1>(a.enc, a.enc_stride, a.pred, a.pred_stride, S, s, t0, nodeU, a.W, J, V, v0, nvt, Wp, Zp, acc);
        // g in registers, then into the tile: row = node (16 wave + frame), column = class of the pass
#pragma unroll
        for (int vt = 0; vt < NVT; vt++)
          if (vt < nvt) {
            const int v = v0 + vt * 16 + i16;
            const float bias = v < V ? a.b[v] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              float g = 0.f;
              if (nu[j] >= 0 && v < V) {
                g = (wb[j] + wy[j]) * expf(acc[0][vt][j] + bias - lse[j]);
                if (v == a.blank) g -= wb[j];
                if (v == lab[j]) g -= wy[j];
              }
              G[(wave * 16 + 4 * kg + j) * BGS + vt * 16 + i16] = g;
            }
          }
        __syncthreads();
        // dz += g W: K = the pass's classes
        for (int vs = 0; vs < nv; vs += 4) {
          const float av = G[(wave * 16 + i16) * BGS + vs + kg];
          const int vr = v0 + vs + kg;
          const float *wr = a.W + (size_t)(vr < V ? vr : 0) * J;
#pragma unroll
          for (int nt = 0; nt < NJ; nt++)
            if (nt * 16 < J) {
              const float bv = vr < V ? wr[nt * 16 + i16] : 0.f;
              dz[nt] = MFMA16(av, bv, dz[nt]);
            }
        }
        // W_grad partial += g^T h: K = the workgroup's 64 nodes; h again as the B operand (a missing node has g = 0)
        for (int nt = wave; nt * 16 < J; nt += 4) {
          const int col = nt * 16 + i16;
          f32x4 dw[NVT];
#pragma unroll
          for (int vt = 0; vt < NVT; vt++) dw[vt] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int q = 0; q < 16; q++) {
            const int node = 4 * q + kg, un = max(nodeU[node], 0);
            const float hb = k_tanh(encL[(node & 15) * Jp + col] + a.pred[((size_t)un * S + s) * a.pred_stride + col]);
#pragma unroll
            for (int vt = 0; vt < NVT; vt++)
              if (vt < nvt) dw[vt] = MFMA16(G[node * BGS + vt * 16 + i16], hb, dw[vt]);
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
          for (int node = 0; node < 64; node++) sum += (double)G[node * BGS + tid];
          bpart[v0 + tid] += sum;
        }
      }
      // dz (1 - h^2) through the tile, 128 columns at a time, to the column owners
#pragma unroll
      for (int c8 = 0; c8 < NJ / 8; c8++)
        if (c8 * 128 < J) {
          __syncthreads();                             // the readers of the tile are done
#pragma unroll
          for (int q = 0; q < 8; q++)
            if ((c8 * 8 + q) * 16 < J) {
              const int col = (c8 * 8 + q) * 16 + i16;
#pragma unroll
              for (int j = 0; j < 4; j++) {
                float v = 0.f;
                if (nu[j] >= 0) {
                  const float h = k_tanh(encL[(4 * kg + j) * Jp + col] + a.pred[((size_t)nu[j] * S + s) * a.pred_stride + col]);
                  v = dz[c8 * 8 + q][j] * (1.f - h * h);
                }
                G[(wave * 16 + 4 * kg + j) * BGS + q * 16 + i16] = v;
              }
            }
          __syncthreads();
          const int c = tid & 127, col = c8 * 128 + c;
          if (col < J) {
            if (tid < 128) {                           // d_pred: offset by offset, frame by frame, runs of equal u
              for (int w = 0; w < 4; w++) {
                int cu = -1;
                float run = 0.f;
                for (int fr = 0; fr < 16; fr++) {
                  const int u = nodeU[w * 16 + fr];
                  if (u < 0) continue;
                  if (u != cu) {
                    if (cu >= 0) win[(size_t)cu * J + col] += run;
                    cu = u; run = 0.f;
                  }
                  run += G[(w * 16 + fr) * BGS + c];
                }
                if (cu >= 0) win[(size_t)cu * J + col] += run;
              }
            } else {                                   // d_enc: the four offsets of a frame in order
              for (int fr = 0; fr < 16 && t0 + fr < Ts; fr++) {
                const float sum = ((G[fr * BGS + c] + G[(16 + fr) * BGS + c]) + G[(32 + fr) * BGS + c]) + G[(48 + fr) * BGS + c];
                float *p = a.d_enc + ((size_t)(t0 + fr) * S + s) * a.de_stride + col;
                *p = rb == 0 ? sum : *p + sum;
              }
            }
          }
        }
    }
  }
}

__global__ __launch_bounds__(256) void k_rband_finish(BandArgs a) {
  const size_t J = a.J, ne = (size_t)a.S * a.T * J, np = (size_t)a.S * a.U1 * J, nw = (size_t)a.V * J + a.V;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < ne + np + nw; e += (size_t)gridDim.x * 256) {
    if (e < ne) {                                      // rows t < T_s of a running stream were written by their units
      const int r = (int)(e / J), c = (int)(e - (size_t)r * J), s = r % a.S, t = r / a.S;
      const int4 me = a.ws.meta[s];
      if (me.x == 0 || (me.x == 1 && t >= me.y)) a.d_enc[(size_t)r * a.de_stride + c] = 0.f;
    } else if (e < ne + np) {
      const size_t i = e - ne;
      const int r = (int)(i / J), c = (int)(i - (size_t)r * J), s = r % a.S, u = r / a.S;
      const int4 me = a.ws.meta[s];
      if (me.x == -1) continue;
      float v = 0.f;
      if (me.x == 1 && u <= me.z) {
        const int Ts = me.y, R = a.R, nb = (Ts + RT - 1) / RT;
        const int *u0 = a.band + (size_t)s * a.T;
        int b0 = 0, b1 = nb;                           // the first block whose window reaches up to u
        while (b0 < b1) {
          const int m = (b0 + b1) >> 1;
          if (u0[min(m * RT + RT, Ts) - 1] + R - 1 >= u) b1 = m; else b0 = m + 1;
        }
        const float *win = a.ws.dpp + (size_t)s * a.prow * J + c;
        for (int bk = b0; bk < nb && u0[bk * RT] <= u; bk++) v += win[((size_t)u + (size_t)bk * R) * J];
      }
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

__global__ __launch_bounds__(256) void k_rband_from_frames(const int *frames, const int *lens, const int *loff, int T, int R, int left, int *band) {
  __shared__ int sc[256];
  __shared__ int bad, carry;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int Ts = lens[s], o0 = loff[s], U = loff[s + 1] - o0;
  int *row = band + (size_t)s * T;
  if (Ts <= 0 || Ts > T || U < 0 || o0 < 0) {
    for (int t = tid; t < T; t += 256) row[t] = Ts == 0 ? 0 : -1;
    return;
  }
  if (tid == 0) { bad = 0; carry = INT_MIN; }
  __syncthreads();
  const int hi = max(0, U + 1 - R), R1 = R - 1;
  if (frames) {
    int b = 0;
    for (int i = tid; i < U; i += 256) {
      const int f = frames[o0 + i];
      if (f < 0 || f >= Ts || (i + 1 < U && frames[o0 + i + 1] < f)) b = 1;
    }
    if (b) atomicOr(&bad, 1);
  }
  band_close(row, Ts, T, R1, hi, [&](int t) {          // the suffix scan and the row: klstm_rnnt_dev.h
    int c;
    if (frames) {                                      // c(t) = #{i : f_i < t}
      int i0 = 0, i1 = U;
      while (i0 < i1) {
        const int m = (i0 + i1) >> 1;
        if (frames[o0 + m] < t) i0 = m + 1; else i1 = m;
      }
      c = i0;
    } else c = (int)((long long)t * U / Ts);
    return t == Ts - 1 ? hi : min(max(c - left, 0), hi);
  }, sc, &carry, &bad);
}

static bool band_al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

const char *band_limits(int T, int S, int Umax, int R, int J, int V) {
  if (S < 1 || S > 32) return "1 <= S <= 32";
  if (T < 1) return "1 <= T";
  if (Umax < 0 || Umax > 1023) return "0 <= Umax <= 1023";
  if (R < 1 || R > 64) return "1 <= R <= 64";
  if ((long long)T * R * S > (1ll << 24)) return "S T R <= 2^24";
  if (J < 16 || J > 1024 || J % 16 != 0) return "16 <= J <= 1024, J % 16 == 0";
  if (V < 2 || V > 4096) return "2 <= V <= 4096";
  return nullptr;
}

klstm_status band_eval_args(const char *name, const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b,
                            int T, int S, int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                            int R, const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                            float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, size_t extra, BandArgs *out,
                            int *ngrad_out, size_t *band_bytes) {
  if (const char *why = band_limits(T, S, Umax, R, J, V))
    return fail(KLSTM_ERR_SHAPE, "%s: T %d, S %d, Umax %d, R %d, J %d, V %d: the limit is %s", name, T, S, Umax, R, J, V, why);
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "%s: blank %d outside [0, %d)", name, blank, V);
  if (!enc || !pred || !W || !b || !lens_dev || !labels_dev || !label_offsets_dev || !band_lo_dev || !utt_loss_dev || !workspace)
    return fail(KLSTM_ERR_ARG, "%s: null argument", name);
  const int ngrad = (d_enc != nullptr) + (d_pred != nullptr) + (W_grad != nullptr) + (b_grad != nullptr);
  if (ngrad != 0 && ngrad != 4) return fail(KLSTM_ERR_ARG, "%s: the four gradient outputs are given together or not at all", name);
  if (enc_stride < J || pred_stride < J || (ngrad && (d_enc_stride < J || d_pred_stride < J)))
    return fail(KLSTM_ERR_ARG, "%s: row stride below the width %d (%d, %d, %d, %d)", name, J, enc_stride, pred_stride, d_enc_stride, d_pred_stride);
  if (!band_al4(enc) || !band_al4(pred) || !band_al4(W) || !band_al4(b) || !band_al4(d_enc) || !band_al4(d_pred) || !band_al4(W_grad) ||
      !band_al4(b_grad) || !band_al4(utt_loss_dev) || !band_al4(band_lo_dev) || (reinterpret_cast<uintptr_t>(totals_dev) & 7))
    return fail(KLSTM_ERR_ARG, "%s: misaligned pointer", name);
  BandArgs a;
  size_t need = 0;
  a.ws = band_carve(workspace, T, S, Umax + 1, R, J, V, ngrad != 0, &need);
  *band_bytes = need;
  need += extra;
  if (workspace_bytes < need) return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(KLSTM_ERR_ARG, "%s: the workspace is not 256-byte aligned", name);
  a.enc = enc; a.pred = pred; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.U1 = Umax + 1; a.J = J; a.V = V; a.blank = blank; a.R = R;
  a.lens = lens_dev; a.labels = labels_dev; a.loff = label_offsets_dev; a.band = band_lo_dev;
  a.d_enc = d_enc; a.d_pred = d_pred; a.Wg = W_grad; a.bg = b_grad; a.de_stride = d_enc_stride; a.dp_stride = d_pred_stride;
  a.utt_loss = utt_loss_dev; a.totals = totals_dev;
  a.splits = band_splits(J, V); a.ntb = (T + RT - 1) / RT; a.prow = a.U1 + a.ntb * R; a.L = T + OFFS_U;
  *out = a;
  *ngrad_out = ngrad;
  return KLSTM_OK;
}

hipError_t band_launch_prep(const BandArgs &a, hipStream_t st) { return launch(k_rband_prep, dim3(a.S), dim3(256), 0, st, LaunchProbe(), a); }

hipError_t band_launch_joint_fwd(const BandArgs &a, hipStream_t st) {
  return launch(k_rband_joint_fwd, dim3(a.ntb, (a.R + BR - 1) / BR, a.S), dim3(256), 0, st, LaunchProbe(), a);
}

hipError_t band_launch_lattice(const BandArgs &a, hipStream_t st) {
  const size_t N = (size_t)a.S * a.T * a.R;
  const hipError_t e = launch(k_rband_lattice, dim3(a.S, 2), dim3(64), 0, st, LaunchProbe(), a);
  return e != hipSuccess ? e : launch(k_rband_weights, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, LaunchProbe(), a);
}

hipError_t band_launch_finish(const BandArgs &a, hipStream_t st) {
  const size_t nfin = (size_t)a.S * a.T * a.J + (size_t)a.S * a.U1 * a.J + (size_t)a.V * a.J + a.V;
  const size_t gfin = (nfin + 255) / 256;
  return launch(k_rband_finish, dim3((unsigned)(gfin < 4096 ? gfin : 4096)), dim3(256), 0, st, LaunchProbe(), a);
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_band_workspace_bytes(int T, int S, int Umax, int R, int J, int V) {
  if (const char *why = band_limits(T, S, Umax, R, J, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_band_workspace_bytes: T %d, S %d, Umax %d, R %d, J %d, V %d: the limit is %s", T, S, Umax, R, J, V, why);
    return 0;
  }
  size_t bytes = 0;
  band_carve(nullptr, T, S, Umax + 1, R, J, V, true, &bytes);
  return bytes;
}

size_t krnnt_band_forward_workspace_bytes(int T, int S, int R) {
  if (const char *why = band_limits(T, S, 0, R, 16, 2)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_band_forward_workspace_bytes: T %d, S %d, R %d: the limit is %s", T, S, R, why);
    return 0;
  }
  size_t bytes = 0;
  band_carve(nullptr, T, S, 1, R, 16, 2, false, &bytes);
  return bytes;
}

klstm_status krnnt_band_eval(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                             int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank, int R,
                             const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                             float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  BandArgs a;
  int ngrad = 0;
  size_t band_bytes = 0;
  const klstm_status bad = band_eval_args("krnnt_band_eval", enc, enc_stride, pred, pred_stride, W, b, T, S, Umax, J, V, lens_dev, labels_dev,
                                          label_offsets_dev, blank, R, band_lo_dev, d_enc, d_enc_stride, d_pred, d_pred_stride, W_grad, b_grad,
                                          utt_loss_dev, totals_dev, workspace, workspace_bytes, 0, &a, &ngrad, &band_bytes);
  if (bad != KLSTM_OK) return bad;
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(band_launch_prep(a, st));
  HIPCHK(band_launch_joint_fwd(a, st));
  HIPCHK(band_launch_lattice(a, st));
  if (!ngrad) return KLSTM_OK;
  const size_t shm = ((size_t)RT * (J + 2) + VP * WPS + 64 * WPS + 64 * BGS + 64) * sizeof(float);
  if (J <= 128) HIPCHK(launch(k_rband_joint_bwd<8>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  else if (J <= 512) HIPCHK(launch(k_rband_joint_bwd<32>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  else HIPCHK(launch(k_rband_joint_bwd<64>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), a));
  HIPCHK(band_launch_finish(a, st));
  return KLSTM_OK;
}

klstm_status krnnt_band_from_frames(const int *label_frames_dev, const int *lens_dev, const int *label_offsets_dev, int T, int S, int R, int left,
                                    int *band_lo_dev, void *hip_stream) {
  if (S < 1 || S > 32 || T < 1 || R < 1 || R > 64 || (long long)T * R * S > (1ll << 24))
    return fail(KLSTM_ERR_SHAPE, "krnnt_band_from_frames: T %d, S %d, R %d beyond 1 <= S <= 32, 1 <= T, 1 <= R <= 64, S T R <= 2^24", T, S, R);
  if (left < 0 || left >= R) return fail(KLSTM_ERR_SHAPE, "krnnt_band_from_frames: left %d outside [0, %d)", left, R);
  if (!lens_dev || !label_offsets_dev || !band_lo_dev) return fail(KLSTM_ERR_ARG, "krnnt_band_from_frames: null argument");
  if (!band_al4(label_frames_dev) || !band_al4(lens_dev) || !band_al4(label_offsets_dev) || !band_al4(band_lo_dev))
    return fail(KLSTM_ERR_ARG, "krnnt_band_from_frames: misaligned pointer");
  HIPCHK(launch(k_rband_from_frames, dim3(S), dim3(256), 0, (hipStream_t)hip_stream, LaunchProbe(), label_frames_dev, lens_dev, label_offsets_dev, T,
                R, left, band_lo_dev));
  return KLSTM_OK;
}

}  // extern "C"
