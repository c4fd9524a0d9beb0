// kaldi-lstm_amd/csrc/klstm_rnnt_simple.hip -- the additive "simple joiner" transducer loss and the band it selects: krnnt_simple_eval,
// its workspace size and krnnt_band_from_occupation (include/klstm_rnnt.h, THE SIMPLE JOINER, states every quantity; the
// torch yardstick: tests/rnnt_simple_ref.py).  The logits of node (t, u) are am[t] + lm[u], so the normaliser of all nodes of a stream
// is one matrix product, P = Ea El^T with Ea = exp(am - rowmax), El = exp(lm - rowmax), and both gradients are two more products with
// q = occ / P as the left operand.  No array of nodes x classes exists anywhere.
//   k_rsimple_exp     one workgroup per row of am and of lm: the row maximum, then exp(x - max) into the workspace, row (s, t) or (s, u)
//                     of Vp = V rounded up to 32 floats, the tail zero: the product kernels run whole K panels without class masks.
//                     A row outside its stream's lattice (t >= T_s, u > U_s, a stream that does not run) is written as zeros, so whatever
//                     the caller left in those rows of am / lm never reaches a sum.
//   k_rsimple_norm    a workgroup (4 waves) owns 16 frames x 64 label positions of one stream, a wave one 16 x 16 accumulator tile
//                     (MFMA16: exact f32 products).  K = Vp streams through LDS in panels of 32, both operands [row][k] with the row
//                     stride 34 of the joint's W panel: an operand read of lane (i, kg) hits bank 2 i + kg, 32 distinct banks per half
//                     wave, and the panel's stores run along k.  Every panel is a chain of its own that is added to the tile's sums.
//                     The epilogue clamps P at FLT_MIN, forms lse = ma + ml + log P, gathers a_blank and a_y from the ORIGINAL logits
//                     and writes lpb, lpy and P for the nodes under t < T_s, u <= U_s only.  P goes to the plane that holds lse in
//                     krnnt_eval (nothing behind reads lse): q = occ / P then needs no exp(lse - ma - ml), which would cost digits.
//   (klstm_rnnt.hip)  k_rnnt_prep before, k_rnnt_lattice and k_rnnt_weights behind, on the same planes: rnnt_launch_prep / _lattice.
//   k_rsimple_occ     one thread per node: occ = w_b + w_y to the caller's plane (zeros outside the lattice; a rejected stream's part
//                     untouched), q = occ / P over P in place.
//   k_rsimple_dam     d_am: a workgroup owns 16 frames x 128 classes (a wave 2 class tiles) and walks u = 0 .. U_s in order, 32 at a time:
//                     acc += q[t][u] El[u][v], the q panel in LDS [t][u] (stride 34), El rows straight from the workspace (16 lanes read
//                     64 consecutive bytes; the waves share no El element, so LDS would add a copy and no reuse).  One accumulation
//                     chain over all u: the order is fixed.  Epilogue: Ea[t][v] acc minus the indicator terms, summed in double by the
//                     thread that owns the element (all w_b of the frame for v = blank; w_y(t, u) of every u whose label is v; the
//                     stream's labels sit in LDS).  One writer per element; rows t >= T_s and idle streams: zeros.
//   k_rsimple_dlm     d_lm: 16 label rows x 128 classes, K = t walked in order over T_s; the q panel is staged transposed, [u][t].  The
//                     indicator terms of row u: all w_b(., u) for v = blank, all w_y(., u) for v = y_{u+1}.
//   k_rocc_center     krnnt_band_from_occupation, first kernel: one wave per (stream, frame); lane l takes the candidates k = l, l + 64,
//                     .. <= hi with the window sum in double in the order of r, keeps its best under `>`, then a wave arg-max where an
//                     equal sum goes to the lower k.  c(t) goes to band_lo itself.
//   k_rocc_band       one workgroup per stream: c(0) = 0 and c(T_s - 1) = hi, the prefix maximum in chunks of 256 frames from the start
//                     (an LDS scan per chunk and a carry), then band_close() (klstm_rnnt_dev.h), the suffix scan krnnt_band_from_frames
//                     ends with.
// BOUNDS.  Rows of the workspace operands are read only under t < T and u <= Umax (zeros beyond), columns under Vp; node planes under
// t < T, u <= Umax; am / lm / d_am / d_lm under v < V; a label is used as a column only for a stream the prep kernel accepted (every
// label in [0, V)); occ is read only for u <= U_s <= Umax (a stream with more labels than Umax gets a row of -1); offsets are size_t.
#include <cfloat>
#include <climits>
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_ctc_host.h"
#include "klstm_host.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_dev.h"

namespace klstm {

constexpr int SU = 64;                      // label positions of a normaliser tile (RT = 16 frames; KP, WPS: klstm_rnnt_dev.h)
constexpr int GV = 128;                     // classes of a gradient tile

struct SimpleArgs {
  RnntArgs r;                               // T, S, U1, V, blank, lens, labels, loff, utt_loss, totals, ws: what klstm_rnnt.hip's kernels read
  const float *am, *lm;
  int am_stride, lm_stride, Vp;
  float *Ea, *El, *ma, *ml;                 // [S T][Vp], [S U1][Vp], [S T], [S U1]
  float *d_am, *d_lm, *occ;
  int dam_stride, dlm_stride;
};

static int simple_vp(int V) { return (V + KP - 1) / KP * KP; }

// krnnt_eval's forward workspace, then the exponentiated operands and the row maxima (include/klstm_rnnt.h states the formula)
static void simple_carve(void *base, int T, int S, int U1, int V, SimpleArgs *a, size_t *bytes) {
  size_t head = 0;
  a->r.ws = rnnt_carve(base, T, S, U1, 16, 2, false, &head);
  CtcCarver c(base);
  c.off = head;
  const size_t Vp = simple_vp(V);
  a->Vp = (int)Vp;
  a->Ea = c.take<float>((size_t)S * T * Vp);
  a->El = c.take<float>((size_t)S * U1 * Vp);
  a->ma = c.take<float>((size_t)S * T);
  a->ml = c.take<float>((size_t)S * U1);
  *bytes = c.bytes();
}

__global__ __launch_bounds__(256) void k_rsimple_exp(SimpleArgs a) {
  __shared__ float red[4];
  const int T = a.r.T, S = a.r.S, U1 = a.r.U1, V = a.r.V, Vp = a.Vp, tid = threadIdx.x;
  const int row = blockIdx.x, nam = S * T;
  const bool is_am = row < nam;
  const int i = is_am ? row : row - nam, s = is_am ? i / T : i / U1, p = is_am ? i - s * T : i - s * U1;
  const int4 me = a.r.ws.meta[s];
  const bool live = me.x == 1 && (is_am ? p < me.y : p <= me.z);
  float *dst = (is_am ? a.Ea : a.El) + (size_t)i * Vp;
  float *mx = (is_am ? a.ma : a.ml) + i;
  if (!live) {
    for (int v = tid; v < Vp; v += 256) dst[v] = 0.f;
    if (tid == 0) *mx = 0.f;
    return;
  }
  const float *src = is_am ? a.am + ((size_t)p * S + s) * a.am_stride : a.lm + ((size_t)p * S + s) * a.lm_stride;
  float m = -FLT_MAX;
  for (int v = tid; v < V; v += 256) m = fmaxf(m, src[v]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int v = tid; v < Vp; v += 256) dst[v] = v < V ? expf(src[v] - m) : 0.f;
  if (tid == 0) *mx = m;
}

__global__ __launch_bounds__(256) void k_rsimple_norm(SimpleArgs a) {
  __shared__ float Ap[RT * WPS];
  __shared__ float Bp[SU * WPS];
  const int T = a.r.T, S = a.r.S, U1 = a.r.U1, Vp = a.Vp;
  const int s = blockIdx.z, t0 = blockIdx.x * RT, u0 = blockIdx.y * SU;
  const int4 me = a.r.ws.meta[s];
  if (me.x != 1 || t0 >= me.y || u0 > me.z) return;
  const int Ts = me.y, U = me.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const float *EaS = a.Ea + (size_t)s * T * Vp, *ElS = a.El + (size_t)s * U1 * Vp;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kp = 0; kp < Vp; kp += KP) {
    __syncthreads();                                   // the panel before is done with
    for (int e = tid; e < RT * KP; e += 256) {
      const int r = e / KP, k = e - r * KP;
      Ap[r * WPS + k] = t0 + r < T ? EaS[(size_t)(t0 + r) * Vp + kp + k] : 0.f;
    }
    for (int e = tid; e < SU * KP; e += 256) {
      const int r = e / KP, k = e - r * KP;
      Bp[r * WPS + k] = u0 + r < U1 ? ElS[(size_t)(u0 + r) * Vp + kp + k] : 0.f;
    }
    __syncthreads();
    f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KP; ks += 4) part = MFMA16(Ap[i16 * WPS + ks + kg], Bp[(wave * 16 + i16) * WPS + ks + kg], part);
    acc += part;
  }
  const int u = u0 + wave * 16 + i16;
  if (u > U) return;
  const int S_ = S, blank = a.r.blank;
  const float *lrow = a.lm + ((size_t)u * S_ + s) * a.lm_stride;
  const int lab = u < U ? a.r.labels[me.w + u] : -1;
  const float ml = a.ml[(size_t)s * U1 + u], lb = lrow[blank], ly = lab >= 0 ? lrow[lab] : 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int t = t0 + 4 * kg + j;
    if (t < Ts) {
      const float *arow = a.am + ((size_t)t * S_ + s) * a.am_stride;
      const float P = fmaxf(acc[j], FLT_MIN), lse = a.ma[(size_t)s * T + t] + ml + logf(P);
      const size_t n = ((size_t)s * T + t) * U1 + u;
      a.r.ws.lpb[n] = arow[blank] + lb - lse;
      a.r.ws.lpy[n] = lab >= 0 ? arow[lab] + ly - lse : RLOG0;
      a.r.ws.lse[n] = P;
    }
  }
}

__global__ __launch_bounds__(256) void k_rsimple_occ(SimpleArgs a) {
  const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x, N = (size_t)a.r.S * a.r.T * a.r.U1;
  if (n >= N) return;
  const int U1 = a.r.U1, u = (int)(n % U1), t = (int)((n / U1) % a.r.T), s = (int)(n / ((size_t)U1 * a.r.T));
  const int4 me = a.r.ws.meta[s];
  float occ = 0.f, q = 0.f;
  if (me.x == 1 && t < me.y && u <= me.z) {
    occ = a.r.ws.wb[n] + a.r.ws.wy[n];
    q = occ / a.r.ws.lse[n];
  }
  a.r.ws.lse[n] = q;
  if (a.occ && me.x != -1) a.occ[n] = occ;
}

// the labels of the stream into LDS (U <= 1023)
__device__ __forceinline__ void simple_labels(int *labL, const int *labels, int o0, int U) {
  for (int i = threadIdx.x; i < U; i += blockDim.x) labL[i] = labels[o0 + i];
}

__global__ __launch_bounds__(256) void k_rsimple_dam(SimpleArgs a) {
  __shared__ float Qp[RT * WPS];
  __shared__ int labL[1024];
  const int T = a.r.T, S = a.r.S, U1 = a.r.U1, V = a.r.V, Vp = a.Vp;
  const int s = blockIdx.z, t0 = blockIdx.x * RT, v0 = blockIdx.y * GV;
  const int4 me = a.r.ws.meta[s];
  if (me.x == -1) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const int Ts = me.y, U = me.z;
  if (me.x == 0 || t0 >= Ts) {                         // an idle stream, frames behind the stream's end: zero rows
    for (int e = tid; e < RT * GV; e += 256) {
      const int t = t0 + e / GV, v = v0 + e % GV;
      if (t < T && v < V) a.d_am[((size_t)t * S + s) * a.dam_stride + v] = 0.f;
    }
    return;
  }
  simple_labels(labL, a.r.labels, me.w, U);
  const float *q = a.r.ws.lse + (size_t)s * T * U1, *ElS = a.El + (size_t)s * U1 * Vp;
  const int vc[2] = {v0 + wave * 32 + i16, v0 + wave * 32 + 16 + i16};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int up = 0; up <= U; up += KP) {
    __syncthreads();                                   // the panel before is done with (and labL is visible)
    for (int e = tid; e < RT * KP; e += 256) {
      const int r = e / KP, k = e - r * KP;
      Qp[r * WPS + k] = (t0 + r < T && up + k < U1) ? q[(size_t)(t0 + r) * U1 + up + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KP; ks += 4) {
      const int u = up + ks + kg;
      const float av = Qp[i16 * WPS + ks + kg];
      const float *er = ElS + (size_t)(u < U1 ? u : 0) * Vp;
#pragma unroll
      for (int c = 0; c < 2; c++) acc[c] = MFMA16(av, (u < U1 && vc[c] < Vp) ? er[vc[c]] : 0.f, acc[c]);
    }
  }
  const float *wbS = a.r.ws.wb + (size_t)s * T * U1, *wyS = a.r.ws.wy + (size_t)s * T * U1;
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int t = t0 + 4 * kg + j, v = vc[c];
      if (t >= T || v >= V) continue;
      float out = 0.f;
      if (t < Ts) {
        double ind = 0.0;
        if (v == a.r.blank)
          for (int u = 0; u <= U; u++) ind += (double)wbS[(size_t)t * U1 + u];
        else
          for (int u = 0; u < U; u++)
            if (labL[u] == v) ind += (double)wyS[(size_t)t * U1 + u];
        out = (float)((double)a.Ea[((size_t)s * T + t) * Vp + v] * (double)acc[c][j] - ind);
      }
      a.d_am[((size_t)t * S + s) * a.dam_stride + v] = out;
    }
}

__global__ __launch_bounds__(256) void k_rsimple_dlm(SimpleArgs a) {
  __shared__ float Qp[RT * WPS];
  const int T = a.r.T, S = a.r.S, U1 = a.r.U1, V = a.r.V, Vp = a.Vp;
  const int s = blockIdx.z, u0 = blockIdx.x * RT, v0 = blockIdx.y * GV;
  const int4 me = a.r.ws.meta[s];
  if (me.x == -1) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const int Ts = me.y, U = me.z;
  if (me.x == 0 || u0 > U) {                           // an idle stream, label rows behind the stream's last: zero rows
    for (int e = tid; e < RT * GV; e += 256) {
      const int u = u0 + e / GV, v = v0 + e % GV;
      if (u < U1 && v < V) a.d_lm[((size_t)u * S + s) * a.dlm_stride + v] = 0.f;
    }
    return;
  }
  const float *q = a.r.ws.lse + (size_t)s * T * U1, *EaS = a.Ea + (size_t)s * T * Vp;
  const int vc[2] = {v0 + wave * 32 + i16, v0 + wave * 32 + 16 + i16};
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int tp = 0; tp < Ts; tp += KP) {
    __syncthreads();                                   // the panel before is done with
    for (int e = tid; e < RT * KP; e += 256) {         // transposed: 16 consecutive u of one frame per 16 threads
      const int r = e & (RT - 1), k = e / RT;
      Qp[r * WPS + k] = (tp + k < T && u0 + r < U1) ? q[(size_t)(tp + k) * U1 + u0 + r] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < KP; ks += 4) {
      const int t = tp + ks + kg;
      const float av = Qp[i16 * WPS + ks + kg];
      const float *er = EaS + (size_t)(t < T ? t : 0) * Vp;
#pragma unroll
      for (int c = 0; c < 2; c++) acc[c] = MFMA16(av, (t < T && vc[c] < Vp) ? er[vc[c]] : 0.f, acc[c]);
    }
  }
  const float *wbS = a.r.ws.wb + (size_t)s * T * U1, *wyS = a.r.ws.wy + (size_t)s * T * U1;
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int u = u0 + 4 * kg + j, v = vc[c];
      if (u >= U1 || v >= V) continue;
      float out = 0.f;
      if (u <= U) {
        double ind = 0.0;
        if (v == a.r.blank)
          for (int t = 0; t < Ts; t++) ind += (double)wbS[(size_t)t * U1 + u];
        else if (u < U && a.r.labels[me.w + u] == v)
          for (int t = 0; t < Ts; t++) ind += (double)wyS[(size_t)t * U1 + u];
        out = (float)((double)a.El[((size_t)s * U1 + u) * Vp + v] * (double)acc[c][j] - ind);
      }
      a.d_lm[((size_t)u * S + s) * a.dlm_stride + v] = out;
    }
}

// c(t) of the band rule for frame t of stream s into band[s][t]; streams the second kernel refuses are left alone here
__global__ __launch_bounds__(64) void k_rocc_center(const float *occ, const int *lens, const int *loff, int T, int U1, int R, int *band) {
  const int t = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const int Ts = lens[s], U = loff[s + 1] - loff[s];
  if (t >= Ts || Ts > T || U < 0 || U > U1 - 1) return;
  const int hi = max(0, U + 1 - R);
  const float *row = occ + ((size_t)s * T + t) * U1;
  double bw = -HUGE_VAL;
  int bk = -1;
  for (int k = lane; k <= hi; k += 64) {
    double w = 0.0;
    for (int r = 0; r < R && k + r <= U; r++) w += (double)row[k + r];
    if (w > bw) { bw = w; bk = k; }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double ow = __shfl_xor(bw, o);
    const int ok = __shfl_xor(bk, o);
    if (ok >= 0 && (bk < 0 || ow > bw || (ow == bw && ok < bk))) { bw = ow; bk = ok; }
  }
  if (lane == 0) band[(size_t)s * T + t] = max(bk, 0);
}

__global__ __launch_bounds__(256) void k_rocc_band(const int *lens, const int *loff, int T, int U1, int R, int *band) {
  __shared__ int sc[256];
  __shared__ int bad, carry;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int Ts = lens[s], U = loff[s + 1] - loff[s];
  int *row = band + (size_t)s * T;
  if (Ts <= 0 || Ts > T || U < 0 || U > U1 - 1) {
    for (int t = tid; t < T; t += 256) row[t] = Ts == 0 ? 0 : -1;
    return;
  }
  const int hi = max(0, U + 1 - R);
  if (tid == 0) { bad = 0; carry = 0; }
  for (int c0 = 0; c0 < Ts; c0 += 256) {               // m(t): the prefix maximum of c(t), c(0) = 0, c(T_s - 1) = hi
    const int t = c0 + tid;
    int g = 0;
    if (t < Ts) g = t == Ts - 1 ? hi : t == 0 ? 0 : row[t];
    __syncthreads();                                   // the chunk before is done with sc and carry
    sc[tid] = g;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] = max(sc[tid], v);
      __syncthreads();
    }
    g = max(sc[tid], carry);
    const int last = max(sc[255], carry);
    __syncthreads();
    if (tid == 0) carry = last;
    if (t < Ts) row[t] = g;                            // read again below by this very thread
  }
  __syncthreads();
  if (tid == 0) carry = INT_MIN;
  __syncthreads();
  band_close(row, Ts, T, R - 1, hi, [&](int t) { return row[t]; }, sc, &carry, &bad);
}

static bool simple_al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

static const char *simple_limits(int T, int S, int Umax, int V) {
  if (S < 1 || S > 32) return "1 <= S <= 32";
  if (T < 1) return "1 <= T";
  if (Umax < 0 || Umax > 1023) return "0 <= Umax <= 1023";
  if ((long long)T * (Umax + 1) * S > (1ll << 24)) return "T (Umax+1) S <= 2^24";
  if (V < 2 || V > 4096) return "2 <= V <= 4096";
  return nullptr;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_simple_workspace_bytes(int T, int S, int Umax, int V) {
  if (const char *why = simple_limits(T, S, Umax, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_simple_workspace_bytes: T %d, S %d, Umax %d, V %d: the limit is %s", T, S, Umax, V, why);
    return 0;
  }
  SimpleArgs a;
  size_t bytes = 0;
  simple_carve(nullptr, T, S, Umax + 1, V, &a, &bytes);
  return bytes;
}

klstm_status krnnt_simple_eval(const float *am, int am_stride, const float *lm, int lm_stride, int T, int S, int Umax, int V, const int *lens_dev,
                               const int *labels_dev, const int *label_offsets_dev, int blank, float *d_am, int d_am_stride, float *d_lm,
                               int d_lm_stride, float *occ_dev, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                               void *hip_stream) {
  if (const char *why = simple_limits(T, S, Umax, V))
    return fail(KLSTM_ERR_SHAPE, "krnnt_simple_eval: T %d, S %d, Umax %d, V %d: the limit is %s", T, S, Umax, V, why);
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_simple_eval: blank %d outside [0, %d)", blank, V);
  if (!am || !lm || !lens_dev || !labels_dev || !label_offsets_dev || !utt_loss_dev || !workspace)
    return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: null argument");
  const int ngrad = (d_am != nullptr) + (d_lm != nullptr);
  if (ngrad == 1) return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: the two gradient outputs are given together or not at all");
  if (am_stride < V || lm_stride < V || (ngrad && (d_am_stride < V || d_lm_stride < V)))
    return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: row stride below the width %d (%d, %d, %d, %d)", V, am_stride, lm_stride, d_am_stride, d_lm_stride);
  if (!simple_al4(am) || !simple_al4(lm) || !simple_al4(d_am) || !simple_al4(d_lm) || !simple_al4(occ_dev) || !simple_al4(utt_loss_dev) ||
      (reinterpret_cast<uintptr_t>(totals_dev) & 7))
    return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: misaligned pointer");
  SimpleArgs a;
  size_t need = 0;
  const int U1 = Umax + 1;
  simple_carve(workspace, T, S, U1, V, &a, &need);
  if (workspace_bytes < need) return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(KLSTM_ERR_ARG, "krnnt_simple_eval: the workspace is not 256-byte aligned");
  RnntArgs &r = a.r;
  r.enc = r.pred = r.W = r.b = nullptr; r.enc_stride = r.pred_stride = 0;
  r.T = T; r.S = S; r.U1 = U1; r.J = 0; r.V = V; r.blank = blank;
  r.lens = lens_dev; r.labels = labels_dev; r.loff = label_offsets_dev;
  r.d_enc = r.d_pred = r.Wg = r.bg = nullptr; r.de_stride = r.dp_stride = 0;
  r.utt_loss = utt_loss_dev; r.totals = totals_dev;
  r.splits = 0; r.ntb = (T + RT - 1) / RT;
  a.am = am; a.lm = lm; a.am_stride = am_stride; a.lm_stride = lm_stride;
  a.d_am = d_am; a.d_lm = d_lm; a.occ = occ_dev; a.dam_stride = d_am_stride; a.dlm_stride = d_lm_stride;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t N = (size_t)S * T * U1;
  HIPCHK(rnnt_launch_prep(r, st));
  HIPCHK(launch(k_rsimple_exp, dim3((unsigned)(S * T + S * U1)), dim3(256), 0, st, LaunchProbe(), a));
  HIPCHK(launch(k_rsimple_norm, dim3(r.ntb, (U1 + SU - 1) / SU, S), dim3(256), 0, st, LaunchProbe(), a));
  HIPCHK(rnnt_launch_lattice(r, st));
  if (!ngrad && !occ_dev) return KLSTM_OK;
  HIPCHK(launch(k_rsimple_occ, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, LaunchProbe(), a));
  if (!ngrad) return KLSTM_OK;
  const int nvb = (V + GV - 1) / GV;
  HIPCHK(launch(k_rsimple_dam, dim3(r.ntb, nvb, S), dim3(256), 0, st, LaunchProbe(), a));
  HIPCHK(launch(k_rsimple_dlm, dim3((U1 + RT - 1) / RT, nvb, S), dim3(256), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status krnnt_band_from_occupation(const float *occ_dev, const int *lens_dev, const int *label_offsets_dev, int T, int S, int Umax, int R,
                                        int *band_lo_dev, void *hip_stream) {
  if (const char *why = simple_limits(T, S, Umax, 2))
    return fail(KLSTM_ERR_SHAPE, "krnnt_band_from_occupation: T %d, S %d, Umax %d: the limit is %s", T, S, Umax, why);
  if (R < 1 || R > 64) return fail(KLSTM_ERR_SHAPE, "krnnt_band_from_occupation: R %d outside [1, 64]", R);
  if (!occ_dev || !lens_dev || !label_offsets_dev || !band_lo_dev) return fail(KLSTM_ERR_ARG, "krnnt_band_from_occupation: null argument");
  if (!simple_al4(occ_dev) || !simple_al4(lens_dev) || !simple_al4(label_offsets_dev) || !simple_al4(band_lo_dev))
    return fail(KLSTM_ERR_ARG, "krnnt_band_from_occupation: misaligned pointer");
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(launch(k_rocc_center, dim3(T, S), dim3(64), 0, st, LaunchProbe(), occ_dev, lens_dev, label_offsets_dev, T, Umax + 1, R, band_lo_dev));
  HIPCHK(launch(k_rocc_band, dim3(S), dim3(256), 0, st, LaunchProbe(), lens_dev, label_offsets_dev, T, Umax + 1, R, band_lo_dev));
  return KLSTM_OK;
}

}  // extern "C"
