// kaldi-lstm_amd/csrc/klstm_rnnt_align.hip -- transducer forced alignment: krnnt_align (the full lattice), krnnt_band_align (a band, f32 or
// bf16 joint) and their workspace sizes (include/klstm_rnnt.h, FORCED ALIGNMENT, states every quantity; the torch
// yardstick: tests/rnnt_align_ref.py).  lpb / lpy of every node come from the training entries' own forward kernels, launched unchanged
// through the helpers of klstm_rnnt_dev.h / klstm_rnnt_band_dev.h on a workspace that holds nothing but meta and the three planes.  What
// is new is the max-plus lattice with its decisions and the backtrace, one launch per call:
//   k_rnnt_viterbi   one workgroup per stream, one thread per u, along the anti-diagonals d = t + u: the previous diagonal double-buffered
//                    in LDS as doubles, lpb / lpy of the next four diagonals in registers (the walk of rnnt_lattice_run), one barrier per
//                    diagonal (a wave fence when the workgroup is one wave).  No normalisation: v is a sum of at most T + U floats.
//                    THE DECISIONS ARE BITS: a wave's ballot of "the label step won" is one 64-bit word per (diagonal, wave), stored by
//                    lane 0; bit u of diagonal d is the decision at node (d - u, u).  8 (T_s + U) nw bytes per stream where a byte plane
//                    would take T_s (U + 1).  The words stay in LDS behind the two rows when 8 (T + Umax + 1) nw bytes fit what is left
//                    of 64 KiB (the host decides from T and Umax alone); otherwise they go to the workspace and are read back from there.
//                    Tail of the same launch: the workgroup that wrote the words reads them, so the last barrier is all the ordering it
//                    needs; thread 0 walks the T_s + U decisions from (T_s - 1, U) and writes f_u = t, logp_u = lpy(t, u - 1) at every
//                    label step.  With one wave the word of the next step is diagonal d - 1 whatever the decision, and is loaded ahead.
//   k_rband_viterbi  one wave per stream, lane = band offset: the register walk of band_lattice_run<0> (the lane's own frame pointer, u0
//                    of its next eight frames and lpb / lpy of its next four queued in registers), the blank predecessor by __shfl from
//                    lane r + u0(t) - u0(t-1), the label predecessor from lane r - 1, max and `>` in place of logadd.  One ballot word per
//                    diagonal: bit r is the node of that diagonal at band offset r.  The words and the stream's u0 row are staged in LDS
//                    when 8 (T + Umax + 1) + 4 T bytes fit 64 KiB.  Tail, lane 0: at (t, r) bit r of word t + u0(t) + r set: to (t, r - 1)
//                    with f and logp written; otherwise to (t - 1, r + u0(t) - u0(t-1)).  Every step goes one diagonal down, so the next
//                    word never depends on the decision and is loaded ahead; u0 of the two frames before t is kept in registers.
// BOUNDS.  Nodes are touched only under t < T_s, u <= U_s (and r < R, u0(t) + r <= U_s in the band); plane offsets are size_t products;
// a word index is d nw + w with d < T_s + U_s <= T + Umax and w < nw: inside the LDS staging (T + Umax + 1) nw and inside the stream's
// part of the workspace.  A valid band is connected, so the backtrace cannot leave the lattice; the walk is guarded by t >= 0, u >= 0
// (0 <= r < R) all the same, and an output index is written only inside [0, U_s): a corrupted word ends the walk.
// No atomics: runs are bit-identical and a stream's result does not depend on its company.
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_band_dev.h"

namespace klstm {

typedef unsigned long long bpw_t;           // the decisions of one wave on one diagonal
constexpr int AL_ROW = 1024 + 2;            // doubles per LDS row of k_rnnt_viterbi
constexpr size_t AL_LDS = 64 * 1024;        // the LDS of a workgroup of either kernel never passes the default limit

struct AlignOut {
  int *frames; float *logp, *score;
  bpw_t *bp;
  int lds_words;                            // words per stream staged in LDS; 0: they go through bp
};
struct RnntAlignArgs { RnntArgs a; AlignOut o; };
struct BandAlignArgs { BandArgs a; AlignOut o; };

struct AlignWs {
  int4 *meta; float *lpb, *lpy, *lse;
  bpw_t *bp; void *wb;
};

// the layout of both workspaces (include/klstm_rnnt.h states the formulas); base null: only *bytes counts
static AlignWs align_carve(void *base, size_t S, size_t nodes, size_t words, size_t wb_bytes, size_t *bytes) {
  CtcCarver c(base);
  AlignWs w;
  w.meta = c.take<int4>(S);
  w.lpb = c.take<float>(nodes); w.lpy = c.take<float>(nodes); w.lse = c.take<float>(nodes);
  w.bp = c.take<bpw_t>(words);
  w.wb = wb_bytes ? c.take<char>(wb_bytes) : nullptr;
  *bytes = c.bytes();
  return w;
}

__global__ __launch_bounds__(1024) void k_rnnt_viterbi(RnntAlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) double al_lds[];
  const RnntArgs &a = p.a;
  const int s = blockIdx.x, u = threadIdx.x;
  const int4 me = a.ws.meta[s];
  if (me.x != 1) {
    if (u == 0) p.o.score[s] = 0.f;
    return;
  }
  const int Ts = me.y, U = me.z, U1 = a.U1, lane = u & 63, wave = u >> 6, nw = blockDim.x >> 6, nd = Ts + U;
  double(*row)[AL_ROW] = reinterpret_cast<double(*)[AL_ROW]>(al_lds);
  const bool staged = p.o.lds_words > 0, one = nw == 1;
  bpw_t *ldsw = reinterpret_cast<bpw_t *>(al_lds + 2 * AL_ROW), *gw = p.o.bp + (size_t)s * (a.T + U1) * nw;
  const size_t base = (size_t)s * a.T * U1;
  const float *lpb = a.ws.lpb + base, *lpy = a.ws.lpy + base;
  for (int e = u; e < 2 * AL_ROW; e += blockDim.x) (&row[0][0])[e] = (double)RLOG0;
  if (one) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
  // what diagonal e needs of thread u: lpb(t-1, u), lpy(t, u-1), t = e - u
  auto fetch = [&](int e, float &fb, float &fy) {
    fb = 0.f; fy = 0.f;
    const int t = e - u;
    if (e >= nd || u > U || t < 0 || t >= Ts) return;
    if (t > 0) fb = lpb[(size_t)(t - 1) * U1 + u];
    if (u > 0) fy = lpy[(size_t)t * U1 + u - 1];
  };
  float cb[4], cy[4], nb[4], ny[4];
#pragma unroll
  for (int i = 0; i < 4; i++) fetch(i, cb[i], cy[i]);
  for (int e0 = 0; e0 < nd; e0 += 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) fetch(e0 + 4 + i, nb[i], ny[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int e = e0 + i;
      if (e < nd) {
        const int t = e - u, cur = e & 1, prv = cur ^ 1;
        double val = (double)RLOG0;
        bool take = false;
        if (u <= U && t >= 0 && t < Ts) {
          if (e == 0) val = 0.0;
          else {
            const double x1 = t > 0 ? row[prv][u + 1] + cb[i] : (double)RLOG0, x2 = u > 0 ? row[prv][u] + cy[i] : (double)RLOG0;
            take = x2 > x1 && x2 > -1e29;                // `>`: a tie takes the blank step; log 0 never wins
            val = take ? x2 : x1;
            if (val < -1e29) val = (double)RLOG0;
          }
          if (e == nd - 1 && u == U) p.o.score[s] = (float)(val + (double)lpb[(size_t)(Ts - 1) * U1 + U]);
        }
        row[cur][u + 1] = val;
        const bpw_t w = __ballot(take);
        if (lane == 0) {
          if (staged) ldsw[e * nw + wave] = w;
          else gw[(size_t)e * nw + wave] = w;
        }
        if (one) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } else __syncthreads();
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { cb[i] = nb[i]; cy[i] = ny[i]; }
  }
  // the backtrace: the barrier of the last diagonal ordered every word before this thread
  if (u != 0) return;
  auto word = [&](int d, int w) { return staged ? ldsw[d * nw + w] : gw[(size_t)d * nw + w]; };
  int t = Ts - 1, uu = U, d = nd - 1;
  bpw_t w = word(d, uu >> 6);
  while (d > 0 && t >= 0 && uu >= 0) {
    const bpw_t wn = one ? word(d - 1, 0) : 0;           // one wave: the next word whatever the decision
    if ((w >> (uu & 63)) & 1) {
      if (uu == 0) break;
      uu--;
      p.o.frames[me.w + uu] = t;
      if (p.o.logp) p.o.logp[me.w + uu] = lpy[(size_t)t * U1 + uu];
    } else if (--t < 0) break;
    d--;
    w = one ? wn : word(d, uu >> 6);
  }
}

__global__ __launch_bounds__(64) void k_rband_viterbi(BandAlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) bpw_t bl_lds[];
  constexpr int QU = 9, QD = 4;                          // q[i] = u0(t + i - 1): the row before, the lane's row, seven rows ahead
  const BandArgs &a = p.a;
  const int s = blockIdx.x, r = threadIdx.x;
  const int4 me = a.ws.meta[s];
  if (me.x != 1) {
    if (r == 0) p.o.score[s] = 0.f;
    return;
  }
  const int Ts = me.y, U = me.z, R = a.R, nd = Ts + U;
  const int *u0 = a.band + (size_t)s * a.T;
  const size_t base = (size_t)s * a.T * R;
  const float *lpb = a.ws.lpb + base, *lpy = a.ws.lpy + base;
  const bool staged = p.o.lds_words > 0;
  bpw_t *ldsw = bl_lds, *gw = p.o.bp + (size_t)s * a.L;
  int *ldsu = reinterpret_cast<int *>(bl_lds + p.o.lds_words);
  if (staged)
    for (int t = r; t < Ts; t += 64) ldsu[t] = u0[t];
  auto band_at = [&](int t) { return u0[min(max(t, 0), Ts - 1)]; };
  // what row tt gives lane r: lpb(tt-1, u), lpy(tt, u-1), u = ucur + r
  auto fetch = [&](int tt, int uprev, int ucur, float &fb, float &fy) {
    fb = 0.f; fy = 0.f;
    if (r >= R || tt < 0 || tt >= Ts || ucur + r > U) return;
    const int src = r + ucur - uprev;
    if (tt > 0 && src < R) fb = lpb[(size_t)(tt - 1) * R + src];
    if (r > 0) fy = lpy[(size_t)tt * R + r - 1];
  };
  int t = 0, q[QU];
#pragma unroll
  for (int i = 0; i < QU; i++) q[i] = band_at(t + i - 1);
  float cb[QD], cy[QD];
#pragma unroll
  for (int i = 0; i < QD; i++) fetch(t + i, q[i], q[i + 1], cb[i], cy[i]);
  double prev = (double)RLOG0;
  for (int e = 0; e < nd; e++) {
    const int key = t + q[1] + r, u = q[1] + r;
    const bool hit = r < R && t < Ts && key == e;        // key >= e always: the pointer moves on a hit
    const int src = r + q[1] - q[0];                     // the lane that holds (t-1, u): the row shift u0(t) - u0(t-1) in the lane index
    const double pblank = __shfl(prev, min(src, 63));
    const double plabel = __shfl(prev, max(r - 1, 0));
    double val = (double)RLOG0;
    bool take = false;
    if (hit && u <= U) {
      if (e == 0) val = 0.0;
      else {
        const double x1 = (t > 0 && src < R) ? pblank + cb[0] : (double)RLOG0, x2 = r > 0 ? plabel + cy[0] : (double)RLOG0;
        take = x2 > x1 && x2 > -1e29;
        val = take ? x2 : x1;
        if (val < -1e29) val = (double)RLOG0;
      }
      if (e == nd - 1) p.o.score[s] = (float)(val + (double)lpb[(size_t)t * R + r]);       // node (T_s - 1, U)
    }
    const bpw_t w = __ballot(take);
    if (r == 0) {
      if (staged) ldsw[e] = w;
      else gw[e] = w;
    }
    if (hit) {
      t++;
#pragma unroll
      for (int i = 0; i + 1 < QU; i++) q[i] = q[i + 1];
      q[QU - 1] = band_at(t + QU - 2);
#pragma unroll
      for (int i = 0; i + 1 < QD; i++) { cb[i] = cb[i + 1]; cy[i] = cy[i + 1]; }
      fetch(t + QD - 1, q[QD - 1], q[QD], cb[QD - 1], cy[QD - 1]);
    }
    prev = val;
  }
  __syncthreads();                                       // one wave: the staged u0 row of all lanes before lane 0 reads it
  if (r != 0) return;
  auto word = [&](int d) { return staged ? ldsw[d] : gw[d]; };
  auto lo = [&](int tt) { return tt < 0 ? 0 : staged ? ldsu[tt] : u0[tt]; };
  int tb = Ts - 1, c0 = lo(tb), c1 = lo(tb - 1), c2 = lo(tb - 2), rr = U - c0, d = nd - 1;
  bpw_t w = word(d);
  while (d > 0 && tb >= 0 && rr >= 0 && rr < R) {
    const bpw_t wn = word(d - 1);                        // every step goes one diagonal down
    if ((w >> rr) & 1) {
      const int i = c0 + --rr;                           // the label y_{i+1}, entered at (tb, i + 1)
      if (rr < 0 || i < 0 || i >= U) break;
      p.o.frames[me.w + i] = tb;
      if (p.o.logp) p.o.logp[me.w + i] = lpy[(size_t)tb * R + rr];
    } else {
      if (--tb < 0) break;
      rr += c0 - c1;
      c0 = c1; c1 = c2; c2 = lo(tb - 2);
    }
    d--;
    w = wn;
  }
}

static bool align_al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the argument checks both entries share, behind their limits; no HIP call
static klstm_status align_args(const char *name, const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b,
                               int J, int V, const int *lens, const int *labels, const int *loff, int blank, bool banded, const int *band,
                               const int *frames, const float *logp, const float *score, const void *workspace, size_t workspace_bytes, size_t need) {
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "%s: blank %d outside [0, %d)", name, blank, V);
  if (!enc || !pred || !W || !b || !lens || !labels || !loff || (banded && !band) || !frames || !score || !workspace)
    return fail(KLSTM_ERR_ARG, "%s: null argument", name);
  if (enc_stride < J || pred_stride < J) return fail(KLSTM_ERR_ARG, "%s: row stride below the width %d (%d, %d)", name, J, enc_stride, pred_stride);
  if (!align_al4(enc) || !align_al4(pred) || !align_al4(W) || !align_al4(b) || !align_al4(lens) || !align_al4(labels) || !align_al4(loff) ||
      !align_al4(band) || !align_al4(frames) || !align_al4(logp) || !align_al4(score))
    return fail(KLSTM_ERR_ARG, "%s: misaligned pointer", name);
  if (workspace_bytes < need) return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, need);
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(KLSTM_ERR_ARG, "%s: the workspace is not 256-byte aligned", name);
  return KLSTM_OK;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_align_workspace_bytes(int T, int S, int Umax) {
  if (const char *why = rnnt_limits(T, S, Umax, 16, 2)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_align_workspace_bytes: T %d, S %d, Umax %d: the limit is %s", T, S, Umax, why);
    return 0;
  }
  size_t bytes = 0;
  align_carve(nullptr, S, (size_t)S * T * (Umax + 1), (size_t)S * (T + Umax + 1) * ((Umax + 64) / 64), 0, &bytes);
  return bytes;
}

klstm_status krnnt_align(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                         int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                         int *label_frames_dev, float *label_logp_dev, float *score_dev, void *workspace, size_t workspace_bytes,
                         void *hip_stream) {
  if (const char *why = rnnt_limits(T, S, Umax, J, V))
    return fail(KLSTM_ERR_SHAPE, "krnnt_align: T %d, S %d, Umax %d, J %d, V %d: the limit is %s", T, S, Umax, J, V, why);
  const int U1 = Umax + 1, nw = (U1 + 63) / 64;
  size_t need = 0;
  const AlignWs ws = align_carve(workspace, S, (size_t)S * T * U1, (size_t)S * (T + U1) * nw, 0, &need);
  const klstm_status bad = align_args("krnnt_align", enc, enc_stride, pred, pred_stride, W, b, J, V, lens_dev, labels_dev, label_offsets_dev, blank,
                                      false, nullptr, label_frames_dev, label_logp_dev, score_dev, workspace, workspace_bytes, need);
  if (bad != KLSTM_OK) return bad;
  RnntAlignArgs p = {};
  RnntArgs &a = p.a;
  a.enc = enc; a.pred = pred; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.U1 = U1; a.J = J; a.V = V; a.blank = blank;
  a.lens = lens_dev; a.labels = labels_dev; a.loff = label_offsets_dev;
  a.ws.meta = ws.meta; a.ws.lpb = ws.lpb; a.ws.lpy = ws.lpy; a.ws.lse = ws.lse;        // no alpha / beta / weight planes, no partials
  a.ntb = (T + RT - 1) / RT;
  const size_t rows = (size_t)2 * AL_ROW * sizeof(double), words = (size_t)(T + U1) * nw;
  p.o.frames = label_frames_dev; p.o.logp = label_logp_dev; p.o.score = score_dev; p.o.bp = ws.bp;
  p.o.lds_words = rows + words * sizeof(bpw_t) <= AL_LDS ? (int)words : 0;
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(rnnt_launch_prep(a, st));
  HIPCHK(rnnt_launch_joint_fwd(a, st));
  HIPCHK(launch(k_rnnt_viterbi, dim3(S), dim3(nw * 64), rows + (size_t)p.o.lds_words * sizeof(bpw_t), st, LaunchProbe(), p));
  return KLSTM_OK;
}

size_t krnnt_band_align_workspace_bytes(int T, int S, int R, int J, int V, int bf16) {
  if (const char *why = band_limits(T, S, 0, R, J, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_band_align_workspace_bytes: T %d, S %d, R %d, J %d, V %d: the limit is %s", T, S, R, J, V, why);
    return 0;
  }
  size_t bytes = 0;
  align_carve(nullptr, S, (size_t)S * T * R, (size_t)S * (T + OFFS_U), bf16 ? band16_wb_bytes(J, V) : 0, &bytes);
  return bytes;
}

klstm_status krnnt_band_align(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                              int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank, int R,
                              const int *band_lo_dev, int bf16, int *label_frames_dev, float *label_logp_dev, float *score_dev, void *workspace,
                              size_t workspace_bytes, void *hip_stream) {
  if (const char *why = band_limits(T, S, Umax, R, J, V))
    return fail(KLSTM_ERR_SHAPE, "krnnt_band_align: T %d, S %d, Umax %d, R %d, J %d, V %d: the limit is %s", T, S, Umax, R, J, V, why);
  size_t need = 0;
  const AlignWs ws = align_carve(workspace, S, (size_t)S * T * R, (size_t)S * (T + OFFS_U), bf16 ? band16_wb_bytes(J, V) : 0, &need);
  const klstm_status bad = align_args("krnnt_band_align", enc, enc_stride, pred, pred_stride, W, b, J, V, lens_dev, labels_dev, label_offsets_dev,
                                      blank, true, band_lo_dev, label_frames_dev, label_logp_dev, score_dev, workspace, workspace_bytes, need);
  if (bad != KLSTM_OK) return bad;
  BandAlignArgs p = {};
  BandArgs &a = p.a;
  a.enc = enc; a.pred = pred; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.U1 = Umax + 1; a.J = J; a.V = V; a.blank = blank; a.R = R;
  a.lens = lens_dev; a.labels = labels_dev; a.loff = label_offsets_dev; a.band = band_lo_dev;
  a.ws.meta = ws.meta; a.ws.lpb = ws.lpb; a.ws.lpy = ws.lpy; a.ws.lse = ws.lse;
  a.ntb = (T + RT - 1) / RT; a.L = T + OFFS_U;
  const size_t words = (size_t)T + a.U1, lds = words * sizeof(bpw_t) + (size_t)T * sizeof(int);
  p.o.frames = label_frames_dev; p.o.logp = label_logp_dev; p.o.score = score_dev; p.o.bp = ws.bp;
  p.o.lds_words = lds <= AL_LDS ? (int)words : 0;
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(band_launch_prep(a, st));
  if (bf16) HIPCHK(band16_launch_joint_fwd(a, ws.wb, st));
  else HIPCHK(band_launch_joint_fwd(a, st));
  HIPCHK(launch(k_rband_viterbi, dim3(S), dim3(64), p.o.lds_words ? lds : 0, st, LaunchProbe(), p));
  return KLSTM_OK;
}

}  // extern "C"
