// kaldi-lstm_amd/csrc/klstm_rnnt_dev.h -- device code shared by the transducer sources (klstm_rnnt.hip: training; klstm_rnnt_decode.hip:
// greedy decoding): the tile constants, the staging of rows into LDS, the 16-lane reductions of a node's row and joint_logits(), the
// product W tanh(enc[t] + pred[u]) of M-tiles of 16 nodes in MFMA registers (klstm_rnnt.hip's head describes its layout).  Both sources
// are compiled with the same flags (build.py EXTRA_FLAGS), so the logits of a node are the same bits in training and in decoding.
// Also here: the argument and workspace types of klstm_rnnt.hip's kernels with the host helpers that launch its prep, lattice and
// weights kernels (klstm_rnnt_simple.hip runs them on its own lpb / lpy), and band_close(), the scan both band builders end with.
#pragma once
#include <climits>

#include "../../include/klstm_rnnt.h"
#include "klstm_kernels.h"
#include "klstm_math.h"

namespace klstm {

constexpr int RT = KRNNT_TILE_T, VP = KRNNT_PASS_V, NVT = VP / 16;
constexpr int KP = 32, WPS = KP + 2;        // k per W panel, floats per panel row
constexpr float RLOG0 = -1e30f;

// The workspace and the arguments of klstm_rnnt.hip's kernels.  klstm_rnnt_simple.hip fills lpb / lpy itself and runs the same prep,
// lattice and weights kernels on these planes through the two host helpers below (defined in klstm_rnnt.hip).
struct RnntWs {
  int4 *meta; double *loss, *offs;
  float *lpb, *lpy, *lse, *A, *B, *wb, *wy, *dep, *dpp, *wpart;
  double *bpart;
};

struct RnntArgs {
  const float *enc, *pred, *W, *b;
  int enc_stride, pred_stride, T, S, U1, J, V, blank;
  const int *lens, *labels, *loff;
  float *d_enc, *d_pred, *Wg, *bg;
  int de_stride, dp_stride;
  float *utt_loss; double *totals;
  RnntWs ws;
  int splits, ntb;
};

// the layout of krnnt_eval's workspace; base null: only *bytes counts
RnntWs rnnt_carve(void *base, int T, int S, int U1, int J, int V, bool grads, size_t *bytes);
// k_rnnt_prep (status, T_s, U_s, label offset of every stream into ws.meta), and, once lpb / lpy of every node under t < T_s, u <= U_s
// are written, k_rnnt_lattice + k_rnnt_weights (alpha, beta, the loss, w_b, w_y, the totals).  They read T, S, U1, V, blank, lens,
// labels, loff, utt_loss, totals and ws of a.
hipError_t rnnt_launch_prep(const RnntArgs &a, hipStream_t st);
// k_rnnt_joint_fwd: lpb, lpy, lse of every node under t < T_s, u <= U_s from enc, pred, W, b (krnnt_align runs it on a workspace that
// holds nothing but meta and these three planes)
hipError_t rnnt_launch_joint_fwd(const RnntArgs &a, hipStream_t st);
hipError_t rnnt_launch_lattice(const RnntArgs &a, hipStream_t st);

const char *rnnt_limits(int T, int S, int Umax, int J, int V);                  // the limit of krnnt_eval that is broken, or null

// The end of a band builder (krnnt_band_from_frames, krnnt_band_from_occupation; 256 threads, one workgroup per stream).  cand(t) is
// u0(t) before the closure, with cand(T_s - 1) = hi.  From the end u0(t) = max(cand(t), u0(t+1) - R1): the suffix maximum of
// cand(t) - t R1 in chunks of 256 frames (an LDS scan per chunk and a carry).  Then the row: u0 for t < T_s and hi behind it, or -1
// everywhere if *bad is set or u0(0) > 0.  sc [256], carry: LDS; *carry = INT_MIN and *bad are set and fenced by the caller.
template <class F>
__device__ __forceinline__ void band_close(int *row, int Ts, int T, int R1, int hi, F cand, int *sc, int *carry, const int *bad) {
  const int tid = threadIdx.x;
  for (int c0 = (Ts - 1) / 256 * 256; c0 >= 0; c0 -= 256) {
    const int t = c0 + tid;
    int g = INT_MIN;
    if (t < Ts) g = cand(t) - t * R1;
    __syncthreads();                                   // the chunk before is done with sc and carry
    sc[tid] = g;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                // suffix maximum of the chunk
      const int v = tid + o < 256 ? sc[tid + o] : INT_MIN;
      __syncthreads();
      sc[tid] = max(sc[tid], v);
      __syncthreads();
    }
    g = max(sc[tid], *carry);
    __syncthreads();
    if (tid == 0) *carry = g;
    if (t < Ts) row[t] = g + t * R1;
  }
  __syncthreads();
  const bool infeasible = *bad || *carry != 0;         // carry = u0(0) after the last step
  for (int t = infeasible ? tid : Ts + tid; t < T; t += 256) row[t] = infeasible ? -1 : hi;
}

// rows row0 .. row0 + nrows - 1 of stream s (row r of the matrix: (row0 + r) S + s) into dst [nrows][Jp]; rows from nvalid on: zeros
__device__ __forceinline__ void rnnt_stage(float *dst, int Jp, const float *src, int stride, int row0, int nrows, int nvalid, int S, int s, int J) {
  for (int e = threadIdx.x; e < nrows * J; e += blockDim.x) {
    const int r = e / J, c = e - r * J;
    dst[r * Jp + c] = r < nvalid ? src[((size_t)(row0 + r) * S + s) * stride + c] : 0.f;
  }
}

__device__ __forceinline__ float red16_max(float x) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float red16_sum(float x) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) x += __shfl_xor(x, o);
  return x;
}

// The logits (without bias) of MT M-tiles of 16 nodes against the classes v0 .. v0 + 16 nvt - 1: acc[m][vt] in the C layout (row 4 kg + j,
// class 16 vt + i16).  encL [16][Jp]: the M-tiles' enc rows; pl[m]: the pred row of M-tile m.  Called by all 256 threads together.
template <int MT>
__device__ __forceinline__ void joint_logits(const float *encL, int Jp, const float *const (&pl)[MT], const float *__restrict__ W, int J, int V,
                                             int v0, int nvt, float *Wp, f32x4 (&acc)[MT][NVT]) {
  const int tid = threadIdx.x, lane = tid & 63, i16 = lane & 15, kg = lane >> 4;
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
    __syncthreads();
    f32x4 part[MT][NVT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) part[m][vt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < kw; ks += 4) {
      const int k = kp + ks + kg;
      float h[MT];
#pragma unroll
      for (int m = 0; m < MT; m++) h[m] = k_tanh(encL[i16 * Jp + k] + pl[m][k]);
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

}  // namespace klstm
