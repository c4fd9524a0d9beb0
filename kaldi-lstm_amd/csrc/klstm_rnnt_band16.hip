// kaldi-lstm_amd/csrc/klstm_rnnt_band16.hip -- band-pruned transducer training with a bf16 joint: krnnt_band_eval_bf16 and its workspace
// size (include/klstm_rnnt.h, THE BF16 JOINT, states the three roundings; the torch yardstick: tests/rnnt_band_bf16_ref.py).
// The three joint products run on v_mfma_f32_16x16x32_bf16 (f32 accumulation): lane (i16, kg) supplies k = 8 kg .. 8 kg + 7 of row i16 of
// A and of column i16 of B, and holds C rows 4 kg + j of column i16 -- the C layout of the f32 instruction, so everything behind the
// products is the f32 kernels' code.  The lattice, the weights and the finish kernel are klstm_rnnt_band.hip's, launched through the
// helpers of klstm_rnnt_band_dev.h on the planes the kernels here write.
//   k_rband16_convert   Wb [V][Jp] = bf(W), Jp = J up to a multiple of 32 with zeros behind J: a k-panel of 32 is always whole.  With
//                       gradients also the transpose WbT [J][Vp], Vp = V up to a multiple of 32, zeros behind V: the B operand of
//                       dz = gb Wb has k = the classes, and a lane's 8 classes of one column are 16 contiguous bytes of WbT (in Wb they
//                       would be 8 halves gathered from 8 rows).
//   band16_joint_logits the sibling of band_joint_logits(): per k-panel, Zp [node][32] keeps enc + pred in f32 (row stride 36 floats:
//                       lane (i16, kg) reads its 8 floats as two 16-byte loads at dword 36 i16 + 8 kg (+ 4); over the 16 lanes of one
//                       kg the starts 36 i16 mod 64 are the 16 multiples of 4, so each load of a quarter wave touches every one of the
//                       64 banks once), hb = bf(tanh(.)) is formed in registers as the A operand, 8 values per lane.  Wp [class][32]
//                       is copied from Wb with 16-byte loads, row stride 40 halves = 80 bytes = 20 dwords: lane (i16, kg) reads 16
//                       bytes at dword 20 i16 + 4 kg, and 20 i16 mod 64 runs through the 16 multiples of 4 as well -- all 64 banks once
//                       per quarter wave, no conflict (the f32 stride of 34 would leave the 16-byte reads misaligned).  ONE matrix
//                       instruction per (M-tile, class tile, panel), accumulated in panel order: the same bits wherever it is called.
//   k_rband16_joint_fwd the sibling of k_rband_joint_fwd: the same unit of 16 frames x 8 band offsets, nodeU[], passes of 128 classes.
//   k_rband16_joint_bwd<NJ>  the sibling of k_rband_joint_bwd.  g of a pass goes to three LDS tiles: G [node][class] f32 (b_grad sums
//                       the unrounded g in double; the epilogue reuses the tile), Gn [node][class] bf16 (row stride 136 halves = 68
//                       dwords: the A operand of dz += gb WbT, K = the pass's classes in up to 4 instructions of 32; starts
//                       68 i16 + 4 kg mod 64 = 4 i16 + 4 kg: conflict-free) and Gc [class][node] bf16 (row stride 72 halves = 36
//                       dwords, the A operand of W_grad += gb^T hb, K = the 64 nodes in 2 instructions; starts 36 i16: conflict-free).
//                       hb of the W_grad product is formed in registers from encL + pred like the epilogue's h: the same f32 sum, the
//                       same k_tanh, the same rounding as in the logits.  The epilogue (dz (1 - h^2) with the unrounded h, the column
//                       owners, the windows) is the f32 kernel's.
// The bodies around the products repeat klstm_rnnt_band.hip's text instead of sharing functions with it: with the shared functions the
// f32 kernels came out with another register allocation, and their instructions are to stay what they were.
// BOUNDS: as in klstm_rnnt_band.hip (every node access through nodeU[], classes >= V masked at the panel load and in the epilogues).
// Wb is read at rows < V and columns < Jp, WbT at rows < J and columns < v0 + 32 ceil(nv / 32) <= Vp; Gn's columns up to that bound are
// written (zeros behind the last class) before they are read.
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_band_dev.h"

namespace klstm {

#define MFMA32B(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
constexpr int ZS = KP + 4, WS16 = KP + 8;   // floats per row of Zp, halves per row of Wp
constexpr int GNS = VP + 8, GCS = 64 + 8;   // halves per row of Gn [node][class] and of Gc [class][node]
typedef unsigned short bf16_t;              // storage; the arithmetic type is __bf16

struct Band16Args {
  BandArgs a;
  const bf16_t *Wb, *WbT;
  int Jp, Vp;
};

static inline size_t up32(size_t v) { return (v + 31) / 32 * 32; }

__device__ __forceinline__ bf16x8 bf8(const float4 &x, const float4 &y) {
  return bf16x8{(__bf16)x.x, (__bf16)x.y, (__bf16)x.z, (__bf16)x.w, (__bf16)y.x, (__bf16)y.y, (__bf16)y.z, (__bf16)y.w};
}

__global__ __launch_bounds__(256) void k_rband16_convert(const float *__restrict__ W, int V, int J, int Jp, int Vp, bf16_t *Wb, bf16_t *WbT) {
  const size_t n1 = (size_t)V * Jp, n2 = WbT ? (size_t)J * Vp : 0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n1 + n2; e += (size_t)gridDim.x * 256) {
    if (e < n1) {
      const int v = (int)(e / Jp), k = (int)(e - (size_t)v * Jp);
      Wb[e] = k < J ? __builtin_bit_cast(bf16_t, (__bf16)W[(size_t)v * J + k]) : (bf16_t)0;
    } else {
      const size_t i = e - n1;
      const int k = (int)(i / Vp), v = (int)(i - (size_t)k * Vp);
      WbT[i] = v < V ? __builtin_bit_cast(bf16_t, (__bf16)W[(size_t)v * J + k]) : (bf16_t)0;
    }
  }
}

// The logits (without bias) of the workgroup's 4 MT M-tiles, M-tile wave MT + m of the calling wave, against the classes
// v0 .. v0 + 16 nvt - 1; acc in the C layout.  Wp [VP][WS16] halves, Zp [64 MT][ZS] floats.  Called by all 256 threads together.
template <int MT>
__device__ __forceinline__ void band16_joint_logits(const float *__restrict__ enc, int enc_stride, const float *__restrict__ pred, int pred_stride,
                                                    int S, int s, int t0, const int *nodeU, const bf16_t *__restrict__ Wb, int Jp, int J, int V,
                                                    int v0, int nvt, bf16_t *Wp, float *Zp, f32x4 (&acc)[MT][NVT]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) acc[m][vt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kp = 0; kp < J; kp += KP) {
    const int kw = min(KP, J - kp);
    __syncthreads();                                   // the panel before is done with (and the caller's LDS stores are visible)
    for (int e = tid; e < nvt * 16 * 4; e += 256) {    // 16 bytes per thread: 8 k of a class row (Wb is zero behind J)
      const int v = e >> 2, c = e & 3;
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (v0 + v < V) w = *reinterpret_cast<const uint4 *>(Wb + (size_t)(v0 + v) * Jp + kp + 8 * c);
      *reinterpret_cast<uint4 *>(Wp + v * WS16 + 8 * c) = w;
    }
    for (int e = tid; e < 4 * MT * 16 * KP; e += 256) {
      const int node = e / KP, k = e - node * KP, u = nodeU[node];
      float z = 0.f;
      if (u >= 0 && k < kw)
        z = enc[((size_t)(t0 + (node & 15)) * S + s) * enc_stride + kp + k] + pred[((size_t)u * S + s) * pred_stride + kp + k];
      Zp[node * ZS + k] = z;
    }
    __syncthreads();
    bf16x8 hb[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const float4 *z = reinterpret_cast<const float4 *>(Zp + ((wave * MT + m) * 16 + i16) * ZS + 8 * kg);
      const float4 z0 = z[0], z1 = z[1];
      hb[m] = bf8(make_float4(k_tanh(z0.x), k_tanh(z0.y), k_tanh(z0.z), k_tanh(z0.w)),
                  make_float4(k_tanh(z1.x), k_tanh(z1.y), k_tanh(z1.z), k_tanh(z1.w)));
    }
#pragma unroll
    for (int vt = 0; vt < NVT; vt++)
      if (vt < nvt) {
        const bf16x8 bv = *reinterpret_cast<const bf16x8 *>(Wp + (vt * 16 + i16) * WS16 + 8 * kg);
#pragma unroll
        for (int m = 0; m < MT; m++) acc[m][vt] = MFMA32B(hb[m], bv, acc[m][vt]);
      }
  }
}

__global__ __launch_bounds__(256) void k_rband16_joint_fwd(Band16Args p) {
  __shared__ __attribute__((aligned(16))) bf16_t Wp[VP * WS16];
  __shared__ __attribute__((aligned(16))) float Zp[16 * BR * ZS];
  __shared__ int nodeU[16 * BR];
  const BandArgs &a = p.a;
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
    band16_joint_logits<2>(a.enc, a.enc_stride, a.pred, a.pred_stride, a.S, s, t0, nodeU, p.Wb, p.Jp, J, V, v0, nvt, Wp, Zp, acc);
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

// the dynamic LDS of k_rband16_joint_bwd in bytes: encL, Zp, G (floats), then Wp, Gn, Gc (halves, each a multiple of 16 bytes), nodeU
static size_t band16_bwd_lds(int J) {
  return ((size_t)RT * (J + 2) + 64 * ZS + 64 * BGS) * sizeof(float) + ((size_t)VP * WS16 + 64 * GNS + VP * GCS) * sizeof(bf16_t) + 64 * sizeof(int);
}

template <int NJ>
__global__ __launch_bounds__(256) void k_rband16_joint_bwd(Band16Args p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const BandArgs &a = p.a;
  const int J = a.J, V = a.V, Jp = J + 2, S = a.S, R = a.R;
  float *Zp = lds, *G = Zp + 64 * ZS, *encL = G + 64 * BGS;                      // Zp first: its rows are read 16 bytes at a time
  bf16_t *Wp = reinterpret_cast<bf16_t *>(encL + RT * Jp), *Gn = Wp + VP * WS16, *Gc = Gn + 64 * GNS;
  int *nodeU = reinterpret_cast<int *>(Gc + VP * GCS);
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
        const int nvt = (min(VP, V - v0) + 15) / 16, nv = nvt * 16, nq = (nvt + 1) / 2;      // nq: instructions of 32 classes
        f32x4 acc[1][NVT];
        band16_joint_logits<1>(a.enc, a.enc_stride, a.pred, a.pred_stride, S, s, t0, nodeU, p.Wb, p.Jp, J, V, v0, nvt, Wp, Zp, acc);
        // g in registers, then into the tiles: G and Gn by node, Gc by class (a lane's four nodes are 8 contiguous bytes of it);
        // class tile nvt of an odd nvt is written as zeros: the last instruction of 32 classes reads it
#pragma unroll
        for (int vt = 0; vt < NVT; vt++)
          if (vt < 2 * nq) {
            const int v = v0 + vt * 16 + i16;
            const float bias = v < V ? a.b[v] : 0.f;
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
              g[j] = 0.f;
              if (vt < nvt && nu[j] >= 0 && v < V) {
                g[j] = (wb[j] + wy[j]) * expf(acc[0][vt][j] + bias - lse[j]);
                if (v == a.blank) g[j] -= wb[j];
                if (v == lab[j]) g[j] -= wy[j];
              }
              G[(wave * 16 + 4 * kg + j) * BGS + vt * 16 + i16] = g[j];
              Gn[(wave * 16 + 4 * kg + j) * GNS + vt * 16 + i16] = __builtin_bit_cast(bf16_t, (__bf16)g[j]);
            }
            *reinterpret_cast<uint2 *>(Gc + (vt * 16 + i16) * GCS + wave * 16 + 4 * kg) = pack_bf16x4(make_float4(g[0], g[1], g[2], g[3]));
          }
        __syncthreads();
        // dz += gb Wb: K = the pass's classes, 32 per instruction; B from the transposed copy, 16 bytes per lane
        for (int q = 0; q < nq; q++) {
          const bf16x8 av = *reinterpret_cast<const bf16x8 *>(Gn + (wave * 16 + i16) * GNS + 32 * q + 8 * kg);
          const bf16_t *wr = p.WbT + (size_t)i16 * p.Vp + v0 + 32 * q + 8 * kg;
#pragma unroll
          for (int nt = 0; nt < NJ; nt++)
            if (nt * 16 < J) dz[nt] = MFMA32B(av, *reinterpret_cast<const bf16x8 *>(wr + (size_t)nt * 16 * p.Vp), dz[nt]);
        }
        // W_grad partial += gb^T hb: K = the workgroup's 64 nodes in two instructions; hb again as the B operand (a missing node has g = 0)
        for (int nt = wave; nt * 16 < J; nt += 4) {
          const int col = nt * 16 + i16;
          bf16x8 hb[2];
#pragma unroll
          for (int half = 0; half < 2; half++) {
            float h[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const int node = 32 * half + 8 * kg + e, un = max(nodeU[node], 0);
              h[e] = k_tanh(encL[(node & 15) * Jp + col] + a.pred[((size_t)un * S + s) * a.pred_stride + col]);
            }
            hb[half] = bf8(make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]));
          }
#pragma unroll 1
          for (int vt = 0; vt < nvt; vt++) {           // (not unrolled: the unrolled form holds all 16 A operands and spills dz)
              const bf16_t *gr = Gc + (vt * 16 + i16) * GCS + 8 * kg;
              f32x4 dw = MFMA32B(*reinterpret_cast<const bf16x8 *>(gr), hb[0], (f32x4{0.f, 0.f, 0.f, 0.f}));
              dw = MFMA32B(*reinterpret_cast<const bf16x8 *>(gr + 32), hb[1], dw);
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int v = v0 + vt * 16 + 4 * kg + j;
                if (v < V) wpart[(size_t)v * J + col] += dw[j];
              }
            }
        }
        if (tid < nv && v0 + tid < V) {                // b_grad: the unrounded g
          double sum = 0.0;
          for (int node = 0; node < 64; node++) sum += (double)G[node * BGS + tid];
          bpart[v0 + tid] += sum;
        }
      }
      // dz (1 - h^2) through the tile, 128 columns at a time, to the column owners (h unrounded: the rounding is straight-through)
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
                float *de = a.d_enc + ((size_t)(t0 + fr) * S + s) * a.de_stride + col;
                *de = rb == 0 ? sum : *de + sum;
              }
            }
          }
        }
    }
  }
}

// the W copies behind the banded workspace: Wb always, WbT with gradients
static size_t band16_extra(int J, int V, bool grads, size_t *wbt_off) {
  CtcCarver c(nullptr);
  c.take<bf16_t>((size_t)V * up32(J));
  *wbt_off = c.bytes();
  if (grads) c.take<bf16_t>((size_t)J * up32(V));
  return c.bytes();
}

size_t band16_wb_bytes(int J, int V) {
  size_t off = 0;
  band16_extra(J, V, false, &off);
  return off;
}

hipError_t band16_launch_joint_fwd(const BandArgs &a, void *wb, hipStream_t st) {
  Band16Args p;
  p.a = a; p.Wb = static_cast<const bf16_t *>(wb); p.WbT = nullptr; p.Jp = (int)up32(a.J); p.Vp = (int)up32(a.V);
  const size_t ncv = (size_t)a.V * p.Jp, gcv = (ncv + 255) / 256;
  const hipError_t e = launch(k_rband16_convert, dim3((unsigned)(gcv < 4096 ? gcv : 4096)), dim3(256), 0, st, LaunchProbe(), a.W, a.V, a.J, p.Jp, p.Vp,
                              static_cast<bf16_t *>(wb), (bf16_t *)nullptr);
  return e != hipSuccess ? e : launch(k_rband16_joint_fwd, dim3(a.ntb, (a.R + BR - 1) / BR, a.S), dim3(256), 0, st, LaunchProbe(), p);
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_band_bf16_workspace_bytes(int T, int S, int Umax, int R, int J, int V, int want_grads) {
  if (const char *why = band_limits(T, S, Umax, R, J, V)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_band_bf16_workspace_bytes: T %d, S %d, Umax %d, R %d, J %d, V %d: the limit is %s", T, S, Umax, R, J, V, why);
    return 0;
  }
  size_t bytes = 0, off = 0;
  if (want_grads) band_carve(nullptr, T, S, Umax + 1, R, J, V, true, &bytes);
  else band_carve(nullptr, T, S, 1, R, 16, 2, false, &bytes);
  return bytes + band16_extra(J, V, want_grads != 0, &off);
}

klstm_status krnnt_band_eval_bf16(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                                  int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                                  int R, const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                                  float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                                  void *hip_stream) {
  const bool grads = d_enc && d_pred && W_grad && b_grad;
  Band16Args p;
  int ngrad = 0;
  size_t band_bytes = 0, wbt_off = 0;
  const size_t extra = (J >= 16 && J <= 1024 && V >= 2 && V <= 4096) ? band16_extra(J, V, grads, &wbt_off) : 0;
  const klstm_status bad = band_eval_args("krnnt_band_eval_bf16", enc, enc_stride, pred, pred_stride, W, b, T, S, Umax, J, V, lens_dev, labels_dev,
                                          label_offsets_dev, blank, R, band_lo_dev, d_enc, d_enc_stride, d_pred, d_pred_stride, W_grad, b_grad,
                                          utt_loss_dev, totals_dev, workspace, workspace_bytes, extra, &p.a, &ngrad, &band_bytes);
  if (bad != KLSTM_OK) return bad;
  const BandArgs &a = p.a;
  bf16_t *Wb = reinterpret_cast<bf16_t *>(static_cast<char *>(workspace) + band_bytes);
  bf16_t *WbT = ngrad ? reinterpret_cast<bf16_t *>(static_cast<char *>(workspace) + band_bytes + wbt_off) : nullptr;
  p.Wb = Wb; p.WbT = WbT; p.Jp = (int)up32(J); p.Vp = (int)up32(V);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t ncv = (size_t)V * p.Jp + (ngrad ? (size_t)J * p.Vp : 0), gcv = (ncv + 255) / 256;
  HIPCHK(launch(k_rband16_convert, dim3((unsigned)(gcv < 4096 ? gcv : 4096)), dim3(256), 0, st, LaunchProbe(), W, V, J, p.Jp, p.Vp, Wb, WbT));
  HIPCHK(band_launch_prep(a, st));
  HIPCHK(launch(k_rband16_joint_fwd, dim3(a.ntb, (R + BR - 1) / BR, S), dim3(256), 0, st, LaunchProbe(), p));
  HIPCHK(band_launch_lattice(a, st));
  if (!ngrad) return KLSTM_OK;
  const size_t shm = band16_bwd_lds(J);
  if (J <= 128) HIPCHK(launch(k_rband16_joint_bwd<8>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), p));
  else if (J <= 512) HIPCHK(launch(k_rband16_joint_bwd<32>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), p));
  else HIPCHK(launch(k_rband16_joint_bwd<64>, dim3(a.splits), dim3(256), shm, st, LaunchProbe(), p));
  HIPCHK(band_launch_finish(a, st));
  return KLSTM_OK;
}

}  // extern "C"
