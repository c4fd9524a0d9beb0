// kaldi-lstm_amd/csrc/klstm_rnnt_band_dev.h -- what the two band-pruned training sources share (klstm_rnnt_band.hip: the f32 joint and
// the kernels around it; klstm_rnnt_band16.hip: the bf16 joint): the tile constants, the workspace and argument types, the node table
// of a tile and the host helpers.  Those are defined in klstm_rnnt_band.hip: the argument checks of both entries, and the launches of
// its prep, lattice, weights and finish kernels, which the bf16 entry runs unchanged on the planes its own joint wrote.
#pragma once
#include "klstm_ctc_host.h"
#include "klstm_host.h"
#include "klstm_rnnt_dev.h"

namespace klstm {

constexpr int BR = KRNNT_BAND_TILE_R;       // band offsets of a forward tile (RT, VP, NVT, KP, WPS and RLOG0: klstm_rnnt_dev.h)
constexpr int BBU = 4, BGS = VP + 2;        // offsets per backward step (one per wave), floats per row of the g tile
constexpr int OFFS_U = 1024;                // the offsets are sized for Umax = 1023: the forward workspace does not depend on Umax

struct BandWs {
  int4 *meta; double *loss, *offs;
  float *lpb, *lpy, *lse, *A, *B, *wb, *wy, *dpp, *wpart;
  double *bpart;
};

struct BandArgs {
  const float *enc, *pred, *W, *b;
  int enc_stride, pred_stride, T, S, U1, J, V, blank, R;
  const int *lens, *labels, *loff, *band;
  float *d_enc, *d_pred, *Wg, *bg;
  int de_stride, dp_stride;
  float *utt_loss; double *totals;
  BandWs ws;
  int splits, ntb, prow, L;                 // prow: window rows per stream, L: offsets per (stream, direction)
};

// the layout of krnnt_band_eval's workspace (include/klstm_rnnt.h states the formula); base null: only *bytes counts
BandWs band_carve(void *base, int T, int S, int U1, int R, int J, int V, bool grads, size_t *bytes);
const char *band_limits(int T, int S, int Umax, int R, int J, int V);          // the limit that is broken, or null
// Every check of krnnt_band_eval under the entry's name, then *a filled in (the workspace carved, extra bytes demanded behind it) and
// *ngrad = 4 or 0.  No HIP call.
klstm_status band_eval_args(const char *name, const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b,
                            int T, int S, int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                            int R, const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                            float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, size_t extra, BandArgs *a,
                            int *ngrad, size_t *band_bytes);
hipError_t band_launch_prep(const BandArgs &a, hipStream_t st);                // k_rband_prep: ws.meta
hipError_t band_launch_joint_fwd(const BandArgs &a, hipStream_t st);           // k_rband_joint_fwd: lpb / lpy / lse of the band's nodes
// The bf16 joint's forward (klstm_rnnt_band16.hip): Wb [V][Jp] = bf(W) into wb (band16_wb_bytes(J, V) bytes, 256-byte aligned), then
// k_rband16_joint_fwd on it: the same three planes.
size_t band16_wb_bytes(int J, int V);
hipError_t band16_launch_joint_fwd(const BandArgs &a, void *wb, hipStream_t st);
hipError_t band_launch_lattice(const BandArgs &a, hipStream_t st);             // k_rband_lattice + k_rband_weights, once lpb / lpy / lse are written
hipError_t band_launch_finish(const BandArgs &a, hipStream_t st);              // k_rband_finish, behind the backward joint

// u of the tile's nodes into LDS: node = 16 (r - r0) + frame; -1: no such node
__device__ __forceinline__ void band_nodes(int *nodeU, int nnode, const int *u0, int t0, int r0, int Ts, int U, int R) {
  if ((int)threadIdx.x < nnode) {
    const int t = t0 + (threadIdx.x & 15), r = r0 + (threadIdx.x >> 4);
    int u = -1;
    if (t < Ts && r < R) {
      const int c = u0[t] + r;
      if (c <= U) u = c;
    }
    nodeU[threadIdx.x] = u;
  }
}

}  // namespace klstm
