// kaldi-lstm_amd/csrc/klstm_gemm_dev.h -- the 64 x 64 fp32 tile GEMM as device pieces: the job, the operand tiles, the tile
// body with its epilogues (used by k_gemm and its split-K forms in klstm_gemm.hip, by k_grads / k_grads_tm in
// klstm_grads.hip) and, on the host side, make_job and gemm_grid.
#pragma once
#include "klstm_kernels.h"
#include "klstm_step_dev.h"   // load8, keep_if, ldg4

namespace klstm {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// LDS-tiled MFMA GEMM tile (64x64 output, BK = 32, 256 threads = 2x2 waves of 32x32).  The next
// K tile is fetched into registers while the current one is multiplied out of LDS.
// ---------------------------------------------------------------------------------------------
constexpr int GT = 64, GK = 64, GLD = 80;   // LDS row stride 80 floats: k-groups land on disjoint banks

struct GemmJob {
  int M, N, K;
  const float *A; int lda;
  const float *B; int ldb;
  float beta;
  float *Cm; int ldc;
  const float *bias;
  int vecA, vecB;
  // everything above comes from make_job; what follows is optional and off by default.
  // extra destinations of the same result:
  float *Ct = nullptr; int ldct = 0;    // transposed copy  Ct[n][m]  (M % 4 == 0)
  float *C2 = nullptr; int ldc2 = 0;    // second copy      C2[m][n]
  float *C3 = nullptr; int tail0 = 0;   // rows m >= tail0 also to C3[m - tail0][n], dense (ld = N)
  int kslice = 0;         // k_gemm_bf16_nt only: split K, slice length (0: off)
  // fold product only (launch_fold): rows of A are read in gates-packed order (gperm = C) and the result goes straight
  // into the two packed operand arrays of the folded step kernels instead of Cm
  int gperm = 0;
  float4 *pk1 = nullptr; int nch1 = 0;  // [W_rm | W_x] gates array: [C/4 tiles][nch1 chunks of 32][2][64]
  float4 *pk2 = nullptr; int nch2 = 0;  // W_rm^T 4-row array:       [C/4 tiles][nch2 chunks of 128][2][64]
  // gradient product with the Update folded in (launch_grads with a GradsUpdate): Cm is the momentum buffer,
  // Cm = beta*Cm + A*B (:468-487), clipped if clip > 0, then P -= lr*Cm (:504-512); Ct then receives the UPDATED P
  float *P = nullptr; float lr = 0.f, clip = 0.f;
  int s3mode = 1;                            // plane format (klstm_math.h split_store4)
  unsigned short *s3 = nullptr; long s3pl = 0; int s3t = 0;   // the bf16 / fp16 planes of the UPDATED P (s3t = 0: P's layout, ld = ldc; 1: Ct's layout, ld = ldct)
  unsigned short *cth = nullptr;            // (or null) bf16 copy (RNE) of Ct, same layout: the B operand of klstm_gemm16.hip's LDS-DMA form
  int coal = 0;           // 1: Cm = beta*Cm + A*B through the same coalesced 16-byte epilogue without P (N, ldc % 4 == 0, aligned, no bias)
  const unsigned *guard = nullptr;   // k_gemm only: the engine's control words; a persistent launch in front gave up ([2] | [6]) -> write nothing
};

// One operand tile = GT x GK elements = 2 x (8 floats per thread).  Operand stored [X x K] (TA=false: 8 consecutive k
// of one x) or [K x X] (TA=true: 8 consecutive x of one k).  `vec` (block-uniform): rows 16-byte aligned and the
// contiguous extent a multiple of 8 -> branch-free loads.
template <bool TA>
__device__ __forceinline__ void fetch_tile(const float *__restrict__ P, int ld, bool vec, int X, int K, int x0, int k0,
                                           int tid, float (&r)[2][8], int gperm = 0) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    if (!TA) {
      const int x = x0 + (tid >> 2), k = k0 + h * 32 + (tid & 3) * 8;
      // gperm = C: logical row x = 4*cell + gate of the gates-packed order reads stored row gate*C + cell
      const int xs = x < X ? (gperm ? (x & 3) * gperm + (x >> 2) : x) : 0;
      const float *row = P + (size_t)xs * ld;
      if (vec) load8<true>(row, k, K, x < X, r[h]); else load8<false>(row, k, K, x < X, r[h]);
    } else {
      const int k = k0 + h * 32 + (tid >> 3), x = x0 + (tid & 7) * 8;
      const float *row = P + (size_t)(k < K ? k : 0) * ld;
      if (vec) load8<true>(row, x, X, k < K, r[h]); else load8<false>(row, x, X, k < K, r[h]);
    }
  }
}
// The same tile for operands whose rows are 16-byte aligned with a contiguous extent that is a multiple of 8 (every
// product of the engine itself): straight-line code -- clamped addresses, unconditional 16-byte loads, padding zeroed
// with keep_if.  (fetch_tile's runtime `vec` switch and its selects compile to conditional blocks whose joins drain
// every outstanding load: the four fetches of a K tile became four serialized memory round trips.)
struct RawTile { float4 v[2][2]; bool ok[2]; };
template <bool TA>
__device__ __forceinline__ void fetch_tile_vec(const float *__restrict__ P, int ld, int X, int K, int x0, int k0, int tid,
                                               RawTile &t, int gperm = 0) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float *p;
    if (!TA) {
      const int x = x0 + (tid >> 2), k = k0 + h * 32 + (tid & 3) * 8;
      t.ok[h] = x < X && k < K;                            // K % 8 == 0: an 8-group never straddles the end
      const int xc = x < X ? x : 0;
      const int xs = gperm ? (xc & 3) * gperm + (xc >> 2) : xc;
      p = P + (size_t)xs * ld + min(k, K - 8);
    } else {
      const int k = k0 + h * 32 + (tid >> 3), x = x0 + (tid & 7) * 8;
      t.ok[h] = k < K && x < X;                            // X % 8 == 0
      p = P + (size_t)min(k, K - 1) * ld + min(x, X - 8);
    }
    t.v[h][0] = ldg4(p); t.v[h][1] = ldg4(p + 4);
  }
}
// The [K x X] tile of an operand that OTHER workgroups of the same launch have just written with write-through stores (k_grads_tm: the
// d_r rows from the reduce workgroups): 16-byte sc1 loads -- served from beyond this XCD's L2, which may hold a line of it that another
// XCD completed later.  Same addresses, same padding rule.
__device__ __forceinline__ void fetch_tile_vec_coh(const float *__restrict__ P, int ld, int X, int K, int x0, int k0, int tid, RawTile &t) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(P), 0, K * ld * 4, 0x00020000);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int k = k0 + h * 32 + (tid >> 3), x = x0 + (tid & 7) * 8;
    t.ok[h] = k < K && x < X;
    const int off = (min(k, K - 1) * ld + min(x, X - 8)) * 4;
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t q0 = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16), q1 = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16, 0, 16);   // aux 16 = sc1
    t.v[h][0] = __builtin_bit_cast(float4, q0); t.v[h][1] = __builtin_bit_cast(float4, q1);
  }
}
// the padding mask is applied HERE, one K tile later: touching the fetched registers any earlier makes the wave wait for
// the loads before it multiplies the current tile
__device__ __forceinline__ void unpack_tile(const RawTile &t, float (&r)[2][8]) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float4 a = keep_if(t.v[h][0], t.ok[h]), b = keep_if(t.v[h][1], t.ok[h]);
    r[h][0] = a.x; r[h][1] = a.y; r[h][2] = a.z; r[h][3] = a.w;
    r[h][4] = b.x; r[h][5] = b.y; r[h][6] = b.z; r[h][7] = b.w;
  }
}
// LDS layout of an operand tile follows its storage so that the stash is two 16-byte stores either way:
//   TA (stored [K x X]):  Ls[k*GLD + x]   (GLD = 80: the four k-groups of an MFMA read land on disjoint banks)
//   !TA (stored [X x K]): Ls[x*GLX + k]   (GLX = 68: row x shifts the bank by 4, again disjoint for 16 rows x 4 k-groups)
constexpr int GLX = 68;
constexpr int GLDS = GK * GLD;               // floats per operand buffer (>= GT * GLX)
template <bool TA>
__device__ __forceinline__ void stash_tile(float *Ls, int tid, const float (&r)[2][8]) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    float *dst = TA ? Ls + (h * 32 + (tid >> 3)) * GLD + (tid & 7) * 8 : Ls + (tid >> 2) * GLX + h * 32 + (tid & 3) * 8;
    *reinterpret_cast<float4 *>(dst) = make_float4(r[h][0], r[h][1], r[h][2], r[h][3]);
    *reinterpret_cast<float4 *>(dst + 4) = make_float4(r[h][4], r[h][5], r[h][6], r[h][7]);
  }
}
template <bool TA>
__device__ __forceinline__ float lds_operand(const float *Ls, int k, int x) { return TA ? Ls[k * GLD + x] : Ls[x * GLX + k]; }

// 64x64 output tile, 4 waves (2x2) of 32x32, K tile 64.  The next K tile is fetched into registers while the
// current one is multiplied out of LDS (global latency hides under 16 k-steps x 4 MFMAs per wave).
template <bool TA, bool TB, bool VEC, bool COHA = false>   // COHA: A through fetch_tile_vec_coh (TA, VEC)
__device__ __forceinline__ void gemm_tile_impl(const GemmJob &g, int m0, int n0, float *As, float *Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = (f32x4){0, 0, 0, 0};

  float ra[2][8], rb[2][8];
  RawTile ta, tb;
  auto fetch = [&](int k0) {
    if constexpr (VEC) {
      if constexpr (COHA) fetch_tile_vec_coh(g.A, g.lda, g.M, g.K, m0, k0, tid, ta);
      else fetch_tile_vec<TA>(g.A, g.lda, g.M, g.K, m0, k0, tid, ta, g.gperm);
      fetch_tile_vec<!TB>(g.B, g.ldb, g.N, g.K, n0, k0, tid, tb);   // B [N x K] when TB, else [K x N]
    } else {
      fetch_tile<TA>(g.A, g.lda, g.vecA, g.M, g.K, m0, k0, tid, ra, g.gperm);
      fetch_tile<!TB>(g.B, g.ldb, g.vecB, g.N, g.K, n0, k0, tid, rb);
    }
  };
  fetch(0);
  // beta != 0 (momentum folded into the gradient products, :468-487): the old C tile is requested now so that its
  // HBM latency hides under the K loop instead of sitting in front of the stores
  float cold[2][2][4];
  if (g.beta != 0.f && !g.P && !g.coal) {
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int ni = 0; ni < 2; ni++) {
        const int n = n0 + wc * 32 + ni * 16 + i16;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int m = m0 + wr * 32 + mi * 16 + 4 * kg + r;
          const bool ok = n < g.N && m < g.M;
          const float v = g.Cm[ok ? (size_t)m * g.ldc + n : 0];
          cold[mi][ni][r] = ok ? v : 0.f;
        }
      }
  }
  for (int k0 = 0; k0 < g.K; k0 += GK) {
    if constexpr (VEC) { unpack_tile(ta, ra); unpack_tile(tb, rb); }
    stash_tile<TA>(As, tid, ra);
    stash_tile<!TB>(Bs, tid, rb);
    __syncthreads();
    if (k0 + GK < g.K) fetch(k0 + GK);
    // full K tiles run a fully unrolled 16-step body (a runtime trip count defeats the unroller and leaves a rolled
    // ds_read -> MFMA loop); only the last, short tile takes the rolled path and skips its all-zero tail steps
    auto kstep = [&](int kk) {
      const int k = kk * 4 + kg;
      const float a0 = lds_operand<TA>(As, k, wr * 32 + i16), a1 = lds_operand<TA>(As, k, wr * 32 + 16 + i16);
      const float b0 = lds_operand<!TB>(Bs, k, wc * 32 + i16), b1 = lds_operand<!TB>(Bs, k, wc * 32 + 16 + i16);
      acc[0][0] = MFMA16(a0, b0, acc[0][0]);
      acc[0][1] = MFMA16(a0, b1, acc[0][1]);
      acc[1][0] = MFMA16(a1, b0, acc[1][0]);
      acc[1][1] = MFMA16(a1, b1, acc[1][1]);
    };
    if (!TA && TB) {
      // both operands k-contiguous in LDS ([x][k]): one 16-byte read per operand block feeds FOUR k-steps.  Within a
      // group of 16 k the MFMA k-lane kg of step e contracts k = 16j + 4kg + e -- the same bijection for A and B, so the
      // sum is over every k exactly once (zero-filled past K)
#pragma unroll
      for (int j = 0; j < GK / 16; j++) {
        const int ko = 16 * j + 4 * kg;
        const float4 a0 = *reinterpret_cast<const float4 *>(As + (wr * 32 + i16) * GLX + ko);
        const float4 a1 = *reinterpret_cast<const float4 *>(As + (wr * 32 + 16 + i16) * GLX + ko);
        const float4 b0 = *reinterpret_cast<const float4 *>(Bs + (wc * 32 + i16) * GLX + ko);
        const float4 b1 = *reinterpret_cast<const float4 *>(Bs + (wc * 32 + 16 + i16) * GLX + ko);
        const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
        const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          acc[0][0] = MFMA16(av0[e], bv0[e], acc[0][0]);
          acc[0][1] = MFMA16(av0[e], bv1[e], acc[0][1]);
          acc[1][0] = MFMA16(av1[e], bv0[e], acc[1][0]);
          acc[1][1] = MFMA16(av1[e], bv1[e], acc[1][1]);
        }
      }
    } else if (k0 + GK <= g.K) {
#pragma unroll
      for (int kk = 0; kk < GK / 4; kk++) kstep(kk);
    } else {
      const int ksteps = (g.K - k0 + 3) / 4;
      for (int kk = 0; kk < ksteps; kk++) kstep(kk);
    }
    __syncthreads();
  }
  if (g.P || g.coal) {
    // Gradient product with momentum and (P != null) Update folded in (launch_grads + GradsUpdate; N, ldc, ldct multiples of 4, 16-byte
    // aligned blobs).  Everything that touches HBM moves as 16-byte pieces, 256 contiguous bytes per tile row: the tile goes
    // through LDS (the K loop ended with a barrier, As is free), then  corr = beta*corr + grad (:468-487), clip,
    // theta -= lr*corr (:504-512)  on float4 rows, then the transposed copy of the updated parameters.
    float *Cs = As;                                    // 64 x GLX floats <= GLDS
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int ni = 0; ni < 2; ni++) {
        const float e[4] = {acc[mi][ni].x, acc[mi][ni].y, acc[mi][ni].z, acc[mi][ni].w};
#pragma unroll
        for (int r = 0; r < 4; r++) Cs[(wr * 32 + mi * 16 + 4 * kg + r) * GLX + wc * 32 + ni * 16 + i16] = e[r];
      }
    // this thread's four pieces of the old corr and parameter tiles, all requested before the first store (a load behind a store
    // waits for it: the compiler cannot know that the rows do not overlap -- four memory round trips per tile instead of one)
    float4 oc4[4], op4[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + 256 * u, m = m0 + (p >> 4), n = n0 + (p & 15) * 4;
      const size_t off = m < g.M && n + 4 <= g.N ? (size_t)m * g.ldc + n : 0;
      oc4[u] = g.beta != 0.f ? *reinterpret_cast<const float4 *>(g.Cm + off) : make_float4(0.f, 0.f, 0.f, 0.f);
      op4[u] = g.P ? *reinterpret_cast<const float4 *>(g.P + off) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + 256 * u, ml = p >> 4, nq = (p & 15) * 4;
      const int m = m0 + ml, n = n0 + nq;
      if (m < g.M && n + 4 <= g.N) {
        float *cs = Cs + ml * GLX + nq;
        const float4 a = *reinterpret_cast<const float4 *>(cs);
        float4 *cp = reinterpret_cast<float4 *>(g.Cm + (size_t)m * g.ldc + n);
        float4 *pp = reinterpret_cast<float4 *>((g.P ? g.P : g.Cm) + (size_t)m * g.ldc + n);
        float4 pv = op4[u];
        float c[4] = {a.x, a.y, a.z, a.w};
        if (g.beta != 0.f) {
          const float4 o = oc4[u];
          c[0] = g.beta * o.x + c[0]; c[1] = g.beta * o.y + c[1]; c[2] = g.beta * o.z + c[2]; c[3] = g.beta * o.w + c[3];
        }
        if (g.clip > 0.f) {
#pragma unroll
          for (int q = 0; q < 4; q++) { c[q] = c[q] < -g.clip ? -g.clip : c[q]; c[q] = c[q] > g.clip ? g.clip : c[q]; }
        }
        // (plain stores.  Measured and dropped, round 6: corr / parameters / planes as nontemporal stores -- the launch 14.4 -> 15.6 us and
        //  the fold behind it 13.9 -> 14.4 us at 40/800/512: it finds the planes this pass has just written closer than HBM.)
        *cp = make_float4(c[0], c[1], c[2], c[3]);
        if (g.P) {
          pv.x = pv.x + (-g.lr) * c[0]; pv.y = pv.y + (-g.lr) * c[1]; pv.z = pv.z + (-g.lr) * c[2]; pv.w = pv.w + (-g.lr) * c[3];
          *pp = pv;
          *reinterpret_cast<float4 *>(cs) = pv;
          if (g.s3 && !g.s3t) {
            const float v4[4] = {pv.x, pv.y, pv.z, pv.w};
            split_store4(g.s3mode, v4, g.s3 + (size_t)m * g.ldc + n, g.s3pl);
          }
        }
      }
    }
    if (!g.Ct || !g.P) return;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + 256 * u, nl = p >> 4, mq = (p & 15) * 4;
      const int n = n0 + nl, m = m0 + mq;
      if (n < g.N && m + 4 <= g.M) {
        const float *cs = Cs + mq * GLX + nl;
        const float v4[4] = {cs[0], cs[GLX], cs[2 * GLX], cs[3 * GLX]};
        *reinterpret_cast<float4 *>(g.Ct + (size_t)n * g.ldct + m) = make_float4(v4[0], v4[1], v4[2], v4[3]);
        if (g.s3 && g.s3t) split_store4(g.s3mode, v4, g.s3 + (size_t)n * g.ldct + m, g.s3pl);
        if (g.cth) split_store4(3, v4, g.cth + (size_t)n * g.ldct + m, 0);
      }
    }
    return;
  }
  if (g.pk1) {
    // tile rows are in gates-packed order: row r = 4*(cell - cell0) + gate, cell0 = m0/4 (a multiple of 16); columns are
    // the k axis of the folded gates operand and the row (cell) axis of the folded d_m operand.  Stage the tile in LDS,
    // then every thread writes 16-byte pieces in DESTINATION order (runs of 1 KB / 256 B).
    constexpr int CLD = 68;
    float *Cs = As;                                    // 64 x 68 floats <= GLDS; the K loop ended with a barrier
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int ni = 0; ni < 2; ni++) {
        const float e[4] = {acc[mi][ni].x, acc[mi][ni].y, acc[mi][ni].z, acc[mi][ni].w};
#pragma unroll
        for (int r = 0; r < 4; r++) Cs[(wr * 32 + mi * 16 + 4 * kg + r) * CLD + wc * 32 + ni * 16 + i16] = e[r];
      }
    __syncthreads();
    const int C = g.gperm, cell0 = m0 >> 2;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + 256 * u;
      {   // gates array: piece = (packed tile pt, chunk half chl, h, lane16 = kgrp*16 + i) -> row pt*16 + i, cols chl*32 + kgrp*8 + h*4
        const int pt = p >> 8, chl = (p >> 7) & 1, h = (p >> 6) & 1, l16 = p & 63, i = l16 & 15;
        const int nl = chl * 32 + (l16 >> 4) * 8 + h * 4, n = n0 + nl;
        const int cell = cell0 + pt * 4 + (i >> 2);
        if (cell < C && n < g.N) {
          const float4 v = *reinterpret_cast<const float4 *>(Cs + (pt * 16 + i) * CLD + nl);
          g.pk1[(((size_t)(cell >> 2) * g.nch1 + (n >> 5)) * 2 + h) * 64 + l16] = v;
        }
      }
      {   // d_m array: piece = (column quad ct, gate, cell quad kq, cq = column % 4) -> 4 cells of one gate at one column
        const int cq = p & 3, kq = (p >> 2) & 3, gate = (p >> 4) & 3, ct = p >> 6;
        const int c = n0 + ct * 4 + cq, cell = cell0 + kq * 4;
        if (g.pk2 && c < g.N && cell < C) {                  // (pk2 null: only the gates-order operand is wanted)
          const float *cp = Cs + (kq * 16 + gate) * CLD + ct * 4 + cq;
          const float4 v = make_float4(cp[0], cp[4 * CLD], cp[8 * CLD], cp[12 * CLD]);
          const int k = gate * C + cell;
          g.pk2[(((size_t)(c >> 2) * g.nch2 + (k >> 7)) * 2 + ((k >> 6) & 1)) * 64 + ((k & 63) >> 2) * 4 + cq] = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      const int n = n0 + wc * 32 + ni * 16 + i16;
      if (n >= g.N) continue;
      const float bv = g.bias ? g.bias[n] : 0.f;
      const float e[4] = {acc[mi][ni].x, acc[mi][ni].y, acc[mi][ni].z, acc[mi][ni].w};
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = m0 + wr * 32 + mi * 16 + 4 * kg + r;
        if (m >= g.M) continue;
        float *cp = g.Cm + (size_t)m * g.ldc + n;
        float val = e[r] + bv;
        if (g.beta != 0.f) val = g.beta * cold[mi][ni][r] + val;
        *cp = val;
        if (g.C2) g.C2[(size_t)m * g.ldc2 + n] = val;
        if (g.C3 && m >= g.tail0) g.C3[(size_t)(m - g.tail0) * g.N + n] = val;
      }
      if (g.Ct) {               // transposed copy of the raw product (beta == 0, no bias)
        const int m = m0 + wr * 32 + mi * 16 + 4 * kg;
        if (m + 4 <= g.M) *reinterpret_cast<float4 *>(g.Ct + (size_t)n * g.ldct + m) = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
}

template <bool TA, bool TB>
__device__ __forceinline__ void gemm_tile(const GemmJob &g, int m0, int n0, float *As, float *Bs) {
  if (g.vecA && g.vecB) gemm_tile_impl<TA, TB, true>(g, m0, n0, As, Bs);     // block-uniform: the whole K loop is one of two versions
  else gemm_tile_impl<TA, TB, false>(g, m0, n0, As, Bs);
}

struct ReduceArgs {
  const float *ws; int ks, M, N;
  float beta; float *Cm; int ldc;
  const float *bias = nullptr;
  const float *add = nullptr; int add_ld = 0;   // C = beta*C + add + bias + sum of slices
  float *C2 = nullptr; int ldc2 = 0;            // mirrors, as in GemmJob
  float *C3 = nullptr; int tail0 = 0;
  const unsigned *guard = nullptr;              // as in GemmJob
};
__global__ __launch_bounds__(256) void k_splitk_reduce(ReduceArgs a);   // klstm_gemm.hip; launch_gemm_bf16_nt_splitk (klstm_grads.hip) launches it too

static inline GemmJob make_job(bool transA, bool transB, int M, int N, int K, const float *A, int lda, const float *B,
                        int ldb, float beta, float *Cm, int ldc, const float *bias) {
  GemmJob g;
  g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.beta = beta;
  g.Cm = Cm; g.ldc = ldc; g.bias = bias;
  // branch-free 8-wide fetches need aligned rows and a contiguous extent that is a multiple of 8
  g.vecA = aligned16(A) && lda % 4 == 0 && (transA ? M : K) % 8 == 0;
  g.vecB = aligned16(B) && ldb % 4 == 0 && (transB ? K : N) % 8 == 0;
  return g;
}
// k_gemm's 1-D grid: the 64 x 64 output tiles, padded to a multiple of 8 (one share per XCD)
static inline dim3 gemm_grid(int M, int N) { return dim3(cdiv(cdiv(N, GT) * cdiv(M, GT), 8) * 8); }

}  // namespace klstm
