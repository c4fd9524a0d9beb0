// kaldi-lstm_amd/csrc/klstm_grads.hip -- the gradient launch (fp32 64 x 64 tiles: klstm_gemm_dev.h; bf16 128-wide tiles:
// here), the bf16 NT product on the same tiles, and Update + repack; then their launchers.
//
// What each kernel replaces in the reference (google/nnet/bd-nnet-lstm-projected-streams.h):
//   k_grads      : all gradient accumulations (:468-487) in one grouped launch
//   k_update_repack : Update (:504-512) + refresh of the transposed weight copies
#include <type_traits>
#include "klstm_gemm_dev.h"
#include "klstm_persist_dev.h"

namespace klstm {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// all gradient accumulations of one minibatch in ONE launch (...streams.h:468-487):
//   blocks [0, nb0)        W_gifo_x_corr = beta*corr + DGIFO^T * in
//   blocks [nb0, nb1)      W_gifo_r_corr = beta*corr + DGIFO^T * YR[0..T-1]
//   blocks [nb1, nb2)      W_r_m_corr    = beta*corr + DR^T * YM
//   blocks [nb2, nb3)      bias / peephole column sums (AddRowSumMat, AddDiagMatMat x3)
// ---------------------------------------------------------------------------------------------
struct GradsArgs {
  const unsigned *guard;   // the engine's control words: status of the persistent chain ([2], [6]) or of the one-shot all-reduce ([9]) non-zero -> the minibatch is invalid, touch nothing
  float *mark;             // (or null) data-parallel runs: the validity word that rides at the end of the gradient blob through the all-reduce --
                           // 0 when this rank's gradient is real, 1 when the guard stopped it; the SUM every rank receives gates every rank's Update
  GemmJob wx, wr, wm;
  int nb0, nb1, nb2, nvec;   // tile-id ranges of the three products, then nvec column-sum blocks
  int bf16_narrow;           // k_grads_bf16: 128 x 64 tiles instead of 128 x 128
  int C, S, T;
  const float *dgifo, *cc;
  float beta;
  float *g_bias, *g_pi, *g_pf, *g_po;
  float *p_bias, *p_pi, *p_pf, *p_po;   // parameters to update in the same pass (null: gradient only)
  float lr, clip;
  // k_grads_tm ("tail_merge"): the first nred workgroups add the tail workgroups' partial d_r / in_diff rows (TailReduceJob), the
  // W_r_m tiles wait until tr.ctr[0] has reached tr_target
  TailReduceJob tr; int nred; unsigned tr_target;
};

// bias / peephole column sums of k_grads: block vb covers 64 columns of the 4C gate axis with 4 row groups
__device__ __forceinline__ void grads_column_sums(const GradsArgs &a, int vb, float *lds0, float *lds1) {
  const int C = a.C, S = a.S, rows = a.T * a.S;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = vb * 64 + tx;
  float sb = 0.f, sp = 0.f;
  if (col < 4 * C) {
    const int gate = col / C, cell = col - gate * C;
    // DI/DF[1..T] pair with YC[0..T-1]; DO[1..T] pairs with YC[1..T]
    const float *cbase = a.cc + (gate == 3 ? (size_t)S * C : 0) + cell;
    const float *dbase = a.dgifo + (size_t)S * 4 * C + col;
    // 8 row pairs in flight per thread (a serial loop pays one memory latency per row), summed in row order
    for (int r0 = ty; r0 < rows; r0 += 32) {
      float dv[8], cv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int r = min(r0 + 4 * u, rows - 1);
        dv[u] = dbase[(size_t)r * 4 * C];
        cv[u] = cbase[(size_t)r * C];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const bool on = r0 + 4 * u < rows;
        sb += on ? dv[u] : 0.f;
        if (gate != 0) sp += on ? dv[u] * cv[u] : 0.f;
      }
    }
  }
  float(*rb)[64] = reinterpret_cast<float(*)[64]>(lds0);
  float(*rp)[64] = reinterpret_cast<float(*)[64]>(lds1);
  rb[ty][tx] = sb; rp[ty][tx] = sp;
  __syncthreads();
  if (ty == 0 && col < 4 * C) {
    for (int w = 1; w < 4; w++) { sb += rb[w][tx]; sp += rp[w][tx]; }
    const int gate = col / C, cell = col - gate * C;
    auto fold_update = [&](float c, float *pp) {       // :504-512 for one vector element
      if (a.clip > 0.f) { c = c < -a.clip ? -a.clip : c; c = c > a.clip ? a.clip : c; }
      float pv = *pp;
      pv = pv + (-a.lr) * c;
      *pp = pv;
      return c;
    };
    float cb = (a.beta != 0.f ? a.beta * a.g_bias[col] : 0.f) + sb;
    if (a.p_bias) cb = fold_update(cb, a.p_bias + col);
    a.g_bias[col] = cb;
    float *gp = gate == 1 ? a.g_pi : gate == 2 ? a.g_pf : gate == 3 ? a.g_po : nullptr;
    float *pq = gate == 1 ? a.p_pi : gate == 2 ? a.p_pf : gate == 3 ? a.p_po : nullptr;
    if (gp) {
      float cp = (a.beta != 0.f ? a.beta * gp[cell] : 0.f) + sp;
      if (pq) cp = fold_update(cp, pq + cell);
      gp[cell] = cp;
    }
  }
}

// TM (k_grads_tm, "tail_merge"): the launch also runs the reduction of the tail workgroups' partial rows that used to be k_tail_reduce behind the BPTT
// launch.  Workgroups [0, nred) (dispatched first) add the partial rows -- d_r as write-through stores --, wait for their stores'
// acknowledgements and arrive at tr.ctr[0]; the W_r_m tiles (the only readers of d_r) sit at the END of every XCD's range, wait for
// ctr[0] to reach tr_target (the engine's running total of reduce workgroups over its merged launches, this one included: nothing to
// reset, a launch that does nothing still arrives, and nred may differ from launch to launch) and read d_r with sc1
// loads; the W_gifo_x / W_gifo_r tiles and the column sums start at once.  The wait is bounded (200 ms; an expiry is counted in ctr[1] and
// the tile goes on -- the reduce workgroups have the lowest indices, so they are resident or done before any tile that waits for them).
template <bool TM>
__device__ __forceinline__ void grads_body(const GradsArgs &a) {
  const bool invalid = a.guard && (a.guard[2] | a.guard[6] | a.guard[9]);
  if (a.mark && blockIdx.x == 0 && threadIdx.x == 0) *a.mark = invalid ? 1.f : 0.f;
  int bi = (int)blockIdx.x;
  if constexpr (TM) {
    if (bi < a.nred) {
      if (!invalid) {
        const int gidx = bi * 256 + (int)threadIdx.x;
        tail_reduce_outputs<true>(a.tr.tws, a.tr.nslots, a.tr.T, a.tr.S, a.tr.R, a.tr.ncols, a.tr.od, a.tr.od_stride, a.tr.dr, a.tr.in_diff,
                                  a.tr.id_stride, gidx >> 3, a.nred * 32, gidx & 7, nullptr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_fetch_add(a.tr.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    bi -= a.nred;
  }
  if (invalid) return;   // a persistent launch of this minibatch gave up: leave momentum and parameters alone
  __shared__ __attribute__((aligned(16))) float As[GLDS];
  __shared__ __attribute__((aligned(16))) float Bs[GLDS];
  // XCD-aware order: workgroup w lands on XCD w % 8 (observed dispatch rule, speed only); XCD x gets the contiguous
  // m-major tile range [x*cpx, (x+1)*cpx), so its private L2 holds a few A row panels and the B column panels
  // instead of streaming every A panel once per XCD.  (TM: two such ranges per XCD -- its share of the tiles that wait for nobody,
  // then its share of the W_r_m tiles and column sums.)
  const int nbt = a.nb2 + a.nvec;
  int b;
  if constexpr (TM) {
    const int cpx1 = (a.nb1 + 7) >> 3, cpx2 = (nbt - a.nb1 + 7) >> 3, x = bi & 7, pos = bi >> 3;
    if (pos < cpx1) { b = x * cpx1 + pos; if (b >= a.nb1) return; }
    else { b = a.nb1 + x * cpx2 + (pos - cpx1); if (b >= nbt) return; }
  } else {
    const int cpx = (nbt + 7) >> 3;
    b = (bi & 7) * cpx + (bi >> 3);
    if (b >= nbt) return;
  }
  if (b < a.nb2) {
    const GemmJob &g = b < a.nb0 ? a.wx : b < a.nb1 ? a.wr : a.wm;
    const int lb = b < a.nb0 ? b : b < a.nb1 ? b - a.nb0 : b - a.nb1;
    const int ntn = (g.N + GT - 1) / GT;
    if constexpr (TM) {
      if (b >= a.nb1) {
        if (threadIdx.x == 0) {
          const long long t0 = wall_clock64();
          while ((int)(__hip_atomic_load(a.tr.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.tr_target) < 0) {
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > 20000000LL) { __hip_atomic_fetch_add(a.tr.ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
          }
        }
        __syncthreads();
        gemm_tile_impl<true, false, true, true>(g, (lb / ntn) * GT, (lb % ntn) * GT, As, Bs);   // (the merged form is only launched with 16-byte rows)
        return;
      }
    }
    gemm_tile<true, false>(g, (lb / ntn) * GT, (lb % ntn) * GT, As, Bs);
    return;
  }
  grads_column_sums(a, b - a.nb2, As, Bs);
}
// Four waves per SIMD (128 registers; two values spill): a 512-input layer has 954 tiles and column-sum blocks -- at three per SIMD 768 are
// resident and the rest wait a whole tile time (every tile is latency-bound: operands, old corr / parameters, stores).  tools/ab_step.py,
// bench.py --config c4 (A-B of builds, twice each): 40-input layer 14.4 -> 13.7 us, 512-input layer 21.3 -> 18.3 us, configs[3] 0.4110 -> 0.4077 ms.
__global__ __launch_bounds__(256, 4) void k_grads(GradsArgs a) { grads_body<false>(a); }
__global__ __launch_bounds__(256) void k_grads_tm(GradsArgs a) { grads_body<true>(a); }   // "tail_merge"

// ---------------------------------------------------------------------------------------------
// bf16 operand mode: the three gradient products on v_mfma_f32_16x16x32_bf16.  128x128 output tiles (the 64x64 fp32
// tile is L2-bandwidth-bound long before the 16x faster bf16 pipe is busy), K tile 64 (the K loop exposes one memory
// latency per tile: 64 KB in flight per workgroup).  Both operands are stored
// [K x X] (fp32 planes); a thread fetches two consecutive k rows x four x columns, rounds to bf16 (RNE) and writes the
// (k, k+1) pairs as 32-bit words into a k-contiguous LDS layout  word[(x&3)*PLANE + (x>>2)*LDQ + k/2]: four planes by
// x mod 4 (the four columns a thread holds go to four planes), LDQ = 36 and PLANE = 16 mod 64 make the 16-byte operand
// reads of 16 rows x 4 k-groups conflict-free and leave the 32-bit stash writes 2-way (a plain [x][k/2] layout is 8-way:
// its writes alone cost more than the MFMAs).  An MFMA operand (8 consecutive k of one row) is one ds_read_b128.
// fp32 accumulate, beta and the column-sum blocks exactly as in k_grads.
// ---------------------------------------------------------------------------------------------
constexpr int GRADS_BF16_MIN_ROWS = 256;
constexpr int BT = 128, BK = 64, LDQ = 36, PLANE = 32 * LDQ + 16;   // see the layout note above

template <int XQ = 32>                                // x quads of the tile (32: 128 columns, 16: 64)
__device__ __forceinline__ void fetch_pair(const float *__restrict__ P, int ld, int X, int K, int x0, int k0, int u,
                                           float4 (&r)[2], int &ok) {
  const int kp = u / XQ, xq = u % XQ;
  const int k = k0 + 2 * kp, x = x0 + 4 * xq;
  const bool xin = x + 4 <= X;                       // X % 4 == 0 on this path
  const float *p0 = P + (size_t)min(k, K - 1) * ld + (xin ? x : 0);
  const float *p1 = P + (size_t)min(k + 1, K - 1) * ld + (xin ? x : 0);
  r[0] = ldg4(p0); r[1] = ldg4(p1);
  ok = (xin && k < K ? 1 : 0) | (xin && k + 1 < K ? 2 : 0);     // applied by stash_pair, one K tile later (see unpack_tile)
}
__device__ __forceinline__ unsigned pack_pair(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 h = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, h);
}
template <int XQ = 32>
__device__ __forceinline__ void stash_pair(unsigned *Ls, int u, const float4 (&rr)[2], int ok) {
  const float4 r[2] = {keep_if(rr[0], (ok & 1) != 0), keep_if(rr[1], (ok & 2) != 0)};
  const int kp = u / XQ, xq = u % XQ;
  unsigned *d = Ls + xq * LDQ + kp;
  d[0] = pack_pair(r[0].x, r[1].x);
  d[PLANE] = pack_pair(r[0].y, r[1].y);
  d[2 * PLANE] = pack_pair(r[0].z, r[1].z);
  d[3 * PLANE] = pack_pair(r[0].w, r[1].w);
}

// NJ = 16-column blocks per wave: 4 = 128 x 128 tiles, 2 = 128 x 64 (twice the workgroups: the K loop exposes a memory latency per
// tile, and 288 tiles of 128 x 128 leave the 256 CUs with one workgroup each)
template <int NJ, bool NO32 = false>                 // NO32: the kernel's fast epilogues are the ones WITHOUT the fp32 transposed copy (4, 5 instead of 1, 2)
__device__ __forceinline__ void gemm_tile_bf16_tn(const GemmJob &g, int m0, int n0, unsigned *As, unsigned *Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[i][j] = (f32x4){0, 0, 0, 0};
  constexpr int NU = (BK / 2) * 32 / 256;            // (k pair, x quad) units per thread and operand
  constexpr int NUB = (BK / 2) * (8 * NJ) / 256;     // ... of B: 32 NJ columns = 8 NJ quads
  float4 ra[NU][2], rb[NUB][2];
  int oa[NU], ob[NUB];
#pragma unroll
  for (int h = 0; h < NU; h++) fetch_pair(g.A, g.lda, g.M, g.K, m0, 0, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
  for (int h = 0; h < NUB; h++) fetch_pair<8 * NJ>(g.B, g.ldb, g.N, g.K, n0, 0, tid + 256 * h, rb[h], ob[h]);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
#pragma unroll
    for (int h = 0; h < NU; h++) stash_pair(As, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
    for (int h = 0; h < NUB; h++) stash_pair<8 * NJ>(Bs, tid + 256 * h, rb[h], ob[h]);
    __syncthreads();
    if (k0 + BK < g.K) {
#pragma unroll
      for (int h = 0; h < NU; h++) fetch_pair(g.A, g.lda, g.M, g.K, m0, k0 + BK, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
      for (int h = 0; h < NUB; h++) fetch_pair<8 * NJ>(g.B, g.ldb, g.N, g.K, n0, k0 + BK, tid + 256 * h, rb[h], ob[h]);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ks++) {
      bf16x8 af[4], bfr[NJ];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int xa = wr * 64 + i * 16 + i16;
        af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(As + (xa & 3) * PLANE + (xa >> 2) * LDQ + ks * 16 + kg * 4));
      }
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int xb = wc * 16 * NJ + j * 16 + i16;
        bfr[j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(Bs + (xb & 3) * PLANE + (xb >> 2) * LDQ + ks * 16 + kg * 4));
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  if (g.P) {
    // Gradient product with momentum and Update folded in (launch_grads + GradsUpdate on the bf16 tiles; N, ldc, ldct multiples of 4,
    // 16-byte aligned blobs) -- the epilogue of gemm_tile_impl on this tile shape: the 128-row tile leaves in FOUR chunks of 32
    // CONSECUTIVE rows (chunk c = blocks i = 2 (c & 1), + 1 of the two waves with wr = c >> 1: what fits the A staging area; the
    // transposed copy then leaves in whole 128-byte lines per column, its bf16 copy in 64-byte runs), each chunk through LDS as 16-byte
    // row pieces: corr = beta*corr + grad (:468-487), clip, theta -= lr*corr (:504-512), the bf16 / fp16 planes of the updated tile,
    // then its transposed copy.  The K loop ended with a barrier: As is free.
    constexpr int BTN = 32 * NJ, CLD = BTN + 4, Q = BTN / 4, NPU = 32 * Q / 256, NPT = BTN * 8 / 256;
    static_assert(32 * CLD <= 4 * PLANE, "the chunk does not fit the A staging area");
    float *Cs = reinterpret_cast<float *>(As);
    // V = 0: any tile.  V = 1, 2, 3: the three jobs of the many-stream bf16 mode on a FULL tile with momentum (W_gifo_r: bf16 plane in
    // its own layout + transposed copy + that copy's bf16 copy; W_gifo_x: transposed copy + its bf16 copy; W_r_m: transposed copy + bf16
    // plane in the copy's layout; V = 4, 5: as 1, 2 WITHOUT the fp32 transposed copy -- only its bf16 copy has a reader while the
    // per-XCD chains run: 17 MB of writes less per layer) with every load and store UNCONDITIONAL -- the compiler then counts what is outstanding and waits for
    // exactly the loads it needs; behind a conditional store it waits for everything, i.e. for the previous chunk's stores to drain
    // (twice per chunk).
    auto epilogue = [&](auto vtag) {
      constexpr int V = decltype(vtag)::value;
      constexpr bool F = V != 0;
      // this thread's pieces of the old corr and parameter rows of a chunk: requested ONE CHUNK AHEAD (chunk 0's before the loop,
      // chunk i + 1's in front of chunk i's arithmetic and stores), so that only the first memory round trip is exposed -- a tile is
      // usually the only one its compute unit has (256-288 tiles on 256 units), nothing else would hide the other three
      float4 oc4[2][NPU], op4[2][NPU];
      auto fetch_old = [&](int i, float4 (&oc)[NPU], float4 (&op)[NPU]) {
#pragma unroll
        for (int u = 0; u < NPU; u++) {
          const int p = tid + 256 * u, lr = p / Q, m = m0 + 32 * i + lr, n = n0 + (p % Q) * 4;
          const size_t off = F || (m < g.M && n + 4 <= g.N) ? (size_t)m * g.ldc + n : 0;
          if (F) oc[u] = *reinterpret_cast<const float4 *>(g.Cm + off);
          else oc[u] = g.beta != 0.f ? *reinterpret_cast<const float4 *>(g.Cm + off) : make_float4(0.f, 0.f, 0.f, 0.f);
          op[u] = *reinterpret_cast<const float4 *>(g.P + off);
        }
      };
      fetch_old(0, oc4[0], op4[0]);
#pragma unroll
      for (int i = 0; i < 4; i++) {                    // (chunk index: rows m0 + 32 i .. + 31)
        if (wr == (i >> 1)) {
#pragma unroll
          for (int b = 0; b < 2; b++)
#pragma unroll
            for (int j = 0; j < NJ; j++) {
              const f32x4 &av = acc[2 * (i & 1) + b][j];
              const float e[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
              for (int r = 0; r < 4; r++) Cs[(b * 16 + 4 * kg + r) * CLD + wc * 16 * NJ + j * 16 + i16] = e[r];
            }
        }
        if (i < 3) fetch_old(i + 1, oc4[(i + 1) & 1], op4[(i + 1) & 1]);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NPU; u++) {
          const int p = tid + 256 * u, lr = p / Q, nq = (p % Q) * 4;
          const int m = m0 + 32 * i + lr, n = n0 + nq;
          if (F || (m < g.M && n + 4 <= g.N)) {
            float *cs = Cs + lr * CLD + nq;
            const float4 a4 = *reinterpret_cast<const float4 *>(cs);
            float c[4] = {a4.x, a4.y, a4.z, a4.w};
            if (F || g.beta != 0.f) {
              const float4 o = oc4[i & 1][u];
              c[0] = g.beta * o.x + c[0]; c[1] = g.beta * o.y + c[1]; c[2] = g.beta * o.z + c[2]; c[3] = g.beta * o.w + c[3];
            }
            if (g.clip > 0.f) {
#pragma unroll
              for (int q = 0; q < 4; q++) { c[q] = c[q] < -g.clip ? -g.clip : c[q]; c[q] = c[q] > g.clip ? g.clip : c[q]; }
            }
            *reinterpret_cast<float4 *>(g.Cm + (size_t)m * g.ldc + n) = make_float4(c[0], c[1], c[2], c[3]);
            float4 pv = op4[i & 1][u];
            pv.x = pv.x + (-g.lr) * c[0]; pv.y = pv.y + (-g.lr) * c[1]; pv.z = pv.z + (-g.lr) * c[2]; pv.w = pv.w + (-g.lr) * c[3];
            *reinterpret_cast<float4 *>(g.P + (size_t)m * g.ldc + n) = pv;
            *reinterpret_cast<float4 *>(cs) = pv;
            if (V == 1 || V == 4 || (V == 0 && g.s3 && !g.s3t)) {
              const float v4[4] = {pv.x, pv.y, pv.z, pv.w};
              split_store4(F ? 3 : g.s3mode, v4, g.s3 + (size_t)m * g.ldc + n, g.s3pl);
            }
          }
        }
        __syncthreads();
        if (F || g.Ct) {
#pragma unroll
          for (int u = 0; u < NPT; u++) {
            const int p = tid + 256 * u, nl = p >> 3, lr = (p & 7) * 4;
            const int n = n0 + nl, m = m0 + 32 * i + lr;
            if (F || (n < g.N && m + 4 <= g.M)) {
              const float *cs = Cs + lr * CLD + nl;
              const float v4[4] = {cs[0], cs[CLD], cs[2 * CLD], cs[3 * CLD]};
              if (V <= 3) *reinterpret_cast<float4 *>(g.Ct + (size_t)n * g.ldct + m) = make_float4(v4[0], v4[1], v4[2], v4[3]);
              if (V == 3 || (V == 0 && g.s3 && g.s3t)) split_store4(F ? 3 : g.s3mode, v4, g.s3 + (size_t)n * g.ldct + m, g.s3pl);
              if (V == 1 || V == 2 || V == 4 || V == 5 || (V == 0 && g.cth)) split_store4(3, v4, g.cth + (size_t)n * g.ldct + m, 0);
            }
          }
          __syncthreads();
        }
      }
    };
    // (NO32 is the KERNEL's: full tiles of W_gifo_r / W_gifo_x leave the fp32 transposed copy out, partial tiles -- the generic epilogue --
    //  still write it, which is harmless: the engine treats the whole copy as stale.  A kernel with six epilogues, or a generic one with
    //  a pointer test around that store, sent the register allocator into scratch: 872 bytes, 45 -> 73 us per launch.)
    const bool fast = m0 + BT <= g.M && n0 + BTN <= g.N && g.beta != 0.f && g.Ct && (!g.s3 || g.s3mode == 3);
    if (fast && g.s3 && !g.s3t && g.cth) epilogue(std::integral_constant<int, NO32 ? 4 : 1>());
    else if (fast && !g.s3 && g.cth) epilogue(std::integral_constant<int, NO32 ? 5 : 2>());
    else if (fast && g.s3 && g.s3t && !g.cth) epilogue(std::integral_constant<int, 3>());
    else epilogue(std::integral_constant<int, 0>());
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int n = n0 + wc * 16 * NJ + j * 16 + i16;
      if (n >= g.N) continue;
      const float e[4] = {acc[i][j].x, acc[i][j].y, acc[i][j].z, acc[i][j].w};
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = m0 + wr * 64 + i * 16 + 4 * kg + r;
        if (m >= g.M) continue;
        float *cp = g.Cm + (size_t)m * g.ldc + n;
        *cp = g.beta != 0.f ? g.beta * *cp + e[r] : e[r];
      }
    }
}

// NT form on the same tiles: C = A B^T (+ bias), A [M x K] and B [N x K] both k-contiguous (the batched x-projection :246
// in bf16 operand mode: x rows against W_gifo_x rows).  A thread fetches 8 consecutive k of one row (two 16-byte loads), rounds
// to bf16 and writes the four (k, k+1) words as ONE 16-byte store into the same LDS layout (LDQ % 4 == 0).
__device__ __forceinline__ void fetch_row8(const float *__restrict__ P, int ld, int X, int K, int x0, int k0, int u,
                                           float4 (&r)[2], int &ok) {
  const int x = x0 + (u >> 3), k = k0 + 8 * (u & 7);
  ok = x < X && k + 8 <= K;                          // K % 8 == 0 on this path
  const float *p = P + (size_t)(ok ? x : 0) * ld + (ok ? k : 0);
  r[0] = ldg4(p); r[1] = ldg4(p + 4);
}
__device__ __forceinline__ void stash_row8(unsigned *Ls, int u, const float4 (&rr)[2], int ok) {
  const float4 r[2] = {keep_if(rr[0], ok != 0), keep_if(rr[1], ok != 0)};
  const int xl = u >> 3;
  uint4 w;
  w.x = pack_pair(r[0].x, r[0].y); w.y = pack_pair(r[0].z, r[0].w);
  w.z = pack_pair(r[1].x, r[1].y); w.w = pack_pair(r[1].z, r[1].w);
  *reinterpret_cast<uint4 *>(Ls + (xl & 3) * PLANE + (xl >> 2) * LDQ + 4 * (u & 7)) = w;
}
// NJ: 16-column blocks per wave (4: 128-column tiles; 2: 64-column tiles -- twice the workgroups for results with few tiles)
// Split K (launch_gemm_bf16_nt_splitk): blockIdx.y = K slice of g.kslice columns (0: the whole K), its partial tile goes to slab
// blockIdx.y of g.Cm ([slices][M x N], dense); k_splitk_reduce adds the slabs in order.
template <int NJ>
__global__ __launch_bounds__(256) void k_gemm_bf16_nt(GemmJob g) {
  if (g.kslice > 0) {
    const int k0 = (int)blockIdx.y * g.kslice;
    g.A += k0; g.B += k0;
    g.K = g.K - k0 < g.kslice ? g.K - k0 : g.kslice;
    g.Cm += (size_t)blockIdx.y * g.M * g.N;
  }
  constexpr int BTN = 32 * NJ;
  __shared__ __attribute__((aligned(16))) unsigned As[4 * PLANE];
  __shared__ __attribute__((aligned(16))) unsigned Bs[4 * PLANE];
  const int ntm = (g.M + BT - 1) / BT, ntn = (g.N + BTN - 1) / BTN, nt = ntm * ntn;
  const int cpx = (nt + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * cpx + (int)(blockIdx.x >> 3);     // XCD x: a contiguous n-major range (A is small, B streams once)
  if (b >= nt) return;
  const int m0 = (b % ntm) * BT, n0 = (b / ntm) * BTN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  f32x4 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[i][j] = (f32x4){0, 0, 0, 0};
  constexpr int NU = BT * (BK / 8) / 256, NUB = BTN * (BK / 8) / 256;   // (row, 8-k group) units per thread: A, B
  float4 ra[NU][2], rb[NUB][2];
  int oa[NU], ob[NUB];
#pragma unroll
  for (int h = 0; h < NU; h++) fetch_row8(g.A, g.lda, g.M, g.K, m0, 0, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
  for (int h = 0; h < NUB; h++) fetch_row8(g.B, g.ldb, g.N, g.K, n0, 0, tid + 256 * h, rb[h], ob[h]);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
#pragma unroll
    for (int h = 0; h < NU; h++) stash_row8(As, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
    for (int h = 0; h < NUB; h++) stash_row8(Bs, tid + 256 * h, rb[h], ob[h]);
    __syncthreads();
    if (k0 + BK < g.K) {
#pragma unroll
      for (int h = 0; h < NU; h++) fetch_row8(g.A, g.lda, g.M, g.K, m0, k0 + BK, tid + 256 * h, ra[h], oa[h]);
#pragma unroll
      for (int h = 0; h < NUB; h++) fetch_row8(g.B, g.ldb, g.N, g.K, n0, k0 + BK, tid + 256 * h, rb[h], ob[h]);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ks++) {
      bf16x8 af[4], bfr[NJ];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int xa = wr * 64 + i * 16 + i16;
        af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(As + (xa & 3) * PLANE + (xa >> 2) * LDQ + ks * 16 + kg * 4));
      }
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int xb = wc * 16 * NJ + j * 16 + i16;
        bfr[j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(Bs + (xb & 3) * PLANE + (xb >> 2) * LDQ + ks * 16 + kg * 4));
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // lane (i16, kg): rows 4kg + (0..3) of block i at column i16 of block j: 16 lanes = 64 contiguous bytes per row
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int n = n0 + wc * 16 * NJ + j * 16 + i16;
    if (n >= g.N) continue;
    const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float e[4] = {acc[i][j].x, acc[i][j].y, acc[i][j].z, acc[i][j].w};
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = m0 + wr * 64 + i * 16 + 4 * kg + r;
        if (m >= g.M) continue;
        g.Cm[(size_t)m * g.ldc + n] = e[r] + bv + (g.beta != 0.f ? g.beta * g.Cm[(size_t)m * g.ldc + n] : 0.f);
        if (g.C2) g.C2[(size_t)m * g.ldc2 + n] = e[r] + bv;            // (the batched projection: rr rows, output rows, carried r)
        if (g.C3 && m >= g.tail0) g.C3[(size_t)(m - g.tail0) * g.N + n] = e[r] + bv;
      }
    }
  }
}

// NARROW: 128 x 64 tiles as an instance of their own -- half the accumulators and B staging registers: three waves per SIMD instead of two,
// so that twice the tiles are still all resident (a tile is a chain of dependent memory round trips: residency is what counts)
template <bool NO32, bool NARROW = false>
__global__ __launch_bounds__(256, NARROW ? 3 : 2) void k_grads_bf16(GradsArgs a) {
  const bool invalid = a.guard && (a.guard[2] | a.guard[6] | a.guard[9]);
  if (a.mark && blockIdx.x == 0 && threadIdx.x == 0) *a.mark = invalid ? 1.f : 0.f;
  if (invalid) return;   // a persistent launch of this minibatch gave up: leave momentum and parameters alone
  __shared__ __attribute__((aligned(16))) unsigned As[4 * PLANE];
  __shared__ __attribute__((aligned(16))) unsigned Bs[4 * PLANE];
  const int nbt = a.nb2 + a.nvec;
  const int cpx = (nbt + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * cpx + (int)(blockIdx.x >> 3);
  if (b >= nbt) return;
  if (b < a.nb2) {
    const GemmJob &g = b < a.nb0 ? a.wx : b < a.nb1 ? a.wr : a.wm;
    const int lb = b < a.nb0 ? b : b < a.nb1 ? b - a.nb0 : b - a.nb1;
    if constexpr (NARROW) {
      const int ntn = (g.N + BT / 2 - 1) / (BT / 2);
      gemm_tile_bf16_tn<2, NO32>(g, (lb / ntn) * BT, (lb % ntn) * (BT / 2), As, Bs);
    } else {
      const int ntn = (g.N + BT - 1) / BT;
      gemm_tile_bf16_tn<4, NO32>(g, (lb / ntn) * BT, (lb % ntn) * BT, As, Bs);
    }
    return;
  }
  grads_column_sums(a, b - a.nb2, reinterpret_cast<float *>(As), reinterpret_cast<float *>(Bs));
}

// ---------------------------------------------------------------------------------------------
// Update (:504-512) fused with the refresh of the transposed copies the backward kernels read.
// 32x32 tiles of the three matrices (+ 1024-element chunks of the vector parameters).
// ---------------------------------------------------------------------------------------------
struct UpdArgs {
  const unsigned *guard;   // as in GradsArgs
  const float *mark;       // (or null) the validity word behind the all-reduced gradient blob: non-zero = some rank's gradient of this minibatch was not real
  unsigned *peer_skip;     // (or null) counts the Updates that were left out for that reason
  float *param, *corr;
  const float *grad;        // DP: corr = mmt*corr + grad first
  float mmt, lr, clip;
  int touch;                // 0: pure repack (no corr / param writes)
  // three matrices: offset into blob, rows, cols, transposed destination
  long off[3]; int rows[3], cols[3]; float *dstT[3];
  int tb[3];                // first block of matrix i;  vector blocks start at tb_vec
  int tb_vec;
  long voff, vlen;          // vector parameters (bias + 3 peepholes) are contiguous in the blob
  // optional (vector kernel): the three bf16 planes of the fold operands, written from the same tiles (klstm_fold3.hip):
  // a3 in W_gifo_r's own layout (matrix 1), b3 in W_r_m^T's (matrix 2, the transposed destination's)
  unsigned short *a3, *b3; long a_plane, b_plane; int split_mode;
  unsigned short *dstTh[3];  // (or null; vector kernel) bf16 copies (RNE) of the transposed destinations, same layout
};

__device__ __forceinline__ float upd_elem(const UpdArgs &a, long idx) {
  float p = a.param[idx];
  if (a.touch) {
    float c = a.corr[idx];
    if (a.grad) c = a.mmt * c + a.grad[idx];
    if (a.clip > 0.f) { c = c < -a.clip ? -a.clip : c; c = c > a.clip ? a.clip : c; }
    if (a.grad || a.clip > 0.f) a.corr[idx] = c;
    p = p + (-a.lr) * c;
    a.param[idx] = p;
  }
  return p;
}

__global__ __launch_bounds__(256) void k_update_repack(UpdArgs a) {
  // a persistent launch of this minibatch gave up: leave momentum and parameters alone -- on THIS rank (guard) or on ANY rank (the
  // reduced validity word: every rank leaves this Update out, the replicas stay identical; counted, the same number everywhere)
  const bool own = a.guard && (a.guard[2] | a.guard[6] | a.guard[9]);
  if (own || (a.mark && *a.mark != 0.f)) {
    if (a.mark && a.peer_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.peer_skip, 1u);
    return;
  }
  __shared__ float tile[32][33];
  const int b = blockIdx.x, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (b >= a.tb_vec) {
    const long base = (long)(b - a.tb_vec) * 1024;
    for (int j = threadIdx.x; j < 1024; j += 256)
      if (base + j < a.vlen) (void)upd_elem(a, a.voff + base + j);
    return;
  }
  const int mi = b >= a.tb[2] ? 2 : b >= a.tb[1] ? 1 : 0;
  const int rows = a.rows[mi], cols = a.cols[mi];
  const int lb = b - a.tb[mi];
  const int ntc = (cols + 31) / 32;
  const int by = (lb / ntc) * 32, bx = (lb % ntc) * 32;
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    tile[j][tx] = (r < rows && c < cols) ? upd_elem(a, a.off[mi] + (long)r * cols + c) : 0.f;
  }
  __syncthreads();
  float *dst = a.dstT[mi];
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;     // dst[c][r]
    if (dst && c < cols && r < rows) dst[(size_t)c * rows + r] = tile[tx][j];
  }
}

// The same on 64x64 tiles with 16-byte accesses everywhere (cols and rows multiples of 4, 16-byte aligned blobs): every
// thread takes four float4 pieces of a tile row-wise (256 contiguous bytes per tile row), the updated tile goes through LDS
// and leaves transposed as float4 pieces along the row axis.  k_update_repack's 4-byte accesses in 128-byte segments
// reach ~4 TB/s of the 35 MB it moves; this form ~6.
// the three 16-byte loads of one piece, and the arithmetic + stores on them: a tile's four pieces are all requested before the first
// store (a load behind a store waits for it -- the compiler cannot know that the rows do not overlap)
struct UpdPiece { float4 p, c, g; };
__device__ __forceinline__ UpdPiece upd_vec_load(const UpdArgs &a, long idx) {
  UpdPiece q;
  q.p = *reinterpret_cast<const float4 *>(a.param + idx);
  q.c = a.touch ? *reinterpret_cast<const float4 *>(a.corr + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
  q.g = a.touch && a.grad ? *reinterpret_cast<const float4 *>(a.grad + idx) : make_float4(0.f, 0.f, 0.f, 0.f);
  return q;
}
__device__ __forceinline__ float4 upd_vec_apply(const UpdArgs &a, long idx, const UpdPiece &q) {
  float4 p = q.p;
  if (a.touch) {
    float cv[4] = {q.c.x, q.c.y, q.c.z, q.c.w};
    if (a.grad) {
      const float4 g = q.g;
      cv[0] = a.mmt * cv[0] + g.x; cv[1] = a.mmt * cv[1] + g.y; cv[2] = a.mmt * cv[2] + g.z; cv[3] = a.mmt * cv[3] + g.w;
    }
    if (a.clip > 0.f) {
#pragma unroll
      for (int q_ = 0; q_ < 4; q_++) { cv[q_] = cv[q_] < -a.clip ? -a.clip : cv[q_]; cv[q_] = cv[q_] > a.clip ? a.clip : cv[q_]; }
    }
    if (a.grad || a.clip > 0.f) *reinterpret_cast<float4 *>(a.corr + idx) = make_float4(cv[0], cv[1], cv[2], cv[3]);
    p.x = p.x + (-a.lr) * cv[0]; p.y = p.y + (-a.lr) * cv[1]; p.z = p.z + (-a.lr) * cv[2]; p.w = p.w + (-a.lr) * cv[3];
    *reinterpret_cast<float4 *>(a.param + idx) = p;
  }
  return p;
}

__global__ __launch_bounds__(256) void k_update_repack_v(UpdArgs a) {
  // a persistent launch of this minibatch gave up: leave momentum and parameters alone -- on THIS rank (guard) or on ANY rank (the
  // reduced validity word: every rank leaves this Update out, the replicas stay identical; counted, the same number everywhere)
  const bool own = a.guard && (a.guard[2] | a.guard[6] | a.guard[9]);
  if (own || (a.mark && *a.mark != 0.f)) {
    if (a.mark && a.peer_skip && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.peer_skip, 1u);
    return;
  }
  __shared__ __attribute__((aligned(16))) float tile[64 * 68];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.tb_vec) {
    const long base = (long)(b - a.tb_vec) * 1024;
    for (int j = tid; j < 1024; j += 256)
      if (base + j < a.vlen) (void)upd_elem(a, a.voff + base + j);
    return;
  }
  const int mi = b >= a.tb[2] ? 2 : b >= a.tb[1] ? 1 : 0;
  const int rows = a.rows[mi], cols = a.cols[mi];
  const int lb = b - a.tb[mi];
  const int ntc = (cols + 63) / 64;
  const int by = (lb / ntc) * 64, bx = (lb % ntc) * 64;
  UpdPiece piece[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int p = tid + 256 * u, r = by + (p >> 4), c = bx + (p & 15) * 4;
    piece[u] = upd_vec_load(a, a.off[mi] + (r < rows && c + 4 <= cols ? (long)r * cols + c : 0));
  }
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int p = tid + 256 * u, rl = p >> 4, cq = (p & 15) * 4;
    const int r = by + rl, c = bx + cq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows && c + 4 <= cols) {
      v = upd_vec_apply(a, a.off[mi] + (long)r * cols + c, piece[u]);
      if (mi == 1 && a.a3) {
        const float v4[4] = {v.x, v.y, v.z, v.w};
        split_store4(a.split_mode, v4, a.a3 + (size_t)r * cols + c, a.a_plane);
      }
    }
    *reinterpret_cast<float4 *>(tile + rl * 68 + cq) = v;
  }
  __syncthreads();
  float *dst = a.dstT[mi];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int p = tid + 256 * u, cl = p >> 4, rq = (p & 15) * 4;
    const int c = bx + cl, r = by + rq;       // dst[c][r .. r+3]
    if (c < cols && r + 4 <= rows) {
      const float *tp = tile + rq * 68 + cl;
      const float v4[4] = {tp[0], tp[68], tp[2 * 68], tp[3 * 68]};
      if (dst) *reinterpret_cast<float4 *>(dst + (size_t)c * rows + r) = make_float4(v4[0], v4[1], v4[2], v4[3]);   // (null: only the bf16 copy has a reader)
      if (mi == 2 && a.b3) split_store4(a.split_mode, v4, a.b3 + (size_t)c * rows + r, a.b_plane);
      if (a.dstTh[mi]) split_store4(3, v4, a.dstTh[mi] + (size_t)c * rows + r, 0);
    }
  }
}

// C = beta C + add + A B^T with K split into ks slices of klen (a multiple of 64): the partial products go to ws ([ks][M x N] floats),
// k_splitk_reduce adds them in slice order.  For few output tiles and a long K (640 x 512 over K = 4096: 40 tiles of 128 x 64 took 80 us).
hipError_t launch_gemm_bf16_nt_splitk(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float beta, float *Cm, int ldc,
                                      const float *add, int add_ld, float *ws, int ks, int klen, hipStream_t st, LaunchProbe pr, LaunchProbe pr2) {
  GemmJob g = make_job(false, true, M, N, K, A, lda, B, ldb, 0.f, ws, N, nullptr);
  g.kslice = klen;
  auto first = [&]() -> hipError_t {
    if (N % 32 == 0) {                                // (128 x 32 tiles: more workgroups per CU to cover the load latency of a K tile)
      const int nt1 = cdiv(M, BT) * cdiv(N, BT / 4);
      return launch(k_gemm_bf16_nt<1>, dim3(cdiv(nt1, 8) * 8, ks), dim3(256), 0, st, pr, g);
    }
    const int ntm = cdiv(M, BT), ntn = cdiv(N, BT / 2), nt = ntm * ntn;
    return launch(k_gemm_bf16_nt<2>, dim3(cdiv(nt, 8) * 8, ks), dim3(256), 0, st, pr, g);
  };
  hipError_t err = first();
  if (err != hipSuccess) return err;
  ReduceArgs r;
  r.ws = ws; r.ks = ks; r.M = M; r.N = N; r.beta = beta; r.Cm = Cm; r.ldc = ldc; r.add = add; r.add_ld = add_ld;
  const long nb = ((long)M * N + 255) / 256;
  return launch(k_splitk_reduce, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(256), 0, st, pr2, r);
}
// C = A B^T + bias with both operands rounded to bf16 (bf16 operand mode; M >= GRADS_BF16_MIN_ROWS rows, K >= 128 -- at K = 40 the
// 64x64 fp32 tiles are faster: 9.8 vs 12.1 us at 640 x 4096 --, K % 8 == 0, 16-byte aligned rows)
bool gemm_bf16_nt_supported(int M, int K, const float *A, int lda, const float *B, int ldb) {
  return M >= GRADS_BF16_MIN_ROWS && K >= 128 && K % 8 == 0 && lda % 4 == 0 && ldb % 4 == 0 && aligned16(A) && aligned16(B);
}
hipError_t launch_gemm_bf16_nt(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *Cm, int ldc,
                               const float *bias, hipStream_t st, LaunchProbe pr, float *C2, int ldc2, float *C3, int tail0, float beta) {
  GemmJob g = make_job(false, true, M, N, K, A, lda, B, ldb, beta, Cm, ldc, bias);
  g.C2 = C2; g.ldc2 = ldc2; g.C3 = C3; g.tail0 = tail0;
  const dim3 block(256);
  if (cdiv(N, BT / 2) * cdiv(M, BT) < 512 && N % 32 == 0) {   // few 128 x 64 tiles too: 128 x 32 -- every K tile of 64 exposes a memory latency, more
    const dim3 grid(cdiv(cdiv(N, BT / 4) * cdiv(M, BT), 8) * 8);   // workgroups per CU cover it (640 x 1024 over K = 512: 15.9 -> 11 us; 640 x 4096: no change)
    return launch(k_gemm_bf16_nt<1>, grid, block, 0, st, pr, g);
  }
  if (cdiv(N, BT) * cdiv(M, BT) < 384) {             // few 128 x 128 tiles (640 x 4096: 160 on 256 CUs): 128 x 64
    const dim3 grid(cdiv(cdiv(N, BT / 2) * cdiv(M, BT), 8) * 8);
    return launch(k_gemm_bf16_nt<2>, grid, block, 0, st, pr, g);
  }
  const dim3 grid(cdiv(cdiv(N, BT) * cdiv(M, BT), 8) * 8);
  return launch(k_gemm_bf16_nt<4>, grid, block, 0, st, pr, g);
}

bool grads_bf16_tiles(const Dims &d, bool bf16) { return bf16 && d.T * d.S >= GRADS_BF16_MIN_ROWS; }

hipError_t launch_grads(const Dims &d, const float *dgifo, const float *dr, const float *in, int in_stride,
                        const float *rr, const float *mm, const float *cc, float beta, float *dst,
                        hipStream_t st, LaunchProbe pr, bool bf16, const GradsUpdate *upd, const unsigned *guard, float *mark,
                        const TailReduceJob *tr) {
  const int S = d.S, C = d.C, R = d.R, I = d.I, TS = d.T * d.S;
  const long o_wx = 0, o_wr = (long)4 * C * I, o_b = o_wr + (long)4 * C * R, o_pi = o_b + 4 * C,
             o_pf = o_pi + C, o_po = o_pf + C, o_wm = o_po + C;
  const float *dg1 = dgifo + (size_t)S * 4 * C;                      // DGIFO[1..T]
  GradsArgs a;
  a.guard = guard;
  a.mark = mark;
  a.bf16_narrow = 0;
  a.wx = make_job(true, false, 4 * C, I, TS, dg1, 4 * C, in, in_stride, beta, dst + o_wx, I, nullptr);             // :468
  a.wr = make_job(true, false, 4 * C, R, TS, dg1, 4 * C, rr, R, beta, dst + o_wr, R, nullptr);                      // :471 (YR[0..T-1])
  a.wm = make_job(true, false, R, C, TS, dr + (size_t)S * R, R, mm + (size_t)S * C, C, beta, dst + o_wm, C, nullptr); // :486
  a.nb0 = cdiv(4 * C, GT) * cdiv(I, GT);
  a.nb1 = a.nb0 + cdiv(4 * C, GT) * cdiv(R, GT);
  a.nb2 = a.nb1 + cdiv(R, GT) * cdiv(C, GT);
  a.C = C; a.S = S; a.T = d.T; a.dgifo = dgifo; a.cc = cc; a.beta = beta;
  a.g_bias = dst + o_b; a.g_pi = dst + o_pi; a.g_pf = dst + o_pf; a.g_po = dst + o_po;
  a.p_bias = a.p_pi = a.p_pf = a.p_po = nullptr; a.lr = 0.f; a.clip = 0.f;
  if (upd) {                                          // Update folded into the same pass (fp32 tiles and bf16 tiles alike)
    float *pb = upd->params;
    a.wx.P = pb + o_wx; a.wr.P = pb + o_wr; a.wm.P = pb + o_wm;
    a.wx.lr = a.wr.lr = a.wm.lr = a.lr = upd->lr;
    a.wx.clip = a.wr.clip = a.wm.clip = a.clip = upd->clip;
    a.wx.Ct = upd->wxT; a.wx.ldct = 4 * C;           // [I x 4C]
    a.wr.Ct = upd->wrT; a.wr.ldct = 4 * C;           // [R x 4C]
    a.wm.Ct = upd->wmT; a.wm.ldct = R;               // [C x R]
    if (upd->a3) { a.wr.s3 = upd->a3; a.wr.s3pl = upd->a_plane; a.wr.s3t = 0; a.wr.s3mode = upd->split_mode; }
    if (upd->b3) { a.wm.s3 = upd->b3; a.wm.s3pl = upd->b_plane; a.wm.s3t = 1; a.wm.s3mode = upd->split_mode; }
    a.wx.cth = upd->wxTh; a.wr.cth = upd->wrTh;      // (null: none)
    a.p_bias = pb + o_b; a.p_pi = pb + o_pi; a.p_pf = pb + o_pf; a.p_po = pb + o_po;
  }
  if (!upd && aligned16(dst) && C % 4 == 0 && R % 4 == 0 && I % 4 == 0) a.wx.coal = a.wr.coal = a.wm.coal = 1;
  a.nvec = cdiv(4 * C, 64);
  // below ~256 frames per minibatch the products are write-bound and the 64x64 fp32 tiles are faster (80 frames: 13.4 vs
  // 16.5 us); from there on the bf16 tiles win (640 frames at 512/1024/512: 99 -> 55 us)
  const bool bf_ok = bf16 && TS >= GRADS_BF16_MIN_ROWS && aligned16(dgifo) && aligned16(dr) && aligned16(in) && aligned16(rr) && aligned16(mm) &&
                     in_stride % 4 == 0 && C % 4 == 0 && R % 4 == 0 && I % 4 == 0;
  if (bf_ok && upd && !(aligned16(dst) && aligned16(upd->params) && aligned16(upd->wrT) && aligned16(upd->wmT) && aligned16(upd->wxT)))
    return hipErrorInvalidValue;                      // (the fused epilogue moves 16-byte pieces; the engine's blobs are aligned)
  if (bf_ok && tr) return hipErrorInvalidValue;       // (the merged reduction rides on the fp32 tiles only)
  if (bf_ok) {                                        // 128x128 tiles on the bf16 pipe
    // 128 x 64 tiles while 128 x 128 ones would not even give every CU a workgroup (measured at 1024/512, 640 frames: 192 tiles
    // (40 inputs) 24.8 -> 21.3 us; 288 tiles (512 inputs) 30 -> 33.5 us: stays wide)
    // ... and, round 6, whenever the 128 x 64 tiles are ALL resident at the three waves per SIMD their own kernel instance runs at (768
    // workgroups): every tile is a chain of dependent memory round trips, so half the epilogue per tile with every tile in flight wins --
    // 576 tiles at 512 inputs: 41.9 -> 38-39 us per layer, configs[4] 0.659 -> 0.649 ms (A-B of builds, profiles/r06_grads_bf16_narrow_ab.txt;
    // the measurement above was taken when both widths shared one kernel at two waves per SIMD: 576 tiles in 512 slots)
    const int narrow_tiles = cdiv(4 * C, BT) * (cdiv(I, BT / 2) + cdiv(R, BT / 2)) + cdiv(R, BT) * cdiv(C, BT / 2);
    a.bf16_narrow = (cdiv(4 * C, BT) * (cdiv(I, BT) + cdiv(R, BT)) + cdiv(R, BT) * cdiv(C, BT) < 256 || narrow_tiles + a.nvec <= 768) ? 1 : 0;
    const int btn = a.bf16_narrow ? BT / 2 : BT;
    a.nb0 = cdiv(4 * C, BT) * cdiv(I, btn);
    a.nb1 = a.nb0 + cdiv(4 * C, BT) * cdiv(R, btn);
    a.nb2 = a.nb1 + cdiv(R, BT) * cdiv(C, btn);
    if (a.bf16_narrow) {
      if (upd && upd->no_wT32) return launch((k_grads_bf16<true, true>), dim3(cdiv(a.nb2 + a.nvec, 8) * 8), dim3(256), 0, st, pr, a);
      return launch((k_grads_bf16<false, true>), dim3(cdiv(a.nb2 + a.nvec, 8) * 8), dim3(256), 0, st, pr, a);
    }
    if (upd && upd->no_wT32) return launch(k_grads_bf16<true>, dim3(cdiv(a.nb2 + a.nvec, 8) * 8), dim3(256), 0, st, pr, a);
    return launch(k_grads_bf16<false>, dim3(cdiv(a.nb2 + a.nvec, 8) * 8), dim3(256), 0, st, pr, a);
  }
  if (tr) {   // the reduction of the tail workgroups' partial rows on the first workgroups of this launch
    if (!(a.wm.vecA && a.wm.vecB) || !tr->ctr || !tr->tws) return hipErrorInvalidValue;   // (16-byte rows: the engine's own buffers)
    a.tr = *tr; a.nred = tail_reduce_blocks(*tr); a.tr_target = tr->target;
    return launch(k_grads_tm, dim3(a.nred + 8 * (cdiv(a.nb1, 8) + cdiv(a.nb2 + a.nvec - a.nb1, 8))), dim3(256), 0, st, pr, a);
  }
  return launch(k_grads, dim3(cdiv(a.nb2 + a.nvec, 8) * 8), dim3(256), 0, st, pr, a);
}

bool update_repack_vectorised(const Dims &d, const float *param_blob, const float *corr_blob, const float *grad_blob, const float *wrT,
                              const float *wmT, const float *wxT) {
  return d.C % 4 == 0 && d.R % 4 == 0 && d.I % 4 == 0 && aligned16(param_blob) && aligned16(corr_blob) &&
         (!grad_blob || aligned16(grad_blob)) && aligned16(wrT) && aligned16(wmT) && aligned16(wxT);
}
hipError_t launch_update_repack(const Dims &d, float *param_blob, float *corr_blob, const float *grad_blob,
                                float mmt, float lr, float clip, float *wrT, float *wmT, float *wxT,
                                hipStream_t st, LaunchProbe pr, const unsigned *guard, const GradsUpdate *planes, const float *mark,
                                unsigned *peer_skip) {
  const int C = d.C, R = d.R, I = d.I;
  UpdArgs a;
  a.guard = guard;
  a.mark = mark; a.peer_skip = peer_skip;
  a.a3 = a.b3 = nullptr; a.a_plane = a.b_plane = 0; a.split_mode = 1;
  a.dstTh[0] = a.dstTh[1] = a.dstTh[2] = nullptr;
  a.param = param_blob; a.corr = corr_blob; a.grad = grad_blob; a.mmt = mmt; a.lr = lr; a.clip = clip;
  a.touch = (lr != 0.f || grad_blob != nullptr || clip > 0.f) ? 1 : 0;
  const long o_wr = (long)4 * C * I, o_b = o_wr + (long)4 * C * R, o_wm = o_b + 7 * C;
  a.off[0] = 0;    a.rows[0] = 4 * C; a.cols[0] = I; a.dstT[0] = wxT;
  a.off[1] = o_wr; a.rows[1] = 4 * C; a.cols[1] = R; a.dstT[1] = wrT;
  a.off[2] = o_wm; a.rows[2] = R;     a.cols[2] = C; a.dstT[2] = wmT;
  a.voff = o_b; a.vlen = 7 * C;
  const bool vec = update_repack_vectorised(d, param_blob, corr_blob, grad_blob, wrT, wmT, wxT);
  const int tsz = vec ? 64 : 32;
  int nb = 0;
  for (int i = 0; i < 3; i++) { a.tb[i] = nb; nb += cdiv(a.rows[i], tsz) * cdiv(a.cols[i], tsz); }
  a.tb_vec = nb;
  nb += cdiv(7 * C, 1024);
  if (vec && planes) {
    a.a3 = planes->a3; a.b3 = planes->b3; a.a_plane = planes->a_plane; a.b_plane = planes->b_plane; a.split_mode = planes->split_mode;
    a.dstTh[0] = planes->wxTh; a.dstTh[1] = planes->wrTh;
  }
  if (vec) return launch(k_update_repack_v, dim3(nb), dim3(256), 0, st, pr, a);
  return launch(k_update_repack, dim3(nb), dim3(256), 0, st, pr, a);
}

}  // namespace klstm
