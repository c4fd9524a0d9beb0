// kaldi-lstm_amd/csrc/klstm_kernels.hip -- hand-written gfx950 (CDNA4) step kernels of the
// LstmProjectedStreams hot path.  fp32 throughout (Kaldi BaseFloat); every contraction runs on
// the f32-input MFMA  v_mfma_f32_16x16x4_f32  (exact fp32 FMA chain, 157 TF peak), 64-wide waves.
//
// What each kernel replaces in the reference (google/nnet/bd-nnet-lstm-projected-streams.h):
//   k_gates_step : per-step  AddMatMat(r(t-1),W_gifo_r^T) + 2x AddMatDiagVec + Sigmoid x3 + Tanh x2 +
//                  3x AddMatDotMat + ApplyFloor/Ceiling (:275-309, 14 launches); optionally also the
//                  x(t) W_gifo_x^T + bias term (:246,:259) and the state bridge copies (:231,:331)
//   k_proj_step  : per-step  y_r = y_m * W_r_m^T (:312) + the copy into `out` (:328)
//   k_dr_step    : per-step  d_r += DGIFO(t+1) * W_gifo_r (:391) and in_diff(t+1) = DGIFO(t+1) * W_gifo_x
//                  (:457), split-K partial slabs
//   k_dm_step    : per-step  d_m = d_r * W_r_m (:408) + the 15 elementwise launches (:411-440)
// (The tile GEMMs and the weight packing are klstm_gemm.hip, klstm_gemm_dev.h; the gradient launch, the bf16 tiles and Update
// klstm_grads.hip; the output tail -- time shift, softmax / xent rows, column sums, element-wise updates -- klstm_output.hip.)
//
// The recurrence is latency-bound at small NumStream (a dependent kernel boundary costs ~1.6 us on
// this chip, a dependent HBM/L2 round trip 0.5-1 us), so every step kernel is written to make
// exactly ONE memory round trip: all weight / activation / epilogue operands are requested before
// the first MFMA issues.
//
// Skinny-GEMM layout of the step kernels ("weights on M, streams on N"):
//   D[16 weight rows][16 streams] += A[row][k] * B[k][stream],  A lane l: row l&15, k-group l>>4;
//   a lane loads 8 consecutive k (two dwordx4) of its weight row / stream row per 32-wide K chunk
//   and feeds them to 8 MFMAs; the 8 waves of a workgroup split K, partial tiles are summed in a
//   fixed order through LDS (deterministic), and the fused LSTM cell math runs on the summed tile
//   in registers.  D lane l holds stream l&15, rows 4*(l>>4)+{0..3}.
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_step_dev.h"

#include <stdint.h>

namespace klstm {

#pragma clang fp contract(off)

// ---- tile geometry ---------------------------------------------------------------------------------
// SMALL = false: v_mfma_f32_16x16x4_f32, D[16 rows][16 streams]; lane l feeds A row l&15 / B stream l&15
//                of k-group l>>4 and receives rows 4*(l>>4)+{0..3} of stream l&15.
// SMALL = true : NumStream <= 4.  v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4x1 blocks, same FLOP rate):
//                block b = lane>>2 is used as (row group b&3, k-group b>>2), so a lane feeds the SAME A
//                element as above (row l&15, k-group l>>4) but B stream l&3, and receives rows
//                4*((l>>2)&3)+{0..3} of stream l&3 for ITS k-group; the 4 k-groups are added in the
//                fixed-order LDS combine.  No lanes are wasted on padding streams (4x fewer MFMA cycles).
template <bool SMALL> struct Geo {
  static constexpr int STREAMS = SMALL ? 4 : 16;                       // streams per MFMA tile
  __device__ static __forceinline__ int bstream(int lane) { return SMALL ? (lane & 3) : (lane & 15); }
  __device__ static __forceinline__ int q(int lane) { return SMALL ? ((lane >> 2) & 3) : (lane >> 4); }
  __device__ static __forceinline__ bool owner(int lane) { return SMALL ? lane < 16 : true; }
  __device__ static __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
    if (SMALL) return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
};

// Sum the per-wave partial tiles of s-tile `nt` in a fixed order.
template <int NT, bool SMALL>
__device__ __forceinline__ f32x4 reduce_tile(const f32x4 (*red)[NT][64], int nt, int lane) {
  f32x4 v = red[0][nt][lane];          // SMALL: the k-groups were already combined in-wave (VEC_COMBINE)
#pragma unroll
  for (int w = 1; w < NW; w++) v += red[w][nt][lane];
  return v;
}

// K loop shared by the step kernels.  nch chunks of 32 are dealt round-robin to the NW waves; CPW
// chunks per wave are fetched (A and every B tile) before any MFMA so that all loads of a
// super-iteration are in flight together.  afetch(ch, on, av) / bfetch(ch, nt, on, bv) fill 8 floats;
// bpost(ch, nt, on, bv) runs after the MFMAs (side stores of the fetched B operand).
template <int NT, int CPW, bool SMALL, class AF, class BF, class BP>
__device__ __forceinline__ void mma_k_loop(int nch, int wave, f32x4 (&acc)[NT][2], const AF &afetch,
                                           const BF &bfetch, const BP &bpost) {
  for (int base = 0; base < nch; base += CPW * NW) {
    float av[CPW][8];
    float bv[CPW][NT][8];
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      const int ch = base + wave + c * NW;
      const bool on = ch < nch;
      afetch(ch, on, av[c]);
#pragma unroll
      for (int nt = 0; nt < NT; nt++) bfetch(ch, nt, on, bv[c][nt]);
    }
#pragma unroll
    for (int c = 0; c < CPW; c++)
#pragma unroll
      for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[nt][j & 1] = Geo<SMALL>::mma(av[c][j], bv[c][nt][j], acc[nt][j & 1]);
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      const int ch = base + wave + c * NW;
#pragma unroll
      for (int nt = 0; nt < NT; nt++) bpost(ch, nt, ch < nch, bv[c][nt]);
    }
  }
}
struct NoPost { template <class... A> __device__ __forceinline__ void operator()(A &&...) const {} };

// GENERIC kernels (any shape; used when R, I or C is not a multiple of 8): per-element guarded loads straight
// from the natural layouts, 16x16x4 geometry, one K chunk per wave per iteration.
#define GENERIC_GEOMETRY() constexpr int CPW = 1; constexpr bool VEC = false, SMALL = false

#define STEP_PROLOGUE()                                                                          \
  const int lane = threadIdx.x & 63;                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                             \
  const int i16 = lane & 15, kg = lane >> 4;                                                     \
  const int bs = Geo<SMALL>::bstream(lane), q = Geo<SMALL>::q(lane);                             \
  constexpr int TS_ = Geo<SMALL>::STREAMS;                                                       \
  (void)i16; (void)kg; (void)bs; (void)q

// ---------------------------------------------------------------------------------------------
// forward step 1/2: gates + cell.  One workgroup = 4 cells x 4 gates (16 weight rows) x NT stream tiles.
// tile row i -> (cell c0 + i/4, gate i%4) so that after the MFMA a lane owns g,i,f,o of ONE
// (cell, stream) pair in its four accumulator registers and the cell math is lane-local.
// ---------------------------------------------------------------------------------------------
struct GatesArgs {
  int C, R, S, I, t;
  const float *wr, *wx, *bias, *pi, *pf, *po;
  float *gifo, *cc, *hh, *mm;
  const float *cprev, *rprev;     // c(t-1) [S x C], r(t-1) [S x R]
  const float *x; int x_stride;   // frame-t input rows [S x I] (FUSEX)
  float *c_mirror, *r_mirror;     // time block 0 of cc / rr at t == 1 (BPTT reads them), else null
  float *c_save;                  // prev_c at t == T, else null
};

template <int NT, bool FUSEX>
__global__ __launch_bounds__(NW * 64) void k_gates_step(GatesArgs a) {
  GENERIC_GEOMETRY();
  STEP_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, I = a.I, t = a.t;
  const int c0 = blockIdx.x * 4;
  const int sbase = blockIdx.y * TS_ * NT;

  // ---- epilogue operands first: wave nt owns s-tile nt; lane = (cell c0+q, stream bs) ----
  const int e_cell = c0 + q;
  const int e_s = sbase + wave * TS_ + bs;
  const bool e_on = wave < NT && Geo<SMALL>::owner(lane) && e_cell < C && e_s < S;
  const int l_cell = e_on ? e_cell : 0, l_s = e_on ? e_s : 0;          // clamped: loads are unconditional
  const size_t e_row = (size_t)t * S + l_s;
  float pre[4];
#pragma unroll
  for (int g = 0; g < 4; g++) pre[g] = FUSEX ? a.bias[g * C + l_cell] : a.gifo[e_row * 4 * C + g * C + l_cell];
  const float cp = a.cprev[(size_t)l_s * C + l_cell];
  const float wpi = a.pi[l_cell], wpf = a.pf[l_cell], wpo = a.po[l_cell];

  // ---- contraction over [r(t-1) | x(t)] ----
  const int cell_a = c0 + (i16 >> 2), gate_a = i16 & 3;
  const bool row_ok = cell_a < C;
  const size_t wrow_idx = (size_t)gate_a * C + (row_ok ? cell_a : 0);
  const float *wr_row = a.wr + wrow_idx * R;
  const float *wx_row = FUSEX ? a.wx + wrow_idx * I : nullptr;
  const int nchR = (R + KCH - 1) / KCH;
  const int nch = nchR + (FUSEX ? (I + KCH - 1) / KCH : 0);
  const bool mirror_r = a.r_mirror != nullptr && blockIdx.x == 0 && (SMALL ? q == 0 : true);

  f32x4 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) { acc[nt][0] = (f32x4){0, 0, 0, 0}; acc[nt][1] = (f32x4){0, 0, 0, 0}; }

  auto afetch = [&](int ch, bool on, float (&v)[8]) {
    if (!FUSEX || ch < nchR) load8<VEC>(wr_row, ch * KCH + kg * 8, R, on && row_ok, v);
    else load8<VEC>(wx_row, (ch - nchR) * KCH + kg * 8, I, on && row_ok, v);
  };
  auto bfetch = [&](int ch, int nt, bool on, float (&v)[8]) {
    const int s = sbase + nt * TS_ + bs;
    const bool ok = on && s < S;
    if (!FUSEX || ch < nchR) load8<VEC>(a.rprev + (size_t)(ok ? s : 0) * R, ch * KCH + kg * 8, R, ok, v);
    else load8<VEC>(a.x + (size_t)(ok ? s : 0) * a.x_stride, (ch - nchR) * KCH + kg * 8, I, ok, v);
  };
  auto bpost = [&](int ch, int nt, bool on, const float (&v)[8]) {      // :231 (r columns of block 0)
    const int s = sbase + nt * TS_ + bs;
    if (mirror_r && on && s < S && ch < nchR) store8<VEC>(a.r_mirror + (size_t)s * R, ch * KCH + kg * 8, R, v);
  };
  mma_k_loop<NT, CPW, SMALL>(nch, wave, acc, afetch, bfetch, bpost);

  __shared__ f32x4 red[NW][NT][64];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) red[wave][nt][lane] = acc[nt][0] + acc[nt][1];
  __syncthreads();

  if (e_on) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    float ag = v.x + pre[0];
    float ai = v.y + pre[1];
    float af = v.z + pre[2];
    float ao = v.w + pre[3];
    ai += wpi * cp;                                // :278
    af += wpf * cp;                                // :281
    const float gi = k_sigmoid(ai), gf = k_sigmoid(af), gg = k_tanh(ag);   // :284-288
    float c = gg * gi;                             // :291
    c = c + cp * gf;                               // :294
    c = c < -50.f ? -50.f : c;                     // :296
    c = c > 50.f ? 50.f : c;                       // :297
    const float h = k_tanh(c);                     // :300
    ao += wpo * c;                                 // :303
    const float go = k_sigmoid(ao);                // :306
    const float m = h * go;                        // :309
    float *gp = a.gifo + e_row * 4 * C + e_cell;
    gp[0] = gg; gp[C] = gi; gp[2 * C] = gf; gp[3 * C] = go;
    a.cc[e_row * C + e_cell] = c;
    a.hh[e_row * C + e_cell] = h;
    a.mm[e_row * C + e_cell] = m;
    if (a.c_mirror) a.c_mirror[(size_t)e_s * C + e_cell] = cp;   // :231 (c columns)
    if (a.c_save) a.c_save[(size_t)e_s * C + e_cell] = c;         // :331 (c columns)
  }
}

// ---------------------------------------------------------------------------------------------
// forward step 2/2: recurrent projection r(t) = m(t) * W_r_m^T (:312), also written to `out` (:328)
// and, at t == T, to the carried state (:331).  One workgroup = 16 projection rows x NT stream tiles;
// lane owns 4 consecutive r columns.
// ---------------------------------------------------------------------------------------------
struct ProjArgs {
  int C, R, S, t;
  const float *wm, *mm;
  float *rr, *out, *r_save;
  int out_stride;
  int vecOut;
};

template <int NT>
__global__ __launch_bounds__(NW * 64) void k_proj_step(ProjArgs a) {
  GENERIC_GEOMETRY();
  STEP_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int n0 = blockIdx.x * 16;
  const int sbase = blockIdx.y * TS_ * NT;
  const bool row_ok = n0 + i16 < R;
  const float *wrow = a.wm + (size_t)(row_ok ? n0 + i16 : 0) * C;
  const float *mrow = a.mm + (size_t)t * S * C;

  f32x4 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) { acc[nt][0] = (f32x4){0, 0, 0, 0}; acc[nt][1] = (f32x4){0, 0, 0, 0}; }
  auto afetch = [&](int ch, bool on, float (&v)[8]) { load8<VEC>(wrow, ch * KCH + kg * 8, C, on && row_ok, v); };
  auto bfetch = [&](int ch, int nt, bool on, float (&v)[8]) {
    const int s = sbase + nt * TS_ + bs;
    const bool ok = on && s < S;
    load8<VEC>(mrow + (size_t)(ok ? s : 0) * C, ch * KCH + kg * 8, C, ok, v);
  };
  mma_k_loop<NT, CPW, SMALL>((C + KCH - 1) / KCH, wave, acc, afetch, bfetch, NoPost());

  __shared__ f32x4 red[NW][NT][64];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) red[wave][nt][lane] = acc[nt][0] + acc[nt][1];
  __syncthreads();

  if (wave < NT && Geo<SMALL>::owner(lane)) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const int s = sbase + wave * TS_ + bs;
    const int n = n0 + 4 * q;
    if (s < S && n < R) {
      const float e[4] = {v.x, v.y, v.z, v.w};
      store4<VEC>(a.rr + ((size_t)t * S + s) * R, n, R, e);
      float *op = a.out + (size_t)((t - 1) * S + s) * a.out_stride;
      if (a.vecOut) store4<true>(op, n, R, e); else store4<false>(op, n, R, e);
      if (a.r_save) store4<VEC>(a.r_save + (size_t)s * R, n, R, e);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward step 1/2: partial products of DGIFO(t+1) [S x 4C] with W_gifo_r (-> d_r(t), :391) and,
// optionally, W_gifo_x (-> in_diff of frame t+1, :457) over one K slice of the 4C gate rows.
// grid (R tiles + I tiles, stream groups, KS); slab ks holds the partial sum of its slice, the
// consumer (k_dm_step) adds the slabs in fixed order.
// ---------------------------------------------------------------------------------------------
struct DrArgs {
  int C, R, I, S, t;
  const float *wrT, *wxT;   // [R x 4C], [I x 4C]
  const float *dgifo;
  float *part;              // [KS][S][R]
  float *xpart;             // [KS][S][x_ld]  (or in_diff rows of frame 1 when t == 0, KS == 1)
  int x_ld;
  int ntr;                  // number of 16-row tiles over R in grid.x (0 at t == 0)
  int klen;                 // K slice length (multiple of KCH)
  int vecX;
};

template <int NT>
__global__ __launch_bounds__(NW * 64) void k_dr_step(DrArgs a) {
  GENERIC_GEOMETRY();
  STEP_PROLOGUE();
  const int R = a.R, I = a.I, S = a.S, K = 4 * a.C;
  const bool is_x = (int)blockIdx.x >= a.ntr;
  const int n0 = (is_x ? (int)blockIdx.x - a.ntr : (int)blockIdx.x) * 16;
  const int N = is_x ? I : R;
  const int sbase = blockIdx.y * TS_ * NT;
  const int ks = blockIdx.z;
  const int kbeg = ks * a.klen;
  const int kend = min(K, kbeg + a.klen);
  const bool row_ok = n0 + i16 < N;
  const float *wrow = (is_x ? a.wxT : a.wrT) + (size_t)(row_ok ? n0 + i16 : 0) * K;
  const float *drow = a.dgifo + (size_t)(a.t + 1) * S * K;

  f32x4 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) { acc[nt][0] = (f32x4){0, 0, 0, 0}; acc[nt][1] = (f32x4){0, 0, 0, 0}; }
  auto afetch = [&](int ch, bool on, float (&v)[8]) { load8<VEC>(wrow, kbeg + ch * KCH + kg * 8, kend, on && row_ok, v); };
  auto bfetch = [&](int ch, int nt, bool on, float (&v)[8]) {
    const int s = sbase + nt * TS_ + bs;
    const bool ok = on && s < S;
    load8<VEC>(drow + (size_t)(ok ? s : 0) * K, kbeg + ch * KCH + kg * 8, kend, ok, v);
  };
  mma_k_loop<NT, CPW, SMALL>(kend > kbeg ? (kend - kbeg + KCH - 1) / KCH : 0, wave, acc, afetch, bfetch, NoPost());

  __shared__ f32x4 red[NW][NT][64];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) red[wave][nt][lane] = acc[nt][0] + acc[nt][1];
  __syncthreads();

  if (wave < NT && Geo<SMALL>::owner(lane)) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const int s = sbase + wave * TS_ + bs;
    const int n = n0 + 4 * q;
    if (s < S && n < N) {
      const float e[4] = {v.x, v.y, v.z, v.w};
      if (is_x) {
        float *xp = a.xpart + ((size_t)ks * S + s) * a.x_ld;
        if (a.vecX) store4<true>(xp, n, I, e); else store4<false>(xp, n, I, e);
      } else {
        store4<VEC>(a.part + ((size_t)ks * S + s) * R, n, R, e);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward step 2/2: d_r(t) = out_diff(t) + sum of slabs; d_m = d_r * W_r_m (:408) and the whole
// elementwise BPTT cell math (:411-440).  One workgroup = 16 cells x NT stream tiles; lane owns 4
// consecutive cells of one stream.  Workgroup x==0 also materialises d_r(t) (needed by the
// W_r_m gradient, :486); the last workgroup also reduces the in_diff slabs of frame t+1.
// ---------------------------------------------------------------------------------------------
struct DmArgs {
  int C, R, I, S, T, t;
  const float *wmT;       // [C x R]
  const float *pi, *pf, *po;
  const float *gifo, *cc, *hh;
  float *dgifo, *dc, *dr;
  const float *part;      // [KS][S][R]
  int nslab;              // 0 at t == T (the t+1 block is all zero, :351)
  const float *out_diff;
  int od_stride;
  const float *xpart;     // [KS][S][I] in_diff slabs of frame t+1 (null: nothing to reduce)
  float *in_diff;         // rows of frame t+1
  int id_stride;
};

// Side job of the d_m kernels: in_diff(t+1) = sum of its split-K slabs (:457), the (streams x I) elements of a
// stream tile spread evenly over the gx row-tile workgroups of that tile (one workgroup alone takes 16 dependent
// rounds at I = 512, the stacked-layer shape).
__device__ __forceinline__ void reduce_x_slabs(const DmArgs &a, int s_lo, int s_hi, int bx, int gx) {
  if (!a.xpart) return;
  const int I = a.I, S = a.S;
  const int per = ((s_hi - s_lo) * I + gx - 1) / gx;
  const int lo = s_lo * I + bx * per, hi = min(s_hi * I, lo + per);
  for (int idx = lo + (int)threadIdx.x; idx < hi; idx += NW * 64) {
    const int s = idx / I, n = idx - s * I;
    float p[KSMAX];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++) p[ks] = a.xpart[((size_t)(ks < a.nslab ? ks : 0) * S + s) * I + n];
    float sum = p[0];
#pragma unroll
    for (int ks = 1; ks < KSMAX; ks++) sum += ks < a.nslab ? p[ks] : 0.f;
    a.in_diff[(size_t)s * a.id_stride + n] = sum;
  }
}

template <int NT>
__global__ __launch_bounds__(NW * 64) void k_dm_step(DmArgs a) {
  GENERIC_GEOMETRY();
  STEP_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int c0 = blockIdx.x * 16;
  const int sbase = blockIdx.y * TS_ * NT;
  const bool last = (t == a.T);

  reduce_x_slabs(a, sbase, min(S, sbase + TS_ * NT), blockIdx.x, gridDim.x);

  // ---- epilogue operands first: wave nt owns s-tile nt; lane = (stream, cells cb..cb+3) ----
  const int e_s = sbase + wave * TS_ + bs;
  const int cb = c0 + 4 * q;
  const bool e_on = wave < NT && Geo<SMALL>::owner(lane) && e_s < S && cb < C;
  const size_t row = (size_t)t * S + (e_on ? e_s : 0), rown = row + S, rowp = row - S;
  float yg[4], yi[4], yf[4], yo[4], yh[4], cpv[4], dcn[4], fn[4], din[4], dfn[4], wpi[4], wpf[4], wpo[4];
  {
    const float *yp = a.gifo + row * 4 * C;
    load4<VEC>(yp, cb, C, e_on, yg);
    load4<VEC>(yp + C, cb, C, e_on, yi);
    load4<VEC>(yp + 2 * C, cb, C, e_on, yf);
    load4<VEC>(yp + 3 * C, cb, C, e_on, yo);
    load4<VEC>(a.hh + row * C, cb, C, e_on, yh);
    load4<VEC>(a.cc + rowp * C, cb, C, e_on, cpv);
    const bool n_on = e_on && !last;
    const size_t rn = last ? row : rown;                 // clamped: block T+1 is never dereferenced
    load4<VEC>(a.dc + rn * C, cb, C, n_on, dcn);
    load4<VEC>(a.gifo + rn * 4 * C + 2 * C, cb, C, n_on, fn);
    load4<VEC>(a.dgifo + rn * 4 * C + C, cb, C, n_on, din);
    load4<VEC>(a.dgifo + rn * 4 * C + 2 * C, cb, C, n_on, dfn);
    load4<VEC>(a.pi, cb, C, e_on, wpi);
    load4<VEC>(a.pf, cb, C, e_on, wpf);
    load4<VEC>(a.po, cb, C, e_on, wpo);
  }

  const bool row_ok = c0 + i16 < C;
  const float *wrow = a.wmT + (size_t)(row_ok ? c0 + i16 : 0) * R;
  const bool write_dr = blockIdx.x == 0 && (SMALL ? q == 0 : true);

  f32x4 acc[NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) { acc[nt][0] = (f32x4){0, 0, 0, 0}; acc[nt][1] = (f32x4){0, 0, 0, 0}; }
  auto afetch = [&](int ch, bool on, float (&v)[8]) { load8<VEC>(wrow, ch * KCH + kg * 8, R, on && row_ok, v); };
  auto bfetch = [&](int ch, int nt, bool on, float (&v)[8]) {
    const int s = sbase + nt * TS_ + bs;
    const bool ok = on && s < S;
    const int k = ch * KCH + kg * 8;
    const float *odp = a.out_diff + (size_t)((t - 1) * S + (ok ? s : 0)) * a.od_stride;          // :367
    load8<VEC>(odp, k, R, ok, v);
    float p[KSMAX][8];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++)
      load8<VEC>(a.part + ((size_t)(ks < a.nslab ? ks : 0) * S + (ok ? s : 0)) * R, k, R, ok && ks < a.nslab, p[ks]);
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++)
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] += p[ks][j];                                               // :391
  };
  auto bpost = [&](int ch, int nt, bool on, const float (&v)[8]) {
    const int s = sbase + nt * TS_ + bs;
    if (write_dr && on && s < S) store8<VEC>(a.dr + ((size_t)t * S + s) * R, ch * KCH + kg * 8, R, v);
  };
  mma_k_loop<NT, CPW, SMALL>((R + KCH - 1) / KCH, wave, acc, afetch, bfetch, bpost);

  __shared__ f32x4 red[NW][NT][64];
#pragma unroll
  for (int nt = 0; nt < NT; nt++) red[wave][nt][lane] = acc[nt][0] + acc[nt][1];
  __syncthreads();

  if (e_on) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const float dm[4] = {v.x, v.y, v.z, v.w};
    float og[4], oi[4], of[4], oo[4], oc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d_h = k_diff_tanh(dm[j] * yo[j], yh[j]);       // :411-412
      const float d_o = k_diff_sigmoid(dm[j] * yh[j], yo[j]);    // :415-416
      float d_c = d_h;                                           // :424
      d_c = d_c + dcn[j] * fn[j];                                // :425
      d_c = d_c + wpi[j] * din[j];                               // :426
      d_c = d_c + wpf[j] * dfn[j];                               // :427
      d_c = d_c + wpo[j] * d_o;                                  // :428
      of[j] = k_diff_sigmoid(d_c * cpv[j], yf[j]);               // :431-432
      oi[j] = k_diff_sigmoid(d_c * yg[j], yi[j]);                // :435-436
      og[j] = k_diff_tanh(d_c * yi[j], yg[j]);                   // :439-440
      oo[j] = d_o;
      oc[j] = d_c;
    }
    float *dp = a.dgifo + row * 4 * C;
    store4<VEC>(dp, cb, C, og);
    store4<VEC>(dp + C, cb, C, oi);
    store4<VEC>(dp + 2 * C, cb, C, of);
    store4<VEC>(dp + 3 * C, cb, C, oo);
    store4<VEC>(a.dc + row * C, cb, C, oc);
  }
}

// =============================================================================================
// VECTOR PATH (aligned shapes: R, I, C multiples of 8).  Two rules measured on MI355X shape it
// (tools/act_anatomy.hip, tools/step_anatomy.hip): a wave-load whose lanes hit 16+ scattered rows
// costs ~64 L1 lookups (+0.7 us per kernel for an 8 KB operand), while the same bytes fetched
// lane-contiguous cost +0.1 us.  Therefore
//   * weights are read from PACKED copies laid out in MFMA A-operand order
//       pk[tile][chunk][h][lane][4]:  row = rowmap(tile, lane&15), k = chunk*32 + (lane>>4)*8 + h*4 + e
//     (zero padded), written once per Update by k_pack -> every weight load is a contiguous 1 KB;
//   * activations are fetched lane-contiguous from their natural [stream][k] layout, staged in LDS
//     (padded rows, conflict-free ds_read_b128) and read from there in B-operand order.
// =============================================================================================
template <int CPW, bool SMALL> struct VGeo {
  static constexpr int SUPER = CPW * NW;                       // chunks per super-iteration
  static constexpr int LDB = SUPER * KCH + (SMALL ? 16 : 4);   // LDS row stride (floats): b128 reads conflict-free
  static constexpr int LDBH = SUPER * KCH + (SMALL ? 32 : 8);  // same padding in bytes for the bf16 slab (halves)
};

// One contraction: acc[nt] += A(tile rows, chunks [0,nch)) * B(streams, same chunks).
//   apk   : packed weights of this tile, chunk c at apk + c*128 (float4 units)
//   bload(s, k, on) -> float4 of B[s][k..k+3] in natural layout (zeros outside / when !on), k relative to chunk 0;
//                      must be branch-free (clamped addresses + selects) so that all loads of a slab overlap
//   bside(s, k, v): optional side store of the staged natural-layout value (mirrors)
//   BF    : bf16 operands -- chunk c of the packed weights at apk + c*64 (one 16-byte vector of 8 bf16 per lane),
//           B staged as bf16; one 16x16x32 (or two 4x4x4_16b) MFMAs per chunk instead of eight f32 ones
struct NoEpi { __device__ __forceinline__ void operator()() const {} };
//   epi() : issues the caller's epilogue-operand loads; called once, right AFTER the slab and weight loads of the first
//           super-iteration (loads return in order: what is needed last is requested last)
template <int NT, int CPW, bool SMALL, bool BF, class BL, class BS, class EP = NoEpi>
__device__ __forceinline__ void vec_contract(const float4 *__restrict__ apk, int nch, int rows, float *ldsB,
                                             int lane, int wave, f32x4 (&acc)[NT][2], const BL &bload, const BS &bside,
                                             const EP &epi = EP()) {
  (void)rows;
  constexpr int SUPER = VGeo<CPW, SMALL>::SUPER, LDB = VGeo<CPW, SMALL>::LDB, LDBH = VGeo<CPW, SMALL>::LDBH;
  constexpr int TS_ = Geo<SMALL>::STREAMS;
  constexpr int AU = BF ? 64 : 128;                            // float4 units per packed chunk
  unsigned short *ldsH = reinterpret_cast<unsigned short *>(ldsB);
  const int bs = Geo<SMALL>::bstream(lane), kg = lane >> 4;
  // The first super-iteration is PEELED out of the loop (it is the only one whenever K <= SUPER*32, i.e. in every
  // latency-critical shape): at a loop header the compiler drains all outstanding loads (s_waitcnt vmcnt(0)), which made
  // the epilogue operands the callers request up front a full memory round trip in FRONT of the weight fetch.
  auto iter = [&](int base) {
    const int nc = min(SUPER, nch - base);
    // (1) this wave's weight chunks: an even contiguous share [c0, c0 + per) of the super-iteration
    const int per = (nc + NW - 1) / NW;
    const int c0 = wave * per;
    // (2a) the B slab is requested FIRST: loads return in order, and the slab (LDS store, barrier) is needed before the
    //      weights (first MFMA) -- behind 8 weight loads its wait would drain them too
    constexpr int ROWS = NT * TS_, F4ROW = SUPER * 8;
    constexpr int U = (ROWS * F4ROW + NW * 64 - 1) / (NW * 64);
    float4 sv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int idx = threadIdx.x + u * NW * 64;
      const int sl = idx / F4ROW, k = (idx % F4ROW) * 4;
      sv[u] = bload(sl < ROWS ? sl : 0, base * KCH + k, sl < ROWS && k < nc * KCH);
    }
    float4 a0[CPW], a1[CPW];
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      const int cl = min(c0 + c, nc - 1);                      // clamped: always a valid chunk, unused if off
      const float4 *ap = apk + (size_t)(base + cl) * AU + lane;
      a0[c] = ap[0]; a1[c] = BF ? a0[c] : ap[64];
    }
    if (base == 0) epi();
    // (2b) stage B[rows][nc*32] lane-contiguous into LDS: every load of the slab is issued before the first store
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int idx = threadIdx.x + u * NW * 64;
      const int sl = idx / F4ROW, k = (idx % F4ROW) * 4;
      if (sl < ROWS && k < nc * KCH) {
        if constexpr (BF) *reinterpret_cast<uint2 *>(ldsH + sl * LDBH + k) = pack_bf16x4(sv[u]);
        else *reinterpret_cast<float4 *>(ldsB + sl * LDB + k) = sv[u];
        bside(sl, base * KCH + k, sv[u]);
      }
    }
    __syncthreads();
    // (3) MFMAs
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      if (c < per && c0 + c < nc) {
        if constexpr (BF) {
#pragma unroll
          for (int nt = 0; nt < NT; nt++) {
            const float4 braw = *reinterpret_cast<const float4 *>(ldsH + (nt * TS_ + bs) * LDBH + (c0 + c) * KCH + kg * 8);
            if constexpr (SMALL) {
              const float2 alo = make_float2(a0[c].x, a0[c].y), ahi = make_float2(a0[c].z, a0[c].w);
              const float2 blo = make_float2(braw.x, braw.y), bhi = make_float2(braw.z, braw.w);
              acc[nt][0] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(s16x4, alo), __builtin_bit_cast(s16x4, blo), acc[nt][0], 0, 0, 0);
              acc[nt][1] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(s16x4, ahi), __builtin_bit_cast(s16x4, bhi), acc[nt][1], 0, 0, 0);
            } else {
              acc[nt][c & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0[c]), __builtin_bit_cast(bf16x8, braw), acc[nt][c & 1], 0, 0, 0);
            }
          }
          continue;
        }
        const float av[8] = {a0[c].x, a0[c].y, a0[c].z, a0[c].w, a1[c].x, a1[c].y, a1[c].z, a1[c].w};
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
          const float *bp = ldsB + (nt * TS_ + bs) * LDB + (c0 + c) * KCH + kg * 8;
          const float4 b0 = *reinterpret_cast<const float4 *>(bp), b1 = *reinterpret_cast<const float4 *>(bp + 4);
          const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int j = 0; j < 8; j++) acc[nt][j & 1] = Geo<SMALL>::mma(av[j], bv[j], acc[nt][j & 1]);
        }
      }
    }
    if (base + SUPER < nch) __syncthreads();
  };
  if (nch > 0) iter(0); else epi();
  for (int base = SUPER; base < nch; base += SUPER) iter(base);
}
struct NoSide { __device__ __forceinline__ void operator()(int, int, const float4 &) const {} };

#define VEC_PROLOGUE()                                                                           \
  const int lane = threadIdx.x & 63;                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                             \
  const int bs = Geo<SMALL>::bstream(lane), q = Geo<SMALL>::q(lane);                             \
  constexpr int TS_ = Geo<SMALL>::STREAMS;                                                       \
  __shared__ __attribute__((aligned(16))) float ldsB[NT * TS_ * VGeo<CPW, SMALL>::LDB];          \
  __shared__ f32x4 red[NW][NT][64];                                                              \
  f32x4 acc[NT][2];                                                                              \
  _Pragma("unroll") for (int nt = 0; nt < NT; nt++) { acc[nt][0] = (f32x4){0, 0, 0, 0}; acc[nt][1] = (f32x4){0, 0, 0, 0}; } \
  (void)bs; (void)q

// 4x4x1_16b geometry: the four k-groups of a (row, stream) pair sit 16 lanes apart -> xor butterfly first (a+b == b+a
// bitwise, so every lane ends with the same sum), then 8 per-wave partials instead of 32 go through LDS
#define VEC_COMBINE()                                                                            \
  _Pragma("unroll") for (int nt = 0; nt < NT; nt++) {                                            \
    f32x4 _v = acc[nt][0] + acc[nt][1];                                                          \
    if (SMALL) {                                                                                 \
      _Pragma("unroll") for (int _m = 16; _m < 64; _m <<= 1) {                                   \
        _v.x += __shfl_xor(_v.x, _m); _v.y += __shfl_xor(_v.y, _m); _v.z += __shfl_xor(_v.z, _m); _v.w += __shfl_xor(_v.w, _m); \
      }                                                                                          \
    }                                                                                            \
    red[wave][nt][lane] = _v;                                                                    \
  }                                                                                              \
  __syncthreads()

struct GatesVArgs {
  int gx;                // real number of row-tile groups (many-stream kernels pad grid.x to a multiple of 8)
  GatesArgs g;
  const float4 *wpk;     // packed [W_gifo_r | W_gifo_x] : [C/4 tiles][nchR + nchX chunks][2][64]
  int nch_total;         // chunks per tile in wpk (nchR + nchX)
};

template <int NT, int CPW, bool SMALL, bool FUSEX, bool BF>
__global__ __launch_bounds__(NW * 64) void k_gates_v(GatesVArgs va) {
  const GatesArgs &a = va.g;
  VEC_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, I = a.I, t = a.t;
  const int c0 = blockIdx.x * 4;
  const int sbase = blockIdx.y * TS_ * NT;

  // ---- epilogue operands first: wave nt owns s-tile nt; lane = (cell c0+q, stream bs) ----
  const int e_cell = c0 + q;
  const int e_s = sbase + wave * TS_ + bs;
  const bool e_on = wave < NT && Geo<SMALL>::owner(lane) && e_cell < C && e_s < S;
  const int l_cell = e_on ? e_cell : 0, l_s = e_on ? e_s : 0;
  const size_t e_row = (size_t)t * S + l_s;
  // (8 scalar loads: measured 0.1 us faster requested here, under the scalar prologue, than after the weight loads)
  float pre[4];
#pragma unroll
  for (int g = 0; g < 4; g++) pre[g] = FUSEX ? a.bias[g * C + l_cell] : a.gifo[e_row * 4 * C + g * C + l_cell];
  const float cp = a.cprev[(size_t)l_s * C + l_cell];
  const float wpi = a.pi[l_cell], wpf = a.pf[l_cell], wpo = a.po[l_cell];

  const int nchR = R / KCH + (R % KCH != 0);
  const int Rp = nchR * KCH;
  const int nch = nchR + (FUSEX ? (I + KCH - 1) / KCH : 0);
  const bool mirror_r = a.r_mirror != nullptr && blockIdx.x == 0;
  auto bload = [&](int sl, int k, bool on) -> float4 {    // B = [ r(t-1) | pad | x(t) | pad ], branch-free
    const int s = min(sbase + sl, S - 1);
    const bool inr = k < R, inx = FUSEX && k >= Rp && k - Rp < I;
    const float *p = inr ? a.rprev + (size_t)s * R + k : inx ? a.x + (size_t)s * a.x_stride + (k - Rp) : a.rprev;
    const float4 v = ldg4(p);
    return keep_if(v, on && sbase + sl < S && (inr || inx));
  };
  auto bside = [&](int sl, int k, const float4 &v) {      // :231 (r columns of time block 0)
    const int s = sbase + sl;
    if (mirror_r && s < S && k < R) *reinterpret_cast<float4 *>(a.r_mirror + (size_t)s * R + k) = v;
  };
  vec_contract<NT, CPW, SMALL, BF>(va.wpk + (size_t)blockIdx.x * va.nch_total * (BF ? 64 : 128), nch, NT * TS_, ldsB, lane, wave, acc,
                               bload, bside);
  VEC_COMBINE();

  if (e_on) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    float ag = v.x + pre[0];
    float ai = v.y + pre[1];
    float af = v.z + pre[2];
    float ao = v.w + pre[3];
    ai += wpi * cp;                                // :278
    af += wpf * cp;                                // :281
    const float gi = k_sigmoid(ai), gf = k_sigmoid(af), gg = k_tanh(ag);   // :284-288
    float c = gg * gi;                             // :291
    c = c + cp * gf;                               // :294
    c = c < -50.f ? -50.f : c;                     // :296
    c = c > 50.f ? 50.f : c;                       // :297
    const float h = k_tanh(c);                     // :300
    ao += wpo * c;                                 // :303
    const float go = k_sigmoid(ao);                // :306
    const float m = h * go;                        // :309
    float *gp = a.gifo + e_row * 4 * C + e_cell;
    gp[0] = gg; gp[C] = gi; gp[2 * C] = gf; gp[3 * C] = go;
    a.cc[e_row * C + e_cell] = c;
    a.hh[e_row * C + e_cell] = h;
    a.mm[e_row * C + e_cell] = m;
    if (a.c_mirror) a.c_mirror[(size_t)e_s * C + e_cell] = cp;   // :231 (c columns)
    if (a.c_save) a.c_save[(size_t)e_s * C + e_cell] = c;         // :331 (c columns)
  }
}

struct ProjVArgs { int gx; ProjArgs g; const float4 *wpk; };   // packed W_r_m: [R/16 tiles][C/32 chunks][2][64]

template <int NT, int CPW, bool SMALL, bool BF>
__global__ __launch_bounds__(NW * 64) void k_proj_v(ProjVArgs va) {
  const ProjArgs &a = va.g;
  VEC_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int n0 = blockIdx.x * 16;
  const int sbase = blockIdx.y * TS_ * NT;
  const int nch = (C + KCH - 1) / KCH;
  const float *mrow = a.mm + (size_t)t * S * C;
  auto bload = [&](int sl, int k, bool on) -> float4 {
    const float4 v = ldg4(mrow + (size_t)min(sbase + sl, S - 1) * C + min(k, C - 4));
    return keep_if(v, on && sbase + sl < S && k < C);
  };
  vec_contract<NT, CPW, SMALL, BF>(va.wpk + (size_t)blockIdx.x * nch * (BF ? 64 : 128), nch, NT * TS_, ldsB, lane, wave, acc, bload, NoSide());
  VEC_COMBINE();
  if (wave < NT && Geo<SMALL>::owner(lane)) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const int s = sbase + wave * TS_ + bs;
    const int n = n0 + 4 * q;
    if (s < S && n < R) {
      const float e[4] = {v.x, v.y, v.z, v.w};
      store4<true>(a.rr + ((size_t)t * S + s) * R, n, R, e);
      float *op = a.out + (size_t)((t - 1) * S + s) * a.out_stride;
      if (a.vecOut) store4<true>(op, n, R, e); else store4<false>(op, n, R, e);
      if (a.r_save) store4<true>(a.r_save + (size_t)s * R, n, R, e);
    }
  }
}

struct DrVArgs { int gx; DrArgs g; const float4 *wpk; int nch_total; };   // packed [W_gifo_r^T ; W_gifo_x^T]: [(R+I)/16 tiles][4C/32][2][64]

template <int NT, int CPW, bool SMALL, bool BF>
__global__ __launch_bounds__(NW * 64) void k_dr_v(DrVArgs va) {
  const DrArgs &a = va.g;
  VEC_PROLOGUE();
  const int R = a.R, I = a.I, S = a.S, K = 4 * a.C;
  const bool is_x = (int)blockIdx.x >= a.ntr;
  const int ntR = (R + 15) / 16;                               // x tiles follow the R tiles in the packed array
  const int tile = is_x ? ntR + ((int)blockIdx.x - a.ntr) : (int)blockIdx.x;
  const int n0 = (is_x ? (int)blockIdx.x - a.ntr : (int)blockIdx.x) * 16;
  const int N = is_x ? I : R;
  const int sbase = blockIdx.y * TS_ * NT;
  const int ks = blockIdx.z;
  const int kbeg = ks * a.klen;
  const int kend = min(K, kbeg + a.klen);
  const float *drow = a.dgifo + (size_t)(a.t + 1) * S * K;
  auto bload = [&](int sl, int k, bool on) -> float4 {
    const float4 v = ldg4(drow + (size_t)min(sbase + sl, S - 1) * K + min(kbeg + k, K - 4));
    return keep_if(v, on && sbase + sl < S && kbeg + k < kend);
  };
  vec_contract<NT, CPW, SMALL, BF>(va.wpk + ((size_t)tile * va.nch_total + kbeg / KCH) * (BF ? 64 : 128),
                               kend > kbeg ? (kend - kbeg + KCH - 1) / KCH : 0, NT * TS_, ldsB, lane, wave, acc, bload, NoSide());
  VEC_COMBINE();
  if (wave < NT && Geo<SMALL>::owner(lane)) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const int s = sbase + wave * TS_ + bs;
    const int n = n0 + 4 * q;
    if (s < S && n < N) {
      const float e[4] = {v.x, v.y, v.z, v.w};
      if (is_x) {
        float *xp = a.xpart + ((size_t)ks * S + s) * a.x_ld;
        if (a.vecX) store4<true>(xp, n, I, e); else store4<false>(xp, n, I, e);
      } else {
        store4<true>(a.part + ((size_t)ks * S + s) * R, n, R, e);
      }
    }
  }
}

struct DmVArgs { int gx; DmArgs g; const float4 *wpk; };   // packed W_r_m^T: [C/16 tiles][R/32 chunks][2][64]

template <int NT, int CPW, bool SMALL, bool BF>
__global__ __launch_bounds__(NW * 64) void k_dm_v(DmVArgs va) {
  const DmArgs &a = va.g;
  VEC_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int c0 = blockIdx.x * 16;
  const int sbase = blockIdx.y * TS_ * NT;
  const bool last = (t == a.T);

  reduce_x_slabs(a, sbase, min(S, sbase + TS_ * NT), blockIdx.x, gridDim.x);

  // ---- epilogue operands (requested from inside the contraction, after its own loads): wave nt owns s-tile nt;
  //      lane = (stream, cells cb..cb+3) ----
  const int e_s = sbase + wave * TS_ + bs;
  const int cb = c0 + 4 * q;
  const bool e_on = wave < NT && Geo<SMALL>::owner(lane) && e_s < S && cb < C;
  const size_t row = (size_t)t * S + (e_on ? e_s : 0), rown = row + S, rowp = row - S;
  float yg[4], yi[4], yf[4], yo[4], yh[4], cpv[4], dcn[4], fn[4], din[4], dfn[4], wpi[4], wpf[4], wpo[4];
  // 4x4x1 geometry: ONE cell per lane on all 64 lanes of wave nt (cell c0 + lane/4, stream lane%4) -- four cells on each
  // of 16 lanes is four dependent chains of cell math in a row (see k_dmf_v)
  const int s_cell = c0 + (lane >> 2), s_s = sbase + wave * TS_ + (lane & 3);
  const bool s_on = SMALL && wave < NT && s_s < S && s_cell < C;
  const size_t srow = (size_t)t * S + (s_on ? s_s : 0);
  const int slc = s_on ? s_cell : 0;
  float sy[13];
  auto epi = [&]() {
    if constexpr (SMALL) {
      const bool n_on = s_on && !last;
      const size_t rn = last ? srow : srow + S;            // clamped: block T+1 is never dereferenced
      const float *yp = a.gifo + srow * 4 * C + slc;
      sy[0] = yp[0]; sy[1] = yp[C]; sy[2] = yp[2 * C]; sy[3] = yp[3 * C];
      sy[4] = a.hh[srow * C + slc]; sy[5] = a.cc[(srow - S) * C + slc];
      const float d0 = a.dc[rn * C + slc], d1 = a.gifo[rn * 4 * C + 2 * C + slc];
      const float d2 = a.dgifo[rn * 4 * C + C + slc], d3 = a.dgifo[rn * 4 * C + 2 * C + slc];
      sy[6] = n_on ? d0 : 0.f; sy[7] = n_on ? d1 : 0.f; sy[8] = n_on ? d2 : 0.f; sy[9] = n_on ? d3 : 0.f;
      sy[10] = a.pi[slc]; sy[11] = a.pf[slc]; sy[12] = a.po[slc];
      return;
    }
    const float *yp = a.gifo + row * 4 * C;
    load4<true>(yp, cb, C, e_on, yg);
    load4<true>(yp + C, cb, C, e_on, yi);
    load4<true>(yp + 2 * C, cb, C, e_on, yf);
    load4<true>(yp + 3 * C, cb, C, e_on, yo);
    load4<true>(a.hh + row * C, cb, C, e_on, yh);
    load4<true>(a.cc + rowp * C, cb, C, e_on, cpv);
    const bool n_on = e_on && !last;
    const size_t rn = last ? row : rown;                 // clamped: block T+1 is never dereferenced
    load4<true>(a.dc + rn * C, cb, C, n_on, dcn);
    load4<true>(a.gifo + rn * 4 * C + 2 * C, cb, C, n_on, fn);
    load4<true>(a.dgifo + rn * 4 * C + C, cb, C, n_on, din);
    load4<true>(a.dgifo + rn * 4 * C + 2 * C, cb, C, n_on, dfn);
    load4<true>(a.pi, cb, C, e_on, wpi);
    load4<true>(a.pf, cb, C, e_on, wpf);
    load4<true>(a.po, cb, C, e_on, wpo);
  };

  const int nch = (R + KCH - 1) / KCH;
  const bool write_dr = blockIdx.x == 0;
  auto bload = [&](int sl, int k, bool on) -> float4 {    // d_r(t) = out_diff(t) + slabs   (:367, :391), branch-free
    const int s = min(sbase + sl, S - 1), kk = min(k, R - 4);
    float4 v = ldg4(a.out_diff + (size_t)((t - 1) * S + s) * a.od_stride + kk);
    float4 p[KSMAX];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++) p[ks] = ldg4(a.part + ((size_t)(ks < a.nslab ? ks : 0) * S + s) * R + kk);
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++) {
      const bool use = ks < a.nslab;                     // fixed summation order; unused slabs add exactly +0 (select, not
      v.x += use ? p[ks].x : 0.f; v.y += use ? p[ks].y : 0.f;   // multiply: a never-written slab may hold NaN bit patterns)
      v.z += use ? p[ks].z : 0.f; v.w += use ? p[ks].w : 0.f;
    }
    return keep_if(v, on && sbase + sl < S && k < R);
  };
  auto bside = [&](int sl, int k, const float4 &v) {
    const int s = sbase + sl;
    if (write_dr && s < S && k < R) *reinterpret_cast<float4 *>(a.dr + ((size_t)t * S + s) * R + k) = v;
  };
  vec_contract<NT, CPW, SMALL, BF>(va.wpk + (size_t)blockIdx.x * nch * (BF ? 64 : 128), nch, NT * TS_, ldsB, lane, wave, acc, bload, bside, epi);
  VEC_COMBINE();

  if constexpr (SMALL) {
    if (s_on) {
      // rows 4q..4q+3 of stream j live in red[w][nt][4q + j] (k-groups already combined in-wave): this lane's cell is
      // component (lane/4)%4 of q = lane/16
      const float *rp = reinterpret_cast<const float *>(&red[0][wave][((lane >> 4) << 2) | (lane & 3)]) + ((lane >> 2) & 3);
      float dmv = rp[0];
#pragma unroll
      for (int w = 1; w < NW; w++) dmv += rp[(size_t)w * NT * 64 * 4];
      const float d_h = k_diff_tanh(dmv * sy[3], sy[4]);         // :411-412
      const float d_o = k_diff_sigmoid(dmv * sy[4], sy[3]);      // :415-416
      float d_c = d_h;                                           // :424
      d_c = d_c + sy[6] * sy[7];                                 // :425
      d_c = d_c + sy[10] * sy[8];                                // :426
      d_c = d_c + sy[11] * sy[9];                                // :427
      d_c = d_c + sy[12] * d_o;                                  // :428
      float *dp = a.dgifo + srow * 4 * C + s_cell;
      dp[0] = k_diff_tanh(d_c * sy[1], sy[0]);                   // :439-440
      dp[C] = k_diff_sigmoid(d_c * sy[0], sy[1]);                // :435-436
      dp[2 * C] = k_diff_sigmoid(d_c * sy[5], sy[2]);            // :431-432
      dp[3 * C] = d_o;
      a.dc[srow * C + s_cell] = d_c;
    }
    return;
  }
  if (e_on) {
    const f32x4 v = reduce_tile<NT, SMALL>(red, wave, lane);
    const float dm[4] = {v.x, v.y, v.z, v.w};
    float og[4], oi[4], of[4], oo[4], oc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float d_h = k_diff_tanh(dm[j] * yo[j], yh[j]);       // :411-412
      const float d_o = k_diff_sigmoid(dm[j] * yh[j], yo[j]);    // :415-416
      float d_c = d_h;                                           // :424
      d_c = d_c + dcn[j] * fn[j];                                // :425
      d_c = d_c + wpi[j] * din[j];                               // :426
      d_c = d_c + wpf[j] * dfn[j];                               // :427
      d_c = d_c + wpo[j] * d_o;                                  // :428
      of[j] = k_diff_sigmoid(d_c * cpv[j], yf[j]);               // :431-432
      oi[j] = k_diff_sigmoid(d_c * yg[j], yi[j]);                // :435-436
      og[j] = k_diff_tanh(d_c * yi[j], yg[j]);                   // :439-440
      oo[j] = d_o;
      oc[j] = d_c;
    }
    float *dp = a.dgifo + row * 4 * C;
    store4<true>(dp, cb, C, og);
    store4<true>(dp + C, cb, C, oi);
    store4<true>(dp + 2 * C, cb, C, of);
    store4<true>(dp + 3 * C, cb, C, oo);
    store4<true>(a.dc + row * C, cb, C, oc);
  }
}

// =============================================================================================
// MANY-STREAM VECTOR PATH (NumStream > 16 per GPU).  The tiles above make every workgroup re-stage the
// activations of ALL its streams and finish with stream-major (scattered) epilogues -- fine while a step is
// latency-bound, 10x off the MFMA roofline at 64+ streams.  Here the unit of work is one
// (16-row weight tile, 16-stream tile) pair per wave so that every SIMD gets an MFMA chain of 50-64
// instructions: a workgroup = MTW row tiles x KSW K-splits on ONE 16-stream tile (MTW*KSW = 8 waves),
// grid = (row tiles / MTW) x (stream tiles).  The B slab (16 streams x up to 512 k) is staged once and
// shared by the MTW row tiles, the K splits are combined through LDS in fixed order, and the result tile
// [16 streams][MTW*16 rows] is consumed by a coalesced elementwise pass (thread = one stream x one 16-byte
// row segment) whose operands were requested at kernel start.
// =============================================================================================
constexpr int FST = 16;                    // streams per workgroup
// FS = K chunks per slab (16 or 32: the whole contraction in one slab whenever K <= 1024);
// LDS row stride of the B slab FS*32 + 4 floats: conflict-free b128 reads

template <int MTW, int KSW, int FS, bool BF, class BL, class BS>
__device__ __forceinline__ void fat_contract(const float4 *__restrict__ apk, int nch, float *ldsB, int lane, int ksp,
                                             f32x4 (&acc)[2], const BL &bload, const BS &bside) {
  constexpr int FLDB = FS * KCH + 4, FLDBH = FS * KCH + 8;
  constexpr int PER = FS / KSW;              // max chunks of a slab per K split
  constexpr int AU = BF ? 64 : 128;
  unsigned short *ldsH = reinterpret_cast<unsigned short *>(ldsB);
  const int bs = lane & 15, kg = lane >> 4;
  // first slab peeled out of the loop and the activation slab requested before the weights: see vec_contract
  auto iter = [&](int base) {
    const int nc = min(FS, nch - base);
    const int per = (nc + KSW - 1) / KSW;
    const int c0 = ksp * per;
    constexpr int F4ROW = FS * 8, U = (FST * F4ROW) / (NW * 64);
    float4 sv[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int idx = threadIdx.x + u * NW * 64;
      const int sl = idx / F4ROW, k = (idx % F4ROW) * 4;
      sv[u] = bload(sl, base * KCH + k, k < nc * KCH);
    }
    float4 a0[PER], a1[PER];
#pragma unroll
    for (int c = 0; c < PER; c++) {
      const int cl = min(c0 + c, nc - 1);
      const float4 *ap = apk + (size_t)(base + cl) * AU + lane;
      a0[c] = ap[0]; a1[c] = BF ? a0[c] : ap[64];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int idx = threadIdx.x + u * NW * 64;
      const int sl = idx / F4ROW, k = (idx % F4ROW) * 4;
      if (k < nc * KCH) {
        if constexpr (BF) *reinterpret_cast<uint2 *>(ldsH + sl * FLDBH + k) = pack_bf16x4(sv[u]);
        else *reinterpret_cast<float4 *>(ldsB + sl * FLDB + k) = sv[u];
        bside(sl, base * KCH + k, sv[u]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < PER; c++) {
      if (c < per && c0 + c < nc) {
        if constexpr (BF) {
          const float4 braw = *reinterpret_cast<const float4 *>(ldsH + bs * FLDBH + (c0 + c) * KCH + kg * 8);
          acc[c & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a0[c]), __builtin_bit_cast(bf16x8, braw), acc[c & 1], 0, 0, 0);
          continue;
        }
        const float av[8] = {a0[c].x, a0[c].y, a0[c].z, a0[c].w, a1[c].x, a1[c].y, a1[c].z, a1[c].w};
        const float *bp = ldsB + bs * FLDB + (c0 + c) * KCH + kg * 8;
        const float4 b0 = *reinterpret_cast<const float4 *>(bp), b1 = *reinterpret_cast<const float4 *>(bp + 4);
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j & 1] = MFMA16(av[j], bv[j], acc[j & 1]);
      }
    }
    if (base + FS < nch) __syncthreads();
  };
  if (nch > 0) iter(0);
  for (int base = FS; base < nch; base += FS) iter(base);
}

// K-split combine (fixed order) + scatter of the MFMA tiles into the result tile rt[stream][row], row stride RTS.
// GATES: tile row 4q+reg is (cell mt*4+q, gate reg) -> rt column gate*(4*MTW) + cell;  else row mt*16 + 4q + reg.
template <int MTW, int KSW, bool GATES>
__device__ __forceinline__ void fat_combine(f32x4 (&acc)[2], f32x4 (*red)[MTW][64], float *rt, int lane, int mt, int ksp) {
  constexpr int RTS = MTW * 16 + 4;
  if (ksp > 0) red[ksp - 1][mt][lane] = acc[0] + acc[1];
  __syncthreads();
  if (ksp == 0) {
    f32x4 v = acc[0] + acc[1];
#pragma unroll
    for (int p = 0; p < KSW - 1; p++) v += red[p][mt][lane];
    const int q = lane >> 4;
    float *rp = rt + (lane & 15) * RTS;
    if (GATES) { const int cl = mt * 4 + q; rp[cl] = v.x; rp[4 * MTW + cl] = v.y; rp[8 * MTW + cl] = v.z; rp[12 * MTW + cl] = v.w; }
    else *reinterpret_cast<float4 *>(rp + mt * 16 + 4 * q) = make_float4(v.x, v.y, v.z, v.w);
  }
  __syncthreads();
}

#define FAT_PROLOGUE()                                                                           \
  if ((int)blockIdx.x >= va.gx) return;      /* grid.x is padded to a multiple of 8 (XCD affinity of row tiles) */ \
  const int lane = threadIdx.x & 63;                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                             \
  const int mt = wave % MTW, ksp = wave / MTW;                                                   \
  constexpr int RTS = MTW * 16 + 4;                                                              \
  __shared__ __attribute__((aligned(16))) float ldsB[FST * (FS * KCH + 4)];                      \
  __shared__ f32x4 red[KSW - 1][MTW][64];                                                        \
  __shared__ __attribute__((aligned(16))) float rt[FST * RTS];                                   \
  f32x4 acc[2] = {(f32x4){0, 0, 0, 0}, (f32x4){0, 0, 0, 0}}

template <int MTW, int KSW, int FS, bool FUSEX, bool BF>
__global__ __launch_bounds__(NW * 64) void k_gates_f(GatesVArgs va) {
  const GatesArgs &a = va.g;
  FAT_PROLOGUE();
  constexpr int CELLS = 4 * MTW;
  const int C = a.C, R = a.R, S = a.S, I = a.I, t = a.t;
  const int c0 = blockIdx.x * CELLS;
  const int sbase = blockIdx.y * FST;
  // elementwise operands: thread = (stream sbase + tid/CELLS, cell c0 + tid%CELLS)
  const int sl_e = threadIdx.x / CELLS, j_e = threadIdx.x % CELLS;
  const int e_s = sbase + sl_e, e_cell = c0 + j_e;
  const bool e_on = sl_e < FST && e_s < S && e_cell < C;
  const int l_cell = e_on ? e_cell : 0, l_s = e_on ? e_s : 0;
  const size_t e_row = (size_t)t * S + l_s;
  float pre[4];
#pragma unroll
  for (int g = 0; g < 4; g++) pre[g] = FUSEX ? a.bias[g * C + l_cell] : a.gifo[e_row * 4 * C + g * C + l_cell];
  const float cp = a.cprev[(size_t)l_s * C + l_cell];
  const float wpi = a.pi[l_cell], wpf = a.pf[l_cell], wpo = a.po[l_cell];

  const int nchR = (R + KCH - 1) / KCH, Rp = nchR * KCH;
  const int nch = nchR + (FUSEX ? (I + KCH - 1) / KCH : 0);
  const bool mirror_r = a.r_mirror != nullptr && blockIdx.x == 0;
  auto bload = [&](int sl, int k, bool on) -> float4 {    // B = [ r(t-1) | pad | x(t) | pad ], branch-free
    const int s = min(sbase + sl, S - 1);
    const bool inr = k < R, inx = FUSEX && k >= Rp && k - Rp < I;
    const float *p = inr ? a.rprev + (size_t)s * R + k : inx ? a.x + (size_t)s * a.x_stride + (k - Rp) : a.rprev;
    const float4 v = ldg4(p);
    return keep_if(v, on && sbase + sl < S && (inr || inx));
  };
  auto bside = [&](int sl, int k, const float4 &v) {
    const int s = sbase + sl;
    if (mirror_r && s < S && k < R) *reinterpret_cast<float4 *>(a.r_mirror + (size_t)s * R + k) = v;
  };
  fat_contract<MTW, KSW, FS, BF>(va.wpk + (size_t)(blockIdx.x * MTW + mt) * va.nch_total * (BF ? 64 : 128), nch, ldsB, lane, ksp, acc, bload, bside);
  fat_combine<MTW, KSW, true>(acc, red, rt, lane, mt, ksp);

  if (e_on) {
    const float *rp = rt + sl_e * RTS + j_e;
    float ag = rp[0] + pre[0];
    float ai = rp[CELLS] + pre[1];
    float af = rp[2 * CELLS] + pre[2];
    float ao = rp[3 * CELLS] + pre[3];
    ai += wpi * cp;                                // :278
    af += wpf * cp;                                // :281
    const float gi = k_sigmoid(ai), gf = k_sigmoid(af), gg = k_tanh(ag);   // :284-288
    float c = gg * gi;                             // :291
    c = c + cp * gf;                               // :294
    c = c < -50.f ? -50.f : c;                     // :296
    c = c > 50.f ? 50.f : c;                       // :297
    const float h = k_tanh(c);                     // :300
    ao += wpo * c;                                 // :303
    const float go = k_sigmoid(ao);                // :306
    const float m = h * go;                        // :309
    float *gp = a.gifo + e_row * 4 * C + e_cell;
    gp[0] = gg; gp[C] = gi; gp[2 * C] = gf; gp[3 * C] = go;
    a.cc[e_row * C + e_cell] = c;
    a.hh[e_row * C + e_cell] = h;
    a.mm[e_row * C + e_cell] = m;
    if (a.c_mirror) a.c_mirror[(size_t)e_s * C + e_cell] = cp;   // :231 (c columns)
    if (a.c_save) a.c_save[(size_t)e_s * C + e_cell] = c;         // :331 (c columns)
  }
}

template <int MTW, int KSW, int FS, bool BF>
__global__ __launch_bounds__(NW * 64) void k_proj_f(ProjVArgs va) {
  const ProjArgs &a = va.g;
  FAT_PROLOGUE();
  constexpr int Q = MTW * 4;                         // 16-byte row segments per stream
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int n0 = blockIdx.x * MTW * 16;
  const int sbase = blockIdx.y * FST;
  const int nch = (C + KCH - 1) / KCH;
  const int ntile = min((int)blockIdx.x * MTW + mt, (R + 15) / 16 - 1);      // clamped: rows past R are dropped below
  const float *mrow = a.mm + (size_t)t * S * C;
  auto bload = [&](int sl, int k, bool on) -> float4 {
    const float4 v = ldg4(mrow + (size_t)min(sbase + sl, S - 1) * C + min(k, C - 4));
    return keep_if(v, on && sbase + sl < S && k < C);
  };
  fat_contract<MTW, KSW, FS, BF>(va.wpk + (size_t)ntile * nch * (BF ? 64 : 128), nch, ldsB, lane, ksp, acc, bload, NoSide());
  fat_combine<MTW, KSW, false>(acc, red, rt, lane, mt, ksp);
  const int sl_e = threadIdx.x / Q, j_e = threadIdx.x % Q;
  const int s = sbase + sl_e, n = n0 + 4 * j_e;
  if (sl_e < FST && s < S && n < R) {
    const float4 v = *reinterpret_cast<const float4 *>(rt + sl_e * RTS + 4 * j_e);
    const float e[4] = {v.x, v.y, v.z, v.w};
    store4<true>(a.rr + ((size_t)t * S + s) * R, n, R, e);
    float *op = a.out + (size_t)((t - 1) * S + s) * a.out_stride;
    if (a.vecOut) store4<true>(op, n, R, e); else store4<false>(op, n, R, e);
    if (a.r_save) store4<true>(a.r_save + (size_t)s * R, n, R, e);
  }
}

template <int MTW, int KSW, int FS, bool BF>
__global__ __launch_bounds__(NW * 64) void k_dr_f(DrVArgs va) {
  const DrArgs &a = va.g;
  FAT_PROLOGUE();
  constexpr int Q = MTW * 4;
  const int R = a.R, I = a.I, S = a.S, K = 4 * a.C;
  const int ntR16 = (R + 15) / 16, ntX16 = (I + 15) / 16;
  const bool is_x = (int)blockIdx.x >= a.ntr;                      // a.ntr counts MTW-tile groups over R here
  const int g = is_x ? (int)blockIdx.x - a.ntr : (int)blockIdx.x;
  const int tile = is_x ? ntR16 + min(g * MTW + mt, ntX16 - 1) : min(g * MTW + mt, ntR16 - 1);
  const int n0 = g * MTW * 16;
  const int N = is_x ? I : R;
  const int sbase = blockIdx.y * FST;
  const int ks = blockIdx.z;
  const int kbeg = ks * a.klen;
  const int kend = min(K, kbeg + a.klen);
  const float *drow = a.dgifo + (size_t)(a.t + 1) * S * K;
  auto bload = [&](int sl, int k, bool on) -> float4 {
    const float4 v = ldg4(drow + (size_t)min(sbase + sl, S - 1) * K + min(kbeg + k, K - 4));
    return keep_if(v, on && sbase + sl < S && kbeg + k < kend);
  };
  fat_contract<MTW, KSW, FS, BF>(va.wpk + ((size_t)tile * va.nch_total + kbeg / KCH) * (BF ? 64 : 128),
                         kend > kbeg ? (kend - kbeg + KCH - 1) / KCH : 0, ldsB, lane, ksp, acc, bload, NoSide());
  fat_combine<MTW, KSW, false>(acc, red, rt, lane, mt, ksp);
  const int sl_e = threadIdx.x / Q, j_e = threadIdx.x % Q;
  const int s = sbase + sl_e, n = n0 + 4 * j_e;
  if (sl_e < FST && s < S && n < N) {
    const float4 v = *reinterpret_cast<const float4 *>(rt + sl_e * RTS + 4 * j_e);
    const float e[4] = {v.x, v.y, v.z, v.w};
    if (is_x) {
      float *xp = a.xpart + ((size_t)ks * S + s) * a.x_ld;
      if (a.vecX) store4<true>(xp, n, I, e); else store4<false>(xp, n, I, e);
    } else {
      store4<true>(a.part + ((size_t)ks * S + s) * R, n, R, e);
    }
  }
}

template <int MTW, int KSW, int FS, bool BF>
__global__ __launch_bounds__(NW * 64) void k_dm_f(DmVArgs va) {
  const DmArgs &a = va.g;
  FAT_PROLOGUE();
  const int C = a.C, R = a.R, S = a.S, t = a.t;
  const int c0 = blockIdx.x * MTW * 16;
  const int sbase = blockIdx.y * FST;
  const bool last = (t == a.T);

  reduce_x_slabs(a, sbase, min(S, sbase + FST), blockIdx.x, va.gx);

  // elementwise operands, requested before the contraction: thread = (stream, ONE cell) -- 16 streams x 16*MTW cells
  // = 256*MTW of the 512 threads (a thread that walks four cells runs four dependent chains of cell math in a row)
  constexpr int NC = MTW * 16;
  const int sl_e = threadIdx.x / NC, j_e = threadIdx.x % NC;
  const int e_s = sbase + sl_e, e_c = c0 + j_e;
  const bool e_on = sl_e < FST && e_s < S && e_c < C;
  const int lc = e_on ? e_c : 0;
  const size_t row = (size_t)t * S + (e_on ? e_s : 0);
  const bool n_on = e_on && !last;
  const size_t rn = last ? row : row + S;                // clamped: block T+1 is never dereferenced
  const float *yp = a.gifo + row * 4 * C + lc;
  const float yg = yp[0], yi = yp[C], yf = yp[2 * C], yo = yp[3 * C];
  const float yh = a.hh[row * C + lc], cpv = a.cc[(row - S) * C + lc];
  const float dcn_r = a.dc[rn * C + lc], fn_r = a.gifo[rn * 4 * C + 2 * C + lc];
  const float din_r = a.dgifo[rn * 4 * C + C + lc], dfn_r = a.dgifo[rn * 4 * C + 2 * C + lc];
  const float wpi = a.pi[lc], wpf = a.pf[lc], wpo = a.po[lc];

  const int nch = (R + KCH - 1) / KCH;
  const int ctile = min((int)blockIdx.x * MTW + mt, (C + 15) / 16 - 1);
  const bool write_dr = blockIdx.x == 0;
  auto bload = [&](int sl, int k, bool on) -> float4 {    // d_r(t) = out_diff(t) + slabs   (:367, :391), branch-free
    const int s = min(sbase + sl, S - 1), kk = min(k, R - 4);
    float4 v = ldg4(a.out_diff + (size_t)((t - 1) * S + s) * a.od_stride + kk);
    float4 p[KSMAX];
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++) p[ks] = ldg4(a.part + ((size_t)(ks < a.nslab ? ks : 0) * S + s) * R + kk);
#pragma unroll
    for (int ks = 0; ks < KSMAX; ks++) {
      const bool use = ks < a.nslab;                     // fixed summation order; unused slabs add exactly +0 (select, not
      v.x += use ? p[ks].x : 0.f; v.y += use ? p[ks].y : 0.f;   // multiply: a never-written slab may hold NaN bit patterns)
      v.z += use ? p[ks].z : 0.f; v.w += use ? p[ks].w : 0.f;
    }
    return keep_if(v, on && sbase + sl < S && k < R);
  };
  auto bside = [&](int sl, int k, const float4 &v) {
    const int s = sbase + sl;
    if (write_dr && s < S && k < R) *reinterpret_cast<float4 *>(a.dr + ((size_t)t * S + s) * R + k) = v;
  };
  fat_contract<MTW, KSW, FS, BF>(va.wpk + (size_t)ctile * nch * (BF ? 64 : 128), nch, ldsB, lane, ksp, acc, bload, bside);
  fat_combine<MTW, KSW, false>(acc, red, rt, lane, mt, ksp);

  if (e_on) {
    const float dm = rt[sl_e * RTS + j_e];
    const float dcn = n_on ? dcn_r : 0.f, fn = n_on ? fn_r : 0.f, din = n_on ? din_r : 0.f, dfn = n_on ? dfn_r : 0.f;
    const float d_h = k_diff_tanh(dm * yo, yh);                  // :411-412
    const float d_o = k_diff_sigmoid(dm * yh, yo);               // :415-416
    float d_c = d_h;                                             // :424
    d_c = d_c + dcn * fn;                                        // :425
    d_c = d_c + wpi * din;                                       // :426
    d_c = d_c + wpf * dfn;                                       // :427
    d_c = d_c + wpo * d_o;                                       // :428
    float *dp = a.dgifo + row * 4 * C + e_c;
    dp[0] = k_diff_tanh(d_c * yi, yg);                           // :439-440
    dp[C] = k_diff_sigmoid(d_c * yg, yi);                        // :435-436
    dp[2 * C] = k_diff_sigmoid(d_c * cpv, yf);                   // :431-432
    dp[3 * C] = d_o;
    a.dc[row * C + e_c] = d_c;
  }
}

// =============================================================================================
// FOLDED RECURRENCE (NumStream <= small_max, engine option "fold").  At 4-12 streams a step is pure latency:
// two dependent kernels per direction (gates needs all of r, the projection all of m), ~4 us each, MFMA idle.
// With  W_rm = W_gifo_r * W_r_m  [4C x C]  (recomputed after every Update) the recurrence closes over m alone:
//     forward   a(t)   = W_x x(t) + b + W_rm m(t-1)                          (t >= 2; t = 1 uses the carried r, :275)
//     backward  d_m(t) = out_diff(t) W_r_m + dgifo(t+1) W_rm                 (:391 substituted into :408)
// ONE kernel per step and direction; r(1..T) (:312), d_r(1..T) (:391) and in_diff (:457) become batched GEMMs
// outside the chain.  Same algebra as the reference up to fp32 summation order (the parity tests run both paths).
// The forward step is k_gates_v itself with B = m(t-1) and the packed [W_rm | W_x]; the backward step needs a
// contraction over K = 4C for only C rows, i.e. 4-row tiles to fill the chip:
//   4-row geometry of the 4x4x1_16b MFMA: block b = k-group (16 of them), A lane 4b+i = row i, B lane 4b+j = stream j,
//   chunk = 16 k-groups x 8 = 128 k;  packed weights pk[tile4][chunk][h][lane][4]: row = 4*tile + (lane&3),
//   k = 128*chunk + 64h + 4*(lane>>2) + e.
// =============================================================================================

// acc += A(4 rows, chunks [0,nch)) * B(4 streams, same chunks).  Chunk c is dealt to wave c % NW.  No LDS staging: the B
// operand of consumer lane 4b+j (k-group b, stream j) is float4 b of each 64-float half of the chunk in stream j's row;
// it is FETCHED by loader lane 16j+b, so that a load instruction covers 4 x 256 contiguous bytes (lanes of a quad on
// one cache line -- a quad spread over four rows costs four tag lookups), and moved with ds_bpermute.
// brow: row pointer of the LOADER lane's stream (clamped), bok: the CONSUMER lane's stream exists.
__device__ __forceinline__ float perm(int byte_idx, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(byte_idx, __builtin_bit_cast(int, v)));
}
// NG stream groups of 4 share one fetch of the weight chunk.  brow: row pointer of the LOADER lane's stream within group 0
// (clamped per group by the caller through gstride = 4*K or 0), bok[g]: the CONSUMER lane's stream of group g exists.
template <int CPW, int NG>
__device__ __forceinline__ void vec_contract_r4(const float4 *__restrict__ apk, int nch, int K, const float *const (&brow)[NG],
                                                const bool (&bok)[NG], int lane, int wave, int rot, f32x4 (&acc)[NG][2]) {
  const int kg = lane >> 2;
  for (int base = 0; base < nch; base += CPW * NW) {
    float4 a0[CPW], a1[CPW], b0[NG][CPW], b1[NG][CPW];
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      const int ch = base + c * NW + wave;
      int cl = min(ch, nch - 1) + rot;                             // clamped: always a valid chunk, unused if off
      cl = cl >= nch ? cl - nch : cl;                              // rotated: see k_dmf_v
      const float4 *ap = apk + (size_t)cl * 128 + lane;
      a0[c] = ap[0]; a1[c] = ap[64];
      // loader role: lane = 16*stream + q fetches float4 q of each 64-float half of the chunk (4 x 256 contiguous bytes
      // per instruction); the consumer lane 4b+j takes its operand from loader lane 16j+b below
      const int k = cl * KCH4 + (lane & 15) * 4;
#pragma unroll
      for (int g = 0; g < NG; g++) { b0[g][c] = ldg4(brow[g] + min(k, K - 4)); b1[g][c] = ldg4(brow[g] + min(k + 64, K - 4)); }
    }
#pragma unroll
    for (int c = 0; c < CPW; c++) {
      const int ch = base + c * NW + wave;
      int cl = min(ch, nch - 1) + rot;
      cl = cl >= nch ? cl - nch : cl;
      const bool k0 = ch < nch && cl * KCH4 + kg * 4 < K, k1 = ch < nch && cl * KCH4 + 64 + kg * 4 < K;
      const float av[8] = {a0[c].x, a0[c].y, a0[c].z, a0[c].w, a1[c].x, a1[c].y, a1[c].z, a1[c].w};
      const int src = (((lane & 3) << 4) | kg) << 2;               // byte index of loader lane 16j+b
#pragma unroll
      for (int g = 0; g < NG; g++) {
        const bool on0 = k0 && bok[g], on1 = k1 && bok[g];
        const float p[8] = {perm(src, b0[g][c].x), perm(src, b0[g][c].y), perm(src, b0[g][c].z), perm(src, b0[g][c].w),
                            perm(src, b1[g][c].x), perm(src, b1[g][c].y), perm(src, b1[g][c].z), perm(src, b1[g][c].w)};
        const float bv[8] = {on0 ? p[0] : 0.f, on0 ? p[1] : 0.f, on0 ? p[2] : 0.f, on0 ? p[3] : 0.f,
                             on1 ? p[4] : 0.f, on1 ? p[5] : 0.f, on1 ? p[6] : 0.f, on1 ? p[7] : 0.f};
#pragma unroll
        for (int j = 0; j < 8; j++) acc[g][j & 1] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[j], bv[j], acc[g][j & 1], 0, 0, 0);
      }
    }
  }
}

struct DmfArgs {
  int C, S, T, t;
  const float *pi, *pf, *po;
  const float *gifo, *cc, *hh;
  float *dgifo, *dc;
  const float *P;          // out_diff * W_r_m for all frames [T*S x C]
  const float4 *wpk;       // packed W_rm^T, 4-row geometry: [C/4 tiles][nch_total chunks][2][64]
  int nch_total;           // chunks of 128 over 4C
  int nch;                 // chunks to contract: nch_total, or 0 at t == T (dgifo(T+1) = 0, :351)
};

template <int CPW, int NG>
__global__ __launch_bounds__(NW * 64) void k_dmf_v(DmfArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __shared__ f32x4 red[NW][NG][4];
  const int C = a.C, S = a.S, t = a.t, K = 4 * a.C;
  const int c0 = blockIdx.x * 4;
  const int sbase = blockIdx.y * 4 * NG;
  const bool last = (t == a.T);

  // ---- epilogue operands first: lanes 0..15 of wave g = (cell c0 + lane/4, stream sbase + 4g + lane%4): one cell per
  //      lane, so the 15-operation cell math is one short dependent chain instead of four in a row ----
  const int e_i = (lane >> 2) & 3, e_j = lane & 3;
  const int e_s = sbase + 4 * wave + e_j, e_c = c0 + e_i;
  const bool e_on = wave < NG && lane < 16 && e_s < S && e_c < C;
  const size_t row = (size_t)t * S + (e_on ? e_s : 0), rown = row + S, rowp = row - S;
  const int lc = e_on ? e_c : 0;
  const bool n_on = e_on && !last;
  const size_t rn = last ? row : rown;                   // clamped: block T+1 is never dereferenced
  const float *yp = a.gifo + row * 4 * C + lc;
  const float yg = yp[0], yi = yp[C], yf = yp[2 * C], yo = yp[3 * C];
  const float yh = a.hh[row * C + lc], cpv = a.cc[rowp * C + lc];
  const float dcn_r = a.dc[rn * C + lc], fn_r = a.gifo[rn * 4 * C + 2 * C + lc];
  const float din_r = a.dgifo[rn * 4 * C + C + lc], dfn_r = a.dgifo[rn * 4 * C + 2 * C + lc];
  const float wpi = a.pi[lc], wpf = a.pf[lc], wpo = a.po[lc];
  const float pv = a.P[(row - S) * C + lc];              // frame t is row block t-1 of P

  f32x4 acc[NG][2];
  const float *brow[NG];
  bool bok[NG];
#pragma unroll
  for (int g = 0; g < NG; g++) {
    acc[g][0] = (f32x4){0, 0, 0, 0}; acc[g][1] = (f32x4){0, 0, 0, 0};
    bok[g] = sbase + 4 * g + (lane & 3) < S;                                                          // consumer role
    brow[g] = a.dgifo + ((size_t)(last ? t : t + 1) * S + min(sbase + 4 * g + (lane >> 4), S - 1)) * K;   // loader role
  }
  // every workgroup reads the SAME activation rows: started at the same chunk they would all hit one L2 channel at a
  // time, so workgroup w walks the chunks rotated by 7w (the weights are private, their order does not matter)
  const int rot = a.nch > 0 ? (int)((blockIdx.x * 7u) % (unsigned)a.nch) : 0;
  vec_contract_r4<CPW, NG>(a.wpk + (size_t)blockIdx.x * a.nch_total * 128, a.nch, K, brow, bok, lane, wave, rot, acc);

  // the 16 k-groups of a (row, stream) pair sit in the lanes with equal lane&3: xor butterfly (a+b == b+a bitwise, so
  // every lane ends with the same sum), then the 8 waves in fixed order
#pragma unroll
  for (int g = 0; g < NG; g++) {
    f32x4 v = acc[g][0] + acc[g][1];
#pragma unroll
    for (int m = 4; m < 64; m <<= 1) {
      v.x += __shfl_xor(v.x, m); v.y += __shfl_xor(v.y, m); v.z += __shfl_xor(v.z, m); v.w += __shfl_xor(v.w, m);
    }
    if (lane < 4) red[wave][g][lane] = v;
  }
  __syncthreads();

  if (e_on) {
    // row (cell) e_i of stream e_j: component e_i of red[w][wave][e_j]
    const float *rp = reinterpret_cast<const float *>(&red[0][0][0]) + (wave * 4 + e_j) * 4 + e_i;
    float sum = rp[0];
#pragma unroll
    for (int w = 1; w < NW; w++) sum += rp[w * NG * 16];
    const float dm = sum + pv;                                   // :408 with :391 substituted
    const float dcn = n_on ? dcn_r : 0.f, fn = n_on ? fn_r : 0.f, din = n_on ? din_r : 0.f, dfn = n_on ? dfn_r : 0.f;
    const float d_h = k_diff_tanh(dm * yo, yh);                  // :411-412
    const float d_o = k_diff_sigmoid(dm * yh, yo);               // :415-416
    float d_c = d_h;                                             // :424
    d_c = d_c + dcn * fn;                                        // :425
    d_c = d_c + wpi * din;                                       // :426
    d_c = d_c + wpf * dfn;                                       // :427
    d_c = d_c + wpo * d_o;                                       // :428
    const float o_f = k_diff_sigmoid(d_c * cpv, yf);             // :431-432
    const float o_i = k_diff_sigmoid(d_c * yg, yi);              // :435-436
    const float o_g = k_diff_tanh(d_c * yi, yg);                 // :439-440
    float *dp = a.dgifo + row * 4 * C + e_c;
    dp[0] = o_g; dp[C] = o_i; dp[2 * C] = o_f; dp[3 * C] = d_o;
    a.dc[row * C + e_c] = d_c;
    if (last) {     // the batched d_r product reads dgifo(T+1) as rows of its operand: keep that block zero (:351) even
      float *zp = a.dgifo + rown * 4 * C + e_c;                  // after a longer minibatch has used it
      zp[0] = 0.f; zp[C] = 0.f; zp[2 * C] = 0.f; zp[3 * C] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// ---- variant selection -------------------------------------------------------------------------
// generic kernels (any shape): 16 x 16*NT stream tiles, NT in {1,2,4,8}
static inline int pick_nt(int S) {
  const int tiles = cdiv(S, 16);
  return tiles >= 8 ? 8 : tiles >= 4 ? 4 : tiles >= 2 ? 2 : 1;
}
#define GEN_DISPATCH(KERN, nt, grid, st, pr, args, ...)                                           \
  do {                                                                                            \
    const dim3 _blk(NW * 64);                                                                     \
    if (nt == 1) return launch((KERN<1 __VA_ARGS__>), grid, _blk, 0, st, pr, args);               \
    if (nt == 2) return launch((KERN<2 __VA_ARGS__>), grid, _blk, 0, st, pr, args);               \
    if (nt == 4) return launch((KERN<4 __VA_ARGS__>), grid, _blk, 0, st, pr, args);               \
    return launch((KERN<8 __VA_ARGS__>), grid, _blk, 0, st, pr, args);                            \
  } while (0)
// vector kernels: SMALL (4x4x1_16b, S <= 4) with CPW in {1,2,4};  16x16x4 with (NT,CPW) in {(1,1),(1,2),(2,1),(4,1)}
struct VecCfg { bool small; int nt, cpw; };
int g_fat_fine = -1;            // many-stream kernels with half-size row tiles: -1 auto (<= 64 streams), 0 never, 1 always
// measured, fwd+bwd+update us with full-size / half-size row tiles: 512->1024/512 at 32 streams 744 / 653 (gates 6.7 -> 5.3,
// proj 5.7 -> 4.1 us: the full-size tiles leave half the chip without a workgroup); 40/800/512: 32 streams 650 / 561,
// 64: 755 / 710, 128: 1056 / 1102
static inline bool fat_fine(int S) { return g_fat_fine >= 1 || (g_fat_fine < 0 && S <= 64); }
int g_small_nt2 = -1;         // -1 auto, 0 never, 1 always
int g_small_max = 16;           // largest NumStream served by the 4x4x1_16b geometry (4 streams per workgroup, grid.y = S/4);
                                // measured at 40/800/512 (us per minibatch, 4x4x1 vs 16x16x4 tiles): S=8 325 vs 452, S=12 394 vs 460,
                                // S=16 442 vs 474
static inline VecCfg pick_vec(int S, int nch, bool gates = false) {
  VecCfg c;
  const int need = cdiv(nch, NW);
  c.small = S <= g_small_max;
  // two stream groups per workgroup share one fetch of the weight tile: measured at 40/800/512 (g_small_nt2 = 1 forces
  // it everywhere) it only pays for the gates kernel at 9+ streams (7.0 -> 5.7 us at 12; proj/dr/dm lose 0.4-1.0 us)
  if (c.small) { c.nt = (S > 4 && (g_small_nt2 == 1 || (g_small_nt2 < 0 && gates && S > 8))) ? 2 : 1; c.cpw = need <= 1 ? 1 : need == 2 ? 2 : 4; return c; }
  c.nt = S <= 16 ? 1 : S <= 32 ? 2 : 4;
  c.cpw = (c.nt == 1 && need >= 2) ? 2 : 1;
  return c;
}
#define VEC_DISPATCH(KERN, cfg, grid, st, pr, args, ...)                                          \
  do {                                                                                            \
    const dim3 _blk(NW * 64);                                                                     \
    if (cfg.small && cfg.nt == 2) {                                                               \
      if (cfg.cpw == 1) return launch((KERN<2, 1, true __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
      if (cfg.cpw == 2) return launch((KERN<2, 2, true __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
      return launch((KERN<2, 4, true __VA_ARGS__>), grid, _blk, 0, st, pr, args);                 \
    }                                                                                             \
    if (cfg.small) {                                                                              \
      if (cfg.cpw == 1) return launch((KERN<1, 1, true __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
      if (cfg.cpw == 2) return launch((KERN<1, 2, true __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
      return launch((KERN<1, 4, true __VA_ARGS__>), grid, _blk, 0, st, pr, args);                 \
    }                                                                                             \
    if (cfg.nt == 1 && cfg.cpw == 1) return launch((KERN<1, 1, false __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
    if (cfg.nt == 1) return launch((KERN<1, 2, false __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
    if (cfg.nt == 2) return launch((KERN<2, 1, false __VA_ARGS__>), grid, _blk, 0, st, pr, args); \
    return launch((KERN<4, 1, false __VA_ARGS__>), grid, _blk, 0, st, pr, args);                  \
  } while (0)
// many-stream kernels (FwdPtrs / BwdPtrs::fat, S > 16), MTW row tiles x KSW K splits per workgroup: (MF, KF) with the half-size
// row tiles of fat_fine (`fine`), else (MC, KC); FS = chunks of the stream slab (16, or 32 for a long contraction)
#define FAT_DISPATCH(KERN, fine, MF, KF, MC, KC, FS, grid, st, pr, args, ...)                     \
  do {                                                                                            \
    const dim3 _blk(NW * 64);                                                                     \
    if (fine) return launch((KERN<MF, KF, FS __VA_ARGS__>), grid, _blk, 0, st, pr, args);         \
    return launch((KERN<MC, KC, FS __VA_ARGS__>), grid, _blk, 0, st, pr, args);                   \
  } while (0)
#define COMMA ,
static inline dim3 vec_grid(int ntiles, int S, const VecCfg &c, int z = 1) {
  return dim3(ntiles, cdiv(S, (c.small ? 4 : 16) * c.nt), z);
}

hipError_t launch_gates_step(const Dims &d0, const FwdPtrs &p, int t, bool fuse_x, const float *in,
                             int in_stride, hipStream_t st, LaunchProbe pr, bool fold) {
  // fold (t >= 2, S <= small_max): the recurrent operand is m(t-1) and the packed weights are [W_rm | W_x]; the kernel
  // is the same with R := C
  Dims d = d0;
  if (fold) d.R = d0.C;
  GatesArgs a;
  a.C = d.C; a.R = d.R; a.S = d.S; a.I = d.I; a.t = t;
  a.wr = p.wr; a.wx = p.wx; a.bias = p.bias; a.pi = p.pi; a.pf = p.pf; a.po = p.po;
  a.gifo = p.gifo; a.cc = p.cc; a.hh = p.hh; a.mm = p.mm;
  a.cprev = t == 1 ? p.prev_c : p.cc + (size_t)(t - 1) * d.S * d.C;
  a.rprev = fold ? p.mm + (size_t)(t - 1) * d.S * d.C : t == 1 ? p.prev_r : p.rr + (size_t)(t - 1) * d.S * d.R;
  a.x = fuse_x ? in + (size_t)(t - 1) * d.S * in_stride : nullptr;
  a.x_stride = in_stride;
  a.c_mirror = t == 1 ? p.cc : nullptr;
  a.r_mirror = (t == 1 && !fold) ? p.rr : nullptr;
  a.c_save = t == d.T ? p.next_c : nullptr;          // (the carried state is double-buffered: read prev_*, write next_*)
  const float4 *wpk = fold ? p.pk_fold : p.pk_gates;
  const bool vec = wpk != nullptr && aligned16(p.rr) && aligned16(p.prev_r) && aligned16(p.mm) &&
                   (!fuse_x || (aligned16(in) && in_stride % 4 == 0));
  if (fold && !vec) return hipErrorInvalidValue;      // the engine only folds on the vector path
  if (vec) {
    GatesVArgs va; va.g = a; va.wpk = wpk;
    va.nch_total = cdiv(d.R, KCH) + cdiv(d.I, KCH);
    if (p.fat && d.S > 16) {
      // (MTW, KSW) = (4, 2): 4 row tiles (16 cells) x 2 K splits per workgroup; fine (few stream tiles) = (2, 4): 8 cells x 4 K
      // splits -> twice the workgroups.  A 32-chunk slab when the contraction has more than 16 chunks.
      const bool fine = fat_fine(d.S);
      va.gx = cdiv(d.C, fine ? 8 : 16);
      const dim3 fgrid(cdiv(va.gx, 8) * 8, cdiv(d.S, FST));
      const bool big = (fuse_x ? cdiv(d.R, KCH) + cdiv(d.I, KCH) : cdiv(d.R, KCH)) > 16;
      if (p.bf16) {
        if (fuse_x && big) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 32, fgrid, st, pr, va, COMMA true COMMA true);
        if (fuse_x) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 16, fgrid, st, pr, va, COMMA true COMMA true);
        if (big) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 32, fgrid, st, pr, va, COMMA false COMMA true);
        FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 16, fgrid, st, pr, va, COMMA false COMMA true);
      }
      if (fuse_x && big) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 32, fgrid, st, pr, va, COMMA true COMMA false);
      if (fuse_x) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 16, fgrid, st, pr, va, COMMA true COMMA false);
      if (big) FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 32, fgrid, st, pr, va, COMMA false COMMA false);
      FAT_DISPATCH(k_gates_f, fine, 2, 4, 4, 2, 16, fgrid, st, pr, va, COMMA false COMMA false);
    }
    const VecCfg cfg = pick_vec(d.S, cdiv(d.R, KCH) + (fuse_x ? cdiv(d.I, KCH) : 0), true);
    const dim3 grid = vec_grid(cdiv(d.C, 4), d.S, cfg);
    if (p.bf16) {
      if (fuse_x) VEC_DISPATCH(k_gates_v, cfg, grid, st, pr, va, COMMA true COMMA true);
      VEC_DISPATCH(k_gates_v, cfg, grid, st, pr, va, COMMA false COMMA true);
    }
    if (fuse_x) VEC_DISPATCH(k_gates_v, cfg, grid, st, pr, va, COMMA true COMMA false);
    VEC_DISPATCH(k_gates_v, cfg, grid, st, pr, va, COMMA false COMMA false);
  }
  const int nt = pick_nt(d.S);
  const dim3 grid(cdiv(d.C, 4), cdiv(d.S, 16 * nt));
  if (fuse_x) GEN_DISPATCH(k_gates_step, nt, grid, st, pr, a, COMMA true);
  GEN_DISPATCH(k_gates_step, nt, grid, st, pr, a, COMMA false);
}

hipError_t launch_proj_step(const Dims &d, const FwdPtrs &p, int t, float *out, int out_stride,
                            hipStream_t st, LaunchProbe pr) {
  ProjArgs a;
  a.C = d.C; a.R = d.R; a.S = d.S; a.t = t;
  a.wm = p.wm; a.mm = p.mm; a.rr = p.rr; a.out = out; a.out_stride = out_stride;
  a.r_save = t == d.T ? p.next_r : nullptr;
  a.vecOut = aligned16(out) && out_stride % 4 == 0 && d.R % 4 == 0;
  const bool vec = p.pk_proj != nullptr && aligned16(p.mm) && aligned16(p.rr) && aligned16(p.prev_r);
  if (vec) {
    ProjVArgs va; va.g = a; va.wpk = p.pk_proj;
    if (p.fat && d.S > 16) {
      // (MTW, KSW) = (2, 4): two 16-row tiles x 4 K splits per workgroup; fine = (1, 8): one 16-row tile x 8 K splits
      const bool fine = fat_fine(d.S);
      va.gx = cdiv(d.R, fine ? 16 : 32);
      const dim3 fgrid(cdiv(va.gx, 8) * 8, cdiv(d.S, FST));
      const bool big = cdiv(d.C, KCH) > 16;
      if (p.bf16 && big) FAT_DISPATCH(k_proj_f, fine, 1, 8, 2, 4, 32, fgrid, st, pr, va, COMMA true);
      if (p.bf16) FAT_DISPATCH(k_proj_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA true);
      if (big) FAT_DISPATCH(k_proj_f, fine, 1, 8, 2, 4, 32, fgrid, st, pr, va, COMMA false);
      FAT_DISPATCH(k_proj_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA false);
    }
    const VecCfg cfg = pick_vec(d.S, cdiv(d.C, KCH));
    if (p.bf16) VEC_DISPATCH(k_proj_v, cfg, vec_grid(cdiv(d.R, 16), d.S, cfg), st, pr, va, COMMA true);
    VEC_DISPATCH(k_proj_v, cfg, vec_grid(cdiv(d.R, 16), d.S, cfg), st, pr, va, COMMA false);
  }
  const int nt = pick_nt(d.S);
  const dim3 grid(cdiv(d.R, 16), cdiv(d.S, 16 * nt));
  GEN_DISPATCH(k_proj_step, nt, grid, st, pr, a, );
}

void set_small_max(int s) { g_small_max = s; }
void set_small_nt2(int v) { g_small_nt2 = v; }
void set_fat_fine(int v) { g_fat_fine = v; }
int get_small_max() { return g_small_max; }

int dr_split_k(const Dims &d) {
  // enough (R/16 x KS) workgroups to spread the 4C-long contraction over the chip at small S
  const int K = 4 * d.C;
  int ks = KSMAX;
  while (ks > 1 && cdiv(K, ks) < NW * KCH) ks >>= 1;
  return ks;
}

hipError_t launch_dr_step(const Dims &d, const BwdPtrs &p, int t, float *in_diff, int id_stride,
                          hipStream_t st, LaunchProbe pr) {
  DrArgs a;
  a.C = d.C; a.R = d.R; a.I = d.I; a.S = d.S; a.t = t;
  a.wrT = p.wrT; a.wxT = p.wxT; a.dgifo = p.dgifo; a.part = p.dr_part;
  const int K = 4 * d.C;
  const int ks = t == 0 ? 1 : p.ks;
  a.klen = cdiv(cdiv(K, ks), KCH) * KCH;
  a.ntr = t == 0 ? 0 : cdiv(d.R, 16);
  const int ntx = in_diff ? cdiv(d.I, 16) : 0;
  if (t == 0) { a.xpart = in_diff; a.x_ld = id_stride; }        // frame 1, written in place
  else { a.xpart = p.dx_part; a.x_ld = d.I; }
  a.vecX = aligned16(a.xpart) && a.x_ld % 4 == 0 && d.I % 4 == 0;
  if (a.ntr + ntx == 0) return hipSuccess;
  const bool vec = p.pk_dr != nullptr && aligned16(p.dgifo) && aligned16(p.dr_part);
  if (vec) {
    DrVArgs va; va.g = a; va.wpk = p.pk_dr; va.nch_total = cdiv(K, KCH);
    if (p.fat && d.S > 16) {
      // (MTW, KSW) = (2, 4): 32-row groups (2 row tiles x 4 K splits); fine = (1, 8): 16-row groups (one row tile x 8 K splits)
      const bool fine = fat_fine(d.S);
      const int grp = fine ? 16 : 32;
      va.g.ntr = t == 0 ? 0 : cdiv(d.R, grp);
      va.gx = va.g.ntr + (in_diff ? cdiv(d.I, grp) : 0);
      const dim3 fgrid(cdiv(va.gx, 8) * 8, cdiv(d.S, FST), ks);
      // the slab is 16 chunks whatever the length (a 32-chunk slab was measured slower here: 66 KB of LDS and 16 weight
      // registers per lane cost more in occupancy than the second staging round trip they save)
      if (p.bf16) FAT_DISPATCH(k_dr_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA true);
      FAT_DISPATCH(k_dr_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA false);
    }
    const VecCfg cfg = pick_vec(d.S, cdiv(a.klen, KCH));
    if (p.bf16) VEC_DISPATCH(k_dr_v, cfg, vec_grid(a.ntr + ntx, d.S, cfg, ks), st, pr, va, COMMA true);
    VEC_DISPATCH(k_dr_v, cfg, vec_grid(a.ntr + ntx, d.S, cfg, ks), st, pr, va, COMMA false);
  }
  const int nt = pick_nt(d.S);
  const dim3 grid(a.ntr + ntx, cdiv(d.S, 16 * nt), ks);
  GEN_DISPATCH(k_dr_step, nt, grid, st, pr, a, );
}

hipError_t launch_dm_step(const Dims &d, const BwdPtrs &p, int t, const float *out_diff, int od_stride,
                          float *in_diff, int id_stride, hipStream_t st, LaunchProbe pr) {
  DmArgs a;
  a.C = d.C; a.R = d.R; a.I = d.I; a.S = d.S; a.T = d.T; a.t = t;
  a.wmT = p.wmT; a.pi = p.pi; a.pf = p.pf; a.po = p.po;
  a.gifo = p.gifo; a.cc = p.cc; a.hh = p.hh;
  a.dgifo = p.dgifo; a.dc = p.dc; a.dr = p.dr;
  a.part = p.dr_part; a.nslab = (t == d.T) ? 0 : p.ks;
  a.out_diff = out_diff; a.od_stride = od_stride;
  const bool red_x = in_diff != nullptr && t < d.T;
  a.xpart = red_x ? p.dx_part : nullptr;
  a.in_diff = red_x ? in_diff + (size_t)t * d.S * id_stride : nullptr;     // rows of frame t+1
  a.id_stride = id_stride;
  const bool vec = p.pk_dm != nullptr && aligned16(p.dr_part) && aligned16(p.dr) && aligned16(out_diff) &&
                   od_stride % 4 == 0 && aligned16(p.dgifo) && aligned16(p.dc) && aligned16(p.gifo) &&
                   aligned16(p.cc) && aligned16(p.hh) && aligned16(p.pi) && aligned16(p.pf) && aligned16(p.po);
  if (vec) {
    DmVArgs va; va.g = a; va.wpk = p.pk_dm;
    if (p.fat && d.S > 16) {
      // (MTW, KSW) = (2, 4): two 16-row tiles x 4 K splits per workgroup; fine = (1, 8): one 16-row tile x 8 K splits
      const bool fine = fat_fine(d.S);
      va.gx = cdiv(d.C, fine ? 16 : 32);
      const dim3 fgrid(cdiv(va.gx, 8) * 8, cdiv(d.S, FST));
      const bool big = cdiv(d.R, KCH) > 16;
      if (p.bf16 && big) FAT_DISPATCH(k_dm_f, fine, 1, 8, 2, 4, 32, fgrid, st, pr, va, COMMA true);
      if (p.bf16) FAT_DISPATCH(k_dm_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA true);
      if (big) FAT_DISPATCH(k_dm_f, fine, 1, 8, 2, 4, 32, fgrid, st, pr, va, COMMA false);
      FAT_DISPATCH(k_dm_f, fine, 1, 8, 2, 4, 16, fgrid, st, pr, va, COMMA false);
    }
    const VecCfg cfg = pick_vec(d.S, cdiv(d.R, KCH));
    if (p.bf16) VEC_DISPATCH(k_dm_v, cfg, vec_grid(cdiv(d.C, 16), d.S, cfg), st, pr, va, COMMA true);
    VEC_DISPATCH(k_dm_v, cfg, vec_grid(cdiv(d.C, 16), d.S, cfg), st, pr, va, COMMA false);
  }
  const int nt = pick_nt(d.S);
  const dim3 grid(cdiv(d.C, 16), cdiv(d.S, 16 * nt));
  GEN_DISPATCH(k_dm_step, nt, grid, st, pr, a, );
}

hipError_t launch_dmf_step(const Dims &d, const BwdPtrs &p, int t, const float *P, hipStream_t st, LaunchProbe pr) {
  DmfArgs a;
  a.C = d.C; a.S = d.S; a.T = d.T; a.t = t;
  a.pi = p.pi; a.pf = p.pf; a.po = p.po; a.gifo = p.gifo; a.cc = p.cc; a.hh = p.hh;
  a.dgifo = p.dgifo; a.dc = p.dc; a.P = P; a.wpk = p.pk_fold;
  a.nch_total = cdiv(4 * d.C, KCH4);
  a.nch = t == d.T ? 0 : a.nch_total;
  const dim3 blk(NW * 64);
  const int need = cdiv(a.nch_total, NW);
  if (d.S > 4) {                               // two stream groups per workgroup share the weight fetch
    const dim3 grid(cdiv(d.C, 4), cdiv(d.S, 8));
    if (need <= 1) return launch((k_dmf_v<1, 2>), grid, blk, 0, st, pr, a);
    if (need == 2) return launch((k_dmf_v<2, 2>), grid, blk, 0, st, pr, a);
    return launch((k_dmf_v<4, 2>), grid, blk, 0, st, pr, a);
  }
  const dim3 grid(cdiv(d.C, 4), cdiv(d.S, 4));
  if (need <= 1) return launch((k_dmf_v<1, 1>), grid, blk, 0, st, pr, a);
  if (need == 2) return launch((k_dmf_v<2, 1>), grid, blk, 0, st, pr, a);
  return launch((k_dmf_v<4, 1>), grid, blk, 0, st, pr, a);
}


}  // namespace klstm
