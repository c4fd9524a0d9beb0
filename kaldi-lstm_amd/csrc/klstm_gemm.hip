// kaldi-lstm_amd/csrc/klstm_gemm.hip -- weight packing and the 64 x 64 fp32 tile GEMM kernels (tile body: klstm_gemm_dev.h)
// with their split-K forms; then their launchers.
//
// What each kernel replaces in the reference (google/nnet/bd-nnet-lstm-projected-streams.h):
//   k_gemm       : batched x-projection (:246 + :259) when it is not fused into the step kernel
#include "klstm_gemm_dev.h"

namespace klstm {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------
// k_pack: (re)build the four packed weight copies from the natural blob + its transposes.
// One thread per packed float4 (destination-contiguous, so the writes are coalesced 1 KB/wave).
//   array 0 gates: rows (cell-major: tile row i -> gate i&3, cell 4*tile + i>>2), k over [R | pad | I | pad]
//   array 1 proj : rows n of W_r_m   [R x C],   k over C
//   array 2 dr   : rows n of [W_gifo_r^T ; W_gifo_x^T]  ([R x 4C] tiles then [I x 4C] tiles), k over 4C
//   array 3 dm   : rows c of W_r_m^T [C x R],   k over R
// ---------------------------------------------------------------------------------------------
struct PackArgs {
  int C, R, I;
  const float *wx, *wr, *wm, *wrT, *wmT, *wxT;
  float4 *pk[4];
  long n4[4];          // 16-byte vector count of each array (0: array not selected in this launch)
  int nch[4];          // chunks per tile
  int bf16;            // 1: entries are 8 bf16 (RNE of the fp32 master) covering k..k+7 -> half as many vectors
  float4 *foldx;       // fp32 only: the W_x chunks of array 0 are also the W_x chunks of the folded gates array
  int nch_fold, nchm_fold;
};

__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
  const int C = a.C, R = a.R, I = a.I;
  const long total = a.n4[0] + a.n4[1] + a.n4[2] + a.n4[3];
  for (long gid = blockIdx.x * 256L + threadIdx.x; gid < total; gid += (long)gridDim.x * 256) {
    int arr = 0; long id = gid;
    while (id >= a.n4[arr]) { id -= a.n4[arr]; arr++; }
    const int lane = (int)(id & 63), h = a.bf16 ? 0 : (int)((id >> 6) & 1);
    const long tc = a.bf16 ? id >> 6 : id >> 7;
    const int nch = a.nch[arr];
    const int tile = (int)(tc / nch), ch = (int)(tc - (long)tile * nch);
    const int i = lane & 15;
    const int k = ch * KCH + (lane >> 4) * 8 + h * 4;
    const float *src = nullptr;
    int klim = 0, koff = k;
    bool row_ok = false;
    if (arr == 0) {
      const int cell = tile * 4 + (i >> 2), gate = i & 3;
      row_ok = cell < C;
      const int nchR = (R + KCH - 1) / KCH;
      if (ch < nchR) { src = a.wr + ((size_t)gate * C + (row_ok ? cell : 0)) * R; klim = R; }
      else { src = a.wx + ((size_t)gate * C + (row_ok ? cell : 0)) * I; klim = I; koff = k - nchR * KCH; }
    } else if (arr == 1) {
      const int n = tile * 16 + i; row_ok = n < R; src = a.wm + (size_t)(row_ok ? n : 0) * C; klim = C;
    } else if (arr == 2) {
      const int ntR = (R + 15) / 16;
      if (tile < ntR) { const int n = tile * 16 + i; row_ok = n < R; src = a.wrT + (size_t)(row_ok ? n : 0) * 4 * C; }
      else { const int n = (tile - ntR) * 16 + i; row_ok = n < I; src = a.wxT + (size_t)(row_ok ? n : 0) * 4 * C; }
      klim = 4 * C;
    } else {
      const int c = tile * 16 + i; row_ok = c < C; src = a.wmT + (size_t)(row_ok ? c : 0) * R; klim = R;
    }
    float4 v = f4zero();
    if (row_ok && koff + 4 <= klim) v = ldg4(src + koff);     // all extents are multiples of 8 on this path
    if (a.bf16) {
      float4 w = f4zero();
      if (row_ok && koff + 8 <= klim) w = ldg4(src + koff + 4);
      const uint2 lo = pack_bf16x4(v), hi = pack_bf16x4(w);
      v = __builtin_bit_cast(float4, make_uint4(lo.x, lo.y, hi.x, hi.y));
    }
    a.pk[arr][id] = v;
    if (arr == 0 && a.foldx && !a.bf16) {
      const int nchR = (R + KCH - 1) / KCH;
      if (ch >= nchR) a.foldx[(((size_t)tile * a.nch_fold + a.nchm_fold + (ch - nchR)) * 2 + h) * 64 + lane] = v;
    }
  }
}

// 1-D grid padded to a multiple of 8.  XCD-aware order: workgroup w lands on XCD w % 8 (observed dispatch rule, speed
// only); XCD x gets the contiguous m-major tile range [x*cpx, (x+1)*cpx), so its private L2 keeps a few A row panels and
// the B column panels instead of every XCD streaming every panel from the fabric.
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_gemm(GemmJob g) {
  __shared__ __attribute__((aligned(16))) float As[GLDS];
  __shared__ __attribute__((aligned(16))) float Bs[GLDS];
  const int ntn = (g.N + GT - 1) / GT, nbt = ((g.M + GT - 1) / GT) * ntn;
  const int cpx = (nbt + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * cpx + (int)(blockIdx.x >> 3);
  if (b >= nbt) return;
  if (g.guard && (g.guard[2] | g.guard[6])) return;          // (grid-uniform, before any barrier)
  gemm_tile<TA, TB>(g, (b / ntn) * GT, (b % ntn) * GT, As, Bs);
}

// Split-K variant for short-and-wide products whose 64x64 output tiles cannot fill the chip (AffineTransform
// in_diff: 80 x 512 over K = 16624 is 16 tiles): blockIdx.z owns K slice z and writes its partial tile to
// ws[z][M][N]; k_splitk_reduce sums the slices in fixed order (deterministic, no atomics).
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_gemm_splitk(GemmJob g, int klen, float *ws) {
  __shared__ __attribute__((aligned(16))) float As[GLDS];
  __shared__ __attribute__((aligned(16))) float Bs[GLDS];
  const int k0 = blockIdx.z * klen;
  GemmJob s = g;
  s.K = min(g.K - k0, klen);
  s.A = TA ? g.A + (size_t)k0 * g.lda : g.A + k0;
  s.B = TB ? g.B + k0 : g.B + (size_t)k0 * g.ldb;
  s.vecA = g.vecA && (TA || s.K % 8 == 0);
  s.vecB = g.vecB && (!TB || s.K % 8 == 0);
  s.beta = 0.f; s.bias = nullptr;
  s.Cm = ws + (size_t)blockIdx.z * g.M * g.N; s.ldc = g.N;
  gemm_tile<TA, TB>(s, blockIdx.y * GT, blockIdx.x * GT, As, Bs);
}
__global__ __launch_bounds__(256) void k_splitk_reduce(ReduceArgs a) {
  if (a.guard && (a.guard[2] | a.guard[6])) return;
  const long total = (long)a.M * a.N;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = (int)(i / a.N), n = (int)(i - (long)m * a.N);
    float v = 0.f;
    for (int z0 = 0; z0 < a.ks; z0 += 8) {           // 8 independent loads in flight, summed in slice order
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = a.ws[(size_t)min(z0 + j, a.ks - 1) * total + i];
#pragma unroll
      for (int j = 0; j < 8; j++) v += (z0 + j < a.ks) ? t[j] : 0.f;
    }
    if (a.bias) v += a.bias[n];
    if (a.add) v = a.add[(size_t)m * a.add_ld + n] + v;
    float *cp = a.Cm + (size_t)m * a.ldc + n;
    if (a.beta != 0.f) v = a.beta * *cp + v;
    *cp = v;
    if (a.C2) a.C2[(size_t)m * a.ldc2 + n] = v;
    if (a.C3 && m >= a.tail0) a.C3[(size_t)(m - a.tail0) * a.N + n] = v;
  }
}

// Two NN split-K products that share K and the slice length in ONE launch pair (the folded BPTT tail: d_r and in_diff
// both contract dgifo rows over 4C): tiles [0, nb1) belong to job 1, the rest to job 2.
__global__ __launch_bounds__(256) void k_gemm_splitk2(GemmJob g1, GemmJob g2, int nb1, int klen, float *ws1, float *ws2) {
  __shared__ __attribute__((aligned(16))) float As[GLDS];
  __shared__ __attribute__((aligned(16))) float Bs[GLDS];
  const bool second = (int)blockIdx.x >= nb1;
  const GemmJob &g = second ? g2 : g1;
  const int lb = second ? (int)blockIdx.x - nb1 : (int)blockIdx.x;
  const int ntn = (g.N + GT - 1) / GT;
  const int k0 = blockIdx.z * klen;
  GemmJob s = g;
  s.K = min(g.K - k0, klen);
  s.A = g.A + k0;
  s.B = g.B + (size_t)k0 * g.ldb;
  s.vecA = g.vecA && s.K % 8 == 0;
  s.beta = 0.f; s.bias = nullptr;
  s.Cm = (second ? ws2 : ws1) + (size_t)blockIdx.z * g.M * g.N; s.ldc = g.N;
  gemm_tile<false, false>(s, (lb / ntn) * GT, (lb % ntn) * GT, As, Bs);
}
__global__ __launch_bounds__(256) void k_splitk_reduce2(ReduceArgs r1, ReduceArgs r2, int nbr1) {
  const bool second = (int)blockIdx.x >= nbr1;
  const ReduceArgs &a = second ? r2 : r1;
  const int nb = second ? (int)gridDim.x - nbr1 : nbr1;
  const int bid = second ? (int)blockIdx.x - nbr1 : (int)blockIdx.x;
  const long total = (long)a.M * a.N;
  for (long i = bid * 256L + threadIdx.x; i < total; i += (long)nb * 256) {
    const int m = (int)(i / a.N), n = (int)(i - (long)m * a.N);
    float v = 0.f;
    for (int z0 = 0; z0 < a.ks; z0 += 8) {
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = a.ws[(size_t)min(z0 + j, a.ks - 1) * total + i];
#pragma unroll
      for (int j = 0; j < 8; j++) v += (z0 + j < a.ks) ? t[j] : 0.f;
    }
    if (a.add) v = a.add[(size_t)m * a.add_ld + n] + v;
    a.Cm[(size_t)m * a.ldc + n] = v;
  }
}

// x chunks of the folded gates array (the W_rm chunks are written by the fold product itself)
__global__ __launch_bounds__(256) void k_pack_foldx(const float *__restrict__ wx, float4 *__restrict__ pk, int C, int I, int nch1) {
  const int nchM = (C + KCH - 1) / KCH, nchX = nch1 - nchM;
  const long total = (long)((C + 3) / 4) * nchX * 128;
  for (long id = blockIdx.x * 256L + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
    const int lane = (int)(id & 63), h = (int)((id >> 6) & 1);
    const long tc = id >> 7;
    const int tile = (int)(tc / nchX), chx = (int)(tc - (long)tile * nchX);
    const int i = lane & 15, cell = tile * 4 + (i >> 2), gate = i & 3;
    const int k = chx * KCH + (lane >> 4) * 8 + h * 4;
    float4 v = f4zero();
    if (cell < C && k + 4 <= I) v = ldg4(wx + ((size_t)gate * C + cell) * I + k);
    pk[(((size_t)tile * nch1 + nchM + chx) * 2 + h) * 64 + lane] = v;
  }
}

// W_rm = W_gifo_r [4C x R] * W_r_m [R x C] once per Update, written directly as the two packed operands of the folded
// step kernels (NT form on the transposed copy W_r_m^T [C x R]: both operands k-contiguous); then the x chunks.
// pk_fold[0/1] must have been zero-filled once (padding rows / k tails are never written).
hipError_t launch_fold(const Dims &d, const float *param_blob, const float *wmT, float *pk_fold[2], bool pack_x,
                       hipStream_t st, LaunchProbe pr, LaunchProbe pr2, void *scratch3, LaunchProbe pr3, bool planes_fresh, int mode3) {
  const long o_wr = (long)4 * d.C * d.I;
  GemmJob g = make_job(false, true, 4 * d.C, d.C, d.R, param_blob + o_wr, d.R, wmT, d.R, 0.f, nullptr, d.C, nullptr);
  g.gperm = d.C;
  g.pk1 = reinterpret_cast<float4 *>(pk_fold[0]); g.nch1 = cdiv(d.C, KCH) + cdiv(d.I, KCH);
  g.pk2 = reinterpret_cast<float4 *>(pk_fold[1]); g.nch2 = cdiv(4 * d.C, KCH4);
  const dim3 grid = gemm_grid(4 * d.C, d.C), block(256);
  auto first = [&]() -> hipError_t {
    if (scratch3 && fold_bf16x3_supported(d, mode3))
      return launch_fold_bf16x3(d, mode3, param_blob + o_wr, wmT, scratch3, pk_fold, g.nch1, g.nch2, st, pr3, pr, planes_fresh);   // klstm_fold3.hip
    if (fold_direct_supported(d)) return launch_fold_direct(d, param_blob + o_wr, wmT, pk_fold, g.nch1, g.nch2, st, pr);   // klstm_fold.hip
    return launch((k_gemm<false, true>), grid, block, 0, st, pr, g);
  };
  hipError_t err = first();
  if (err != hipSuccess || !pack_x) return err;
  const long nx = (long)cdiv(d.C, 4) * cdiv(d.I, KCH) * 128;
  return launch(k_pack_foldx, dim3((unsigned)cdiv((int)nx, 256)), block, 0, st, pr2, param_blob, g.pk1, d.C, d.I, g.nch1);
}

// r(1..T) = m(1..T) W_r_m^T (:312) for all frames at once -> rr rows, out rows (:328), last block -> prev_r (:331)
hipError_t launch_rbatch(const Dims &d, const FwdPtrs &p, float *out, int out_stride, float *ws, hipStream_t st,
                         LaunchProbe pr, LaunchProbe pr2, const unsigned *guard) {
  const int M = d.T * d.S;
  int kl = 0;
  const int ks = gemm_splitk_plan(M, d.R, d.C, &kl);
  if (ks > 1 && ws)
    return launch_gemm_splitk(false, true, M, d.R, d.C, p.mm + (size_t)d.S * d.C, d.C, p.wm, d.C, 0.f, p.rr + (size_t)d.S * d.R,
                              d.R, nullptr, ws, ks, kl, st, nullptr, 0, pr, pr2, out, out_stride, p.next_r, M - d.S, guard);
  GemmJob g = make_job(false, true, M, d.R, d.C, p.mm + (size_t)d.S * d.C, d.C, p.wm, d.C, 0.f,
                       p.rr + (size_t)d.S * d.R, d.R, nullptr);
  g.C2 = out; g.ldc2 = out_stride;
  g.C3 = p.next_r; g.tail0 = M - d.S;
  g.guard = guard;
  return launch((k_gemm<false, true>), gemm_grid(M, d.R), dim3(256), 0, st, pr, g);
}

bool pack_supported(const Dims &d) { return d.R % 8 == 0 && d.I % 8 == 0 && d.C % 8 == 0; }
void pack_sizes_fold(const Dims &d, long n4[2]) {
  n4[0] = (long)cdiv(d.C, 16) * 4 * (cdiv(d.C, KCH) + cdiv(d.I, KCH)) * 128;
  n4[1] = (long)cdiv(d.C, 4) * cdiv(4 * d.C, KCH4) * 128;
}
void pack_sizes(const Dims &d, long n4[4]) {
  // gates tiles are 4 cells each; a fat workgroup walks 4 of them, so round up to 16 cells (zero rows)
  n4[0] = (long)cdiv(d.C, 16) * 4 * (cdiv(d.R, KCH) + cdiv(d.I, KCH)) * 128;
  n4[1] = (long)cdiv(d.R, 16) * cdiv(d.C, KCH) * 128;
  n4[2] = (long)(cdiv(d.R, 16) + cdiv(d.I, 16)) * cdiv(4 * d.C, KCH) * 128;
  n4[3] = (long)cdiv(d.C, 16) * cdiv(d.R, KCH) * 128;
}
hipError_t launch_pack(const Dims &d, const float *param_blob, const float *wrT, const float *wmT, const float *wxT,
                       float *pk[4], int mask, bool bf16, hipStream_t st, LaunchProbe pr, float *foldx) {
  PackArgs a;
  a.bf16 = bf16 ? 1 : 0;
  a.foldx = reinterpret_cast<float4 *>(foldx);
  a.nchm_fold = cdiv(d.C, KCH); a.nch_fold = a.nchm_fold + cdiv(d.I, KCH);
  a.C = d.C; a.R = d.R; a.I = d.I;
  const long o_wr = (long)4 * d.C * d.I, o_wm = o_wr + (long)4 * d.C * d.R + 7 * d.C;
  a.wx = param_blob; a.wr = param_blob + o_wr; a.wm = param_blob + o_wm;
  a.wrT = wrT; a.wmT = wmT; a.wxT = wxT;
  pack_sizes(d, a.n4);
  for (int i = 0; i < 4; i++) { if (!(mask & (1 << i))) a.n4[i] = 0; if (bf16) a.n4[i] /= 2; }
  a.nch[0] = cdiv(d.R, KCH) + cdiv(d.I, KCH); a.nch[1] = cdiv(d.C, KCH); a.nch[2] = cdiv(4 * d.C, KCH); a.nch[3] = cdiv(d.R, KCH);
  long total = 0;
  for (int i = 0; i < 4; i++) { a.pk[i] = reinterpret_cast<float4 *>(pk[i]); total += a.n4[i]; }
  if (total == 0) return hipSuccess;
  const long nb = (total + 255) / 256;
  return launch(k_pack, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, st, pr, a);
}

hipError_t launch_gemm(bool transA, bool transB, int M, int N, int K, const float *A, int lda,
                       const float *B, int ldb, float beta, float *Cm, int ldc, const float *bias,
                       hipStream_t st, LaunchProbe pr) {
  const GemmJob g = make_job(transA, transB, M, N, K, A, lda, B, ldb, beta, Cm, ldc, bias);
  const dim3 grid = gemm_grid(M, N), block(256);
  if (transA && transB) return launch((k_gemm<true, true>), grid, block, 0, st, pr, g);
  if (transA && !transB) return launch((k_gemm<true, false>), grid, block, 0, st, pr, g);
  if (!transA && transB) return launch((k_gemm<false, true>), grid, block, 0, st, pr, g);
  return launch((k_gemm<false, false>), grid, block, 0, st, pr, g);
}

// Cm = beta*Cm + A^T B (gradient of a weight matrix, K = frames), then P -= lr*Cm in the same pass (GemmJob::P):
// AffineTransform::Update with the momentum folded into the product like ...streams.h:468-487.  N, ldc multiples of 4,
// 16-byte aligned Cm / P.
hipError_t launch_gemm_tn_update(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float beta, float *Cm,
                                 float *P, int ldc, float lr, hipStream_t st, LaunchProbe pr) {
  GemmJob g = make_job(true, false, M, N, K, A, lda, B, ldb, beta, Cm, ldc, nullptr);
  g.P = P; g.lr = lr;
  return launch((k_gemm<true, false>), gemm_grid(M, N), dim3(256), 0, st, pr, g);
}

// Cm = beta*Cm + A^T B through the coalesced epilogue (N, ldc % 4 == 0, 16-byte aligned Cm)
hipError_t launch_gemm_tn_coal(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float beta, float *Cm,
                               int ldc, hipStream_t st, LaunchProbe pr) {
  GemmJob g = make_job(true, false, M, N, K, A, lda, B, ldb, beta, Cm, ldc, nullptr);
  g.coal = 1;
  return launch((k_gemm<true, false>), gemm_grid(M, N), dim3(256), 0, st, pr, g);
}

// Split-K plan: worth it when the output tiles cover less than half the chip and K is long.
int gemm_splitk_plan(int M, int N, int K, int *klen) {
  const int tiles = cdiv(M, GT) * cdiv(N, GT);
  if (tiles >= 128 || K <= GK) { *klen = K; return 1; }
  const int ks = cdiv(768, tiles);                   // ~3 workgroups per CU
  const int kl = cdiv(cdiv(K, ks), GK) * GK;         // whole K tiles; a slice is at least one
  *klen = kl;
  return cdiv(K, kl);
}
hipError_t launch_gemm_splitk(bool transA, bool transB, int M, int N, int K, const float *A, int lda, const float *B,
                              int ldb, float beta, float *Cm, int ldc, const float *bias, float *ws, int ks, int klen,
                              hipStream_t st, const float *add, int add_ld, LaunchProbe pr, LaunchProbe pr2, float *C2,
                              int ldc2, float *C3, int tail0, const unsigned *guard) {
  const GemmJob g = make_job(transA, transB, M, N, K, A, lda, B, ldb, 0.f, nullptr, N, nullptr);
  const dim3 grid(cdiv(N, GT), cdiv(M, GT), ks), block(256);
  auto first = [&]() -> hipError_t {
    if (transA && transB) return launch((k_gemm_splitk<true, true>), grid, block, 0, st, pr, g, klen, ws);
    if (transA) return launch((k_gemm_splitk<true, false>), grid, block, 0, st, pr, g, klen, ws);
    if (transB) return launch((k_gemm_splitk<false, true>), grid, block, 0, st, pr, g, klen, ws);
    return launch((k_gemm_splitk<false, false>), grid, block, 0, st, pr, g, klen, ws);
  };
  hipError_t err = first();
  if (err != hipSuccess) return err;
  ReduceArgs r;
  r.ws = ws; r.ks = ks; r.M = M; r.N = N; r.beta = beta; r.Cm = Cm; r.ldc = ldc; r.bias = bias; r.add = add; r.add_ld = add_ld;
  r.C2 = C2; r.ldc2 = ldc2; r.C3 = C3; r.tail0 = tail0; r.guard = guard;
  const long nb = ((long)M * N + 255) / 256;
  return launch(k_splitk_reduce, dim3((unsigned)(nb > 2048 ? 2048 : nb)), block, 0, st, pr2, r);
}

// Folded BPTT tail: d_r(1..T) = out_diff + dgifo(2..T+1) W_gifo_r (:391) and, if in_diff != nullptr,
// in_diff = dgifo(1..T) W_gifo_x (:457).  ws: bwd_tail_ws_floats(d) floats.
size_t bwd_tail_ws_floats(const Dims &d) {
  int kl = 0;
  const int ks = gemm_splitk_plan(d.T * d.S, d.R, 4 * d.C, &kl);
  return (size_t)ks * d.T * d.S * (d.R + d.I);
}
hipError_t launch_bwd_tail(const Dims &d, const float *dgifo, const float *wr, const float *wx, const float *out_diff,
                           int od_stride, float *dr, float *in_diff, int id_stride, float *ws, hipStream_t st, LaunchProbe pr,
                           LaunchProbe pr2) {
  const int M = d.T * d.S, K4 = 4 * d.C;
  int kl = 0;
  int ks = gemm_splitk_plan(M, d.R, K4, &kl);
  // few frames: both products on the f16 matrix cores at fp32 accuracy, all rows per wave (klstm_fold.hip k_skinny_nn16; 80 frames,
  // 800/512/512: 16.3 us for the tiled split-K launch -> see docs/DESIGN_rounds_1-4.md 10)
  const int G16 = aligned16(dgifo) && aligned16(wr) && aligned16(wx) ? skinny16_pair_groups(M, d.R, in_diff ? d.I : 0, K4, ks) : 0;
  const GemmJob g1 = make_job(false, false, M, d.R, K4, dgifo + (size_t)2 * d.S * K4, K4, wr, d.R, 0.f, nullptr, d.R, nullptr);
  const GemmJob g2 = make_job(false, false, M, d.I, K4, dgifo + (size_t)d.S * K4, K4, wx, d.I, 0.f, nullptr, d.I, nullptr);
  const int nb1 = cdiv(M, GT) * cdiv(d.R, GT), nb2 = in_diff ? cdiv(M, GT) * cdiv(d.I, GT) : 0;
  float *ws2 = ws + (size_t)ks * M * d.R;
  auto first = [&]() -> hipError_t {
    if (G16 > 0) {
      const int G = G16;
      ks = G;                                            // (ws2 above was placed for the larger tiled plan: still in range)
      return launch_skinny16_pair(M, K4, dgifo + (size_t)2 * d.S * K4, dgifo + (size_t)d.S * K4, K4, wr, d.R, wx, in_diff ? d.I : 0, ws, ws2, G, st, pr);
    }
    return launch(k_gemm_splitk2, dim3(nb1 + nb2, 1, ks), dim3(256), 0, st, pr, g1, g2, nb1, kl, ws, ws2);
  };
  hipError_t err = first();
  if (err != hipSuccess) return err;
  ReduceArgs r1, r2;
  r1.ws = ws; r1.ks = ks; r1.M = M; r1.N = d.R; r1.beta = 0.f; r1.Cm = dr + (size_t)d.S * d.R; r1.ldc = d.R;
  r1.add = out_diff; r1.add_ld = od_stride;
  r2 = r1;
  r2.ws = ws2; r2.N = d.I; r2.Cm = in_diff; r2.ldc = id_stride; r2.add = nullptr; r2.add_ld = 0;
  const int nbr1 = cdiv(M * d.R, 256), nbr2 = in_diff ? cdiv(M * d.I, 256) : 0;
  return launch(k_splitk_reduce2, dim3(nbr1 + nbr2), dim3(256), 0, st, pr2, r1, r2, nbr1);
}

}  // namespace klstm
