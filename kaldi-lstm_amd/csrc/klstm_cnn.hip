// kaldi-lstm_amd/csrc/klstm_cnn.hip -- nnet1's convolutional and max-pooling components and the activations between them: the kcnn_*
// entries of include/klstm_cnn.h (which defines every quantity; the numpy yardsticks: tests/cnn_ref.py) and their kernels.
// The three products of the convolution run on the f32-input matrix instruction (MFMA16: 16 x 16 x 4, exact f32 products, f32
// accumulation); none of them ever has an im2col matrix in memory: the P overlapping patches of a row are formed from the row's copy in
// LDS through a table koff[k] = s * st + d of the K patch positions (k = s * pd + d).
//   k_conv_fwd   GEMM [(r,p)] x [f] over k.  A workgroup (8 waves) keeps a tile of FT filters (all F when they fit) transposed in LDS for
//                the whole launch and walks row blocks of RB rows grid-stride: the rows go global -> LDS once, a wave takes 16 (r,p) x 16 f.
//   k_conv_bwd   G[(r,p), k] = sum_f out_diff[(r,p), f] filters[f, k] per patch, then overlap-add over p into the row block's in_diff
//                accumulator in LDS.  A wave owns WHOLE rows (RW of them), so no two waves ever add to one element; inside a wave the 16
//                (r,p) of a result tile are added one after the other (16 lanes, distinct k, distinct targets).  No atomics; the
//                finished rows are written once.  out_diff comes straight from global (each lane's quad of f is contiguous), four k tiles
//                per pass so that it is fetched once per 64 k.  The filters are in LDS: all of them for the launch when they fit, else
//                tile by tile over f for every row block.
//   k_conv_grad  [f] x [k] over (r,p), a fixed split: chunk c = rows [c KCNN_GRAD_SPLIT_ROWS, ...), whatever the strides.  A workgroup
//                (4 waves) owns 32 f x 256 k of one chunk (a wave: 2 x 4 tiles, 32 accumulator registers), stages the chunk's input rows
//                16 at a time in LDS (MFMA chains of CNN_CHAIN terms, each added to the chunk's sums: short chains round less) and writes its PARTIAL to the
//                workspace; the bias partials, sums of the A operands of wave 0 of k block 0, are kept in double as (high, low) floats.
//   k_conv_stage2<UPDATE>  one thread per parameter sums the chunks' partials in order of c, in double, and rounds once; UPDATE: corr =
//                momentum corr + grad, param -= lr corr.  A launch of its own behind k_conv_grad on the same stream: every partial
//                exists before a parameter moves.
//   k_pool_fwd<V> / k_pool_bwd<V> / k_act<KIND, DIFF, V>  row kernels, one lane per quad of four columns (V = 4), 16 bytes per access
//                when every pointer and stride is 16-byte aligned (and w % 4 == 0 for the pools), else per element (V = 1): the same bits.
// KNOWN SLOW SPOTS (first version; what they cost is in DESIGN.md 4w): k_conv_fwd issues three LDS reads (koff, X, Bt) per MFMA and one 16 x 16 tile per wave
// at a time; k_conv_bwd serialises 16 LDS read-add-writes per 16 x 16 tile in its overlap-add (reducing over p in registers, or a
// per-wave LDS tile whose columns each lane adds up, would not); k_conv_grad leaves the waves whose 64 k start at or beyond K idle
// (two of four at K = 88) and reads the input once per (32-f block, 256-k block) workgroup, out_diff once per k block.
// BOUNDS.  Every global access is guarded by r < rows and by the column's own limit (c < D_in, f < F, k < K); masked lanes read nothing
// and contribute +0.  LDS indices: X[rl * D_in + c] with rl < RB, c = p ps + koff[k] <= (P-1) ps + (n-1) st + pd - 1 = D_in - 1.
// Row offsets are size_t products.
#include <cstdint>
#include <initializer_list>

#include "../../include/klstm_cnn.h"
#include "klstm_host.h"
#include "klstm_kernels.h"
#include "klstm_math.h"

namespace klstm {

constexpr unsigned CNN_MAX_WG = 2048;            // the cap of a memory-bound grid-stride pass
constexpr size_t CNN_LDS_BUDGET = 156 * 1024;    // of the CU's 160 KB
constexpr int CNN_GB = 16;                       // rows the gradient kernel stages at a time
constexpr int CNN_CHAIN = 32;                    // reduction terms one MFMA accumulator chain takes (8 instructions) before it is added to the total

struct ConvShape { int Din, Dout, pd, ps, st, n, P, K, F; };

static bool conv_shape(int Din, int Dout, int pd, int ps, int st, ConvShape *s) {
  if (Din < 1 || Dout < 1 || pd < 1 || ps < 1 || st < 1) return false;
  if (Din % st != 0 || pd > st || (st - pd) % ps != 0) return false;
  const int P = 1 + (st - pd) / ps;
  if (Dout % P != 0) return false;
  const long long K = (long long)(Din / st) * pd;
  if (K > 0x7fffffff) return false;
  *s = ConvShape{Din, Dout, pd, ps, st, Din / st, P, (int)K, Dout / P};
  return true;
}

__device__ __forceinline__ int conv_koff(const ConvShape &s, int k) { return (k / s.pd) * s.st + k % s.pd; }

// ---------------------------------------------------------------- forward
struct ConvFwdArgs {
  const float *in, *filt, *bias; float *out;
  int in_stride, out_stride, rows;
  ConvShape s;
  int FT, FTp, RB, K4;      // filters per tile (multiple of 16), its LDS row stride, rows per block, K rounded up to 4
};

__global__ __launch_bounds__(512) void k_conv_fwd(ConvFwdArgs a) {
  extern __shared__ float lds[];
  const ConvShape &s = a.s;
  float *Bt = lds;                                   // [K4][FTp]: Bt[k][j] = filters[f0 + j][k], zero beyond
  float *bl = Bt + (size_t)a.K4 * a.FTp;             // [FT]
  int *koff = reinterpret_cast<int *>(bl + a.FT);    // [K4]
  float *X = reinterpret_cast<float *>(koff + a.K4); // [RB][Din]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6, i16 = lane & 15, kg = lane >> 4;
  const int f0 = blockIdx.y * a.FT, nf = min(a.FT, s.F - f0);
  for (int e = tid; e < a.FT * a.K4; e += blockDim.x) {
    const int j = e / a.K4, k = e - j * a.K4;
    Bt[(size_t)k * a.FTp + j] = (j < nf && k < s.K) ? a.filt[(size_t)(f0 + j) * s.K + k] : 0.f;
  }
  for (int e = tid; e < a.FT; e += blockDim.x) bl[e] = e < nf ? a.bias[f0 + e] : 0.f;
  for (int k = tid; k < a.K4; k += blockDim.x) koff[k] = k < s.K ? conv_koff(s, k) : 0;
  const int nrb = (a.rows + a.RB - 1) / a.RB, ntl = (nf + 15) / 16;
  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    __syncthreads();                                 // the last block's X is done with (first pass: nothing)
    const int r0 = rb * a.RB, nr = min(a.RB, a.rows - r0);
    for (int e = tid; e < a.RB * s.Din; e += blockDim.x) {
      const int rl = e / s.Din, c = e - rl * s.Din;
      X[e] = rl < nr ? a.in[(size_t)(r0 + rl) * a.in_stride + c] : 0.f;
    }
    __syncthreads();
    const int M = nr * s.P, mt = (M + 15) / 16;
    for (int t = wave; t < mt * ntl; t += nwave) {
      const int tm = t / ntl, tn = t - tm * ntl;
      const int m = tm * 16 + i16, mm = m < M ? m : 0, r = mm / s.P, p = mm - r * s.P;
      const float *xa = X + r * s.Din + p * s.ps;
      const float *bp = Bt + tn * 16 + i16;
      // the sum over k in pieces of CNN_CHAIN k, each from zero, added up in order: one long MFMA chain rounds worse than that (K = 480
      // missed the bar of tests/test_cnn_gpu.py in one chain)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < a.K4; k0 += CNN_CHAIN) {
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
        const int kend = min(k0 + CNN_CHAIN, a.K4);
        for (int k = k0 + kg; k < kend; k += 4) {
          const float av = k < s.K ? xa[koff[k]] : 0.f;
          part = MFMA16(av, bp[(size_t)k * a.FTp], part);
        }
        acc += part;
      }
      const int f = tn * 16 + i16;
      const float e4[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int mo = tm * 16 + 4 * kg + j;
        if (mo < M && f < nf) {
          const int ro = mo / s.P, po = mo - ro * s.P;
          a.out[(size_t)(r0 + ro) * a.out_stride + (size_t)po * s.F + f0 + f] = bl[f] + e4[j];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- backward (in_diff)
struct ConvBwdArgs {
  const float *od, *filt; float *id;
  int od_stride, id_stride, rows;
  ConvShape s;
  int FT, nft, Kp, K16, RW, RB;   // f per filter tile (multiple of 4), tiles, LDS row stride of a filter row, K rounded up to 16, rows per wave, per block
};

__device__ __forceinline__ void conv_bwd_load_filters(const ConvBwdArgs &a, float *Wl, int ft0) {
  const ConvShape &s = a.s;                          // Wl[j][k] = filters[ft0 + j][k], zero beyond F and K
  for (int e = threadIdx.x; e < a.FT * a.K16; e += blockDim.x) {
    const int j = e / a.K16, k = e - j * a.K16;
    Wl[(size_t)j * a.Kp + k] = (ft0 + j < s.F && k < s.K) ? a.filt[(size_t)(ft0 + j) * s.K + k] : 0.f;
  }
}

__global__ __launch_bounds__(512) void k_conv_bwd(ConvBwdArgs a) {
  extern __shared__ float lds[];
  const ConvShape &s = a.s;
  float *Wl = lds;                                         // [FT][Kp]
  int *koff = reinterpret_cast<int *>(Wl + (size_t)a.FT * a.Kp);   // [K16]
  float *acc_l = reinterpret_cast<float *>(koff + a.K16);  // [RB][Din]: the block's in_diff
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  for (int k = tid; k < a.K16; k += blockDim.x) koff[k] = k < s.K ? conv_koff(s, k) : 0;
  if (a.nft == 1) conv_bwd_load_filters(a, Wl, 0);
  const int nrb = (a.rows + a.RB - 1) / a.RB;
  for (int rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    __syncthreads();                                       // the last block's accumulator was written out
    const int r0 = rb * a.RB, nr = min(a.RB, a.rows - r0);
    for (int e = tid; e < a.RB * s.Din; e += blockDim.x) acc_l[e] = 0.f;
    const int rw0 = wave * a.RW, nrw = max(0, min(a.RW, nr - rw0));   // this wave's rows: rw0 .. rw0 + nrw
    const int M = nrw * s.P, mt = (M + 15) / 16;
    for (int ft = 0; ft < a.nft; ft++) {
      const int ft0 = ft * a.FT;
      if (a.nft > 1) { __syncthreads(); conv_bwd_load_filters(a, Wl, ft0); }
      __syncthreads();                                     // filters, koff and the zeroed accumulator are there
      const int fend = min(a.FT, s.F - ft0);               // the reduction runs over f = ft0 .. ft0 + fend (rounded up to 4: zeros)
      for (int tm = 0; tm < mt; tm++) {
        const int m = tm * 16 + i16;
        const bool mv = m < M;
        const int mm = mv ? m : 0, rl = rw0 + mm / s.P, p = mm % s.P;
        const float *odp = a.od + (size_t)(r0 + rl) * a.od_stride + (size_t)p * s.F + ft0;
        for (int k0 = 0; k0 < a.K16; k0 += 64) {
          f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
          for (int fq = 0; fq < fend; fq += 4) {           // wave-uniform trips; f < FT (a multiple of 4), rows beyond F are zeros
            const int f = fq + kg;
            const float av = (mv && f < fend) ? odp[f] : 0.f;
            const float *wp = Wl + (size_t)f * a.Kp + k0 + i16;
#pragma unroll
            for (int u = 0; u < 4; u++)
              if (k0 + u * 16 < a.K16) acc[u] = MFMA16(av, wp[u * 16], acc[u]);
          }
          // overlap-add: element j of lane (i16, kg) is G[(r,p) = tile row 4 kg + j][k = k0 + 16 u + i16]
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int k = k0 + u * 16 + i16;
            if (k0 + u * 16 >= a.K16) continue;
            const float e4[4] = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
            const int ko = koff[k < a.K16 ? k : 0];
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
              for (int j = 0; j < 4; j++) {
                const int mo = tm * 16 + 4 * g + j;        // wave-uniform
                if (mo < M) {
                  if (kg == g && k < s.K) {
                    const int ro = rw0 + mo / s.P, po = mo % s.P;
                    acc_l[ro * s.Din + po * s.ps + ko] += e4[j];
                  }
                  // ORDER.  The next row's adds may hit the words this row's just wrote (another lane's p ps + d).  Three things keep
                  // them behind: the lanes of a wave issue an LDS instruction together and LDS serves one wave's instructions
                  // in order; the fence orders this lane's LDS accesses at wavefront scope for the compiler and the memory
                  // model; the barrier keeps the scheduler from moving code across.
                  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                  __builtin_amdgcn_wave_barrier();
                }
              }
          }
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < nr * s.Din; e += blockDim.x) {
      const int rl = e / s.Din, c = e - rl * s.Din;
      a.id[(size_t)(r0 + rl) * a.id_stride + c] = acc_l[e];
    }
  }
}

// ---------------------------------------------------------------- gradient: partials, then the fixed-order second stage
struct ConvGradArgs {
  const float *in, *od; float *ws;
  int in_stride, od_stride, rows;
  ConvShape s;
};

__global__ __launch_bounds__(256) void k_conv_grad(ConvGradArgs a) {
  extern __shared__ float lds[];
  const ConvShape &s = a.s;
  float *X = lds;                                          // [CNN_GB][Din]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const int chunk = blockIdx.x, fb = blockIdx.y * 32, kb = blockIdx.z * 256 + wave * 64;
  const bool bias_wave = blockIdx.z == 0 && wave == 0, active = kb < s.K || bias_wave;
  const int c0 = chunk * KCNN_GRAD_SPLIT_ROWS, cn = min((int)KCNN_GRAD_SPLIT_ROWS, a.rows - c0);
  int ko[4]; bool kv[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const int k = kb + u * 16 + i16; kv[u] = k < s.K; ko[u] = kv[u] ? conv_koff(s, k) : 0; }
  const bool fv[2] = {fb + i16 < s.F, fb + 16 + i16 < s.F};
  f32x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int u = 0; u < 4; u++) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  double bsum[2] = {0.0, 0.0};                             // the bias sums in double: a sum of signed terms may cancel
  for (int b0 = 0; b0 < cn; b0 += CNN_GB) {
    __syncthreads();
    const int r0 = c0 + b0, nr = min(CNN_GB, cn - b0);
    for (int e = tid; e < nr * s.Din; e += blockDim.x) {
      const int rl = e / s.Din, c = e - rl * s.Din;
      X[e] = a.in[(size_t)(r0 + rl) * a.in_stride + c];
    }
    __syncthreads();
    if (!active) continue;
    f32x4 sub[2][4];                                       // this stage's own sums, added to the chunk's afterwards: short chains round less
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int u = 0; u < 4; u++) sub[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int M = nr * s.P;
    int r = 0, p = kg;                                     // this lane's (r,p) of the step: virtual row m0 + kg
    while (p >= s.P) { p -= s.P; r++; }
    for (int m0 = 0; m0 < M; m0 += 4) {
      const bool mv = m0 + kg < M;
      const float *odp = a.od + (size_t)(r0 + (mv ? r : 0)) * a.od_stride + (size_t)(mv ? p : 0) * s.F + fb + i16;
      const float a0 = (mv && fv[0]) ? odp[0] : 0.f, a1 = (mv && fv[1]) ? odp[16] : 0.f;
      const float *xp = X + (mv ? r * s.Din + p * s.ps : 0);
      if (bias_wave) { bsum[0] += (double)a0; bsum[1] += (double)a1; }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const float bv = (mv && kv[u]) ? xp[ko[u]] : 0.f;
        sub[0][u] = MFMA16(a0, bv, sub[0][u]);
        sub[1][u] = MFMA16(a1, bv, sub[1][u]);
      }
      p += 4;
      while (p >= s.P) { p -= s.P; r++; }
      if ((m0 + 4) % CNN_CHAIN == 0) {                     // (wave-uniform) a chain of CNN_CHAIN terms is full: to the chunk's sums
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
          for (int u = 0; u < 4; u++) { acc[t][u] += sub[t][u]; sub[t][u] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int u = 0; u < 4; u++) acc[t][u] += sub[t][u];
  }
  const size_t nelem = (size_t)s.F * s.K + 2 * (size_t)s.F;     // the bias partials are doubles, kept as (high, low) floats
  float *w = a.ws + (size_t)chunk * nelem;
  if (kb < s.K) {
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const float e4[4] = {acc[t][u].x, acc[t][u].y, acc[t][u].z, acc[t][u].w};
        const int k = kb + u * 16 + i16;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int f = fb + t * 16 + 4 * kg + j;
          if (f < s.F && k < s.K) w[(size_t)f * s.K + k] = e4[j];
        }
      }
  }
  if (bias_wave) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const double v0 = __shfl(bsum[t], i16), v1 = __shfl(bsum[t], i16 + 16), v2 = __shfl(bsum[t], i16 + 32), v3 = __shfl(bsum[t], i16 + 48);
      const double d = ((v0 + v1) + v2) + v3;
      const float hi = (float)d;
      const int f = fb + t * 16 + i16;
      if (kg == 0 && f < s.F) { w[(size_t)s.F * s.K + 2 * f] = hi; w[(size_t)s.F * s.K + 2 * f + 1] = (float)(d - (double)hi); }
    }
  }
}

#pragma clang fp contract(off)
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_conv_stage2(const float *__restrict__ ws, int nchunk, size_t nfk, size_t nelem, float *p0, float *p1,
                                                    float *c0, float *c1, float lr0, float lr1, float mmt) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, nout = nfk + (nelem - nfk) / 2;     // one thread per parameter
  if (e >= nout) return;
  const bool first = e < nfk;
  const size_t i = first ? e : e - nfk;
  double gd = 0.0;                                         // in order of c, in double: one rounding at the end
  if (first) for (int c = 0; c < nchunk; c++) gd += (double)ws[(size_t)c * nelem + e];
  else for (int c = 0; c < nchunk; c++) gd += (double)ws[(size_t)c * nelem + nfk + 2 * i] + (double)ws[(size_t)c * nelem + nfk + 2 * i + 1];
  const float g = (float)gd;
  if (!UPDATE) {
    (first ? p0 : p1)[i] = g;
  } else {
    float *corr = first ? c0 : c1, *par = first ? p0 : p1;
    const float cv = mmt * corr[i] + g;
    corr[i] = cv;
    par[i] = par[i] - (first ? lr0 : lr1) * cv;
  }
}

// ---------------------------------------------------------------- pooling and activations: one lane per quad of four columns
struct PoolArgs {
  const float *in, *out, *od; float *dst;                 // forward: in -> dst; backward: in, out, od -> dst
  int in_stride, out_stride, od_stride, dst_stride, rows;
  int Pin, Q, z, g, w;
  int vec;
};

template <int V>
__global__ __launch_bounds__(256) void k_pool_fwd(PoolArgs a) {
  const size_t nq = (size_t)(a.w + V - 1) / V, per = (size_t)a.Q * nq, items = (size_t)a.rows * per;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const size_t r = i / per, rem = i - r * per;
    const int q = (int)(rem / nq), f = (int)(rem - (size_t)q * nq) * V;
    const float *ip = a.in + r * (size_t)a.in_stride + (size_t)(q * a.g) * a.w + f;
    float *op = a.dst + r * (size_t)a.dst_stride + (size_t)q * a.w + f;
    if (V == 4) {
      float4 m = *reinterpret_cast<const float4 *>(ip);
      for (int j = 1; j < a.z; j++) {
        const float4 v = *reinterpret_cast<const float4 *>(ip + (size_t)j * a.w);
        if (v.x > m.x) m.x = v.x;
        if (v.y > m.y) m.y = v.y;
        if (v.z > m.z) m.z = v.z;
        if (v.w > m.w) m.w = v.w;
      }
      *reinterpret_cast<float4 *>(op) = m;
    } else {
      float m = ip[0];
      for (int j = 1; j < a.z; j++) { const float v = ip[(size_t)j * a.w]; if (v > m) m = v; }
      op[0] = m;
    }
  }
}

template <int V>
__global__ __launch_bounds__(256) void k_pool_bwd(PoolArgs a) {
  const size_t nq = (size_t)(a.w + V - 1) / V, per = (size_t)a.Pin * nq, items = (size_t)a.rows * per;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const size_t r = i / per, rem = i - r * per;
    const int p = (int)(rem / nq), f = (int)(rem - (size_t)p * nq) * V;
    // the pools that contain p: q g <= p <= q g + z - 1, q < Q
    const int qlo = p - a.z + 1 > 0 ? (p - a.z + 1 + a.g - 1) / a.g : 0, qhi = min(a.Q - 1, p / a.g), cnt = qhi - qlo + 1;
    const float *ip = a.in + r * (size_t)a.in_stride + (size_t)p * a.w + f;
    const float *yp = a.out + r * (size_t)a.out_stride + f, *dp = a.od + r * (size_t)a.od_stride + f;
    float *op = a.dst + r * (size_t)a.dst_stride + (size_t)p * a.w + f;
    const float scale = cnt > 0 ? 1.0f / (float)cnt : 0.f;
    if (V == 4) {
      const float4 v = *reinterpret_cast<const float4 *>(ip);
      float4 sum = {0.f, 0.f, 0.f, 0.f};
      for (int q = qlo; q <= qhi; q++) {
        const float4 y = *reinterpret_cast<const float4 *>(yp + (size_t)q * a.w), d = *reinterpret_cast<const float4 *>(dp + (size_t)q * a.w);
        sum.x += v.x == y.x ? d.x : 0.f;
        sum.y += v.y == y.y ? d.y : 0.f;
        sum.z += v.z == y.z ? d.z : 0.f;
        sum.w += v.w == y.w ? d.w : 0.f;
      }
      float4 o = {0.f, 0.f, 0.f, 0.f};
      if (cnt > 0) { o.x = sum.x * scale; o.y = sum.y * scale; o.z = sum.z * scale; o.w = sum.w * scale; }
      *reinterpret_cast<float4 *>(op) = o;
    } else {
      const float v = ip[0];
      float sum = 0.f;
      for (int q = qlo; q <= qhi; q++) sum += v == yp[(size_t)q * a.w] ? dp[(size_t)q * a.w] : 0.f;
      op[0] = cnt > 0 ? sum * scale : 0.f;
    }
  }
}

struct ActArgs {
  const float *a, *b; float *dst;                          // forward: a = in; diff: a = the output y, b = out_diff
  int a_stride, b_stride, dst_stride, rows, cols;
};

template <int KIND> __device__ __forceinline__ float act_fwd(float x) { return KIND == KCNN_SIGMOID ? k_sigmoid(x) : k_tanh(x); }
template <int KIND> __device__ __forceinline__ float act_diff(float d, float y) { return KIND == KCNN_SIGMOID ? k_diff_sigmoid(d, y) : k_diff_tanh(d, y); }

template <int KIND, bool DIFF, int V>
__global__ __launch_bounds__(256) void k_act(ActArgs a) {
  const size_t nq = (size_t)(a.cols + V - 1) / V, items = (size_t)a.rows * nq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const size_t r = i / nq;
    const int c = (int)(i - r * nq) * V;
    const float *ap = a.a + r * (size_t)a.a_stride + c;
    float *op = a.dst + r * (size_t)a.dst_stride + c;
    if (V == 4 && c + 4 <= a.cols) {
      const float4 x = *reinterpret_cast<const float4 *>(ap);
      float4 o;
      if (DIFF) {
        const float4 d = *reinterpret_cast<const float4 *>(a.b + r * (size_t)a.b_stride + c);
        o.x = act_diff<KIND>(d.x, x.x); o.y = act_diff<KIND>(d.y, x.y); o.z = act_diff<KIND>(d.z, x.z); o.w = act_diff<KIND>(d.w, x.w);
      } else {
        o.x = act_fwd<KIND>(x.x); o.y = act_fwd<KIND>(x.y); o.z = act_fwd<KIND>(x.z); o.w = act_fwd<KIND>(x.w);
      }
      *reinterpret_cast<float4 *>(op) = o;
    } else {
      const int n = min(V, a.cols - c);
      for (int j = 0; j < n; j++) op[j] = DIFF ? act_diff<KIND>(a.b[r * (size_t)a.b_stride + c + j], ap[j]) : act_fwd<KIND>(ap[j]);
    }
  }
}

// ---------------------------------------------------------------- host side
static unsigned rowpass_grid(size_t items) {
  const size_t target = (size_t)CNN_MAX_WG * 256;
  return (unsigned)(((items < target ? items : target) + 255) / 256);
}
static bool all16(std::initializer_list<const void *> ps, std::initializer_list<int> strides) {
  for (const void *p : ps) if ((uintptr_t)p % 16 != 0) return false;
  for (int s : strides) if (s % 4 != 0) return false;
  return true;
}
static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// the forward tiling: all F in one tile when they fit beside 16 rows, else halves of it; nothing fits: false
static bool conv_fwd_plan(const ConvShape &s, ConvFwdArgs *a, size_t *shm) {
  a->K4 = round_up(s.K, 4);
  for (int RB = 16; RB >= 1; RB /= 4)
    for (int FT = round_up(s.F, 16);; FT = round_up(FT / 2, 16)) {
      const int FTp = FT % 32 == 0 ? FT + 16 : FT;         // rows k and k + 1 of Bt land in different halves of the banks
      const size_t need = ((size_t)a->K4 * FTp + FT + a->K4 + (size_t)RB * s.Din) * 4;
      if (need <= CNN_LDS_BUDGET) { a->FT = FT; a->FTp = FTp; a->RB = RB; *shm = need; return true; }
      if (FT == 16) break;
    }
  return false;
}
static bool conv_bwd_plan(const ConvShape &s, ConvBwdArgs *a, size_t *shm) {
  a->K16 = round_up(s.K, 16);
  a->Kp = a->K16 % 32 == 0 ? a->K16 + 16 : a->K16;
  const int RW0 = (32 + s.P - 1) / s.P;
  for (int RW = RW0 < 1 ? 1 : RW0 > 4 ? 4 : RW0; RW >= 1; RW--)
    for (int FT = round_up(s.F, 4);; FT = round_up(FT / 2, 4)) {
      const size_t need = ((size_t)FT * a->Kp + a->K16 + (size_t)8 * RW * s.Din) * 4;
      if (need <= CNN_LDS_BUDGET) { a->FT = FT; a->nft = (s.F + FT - 1) / FT; a->RW = RW; a->RB = 8 * RW; *shm = need; return true; }
      if (FT == 4) break;
    }
  return false;
}

static klstm_status conv_grad_common(const char *who, const float *in, int in_stride, const float *od, int od_stride, int rows, int Din,
                                     int Dout, int pd, int ps, int st, float *p0, float *p1, float *c0, float *c1, bool update, float lr0,
                                     float lr1, float mmt, float *ws, size_t ws_floats, void *hip_stream) {
  ConvShape s;
  if (!conv_shape(Din, Dout, pd, ps, st, &s))
    return fail(KLSTM_ERR_ARG, "%s: inconsistent numbers (in %d, out %d, patch dim %d, step %d, stride %d)", who, Din, Dout, pd, ps, st);
  if (rows < 0) return fail(KLSTM_ERR_ARG, "%s: rows %d", who, rows);
  if (rows == 0) return KLSTM_OK;
  if (!in || !od || !p0 || !p1 || (update && (!c0 || !c1))) return fail(KLSTM_ERR_ARG, "%s: null argument", who);
  if (in_stride < Din || od_stride < Dout) return fail(KLSTM_ERR_ARG, "%s: row stride below the width (%d < %d or %d < %d)", who, in_stride, Din, od_stride, Dout);
  const size_t need = kcnn_conv_workspace_floats(rows, Din, Dout, pd, ps, st);
  if (!ws || ws_floats < need) return fail(KLSTM_ERR_ARG, "%s: workspace of %zu floats, %zu needed", who, ws ? ws_floats : (size_t)0, need);
  if ((size_t)CNN_GB * Din * 4 > CNN_LDS_BUDGET) return fail(KLSTM_ERR_ARG, "%s: an input row of %d floats does not fit the kernel's LDS", who, Din);
  const int nchunk = (rows + KCNN_GRAD_SPLIT_ROWS - 1) / KCNN_GRAD_SPLIT_ROWS;
  hipStream_t stq = (hipStream_t)hip_stream;
  ConvGradArgs a{in, od, ws, in_stride, od_stride, rows, s};
  HIPCHK(launch(k_conv_grad, dim3(nchunk, (s.F + 31) / 32, (s.K + 255) / 256), dim3(256), (size_t)CNN_GB * Din * 4, stq, LaunchProbe(), a));
  const size_t nfk = (size_t)s.F * s.K, nelem = nfk + 2 * (size_t)s.F;
  const dim3 g2((unsigned)((nfk + s.F + 255) / 256));
  if (update) HIPCHK(launch(k_conv_stage2<true>, g2, dim3(256), 0, stq, LaunchProbe(), (const float *)ws, nchunk, nfk, nelem, p0, p1, c0, c1, lr0, lr1, mmt));
  else HIPCHK(launch(k_conv_stage2<false>, g2, dim3(256), 0, stq, LaunchProbe(), (const float *)ws, nchunk, nfk, nelem, p0, p1, c0, c1, lr0, lr1, mmt));
  return KLSTM_OK;
}

struct PoolShape { int Pin, Q; };
static bool pool_shape(int Din, int Dout, int z, int g, int w, PoolShape *s) {
  if (Din < 1 || Dout < 1 || z < 1 || g < 1 || w < 1 || Din % w != 0) return false;
  const int Pin = Din / w;
  if (z > Pin) return false;
  const int Q = 1 + (Pin - z) / g;                         // rounded down: the last patches may lie in no pool
  if ((long long)Q * w != Dout) return false;
  *s = PoolShape{Pin, Q};
  return true;
}

template <int KIND, bool DIFF>
static hipError_t launch_act(const ActArgs &a, bool vec, hipStream_t st) {
  if (vec) return launch(k_act<KIND, DIFF, 4>, dim3(rowpass_grid((size_t)a.rows * ((a.cols + 3) / 4))), dim3(256), 0, st, LaunchProbe(), a);
  return launch(k_act<KIND, DIFF, 1>, dim3(rowpass_grid((size_t)a.rows * a.cols)), dim3(256), 0, st, LaunchProbe(), a);
}

}  // namespace klstm

using namespace klstm;

extern "C" {

klstm_status kcnn_conv_plan(int in_dim, int out_dim, int patch_dim, int patch_step, int patch_stride, int *n, int *P, int *K, int *F) {
  if (!n || !P || !K || !F) return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: null argument");
  ConvShape s;
  if (in_dim < 1 || out_dim < 1 || patch_dim < 1 || patch_step < 1 || patch_stride < 1)
    return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: a number below 1 (in %d, out %d, patch dim %d, step %d, stride %d)", in_dim, out_dim, patch_dim, patch_step, patch_stride);
  if (in_dim % patch_stride != 0) return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: patch stride %d does not divide the input dim %d", patch_stride, in_dim);
  if (patch_dim > patch_stride) return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: patch dim %d above the patch stride %d", patch_dim, patch_stride);
  if ((patch_stride - patch_dim) % patch_step != 0)
    return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: patch step %d does not divide stride - dim = %d", patch_step, patch_stride - patch_dim);
  if (!conv_shape(in_dim, out_dim, patch_dim, patch_step, patch_stride, &s))
    return fail(KLSTM_ERR_ARG, "kcnn_conv_plan: %d patches do not divide the output dim %d", 1 + (patch_stride - patch_dim) / patch_step, out_dim);
  *n = s.n; *P = s.P; *K = s.K; *F = s.F;
  return KLSTM_OK;
}

size_t kcnn_conv_workspace_floats(int rows, int in_dim, int out_dim, int patch_dim, int patch_step, int patch_stride) {
  ConvShape s;
  if (rows <= 0 || !conv_shape(in_dim, out_dim, patch_dim, patch_step, patch_stride, &s)) return 0;
  return (size_t)((rows + KCNN_GRAD_SPLIT_ROWS - 1) / KCNN_GRAD_SPLIT_ROWS) * ((size_t)s.F * s.K + 2 * (size_t)s.F);
}

klstm_status kcnn_conv_propagate(const float *in, int in_stride, int rows, int in_dim, int out_dim, int patch_dim, int patch_step,
                                 int patch_stride, const float *filters, const float *bias, float *out, int out_stride, void *hip_stream) {
  ConvFwdArgs a;
  if (!conv_shape(in_dim, out_dim, patch_dim, patch_step, patch_stride, &a.s))
    return fail(KLSTM_ERR_ARG, "kcnn_conv_propagate: inconsistent numbers (in %d, out %d, patch dim %d, step %d, stride %d)", in_dim, out_dim, patch_dim, patch_step, patch_stride);
  if (rows < 0) return fail(KLSTM_ERR_ARG, "kcnn_conv_propagate: rows %d", rows);
  if (rows == 0) return KLSTM_OK;
  if (!in || !filters || !bias || !out) return fail(KLSTM_ERR_ARG, "kcnn_conv_propagate: null argument");
  if (in_stride < in_dim || out_stride < out_dim)
    return fail(KLSTM_ERR_ARG, "kcnn_conv_propagate: row stride below the width (%d < %d or %d < %d)", in_stride, in_dim, out_stride, out_dim);
  size_t shm = 0;
  if (!conv_fwd_plan(a.s, &a, &shm)) return fail(KLSTM_ERR_ARG, "kcnn_conv_propagate: K = %d, D_in = %d do not fit the kernel's LDS tiling", a.s.K, in_dim);
  a.in = in; a.filt = filters; a.bias = bias; a.out = out; a.in_stride = in_stride; a.out_stride = out_stride; a.rows = rows;
  const int nrb = (rows + a.RB - 1) / a.RB;
  HIPCHK(launch(k_conv_fwd, dim3(nrb < 512 ? nrb : 512, (a.s.F + a.FT - 1) / a.FT), dim3(512), shm, (hipStream_t)hip_stream, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status kcnn_conv_backpropagate(const float *out_diff, int od_stride, int rows, int in_dim, int out_dim, int patch_dim, int patch_step,
                                     int patch_stride, const float *filters, float *in_diff, int id_stride, void *hip_stream) {
  ConvBwdArgs a;
  if (!conv_shape(in_dim, out_dim, patch_dim, patch_step, patch_stride, &a.s))
    return fail(KLSTM_ERR_ARG, "kcnn_conv_backpropagate: inconsistent numbers (in %d, out %d, patch dim %d, step %d, stride %d)", in_dim, out_dim, patch_dim, patch_step, patch_stride);
  if (rows < 0) return fail(KLSTM_ERR_ARG, "kcnn_conv_backpropagate: rows %d", rows);
  if (rows == 0 || !in_diff) return KLSTM_OK;
  if (!out_diff || !filters) return fail(KLSTM_ERR_ARG, "kcnn_conv_backpropagate: null argument");
  if (od_stride < out_dim || id_stride < in_dim)
    return fail(KLSTM_ERR_ARG, "kcnn_conv_backpropagate: row stride below the width (%d < %d or %d < %d)", od_stride, out_dim, id_stride, in_dim);
  size_t shm = 0;
  if (!conv_bwd_plan(a.s, &a, &shm)) return fail(KLSTM_ERR_ARG, "kcnn_conv_backpropagate: K = %d, D_in = %d do not fit the kernel's LDS tiling", a.s.K, in_dim);
  a.od = out_diff; a.filt = filters; a.id = in_diff; a.od_stride = od_stride; a.id_stride = id_stride; a.rows = rows;
  const int nrb = (rows + a.RB - 1) / a.RB;
  HIPCHK(launch(k_conv_bwd, dim3(nrb < 512 ? nrb : 512), dim3(512), shm, (hipStream_t)hip_stream, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status kcnn_conv_gradient(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim, int out_dim,
                                int patch_dim, int patch_step, int patch_stride, float *filters_grad, float *bias_grad, float *ws,
                                size_t ws_floats, void *hip_stream) {
  return conv_grad_common("kcnn_conv_gradient", in, in_stride, out_diff, od_stride, rows, in_dim, out_dim, patch_dim, patch_step, patch_stride,
                          filters_grad, bias_grad, nullptr, nullptr, false, 0.f, 0.f, 0.f, ws, ws_floats, hip_stream);
}

klstm_status kcnn_conv_update(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim, int out_dim,
                              int patch_dim, int patch_step, int patch_stride, float *filters, float *bias, float *filters_corr,
                              float *bias_corr, float lr, float lr_bias, float momentum, float *ws, size_t ws_floats, void *hip_stream) {
  return conv_grad_common("kcnn_conv_update", in, in_stride, out_diff, od_stride, rows, in_dim, out_dim, patch_dim, patch_step, patch_stride,
                          filters, bias, filters_corr, bias_corr, true, lr, lr_bias, momentum, ws, ws_floats, hip_stream);
}

klstm_status kcnn_pool_propagate(const float *in, int in_stride, int rows, int in_dim, int out_dim, int pool_size, int pool_step,
                                 int pool_stride, float *out, int out_stride, void *hip_stream) {
  PoolShape s;
  if (!pool_shape(in_dim, out_dim, pool_size, pool_step, pool_stride, &s))
    return fail(KLSTM_ERR_ARG, "kcnn_pool_propagate: inconsistent numbers (in %d, out %d, pool size %d, step %d, stride %d)", in_dim, out_dim, pool_size, pool_step, pool_stride);
  if (rows < 0) return fail(KLSTM_ERR_ARG, "kcnn_pool_propagate: rows %d", rows);
  if (rows == 0) return KLSTM_OK;
  if (!in || !out) return fail(KLSTM_ERR_ARG, "kcnn_pool_propagate: null argument");
  if (in_stride < in_dim || out_stride < out_dim)
    return fail(KLSTM_ERR_ARG, "kcnn_pool_propagate: row stride below the width (%d < %d or %d < %d)", in_stride, in_dim, out_stride, out_dim);
  PoolArgs a{in, nullptr, nullptr, out, in_stride, 0, 0, out_stride, rows, s.Pin, s.Q, pool_size, pool_step, pool_stride, 0};
  a.vec = pool_stride % 4 == 0 && all16({in, out}, {in_stride, out_stride});
  hipStream_t st = (hipStream_t)hip_stream;
  if (a.vec) HIPCHK(launch(k_pool_fwd<4>, dim3(rowpass_grid((size_t)rows * s.Q * (pool_stride / 4))), dim3(256), 0, st, LaunchProbe(), a));
  else HIPCHK(launch(k_pool_fwd<1>, dim3(rowpass_grid((size_t)rows * out_dim)), dim3(256), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status kcnn_pool_backpropagate(const float *in, int in_stride, const float *out, int out_stride, const float *out_diff, int od_stride,
                                     int rows, int in_dim, int out_dim, int pool_size, int pool_step, int pool_stride, float *in_diff,
                                     int id_stride, void *hip_stream) {
  PoolShape s;
  if (!pool_shape(in_dim, out_dim, pool_size, pool_step, pool_stride, &s))
    return fail(KLSTM_ERR_ARG, "kcnn_pool_backpropagate: inconsistent numbers (in %d, out %d, pool size %d, step %d, stride %d)", in_dim, out_dim, pool_size, pool_step, pool_stride);
  if (rows < 0) return fail(KLSTM_ERR_ARG, "kcnn_pool_backpropagate: rows %d", rows);
  if (rows == 0 || !in_diff) return KLSTM_OK;
  if (!in || !out || !out_diff) return fail(KLSTM_ERR_ARG, "kcnn_pool_backpropagate: null argument");
  if (in_stride < in_dim || id_stride < in_dim || out_stride < out_dim || od_stride < out_dim)
    return fail(KLSTM_ERR_ARG, "kcnn_pool_backpropagate: row stride below the width (%d, %d < %d or %d, %d < %d)", in_stride, id_stride, in_dim, out_stride, od_stride, out_dim);
  PoolArgs a{in, out, out_diff, in_diff, in_stride, out_stride, od_stride, id_stride, rows, s.Pin, s.Q, pool_size, pool_step, pool_stride, 0};
  a.vec = pool_stride % 4 == 0 && all16({in, out, out_diff, in_diff}, {in_stride, out_stride, od_stride, id_stride});
  hipStream_t st = (hipStream_t)hip_stream;
  if (a.vec) HIPCHK(launch(k_pool_bwd<4>, dim3(rowpass_grid((size_t)rows * s.Pin * (pool_stride / 4))), dim3(256), 0, st, LaunchProbe(), a));
  else HIPCHK(launch(k_pool_bwd<1>, dim3(rowpass_grid((size_t)rows * in_dim)), dim3(256), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

klstm_status kcnn_activation(int kind, const float *in, int in_stride, int rows, int cols, float *out, int out_stride, void *hip_stream) {
  if (kind != KCNN_SIGMOID && kind != KCNN_TANH) return fail(KLSTM_ERR_ARG, "kcnn_activation: unknown kind %d", kind);
  if (rows < 0 || cols < 0) return fail(KLSTM_ERR_ARG, "kcnn_activation: bad size (rows %d, cols %d)", rows, cols);
  if (rows == 0 || cols == 0) return KLSTM_OK;
  if (!in || !out) return fail(KLSTM_ERR_ARG, "kcnn_activation: null argument");
  if (in_stride < cols || out_stride < cols) return fail(KLSTM_ERR_ARG, "kcnn_activation: row stride below the column count (%d / %d < %d)", in_stride, out_stride, cols);
  if (in == out && in_stride != out_stride) return fail(KLSTM_ERR_ARG, "kcnn_activation: in == out with two strides (%d, %d)", in_stride, out_stride);
  const ActArgs a{in, nullptr, out, in_stride, 0, out_stride, rows, cols};
  const bool vec = all16({in, out}, {in_stride, out_stride});
  hipStream_t st = (hipStream_t)hip_stream;
  if (kind == KCNN_SIGMOID) HIPCHK((launch_act<KCNN_SIGMOID, false>(a, vec, st)));
  else HIPCHK((launch_act<KCNN_TANH, false>(a, vec, st)));
  return KLSTM_OK;
}

klstm_status kcnn_activation_diff(int kind, const float *out, int out_stride, const float *out_diff, int od_stride, int rows, int cols,
                                  float *in_diff, int id_stride, void *hip_stream) {
  if (kind != KCNN_SIGMOID && kind != KCNN_TANH) return fail(KLSTM_ERR_ARG, "kcnn_activation_diff: unknown kind %d", kind);
  if (rows < 0 || cols < 0) return fail(KLSTM_ERR_ARG, "kcnn_activation_diff: bad size (rows %d, cols %d)", rows, cols);
  if (rows == 0 || cols == 0 || !in_diff) return KLSTM_OK;
  if (!out || !out_diff) return fail(KLSTM_ERR_ARG, "kcnn_activation_diff: null argument");
  if (out_stride < cols || od_stride < cols || id_stride < cols)
    return fail(KLSTM_ERR_ARG, "kcnn_activation_diff: row stride below the column count (%d / %d / %d < %d)", out_stride, od_stride, id_stride, cols);
  if (in_diff == out_diff && id_stride != od_stride) return fail(KLSTM_ERR_ARG, "kcnn_activation_diff: in_diff == out_diff with two strides (%d, %d)", id_stride, od_stride);
  const ActArgs a{out, out_diff, in_diff, out_stride, od_stride, id_stride, rows, cols};
  const bool vec = all16({out, out_diff, in_diff}, {out_stride, od_stride, id_stride});
  hipStream_t st = (hipStream_t)hip_stream;
  if (kind == KCNN_SIGMOID) HIPCHK((launch_act<KCNN_SIGMOID, true>(a, vec, st)));
  else HIPCHK((launch_act<KCNN_TANH, true>(a, vec, st)));
  return KLSTM_OK;
}

}  // extern "C"
