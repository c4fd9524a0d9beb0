// kaldi-lstm_amd/csrc/klstm_score.hip -- the two stateless kernels of batched scoring (include/klstm_scorer.hpp):
//   k_pack_streams          concatenated utterances -> one time-major chunk (row = t*S + s), the TimeShift / targets delay applied
//                           per utterance (standard/nnet/nnet-time-shift.h:42-51 on each utterance; the trainer's batcher,
//                           bd-nnet-train-lstm-streams.cc:198-201), plus the chunk's reset flags
//   k_log_softmax_scatter   the Affine output rows of a chunk -> posterior / log-posterior / log-likelihood, each row written to
//                           its row of the per-utterance output (padding rows: dst -1, never written)
//   k_reverse_streams       per-stream, length-aware time reversal of a time-major block (the bidirectional layer,
//                           include/klstm_blstm.hpp): the backward direction's input, output, out_diff and in_diff
#include "../../include/klstm.h"
#include "klstm_kernels.h"

namespace klstm {

// One workgroup per output row (blockIdx.y = t*S + s), lane-contiguous columns like k_time_shift.  desc[3s .. 3s+2] = {row offset of
// the utterance in feats, its length, the frame the chunk starts at}; length <= 0: idle stream (zero rows).  Frame t of the chunk
// reads feats[off + clamp(start + t + shift, 0, len - 1)]: rows past the end repeat the last row (the trainer's padding, finite).
__global__ void k_pack_streams(const float *__restrict__ feats, int dim, int feat_stride, const int *__restrict__ desc, int S, int shift,
                               float *__restrict__ out, int out_stride, int *__restrict__ reset, int vec) {
  const int row = blockIdx.y, s = row % S, t = row / S;
  const int off = desc[3 * s], len = desc[3 * s + 1], start = desc[3 * s + 2];
  float *op = out + (size_t)row * out_stride;
  if (reset && t == 0 && blockIdx.x == 0 && threadIdx.x == 0) reset[s] = (len <= 0 || start == 0) ? 1 : 0;
  if (len <= 0) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < dim; c += gridDim.x * blockDim.x) op[c] = 0.f;
    return;
  }
  int src = start + t + shift;
  src = src < 0 ? 0 : src;
  src = src > len - 1 ? len - 1 : src;
  const float *ip = feats + (size_t)(off + src) * feat_stride;
  if (vec) {
    for (int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4; c < dim; c += gridDim.x * blockDim.x * 4)
      *reinterpret_cast<float4 *>(op + c) = *reinterpret_cast<const float4 *>(ip + c);
  } else {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < dim; c += gridDim.x * blockDim.x) op[c] = ip[c];
  }
}

// One workgroup per row (blockIdx.x = t*S + s), lane-contiguous columns (blockIdx.y tiles them).  The stream's length is clamped to
// [0, T] here, so no lens value can make a row read outside the block.  Modes (klstm.h klstm_reverse_streams):
//   0  t <  len: out[t] = in[len-1-t]   t >= len: out[t] = 0
//   1  t <  len: out[t] += in[len-1-t]  t >= len: untouched
//   2  t <  len: untouched              t >= len: out[t] = 0        (in unused)
//   3  t <  len: out[t] = in[t]         t >= len: out[t] = 0        (masked copy, no reversal)
__global__ void k_reverse_streams(const float *__restrict__ in, int in_stride, int S, int T, int cols, const int *__restrict__ lens,
                                  float *__restrict__ out, int out_stride, int mode, int vec) {
  const int row = blockIdx.x, s = row % S, t = row / S;
  int len = lens[s];
  len = len < 0 ? 0 : len > T ? T : len;
  const bool valid = t < len;
  if ((mode == 1 && !valid) || (mode == 2 && valid)) return;
  float *op = out + (size_t)row * out_stride;
  const int c0 = blockIdx.y * blockDim.x + threadIdx.x, step = gridDim.y * blockDim.x;
  if (!valid) {
    if (vec) {
      for (int c = c0 * 4; c < cols; c += step * 4) *reinterpret_cast<float4 *>(op + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int c = c0; c < cols; c += step) op[c] = 0.f;
    }
    return;
  }
  const int src = mode == 3 ? row : (len - 1 - t) * S + s;
  const float *ip = in + (size_t)src * in_stride;
  if (vec) {
    for (int c = c0 * 4; c < cols; c += step * 4) {
      float4 v = *reinterpret_cast<const float4 *>(ip + c);
      if (mode == 1) {
        const float4 o = *reinterpret_cast<const float4 *>(op + c);
        v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
      }
      *reinterpret_cast<float4 *>(op + c) = v;
    }
  } else {
    for (int c = c0; c < cols; c += step) op[c] = mode == 1 ? op[c] + ip[c] : ip[c];
  }
}

__device__ __forceinline__ float score_reduce(float v, float *sm, bool is_max) {   // (k_softmax_rows' block_reduce)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o); v = is_max ? fmaxf(v, w) : v + w; }
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = is_max ? fmaxf(r, sm[w]) : r + sm[w];
  return r;
}
// the value of one column from e = exp(a - max) (posterior) or a - max (the log forms); lse = log(sum)
__device__ __forceinline__ float score_value(int mode, float e, float am, float inv, float lse, const float *lp, float ps, int c) {
  if (mode == KLSTM_SCORE_POSTERIOR) return e * inv;
  const float v = am - lse;
  return mode == KLSTM_SCORE_LOGLIKE ? v - ps * lp[c] : v;
}

// Wide rows (the 16624-way output layer): k_softmax_rows_v's form -- 1024 threads per row, the whole row in registers, one pass
// over memory.  The posterior is its arithmetic exactly; the log forms take (a - max) - log(sum) from the same sum.
__global__ __launch_bounds__(1024) void k_log_softmax_scatter_v(const float *__restrict__ in, int cols, int in_stride,
                                                                const int *__restrict__ dst_row, float *__restrict__ out, int out_stride,
                                                                int mode, const float *__restrict__ log_prior, float prior_scale) {
  __shared__ float sm[16];
  const int dst = dst_row[blockIdx.x];
  if (dst < 0) return;                               // padding row (whole workgroup: no barrier is skipped by part of it)
  const float4 *ip = reinterpret_cast<const float4 *>(in + (size_t)blockIdx.x * in_stride);
  float4 *op = reinterpret_cast<float4 *>(out + (size_t)dst * out_stride);
  const int n4 = cols >> 2;
  float4 v[8];
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = threadIdx.x + 1024 * u;
    const float4 t = ip[c < n4 ? c : 0];
    v[u] = c < n4 ? t : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
  }
  float mx = -3.4e38f;
#pragma unroll
  for (int u = 0; u < 8; u++) mx = fmaxf(mx, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
  mx = score_reduce(mx, sm, true);
  float4 d[8];                                       // a - max (the log forms' operand)
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const bool on = threadIdx.x + 1024 * u < n4;
    d[u] = make_float4(v[u].x - mx, v[u].y - mx, v[u].z - mx, v[u].w - mx);
    v[u].x = on ? expf(d[u].x) : 0.f; v[u].y = on ? expf(d[u].y) : 0.f;
    v[u].z = on ? expf(d[u].z) : 0.f; v[u].w = on ? expf(d[u].w) : 0.f;
    sum += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  sum = score_reduce(sum, sm, false);
  const float inv = 1.f / sum, lse = logf(sum);
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = threadIdx.x + 1024 * u;
    if (c < n4)
      op[c] = make_float4(score_value(mode, v[u].x, d[u].x, inv, lse, log_prior, prior_scale, 4 * c),
                          score_value(mode, v[u].y, d[u].y, inv, lse, log_prior, prior_scale, 4 * c + 1),
                          score_value(mode, v[u].z, d[u].z, inv, lse, log_prior, prior_scale, 4 * c + 2),
                          score_value(mode, v[u].w, d[u].w, inv, lse, log_prior, prior_scale, 4 * c + 3));
  }
}
// Any shape: k_softmax_rows' three sweeps over the row (256 threads).
__global__ __launch_bounds__(256) void k_log_softmax_scatter(const float *__restrict__ in, int cols, int in_stride,
                                                             const int *__restrict__ dst_row, float *__restrict__ out, int out_stride,
                                                             int mode, const float *__restrict__ log_prior, float prior_scale) {
  __shared__ float sm[4];
  const int dst = dst_row[blockIdx.x];
  if (dst < 0) return;
  const float *ip = in + (size_t)blockIdx.x * in_stride;
  float *op = out + (size_t)dst * out_stride;
  float mx = -3.4e38f;
  for (int c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, ip[c]);
  mx = score_reduce(mx, sm, true);
  float sum = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) sum += expf(ip[c] - mx);
  sum = score_reduce(sum, sm, false);
  const float inv = 1.f / sum, lse = logf(sum);
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float am = ip[c] - mx;
    op[c] = score_value(mode, mode == KLSTM_SCORE_POSTERIOR ? expf(am) : 0.f, am, inv, lse, log_prior, prior_scale, c);
  }
}

static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t launch_pack_streams(const float *feats, int dim, int feat_stride, const int *desc, int S, int T, int shift, float *out,
                               int out_stride, int *reset, hipStream_t st) {
  const int vec = dim % 4 == 0 && feat_stride % 4 == 0 && out_stride % 4 == 0 && al16(feats) && al16(out);
  const int per = vec ? dim / 4 : dim;
  const int bx = per <= 64 ? 64 : per <= 128 ? 128 : 256;
  const int gx = (per + bx - 1) / bx;
  return launch(k_pack_streams, dim3(gx, T * S), dim3(bx), 0, st, LaunchProbe{}, feats, dim, feat_stride, desc, S, shift, out, out_stride, reset,
                vec);
}
hipError_t launch_reverse_streams(const float *in, int in_stride, int S, int T, int cols, const int *lens, float *out, int out_stride,
                                  int mode, hipStream_t st) {
  const bool in_ok = mode == 2 || (in_stride % 4 == 0 && al16(in));
  const int vec = cols % 4 == 0 && out_stride % 4 == 0 && al16(out) && in_ok;
  const int per = vec ? cols / 4 : cols;
  const int bx = per <= 64 ? 64 : per <= 128 ? 128 : 256;
  const int gy = (per + bx - 1) / bx;
  return launch(k_reverse_streams, dim3(T * S, gy), dim3(bx), 0, st, LaunchProbe{}, in, in_stride, S, T, cols, lens, out, out_stride,
                mode, vec);
}
hipError_t launch_log_softmax_scatter(const float *in, int rows, int cols, int in_stride, const int *dst_row, float *out, int out_stride,
                                      int mode, const float *log_prior, float prior_scale, hipStream_t st) {
  const bool wide = cols % 4 == 0 && cols <= 32768 && cols >= 2048 && in_stride % 4 == 0 && out_stride % 4 == 0 && al16(in) && al16(out);
  return launch(wide ? k_log_softmax_scatter_v : k_log_softmax_scatter, dim3(rows), dim3(wide ? 1024 : 256), 0, st, LaunchProbe{}, in, cols,
                in_stride, dst_row, out, out_stride, mode, log_prior, prior_scale);
}

}  // namespace klstm
