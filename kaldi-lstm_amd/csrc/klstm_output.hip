// kaldi-lstm_amd/csrc/klstm_output.hip -- the output tail of the gfx950 kernels: time shift, softmax / cross-entropy
// rows, column sums and the element-wise updates, then their launchers.  fp32 throughout (Kaldi BaseFloat).
// (The per-step recurrence kernels, the tile GEMMs, gradients and Update: klstm_kernels.hip.)
#include "klstm_kernels.h"
#include "klstm_math.h"

namespace klstm {

#pragma clang fp contract(off)

// TimeShift::PropagateFnc (standard/nnet/nnet-time-shift.h:42-51): out[dst] = in[clamp(dst + shift, 0, rows-1)]
// (shift == 0 is TransmitComponent's copy, nnet-transmit-component.h:26-33).  One row per blockIdx.y, lane-contiguous.
__global__ void k_time_shift(const float *__restrict__ in, int rows, int cols, int in_stride, float *__restrict__ out,
                             int out_stride, int shift, int vec) {
  const int dst = blockIdx.y;
  int src = dst + shift;
  src = src < 0 ? 0 : src;
  src = src > rows - 1 ? rows - 1 : src;
  const float *ip = in + (size_t)src * in_stride;
  float *op = out + (size_t)dst * out_stride;
  if (vec) {
    for (int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4; c < cols; c += gridDim.x * blockDim.x * 4)
      *reinterpret_cast<float4 *>(op + c) = *reinterpret_cast<const float4 *>(ip + c);
  } else {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x) op[c] = ip[c];
  }
}

// Xent::EvalMasked for GENERAL posteriors (google/nnet/nnet-loss.cc:76-142): frame r carries the (pdf, weight) entries
// post_pdf/post_w[post_off[r] .. post_off[r+1]); the reference scatters them into a dense zero matrix (`tgt(t, pdf) += w`,
// so repeated pdfs add up, :86-96) and then works on dense rows.  Here the dense target never exists: one workgroup per
// row writes diff = y*mask, then the first occurrence of every pdf fixes its column to (y - t)*mask (:102-107) and
// contributes -mask*t*log(y) (:122-128) and -mask*t*log(t + 1e-20) (:130-136); the target's arg-max (:113) is found among
// the entries and the implicit zeros with FindRowMaxId's lowest-index tie break.  A frame may have any number of entries: up to
// 256 are staged in LDS for thread 0 (the fast path: diff and row_correct of such a frame are those it has always given); what lies
// past them is kept per thread and combined afterwards, and the lowest zero of such a frame is searched by the whole workgroup.
// The two entropies of every frame are the per-thread sums added in double.
__global__ __launch_bounds__(256) void k_xent_post_rows(const float *__restrict__ y, int cols, int stride, const int *__restrict__ post_off,
                                                        const int *__restrict__ post_pdf, const float *__restrict__ post_w,
                                                        const float *__restrict__ mask, float *__restrict__ diff, int diff_stride,
                                                        float *__restrict__ row_xent, float *__restrict__ row_ent,
                                                        float *__restrict__ row_correct) {
  __shared__ float smv[4];
  __shared__ int smi[4];
  __shared__ float s_xe[256], s_en[256], s_acc[256];
  __shared__ int s_first[256];
  __shared__ float s_tacc[256];                      // rows of more than 256 entries: every thread's best among its entries past the staging
  __shared__ int s_tpdf[256], s_tcnt[256], s_need, s_z;
  const int row = blockIdx.x;
  const float *yp = y + (size_t)row * stride;
  float *dp = diff + (size_t)row * diff_stride;
  const float m = mask[row];
  const int e0 = post_off[row], n = post_off[row + 1] - e0;
  float best = -3.4e38f; int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float v = yp[c];
    dp[c] = v * m;                                   // (y - 0) * mask; columns with a target are redone below
    if (v > best) { best = v; bi = c; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {                 // arg-max of the network output, lowest index on ties
    const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { smv[wave] = best; smi[wave] = bi; }
  __syncthreads();                                   // also orders the dense diff pass before the per-entry fix-up
  float xe = 0.f, en = 0.f;
  float lt = -3.4e38f; int li = 0x7fffffff, lc = 0;   // target arg-max and number of distinct pdfs among this thread's entries >= 256
  for (int e = threadIdx.x; e < n; e += 256) {       // any number of entries: the first 256 are staged in LDS for thread 0, the rest kept per thread
    const int pdf = post_pdf[e0 + e];
    float acc = 0.f; bool first = true;
    for (int k = 0; k < n; k++)
      if (post_pdf[e0 + k] == pdf) { acc += post_w[e0 + k]; if (k < e) first = false; }   // same order of additions as the scatter
    if (e < 256) { s_acc[e] = acc; s_first[e] = first ? pdf : -1; }
    else if (first) { lc++; if (acc > lt || (acc == lt && pdf < li)) { lt = acc; li = pdf; } }
    if (first) {
      const float v = yp[pdf];
      dp[pdf] = (v - acc) * m;                       // :102-107
      xe -= (logf(v) * acc) * m;                     // :122-128
      en -= (logf(acc + 1e-20f) * acc) * m;          // :130-136
    }
  }
  s_xe[threadIdx.x] = xe; s_en[threadIdx.x] = en;
  s_tacc[threadIdx.x] = lt; s_tpdf[threadIdx.x] = li; s_tcnt[threadIdx.x] = lc;
  __syncthreads();
  float tb = -3.4e38f; int ti = 0x7fffffff;
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) if (smv[w] > best || (smv[w] == best && smi[w] < bi)) { best = smv[w]; bi = smi[w]; }
    // the 256 per-thread sums in double, rounded once (a float32 accumulator over 256 terms would lose ~sqrt(256) 2^-25 of the result,
    // more than the 2^-21 that tests/test_output_tail_gpu.py allows)
    double dx = 0.0, de = 0.0;
    for (int t = 0; t < 256; t++) { dx += (double)s_xe[t]; de += (double)s_en[t]; }
    const float sx = (float)dx, se = (float)de;
    // arg-max of the (virtual) dense target row
    const int ne = n < 256 ? n : 256;
    int distinct = 0;
    for (int e = 0; e < ne; e++)
      if (s_first[e] >= 0) { distinct++; if (s_acc[e] > tb || (s_acc[e] == tb && s_first[e] < ti)) { tb = s_acc[e]; ti = s_first[e]; } }
    if (n > 256)
      for (int t = 0; t < 256; t++) {
        distinct += s_tcnt[t];
        if (s_tcnt[t] && (s_tacc[t] > tb || (s_tacc[t] == tb && s_tpdf[t] < ti))) { tb = s_tacc[t]; ti = s_tpdf[t]; }
      }
    const bool zero_wins = distinct < cols && tb <= 0.f;   // an implicit zero is (one of) the maxima: lowest index whose value is 0
    if (zero_wins && n <= 256) {
      int z = 0;
      for (bool again = true; again;) {
        again = false;
        for (int e = 0; e < ne; e++) if (s_first[e] == z && s_acc[e] != 0.f) { z++; again = true; break; }
      }
      if (tb < 0.f || z < ti) ti = z;
    }
    row_xent[row] = sx; row_ent[row] = se;
    if (n <= 256) row_correct[row] = (m == 1.f && bi == ti) ? 1.f : 0.f;
    s_need = zero_wins ? 1 : 0; s_z = 0x7fffffff;
  }
  if (n <= 256) return;
  // more than 256 entries: the accumulated weights past the staging live nowhere, so the lowest zero of the (virtual) dense target row is
  // found by building its columns again, 256 candidates a round with the scatter's order of additions.  At most `distinct` <= n columns
  // are not zero: a few rounds.
  __syncthreads();
  if (s_need) {
    for (int base = 0; base < cols; base += 256) {
      const int c = base + threadIdx.x;
      if (c < cols) {
        float acc = 0.f;
        for (int k = 0; k < n; k++) if (post_pdf[e0 + k] == c) acc += post_w[e0 + k];
        if (!(acc != 0.f)) atomicMin(&s_z, c);
      }
      __syncthreads();
      const bool found = s_z != 0x7fffffff;
      __syncthreads();                               // (nobody lowers s_z in the next round before everyone has read this one's)
      if (found) break;
    }
    if (threadIdx.x == 0 && (tb < 0.f || s_z < ti)) ti = s_z;
  }
  if (threadIdx.x == 0) row_correct[row] = (m == 1.f && bi == ti) ? 1.f : 0.f;
}


// ---------------------------------------------------------------------------------------------
// output tail of the nnet: Softmax rows, Xent::EvalMasked, and the small vector ops of
// AffineTransform::Update.  One 256-thread workgroup per frame row, lane-contiguous column sweeps.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_reduce(float v, float *sm, bool is_max) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o); v = is_max ? fmaxf(v, w) : v + w; }
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  float r = sm[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++) r = is_max ? fmaxf(r, sm[w]) : r + sm[w];
  return r;
}
// Softmax::PropagateFnc [UPSTREAM-unvendored nnet-activation.h -> CuMatrix::ApplySoftMaxPerRow]: y = exp(x - max) / sum
__global__ __launch_bounds__(256) void k_softmax_rows(const float *__restrict__ in, int cols, int in_stride,
                                                      float *__restrict__ out, int out_stride) {
  __shared__ float sm[4];
  const float *ip = in + (size_t)blockIdx.x * in_stride;
  float *op = out + (size_t)blockIdx.x * out_stride;
  float mx = -3.4e38f;
  for (int c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, ip[c]);
  mx = block_reduce(mx, sm, true);
  float sum = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) { const float e = expf(ip[c] - mx); op[c] = e; sum += e; }
  sum = block_reduce(sum, sm, false);
  const float inv = 1.f / sum;
  for (int c = threadIdx.x; c < cols; c += 256) op[c] *= inv;
}
// Wide rows (the 16624-way output layer): 1024 threads per row, the whole row in registers (8 x float4 per thread, all
// loads issued up front), one pass over memory: 26 -> ~6 us at 80 x 16624.  Needs cols % 4 == 0, cols <= 32768 and
// 16-byte aligned rows; other shapes use k_softmax_rows.
__global__ __launch_bounds__(1024) void k_softmax_rows_v(const float *__restrict__ in, int cols, int in_stride,
                                                        float *__restrict__ out, int out_stride) {
  __shared__ float sm[16];
  const float4 *ip = reinterpret_cast<const float4 *>(in + (size_t)blockIdx.x * in_stride);
  float4 *op = reinterpret_cast<float4 *>(out + (size_t)blockIdx.x * out_stride);
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
  mx = block_reduce(mx, sm, true);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const bool on = threadIdx.x + 1024 * u < n4;
    v[u].x = on ? expf(v[u].x - mx) : 0.f; v[u].y = on ? expf(v[u].y - mx) : 0.f;
    v[u].z = on ? expf(v[u].z - mx) : 0.f; v[u].w = on ? expf(v[u].w - mx) : 0.f;
    sum += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  sum = block_reduce(sum, sm, false);
  const float inv = 1.f / sum;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = threadIdx.x + 1024 * u;
    if (c < n4) op[c] = make_float4(v[u].x * inv, v[u].y * inv, v[u].z * inv, v[u].w * inv);
  }
}
// Xent::EvalMasked (google/nnet/nnet-loss.cc:76-142) for one-hot targets (alignments): per frame row
//   diff = (y - t) * mask (:102-107), row_xent = -mask * log(y[target]) (:122-128),
//   row_correct = mask == 1 && argmax(y) == target (:109-120; first maximum wins like FindRowMaxId).
__global__ __launch_bounds__(256) void k_xent_rows(const float *__restrict__ y, int cols, int stride,
                                                   const int *__restrict__ target, const float *__restrict__ mask,
                                                   float *__restrict__ diff, int diff_stride,
                                                   float *__restrict__ row_xent, float *__restrict__ row_correct) {
  __shared__ float smv[4];
  __shared__ int smi[4];
  const int row = blockIdx.x;
  const float *yp = y + (size_t)row * stride;
  float *dp = diff + (size_t)row * diff_stride;
  const int tgt = target[row];
  const float m = mask[row];
  float best = -3.4e38f; int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < cols; c += 256) {
    const float v = yp[c];
    dp[c] = (v - (c == tgt ? 1.f : 0.f)) * m;
    if (v > best) { best = v; bi = c; }
  }
  // argmax with lowest-index tie break
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { smv[wave] = best; smi[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) if (smv[w] > best || (smv[w] == best && smi[w] < bi)) { best = smv[w]; bi = smi[w]; }
    row_xent[row] = (tgt >= 0 && tgt < cols) ? -m * logf(yp[tgt]) : 0.f;
    row_correct[row] = (m == 1.f && bi == tgt) ? 1.f : 0.f;
  }
}
__global__ __launch_bounds__(1024) void k_xent_rows_v(const float *__restrict__ y, int cols, int stride,
                                                     const int *__restrict__ target, const float *__restrict__ mask,
                                                     float *__restrict__ diff, int diff_stride,
                                                     float *__restrict__ row_xent, float *__restrict__ row_correct) {
  __shared__ float smv[16];
  __shared__ int smi[16];
  const int row = blockIdx.x;
  const float4 *yp = reinterpret_cast<const float4 *>(y + (size_t)row * stride);
  float4 *dp = reinterpret_cast<float4 *>(diff + (size_t)row * diff_stride);
  const int tgt = target[row];
  const float m = mask[row];
  const int n4 = cols >> 2;
  float4 v[8];
#pragma unroll
  for (int u = 0; u < 8; u++) { const int c = threadIdx.x + 1024 * u; v[u] = yp[c < n4 ? c : 0]; }
  float best = -3.4e38f; int bi = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = threadIdx.x + 1024 * u;
    if (c < n4) {
      const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int col = 4 * c + j;
        d[j] = (e[j] - (col == tgt ? 1.f : 0.f)) * m;
        if (e[j] > best) { best = e[j]; bi = col; }          // ascending columns per thread: first maximum wins
      }
      dp[c] = make_float4(d[0], d[1], d[2], d[3]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { smv[wave] = best; smi[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) if (smv[w] > best || (smv[w] == best && smi[w] < bi)) { best = smv[w]; bi = smi[w]; }
    row_xent[row] = (tgt >= 0 && tgt < cols) ? -m * logf(y[(size_t)row * stride + tgt]) : 0.f;
    row_correct[row] = (m == 1.f && bi == tgt) ? 1.f : 0.f;
  }
}
// Softmax and Xent::EvalMasked of a wide row in ONE pass: k_softmax_rows_v's arithmetic, then k_xent_rows_v's on the registers
// (same operations in the same order: the same bits as the pair), the posterior row written only if the caller wants it.
// 80 x 16624: 9.2 + 6.3 us and 21 MB -> one launch, 10.6 MB.
__global__ __launch_bounds__(1024) void k_softmax_xent_rows_v(const float *__restrict__ in, int cols, int in_stride, float *__restrict__ post,
                                                             int post_stride, const int *__restrict__ target, const float *__restrict__ mask,
                                                             float *__restrict__ diff, int diff_stride, float *row_xent,
                                                             float *row_correct, double *totals, unsigned *ticket) {
  __shared__ float sm[16];
  __shared__ float smv[16];
  __shared__ int smi[16];
  __shared__ float s_yt;
  __shared__ int s_last;
  __shared__ double s_tot[3][16];
  const int row = blockIdx.x;
  const float4 *ip = reinterpret_cast<const float4 *>(in + (size_t)row * in_stride);
  float4 *dp = reinterpret_cast<float4 *>(diff + (size_t)row * diff_stride);
  const int tgt = target[row];
  const float m = mask[row];
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
  mx = block_reduce(mx, sm, true);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const bool on = threadIdx.x + 1024 * u < n4;
    v[u].x = on ? expf(v[u].x - mx) : 0.f; v[u].y = on ? expf(v[u].y - mx) : 0.f;
    v[u].z = on ? expf(v[u].z - mx) : 0.f; v[u].w = on ? expf(v[u].w - mx) : 0.f;
    sum += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  sum = block_reduce(sum, sm, false);
  const float inv = 1.f / sum;
  float best = -3.4e38f; int bi = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    const int c = threadIdx.x + 1024 * u;
    if (c < n4) {
      const float e[4] = {v[u].x * inv, v[u].y * inv, v[u].z * inv, v[u].w * inv};
      if (post) reinterpret_cast<float4 *>(post + (size_t)row * post_stride)[c] = make_float4(e[0], e[1], e[2], e[3]);
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int col = 4 * c + j;
        d[j] = (e[j] - (col == tgt ? 1.f : 0.f)) * m;
        if (col == tgt) s_yt = e[j];
        if (e[j] > best) { best = e[j]; bi = col; }          // ascending columns per thread: first maximum wins
      }
      dp[c] = make_float4(d[0], d[1], d[2], d[3]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { smv[wave] = best; smi[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) if (smv[w] > best || (smv[w] == best && smi[w] < bi)) { best = smv[w]; bi = smi[w]; }
    // (write-through, agent scope: the workgroup that takes the last ticket reads them with agent-scope loads)
    __hip_atomic_store(row_xent + row, (tgt >= 0 && tgt < cols) ? -m * logf(s_yt) : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(row_correct + row, (m == 1.f && bi == tgt) ? 1.f : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!totals) return;
  // statistics onto the device totals without a launch of their own: the workgroup that takes the last ticket sees every row's two
  // numbers and adds them up in a fixed order.  Round 6: the two numbers leave as write-through (sc1) stores and the ticket is taken
  // once they are acknowledged (s_waitcnt vmcnt(0)) -- no __threadfence(): an agent-scope release writes back EVERY dirty line of the
  // L2 (here: the 5.3 MB of derivatives the launch has just stored; ~3.5 us and more per workgroup, MI355X_MICROARCH.md) for 8 bytes
  // that matter.  The same store-then-flag idiom as the granules of the persistent chains (klstm_persist_dev.h publish()).
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  for (int r = threadIdx.x; r < (int)gridDim.x; r += 1024) {
    t0 += (double)__hip_atomic_load(row_xent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t1 += (double)__hip_atomic_load(row_correct + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t2 += (double)mask[r];
  }
  for (int o = 32; o > 0; o >>= 1) { t0 += __shfl_xor(t0, o); t1 += __shfl_xor(t1, o); t2 += __shfl_xor(t2, o); }
  if (lane == 0) { s_tot[0][wave] = t0; s_tot[1][wave] = t1; s_tot[2][wave] = t2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int w = 0; w < 16; w++) t += s_tot[threadIdx.x][w];
    totals[threadIdx.x] += t;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (ready for the next launch on this stream)
}
// dst[j] = beta*dst[j] + sum_rows src[row][j]   (AddRowSumMat)
// dst[j] = beta*dst[j] + sum over rows of src[r][j]: 64 columns x 4 row groups per workgroup, 8 loads in flight per thread
// (a serial row loop costs one memory latency per row: 20 us for 80 rows), row groups combined through LDS in fixed order
__global__ __launch_bounds__(256) void k_col_sum(const float *__restrict__ src, int rows, int cols, int stride, float beta,
                                                 float *__restrict__ dst) {
  __shared__ float part[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + tx;
  const int jc = j < cols ? j : 0;
  float s = 0.f;
  for (int r0 = ty; r0 < rows; r0 += 32) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; u++) t[u] = src[(size_t)min(r0 + 4 * u, rows - 1) * stride + jc];
#pragma unroll
    for (int u = 0; u < 8; u++) s += (r0 + 4 * u < rows) ? t[u] : 0.f;
  }
  part[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && j < cols) {
    s = part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx];
    dst[j] = (beta != 0.f ? beta * dst[j] : 0.f) + s;
  }
}
__global__ void k_axpy(float *__restrict__ y, const float *__restrict__ x, float a, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = y[i] + a * x[i];
}

// corr = mmt*corr + grad ; param -= lr*corr  in one pass (the post-all-reduce step of a data-parallel Affine layer)
__global__ void k_sgd_momentum(float *__restrict__ param, float *__restrict__ corr, const float *__restrict__ grad, float mmt,
                               float lr, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float c = mmt * corr[i] + grad[i];
    corr[i] = c;
    param[i] = param[i] + (-lr) * c;
  }
}
__global__ void k_apply_momentum(float *__restrict__ corr, const float *__restrict__ grad, float mmt, long n, const unsigned *guard,
                                 const float *mark) {
  if (guard && (guard[2] | guard[6] | guard[9])) return;          // a persistent launch of this minibatch gave up: its gradient must not reach the momentum buffers
  if (mark && *mark != 0.f) return;                               // (or a peer's: UpdArgs::mark)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    corr[i] = mmt * corr[i] + grad[i];
}

// Loss statistics of a minibatch onto device totals (Xent::EvalMasked adds its three scalars to loss_, correct_, frames_ on the host,
// nnet-loss.cc:136-141; a trainer that reports every N minibatches reads the totals once): totals[0] += sum row_xent (double),
// totals[1] += sum row_correct, totals[2] += sum mask.  One workgroup, fixed summation order.
__global__ __launch_bounds__(256) void k_xent_accumulate(const float *__restrict__ row_xent, const float *__restrict__ row_correct,
                                                          const float *__restrict__ mask, int rows, double *totals) {
  __shared__ double red[3][256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) { s0 += (double)row_xent[r]; s1 += (double)row_correct[r]; s2 += (double)mask[r]; }
  red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int q = 0; q < 3; q++) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 3) totals[threadIdx.x] += red[threadIdx.x][0];
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline int ew_grid(long n) { long g = (n + 255) / 256; return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g)); }
// a row fits the registers of 1024 threads in 16-byte pieces (the _v row kernels); a, b: the two row arrays the kernel moves that way
static bool row_in_registers(int cols, const float *a, int a_stride, const float *b, int b_stride) {
  return cols % 4 == 0 && cols <= 32768 && cols >= 2048 && a_stride % 4 == 0 && b_stride % 4 == 0 && aligned16(a) && aligned16(b);
}

hipError_t launch_time_shift(const float *in, int rows, int cols, int in_stride, float *out, int out_stride, int shift,
                             hipStream_t st, LaunchProbe pr) {
  const int vec = aligned16(in) && aligned16(out) && in_stride % 4 == 0 && out_stride % 4 == 0 && cols % 4 == 0;
  const int per = vec ? 4 : 1;
  return launch(k_time_shift, dim3(cdiv(cdiv(cols, per), 256), rows), dim3(256), 0, st, pr, in, rows, cols, in_stride, out, out_stride, shift, vec);
}

hipError_t launch_softmax(const float *in, int rows, int cols, int in_stride, float *out, int out_stride, hipStream_t st) {
  LaunchProbe pr;
  const bool wide = row_in_registers(cols, in, in_stride, out, out_stride);
  if (wide) return launch(k_softmax_rows_v, dim3(rows), dim3(1024), 0, st, pr, in, cols, in_stride, out, out_stride);
  return launch(k_softmax_rows, dim3(rows), dim3(256), 0, st, pr, in, cols, in_stride, out, out_stride);
}
hipError_t launch_xent(const float *y, int rows, int cols, int stride, const int *target, const float *mask, float *diff,
                       int diff_stride, float *row_xent, float *row_correct, hipStream_t st) {
  LaunchProbe pr;
  const bool wide = row_in_registers(cols, y, stride, diff, diff_stride);
  if (wide) return launch(k_xent_rows_v, dim3(rows), dim3(1024), 0, st, pr, y, cols, stride, target, mask, diff, diff_stride, row_xent, row_correct);
  return launch(k_xent_rows, dim3(rows), dim3(256), 0, st, pr, y, cols, stride, target, mask, diff, diff_stride, row_xent, row_correct);
}
// one pass when the row fits the registers of 1024 threads (returns hipErrorNotSupported otherwise: the caller runs the pair)
hipError_t launch_softmax_xent(const float *in, int rows, int cols, int in_stride, float *post, int post_stride, const int *target,
                               const float *mask, float *diff, int diff_stride, float *row_xent, float *row_correct, double *totals,
                               unsigned *ticket, hipStream_t st) {
  LaunchProbe pr;
  const bool wide = row_in_registers(cols, in, in_stride, diff, diff_stride) && (!post || (post_stride % 4 == 0 && aligned16(post)));
  if (!wide) return hipErrorNotSupported;
  return launch(k_softmax_xent_rows_v, dim3(rows), dim3(1024), 0, st, pr, in, cols, in_stride, post, post_stride, target, mask, diff, diff_stride, row_xent, row_correct, totals, ticket);
}
hipError_t launch_xent_post(const float *y, int rows, int cols, int stride, const int *post_off, const int *post_pdf, const float *post_w,
                            const float *mask, float *diff, int diff_stride, float *row_xent, float *row_ent, float *row_correct,
                            hipStream_t st) {
  LaunchProbe pr;
  return launch(k_xent_post_rows, dim3(rows), dim3(256), 0, st, pr, y, cols, stride, post_off, post_pdf, post_w, mask, diff, diff_stride, row_xent, row_ent, row_correct);
}
hipError_t launch_xent_accumulate(const float *row_xent, const float *row_correct, const float *mask, int rows, double *totals, hipStream_t st) {
  LaunchProbe pr;
  return launch(k_xent_accumulate, dim3(1), dim3(256), 0, st, pr, row_xent, row_correct, mask, rows, totals);
}
hipError_t launch_col_sum(const float *src, int rows, int cols, int stride, float beta, float *dst, hipStream_t st) {
  LaunchProbe pr;
  return launch(k_col_sum, dim3(cdiv(cols, 64)), dim3(256), 0, st, pr, src, rows, cols, stride, beta, dst);
}
hipError_t launch_axpy(float *y, const float *x, float a, long n, hipStream_t st) {
  LaunchProbe pr;
  return launch(k_axpy, dim3(ew_grid(n)), dim3(256), 0, st, pr, y, x, a, n);
}
hipError_t launch_sgd_momentum(float *param, float *corr, const float *grad, float mmt, float lr, long n, hipStream_t st) {
  LaunchProbe pr;
  return launch(k_sgd_momentum, dim3(ew_grid(n)), dim3(256), 0, st, pr, param, corr, grad, mmt, lr, n);
}
hipError_t launch_apply_momentum(float *corr, const float *grad, float mmt, long n, hipStream_t st, LaunchProbe pr, const unsigned *guard,
                                 const float *mark) {
  return launch(k_apply_momentum, dim3(ew_grid(n)), dim3(256), 0, st, pr, corr, grad, mmt, n, guard, mark);
}

}  // namespace klstm
