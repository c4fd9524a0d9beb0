// kaldi-lstm_amd/csrc/klstm_dropout.hip -- forward-connection dropout with a counter-based mask: the two kdrop_* entries of
// include/klstm_dropout.h (which defines every quantity; the numpy twin: tests/dropout_ref.py) and their kernels.
//   k_drop_element<COPY>  one lane per QUAD of four columns: one Philox4x32-10 call gives the quad's four words.  Lanes run along the
//                  quads of a row, then down the rows: a grid-stride pass of at most DROP_MAX_WG workgroups of 256 whose (row, quad)
//                  pair is stepped, not divided, from one pass to the next.  COPY (p == 1 out of place): the same walk without the
//                  draw and without the selection.
//   k_drop_sequence  KDROP_SEQUENCE: an item is (split, stream, quad); its lane draws the words of (stream, quad) ONCE and walks down
//                  that stream's rows r = s + S (split + k nsplit).  nsplit is chosen on the host so that the items fill the grid.
// Both move a whole quad as one float4 in and one float4 out (16 bytes per lane) when both pointers and both strides are 16-byte
// aligned; the tail quad of a row, and every quad otherwise, goes element by element through the same selection: the same bits.
// No LDS, no atomics, nothing stored but the output.
// BOUNDS.  A lane touches columns 4 q .. min(4 q + 3, cols - 1) of a row r < rows only; q < ceil(cols / 4); seq_id is read at
// s < min(S, rows).  Row offsets are size_t products.  In place every element is read before it is written, by the same lane.
#include <cstdint>

#include "../../include/klstm_dropout.h"
#include "klstm_host.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr unsigned DROP_MAX_WG = 2048;     // the cap of a memory-bound grid-stride pass (256 CUs x 8 workgroups)

struct DropWords { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al. 2011): counter (c0, c1, c2, c3), key (k0, k1)
__host__ __device__ __forceinline__ DropWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return DropWords{{c0, c1, c2, c3}};
}

struct DropArgs {
  const float *in; float *out;
  int in_stride, out_stride, rows, cols;
  uint32_t nq;            // quads per row, the tail quad included
  uint32_t thr; float scale;
  uint32_t k0, k1, step, tag;
  int vec;                // both pointers and both strides 16-byte aligned
};

template <bool COPY>
__device__ __forceinline__ void drop_quad(const DropArgs &a, size_t r, uint32_t q, const DropWords &d) {
  const float *ip = a.in + r * (size_t)a.in_stride + (size_t)q * 4;
  float *op = a.out + r * (size_t)a.out_stride + (size_t)q * 4;
  const int n = a.cols - (int)(q * 4);            // >= 1: q < nq
  if (a.vec && n >= 4) {
    const float4 v = *reinterpret_cast<const float4 *>(ip);
    float4 o;
    if (COPY) {
      o = v;
    } else {
      o.x = d.w[0] < a.thr ? v.x * a.scale : 0.f;
      o.y = d.w[1] < a.thr ? v.y * a.scale : 0.f;
      o.z = d.w[2] < a.thr ? v.z * a.scale : 0.f;
      o.w = d.w[3] < a.thr ? v.w * a.scale : 0.f;
    }
    *reinterpret_cast<float4 *>(op) = o;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < n) op[j] = COPY ? ip[j] : (d.w[j] < a.thr ? ip[j] * a.scale : 0.f);
  }
}

template <bool COPY>
__global__ __launch_bounds__(256) void k_drop_element(DropArgs a) {
  const uint32_t stride = gridDim.x * 256u, i0 = blockIdx.x * 256u + threadIdx.x;     // < 2^19
  const uint32_t dr = stride / a.nq, dq = stride - dr * a.nq;
  uint32_t r = i0 / a.nq, q = i0 - r * a.nq;                                          // r < 2^31 + 2^19 + 1: no wrap
  while (r < (uint32_t)a.rows) {
    DropWords d = {};
    if (!COPY) d = philox4x32_10(q, r, a.step, a.tag, a.k0, a.k1);
    drop_quad<COPY>(a, r, q, d);
    r += dr; q += dq;
    if (q >= a.nq) { q -= a.nq; r++; }
  }
}

__global__ __launch_bounds__(256) void k_drop_sequence(DropArgs a, const unsigned *__restrict__ seq_id, uint32_t S, uint32_t Seff,
                                                      uint32_t nsplit) {
  const unsigned long long per = (unsigned long long)Seff * a.nq, items = per * nsplit;
  const unsigned long long hop = (unsigned long long)nsplit * S;
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < items; i += gridDim.x * 256ull) {
    const unsigned long long sq = i % per;
    const uint32_t split = (uint32_t)(i / per), s = (uint32_t)(sq / a.nq), q = (uint32_t)(sq - (unsigned long long)s * a.nq);
    const DropWords d = philox4x32_10(q, seq_id[s], 0u, a.tag, a.k0, a.k1);
    for (unsigned long long r = s + (unsigned long long)split * S; r < (unsigned long long)a.rows; r += hop) drop_quad<false>(a, (size_t)r, q, d);
  }
}

static bool drop_retention_ok(float p) { return p >= 0x1p-32f && p <= 1.f; }      // false for a NaN
static void drop_numbers(float p, unsigned *thr, float *scale) {
  const double t = (double)p * 4294967296.0;                                       // exact: a float times a power of two
  *thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;                            // t >= 1: the cast is the floor
  *scale = 1.0f / p;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

klstm_status kdrop_threshold(float retention, unsigned *thr, float *scale) {
  if (!thr || !scale) return fail(KLSTM_ERR_ARG, "kdrop_threshold: null argument");
  if (!drop_retention_ok(retention)) return fail(KLSTM_ERR_ARG, "kdrop_threshold: retention %g outside [2^-32, 1]", (double)retention);
  drop_numbers(retention, thr, scale);
  return KLSTM_OK;
}

klstm_status kdrop_apply(const float *in, int in_stride, int rows, int cols, float *out, int out_stride, float retention,
                         unsigned long long seed, unsigned step, unsigned salt, int mode, int num_stream, const unsigned *seq_id_dev,
                         void *hip_stream) {
  if (rows < 0 || cols < 0) return fail(KLSTM_ERR_ARG, "kdrop_apply: bad size (rows %d, cols %d)", rows, cols);
  if (!drop_retention_ok(retention)) return fail(KLSTM_ERR_ARG, "kdrop_apply: retention %g outside [2^-32, 1]", (double)retention);
  if (salt >= 0x80000000u) return fail(KLSTM_ERR_ARG, "kdrop_apply: salt %u is not below 2^31", salt);
  if (mode != KDROP_ELEMENT && mode != KDROP_SEQUENCE) return fail(KLSTM_ERR_ARG, "kdrop_apply: unknown mode %d", mode);
  if (mode == KDROP_SEQUENCE && num_stream < 1) return fail(KLSTM_ERR_ARG, "kdrop_apply: num_stream %d in KDROP_SEQUENCE", num_stream);
  if (mode == KDROP_SEQUENCE && !seq_id_dev) return fail(KLSTM_ERR_ARG, "kdrop_apply: KDROP_SEQUENCE needs seq_id_dev");
  if (rows == 0 || cols == 0) return KLSTM_OK;
  if (!in || !out) return fail(KLSTM_ERR_ARG, "kdrop_apply: null argument");
  if (in_stride < cols || out_stride < cols)
    return fail(KLSTM_ERR_ARG, "kdrop_apply: row stride below the column count (%d / %d < %d)", in_stride, out_stride, cols);
  if (in == out) {
    if (in_stride != out_stride) return fail(KLSTM_ERR_ARG, "kdrop_apply: in == out with two strides (%d, %d)", in_stride, out_stride);
  } else {
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + ((size_t)(rows - 1) * in_stride + cols) * sizeof(float);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + ((size_t)(rows - 1) * out_stride + cols) * sizeof(float);
    if (a0 < b1 && b0 < a1) return fail(KLSTM_ERR_ARG, "kdrop_apply: in and out overlap (only in == out may)");
  }
  const bool copy = retention == 1.f;
  if (copy && in == out) return KLSTM_OK;

  DropArgs a;
  a.in = in; a.out = out; a.in_stride = in_stride; a.out_stride = out_stride; a.rows = rows; a.cols = cols;
  a.nq = ((uint32_t)cols + 3u) / 4u;
  a.thr = 0; a.scale = 1.f;
  if (!copy) drop_numbers(retention, &a.thr, &a.scale);
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.step = step;
  a.tag = mode == KDROP_SEQUENCE ? (salt | 0x80000000u) : salt;
  a.vec = ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0) && in_stride % 4 == 0 && out_stride % 4 == 0;
  hipStream_t st = (hipStream_t)hip_stream;
  const unsigned long long target = (unsigned long long)DROP_MAX_WG * 256;
  if (copy || mode == KDROP_ELEMENT) {
    const unsigned long long items = (unsigned long long)rows * a.nq;
    const unsigned grid = (unsigned)((items < target ? items : target) + 255) / 256;
    if (copy) HIPCHK(launch(k_drop_element<true>, dim3(grid), dim3(256), 0, st, LaunchProbe(), a));
    else HIPCHK(launch(k_drop_element<false>, dim3(grid), dim3(256), 0, st, LaunchProbe(), a));
  } else {
    const uint32_t S = (uint32_t)num_stream, Seff = S < (uint32_t)rows ? S : (uint32_t)rows;
    const unsigned long long per = (unsigned long long)Seff * a.nq, frames = ((unsigned long long)rows + S - 1) / S;
    unsigned long long nsplit = (target + per - 1) / per;                       // enough items to fill the grid, at most one per frame
    if (nsplit > frames) nsplit = frames;
    if (nsplit < 1) nsplit = 1;
    const unsigned long long items = per * nsplit;
    const unsigned grid = (unsigned)((items < target ? items : target) + 255) / 256;
    HIPCHK(launch(k_drop_sequence, dim3(grid), dim3(256), 0, st, LaunchProbe(), a, seq_id_dev, S, Seff, (uint32_t)nsplit));
  }
  return KLSTM_OK;
}

}  // extern "C"
