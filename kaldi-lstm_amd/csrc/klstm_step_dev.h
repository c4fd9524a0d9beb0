// kaldi-lstm_amd/csrc/klstm_step_dev.h -- device pieces that the step kernels (klstm_kernels.hip) and the tile GEMM
// (klstm_gemm_dev.h) both use: the guarded / branch-free operand fetches and the K chunk of the folded operands.
#pragma once
#include "klstm_math.h"

namespace klstm {

#pragma clang fp contract(off)

// ---- operand fetch helpers -----------------------------------------------------------------------
// VEC = true : rows are 16-byte aligned and every contraction length is a multiple of 8.  The load is
//              branch-free: a lane that is out of range reads the (always valid) start of its row and
//              the result is zeroed with selects, so every load of a kernel can be in flight at once.
// VEC = false: generic per-element guarded loads (odd test shapes); correct but latency-serialised.
template <bool VEC>
__device__ __forceinline__ void load8(const float *__restrict__ row, int k, int K, bool ok, float (&v)[8]) {
  if (VEC) {
    const bool in = ok && (k + 8 <= K);
    const float4 *p = reinterpret_cast<const float4 *>(row + (in ? k : 0));
    const float4 a = p[0], b = p[1];
    v[0] = in ? a.x : 0.f; v[1] = in ? a.y : 0.f; v[2] = in ? a.z : 0.f; v[3] = in ? a.w : 0.f;
    v[4] = in ? b.x : 0.f; v[5] = in ? b.y : 0.f; v[6] = in ? b.z : 0.f; v[7] = in ? b.w : 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (ok && k + j < K) ? row[k + j] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void store8(float *__restrict__ row, int k, int K, const float (&v)[8]) {
  if (VEC) {
    if (k + 8 <= K) {
      *reinterpret_cast<float4 *>(row + k) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4 *>(row + k + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j++) if (k + j < K) row[k + j] = v[j];
  }
}
// 4 consecutive columns c..c+3 of a row (VEC: C % 4 == 0, 16-byte aligned rows)
template <bool VEC>
__device__ __forceinline__ void load4(const float *__restrict__ p, int c, int C, bool ok, float (&v)[4]) {
  if (VEC) {
    const bool in = ok && (c + 4 <= C);
    const float4 a = *reinterpret_cast<const float4 *>(p + (in ? c : 0));
    v[0] = in ? a.x : 0.f; v[1] = in ? a.y : 0.f; v[2] = in ? a.z : 0.f; v[3] = in ? a.w : 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = (ok && c + j < C) ? p[c + j] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ p, int c, int C, const float (&v)[4]) {
  if (VEC) { if (c + 4 <= C) *reinterpret_cast<float4 *>(p + c) = make_float4(v[0], v[1], v[2], v[3]); }
  else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (c + j < C) p[c + j] = v[j];
  }
}

// Zero a fetched vector where the lane's element is padding.  Written as a bitwise AND with an OPAQUE lane mask: as a
// select the compiler sinks the load into a conditional block and drains every outstanding load (s_waitcnt vmcnt(0)) at
// its join -- the activation slab of the gates kernel was two serialized memory round trips in front of the weight fetch.
__device__ __forceinline__ float4 keep_if(const float4 &v, bool c) {
  unsigned m = c ? 0xffffffffu : 0u;
  asm volatile("" : "+v"(m));
  return make_float4(__builtin_bit_cast(float, __builtin_bit_cast(unsigned, v.x) & m),
                     __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v.y) & m),
                     __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v.z) & m),
                     __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v.w) & m));
}
__device__ __forceinline__ float4 ldg4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

constexpr int KCH4 = 128;                  // K chunk of the 4-row geometry (FOLDED RECURRENCE, klstm_kernels.hip): k_dmf_v, launch_fold, pack_sizes_fold

}  // namespace klstm
