// kaldi-lstm_amd/csrc/klstm_ctc_dev.h -- device code shared by the CTC kernels (klstm_ctc.hip: the loss; klstm_ctc_align.hip: the forced
// alignment): the status of an utterance and the maximum over a wave.
#pragma once
#include <hip/hip_runtime.h>

namespace klstm {

constexpr float CTC_NEG = -1e30f;      // "log 0": absorbs every offset (ulp 7e22), exp(CTC_NEG - m) = 0

// 0 idle (len 0), 1 feasible, 2 rejected.  Uniform over the workgroup; sm: 2 ints of LDS.
__device__ __forceinline__ int ctc_status(int len, int T, int L, int Lcap, const int *__restrict__ lab, int K, int blank, int *sm) {
  if (len == 0) return 0;
  if (len < 0 || len > T || L < 0 || L > Lcap) return 2;
  if (threadIdx.x == 0) { sm[0] = 0; sm[1] = 0; }
  __syncthreads();
  int rep = 0, bad = 0;
  for (int j = threadIdx.x; j < L; j += blockDim.x) {
    const int c = lab[j];
    bad |= (c < 0 || c >= K || c == blank);
    rep += (j > 0 && lab[j - 1] == c);
  }
  if (rep) atomicAdd(&sm[0], rep);       // integer: the order of arrival does not matter
  if (bad) atomicOr(&sm[1], 1);
  __syncthreads();
  const int r = sm[0], b = sm[1];
  __syncthreads();
  return (b || len < L + r) ? 2 : 1;
}

// Maximum over the wave, the same value in every lane.  DPP row shifts and row broadcasts (the data path of the VALU, a few cycles
// each) instead of six trips through the LDS crossbar (__shfl_xor = ds_bpermute): this reduction sits on the dependent chain of
// every step.  max is idempotent, so the inclusive-scan form needs no bank masks; lanes without a source keep their own value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return fmaxf(v, __int_as_float(o));
}
__device__ __forceinline__ float wave_max(float v) {
  v = dpp_max<0x111, 0xf>(v);      // row_shr:1
  v = dpp_max<0x112, 0xf>(v);      // row_shr:2
  v = dpp_max<0x114, 0xf>(v);      // row_shr:4
  v = dpp_max<0x118, 0xf>(v);      // row_shr:8   lane 15 of every row of 16: the row's maximum
  v = dpp_max<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
  v = dpp_max<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3: lane 63 holds the maximum of the wave
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

}  // namespace klstm
