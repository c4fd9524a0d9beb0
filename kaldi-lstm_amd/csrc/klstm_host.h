// kaldi-lstm_amd/csrc/klstm_host.h -- what the host-side translation units behind the C-ABI of include/klstm.h share (klstm_engine.hip,
// klstm_api_ops.hip, klstm_api_ctc.hip, klstm_comm.hip): the one error channel that klstm_last_error() reads, and HIPCHK.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/klstm.h"

namespace klstm {

// Both write the calling thread's error string (one thread_local, defined in klstm_engine.hip): the last failure or note wins.
klstm_status fail(klstm_status st, const char *fmt, ...);
void note(const char *fmt, ...);   // a remark for klstm_last_error() that is not a failure (why a faster path was not taken)

constexpr int NT2_TICKETS = 8192;   // ticket words of a split-K launch of klstm_gemm16.hip (the engine's, and klstm_debug_gemm_bf16_nt2's)

}  // namespace klstm

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return ::klstm::fail(KLSTM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
