// kaldi-lstm_amd/csrc/klstm_api_ops.hip -- the C-ABI entries of include/klstm.h that take no engine: device memory helpers (with the
// one-wave kernel of small device-to-host copies), klstm_time_shift, AffineTransform / Softmax / Xent, the stream packers, the SGD step,
// and the klstm_debug_* entries that tests and probes use.  Checks, then one launcher of klstm_kernels.h each.
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <utility>

#include "klstm_host.h"
#include "klstm_kernels.h"

using namespace klstm;

static int g_d2h_small = 1;           // process-wide A-B knob ("d2h_small"): klstm_memcpy_d2h's small-copy kernel (below)
void klstm::set_d2h_small(int v) { g_d2h_small = v != 0; }

extern "C" {

klstm_status klstm_time_shift(const float *in, int rows, int cols, int in_stride, float *out, int out_stride, int shift,
                              void *hip_stream) {
  if (!in || !out) return fail(KLSTM_ERR_ARG, "klstm_time_shift: null argument");
  if (rows < 0 || cols < 0 || in_stride < cols || out_stride < cols) return fail(KLSTM_ERR_ARG, "klstm_time_shift: bad shape");
  if (rows == 0 || cols == 0) return KLSTM_OK;
  HIPCHK(launch_time_shift(in, rows, cols, in_stride, out, out_stride, shift, (hipStream_t)hip_stream));
  return KLSTM_OK;
}

// ---- device memory helpers (keep the C++ mirror and other FFI users free of HIP headers) ----
klstm_status klstm_malloc(void **p, size_t bytes) {
  if (!p) return fail(KLSTM_ERR_ARG, "klstm_malloc: null argument");
  HIPCHK(hipMalloc(p, bytes ? bytes : 4));
  return KLSTM_OK;
}
klstm_status klstm_free(void *p) { if (p) HIPCHK(hipFree(p)); return KLSTM_OK; }
klstm_status klstm_memcpy_h2d(void *dst, const void *src, size_t bytes, void *hip_stream) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  return KLSTM_OK;
}
// Small device-to-host copies -- the three scalars Xent::EvalMasked reads back EVERY minibatch (google/nnet/nnet-loss.cc:110-141: what an
// unmodified bd-nnet-train-lstm-streams does), a CuVector::CopyToVec of a few numbers.  hipMemcpy of pageable memory costs ~45 us of idle
// GPU per call on this stack (staging + completion signal + wake-up: profiles/r05 kaldi_adapter with_d2h_per_minibatch), a third of a
// 150 us minibatch.  Up to D2H_SMALL_BYTES the copy is a ONE-WAVE KERNEL on the caller's stream that writes {sequence tag, word} granules
// into a host-mapped staging buffer (8-byte system-scope stores: tag and word cannot tear, the data is the flag -- no fence, no completion
// signal; the idiom of the persistent chains' granules and of "persist_verify"'s done word), and the host spins on the tags: it has the
// numbers one PCIe write after the kernel ran.  Same semantics as before: stream-ordered behind everything queued on hip_stream, returns
// when dst is filled.  Anything else (larger, unaligned, no mapped memory) takes hipMemcpyAsync + hipStreamSynchronize.
constexpr size_t D2H_SMALL_BYTES = 256;
__global__ __launch_bounds__(64) void k_d2h_small(const unsigned *__restrict__ src, unsigned long long *dst, int nwords, unsigned seq) {
  const int i = threadIdx.x;
  if (i < nwords)
    __hip_atomic_store(dst + i, ((unsigned long long)seq << 32) | src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
struct D2hStage {
  unsigned long long *host = nullptr, *dev = nullptr;
  int device = -1;
  unsigned seq = 0;
  bool broken = false;
  ~D2hStage() { if (host) (void)hipHostFree(host); }
};
static bool d2h_small(void *dst, const void *src, size_t bytes, hipStream_t st) {
  static thread_local D2hStage sg;    // (the call is synchronous: one staging buffer per calling thread)
  if (!g_d2h_small || sg.broken || bytes == 0 || bytes > D2H_SMALL_BYTES || (bytes & 3) || (reinterpret_cast<uintptr_t>(src) & 3)) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (!sg.host) {
    void *hp = nullptr;
    if (hipHostMalloc(&hp, (D2H_SMALL_BYTES / 4) * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
      (void)hipGetLastError(); sg.broken = true; return false;
    }
    memset(hp, 0, (D2H_SMALL_BYTES / 4) * sizeof(unsigned long long));
    sg.host = static_cast<unsigned long long *>(hp);
  }
  if (sg.device != dev) {
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, sg.host, 0) != hipSuccess) { (void)hipGetLastError(); sg.broken = true; return false; }
    sg.dev = static_cast<unsigned long long *>(dp); sg.device = dev;
  }
  if (++sg.seq == 0) sg.seq = 1;      // (0 = what the buffer holds before its first use)
  const int nw = (int)(bytes / 4);
  if (launch(k_d2h_small, dim3(1), dim3(64), 0, st, LaunchProbe{}, static_cast<const unsigned *>(src), sg.dev, nw, sg.seq) != hipSuccess)
    return false;
  const volatile unsigned long long *q = sg.host;
  const auto t0 = std::chrono::steady_clock::now();
  int have = 0;
  bool synced = false;
  for (unsigned spins = 1; have < nw; spins++) {
    while (have < nw && (unsigned)(q[have] >> 32) == sg.seq) have++;
    if (have == nw) break;
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
    if ((spins & 1023) == 0 && !synced && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
      // a long queue in front of the copy: sleep in the runtime instead of burning a core; the granules are there when it returns
      if (hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return false; }
      synced = true;
    } else if (synced && (spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      return false;                   // (never seen: the ordinary copy answers)
    }
  }
  unsigned *out = static_cast<unsigned *>(dst);
  if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) for (int i = 0; i < nw; i++) out[i] = (unsigned)q[i];
  else for (int i = 0; i < nw; i++) { const unsigned w = (unsigned)q[i]; memcpy(static_cast<char *>(dst) + 4 * i, &w, 4); }
  return true;
}
klstm_status klstm_memcpy_d2h(void *dst, const void *src, size_t bytes, void *hip_stream) {
  if (d2h_small(dst, src, bytes, (hipStream_t)hip_stream)) return KLSTM_OK;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_memset_zero(void *dst, size_t bytes, void *hip_stream) {
  HIPCHK(hipMemsetAsync(dst, 0, bytes, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_stream_synchronize(void *hip_stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  return KLSTM_OK;
}

// ---- AffineTransform / Softmax / Xent::EvalMasked (stateless) ----
klstm_status klstm_affine_propagate(const float *in, int rows, int in_dim, int in_stride, const float *W,
                                    const float *bias, float *out, int out_dim, int out_stride, void *hip_stream) {
  if (!in || !W || !out) return fail(KLSTM_ERR_ARG, "klstm_affine_propagate: null argument");
  if (direct_nt_supported(rows, out_dim, in_dim, in, in_stride, W, in_dim)) {     // few frames, wide layer: the output tail
    HIPCHK(launch_direct_nt(rows, out_dim, in_dim, in, in_stride, W, in_dim, out, out_stride, bias, (hipStream_t)hip_stream));
    return KLSTM_OK;
  }
  HIPCHK(launch_gemm(false, true, rows, out_dim, in_dim, in, in_stride, W, in_dim, 0.f, out, out_stride, bias,
                     (hipStream_t)hip_stream));
  return KLSTM_OK;
}
// split-K workspace of the stateless ops: one growing buffer per (device, stream), owned by the library
static klstm_status splitk_workspace(hipStream_t st, size_t floats, float **ws) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, std::pair<float *, size_t>> pool;
  int devid = 0;
  HIPCHK(hipGetDevice(&devid));
  std::lock_guard<std::mutex> lk(mu);
  auto &slot = pool[std::make_pair(devid, st)];
  if (slot.second < floats) {
    HIPCHK(hipStreamSynchronize(st));                // earlier launches may still read the old buffer
    if (slot.first) (void)hipFree(slot.first);
    slot.first = nullptr; slot.second = 0;
    HIPCHK(hipMalloc(&slot.first, floats * sizeof(float)));
    slot.second = floats;
  }
  *ws = slot.first;
  return KLSTM_OK;
}
klstm_status klstm_affine_backpropagate(const float *out_diff, int rows, int out_dim, int od_stride, const float *W,
                                        int in_dim, float *in_diff, int id_stride, void *hip_stream) {
  if (!out_diff || !W || !in_diff) return fail(KLSTM_ERR_ARG, "klstm_affine_backpropagate: null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  if (skinny_nn_supported(rows, in_dim, out_dim, out_diff, od_stride, W, in_dim, in_diff, id_stride)) {   // few frames, wide layer (klstm_fold.hip)
    float *ws = nullptr;
    klstm_status s = splitk_workspace(st, skinny_nn_workspace_floats(rows, in_dim, out_dim), &ws);
    if (s != KLSTM_OK) return s;
    HIPCHK(launch_skinny_nn(rows, in_dim, out_dim, out_diff, od_stride, W, in_dim, in_diff, id_stride, ws, st));
    return KLSTM_OK;
  }
  int klen = 0;
  const int ks = gemm_splitk_plan(rows, in_dim, out_dim, &klen);       // contraction over the (long) output axis
  if (ks > 1) {
    float *ws = nullptr;
    klstm_status s = splitk_workspace(st, (size_t)ks * rows * in_dim, &ws);
    if (s != KLSTM_OK) return s;
    HIPCHK(launch_gemm_splitk(false, false, rows, in_dim, out_dim, out_diff, od_stride, W, in_dim, 0.f, in_diff, id_stride,
                              nullptr, ws, ks, klen, st));
    return KLSTM_OK;
  }
  HIPCHK(launch_gemm(false, false, rows, in_dim, out_dim, out_diff, od_stride, W, in_dim, 0.f, in_diff, id_stride, nullptr, st));
  return KLSTM_OK;
}
klstm_status klstm_affine_update(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim,
                                 int out_dim, float *W, float *bias, float *W_corr, float *bias_corr, float lr,
                                 float lr_bias, float momentum, void *hip_stream) {
  if (!in || !out_diff || !W || !bias || !W_corr || !bias_corr) return fail(KLSTM_ERR_ARG, "klstm_affine_update: null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  if (outer_f16_supported(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, W_corr, in_dim, W, bias_corr)) {   // few frames, wide layer (klstm_outer.hip)
    if (reinterpret_cast<uintptr_t>(bias) & 15) {        // (the bias step rides along in 16-byte pieces)
      HIPCHK(launch_outer_f16(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, momentum, W_corr, in_dim, W, lr, momentum,
                              bias_corr, nullptr, 0.f, st));
      HIPCHK(launch_axpy(bias, bias_corr, -lr_bias, out_dim, st));
    } else {
      HIPCHK(launch_outer_f16(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, momentum, W_corr, in_dim, W, lr, momentum,
                              bias_corr, bias, lr_bias, st));
    }
    return KLSTM_OK;
  }
  if (in_dim % 4 == 0 && ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(W_corr)) & 15) == 0) {
    // gradient product, momentum and Update of the weight matrix in one pass (no second trip over the 3 x 34 MB)
    HIPCHK(launch_gemm_tn_update(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, momentum, W_corr, W, in_dim, lr, st));
  } else {
    HIPCHK(launch_gemm(true, false, out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, momentum, W_corr, in_dim, nullptr, st));
    HIPCHK(launch_axpy(W, W_corr, -lr, (long)out_dim * in_dim, st));
  }
  HIPCHK(launch_col_sum(out_diff, rows, out_dim, od_stride, momentum, bias_corr, st));
  HIPCHK(launch_axpy(bias, bias_corr, -lr_bias, out_dim, st));
  return KLSTM_OK;
}
klstm_status klstm_affine_gradient(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim,
                                   int out_dim, float *W_grad, float *bias_grad, void *hip_stream) {
  if (!in || !out_diff || !W_grad || !bias_grad) return fail(KLSTM_ERR_ARG, "klstm_affine_gradient: null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  if (outer_f16_supported(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, W_grad, in_dim, nullptr, bias_grad)) {
    HIPCHK(launch_outer_f16(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, 0.f, W_grad, in_dim, nullptr, 0.f, 0.f,
                            bias_grad, nullptr, 0.f, st));
    return KLSTM_OK;
  }
  if (in_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(W_grad) & 15) == 0)
    HIPCHK(launch_gemm_tn_coal(out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, 0.f, W_grad, in_dim, st));
  else
    HIPCHK(launch_gemm(true, false, out_dim, in_dim, rows, out_diff, od_stride, in, in_stride, 0.f, W_grad, in_dim, nullptr, st));
  HIPCHK(launch_col_sum(out_diff, rows, out_dim, od_stride, 0.f, bias_grad, st));
  return KLSTM_OK;
}
klstm_status klstm_pack_streams(const float *feats, int dim, int feat_stride, const int *stream_desc_dev, int num_stream, int T,
                                int shift, float *out, int out_stride, int *reset_dev, void *hip_stream) {
  if ((!feats || !stream_desc_dev || !out) && T > 0) return fail(KLSTM_ERR_ARG, "klstm_pack_streams: null argument");
  if (dim < 0 || num_stream <= 0 || T < 0 || feat_stride < dim || out_stride < dim)
    return fail(KLSTM_ERR_ARG, "klstm_pack_streams: bad size (dim %d, streams %d, T %d, strides %d / %d)", dim, num_stream, T, feat_stride, out_stride);
  if ((long)T * num_stream > 65535) return fail(KLSTM_ERR_SHAPE, "klstm_pack_streams: T * num_stream > 65535");
  if (T == 0 || dim == 0) return KLSTM_OK;
  HIPCHK(launch_pack_streams(feats, dim, feat_stride, stream_desc_dev, num_stream, T, shift, out, out_stride, reset_dev, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_reverse_streams(const float *in, int in_stride, int S, int T, int cols, const int *lens_dev, float *out, int out_stride,
                                   int mode, void *hip_stream) {
  if (mode < KLSTM_REVERSE_SET || mode > KLSTM_REVERSE_MASK_COPY) return fail(KLSTM_ERR_ARG, "klstm_reverse_streams: unknown mode %d", mode);
  const bool reads = mode != KLSTM_REVERSE_ZERO_PAD;
  if (S <= 0 || T < 0 || cols < 0) return fail(KLSTM_ERR_ARG, "klstm_reverse_streams: bad size (streams %d, T %d, cols %d)", S, T, cols);
  if ((long)T * S > INT_MAX) return fail(KLSTM_ERR_SHAPE, "klstm_reverse_streams: T * num_stream > INT_MAX");
  if (T == 0 || cols == 0) return KLSTM_OK;
  if (out_stride < cols || (reads && in_stride < cols))
    return fail(KLSTM_ERR_ARG, "klstm_reverse_streams: row stride below the column count (%d / %d < %d)", in_stride, out_stride, cols);
  if (!out || !lens_dev || (reads && !in)) return fail(KLSTM_ERR_ARG, "klstm_reverse_streams: null argument");
  if ((mode == KLSTM_REVERSE_SET || mode == KLSTM_REVERSE_ADD) && in == out)
    return fail(KLSTM_ERR_ARG, "klstm_reverse_streams: in == out (the reversal cannot run in place)");
  HIPCHK(launch_reverse_streams(in, in_stride, S, T, cols, lens_dev, out, out_stride, mode, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_log_softmax_scatter(const float *in, int rows, int cols, int in_stride, const int *dst_row_dev, float *out,
                                       int out_stride, int mode, const float *log_prior_dev, float prior_scale, void *hip_stream) {
  if ((!in || !dst_row_dev || !out) && rows > 0) return fail(KLSTM_ERR_ARG, "klstm_log_softmax_scatter: null argument");
  if (rows < 0 || cols <= 0 || in_stride < cols || out_stride < cols) return fail(KLSTM_ERR_ARG, "klstm_log_softmax_scatter: bad size");
  if (mode != KLSTM_SCORE_POSTERIOR && mode != KLSTM_SCORE_LOGPOST && mode != KLSTM_SCORE_LOGLIKE)
    return fail(KLSTM_ERR_ARG, "klstm_log_softmax_scatter: unknown mode %d", mode);
  if (mode == KLSTM_SCORE_LOGLIKE && !log_prior_dev) return fail(KLSTM_ERR_ARG, "klstm_log_softmax_scatter: log-likelihoods need log_prior");
  if (rows == 0) return KLSTM_OK;
  HIPCHK(launch_log_softmax_scatter(in, rows, cols, in_stride, dst_row_dev, out, out_stride, mode, log_prior_dev, prior_scale,
                                    (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_sgd_momentum_update(float *param, float *corr, const float *grad, long n, float momentum, float lr,
                                       void *hip_stream) {
  if (!param || !corr || !grad || n < 0) return fail(KLSTM_ERR_ARG, "klstm_sgd_momentum_update: bad argument");
  if (n == 0) return KLSTM_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(launch_sgd_momentum(param, corr, grad, momentum, lr, n, st));
  return KLSTM_OK;
}
klstm_status klstm_softmax(const float *in, int rows, int cols, int in_stride, float *out, int out_stride, void *hip_stream) {
  if (!in || !out) return fail(KLSTM_ERR_ARG, "klstm_softmax: null argument");
  if (rows > 0) HIPCHK(launch_softmax(in, rows, cols, in_stride, out, out_stride, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_xent_eval_masked(const float *net_out, int rows, int cols, int stride, const int *targets_dev,
                                    const float *mask_dev, float *diff, int diff_stride, float *row_xent_dev,
                                    float *row_correct_dev, void *hip_stream) {
  if (!net_out || !targets_dev || !mask_dev || !diff || !row_xent_dev || !row_correct_dev)
    return fail(KLSTM_ERR_ARG, "klstm_xent_eval_masked: null argument");
  if (rows > 0) HIPCHK(launch_xent(net_out, rows, cols, stride, targets_dev, mask_dev, diff, diff_stride, row_xent_dev,
                                   row_correct_dev, (hipStream_t)hip_stream));
  return KLSTM_OK;
}

// ticket word of the one-pass loss kernel (which workgroup is the last of a launch): one per (device, stream), zero between launches
static klstm_status loss_ticket(hipStream_t st, unsigned **ticket) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, unsigned *> pool;
  int devid = 0;
  HIPCHK(hipGetDevice(&devid));
  std::lock_guard<std::mutex> lk(mu);
  unsigned *&slot = pool[std::make_pair(devid, st)];
  if (!slot) {
    HIPCHK(hipMalloc(&slot, sizeof(unsigned)));
    HIPCHK(hipMemset(slot, 0, sizeof(unsigned)));       // (synchronous with respect to the host: done before any launch uses it)
  }
  *ticket = slot;
  return KLSTM_OK;
}
klstm_status klstm_softmax_xent_masked(const float *net_in, int rows, int cols, int in_stride, float *post, int post_stride,
                                       const int *targets_dev, const float *mask_dev, float *diff, int diff_stride, float *row_xent_dev,
                                       float *row_correct_dev, double *totals_dev, void *hip_stream) {
  if (!net_in || !targets_dev || !mask_dev || !diff || !row_xent_dev || !row_correct_dev)
    return fail(KLSTM_ERR_ARG, "klstm_softmax_xent_masked: null argument");
  if (rows <= 0) return KLSTM_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  unsigned *ticket = nullptr;
  if (totals_dev) {
    const klstm_status s = loss_ticket(st, &ticket);
    if (s != KLSTM_OK) return s;
  }
  const hipError_t e = launch_softmax_xent(net_in, rows, cols, in_stride, post, post_stride, targets_dev, mask_dev, diff, diff_stride,
                                           row_xent_dev, row_correct_dev, totals_dev, ticket, st);
  if (e == hipSuccess) return KLSTM_OK;
  if (e != hipErrorNotSupported) HIPCHK(e);
  // rows the one-pass kernel does not serve: the two kernels, through the caller's posterior matrix
  if (!post) return fail(KLSTM_ERR_ARG, "klstm_softmax_xent_masked: this shape needs the posterior matrix (post) as the buffer between its two kernels");
  HIPCHK(launch_softmax(net_in, rows, cols, in_stride, post, post_stride, st));
  HIPCHK(launch_xent(post, rows, cols, post_stride, targets_dev, mask_dev, diff, diff_stride, row_xent_dev, row_correct_dev, st));
  if (totals_dev) HIPCHK(launch_xent_accumulate(row_xent_dev, row_correct_dev, mask_dev, rows, totals_dev, st));
  return KLSTM_OK;
}

klstm_status klstm_xent_accumulate(const float *row_xent_dev, const float *row_correct_dev, const float *mask_dev, int rows,
                                   double *totals_dev, void *hip_stream) {
  if (!row_xent_dev || !row_correct_dev || !mask_dev || !totals_dev || rows < 0) return fail(KLSTM_ERR_ARG, "klstm_xent_accumulate: bad argument");
  if (rows > 0) HIPCHK(launch_xent_accumulate(row_xent_dev, row_correct_dev, mask_dev, rows, totals_dev, (hipStream_t)hip_stream));
  return KLSTM_OK;
}

klstm_status klstm_xent_eval_masked_post(const float *net_out, int rows, int cols, int stride, const int *post_offsets_dev,
                                         const int *post_pdf_dev, const float *post_weight_dev, const float *mask_dev, float *diff,
                                         int diff_stride, float *row_xent_dev, float *row_entropy_dev, float *row_correct_dev,
                                         void *hip_stream) {
  if (!net_out || !post_offsets_dev || !mask_dev || !diff || !row_xent_dev || !row_entropy_dev || !row_correct_dev)
    return fail(KLSTM_ERR_ARG, "klstm_xent_eval_masked_post: null argument");
  if (rows > 0) HIPCHK(launch_xent_post(net_out, rows, cols, stride, post_offsets_dev, post_pdf_dev, post_weight_dev, mask_dev, diff,
                                        diff_stride, row_xent_dev, row_entropy_dev, row_correct_dev, (hipStream_t)hip_stream));
  return KLSTM_OK;
}

}  // extern "C"

// ---- test support: hold compute units busy (uneven-load tests of the persistent chain) ----
namespace {
__global__ __launch_bounds__(1024) void k_occupy(long long ticks, unsigned *where) {
  extern __shared__ float hog[];                   // 96 KB: nothing else fits next to this workgroup
  hog[threadIdx.x] = (float)threadIdx.x;
  if (where && threadIdx.x == 0) {                   // which XCD / SE / CU this workgroup landed on (HW_REG_XCC_ID = 20, HW_REG_HW_ID = 4)
    unsigned xcc, hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    where[2 * blockIdx.x] = xcc; where[2 * blockIdx.x + 1] = hwid;
  }
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
  if (hog[threadIdx.x] < 0.f && where) where[0] = 1u;
}
}  // namespace

extern "C" klstm_status klstm_debug_occupy(int device, int workgroups, int microseconds, void *hip_stream, unsigned *where_dev) {
  if (workgroups <= 0 || microseconds <= 0) return fail(KLSTM_ERR_ARG, "klstm_debug_occupy: bad arguments");
  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (!st) {                                         // a stream of its own per device (streams belong to the device they were made on)
    static std::mutex mu;
    static std::map<int, hipStream_t> own;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t &o = own[device];
    if (!o) HIPCHK(hipStreamCreateWithFlags(&o, hipStreamNonBlocking));
    st = o;
  }
  HIPCHK(launch(k_occupy, dim3(workgroups), dim3(1024), 96 * 1024, st, LaunchProbe{}, (long long)microseconds * 100, where_dev));
  return KLSTM_OK;
}

// Test / probe support for klstm_gemm16.hip (tools/gemm16_probe.py, tests/test_gemm16_gpu.py): C = A B^T (+ bias) (+ add) for one or
// two products that share their K, bf16-rounded operands, fp32 accumulate, on hip_stream (NULL: the default stream).
//   mnk: 3 ints per job; ptrs: A, B, C, bias, add per job (device pointers, bias / add may be null); lds: lda, ldb, ldc, add_ld per job
//   force_nj / force_ks: 0 = the launcher's plan; plan_out (or null): nj, ks, output tiles of the plan that ran
extern "C" klstm_status klstm_debug_gemm_bf16_nt2(int njobs, const int *mnk, const float *const *ptrs, const int *lds, int force_nj, int force_ks,
                                                  void *hip_stream, int *plan_out) {
  return klstm_debug_gemm_bf16_nt2h(njobs, mnk, ptrs, lds, nullptr, force_nj, force_ks, hip_stream, plan_out);
}
extern "C" klstm_status klstm_debug_gemm_bf16_nt2h(int njobs, const int *mnk, const float *const *ptrs, const int *lds,
                                                   const unsigned short *const *copies, int force_nj, int force_ks, void *hip_stream, int *plan_out) {
  if (njobs == 0) { gemm_bf16_nt2_debug_buffer(reinterpret_cast<long long *>(const_cast<int *>(mnk))); return KLSTM_OK; }   // (probe: timing buffer on / off)
  if (njobs < 1 || njobs > 2 || !mnk || !ptrs || !lds) return fail(KLSTM_ERR_ARG, "klstm_debug_gemm_bf16_nt2: bad arguments");
  Nt2Job jobs[2];
  for (int q = 0; q < njobs; q++) {
    jobs[q] = Nt2Job{mnk[3 * q], mnk[3 * q + 1], mnk[3 * q + 2], ptrs[5 * q], lds[4 * q], ptrs[5 * q + 1], lds[4 * q + 1],
                     const_cast<float *>(ptrs[5 * q + 2]), lds[4 * q + 2], ptrs[5 * q + 3], ptrs[5 * q + 4], lds[4 * q + 3]};
    if (!gemm_bf16_nt2_supported(jobs[q])) return fail(KLSTM_ERR_SHAPE, "klstm_debug_gemm_bf16_nt2: job %d not supported by the kernel", q);
    if (copies) {
      jobs[q].Ah = copies[2 * q]; jobs[q].Bh = copies[2 * q + 1];
      if ((jobs[q].Ah || jobs[q].Bh) && !gemm_bf16_nt2_copies_usable(jobs[q]))
        return fail(KLSTM_ERR_SHAPE, "klstm_debug_gemm_bf16_nt2h: job %d: both bf16 copies, 16-byte aligned, leading dimensions %% 8 == 0", q);
    }
  }
  const Nt2Plan pl = gemm_bf16_nt2_plan(jobs, njobs, force_nj, force_ks);
  static std::mutex mu;
  static float *ws = nullptr; static size_t ws_floats = 0; static unsigned *tickets = nullptr;
  std::lock_guard<std::mutex> lk(mu);
  hipStream_t st = (hipStream_t)hip_stream;
  if (pl.ws_floats > ws_floats) {
    HIPCHK(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr; ws_floats = 0;
    HIPCHK(hipMalloc(&ws, pl.ws_floats * sizeof(float)));
    ws_floats = pl.ws_floats;
  }
  if (!tickets) {
    HIPCHK(hipMalloc(&tickets, NT2_TICKETS * sizeof(unsigned)));
    HIPCHK(hipMemset(tickets, 0, NT2_TICKETS * sizeof(unsigned)));
  }
  if (pl.nt > NT2_TICKETS) return fail(KLSTM_ERR_SHAPE, "klstm_debug_gemm_bf16_nt2: %d output tiles", pl.nt);
  HIPCHK(launch_gemm_bf16_nt2(jobs, njobs, pl, ws, ws_floats, tickets, NT2_TICKETS, st));
  if (plan_out) { plan_out[0] = pl.nj; plan_out[1] = pl.ks; plan_out[2] = pl.nt; }
  return KLSTM_OK;
}
