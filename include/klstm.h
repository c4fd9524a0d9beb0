/*
 * include/klstm.h -- C-ABI of the MI355X-native LstmProjectedStreams engine.
 *
 * This is the drop-in boundary for ONE path of dophist/kaldi-lstm: the multi-stream LSTMP
 * forward + truncated BPTT + SGD update of
 *     google/nnet/bd-nnet-lstm-projected-streams.h   (class LstmProjectedStreams)
 * It replaces, for that component only, the google/cudamatrix (CuMatrix + cuBLAS +
 * bd-cu-kernels.cu) layer the reference component calls into.  A Kaldi Component that
 * forwards its virtuals to these entry points is shown in INTEGRATION.md; the C++ mirror of
 * the reference class lives in include/klstm_component.hpp.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no exceptions cross this boundary.  Every call
 *     returns a klstm_status; klstm_last_error() gives the message of the calling thread's
 *     last failure (the adapter maps non-zero to KALDI_ERR, i.e. std::runtime_error, which is
 *     how the reference reports CU_SAFE_CALL failures, cu-matrix.cc:813).
 *   - all matrices are fp32 (Kaldi BaseFloat), row-major with an explicit row stride in
 *     ELEMENTS (CuMatrixBase::Stride(), cu-matrix.h:479-489: rows are pitched, always honour
 *     the stride).  Minibatch matrices are time-major: row = t*num_stream + s
 *     (bd-nnet-train-lstm-streams.cc:191-199; ...streams.h:263-272).
 *   - `in`, `out`, `out_diff`, `in_diff` are DEVICE pointers owned and pre-sized by the caller
 *     (Nnet owns them in Kaldi); the engine owns parameters, gradient/momentum buffers, the
 *     carried stream state and the activation slabs (...streams.h:577-620).
 *   - one engine = one GPU = one HIP stream; calls on one handle must be host-serialised
 *     (the reference is single-threaded, bd-nnet-train-lstm-streams.cc:93).  All calls are
 *     asynchronous on the engine's stream except the *_host copies and klstm_synchronize.
 *   - the flat parameter/gradient blob order is GetParams order (...streams.h:162-189):
 *       w_gifo_x [4C x I] | w_gifo_r [4C x R] | bias [4C] | peephole_i_c [C] |
 *       peephole_f_c [C] | peephole_o_c [C] | w_r_m [R x C]      (4C rows ordered g,i,f,o)
 */
#ifndef KLSTM_H_
#define KLSTM_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct klstm_engine klstm_engine;

typedef enum {
  KLSTM_OK = 0,
  KLSTM_ERR_ARG = 1,    /* bad argument (null pointer, negative size)                     */
  KLSTM_ERR_SHAPE = 2,  /* KALDI_ASSERT-class violation: rows % num_stream != 0 (:225),
                           reset flag count != num_stream (:214), bwd rows != fwd rows     */
  KLSTM_ERR_STATE = 3,  /* call order violated (backpropagate without propagate)           */
  KLSTM_ERR_HIP = 4,    /* a HIP runtime call failed                                       */
  KLSTM_ERR_NOGPU = 5   /* no usable gfx950 device: there is NO CPU fallback               */
} klstm_status;

/* flags for klstm_backpropagate */
#define KLSTM_BPTT_DEFAULT        0
/* data-parallel mode: leave the pure local gradient (beta = 0) in the gradient blob and do
 * NOT touch the momentum buffers; the caller all-reduces klstm_grad_blob() and then calls
 * klstm_apply_momentum().  (The reference folds momentum into the gradient GEMM's beta,
 * ...streams.h:465-487, which would multiply momentum by the number of ranks.) */
#define KLSTM_BPTT_DEFER_MOMENTUM 1
/* "klstm_update follows immediately, with the input rows unchanged": Kaldi's Component::Backpropagate runs
 * BackpropagateFnc and then Update on the same (input, out_diff) pair, so the gradient products (:468-487) may wait for
 * the learning rate and run as ONE pass together with the Update (:504-512): corr = momentum*corr + grad, theta -= lr*corr,
 * transposed copies refreshed -- one launch and 16 MB of HBM traffic less per minibatch.  Results are identical.  The
 * engine keeps the `in` pointer until then: any other call that observes or changes gradients, momentum buffers,
 * parameters or activations in between (get_corr, set_params, propagate, ...) first runs the gradient products the
 * ordinary way, so only a caller that overwrites the rows of `in` before klstm_update breaks the contract.
 * Ignored together with KLSTM_BPTT_DEFER_MOMENTUM. */
#define KLSTM_BPTT_FUSE_UPDATE    2

/* Message of the calling thread's most recent failing call ("" if none). */
const char *klstm_last_error(void);
/* Library / kernel-arch identification string, e.g. "klstm 0.4 gfx950 (...)". */
const char *klstm_version(void);
/* The host's bookkeeping of the value-only granule rings ("persist_gran", below), exported so that it can be checked without a device:
 * what value-only launch number `ordinal` (counting from 0) does at T frames, when the last user of the OTHER
 * ring wrote `last_other` slots and a ring has `slots` slots; cap = 0: the engine's cap.  out[0] = 1 value-only / 0 tagged (T + 2 above
 * the cap), out[1] = the ring it uses, out[2] = slots 1 .. out[2] of the other ring it writes the poison pattern into again, out[3] = the
 * slot count the rings must be re-allocated (and poisoned) at first, 0: none. */
void klstm_gran_plan(unsigned ordinal, int T, int last_other, int slots, int cap, int out[4]);

/* Replaces: LstmProjectedStreams(input_dim, output_dim) + <CellDim>/<NumStream> of
 * InitData/ReadData (...streams.h:27-33, :55-99, :101-131).  recur_dim == output_dim.
 * Parameters start at zero, momentum buffers and stream state at zero (kSetZero, :76-97).
 * device: HIP device ordinal.  hip_stream: a hipStream_t to run on (e.g. the caller
 * framework's current stream; must not be the legacy NULL stream, graphs cannot be captured
 * on it) or NULL to use the library's process-wide per-device BLOCKING stream: it is shared by
 * all engines created this way (stacked LSTM components stay ordered with each other) and is
 * implicitly ordered with the legacy default stream like everything else in a Kaldi process. */
klstm_status klstm_create(int input_dim, int cell_dim, int recur_dim, int num_stream,
                          int device, void *hip_stream, klstm_engine **out);
void klstm_destroy(klstm_engine *e);

/* dims / NumParams (...streams.h:152-160) */
int klstm_input_dim(const klstm_engine *e);
int klstm_cell_dim(const klstm_engine *e);
int klstm_recur_dim(const klstm_engine *e);
int klstm_num_stream(const klstm_engine *e);
long klstm_num_params(const klstm_engine *e);

/* Parameter / momentum / gradient blobs, flat GetParams order.  *_host variants take host
 * pointers and synchronise; the device variants are stream-ordered.
 * Replaces ReadData's tensor loads (:109-117), GetParams (:162-189) and the *_corr_ members
 * that InfoGradient inspects (:201-210). */
klstm_status klstm_set_params_host(klstm_engine *e, const float *flat);
klstm_status klstm_get_params_host(klstm_engine *e, float *flat);
klstm_status klstm_set_params_device(klstm_engine *e, const float *flat_dev);
klstm_status klstm_get_corr_host(klstm_engine *e, float *flat);   /* momentum buffers *_corr_ */
klstm_status klstm_set_corr_host(klstm_engine *e, const float *flat);
klstm_status klstm_get_grads_host(klstm_engine *e, float *flat);  /* pure gradient (DP mode) */
/* Device address of the contiguous gradient blob (num_params floats) for an in-place
 * all-reduce (RCCL ncclAllReduce / torch.distributed.all_reduce) in DP mode. */
float *klstm_grad_blob(klstm_engine *e);
/* Floats a collective over the engine's OWN gradient blob should cover: num_params rounded up to a multiple of 4, + 4.  The first of
 * the extra floats is the VALIDITY WORD of data-parallel runs: the gradient kernel writes 0 (this rank's gradient is real) or 1 (a
 * persistent launch of this minibatch gave up and the device-side guard stopped the gradient products); summed over the ranks together
 * with the gradient, it tells every rank's momentum / Update kernels after the all-reduce whether ANY rank's gradient was not real, and
 * then EVERY rank leaves that Update out -- replicas stay identical without a host wait in front of the collective
 * (klstm_allreduce_grads below).  A caller that runs its own all-reduce over num_params floats only (torch.distributed on
 * klstm_grad_blob()) does not get this: it sets "persist_verify" = 1 instead.  With a blob bound by klstm_bind_grad_blob: num_params. */
long klstm_grad_blob_len(const klstm_engine *e);
/* Use caller-owned device storage (num_params floats, 16-byte aligned) as this engine's gradient blob from now
 * on: a stacked net places the blobs of all its layers back to back in ONE buffer so that a minibatch needs one
 * all-reduce for the whole model.  NULL returns to the engine's own buffer. */
klstm_status klstm_bind_grad_blob(klstm_engine *e, float *grad_dev);
float *klstm_param_blob(klstm_engine *e);

/* Reset (...streams.h:212-220): for every s with flags[s] == 1 zero stream s's carried
 * state.  n must equal num_stream (KALDI_ASSERT :214 -> KLSTM_ERR_SHAPE). */
klstm_status klstm_reset(klstm_engine *e, const int *flags, int n);
/* Carried state of prev_nnet_state_ that is ever consumed: c [S x C] and r [S x R]
 * (only these column groups are read back, :275,:278,:281,:294). Host pointers. */
klstm_status klstm_get_state_host(klstm_engine *e, float *c, float *r);
klstm_status klstm_set_state_host(klstm_engine *e, const float *c, const float *r);

/* PropagateFnc (...streams.h:222-332).  in [rows x I], out [rows x R], device pointers,
 * strides in elements.  rows % num_stream must be 0 (:225).  Carries state in and out
 * (:231, :331). */
klstm_status klstm_propagate(klstm_engine *e, const float *in, int rows, int in_stride,
                             float *out, int out_stride);
/* Forward only (scoring, include/klstm_scorer.hpp): the same out rows and the same carried state as klstm_propagate,
 * bit for bit, but nothing is kept for a backward pass -- klstm_backpropagate answers KLSTM_ERR_STATE until the next
 * klstm_propagate.  Where the fp32 persistent chain runs one of the measured geometries (40/800/512 from 5 streams,
 * 512/800/512 up to 8) the launch leaves out every activation-plane store the BPTT would read; every other path (and a persistent
 * launch that gives up) runs the ordinary forward pass.  klstm_profile_query(e, "fwd_inference_launches") counts the former. */
klstm_status klstm_propagate_inference(klstm_engine *e, const float *in, int rows, int in_stride,
                                       float *out, int out_stride);

/* BackpropagateFnc (...streams.h:334-499) for the minibatch of the immediately preceding
 * klstm_propagate (it reuses that call's activation slab, :342-349; rows must match).
 * in_diff may be NULL (the reference always computes it, :457; NULL skips that GEMM).
 * momentum = opts_.momentum (:465).  flags: KLSTM_BPTT_*.
 * Default mode leaves  corr = momentum*corr + grad  in the momentum buffers (:468-487). */
klstm_status klstm_backpropagate(klstm_engine *e, const float *in, int in_stride,
                                 const float *out_diff, int out_diff_stride,
                                 float *in_diff, int in_diff_stride, int rows,
                                 float momentum, int flags);

/* The same two calls for HOST matrices (a Kaldi CuMatrix holds host memory when the process runs with
 * --use-gpu=no, cu-matrix.h:479-481; SURVEY 8(b) "data type at the boundary").  Rows are staged through
 * engine-owned device buffers with stream-ordered 2-D copies, the computation is the device path above (there is
 * no CPU path), and the call returns after out / in_diff have landed in host memory. */
klstm_status klstm_propagate_host(klstm_engine *e, const float *in_host, int rows, int in_stride,
                                  float *out_host, int out_stride);
klstm_status klstm_backpropagate_host(klstm_engine *e, const float *in_host, int in_stride,
                                      const float *out_diff_host, int out_diff_stride,
                                      float *in_diff_host, int in_diff_stride, int rows,
                                      float momentum, int flags);
/* 1 if p is device-accessible memory of the engine's GPU (hipMalloc / managed / registered host memory),
 * 0 if it is plain host memory, <0 on error: lets an adapter pick the right pair of calls once per matrix. */
int klstm_pointer_on_device(const klstm_engine *e, const void *p);

/* Data parallelism over utterance streams: every rank runs klstm_backpropagate(.., KLSTM_BPTT_DEFER_MOMENTUM),
 * then ONE in-place fp32 sum over the ranks of the gradient blob, then klstm_apply_momentum + klstm_update on every rank.
 *   klstm_allreduce_grads   ncclAllReduce(sum, fp32) of this engine's gradient blob (also a blob bound with
 *                           klstm_bind_grad_blob) over the ranks of `rccl_comm` (an ncclComm_t), enqueued on the engine's stream.
 *                           A rank whose persistent chain gave up in this minibatch must not hand its (missing) gradient to the
 *                           others: with the engine's own blob the validity word of klstm_grad_blob_len() rides along -- no host
 *                           wait; the minibatch is left out by every rank and counted (klstm_profile_query "dp_updates_left_out"),
 *                           and what the host has already heard of is answered (run again) before the collective is enqueued;
 *                           with "persist_verify" = 1 or a bound blob the call waits for the engine's stream and answers a
 *                           give-up first, so that every rank reduces a real gradient.
 *   klstm_allreduce_buffer  the same for any device buffer of n floats, e.g. the fused blob of a stacked net, on hip_stream
 *   klstm_comm_*            thin pass-throughs to ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy for callers without RCCL
 *                           headers: rank 0 obtains the 128-byte id and hands it to the other ranks by its own means (file,
 *                           MPI, the launcher's store), every rank then calls klstm_comm_init_rank (collective).
 * RCCL is resolved in the running process at the first of these calls (no link-time dependency of libklstm.so). */
#define KLSTM_COMM_ID_BYTES 128
klstm_status klstm_comm_get_unique_id(void *id128);
klstm_status klstm_comm_init_rank(int device, int nranks, int rank, const void *id128, void **comm);
klstm_status klstm_comm_destroy(void *comm);
klstm_status klstm_comm_count(void *comm, int *nranks);       /* ncclCommCount: how many ranks the communicator really spans */
klstm_status klstm_allreduce_grads(klstm_engine *e, void *rccl_comm);
klstm_status klstm_allreduce_buffer(float *buf_dev, size_t n, void *rccl_comm, void *hip_stream);

/* One-shot all-reduce over peer-mapped blobs (kaldi-lstm_amd/csrc/klstm_oneshot.hip).  PREPARED AND OFF: nothing in
 * the library calls it, and it has never run across devices (one-GPU lease) -- only as a 1-rank self-loop and between two
 * processes on one GPU.  Every rank: create (its own blob of n floats, hipMalloc memory), export two handles, hand them to every
 * peer by any means, connect with everybody's handles in rank order, then once per minibatch klstm_oneshot_allreduce (in place,
 * on hip_stream; all ranks, same order).  Sums are added in rank order by ONE rank per 1/N slice: bit-identical on all ranks.
 * Every wait is bounded (timeout_ms, default 2000); klstm_oneshot_status reads 0 or the phase that expired (after a stream
 * synchronisation). */
typedef struct klstm_oneshot klstm_oneshot;
typedef struct { unsigned char bytes[80]; } klstm_ipc_handle;     /* hipIpcMemHandle_t of the allocation + the blob's offset in it */
klstm_status klstm_oneshot_create(int device, float *blob_dev, long n, klstm_oneshot **out);
klstm_status klstm_oneshot_export(klstm_oneshot *g, klstm_ipc_handle *blob, klstm_ipc_handle *flags);
klstm_status klstm_oneshot_connect(klstm_oneshot *g, int rank, int nranks, const klstm_ipc_handle *blobs, const klstm_ipc_handle *flags);
klstm_status klstm_oneshot_allreduce(klstm_oneshot *g, void *hip_stream, int timeout_ms);
klstm_status klstm_oneshot_status(klstm_oneshot *g, unsigned *status);
klstm_status klstm_oneshot_destroy(klstm_oneshot *g);
const char *klstm_oneshot_last_error(void);
/* on the engine's stream, behind its gradient products; the group was created on klstm_grad_blob(engine) over klstm_grad_blob_len(engine)
 * floats (the validity word rides along, as in klstm_allreduce_grads) or over num_params floats (then the call waits and looks first) */
klstm_status klstm_allreduce_grads_oneshot(klstm_engine *e, klstm_oneshot *group, int timeout_ms);

/* DP mode only, after the all-reduce of klstm_grad_blob():  corr = momentum*corr + grad. */
klstm_status klstm_apply_momentum(klstm_engine *e, float momentum);

/* Update (...streams.h:501-512):  theta -= learn_rate * theta_corr  for all seven tensors.
 * clip_grad > 0 first clips every corr element to +-clip_grad IN PLACE, which is the
 * standard/ LstmProjected::Update behaviour (standard/nnet/nnet-lstm-projected.h:480-493,
 * max_grad = 50); pass 0 for the google/ component. */
klstm_status klstm_update(klstm_engine *e, float learn_rate, float clip_grad);

/* Block until everything queued on the engine's stream has finished. */
klstm_status klstm_synchronize(klstm_engine *e);

/* Test / diagnostics hook (the reference's DEBUG dumps, :314-324, :443-453): copy the
 * activation slab of the last propagate (which = 0) or backpropagate (which = 1) to host in
 * the REFERENCE layout [(T+2)*S rows] x [G|I|F|O|C|H|M|R], T = rows/S of that call.
 * Row-blocks the engine never materialises (the slab's dummy blocks) read as zero. */
klstm_status klstm_get_activations_host(klstm_engine *e, int which, float *dst);

/* Stateless helpers for the two trivial components the reference puts in front of the LSTM
 * (README.md:46-49).  Device pointers, strides in elements, enqueued on hip_stream (NULL = default).
 *   TimeShift::PropagateFnc (standard/nnet/nnet-time-shift.h:42-51): out[t] = in[clamp(t + shift, 0, rows-1)]
 *   TransmitComponent::PropagateFnc / BackpropagateFnc (standard/nnet/nnet-transmit-component.h:26-33):
 *   identity = shift 0. */
klstm_status klstm_time_shift(const float *in, int rows, int cols, int in_stride, float *out,
                              int out_stride, int shift, void *hip_stream);

/* Device memory helpers so that FFI users (the C++ mirror, ctypes) need no HIP headers.  The memcpy
 * calls synchronise hip_stream. */
klstm_status klstm_malloc(void **p, size_t bytes);
klstm_status klstm_free(void *p);
klstm_status klstm_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *hip_stream);
klstm_status klstm_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *hip_stream);
klstm_status klstm_memset_zero(void *dst_dev, size_t bytes, void *hip_stream);
klstm_status klstm_stream_synchronize(void *hip_stream);

/* Output tail of the nnet the trainer runs behind the LSTM (README.md:24-29): stateless ops on device
 * matrices, strides in elements.  The AffineTransform / Softmax classes themselves are NOT vendored in the
 * reference ([UPSTREAM] nnet-affine-transform.h, nnet-activation.h); only their use is (google/nnet.proto:4-5).
 *   affine_propagate     out = in * W^T + bias                (W is [out_dim x in_dim], Kaldi's linearity_)
 *   affine_backpropagate in_diff = out_diff * W
 *   affine_update        W_corr = momentum*W_corr + out_diff^T * in ; bias_corr = momentum*bias_corr + colsum(out_diff);
 *                        W -= lr * W_corr ; bias -= lr_bias * bias_corr
 *   softmax              per-row softmax
 *   xent_eval_masked     Xent::EvalMasked, google/nnet/nnet-loss.cc:76-142, for one-hot targets:
 *                        diff = (net_out - onehot(target)) * mask ; row_xent[r] = -mask*log(net_out[r][target]) ;
 *                        row_correct[r] = (mask == 1 && argmax(net_out[r]) == target).  The caller sums the two
 *                        per-row arrays on the host (the reference also copies scalars back, :110-141). */
klstm_status klstm_affine_propagate(const float *in, int rows, int in_dim, int in_stride, const float *W,
                                    const float *bias, float *out, int out_dim, int out_stride, void *hip_stream);
klstm_status klstm_affine_backpropagate(const float *out_diff, int rows, int out_dim, int od_stride,
                                        const float *W, int in_dim, float *in_diff, int id_stride, void *hip_stream);
klstm_status klstm_affine_update(const float *in, int in_stride, const float *out_diff, int od_stride, int rows,
                                 int in_dim, int out_dim, float *W, float *bias, float *W_corr, float *bias_corr,
                                 float lr, float lr_bias, float momentum, void *hip_stream);
/* data-parallel pieces of the same layer: the pure local gradient (no momentum, no update) into caller storage,
 * and the post-all-reduce step  corr = momentum*corr + grad ; param -= lr*corr  on any flat tensor */
klstm_status klstm_affine_gradient(const float *in, int in_stride, const float *out_diff, int od_stride, int rows,
                                   int in_dim, int out_dim, float *W_grad, float *bias_grad, void *hip_stream);
klstm_status klstm_sgd_momentum_update(float *param, float *corr, const float *grad, long n, float momentum, float lr,
                                       void *hip_stream);
klstm_status klstm_softmax(const float *in, int rows, int cols, int in_stride, float *out, int out_stride,
                           void *hip_stream);
klstm_status klstm_xent_eval_masked(const float *net_out, int rows, int cols, int stride, const int *targets_dev,
                                    const float *mask_dev, float *diff, int diff_stride, float *row_xent_dev,
                                    float *row_correct_dev, void *hip_stream);

/* Softmax followed by Xent::EvalMasked (one-hot targets) as ONE pass over the rows: the same arithmetic in the same order as
 * klstm_softmax + klstm_xent_eval_masked (bit-identical diff and statistics), without the trip of the posterior matrix
 * through memory.  post may be NULL (a training step only needs diff); if not NULL it receives the softmax output.
 * Rows the one-pass kernel does not serve (cols % 4 != 0, cols < 2048 or > 32768, unaligned rows) run the two kernels through
 * `post`, which must then be given (KLSTM_ERR_ARG otherwise).  totals_dev (may be NULL): three doubles on the device that the
 * statistics of this minibatch are added to, as klstm_xent_accumulate does, inside the same launch (the workgroup that
 * finishes last adds the rows up in a fixed order). */
klstm_status klstm_softmax_xent_masked(const float *net_in, int rows, int cols, int in_stride, float *post, int post_stride,
                                       const int *targets_dev, const float *mask_dev, float *diff, int diff_stride,
                                       float *row_xent_dev, float *row_correct_dev, double *totals_dev, void *hip_stream);

/* The three per-minibatch statistics of Xent::EvalMasked added onto device totals (the reference adds them to loss_, frames_,
 * correct_ on the host after copying the scalars back, google/nnet/nnet-loss.cc:110-142): totals_dev[0] += sum row_xent,
 * totals_dev[1] += sum row_correct, totals_dev[2] += sum mask, in double, fixed order, no synchronisation.  A trainer that
 * reports every N minibatches (bd-nnet-train-lstm-streams.cc:240-257) reads the three doubles once per report. */
klstm_status klstm_xent_accumulate(const float *row_xent_dev, const float *row_correct_dev, const float *mask_dev, int rows,
                                   double *totals_dev, void *hip_stream);

/* Xent::EvalMasked for GENERAL posteriors (google/nnet/nnet-loss.cc:76-142): frame r carries the entries
 * post_pdf/post_weight[post_offsets[r] .. post_offsets[r+1]) (CSR, device arrays; repeated pdfs of a frame add up like the
 * reference's `tgt(t, pdf) += weight`, :86-96).  diff = (net_out - target) * mask; per row: cross entropy -mask*sum t*log(y),
 * target entropy -mask*sum t*log(t + 1e-20), and 1 if mask == 1 and the arg-maxima of net_out and of the target row agree
 * (lowest index on ties, zeros of the dense target row included).  The dense rows x cols target matrix of the reference
 * (5.3 MB per minibatch at 80 x 16624, built on the host and copied) never exists.  A frame may carry any number of entries:
 * there is no limit (up to 256 are staged on chip; a longer frame costs more time, not correctness).  pdf range checks are the
 * caller's (the reference raises on the host while it builds the matrix, :89-92). */
klstm_status klstm_xent_eval_masked_post(const float *net_out, int rows, int cols, int stride, const int *post_offsets_dev,
                                         const int *post_pdf_dev, const float *post_weight_dev, const float *mask_dev, float *diff,
                                         int diff_stride, float *row_xent_dev, float *row_entropy_dev, float *row_correct_dev,
                                         void *hip_stream);

/* Batched scoring (include/klstm_scorer.hpp): many utterances packed into the S streams of one engine, forward only.
 * klstm_pack_streams  gathers one time-major chunk [T*S x dim] (row = t*S + s) from `feats`, the utterances' rows concatenated
 *   (row stride feat_stride).  stream_desc_dev: 3 ints per stream on the device, {row offset of the utterance in feats, its length,
 *   the frame the chunk starts at}; length <= 0 marks an idle stream (rows of zeros).  Row t of stream s is
 *   feats[off + clamp(start + t + shift, 0, len - 1)]: the TimeShift / targets delay applied to each utterance on its own
 *   (standard/nnet/nnet-time-shift.h:42-51), rows past the end repeat the last row like the trainer's padding
 *   (bd-nnet-train-lstm-streams.cc:198-201).  reset_dev (may be NULL): per stream 1 if the chunk starts its utterance (start == 0)
 *   or the stream is idle, else 0 -- the flags of klstm_reset for this chunk.
 * klstm_log_softmax_scatter  for each input row i of a chunk's Affine output with dst_row_dev[i] >= 0, writes row dst_row_dev[i] of
 *   `out` (dst_row_dev[i] < 0: a padding row, nothing is written):
 *     KLSTM_SCORE_POSTERIOR  softmax(a), the arithmetic of klstm_softmax (bit-identical to it);
 *     KLSTM_SCORE_LOGPOST    (a - max) - log(sum_j exp(a_j - max)), computed directly: it differs from log(klstm_softmax(a)) by the
 *                            rounding of the posterior (relative 6e-8 of a value near 1, far more in the tail where the posterior
 *                            underflows: the log form stays finite there, log of the Softmax output gives -inf);
 *     KLSTM_SCORE_LOGLIKE    the log-posterior - prior_scale * log_prior_dev[j] (a device vector of cols floats).  Turning Kaldi's
 *                            class-frame-counts into log priors is the caller's job; this is not claimed to match nnet-forward's
 *                            PdfPrior bit for bit.
 *   Rows of 2048..32768 columns (cols % 4 == 0, 16-byte aligned rows) are held in registers, one pass over memory; other shapes
 *   take three sweeps over the row. */
#define KLSTM_SCORE_POSTERIOR 0
#define KLSTM_SCORE_LOGPOST   1
#define KLSTM_SCORE_LOGLIKE   2
klstm_status klstm_pack_streams(const float *feats, int dim, int feat_stride, const int *stream_desc_dev, int num_stream, int T,
                                int shift, float *out, int out_stride, int *reset_dev, void *hip_stream);
klstm_status klstm_log_softmax_scatter(const float *in, int rows, int cols, int in_stride, const int *dst_row_dev, float *out,
                                       int out_stride, int mode, const float *log_prior_dev, float prior_scale, void *hip_stream);

/* The bidirectional layer (include/klstm_blstm.hpp): per-stream, length-aware time reversal of a time-major
 * block.  in / out [T*S x cols] (row t*S + s), device pointers, strides in elements (column windows such as `ptr + R` with stride 2R
 * are fine: rows need no alignment); lens_dev: S ints on the device, the length of the utterance in stream s, which starts at t = 0
 * (0 = idle stream; a value outside [0, T] is clamped to it).  Rows t >= lens[s] are padding.
 *   KLSTM_REVERSE_SET        t < len: out[t] = in[len-1-t]     padding rows: out = 0
 *   KLSTM_REVERSE_ADD        t < len: out[t] += in[len-1-t]    padding rows: untouched
 *   KLSTM_REVERSE_ZERO_PAD   t < len: untouched                padding rows: out = 0      (in is not read, may be NULL)
 *   KLSTM_REVERSE_MASK_COPY  t < len: out[t] = in[t]           padding rows: out = 0      (no reversal)
 * in and out must not overlap in the reversing modes (in == out is refused).  T == 0 or cols == 0: nothing to do.  Enqueued on
 * hip_stream (NULL = the legacy default stream). */
#define KLSTM_REVERSE_SET        0
#define KLSTM_REVERSE_ADD        1
#define KLSTM_REVERSE_ZERO_PAD   2
#define KLSTM_REVERSE_MASK_COPY  3
klstm_status klstm_reverse_streams(const float *in, int in_stride, int S, int T, int cols, const int *lens_dev, float *out, int out_stride,
                                   int mode, void *hip_stream);

/* Connectionist temporal classification over whole utterances (include/klstm_nnet.hpp class Ctc): the
 * sequence-level objective of a net that ends in <Softmax>, for label sequences without an alignment.  Stateless, asynchronous on
 * hip_stream, decided entirely on the device (no host round trip, no error return for a bad utterance).
 *   net_out [T*S x K]    posteriors as <Softmax> writes them, row t*S + s, row stride `stride` elements; read, never modified.
 *                        log y is taken as log(max(y, FLT_MIN))
 *   lens_dev [S]         frames of the utterance in stream s, which starts at t = 0 (the array of SetSeqLengths); 0 = idle stream
 *   labels_dev, label_offsets_dev [S+1]   CSR: the labels of stream s are labels_dev[off[s] .. off[s+1]), values in [0, K) except `blank`
 *   blank                the blank's index, any value in [0, K)
 *   diff [T*S x K]       the gradient with respect to the SOFTMAX INPUT, as Xent produces it (SoftmaxLayer passes it through):
 *                        diff(t,s,k) = y(t,s,k) - gamma(t,s,k), gamma = the posterior occupation of class k at frame t (sums to 1 over
 *                        k on a valid frame).  Rows t >= lens[s] are WRITTEN as zero.  Must not overlap net_out
 *   utt_loss_dev [S]     -log p(labels | x); 0 for an idle stream, +inf for a rejected one
 *   totals_dev           NULL, or four doubles on the device that this minibatch is ADDED to, streams in order: sum of the losses of
 *                        the utterances counted, utterances counted, utterances rejected, frames of the utterances counted
 *   workspace            klstm_ctc_workspace_bytes(T, S, max_label_len) bytes of device memory, 16-byte aligned: both chains' rows are
 *                        kept, 2 * T*S * (2 max_label_len + 1) floats (1.07 GB at T*S = 65535 with 1023 labels; 39 MB at T = 1000,
 *                        S = 16, 150 labels).  The label capacity (and with it the launch geometry) follows from workspace_bytes.
 * REJECTED (infeasible) utterances: lens[s] < L + (number of adjacent equal labels), a label outside [0, K) or equal to blank, lens[s]
 * outside [0, T], or more labels than the workspace was sized for.  Their diff rows are zero, their loss +inf, they count as rejected
 * and not in the loss sum.  An empty label sequence is feasible (all blank).
 * Bit-identical from run to run and independent of which stream an utterance sits in: no floating-point atomics; a class that appears
 * several times in a label sequence (and the blank) is summed in a fixed order.
 * Limits: S <= 32, T * S <= 65535, K <= 32768, max_label_len <= 1023; beyond them KLSTM_ERR_SHAPE and nothing is launched
 * (klstm_ctc_workspace_bytes answers 0 and leaves the message in klstm_last_error()). */
size_t klstm_ctc_workspace_bytes(int T, int S, int max_label_len);
klstm_status klstm_ctc_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                            const int *label_offsets_dev, int blank, float *diff, int diff_stride, float *utt_loss_dev,
                            double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* CTC best-path (greedy) decoding of whole utterances and the token error rate against reference label sequences (include/klstm_nnet.hpp
 * class CtcGreedyDecoder).  Stateless, asynchronous on hip_stream, decided entirely on the device.
 *   net_out [T*S x K]    posteriors, row t*S + s, row stride `stride` elements (any stride >= K, any 4-byte aligned start: a column window
 *                        is fine); read, never modified; columns beyond K are never touched
 *   lens_dev [S]         frames of the utterance in stream s, which starts at t = 0; 0 = idle stream
 *   blank                the blank's index, any value in [0, K)
 *   class_weight_dev     NULL, or K floats w: the winner of a frame is argmax_k key(y[k] * w[k]) with ONE fp32 multiply rounded to nearest
 *                        (label priors enter as w[k] = prior[k]^-alpha, computed by the caller); NULL = no multiply at all.
 *                        key(v) = v, or -inf where v is NaN (a NaN never wins); ties go to the LOWEST column; a row of all NaN gives 0
 *   hyp_dev [S*T]        the hypothesis of stream s at hyp_dev[s*T .. s*T + hyp_len_dev[s]): the classes of the frames t with
 *                        c(t) != blank and (t == 0 or c(t-1) != c(t)), in order.  Entries beyond hyp_len are left alone
 *   hyp_len_dev [S]      its length
 *   score_dev            NULL, or [S]: sum over the valid frames of log(max(y[t,s,best], FLT_MIN)) of the UNWEIGHTED posterior of the
 *                        winner (a NaN there counts as FLT_MIN), accumulated in double in a fixed order, stored as float
 *   frame_class_dev      NULL, or [T*S]: the winner of row t*S + s (the best-path alignment); -1 on padding rows (t >= lens[s]) and on
 *                        every row of an idle or rejected stream.  Those rows of net_out are NOT READ and may hold anything
 *   ref_labels_dev, ref_offsets_dev [S+1]   both NULL (no scoring), or the CSR pair klstm_ctc_eval takes
 *   errors_dev           NULL, or [S]: the Levenshtein distance (substitution, insertion, deletion cost 1 each) between the hypothesis
 *                        and the reference of stream s, exact; -1 where the stream is not counted.  Needs the references
 *   totals_dev           NULL, or five doubles on the device that this minibatch is ADDED to by one thread, streams in order (every term
 *                        is an integer): edit errors, reference tokens, hypothesis tokens, utterances counted, utterances with at least
 *                        one error.  Needs the references
 *   workspace            klstm_ctc_decode_workspace_bytes(T, S, max_ref_len) bytes of device memory, 16-byte aligned (8 bytes per row and
 *                        a few hundred more; the edit-distance row lives in registers, so max_ref_len is only checked against the limit).
 *                        One call at a time per workspace
 * STATUS of a stream: lens[s] == 0 idle, lens[s] outside [0, T] rejected: hyp_len 0, score 0, errors -1, not counted, frame_class -1.
 * A reference with a label outside [0, K) or equal to blank, or with more than 1023 labels: hypothesis and score as usual, errors -1,
 * not counted.  An empty reference is legal (errors = hyp_len).
 * Bit-identical from run to run and independent of which stream an utterance sits in: no floating-point atomics.
 * Limits: S <= 32, T * S <= 65535, 2 <= K <= 32768, max_ref_len <= 1023; beyond them KLSTM_ERR_SHAPE and nothing is launched
 * (klstm_ctc_decode_workspace_bytes answers 0 and leaves the message in klstm_last_error()). */
size_t klstm_ctc_decode_workspace_bytes(int T, int S, int max_ref_len);
klstm_status klstm_ctc_decode(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                              const float *class_weight_dev, int *hyp_dev, int *hyp_len_dev, float *score_dev, int *frame_class_dev,
                              const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev, double *totals_dev,
                              void *workspace, size_t workspace_bytes, void *hip_stream);

/* CTC prefix beam search of whole utterances: the most probable LABELLINGS (sums over alignments) as an n-best list with scores, and
 * their edit distances against reference label sequences (include/klstm_nnet.hpp class CtcBeamDecoder; DESIGN.md
 * 4k).  Stateless, asynchronous on hip_stream, decided entirely on the device.  net_out, stride, lens_dev, blank, class_weight_dev
 * and the references exactly as klstm_ctc_decode takes them.
 * THE SEARCH is defined bit for bit by tests/ctc_beam_ref.py.  Probabilities stay in the linear domain; every step is ONE fp32
 * product or sum rounded to nearest.  The emission e[k] = y[k] * w[k] (y[k] without weights); a NaN or a value below 2^-60 counts as
 * exactly 0, a value above 2^60 as 2^60.  Per frame: the `cands` non-blank classes with the largest e > 0 (ties: the lower column)
 * extend each of the at most `beam` prefixes; an extension that equals a prefix of the beam is added to that prefix's entry; the
 * `beam` largest totals pb + pnb survive (ties: the stay entries in beam order, then the extensions in order of parent and rank); the
 * beam is rescaled by the power of two that brings its largest total into [0.5, 1), values below 2^-60 become 0.  Two prefixes are
 * the same iff their lengths and their 64-bit hashes agree (h(empty) = KLSTM_CTC_HASH_START; H(h, c): x = (h ^ (c + 1)) *
 * KLSTM_CTC_HASH_MUL mod 2^64, x ^ (x >> 29); the two constants are defined below this comment).
 *   beam, cands, nbest   1 <= beam <= 64, 1 <= cands <= min(K - 1, 32), 1 <= nbest <= beam
 *   hyp_dev [S*N*T]      hypothesis q of stream s at hyp_dev[(s*N + q)*T .. + hyp_len_dev[s*N + q]), q < nbest_count_dev[s]: the first
 *                        N beam entries with a total > 0, best first.  Entries beyond hyp_len and list slots beyond nbest_count are
 *                        left alone
 *   hyp_len_dev [S*N], nbest_count_dev [S]
 *   score_dev            NULL, or [S*N]: log p of the hypothesis as the search summed it (a lower bound of log p(labels | y)):
 *                        float(log(double(total)) + exponent * ln 2)
 *   errors_dev           NULL, or [S*N]: the Levenshtein distance of every listed hypothesis to the reference of its stream; -1 in slots
 *                        beyond nbest_count and where the stream is not counted.  Needs the references
 *   totals_dev           NULL, or six doubles on the device that this minibatch is ADDED to by one thread, streams in order: 1-best edit
 *                        errors, reference tokens, 1-best hypothesis tokens, utterances counted, utterances with a 1-best error, oracle
 *                        errors (the minimum over the list).  Needs the references
 *   workspace            klstm_ctc_beam_workspace_bytes(T, S, beam, cands) bytes of device memory, 16-byte aligned: 8 bytes per row and
 *                        candidate, 8 bytes per frame and beam entry (the prefix tree) and about 1 KB.  One call at a time per workspace
 * STATUS of a stream: lens[s] == 0 idle, lens[s] outside [0, T] rejected: nbest_count 0, errors -1, not counted.  A DEAD utterance (a
 * frame in which every emission is 0) lists the first entry of its beam alone, with score -inf.  A reference with a label outside
 * [0, K) or equal to blank, or with more than 1023 labels: the list as usual, errors -1, not counted.  Rows t >= lens[s] and all rows of
 * idle / rejected streams are NOT READ.
 * Bit-identical from run to run and independent of which stream an utterance sits in: no floating-point atomics.
 * Limits: S <= 32, T * S <= 65535, 2 <= K <= 32768, beam <= 64, cands <= min(K - 1, 32), nbest <= beam; beyond them KLSTM_ERR_SHAPE
 * and nothing is launched (klstm_ctc_beam_workspace_bytes answers 0 and leaves the message in klstm_last_error()). */
#define KLSTM_CTC_HASH_START 0x243F6A8885A308D3ull      /* the hash of the empty sequence */
#define KLSTM_CTC_HASH_MUL   0x9E3779B97F4A7C15ull      /* the multiplier of one step */
size_t klstm_ctc_beam_workspace_bytes(int T, int S, int beam, int cands);
klstm_status klstm_ctc_beam_decode(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                   const float *class_weight_dev, int beam, int cands, int nbest, int *hyp_dev, int *hyp_len_dev,
                                   int *nbest_count_dev, float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev,
                                   int *errors_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* The same search with a LABEL LANGUAGE MODEL fused in (include/klstm_nnet.hpp class CtcLabelLm, CtcBeamDecoder::SetLanguageModel;
 * INTEGRATION.md 3h; the definition is tests/ctc_beam_lm_ref.py).  The LM is a dense deterministic weighted automaton
 * over the labels: state 0 is the start; from state q, label c leads to state lm_next_dev[q*K + c] and multiplies the probability
 * of the prefix by lm_weight_dev[q*K + c]; lm_final_dev[q] (may be NULL) multiplies a hypothesis that ends in q.  An n-gram model
 * (states = histories, weight = P(c | q)^alpha * e^beta folded on the host), a lexicon (a trie whose separator returns to the root,
 * weight 0 where no word continues, final 0 inside a word) and their composition are all tables of this form.
 *   the fused emission of extending a prefix in state q by candidate c:  f = flush(float32(e[c] * flush(weight[q][c]))), flush
 *   being the emission rule (NaN or below 2^-60: exactly 0, above 2^60: 2^60); f = 0 where next[q][c] lies outside [0, lm_states): a
 *   bad table entry is a forbidden extension, decided on the device, never a fault.  The extension is worth float32(p * f) wherever
 *   klstm_ctc_beam_decode has p * e[c]: merged into the entry of the same prefix, or as a new entry, whose state is next[q][c].
 *   Candidates are still chosen by the emission alone.  The blank's column of both tables is never read.
 *   with lm_final_dev: tf = float32(total * flush(final[state])); the list is the beam entries with tf > 0 by tf descending (ties: the
 *   earlier beam position), the first nbest.  None (also: every extension forbidden in some frame and the blank's emission 0): the
 *   utterance is DEAD as above.  Without it the list is klstm_ctc_beam_decode's.
 *   score_dev            the FUSED score, acoustic times language model as the search summed them: float(log(double(tf)) +
 *                        exponent * ln 2)
 * Everything else -- arguments, outputs, statuses, the workspace (klstm_ctc_beam_workspace_bytes, unchanged) -- as
 * klstm_ctc_beam_decode, which is this call without tables and returns the bits it always did.  Bit-identical from run to run,
 * independent of the stream an utterance sits in and of where the tables are read from: klstm_ctc_beam_lm_resident answers 1 where a
 * call of that shape stages the tables into LDS (8 bytes per entry) and 0 where it gathers them from global memory.
 * Limits: 1 <= lm_states, lm_states * K <= 2^24; beyond them KLSTM_ERR_SHAPE and nothing is launched.  A null lm_next_dev or
 * lm_weight_dev: KLSTM_ERR_ARG. */
klstm_status klstm_ctc_beam_decode_lm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                      const float *class_weight_dev, int beam, int cands, int nbest, int lm_states, const int *lm_next_dev,
                                      const float *lm_weight_dev, const float *lm_final_dev, int *hyp_dev, int *hyp_len_dev,
                                      int *nbest_count_dev, float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev,
                                      int *errors_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);
int klstm_ctc_beam_lm_resident(int lm_states, int K, int beam, int cands);

/* STREAMING CTC prefix beam search: the search of klstm_ctc_beam_decode / _lm fed chunk by chunk, with the beam carried across the
 * calls in device memory the caller owns (include/klstm_nnet.hpp class CtcStreamDecoder; include/klstm_scorer.hpp DecodeCtcStreaming;
 * INTEGRATION.md 3j; the definition is tests/ctc_beam_stream_ref.py).  The calls themselves are stateless and
 * asynchronous on hip_stream; everything is decided on the device.
 * klstm_ctc_beam_stream_step consumes lens_dev[s] frames of stream s from net_out (rows t * S + s, t < T; stride, blank,
 * class_weight_dev, beam, cands and the language-model tables as the whole-utterance calls take them; lm_states 0: no LM):
 *   lens_dev [S]         the frames of THIS chunk: 0 is idle (its state is not read, not written and not reset, even with start set),
 *                        a value outside [0, T] is rejected and treated as idle.  Rows t >= lens[s] are NOT READ
 *   start_dev            NULL (no stream starts), or [S]: nonzero begins a new utterance in stream s with this chunk.  State that no
 *                        step has ever started counts as started at its first non-idle step: zero-filled state is a valid "nothing yet"
 *   state                klstm_ctc_beam_stream_state_bytes(max_frames, S, beam) bytes, 16-byte aligned, zero-filled before the first
 *                        step, the SAME max_frames, S and beam in every call on it.  Per stream, 256-byte aligned: a header of 16
 *                        ints (started, frames consumed, beam entries, exponent, overflow flag), 64 beam entries (hash and parent
 *                        hash, node, last token, length, LM state, pb, pnb: 2.5 KB), then the prefix tree at 8 bytes per frame and
 *                        beam entry (parent and token of node 1 + frame * beam + slot; node 0 is the empty prefix)
 *   OVERFLOW             a stream with frames + lens[s] > max_frames is rejected for this call: its state is unchanged but for a
 *                        sticky flag in the header, which the next start clears.  Never a fault, never a partial write
 *   workspace            klstm_ctc_beam_stream_workspace_bytes(T, S, cands, nbest) bytes, 16-byte aligned: 1.5 KB and 8 bytes per row
 *                        and candidate.  One call at a time per workspace; step and emit may share it
 * klstm_ctc_beam_stream_emit writes the current n-best lists.  It modifies nothing in the state, so it may be called between any two
 * steps, any number of times.  hyp_dev / hyp_len_dev / nbest_count_dev / score_dev / the references / errors_dev / totals_dev as
 * klstm_ctc_beam_decode, with hyp_stride >= max_frames in the place of T:
 *   mode_dev [S]         0: skip (the list outputs of the stream are left alone, nbest_count 0); 1: the list without the LM's final
 *                        weights; 2: the list with them (lm_final_dev, may be NULL), ranked as klstm_ctc_beam_decode_lm ranks it.
 *                        Edit distances and totals cover the streams emitted with mode 2; every other stream has errors -1
 *   frames_dev           NULL, or [S]: frames consumed so far; -1 - frames once a step was rejected for overflow
 *   stable_len_dev       NULL, or [S] (modes 1 and 2): the length of the longest common prefix, token by token, of all beam entries
 *                        with a total > 0 (a DEAD beam: the first entry's length).  Every hypothesis the utterance can list from now
 *                        on begins with the first stable_len tokens of today's 1-best: they can no longer change
 *   workspace            at least klstm_ctc_beam_stream_workspace_bytes(1, S, 1, nbest) bytes
 * THE CONTRACT.  For any split of an utterance into chunks, and whatever the other streams do meanwhile, emit with mode 2 (mode 1:
 * without final weights) after the last frame writes what klstm_ctc_beam_decode / _lm write for the whole utterance with the same
 * parameters, and after n frames what that call writes for its first n frames: hypotheses, lengths, counts, the bits of the scores,
 * edit distances and the six totals.  A resumed search has no rounding of its own.
 * Limits: S <= 32 and T * S <= 65535 per call; K, beam, cands, nbest and the LM as the whole-utterance calls; 1 <= max_frames,
 * max_frames * beam + 1 < 2^31, hyp_stride >= max_frames; beyond them KLSTM_ERR_SHAPE and nothing is launched (the size queries
 * answer 0 and leave the message in klstm_last_error()).  Null required pointers, a state or a workspace that is too small or
 * misaligned: KLSTM_ERR_ARG. */
size_t klstm_ctc_beam_stream_state_bytes(int max_frames, int S, int beam);
size_t klstm_ctc_beam_stream_workspace_bytes(int T, int S, int cands, int nbest);
klstm_status klstm_ctc_beam_stream_step(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *start_dev,
                                        int blank, const float *class_weight_dev, int beam, int cands, int lm_states,
                                        const int *lm_next_dev, const float *lm_weight_dev, void *state, size_t state_bytes, int max_frames,
                                        void *workspace, size_t workspace_bytes, void *hip_stream);
klstm_status klstm_ctc_beam_stream_emit(int S, int K, int blank, int beam, int nbest, const int *mode_dev, int lm_states,
                                        const float *lm_final_dev, const void *state, size_t state_bytes, int max_frames, int *hyp_dev,
                                        int hyp_stride, int *hyp_len_dev, int *nbest_count_dev, float *score_dev, int *frames_dev,
                                        int *stable_len_dev, const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev,
                                        double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* The same searches with a SPARSE BACK-OFF language model: a high-order n-gram over characters or word pieces, which the dense tables
 * cannot hold (include/klstm_nnet.hpp class CtcSparseLabelLm, ReadArpaLabelLm; the definition of a
 * lookup is sparse_lm_lookup of kaldi-lstm_amd/lm.py).  The model is a deterministic automaton with back-off (failure) arcs over the K
 * classes, state 0 the start, its arcs in CSR form, all arrays on the device:
 *   arc_offsets_dev [states + 1]; arc_labels_dev [arcs], strictly ascending within a state, never the blank; arc_next_dev [arcs];
 *   arc_weight_dev [arcs]; backoff_dev [states], the state to fall back to or -1; backoff_weight_dev [states].  Every back-off chain
 *   ends (-1) after at most 8 back-offs: n-grams up to order 9.
 * THE LOOKUP (q, c) -> (g, n): if state q has an arc for c, n is its next and g its weight -- after a back-off, float32(product *
 * weight).  Otherwise, with backoff[q] < 0: g = 0, n = -1 (forbidden); else product = flush(float32(product * flush(backoff_weight[q]))),
 * q = backoff[q], and again; the product starts at 1, flush is the emission rule.  (g, n) then stand where weight[q][c] and next[q][c] of
 * klstm_ctc_beam_decode_lm stand, and everything after them is that call's: the results are, bit for bit, those of the dense call on
 * the expansion of the model.  An n outside [0, states) forbids the extension.
 * klstm_ctc_slm_build turns the arrays into an opaque blob of klstm_ctc_slm_bytes(states, arcs, K) bytes (16-byte aligned, about 16
 * bytes per state and 44 per arc; the arrays may be freed once the build has run), once per model, asynchronously on hip_stream.  It
 * VALIDATES on the device, so that no content of the arrays can lead a search out of the blob, and counts into status_dev [8] (may be
 * NULL): states DROPPED (they lose all arcs and keep their back-off) for [0] labels not strictly ascending, [1] a label outside
 * [0, K), [2] a blank arc, [3] an arc range outside [0, arcs]; back-offs CUT to -1 for [4] a target outside [-1, states), [5] a chain
 * of more than 8 back-offs, cycles included (decided for every state on the arrays as given); [6] states stored as a direct row of K
 * entries (those with at least K / 4 arcs), the others by their sorted labels; [7] 0.  For a state with several faults the first arc
 * at fault decides, in the order [3], then per arc [1], [2], [0].
 * klstm_ctc_beam_decode_slm / klstm_ctc_beam_stream_step_slm are klstm_ctc_beam_decode_lm / klstm_ctc_beam_stream_step with (slm,
 * slm_bytes, lm_states, lm_final_dev [lm_states] or NULL) in the place of the tables: the same arguments, checks, statuses, asynchrony,
 * workspace and state.  klstm_ctc_beam_stream_emit serves both kinds of model: it reads lm_final_dev alone (with a sparse model pass
 * lm_states = 1).  The blob is known by its address: one that klstm_ctc_slm_build did not write, or wrote for other states or
 * classes, or slm_bytes below klstm_ctc_slm_bytes: KLSTM_ERR_ARG, as for a null slm.
 * Limits: 1 <= states <= 2^24, 1 <= arcs <= 2^26, 2 <= K <= 32768; beyond them KLSTM_ERR_SHAPE (klstm_ctc_slm_bytes answers 0). */
size_t klstm_ctc_slm_bytes(int states, int arcs, int K);
klstm_status klstm_ctc_slm_build(int states, int arcs, int K, int blank, const int *arc_offsets_dev, const int *arc_labels_dev,
                                 const int *arc_next_dev, const float *arc_weight_dev, const int *backoff_dev, const float *backoff_weight_dev,
                                 void *slm, size_t slm_bytes, int *status_dev, void *hip_stream);
klstm_status klstm_ctc_beam_decode_slm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                       const float *class_weight_dev, int beam, int cands, int nbest, const void *slm, size_t slm_bytes,
                                       int lm_states, const float *lm_final_dev, int *hyp_dev, int *hyp_len_dev, int *nbest_count_dev,
                                       float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev,
                                       double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);
klstm_status klstm_ctc_beam_stream_step_slm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *start_dev,
                                            int blank, const float *class_weight_dev, int beam, int cands, const void *slm, size_t slm_bytes,
                                            int lm_states, void *state, size_t state_bytes, int max_frames, void *workspace,
                                            size_t workspace_bytes, void *hip_stream);

/* Minimum expected token error over CTC n-best lists (MWER / minimum Bayes risk over n-best; include/klstm_nnet.hpp class CtcMbr;
 * INTEGRATION.md 3i): the sequence-discriminative objective that follows CTC training, on the lists and edit distances
 * klstm_ctc_beam_decode wrote.  Stateless, asynchronous on hip_stream, decided entirely on the device.  net_out, stride, lens_dev,
 * blank, diff and diff_stride exactly as klstm_ctc_eval takes them.  For stream s, over its listed entries q < nbest_count[s]:
 *   l_q = log p(h_q | y)      what klstm_ctc_eval returns as -utt_loss for the labels h_q (the same chain, the same bits), kept in double
 *   P_q = softmax_q(risk_scale * l_q)   in double, q ascending, over the entries that are not dropped
 *   R   = sum_q P_q W_q       the expected errors, W_q = errors_dev[s*N + q]
 *   diff(t,k) = risk_scale * sum_q P_q (W_q - R) gamma_q(t,k) + ctc_weight * (y(t,k) - gamma_ref(t,k))
 * the gradient of R + ctc_weight * (-log p(ref | y)) with respect to the SOFTMAX INPUT; gamma_q = the per-frame occupation of h_q.
 * The coefficient risk_scale * P_q (W_q - R) is rounded to float once; the row is accumulated in fp32, q ascending, the reference last.
 *   hyp_dev, hyp_stride, hyp_len_dev [S*N], nbest_count_dev [S], errors_dev [S*N], list_n = N
 *                        the arrays of klstm_ctc_beam_decode, unchanged (hyp_stride = T there): labelling q of stream s at
 *                        hyp_dev[(s*N + q)*hyp_stride .. + hyp_len].  Slots q >= nbest_count[s] are NOT READ
 *   ref_labels_dev, ref_offsets_dev [S+1]   the CSR pair klstm_ctc_eval takes; both NULL if and only if ctc_weight == 0
 *   risk_scale, ctc_weight   finite, risk_scale > 0, ctc_weight >= 0
 *   risk_dev [S]         R as float; 0 for an idle stream, -1 for a rejected or skipped one
 *   hyp_logp_dev         NULL, or [S*N]: float(l_q); -inf for a dropped or unlisted entry and on streams that are not counted
 *   hyp_post_dev         NULL, or [S*N]: float(P_q); 0 there
 *   ref_loss_dev         NULL, or [S]: -log p(ref | y) with the bits of klstm_ctc_eval's utt_loss on a counted stream when ctc_weight > 0,
 *                        0 otherwise
 *   totals_dev           NULL, or six doubles that this minibatch is ADDED to, streams in order: sum of R, sum of the cost of entry 0,
 *                        utterances counted, utterances rejected or skipped, frames counted, sum of the reference losses
 *   workspace            klstm_ctc_mbr_workspace_bytes(T, S, list_n, max_len, with_ref) bytes, 16-byte aligned: both chains' rows of
 *                        EVERY entry, 2 * T*S * (list_n + with_ref) * (2 max_len + 1) floats (350 MB at T = 1000, S = 16, 8 entries and
 *                        the reference, 150 labels), 128 KB per stream for the class map and the per-entry links.  The label capacity
 *                        (and with it the launch geometry) follows from workspace_bytes.  One call at a time per workspace
 * An ENTRY IS DROPPED (no contribution) when its length is outside [0, capacity] or above hyp_stride, a label is outside [0, K) or
 * equals blank, or lens[s] < length + (adjacent equal labels).  An empty labelling is legal.
 * STATUS of a stream: lens[s] == 0 idle.  REJECTED: lens[s] outside [0, T], nbest_count[s] outside [0, N], or ctc_weight > 0 and the
 * reference is one klstm_ctc_eval rejects.  SKIPPED: nbest_count[s] == 0, a listed cost < 0, or every entry dropped.  All of them
 * get zero diff rows and hyp_post 0; padding rows (t >= lens[s]) are written as zero; those rows of net_out are NOT READ.
 * Bit-identical from run to run and independent of which stream an utterance sits in: no floating-point atomics.
 * Limits: S <= 32, T * S <= 65535, 2 <= K <= 32768, 1 <= list_n <= 16, max_len <= 1023, hyp_stride >= 1; beyond them KLSTM_ERR_SHAPE /
 * KLSTM_ERR_ARG and nothing is launched (klstm_ctc_mbr_workspace_bytes answers 0 and leaves the message in klstm_last_error()). */
size_t klstm_ctc_mbr_workspace_bytes(int T, int S, int list_n, int max_len, int with_ref);
klstm_status klstm_ctc_mbr_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank, const int *hyp_dev,
                                int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const int *errors_dev, int list_n,
                                const int *ref_labels_dev, const int *ref_offsets_dev, float risk_scale, float ctc_weight, float *diff,
                                int diff_stride, float *risk_dev, float *hyp_logp_dev, float *hyp_post_dev, float *ref_loss_dev,
                                double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* Minimum Bayes risk decoding and token / word confidences over CTC n-best lists (include/klstm_nnet.hpp class CtcConsensus;
 * INTEGRATION.md 3m): the decode-time counterpart of klstm_ctc_mbr_eval, Kaldi's lattice-mbr-decode in n-best form.
 * Stateless, asynchronous on hip_stream, decided entirely on the device; nothing is read back.  For stream s, over its LIVE entries:
 *   units        separator < 0: the tokens of an entry.  separator >= 0: its words, the maximal runs of tokens other than the separator
 *                (leading, trailing and repeated separators make no empty words).  Two words are equal iff their 64-bit keys are: the
 *                hash the beam search knows its prefixes by, h <- x ^ (x >> 29) with x = (h ^ (token + 1)) * KLSTM_CTC_HASH_MUL,
 *                folded over the word's tokens from h = KLSTM_CTC_HASH_START
 *   P_q          exp(z_q - max z) / Z with z_q = (double)scale * (double)logp_q and Z summed q ascending, in double
 *   D[q][r]      the Levenshtein distance between the unit sequences of entries q and r
 *   R_q          sum_r P_r D[q][r], r ascending, in double: the expected unit errors of answering with entry q
 *   map, mbr     argmax z and argmin R, ties to the lowest q; pick = pivot_mode ? mbr : map
 *   conf_u       sum_r P_r [unit u of the pick is matched against entry r], r ascending, in double.  Matched: in the full table over
 *                the pick's units (i) and entry r's (j), walk from the far corner -- the diagonal if D[i][j] = D[i-1][j-1] + (a_i != b_j),
 *                else up (i - 1) if D[i][j] = D[i-1][j] + 1, else left -- and unit i is matched iff it is left by a diagonal step with
 *                a_i = b_j.  The pick is matched against itself throughout, so conf_u >= P_pick
 *   hyp_dev, hyp_stride, hyp_len_dev [S*N], nbest_count_dev [S], list_n = N    the arrays of klstm_ctc_beam_decode, unchanged.  Slots
 *                        q >= nbest_count[s] are NOT READ
 *   logp_dev [S*N]       natural logarithms: the search's score_dev, or hyp_logp_dev of klstm_ctc_mbr_eval
 *   errors_dev           NULL, or [S*N] as the search wrote them with references (totals 8 and 9 only)
 *   max_len              the unit and token capacity, <= 1023
 *   scale                finite, > 0
 *   pick_dev, map_dev, mbr_dev [S]   -1 on a stream that is idle or rejected
 *   post_dev [S*N]       float(P_q); 0 for a dropped or unlisted entry
 *   risk_dev [S*N]       float(R_q); -1 there
 *   unit_len_dev [S*N]   the number of units; 0 there
 *   conf_dev, conf_stride    float(conf_u) at conf_dev[s*conf_stride + u] for the units of the pick; nothing else is written.
 *                        conf_stride >= min(hyp_stride, max_len)
 *   dist_dev             NULL, or [S*N*N]: D, exact and symmetric; -1 where either entry is dropped or unlisted
 *   totals_dev           NULL, or ten doubles that this minibatch is ADDED to, streams in order: streams done, streams idle or rejected,
 *                        sum of R[pick], sum of R[map], streams with mbr != map, sum of the picks' units, sum of conf over them, entries
 *                        dropped, sum of errors[pick], sum of errors[map] (the last two 0 without errors_dev)
 *   workspace            klstm_ctc_consensus_workspace_bytes(S, list_n, max_len, separator >= 0) bytes, 16-byte aligned: per entry 24
 *                        bytes, 4 N bytes of distances, max_len bytes of matches, in word mode 8 max_len bytes of keys, and for
 *                        max_len > 255 (where a table of back-pointers no longer fits LDS) 256 max_len bytes of table.  One call at a
 *                        time per workspace
 * AN ENTRY q < nbest_count[s] IS LIVE iff logp is finite, 0 <= hyp_len <= min(hyp_stride, max_len) and no token is negative; every
 * other one is dropped and counted.  STATUS of a stream: REJECTED with nbest_count[s] outside [0, N]; IDLE with a count of 0 or no
 * live entry; done otherwise.
 * Bit-identical from run to run: no floating-point atomics, every sum in index order.
 * Limits: 1 <= S <= 32, 1 <= list_n <= 64, 0 <= max_len <= 1023; beyond them KLSTM_ERR_SHAPE and nothing is launched
 * (klstm_ctc_consensus_workspace_bytes answers 0 and leaves the message in klstm_last_error(); neither touches a device then).  A
 * workspace below the size query, a null or misaligned pointer, a bad scale, pivot_mode or stride: KLSTM_ERR_ARG. */
size_t klstm_ctc_consensus_workspace_bytes(int S, int list_n, int max_len, int word_mode);
klstm_status klstm_ctc_consensus(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                                 const int *errors_dev, int S, int list_n, int max_len, float scale, int separator, int pivot_mode,
                                 int *pick_dev, int *map_dev, int *mbr_dev, float *post_dev, float *risk_dev, int *unit_len_dev,
                                 float *conf_dev, int conf_stride, int *dist_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                                 void *hip_stream);

/* Second-pass rescoring of CTC n-best lists with token and word back-off language models (include/klstm_nnet.hpp class CtcRescorer;
 * Python ctc_nbest_rescore; the definition is tests/ctc_rescore_ref.py): the stage between
 * klstm_ctc_beam_decode* and klstm_ctc_consensus -- re-rank the list with a model too large, or of the wrong kind, to fuse into the
 * search.  Stateless, asynchronous on hip_stream, decided entirely on the device; nothing is read back.  Both models are blobs of
 * klstm_ctc_slm_build, known by their addresses.  For stream s, over its entries q < nbest_count[s]:
 *   WELL FORMED      logp finite, 0 <= hyp_len <= min(hyp_stride, max_len), every token in [0, K).  Every other listed entry is
 *                    DROPPED and counted; tokens are range-checked before any lookup
 *   units            num_words = 0: the tokens.  num_words > 0: the words, the maximal runs of tokens other than `separator` (leading,
 *                    trailing and repeated separators make no empty word), known by the 64-bit key klstm_ctc_consensus knows them by
 *   word table       word_keys_dev [num_words] ascending, word_ids_dev [num_words]: the class of a word in the word model.  The key k is
 *                    looked up by lo = 0, hi = W; while lo < hi: mid = (lo + hi) >> 1, key[mid] < k ? lo = mid + 1 : hi = mid; a hit
 *                    iff lo < W and key[lo] = k.  A word is OUT OF VOCABULARY on a miss, on a class outside [0, add_classes) and on
 *                    the class add_reserved (the `blank` the word model was built with); it takes unk_id, and with unk_id < 0 it
 *                    FORBIDS the entry.  An unsorted table can only produce misses
 *   logw(model)      from state 0 and (m, e) = (1.0, 0), per unit u: (g, next) = the model's lookup (sparse_lm_lookup of lm.py, bit for
 *                    bit), gf = flush(g) (NaN or below 2^-60: 0, above 2^60: 2^60); gf = 0 or next outside [0, states) FORBIDS the
 *                    entry; else (m, de) = frexp(m * (double)gf), e += de, state = next.  With final weights flush(final[state])
 *                    enters the same way after the last unit.  logw = log(m) + (double)e * 0.6931471805599453
 *   sub              NULL, or a model over the K tokens: the one the first pass fused; its logw is taken OUT of logp
 *   add              NULL, or a model over the K tokens (num_words = 0, add_classes = K) or over the words (add_classes = V <= 32768
 *                    classes, one of them reserved: a word vocabulary holds at most 32767 words)
 *   z_q              (double)am_scale * (double)logp_q - logw_sub + (double)add_scale * logw_add + (double)unit_bonus * units_q,
 *                    left to right, one IEEE double operation each; an absent model contributes nothing
 *   ranking          the entries neither dropped nor forbidden, by z descending, ties to the lower q
 *   hyp_dev, hyp_stride, hyp_len_dev [S*N], nbest_count_dev [S], logp_dev [S*N], errors_dev (NULL ok), list_n = N
 *                        the arrays of klstm_ctc_beam_decode as klstm_ctc_consensus takes them.  Slots q >= nbest_count[s] are NOT READ
 *   order_dev [S*N]      the entry of rank r; -1 from live_count[s] on, and everywhere on an idle or rejected stream
 *   live_count_dev [S]   the entries ranked
 *   score_dev [S*N]      float(z_q); -inf for a dropped, forbidden or unlisted entry
 *   add_logp_dev, sub_logp_dev   NULL, or [S*N]: float(logw), 0 for an absent model, -inf where the model forbids and for a dropped or
 *                        unlisted entry
 *   units_dev, oov_dev   NULL, or [S*N] ints: the units of the entry and how many of its words are out of vocabulary (0 for a dropped
 *                        or unlisted entry)
 *   out_n                0, or 1 <= out_n <= N: the first min(live, out_n) entries of the ranking are written in the layout
 *                        klstm_ctc_consensus and klstm_ctc_mbr_eval read -- out_hyp_dev [S*out_n*out_stride] (the tokens, copied),
 *                        out_len_dev, out_score_dev = float(z), out_errors_dev (NULL ok; -1 without errors_dev) [S*out_n], out_count_dev
 *                        [S]; slots beyond the count are left alone.  out_stride >= min(hyp_stride, max_len)
 *   totals_dev           NULL, or eight doubles that this minibatch is ADDED to, streams in order: streams done, streams idle or
 *                        rejected, entries dropped, entries forbidden, streams whose 1-best changed, sum of errors of the first pass's
 *                        entry 0, sum of errors of the new 1-best (both over the done streams, 0 without errors_dev; the first is
 *                        errors[s*N] whatever became of entry 0: it is read even where that entry was dropped or forbidden), words
 *                        out of vocabulary
 *   workspace            klstm_ctc_rescore_workspace_bytes(S, list_n, max_len, num_words > 0) bytes, 16-byte aligned.  One call at a
 *                        time per workspace
 * STATUS of a stream: REJECTED with nbest_count[s] outside [0, N]; IDLE with a count of 0 or no rankable entry; done otherwise.
 * Bit-identical from run to run: no floating-point atomics.
 * Limits: 1 <= S <= 32, 1 <= list_n <= 64, 0 <= max_len <= 1023, 2 <= K <= 32768, 0 <= num_words <= 2^24, 0 <= out_n <= list_n; beyond
 * them KLSTM_ERR_SHAPE and nothing is launched (klstm_ctc_rescore_workspace_bytes answers 0 and leaves the message in
 * klstm_last_error(); neither touches a device then).  A null required pointer, a small or misaligned workspace, a non-finite scale,
 * neither model given, word arguments without `add`, a separator outside [0, K), an unk_id or add_reserved that is no class of the word
 * model, a model that was not built at its address or for other sizes: KLSTM_ERR_ARG with the outputs untouched.
 * The same lists rescored with an LSTM language model: the entries of klstm_nlm.h, a family of their own in this library. */
size_t klstm_ctc_rescore_workspace_bytes(int S, int list_n, int max_len, int word_mode);
klstm_status klstm_ctc_nbest_rescore(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                                     const int *errors_dev, int S, int list_n, int max_len, int K, const void *sub_slm, size_t sub_bytes,
                                     int sub_states, const float *sub_final_dev, const void *add_slm, size_t add_bytes, int add_states,
                                     int add_classes, const float *add_final_dev, const unsigned long long *word_keys_dev,
                                     const int *word_ids_dev, int num_words, int unk_id, int separator, int add_reserved, float am_scale,
                                     float add_scale, float unit_bonus, int *order_dev, int *live_count_dev, float *score_dev,
                                     float *add_logp_dev, float *sub_logp_dev, int *units_dev, int *oov_dev, int out_n, int *out_hyp_dev,
                                     int out_stride, int *out_len_dev, int *out_count_dev, float *out_score_dev, int *out_errors_dev,
                                     double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* MMI (CTC-CRF) training against a label language model (include/klstm_nnet.hpp class CtcMmi): the
 * posterior of the reference under the automaton the beam search multiplies in (klstm_ctc_beam_decode_lm's tables), with the normaliser
 * summed exactly over EVERY labelling the automaton accepts.  Stateless apart from the note below, asynchronous on hip_stream, decided
 * entirely on the device.  net_out, stride, lens_dev, labels_dev / label_offsets_dev, blank, diff and diff_stride exactly as
 * klstm_ctc_eval takes them.  With y = max(net_out, FLT_MIN) (a NaN counts as FLT_MIN) and W(l) = the product of the weights of l's arcs
 * from state 0 times final of the state it ends in (0 if an arc is absent):
 *   num  = p_ctc(ref | y)      what klstm_ctc_eval returns as -utt_loss (the same chain, the same bits), kept in double
 *   Z    = sum over all frame paths pi of W(collapse(pi)) * prod_t y(t, pi_t)
 *   loss = -log num - log W(ref) + log Z                                       >= 0
 *   diff(t,k) = gamma_den(t,k) - gamma_ref(t,k) + ctc_weight * (y(t,k) - gamma_ref(t,k))
 * the gradient with respect to the SOFTMAX INPUT; gamma_den(t,k): the posterior under the denominator that frame t emits class k.
 * An arc (q, k) is ABSENT when k == blank, weight[q*K + k] is not > 0, or next[q*K + k] is outside [0, lm_states).  final NULL: all ones;
 * a final weight that is not > 0 counts as 0.
 * THE GRAPH is built once per language model by klstm_ctc_mmi_graph_build into a caller-owned device buffer of
 * klstm_ctc_mmi_graph_bytes(lm_states, K) bytes (16-byte aligned; about 56 bytes per table cell) and serves every call after it on
 * the same or a later-ordered stream: the validated arcs, the denominator states they reach ((LM state, class of the last frame)
 * pairs), every state's incoming arcs in ascending source state.  The tables are not needed after the build.  The library remembers
 * per ADDRESS what the last build there was for (states, K, blank); klstm_ctc_mmi_eval returns KLSTM_ERR_ARG for an address nothing
 * was built at and for a graph built for other values.  A graph is not to be copied to another address.
 *   ctc_weight           finite, >= 0
 *   loss_dev [S]         the loss as float; 0 for an idle stream, +inf for a rejected one
 *   num_logp_dev         NULL, or [S]: float(log num), bit for bit -utt_loss of klstm_ctc_eval; 0 on streams that are not counted
 *   den_logz_dev         NULL, or [S]: float(log Z); 0 there
 *   lm_logw_dev          NULL, or [S]: float(log W(ref)); 0 there
 *   totals_dev           NULL, or five doubles that this minibatch is ADDED to, streams in order: sum of loss, utterances counted,
 *                        utterances rejected, frames counted, sum of -num_logp
 *   workspace            klstm_ctc_mmi_workspace_bytes(T, S, K, lm_states, max_label_len) bytes, 16-byte aligned: the reference's rows as
 *                        klstm_ctc_eval keeps them and 2 * T*S * lm_states*K floats for the denominator's (sized for the densest
 *                        automaton; the rows written are as long as the graph has states: 2 lm_states for an n-gram model).  The
 *                        label capacity (and with it the reference chain's launch geometry, which changes no bit) follows from
 *                        workspace_bytes.  One call at a time per workspace
 * STATUS of a stream: lens[s] == 0 idle.  REJECTED: whatever klstm_ctc_eval rejects, and a reference with W(ref) = 0.  An empty
 * reference is legal where final[0] > 0.  Idle and rejected streams get zero diff rows; padding rows (t >= lens[s]) are written as
 * zero; those rows of net_out are NOT READ.
 * NUMBERS.  The denominator runs in the log domain in float32, every frame's row taken relative to its own maximum; the maxima are
 * summed in double.  No term of either recursion is formed by a subtraction ("all of a state's mass but one class" is summed without
 * that class).  gamma_den and gamma_ref are normalised per frame in double.
 * Bit-identical from run to run and independent of which stream an utterance sits in: no floating-point atomics.
 * Limits: S <= 32, T * S <= 65535, K >= 2, lm_states >= 1, lm_states * K <= 16384, max_label_len <= 1023; beyond them KLSTM_ERR_SHAPE
 * and nothing is launched (the size queries answer 0 and leave the message in klstm_last_error()). */
size_t klstm_ctc_mmi_graph_bytes(int lm_states, int K);
klstm_status klstm_ctc_mmi_graph_build(int lm_states, int K, int blank, const int *lm_next_dev, const float *lm_weight_dev,
                                       const float *lm_final_dev, void *graph, size_t graph_bytes, void *hip_stream);
size_t klstm_ctc_mmi_workspace_bytes(int T, int S, int K, int lm_states, int max_label_len);
klstm_status klstm_ctc_mmi_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                                const int *label_offsets_dev, int blank, const void *graph, size_t graph_bytes, int lm_states,
                                float ctc_weight, float *diff, int diff_stride, float *loss_dev, float *num_logp_dev,
                                float *den_logz_dev, float *lm_logw_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                                void *hip_stream);

/* CTC forced alignment (Viterbi) of whole utterances: the single most probable alignment of the label sequence of stream s to its
 * frames (include/klstm_nnet.hpp class CtcAligner).  Stateless, asynchronous on hip_stream, decided
 * entirely on the device.  net_out, lens_dev, labels_dev / label_offsets_dev and blank exactly as klstm_ctc_eval takes them (row
 * t*S + s, any row stride >= K, any 4-byte aligned start: a column window is fine; read, never modified).
 * THE PATH.  Lattice states 0 .. 2L (even: blank, odd i: label i >> 1); start in state 0 or 1, end in 2L or 2L - 1, per frame stay,
 * advance by one, or skip a blank onto a label that differs from the label before it.  The emission of a frame is
 * log(max(y[class], FLT_MIN)), a NaN counts as FLT_MIN.  The path with the largest sum of emissions wins; among equal predecessors
 * stay is preferred, then advance, then skip; at the end state 2L over 2L - 1.  The sums run in float32.
 *   class_weight_dev     NULL, or K floats w: the emission becomes log(max(y[k] * w[k], FLT_MIN)) with ONE fp32 multiply (label priors
 *                        enter as w[k] = prior[k]^-alpha, computed by the caller); the score stays that of the unweighted posterior
 *   frame_class_dev [T*S]   the class of frame (t, s) on the path (blank or a label); -1 on padding rows (t >= lens[s]) and on every
 *                        row of an idle or rejected stream: comparable with klstm_ctc_decode's frame_class element by element
 *   frame_pos_dev        NULL, or [T*S]: the label position j in [0, L) the frame belongs to; -1 on a blank frame and wherever
 *                        frame_class is -1
 *   token_begin_dev, token_end_dev   both NULL, or parallel to labels_dev: the first frame of token j and one past its last frame
 *                        (end > begin for every token of an aligned utterance); -1 for idle and rejected streams
 *   score_dev            NULL, or [S]: the sum of the UNWEIGHTED emissions along the returned path, accumulated in double in a fixed
 *                        order, stored as float; 0 for an idle stream, -inf for a rejected one
 *   totals_dev           NULL, or five doubles on the device that this minibatch is ADDED to by one thread, streams in order: sum of the
 *                        scores of the utterances aligned, utterances aligned, utterances rejected, frames, blank frames
 *   workspace            klstm_ctc_align_workspace_bytes(T, S, max_label_len) bytes of device memory, 16-byte aligned: two bits per
 *                        lattice state and frame (8 bytes per 32 states; 75 KB per stream at T = 1000 with 150 labels, 33 MB at
 *                        T*S = 65535 with 1023) and 512 bytes.  The label capacity (and with it the launch geometry) follows from
 *                        workspace_bytes.  One call at a time per workspace
 * STATUS of a stream, as klstm_ctc_eval decides it: lens[s] == 0 idle; REJECTED when lens[s] is outside [0, T], lens[s] < L + (number
 * of adjacent equal labels), a label is outside [0, K) or equal to blank, or there are more labels than the workspace was sized
 * for.  An empty label sequence is feasible (all blank).  Rows t >= lens[s] and all rows of idle / rejected streams are NOT READ.
 * Bit-identical from run to run and independent of which stream an utterance sits in and of its neighbours: no floating-point atomics.
 * Limits: S <= 32, T * S <= 65535, 2 <= K <= 32768, max_label_len <= 1023; beyond them KLSTM_ERR_SHAPE and nothing is launched
 * (klstm_ctc_align_workspace_bytes answers 0 and leaves the message in klstm_last_error()). */
size_t klstm_ctc_align_workspace_bytes(int T, int S, int max_label_len);
klstm_status klstm_ctc_align(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                             const int *label_offsets_dev, int blank, const float *class_weight_dev, int *frame_class_dev,
                             int *frame_pos_dev, int *token_begin_dev, int *token_end_dev, float *score_dev, double *totals_dev,
                             void *workspace, size_t workspace_bytes, void *hip_stream);

/* Engine knobs (not part of the reference interface).  Keys:
 *   "graph"   0/1/2  issue plain stream launches (default 0: measured equal or faster at every stream count while the host
 *                  thread keeps ahead, and indifferent to callers that hand in fresh buffers every minibatch) or replay the
 *                  per-call launch sequence from a hipGraph keyed on the caller's pointers (a busy host thread: 40-80
 *                  launches per call on the launch-per-step chains).  1: a graph per call unless the call is one or
 *                  two launches anyway (persistent chain); 2: always
 *   "fold"    -1/0/1  folded recurrence W_rm = W_gifo_r * W_r_m: one kernel per step and direction instead of two
 *                  (DESIGN.md 4a); -1 = auto (NumStream <= 8 and >= 12 frames per stream), 1 = whenever NumStream <=
 *                  16 and I, C, R are multiples of 8.  Same results up to fp32 summation order.
 *   "persist" -1/0/1/2  weights-resident persistent chain for NumStream <= 8: ONE launch per direction runs
 *                  all T steps with the folded operands held in registers and the per-step all-to-all done inside the
 *                  launch.  0 = off, 1 = forward launch only, 2 = both directions whenever the shape allows, -1 = auto (both
 *                  directions from 8 frames per stream).  Same results up to fp32 summation order.  Needs one compute unit
 *                  per workgroup (C/4 backward, C/4 or C/8 forward): an engine on a device (partition) with fewer compute
 *                  units keeps to one launch per step, and klstm_last_error() says so when the option asked for it.
 *                  Every in-kernel wait is bounded.  A launch that GIVES UP (its workgroups were not all resident: another
 *                  process holds part of the chip) records its ordinal and a status word; on the device, every persistent
 *                  launch and every gradient / momentum / Update kernel queued behind it sees the word and does nothing, and
 *                  the carried state the minibatch started from is intact (double-buffered).  The first call that looks
 *                  (propagate / backpropagate / update / reset poll a host-mapped word without a synchronisation;
 *                  klstm_synchronize, the getters and klstm_allreduce_grads read the device words) answers it WITHOUT an
 *                  error: the calls of the CURRENT minibatch -- since the last klstm_propagate / klstm_reset began -- are run
 *                  again on the launch-per-step chain with the arguments they came with (bit-identical to an engine that never
 *                  used the persistent chain), so `in`, `out_diff` and the output buffers of a minibatch must stay the
 *                  caller-provided, unchanged buffers until the next klstm_propagate / klstm_reset on the engine (Kaldi's
 *                  Nnet keeps them exactly that long).  A minibatch older than that cannot be run again: it is DROPPED -- no
 *                  Update, no state advance -- and counted.  `persist_cooldown` minibatches (default 64) on the launch-per-step
 *                  chain follow, then the persistent chain is tried again; a give-up that follows a re-arm closely doubles the
 *                  cool-down (up to 65536 minibatches), a clean run as long as the last cool-down resets it.  klstm_last_error() carries a remark;
 *                  klstm_profile_query(e, "persist_giveups" | "persist_replayed" | "persist_dropped" | "persist_launches" |
 *                  "dp_updates_left_out", ..) returns the counts in *launches (no "profile" option needed).
 *                  "persist_verify" 0/1: 1 = klstm_propagate / klstm_backpropagate wait for their persistent launch, so a
 *                  give-up is answered INSIDE the call, before the caller (or a neighbouring component) has read `out` /
 *                  `in_diff`: fully transparent, at the price of one host wait per call (~6 us of launch gap each; Kaldi
 *                  synchronises per minibatch anyway: the C++ mirror turns it on).  0 (default of the C-ABI): asynchronous, as above.
 *                  The wait is a spin on a host-mapped word the last workgroup of the launch writes (launch count + give-up bit),
 *                  not a stream synchronisation ("persist_verify_spin" 0: hipStreamSynchronize instead; A-B runs).
 *                  With KLSTM_BPTT_FUSE_UPDATE ("klstm_update follows immediately") the wait of klstm_backpropagate happens at the
 *                  END OF THAT klstm_update instead: gradient products + Update (guarded: they do nothing behind a give-up) are
 *                  enqueued while the BPTT launch runs, `in_diff` is valid when klstm_update has returned -- Kaldi's
 *                  Component::Backpropagate returns only then.  (A promised klstm_update that never comes: the next
 *                  klstm_propagate / synchronising call waits and answers.)
 *                  "persist_epoch" 1/0: where a persistent launch takes the epoch of its granule tags and its launch ordinal from.
 *                  Both advance by a fixed amount with every launch the engine enqueues (run, skipped or given up alike), so the
 *                  engine mirrors the device words on the host.  1 (default): a launch that goes straight to the stream (not into
 *                  a graph of the "graph" option) gets both as kernel arguments; one lane of workgroup 0 writes the words' next
 *                  values with fire-and-forget stores, and the workgroups simply exit -- no arrival count, no last-workgroup chain of
 *                  device-scope round trips, no done word -- unless the host waits on that word ("persist_verify" = 1: count and
 *                  report stay).  0: every launch reads the device words at its head and its last workgroup moves them on (what
 *                  captured launches and the bf16 many-stream launches always do).  Bit-identical results; the device words
 *                  hold the same values either way (klstm_profile_query "persist_word_epoch_fwd" | "persist_word_epoch_bwd" |
 *                  "persist_word_launches" read them back), so the setting may change at any minibatch boundary.  A-B runs and tests.
 *                  "persist_gran" 1/0: what the in-launch exchange of the fp32 forward chain carries at 1..4 streams.  0: {tag, value}
 *                  granules of 8 bytes.  1 (default): VALUE-ONLY granules -- the 16 bytes of a cell's four stream values; a dword is
 *                  fresh when it differs from a signalling-NaN pattern the slot held before (no multiply or add returns one, and a
 *                  value with exactly those bits would leave as the canonical quiet NaN).  One slot per step in one of two rings;
 *                  every launch hands the other ring's used slots back as that pattern; the rings grow with the frames per
 *                  minibatch (up to 254: longer minibatches keep the tags).  Launches captured into a graph of the "graph"
 *                  option, "persist_verify" = 1, 5..16 streams and the backward chain keep the tags; the two transports own
 *                  separate buffers, so the setting may change at any minibatch boundary.  Bit-identical results.
 *                  klstm_profile_query(e, "gran_value_launches", ..) counts the launches that exchanged value-only granules.
 *                  Not supported: a hipGraph captured by the CALLER around engine calls that take the persistent chain (the
 *                  engine cannot count launches inside a foreign graph): use "persist" = 0 there.
 *                  Per-engine knobs (A-B experiments and tests): "persist_waves" (forward and backward geometry: 8, 12, 16),
 *                  "persist_xl" (bf16, 9..32 streams, 1024 cells: 1 = the forward launch as one chain per XCD, the default; 0 = one
 *                  copy of the weights over all CUs), "persist_xl_bwd" (the same for the BPTT chain; 0 = one launch per step),
 *                  "persist_bwd_waves" (12, 16), "persist_bwd_interleave" (5..8 streams: 1 = the two stream groups of the backward
 *                  launch as interleaved chains, the default; 0 = one after the other; bit-identical results),
 *                  "persist_tpw", "persist_nap0", "persist_nap", "persist_nap0_bwd",
 *                  "persist_spin_us" (bound of a single in-kernel wait, default 50 000), "persist_ncu" (pretend CU count),
 *                  "persist_test_stall_fwd" / "persist_test_stall_bwd" (workgroup 0 withholds its publish of that step:
 *                  forces the give-up path)
 *   "fold_bf16x3"  0/1/2  the fold product W_rm = W_gifo_r * W_r_m of THIS engine on the 16-bit matrix cores at fp32 accuracy
 *                  (every partial product exact in fp32, fp32 accumulation): 2 (default) = two fp16 planes per
 *                  operand, three products, dropped terms ~7e-7 relative; 1 = three bf16 planes, six products, dropped terms
 *                  below 2^-24; 0 = the fp32 MFMA kernel.  RANGE: identical to the reference's fp32 products in every mode -- in
 *                  mode 2 a parameter at or beyond 65520 (the fp16 range) is noticed by the product itself (range guard, below),
 *                  the affected tiles are recomputed in fp32 and the engine moves to mode 1 by itself.  Parameters below 2^-14
 *                  carry an absolute error of 2^-36 (not a relative one of 2^-22): nothing for a weight matrix whose largest
 *                  entries are above 1e-4.  "fold_direct" 0: the generic tile kernel (process-wide)
 *   "direct_nt_shape", "outer_f16", "skinny_f16", "skinny_f16_pair"  the three products of a WIDE AffineTransform at few frames
 *                  (the output layer of a small-minibatch step) run on the f16 matrix cores at fp32 accuracy:
 *                  both operands split into two fp16 numbers on the fly (x = h1 + h2 / 2048), three products with fp32
 *                  accumulation, the dropped term ~2^-22 relative; measured error against float64 at or below the fp32 MFMA
 *                  kernels'.  RANGE GUARD: the numeric range is the reference's (fp32).  Upper side: an operand at or beyond
 *                  65520 becomes Inf in its first plane and every accumulator it meets Inf / NaN -- never a finite wrong
 *                  number; each wave looks at its accumulators after its K loop, recomputes its outputs in plain fp32 when it
 *                  finds one, and counts the event in a host-mapped word; the launcher reads the word before every launch and
 *                  keeps that product on its fp32 kernel from then on (klstm_profile_query(e, "fp16_redo" | "fp16_redo_nt" |
 *                  "fp16_redo_outer" | "fp16_redo_skinny" | "fp16_redo_fold", ..) returns the counts in *launches).  Lower side:
 *                  DERIVATIVE operands are scaled by a power of two before the split and the result scaled back (exact): every
 *                  column of out_diff by its own in klstm_affine_gradient / _update, out_diff / dgifo by 2^12 in
 *                  klstm_affine_backpropagate and the BPTT tail -- entries of 1e-7 (late training) keep fp32 accuracy (22 bits
 *                  down to 2^-26, an absolute error below 2^-47 under that; derivatives of 16 and more take the guard's path).
 *                  klstm_affine_propagate of <= 80 rows into > 8192 columns: "direct_nt_shape" 99 = the same layout on the fp32
 *                  MFMA, 0 = the register-direct fp32 kernel, 10*NI + waves = geometry of that kernel, 97 = the f16 x 2 product with the
 *                  input rows resident in registers and K cut into four quarters (round 6: measured, not faster at 80 rows);
 *                  klstm_affine_gradient / klstm_affine_update of <= 96 rows and >= 2048 outputs: "outer_f16" 0 = fp32 tiles;
 *                  klstm_affine_backpropagate of <= 80 rows over >= 4096 outputs: "skinny_f16" 0 = fp32 MFMA;
 *                  d_r / in_diff of an engine whose input is too wide for the persistent backward launch: "skinny_f16_pair" 0 =
 *                  the tiled split-K kernel.  All process-wide (A-B experiments and tests)
 *   "fp16_products"  0/1  0 = no product of THIS engine and no stateless klstm_affine_* call on this engine's device runs on fp16 planes
                  (all of the above on their fp32 kernels, the fold product on three bf16 planes): saves a net whose activations,
                  weights or derivatives pass 65504 all the time the slow call of the range guard.  1 = the defaults again, the
                  guards' counters and cool-downs cleared.  Other engines keep their own state.
                  RANGE GUARD STATE: every engine has its own (event words, which families are latched, cool-downs); the stateless
                  klstm_affine_* calls share one per device.  A family whose guard fired runs on its fp32-range kernel for a
                  cool-down (64 fold products = Updates; 2048 looks of a stateless family), then the fp16 planes are tried again; a
                  trigger that follows a re-arm closely doubles the cool-down (up to 2^20), a clean run as long as the last cool-down
                  resets it; klstm_last_error() carries a remark when a family latches and when it comes back.
                  klstm_profile_query(e, "fp16_redo*") = this engine's events + its device's stateless events; "fp16_redo_own" =
                  this engine's only; "fold_mode" = the fold product's format as it runs (1 while latched)
 *   "persist_tail"  0/1/2  d_r / in_diff inside the persistent backward launch (1, default) or as batched products after it (0).
 *                  Inside: on TAIL WORKGROUPS of the same launch where the device has compute units to spare next to the chain's
 *                  C / 4 (they read the chain's exchange without being waited for: the chain runs at its bare pace), else --
 *                  or with 2 -- on the chain's own workgroups (rounds 3-5).  Same contraction order either way: bit-identical results.
 *                  klstm_profile_query(e, "persist_tail_wgs") = tail workgroups of the last backward launch (0: none).
 *   "bf16"    0/1/2  bf16 operands (weights, staged activations, gradient products from 256 frames on) with fp32
 *                  accumulate, fp32 masters (the reference is fp32 only).  Needs I, C, R multiples of 8.
 *                  1 = where it pays: from 9 streams on; an engine of up to 8 streams keeps its fp32 weights-resident chain (faster
 *                  there, and exact; remark in klstm_last_error()).  2 = bf16 operands at any stream count.
 *   "tail_merge"  0/1  1 = the reduction of the tail workgroups' partial d_r / in_diff rows runs on the first workgroups of the gradient
 *                  launch behind the BPTT launch instead of in a launch of its own (k_tail_reduce).  With KLSTM_BPTT_FUSE_UPDATE that launch is
 *                  klstm_update's: `in_diff` is then complete when klstm_update's launches are (klstm_synchronize in between runs it
 *                  at once).  Bit-identical; measured SLOWER (146.0 -> 148.1 us per minibatch at 40/800/512 x 4): default 0, kept for A-B runs.
 *                  klstm_profile_query "tail_merge_launches", "tail_merge_timeouts" (must stay 0).
 *   "fuse_update"  0/1  0 = KLSTM_BPTT_FUSE_UPDATE is ignored: gradient products and Update as separate passes (A-B runs; this engine)
 *   "gemm_copies"  0/1/2  bf16 mode, 9..32 streams with the per-XCD BPTT chain: that chain writes a bf16 copy of its dgifo rows, the Update
 *                  kernels bf16 copies of W_gifo_r^T / W_gifo_x^T, and the batched d_r + in_diff product reads THE COPIES by LDS-DMA
 *                  (1, default; 0: it rounds the fp32 operands while staging them -- the same roundings, twice the bytes).  With 1 the
 *                  Update also leaves the fp32 W_gifo_r^T / W_gifo_x^T out while those chains run (nothing reads them then; whoever
 *                  does -- a launch-per-step chain after a give-up or "persist" = 0, k_pack, the fp32-operand product -- gets them
 *                  transposed from the parameters first); 2 = copies AND fp32 matrices on every Update (A-B runs, tests).  The copies
 *                  are used from the first minibatch after an Update on (klstm_set_params refreshes only the fp32 matrices);
 *                  klstm_profile_query(e, "gemm_copies_launches") counts the launches that read them.  "gemm_copies_plan" = 16 nj + ks
 *                  forces tile width (32 nj columns) and K slices of those launches (0: the planner; A-B runs and tests).
   "fuse_x"  -1/0/1  x(t) W_gifo_x^T inside the step kernel (auto: NumStream <= 16) or as one batched product (:246)
 *   "vector", "fat", "small_max", "small_nt2"  kernel-family selection for A-B experiments and tests
 *   "profile" 0/1  run every kernel eagerly between its own start/stop HIP events on the
 *                  engine's stream (hipExtLaunchKernelGGL); setting the key clears the
 *                  statistics.  Used by bench.py for the roofline line. */
klstm_status klstm_set_option(klstm_engine *e, const char *key, int value);

/* With "profile" on: device time (microseconds, summed) and launch count of `kernel`
 * ("k_gates_step", "k_gates_fold", "k_dmf_step", "k_proj_step", "k_dr_step", "k_dm_step", "k_fold", "k_grads", ...)
 * over everything executed since the option was set.  Synchronises the stream. */
klstm_status klstm_profile_query(klstm_engine *e, const char *kernel, double *total_us,
                                 long *launches);

/* Test support: occupy `workgroups` compute units of `device` for about `microseconds` (one 1024-thread workgroup with
 * 96 KB of LDS per unit, spinning on the wall clock) on `hip_stream` (NULL: a private non-blocking stream).  Used by the
 * uneven-load tests of the persistent chain (MI355X_MICROARCH.md: test every hand-off under uneven load).  where_dev (or
 * NULL): 2 words per workgroup, filled with the XCC id and the HW_ID register of the compute unit it landed on. */
klstm_status klstm_debug_occupy(int device, int workgroups, int microseconds, void *hip_stream, unsigned *where_dev);

/* Test / probe support for the pipelined bf16 product of the many-stream chains (kaldi-lstm_amd/csrc/klstm_gemm16.hip):
 * C = A B^T (+ bias[n]) (+ add[m][n]) for one or two products that share their K in ONE launch, operands rounded to bf16 when staged,
 * fp32 accumulation, K split inside the launch.  mnk: M, N, K per job; ptrs: A [M x K], B [N x K], C, bias (or NULL), add (or NULL)
 * per job, device pointers; lds: lda, ldb, ldc, add_ld per job; force_nj (1 / 2 / 4: tile width 32 nj) and force_ks (1 / 2 / 4 / 8
 * K slices), 0 = the launcher's own plan; plan_out (or NULL) receives nj, ks and the number of output tiles. */
klstm_status klstm_debug_gemm_bf16_nt2(int njobs, const int *mnk, const float *const *ptrs, const int *lds, int force_nj, int force_ks,
                                       void *hip_stream, int *plan_out);
/* The same with bf16 copies of the operands in memory: copies = Ah [M x K], Bh [N x K] per job (unsigned short = bf16 bits, the RNE
 * roundings of A and B, same leading dimensions in elements, % 8 == 0, 16-byte aligned).  When every job has both, the kernel reads
 * THEM by LDS-DMA (half the bytes, no conversion pass) -- bit-identical results; NULL entries: as klstm_debug_gemm_bf16_nt2. */
klstm_status klstm_debug_gemm_bf16_nt2h(int njobs, const int *mnk, const float *const *ptrs, const int *lds,
                                        const unsigned short *const *copies, int force_nj, int force_ks, void *hip_stream, int *plan_out);

#ifdef __cplusplus
}
#endif
#endif /* KLSTM_H_ */
