/* include/klstm_rnnt.h -- the krnnt_* entries of libklstm.so: RNN-transducer training (Graves 2012), the joint network over the
 * T x (U+1) lattice fused with the lattice loss and its gradients (the torch yardstick:
 * tests/rnnt_ref.py).  A family of its own next to klstm.h, like knlm_* and kcnn_*: the same library, klstm_status, klstm_last_error().
 *
 * THE DEFINITION.  Per stream s: T_s frames (0: an idle stream), labels y_1 .. y_U, U = U_s >= 0, each in [0, V) and != blank.
 *     enc  [T*S x J]         row t*S + s: the encoder output, already projected to the joint width
 *     pred [(Umax+1)*S x J]  row u*S + s: the prediction network after it has seen bos, y_1 .. y_u
 *     W [V x J] row-major (Kaldi's linearity_), b [V]
 * Lattice node (t, u), 0 <= t < T_s, 0 <= u <= U:
 *     h        = tanh(enc[t] + pred[u])                      the cell's tanh (hardware exp2 and rcp, <= 3e-7 absolute)
 *     a        = W h + b                                     exact f32 products, f32 accumulation (the f32-input matrix instruction)
 *     lse      = max + log sum_v exp(a_v - max)
 *     lpb(t,u) = a_blank - lse ;  lpy(t,u) = a_{y_{u+1}} - lse  (u < U)
 *     alpha(0,0) = 0 ;  alpha(t,u) = logadd(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpy(t,u-1))
 *     beta(T-1,U) = lpb(T-1,U) ;  beta(t,u) = logadd(beta(t+1,u) + lpb(t,u), beta(t,u+1) + lpy(t,u))
 *     loss_s   = -beta(0,0)
 *     w_b(t,u) = exp(alpha(t,u) + lpb(t,u) + beta(t+1,u) + loss)    beta(T,U) = 0; 0 where t = T-1 and u < U
 *     w_y(t,u) = exp(alpha(t,u) + lpy(t,u) + beta(t,u+1) + loss)    0 at u = U
 *     g_v(t,u) = (w_b + w_y) softmax(a)_v - [v = blank] w_b - [v = y_{u+1}] w_y          = d loss / d a_v
 *     dz       = (g^T W) o (1 - h^2)
 *     d_enc[t] = sum_u dz(t,u) ;  d_pred[u] = sum_t dz(t,u) ;  W_grad = sum_{s,t,u} g h^T ;  b_grad = sum g
 * alpha and beta are kept per anti-diagonal d = t + u relative to the maximum of the diagonal before, the offsets are summed in double,
 * log 0 = -1e30, and the loss is taken in double.  Rows of idle streams, rows t >= T_s of d_enc and rows u > U_s of d_pred are written
 * as zero.  W_grad and b_grad are overwritten (the pure gradient of the call).
 *
 * A stream is REJECTED on the device when T_s < 0, T_s > T, U_s > Umax, or a label is outside [0, V) or equals blank.  That is an
 * argument problem, not a HIP error: the stream gets loss 0, counts in the totals, and its rows of d_enc and d_pred stay untouched
 * (as klstm_ctc_eval treats its streams).
 *
 * totals_dev (may be NULL): five doubles that are added to in stream order: loss sum, frames, labels, streams done, streams rejected.
 *
 * DETERMINISM.  No floating-point atomics anywhere; every sum has a fixed order: results are bit-identical from run to run, and loss,
 * d_enc and d_pred of a stream do not depend on which other streams share the call.
 *
 * LIMITS: 1 <= S <= 32, 1 <= T, 0 <= Umax <= 1023, T (Umax+1) S <= 2^24, J % 16 == 0, 16 <= J <= 1024, 2 <= V <= 4096, blank in
 * [0, V); beyond them KLSTM_ERR_SHAPE and nothing is launched.  A null required pointer, a row stride below the row, a pointer that is
 * not 4-byte aligned, a workspace that is too small or not 256-byte aligned: KLSTM_ERR_ARG with the outputs untouched.  Every check
 * runs before the first HIP call; everything is asynchronous on hip_stream; nothing is read back.
 *
 * THE WORKSPACE holds no array of S T (Umax+1) V or S T (Umax+1) J elements: neither h nor the logits ever go to memory.  With
 * N = S T (Umax+1), up256(x) = x rounded up to 256, tb = ceil(T / KRNNT_TILE_T) and splits = krnnt_grad_splits(J, V):
 *     bytes = up256(16 S)                                  status, T_s, U_s, label offset per stream
 *           + up256(8 S)                                   the losses in double
 *           + up256(16 S (T + Umax + 1))                   the offsets of the alpha and the beta diagonals in double
 *           + 7 up256(4 N)                                 lpb, lpy, lse, alpha, beta, w_b, w_y: one float per node each
 *           + up256(16 S T J)                              the partial d_enc rows of the backward workgroup's 4 waves }
 *           + up256(4 tb S (Umax+1) J)                     the partial d_pred rows of the t blocks                    } the partials' term:
 *           + up256(4 splits V J) + up256(8 splits V)      the partial W_grad (float) and b_grad (double) of the      } no N V, no N J
 *                                                          fixed splits                                               }
 * krnnt_grad_splits(J, V) = 2^24 / (V J) clamped to [8, 256]: a function of the shape alone, never of the launch. */
#ifndef KLSTM_RNNT_H_
#define KLSTM_RNNT_H_

#include <stddef.h>

#include "klstm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KRNNT_TILE_T = 16, KRNNT_TILE_U = 8, KRNNT_PASS_V = 128 };   /* lattice nodes of a forward tile (t x u), classes of a register pass */
enum { KRNNT_BAND_TILE_R = 8 };                                     /* band offsets of a banded forward tile (16 t x 8 r) */

int krnnt_grad_splits(int J, int V);

/* The whole formula (a call with gradients) and its first four lines (a call without: the partials' term is not needed; at S = 8,
 * T = 500, U = 50: 5.8 MB of 99 MB).  0 (and the message in klstm_last_error()) beyond the limits. */
size_t krnnt_workspace_bytes(int T, int S, int Umax, int J, int V);
size_t krnnt_forward_workspace_bytes(int T, int S, int Umax);

/* lens_dev [S] int, labels_dev / label_offsets_dev [S+1]: the CSR arrays of klstm_ctc_eval.  utt_loss_dev [S] floats.  The four gradient
 * outputs d_enc [T*S x J], d_pred [(Umax+1)*S x J], W_grad [V x J], b_grad [V] are given together or all NULL (forward and loss
 * only: the backward kernel is not launched, and a workspace of krnnt_forward_workspace_bytes is enough). */
klstm_status krnnt_eval(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                        int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                        float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad, float *b_grad,
                        float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* BAND-PRUNED TRAINING (the torch yardstick: tests/rnnt_band_ref.py).  The lattice is evaluated only
 * inside a band of R label positions per frame.  Per stream, with h, a, lse, lpb, lpy as in THE DEFINITION:
 *     band_lo[s][t] = u0(t), 0 <= t < T_s ;  node (t, u) is IN BAND iff u0(t) <= u <= min(U, u0(t) + R - 1)
 *     alpha, beta, w_b, w_y: those of THE DEFINITION with every node outside the band taken as log 0: a blank step from (t, u) counts
 *              only if (t+1, u) is in band (or t = T_s - 1, u = U), a label step only if (t, u+1) is in band
 *     loss_s   = -log of the probability of all alignments that stay in the band  (= the full loss when R >= U + 1 and u0 = 0)
 *     d_enc[t], d_pred[u], W_grad, b_grad: the gradients of that loss, the sums over the nodes in band only; a d_pred row whose u is in
 *              no band is zero; rows t >= T_s and u > U_s are zero as in krnnt_eval
 * A band is VALID iff u0(0) = 0, 0 <= u0(t+1) - u0(t) <= R - 1 and u0(T_s - 1) <= U <= u0(T_s - 1) + R - 1: then it is connected and
 * the loss is finite.  A stream with an invalid band is REJECTED on the device like a stream with a bad label: loss 0, counted in
 * totals[3] and totals[4], its rows of d_enc and d_pred untouched.  Entries t >= T_s of a row of band_lo are not read.
 * alpha and beta are kept per anti-diagonal d = t + u relative to the maximum of the diagonal before, in double while they are carried,
 * the offsets summed in double, the loss taken in double; no floating-point atomics, fixed summation orders: runs are bit-identical,
 * loss, d_enc and d_pred of a stream do not depend on its company, and the logits of a node are the same bits in the forward and in
 * the backward kernel.
 *
 * LIMITS: those of krnnt_eval on S, J, V, blank and Umax <= 1023; 1 <= R <= 64; S T R <= 2^24 (in place of T (Umax+1) S <= 2^24):
 * KLSTM_ERR_SHAPE; the argument checks of krnnt_eval (band_lo_dev is required): KLSTM_ERR_ARG.  Every check runs before the first
 * HIP call; everything is asynchronous on hip_stream; nothing is read back.
 *
 * THE WORKSPACE has no term in T (Umax+1): the node planes are band-relative [S][T][R], d_enc needs no partials (a block of 16 frames
 * owns its rows and adds to d_enc itself), and the d_pred partials of a block of frames cover only the label rows its band touches:
 * block k's rows u0(16 k) .. u0(its last frame) + R - 1 live at rows u + k R of a per-stream array of (Umax+1) + tb R rows.  With
 * N = S T R, tb = ceil(T / KRNNT_TILE_T), splits = krnnt_grad_splits(J, V):
 *     bytes = up256(16 S)                                  status, T_s, U_s, label offset per stream
 *           + up256(8 S)                                   the losses in double
 *           + up256(16 S (T + 1024))                       the offsets of the alpha and the beta diagonals in double, sized for Umax = 1023
 *           + 7 up256(4 N)                                 lpb, lpy, lse, alpha, beta, w_b, w_y: one float per band node each
 *           + up256(4 S ((Umax+1) + tb R) J)               the d_pred windows of the frame blocks                     } the partials' term:
 *           + up256(4 splits V J) + up256(8 splits V)      the partial W_grad (float) and b_grad (double)             } gradients only
 * At S = 8, T = 500, U = 50, R = 8, J = 512, V = 64: 39.8 MB against the 99 MB of krnnt_workspace_bytes, 33.6 MB of it the W_grad
 * partials that both share; forward only 1.1 MB against 5.8 MB. */
size_t krnnt_band_workspace_bytes(int T, int S, int Umax, int R, int J, int V);
size_t krnnt_band_forward_workspace_bytes(int T, int S, int R);

/* The arguments of krnnt_eval plus R and band_lo_dev [S][T] (int); the four gradient outputs are given together or all NULL. */
klstm_status krnnt_band_eval(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                             int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank, int R,
                             const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                             float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream);

/* A valid band around an alignment.  label_frames_dev: the frame f_i of every label, CSR by label_offsets_dev (what klstm_ctc_align of
 * an auxiliary CTC head or the greedy decoder's frame_dev give), or NULL.  Per stream, with U = its label count:
 *     c(t)  = #{i : f_i < t}                    NULL frames: the linear c(t) = t U / T_s (integer division)
 *     hi    = max(0, U + 1 - R)
 *     u0(t) = min(max(c(t) - left, 0), hi) ;  u0(T_s - 1) = hi
 *     from the end: u0(t) = max(u0(t), u0(t+1) - (R - 1))            (a suffix maximum of u0(t) - t (R - 1))
 * If the last step lifts u0(0) above 0 (hi > (T_s - 1)(R - 1)), or the frames are not nondecreasing within [0, T_s), the whole row is
 * written as -1 and krnnt_band_eval rejects the stream; so is the row of a stream with T_s < 0 or T_s > T; an idle stream's row is 0.
 * Entries t >= T_s repeat the last value.  LIMITS: 1 <= S <= 32, 1 <= T, 1 <= R <= 64, S T R <= 2^24, 0 <= left < R: KLSTM_ERR_SHAPE. */
klstm_status krnnt_band_from_frames(const int *label_frames_dev, const int *lens_dev, const int *label_offsets_dev, int T, int S, int R, int left,
                                    int *band_lo_dev, void *hip_stream);

/* THE BF16 JOINT (the torch yardstick: tests/rnnt_band_bf16_ref.py).  BAND-PRUNED TRAINING with the
 * three joint products on the bf16 matrix instruction, f32 accumulation; inputs and outputs stay f32.  It is THE DEFINITION inside the
 * band with three roundings, bf(x) = round to nearest even to bfloat16:
 *     h  = tanh(enc[t] + pred[u]) in f32 ;  hb = bf(h) ;  Wb = bf(W), converted once per call
 *     a  = Wb hb + b        products of bf16 values are exact, accumulated in f32 in a fixed order; b is f32
 *     lse, lpb, lpy, alpha, beta, w_b, w_y, the loss: unchanged, from these a (the same lattice and weights kernels run on the planes)
 *     g_v(t, u) in f32 as in THE DEFINITION ;  gb = bf(g)
 *     dz     = (gb^T Wb) o (1 - h^2)   with the unrounded h: the rounding of h counts as the identity (straight-through)
 *     W_grad = sum gb hb^T             f32 accumulation, the partials in a fixed order
 *     b_grad = sum g                   unrounded, in double
 *     d_enc, d_pred: the sums of dz as in BAND-PRUNED TRAINING
 * Everything else is krnnt_band_eval's, word for word: the limits, the argument checks (all before the first HIP call), rejected and
 * idle streams, the five totals, no floating-point atomics, bit-identical runs, a stream's loss and rows independent of its company,
 * a node's logits the same bits in the forward and the backward kernel, everything asynchronous on hip_stream, nothing read back.
 * J is a multiple of 16: the last k-panel of 32 may be half full and is zero-filled.
 * THE WORKSPACE is krnnt_band_workspace_bytes (want_grads) or krnnt_band_forward_workspace_bytes (without) plus the bf16 copies of W,
 * with Jp = J and Vp = V rounded up to a multiple of 32:
 *           + up256(2 V Jp)                                Wb [V][Jp], zeros behind J                     (with and without gradients)
 *           + up256(2 J Vp)                                its transpose [J][Vp], zeros behind V: the B operand of gb Wb   (gradients only)
 * At J = 512, V = 1024: 2 MiB on top of the banded workspace.  0 (and the message) beyond the limits. */
size_t krnnt_band_bf16_workspace_bytes(int T, int S, int Umax, int R, int J, int V, int want_grads);
klstm_status krnnt_band_eval_bf16(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                                  int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                                  int R, const int *band_lo_dev, float *d_enc, int d_enc_stride, float *d_pred, int d_pred_stride, float *W_grad,
                                  float *b_grad, float *utt_loss_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                                  void *hip_stream);

/* FORCED ALIGNMENT (the torch yardstick: tests/rnnt_align_ref.py).  The best single alignment of the
 * given labels: where the model puts its transcript.  Per stream, with lpb, lpy as in THE DEFINITION (krnnt_band_align: as in BAND-PRUNED
 * TRAINING, every node outside the band is log 0; with bf16 != 0 lpb, lpy are those of THE BF16 JOINT, Wb converted once per call):
 *     v(0,0)  = 0
 *     v(t,u)  = max( v(t-1,u) + lpb(t-1,u) ,  v(t,u-1) + lpy(t,u-1) )
 * carried in double.  The label step is taken iff its candidate is strictly greater (`>`): a tie takes the blank step, and a candidate
 * that is log 0 never wins.
 *     score_s = v(T_s-1, U) + lpb(T_s-1, U)         the log-probability of the best alignment, given as a float
 *     path    : the backtrace from (T_s-1, U) to (0,0)
 *     f_i     = the frame t of the label step into node (t, i), i = 1 .. U
 *     logp_i  = lpy(f_i, i-1)
 * f is nondecreasing within [0, T_s): what krnnt_band_from_frames accepts as label_frames_dev.  label_frames_dev and label_logp_dev (may
 * be NULL) are CSR by label_offsets_dev, indexed like labels_dev; score_dev [S].  No diagonal is normalised: a max-plus value is a sum of
 * at most T + U floats.  A REJECTED stream (the rules of krnnt_eval; krnnt_band_align: and an invalid band) and an idle stream get score
 * 0 and their entries of label_frames_dev and label_logp_dev stay untouched.  No atomics: runs are bit-identical and a stream's result
 * does not depend on its company.  Every check runs before the first HIP call; everything is asynchronous on hip_stream; nothing is read
 * back.  LIMITS and argument checks: krnnt_align those of krnnt_eval, krnnt_band_align those of krnnt_band_eval.
 * The decisions are kept as bits, one 64-bit word per (diagonal, wave of 64 label positions), not as a plane of nodes, and neither
 * workspace has a term in N V or N J; the banded one has none in T (Umax+1):
 *     krnnt_align:       up256(16 S) + 3 up256(4 S T (Umax+1)) + up256(8 S (T+Umax+1) ceil((Umax+1)/64))      meta; lpb, lpy, lse; the words
 *     krnnt_band_align:  up256(16 S) + 3 up256(4 S T R) + up256(8 S (T+1024))  [+ up256(2 V Jp) with bf16, Jp = J rounded up to 32] */
size_t krnnt_align_workspace_bytes(int T, int S, int Umax);
klstm_status krnnt_align(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                         int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank,
                         int *label_frames_dev, float *label_logp_dev, float *score_dev, void *workspace, size_t workspace_bytes,
                         void *hip_stream);
size_t krnnt_band_align_workspace_bytes(int T, int S, int R, int J, int V, int bf16);
klstm_status krnnt_band_align(const float *enc, int enc_stride, const float *pred, int pred_stride, const float *W, const float *b, int T, int S,
                              int Umax, int J, int V, const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank, int R,
                              const int *band_lo_dev, int bf16, int *label_frames_dev, float *label_logp_dev, float *score_dev, void *workspace,
                              size_t workspace_bytes, void *hip_stream);

/* THE SIMPLE JOINER (the torch yardstick: tests/rnnt_simple_ref.py).  The first pass of pruned
 * transducer training: a joiner without tanh and without W, whose logits are the sum of an encoder-side and a predictor-side row, is
 * evaluated over the whole lattice; its node occupations select the band that krnnt_band_eval then runs the real joint in.  Per stream s:
 * T_s frames and labels y_1 .. y_U through the CSR arrays of krnnt_eval.
 *     am [T*S x V]          row t*S + s : encoder-side logits      (row stride am_stride)
 *     lm [(Umax+1)*S x V]   row u*S + s : predictor-side logits    (row stride lm_stride)
 *     node (t, u):  a_v      = am[t][v] + lm[u][v]
 *                   ma(t)    = max_v am[t][v]        ml(u) = max_v lm[u][v]
 *                   P(t,u)   = sum_v exp(am[t][v] - ma(t)) * exp(lm[u][v] - ml(u))       clamped below at FLT_MIN
 *                   lse(t,u) = ma(t) + ml(u) + log P(t,u)
 *                   lpb      = a_blank - lse ;  lpy = a_{y_{u+1}} - lse  (u < U)
 *     alpha, beta, loss_s, w_b, w_y : exactly those of THE DEFINITION of krnnt_eval on these lpb, lpy
 *     occ(t,u)   = w_b(t,u) + w_y(t,u)                 the node's posterior; 0 outside t < T_s, u <= U_s
 *     g_v(t,u)   = occ * exp(a_v - lse) - [v = blank] w_b - [v = y_{u+1}] w_y
 *     d_am[t][v] = sum_u g_v(t,u)       d_lm[u][v] = sum_t g_v(t,u)
 * P is the product of two matrices, [T x V] . [V x (Umax+1)]: no array of nodes x classes is ever formed.  exp(a_v - lse) is taken as
 * exp(am[t][v] - ma(t)) exp(lm[u][v] - ml(u)) / P, and the indicator terms are summed in double.
 * DOMAIN.  With the spread max - min of every row of am and of lm at most 40, every factor is at least e^-40 and every term of P at
 * least e^-80 > FLT_MIN: no term leaves the normal float range and the formula is the log-softmax of a.  Beyond that spread terms
 * flush to zero, the clamp keeps log P finite, and the result is approximate (a class both of whose factors vanished counts as
 * impossible).
 * What carries over from krnnt_eval unchanged: the rejection rules (T_s < 0, T_s > T, U_s > Umax, a label outside [0, V) or equal to
 * blank: loss 0, counted in the totals, the stream's rows of d_am and d_lm and its part of occ untouched); the five totals; zero rows
 * t >= T_s of d_am and u > U_s of d_lm, and of idle streams; every check before the first HIP call; everything asynchronous on
 * hip_stream; no floating-point atomics, every sum in a fixed order: runs are bit-identical and a stream's loss, rows and occ do not
 * depend on its company.
 *
 * LIMITS: 1 <= S <= 32, 1 <= T, 0 <= Umax <= 1023, T (Umax+1) S <= 2^24, 2 <= V <= 4096, blank in [0, V): KLSTM_ERR_SHAPE.  The pointer,
 * stride (>= V), alignment and workspace checks of krnnt_eval: KLSTM_ERR_ARG.  d_am [T*S x V] and d_lm [(Umax+1)*S x V] are given
 * together or both NULL; occ_dev [S][T][Umax+1] floats or NULL.
 *
 * THE WORKSPACE holds no array of S T (Umax+1) V elements.  With N = S T (Umax+1) and Vp = V rounded up to 32 (the K panel):
 *     bytes = up256(16 S)                                  status, T_s, U_s, label offset per stream
 *           + up256(8 S)                                   the losses in double
 *           + up256(16 S (T + Umax + 1))                   the offsets of the alpha and the beta diagonals in double
 *           + 7 up256(4 N)                                 lpb, lpy, P (then q = occ / P), alpha, beta, w_b, w_y: one float per node each
 *           + up256(4 S T Vp) + up256(4 S (Umax+1) Vp)     exp(am - ma) and exp(lm - ml), the rows zero-padded to Vp
 *           + up256(4 S T) + up256(4 S (Umax+1))           the row maxima ma and ml
 * At S = 8, T = 500, U = 50, V = 1024: 23.9 MB, 18.1 MB of it the two operands. */
size_t krnnt_simple_workspace_bytes(int T, int S, int Umax, int V);

klstm_status krnnt_simple_eval(const float *am, int am_stride, const float *lm, int lm_stride, int T, int S, int Umax, int V,
                               const int *lens_dev, const int *labels_dev, const int *label_offsets_dev, int blank, float *d_am,
                               int d_am_stride, float *d_lm, int d_lm_stride, float *occ_dev, float *utt_loss_dev, double *totals_dev,
                               void *workspace, size_t workspace_bytes, void *hip_stream);

/* THE BAND RULE: a valid band of width R from node occupations (any non-negative plane [S][T][Umax+1]; krnnt_simple_eval's occ is the
 * intended one).  Per stream, with U its label count and hi = max(0, U + 1 - R):
 *     w(t, k)  = sum_{r = 0}^{R-1} (double) occ(t, k + r)      added in the order of r; terms with k + r > U are 0
 *     c(t)     = the k in [0, hi] with the largest w(t, k); `>` decides, from -infinity at k = 0 on: a tie goes to the lower k, and a
 *                NaN never wins
 *     c(0) = 0, then c(T_s - 1) = hi
 *     m(t)     = max_{t' <= t} c(t')                                   (prefix maximum: nondecreasing)
 *     u0(T_s - 1) = hi ;  from the end: u0(t) = max(m(t), u0(t+1) - (R - 1))
 * If this leaves u0(0) > 0 the row is all -1, as krnnt_band_from_frames writes for a stream that no band of width R can serve; so is
 * the row of a stream with T_s < 0, T_s > T or more labels than Umax.  An idle stream's row is 0; entries t >= T_s repeat the last
 * value.  By construction the result is a VALID band in the sense of krnnt_band_eval.  Sums in double in a fixed order and integer
 * scans: the result is exact.  LIMITS: 1 <= S <= 32, 1 <= T, 0 <= Umax <= 1023, T (Umax+1) S <= 2^24, 1 <= R <= 64: KLSTM_ERR_SHAPE;
 * a null or misaligned pointer: KLSTM_ERR_ARG.  band_lo_dev: [S][T] int, as krnnt_band_eval reads it. */
klstm_status krnnt_band_from_occupation(const float *occ_dev, const int *lens_dev, const int *label_offsets_dev, int T, int S, int Umax,
                                        int R, int *band_lo_dev, void *hip_stream);

/* The prediction network's input: row u*S + s of out [(Umax+1)*S x width] from x_u (x_0 = bos, x_u = y_u).  embed NULL: width = V and
 * the row is the one-hot of x_u.  embed [D x V] row-major (bias [D] or NULL): width = D and out[r, d] = embed[d, x_u] + bias[d].  Rows
 * without an input (u > U_s, or x_u outside [0, V)) are zeros.  1 <= S <= 32, 0 <= Umax <= 1023, 1 <= V, D; bos in [0, V). */
klstm_status krnnt_pack(const int *labels_dev, const int *label_offsets_dev, int S, int Umax, int V, int bos, const float *embed,
                        const float *embed_bias, int D, float *out, int out_stride, void *hip_stream);

/* GREEDY (BEST-PATH) DECODING, label-synchronous (the torch yardstick: tests/rnnt_greedy_ref.py).
 * Plain greedy search per stream, with h, a, lse as in THE DEFINITION above:
 *     t = 0, u = 0, n = 0, score = 0
 *     while t < T_s:   k = argmax_v a_v(t, u)                              (`>` decides: a tie goes to the lower class)
 *         k == blank:  score += a_blank - lse ; t += 1 ; n = 0
 *         otherwise:   score += a_k - lse ; append (k, t) ; u += 1 ; n += 1 ; stop (truncated) when u == max_len ;
 *                      n == max_symbols: t += 1 ; n = 0                    (at most max_symbols labels per frame, no blank is scored)
 * The node (t, u) depends on enc[t] and on the predictor after bos, y_1 .. y_u only, so the walk along t at a fixed u needs one
 * predictor row: krnnt_greedy_step is step u of ALL streams together.  Every live stream has emitted u labels; pred_rows row s is its
 * predictor output; all its frames from t_s on are scanned against that row in parallel (16 frames per matrix tile); the first frame
 * whose argmax is not blank gives label u + 1 and its time, the frames before it are the blank steps of the path and the frames behind
 * it are discarded.  A stream without a hit up to T_s is finished.  So the loop is
 *     krnnt_greedy_begin(...)                          next_in = the rows of bos
 *     repeat up to max_len + 1 times:  pred_rows = predictor(next_in), one row per stream, its state carried from call to call
 *                                      krnnt_greedy_step(...)             next_in = the rows of the labels just emitted
 * and the predictor advances for all live streams at once: no stream ever has to hold its state.  U + 1 dependent steps instead of
 * T + U.  Tokens, frames and score are those of the plain loop: only nodes on the greedy path reach them.
 *
 * next_in [S x width]: row s is the predictor's next input, written as krnnt_pack writes a row (one-hot over V columns, or with embed
 * [D x V] the gathered column plus bias over D); zeros for a stream that is not live.  hyp_dev / frame_dev [S][max_len]: labels and
 * their frames (frame_dev may be NULL); hyp_len_dev [S]; score_dev [S]: the path's log-probability so far, summed in double (blank
 * terms in frame order, each label's term behind the blanks before it) and given as a float; a finished stream's score includes the
 * blanks up to T_s, a truncated stream's ends with its last label.  flags_dev [S]: bit 0 finished, bit 1 truncated (max_len labels),
 * bit 2 rejected (T_s < 0 or T_s > T: no labels, score 0), bit 3 idle (T_s = 0); 0: live.  live_dev: one int, the streams still live.
 * A step after every stream has stopped launches workgroups that leave at once and rewrites the same outputs.
 *
 * state: krnnt_greedy_state_bytes(T, S, J) bytes (0 and a message beyond the limits), 256-byte aligned, private to the decode between
 * begin and the last step, which must give the same T, S, J: per stream the flags, T_s, t_s, the symbols at the current frame, the
 * length, the score in double and hit_chunk; per (stream, chunk of 64 frames, 32 for J > 512) one record: hit frame or -1, label, the
 * label's log-probability, and the sum of log p(blank) over the chunk's frames before the hit.  hit_chunk is lowered with an integer
 * atomicMin by a chunk that has a hit, and a workgroup that starts later and sees a lower chunk there leaves without work: its record
 * would never be read, so the result does not depend on that race.  No floating-point atomics; runs are bit-identical and a stream's
 * tokens, frames and score do not depend on its company.
 *
 * LIMITS: those of krnnt_eval on S, T (T S <= 2^24), J, V and blank; bos in [0, V); 1 <= max_len <= 1023; 1 <= max_symbols; D >= 1 with
 * embed: KLSTM_ERR_SHAPE.  A null required pointer, a row stride below the row, a pointer that is not 4-byte aligned, a state that is
 * too small or not 256-byte aligned: KLSTM_ERR_ARG with the outputs untouched.  Every check runs before the first HIP call; everything
 * is asynchronous on hip_stream; nothing is read back. */
size_t krnnt_greedy_state_bytes(int T, int S, int J);

klstm_status krnnt_greedy_begin(int T, int S, int J, int V, int bos, const int *lens_dev, const float *embed, const float *embed_bias, int D,
                                float *next_in, int next_in_stride, void *state, size_t state_bytes, void *hip_stream);

klstm_status krnnt_greedy_step(const float *enc, int enc_stride, const float *pred_rows, int pred_stride, const float *W, const float *b, int T,
                               int S, int J, int V, int blank, int max_symbols, int max_len, const float *embed, const float *embed_bias, int D,
                               float *next_in, int next_in_stride, int *hyp_dev, int *hyp_len_dev, int *frame_dev, float *score_dev,
                               int *flags_dev, int *live_dev, void *state, size_t state_bytes, void *hip_stream);

/* BEAM SEARCH WITH N-BEST LISTS, label-synchronous (the torch yardstick: tests/rnnt_beam_ref.py).
 * A hypothesis is a label prefix y = y_1 .. y_u; its predictor row is p(y), the predictor after bos, y_1 .. y_u; h, a, lse, lpb are those
 * of THE DEFINITION at node (t, u) with that row, and lpy_y(t, k) = a_k - lse for every class k != blank.
 *     alpha_()(t)  = sum_{t' < t} lpb_()(t')                                  (the empty prefix; alpha(0) = 0)
 *     e_{y+k}(t)   = alpha_y(t) + lpy_y(t, k)                                 the entry column of the child y+k
 *     alpha_{y}(t) = logadd(alpha_y(t-1) + lpb_y(t-1), e_y(t)),  alpha_y(-1) = log 0
 *     complete(y)  = alpha_y(T_s-1) + lpb_y(T_s-1)                            = log Pr(y | x) = -loss_s of krnnt_eval on labels y
 *     prefix(y+k)  = logsumexp_t e_{y+k}(t)                                   = log Pr(the labels start with y+k | x);  prefix(()) = 0
 * In probabilities prefix(y) = complete(y) + sum_k prefix(y+k): prefix(y) bounds complete(z) of every z that extends y.  The search per
 * stream, with beam B, list size N <= B and label cap max_len:
 *     L_0 = { () };  list = empty
 *     step u = 0, 1, ...:
 *         for every y in L_u (slot order): offer (y, complete(y)) to the list   (the N best by score; a tie keeps the earlier entry)
 *         thr = the N-th best score in the list, -inf while it holds fewer than N
 *         candidates (y, k), y in L_u, k != blank, scored prefix(y+k); keep those with score > thr
 *         L_{u+1} = the B best candidates, score descending, ties to the lower (parent slot, class)
 *         L_{u+1} empty: finished.   u + 1 > max_len with L_{u+1} not empty: truncated (the list stands as it is)
 * If no candidate above thr was ever cut by B, the list is the exact N-best over all label sequences of length <= max_len; otherwise bit
 * 4 of the stream's flags (pruned) is set.  alpha, the chunk sums and every listed score are summed in double; scores are given as floats.
 * The loop is that of the greedy search over S B rows, row s B + b: slot b of stream s:
 *     krnnt_beam_begin(...)                          next_in = the bos row in slot 0 of every live stream, parent_dev = -1 everywhere
 *     repeat up to max_len + 1 times:  the predictor's state of row i becomes that of row parent_dev[i] (zero state at -1:
 *                                      krnnt_gather_state), pred_rows = predictor(next_in)
 *                                      krnnt_beam_step(...)               next_in, parent_dev = those of L_{u+1}
 * next_in [S B x width]: rows as krnnt_pack writes them, zeros for an empty slot.  parent_dev [S B]: the ROW (s B + b') of the previous
 * step's pred_rows that the new slot continues, -1 for an empty slot.  The list follows the contract of csrc/klstm_ctc_nbest.h:
 * nbest_hyp [S][N][max_len], nbest_len [S][N], nbest_score [S][N] (complete(y), descending), nbest_count [S]; entries beyond the count:
 * length 0, score 0, tokens untouched.  flags_dev [S]: the bits of the greedy search (a rejected or idle stream: count 0) plus bit 4.
 * live_dev: one int, the live slots of all streams.  A step after every stream has stopped rewrites the same outputs.
 *
 * state: krnnt_beam_state_bytes(T, S, B, J, V) bytes (0 and a message beyond the limits), 256-byte aligned, private to the decode between
 * begin and the last step, which give the same T, S, B, J, V (and every step the same N and max_len).  With SB = S B, FB = 64 (32 for
 * J > 512), nc = ceil(T / FB) and every term rounded up to 256:
 *     bytes = 5 x 4 S                       flags, T_s, step, live slots, list count per stream
 *           + 8 x 32 S + 4 x 32 S           the list's scores in double and its lengths
 *           + 3 x 4 SB                      live, parent row, label per slot
 *           + 4 x 2 x 1024 SB               the token rows of two generations
 *           + 3 x 8 SB T + 2 x 4 SB T       per frame in double: the entry column e, Bl, Cl; lse as two floats (maximum, log of the sum)
 *           + 4 x 8 SB nc                   per chunk in double: A_in, Bl(f1), Cl(f1-1), the offset of Y
 *           + 4 x 2 V SB nc                 X_k and Y_k of every chunk: 2 V floats per (slot, chunk), never T x V
 *           + 8 SB V                        the candidates' prefix scores
 * No atomics; runs are bit-identical, and a stream's list does not depend on its company.
 *
 * LIMITS: those of krnnt_greedy_* on S, T, J, V, blank, bos, max_len and D, and 1 <= N <= B <= 32: KLSTM_ERR_SHAPE.  A null required
 * pointer, a row stride below the row, a pointer that is not 4-byte aligned, a state that is too small or not 256-byte aligned:
 * KLSTM_ERR_ARG with the outputs untouched.  Every check runs before the first HIP call; everything is asynchronous on hip_stream;
 * nothing is read back. */
size_t krnnt_beam_state_bytes(int T, int S, int B, int J, int V);

/* The predictor's side of a step: klstm_set_state_host on the device, without a host round trip.  Stream i of the engine takes the
 * carried (c, r) of stream src_dev[i] (num_stream ints on the device; -1, or anything outside [0, num_stream): zero state).
 * Asynchronous on the engine's stream; afterwards the engine is as if klstm_set_state_host had been given the gathered arrays (resets
 * issued before are forgotten).  An entry of this family, defined with the engine: the list of klstm_* names stays as it is. */
klstm_status krnnt_gather_state(klstm_engine *e, const int *src_dev);

klstm_status krnnt_beam_begin(int T, int S, int B, int J, int V, int bos, const int *lens_dev, const float *embed, const float *embed_bias, int D,
                              float *next_in, int next_in_stride, int *parent_dev, void *state, size_t state_bytes, void *hip_stream);

klstm_status krnnt_beam_step(const float *enc, int enc_stride, const float *pred_rows, int pred_stride, const float *W, const float *b, int T,
                             int S, int B, int N, int J, int V, int blank, int max_len, const float *embed, const float *embed_bias, int D,
                             float *next_in, int next_in_stride, int *parent_dev, int *nbest_hyp, int *nbest_len, float *nbest_score,
                             int *nbest_count, int *flags_dev, int *live_dev, void *state, size_t state_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
