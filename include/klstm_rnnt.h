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

/* The prediction network's input: row u*S + s of out [(Umax+1)*S x width] from x_u (x_0 = bos, x_u = y_u).  embed NULL: width = V and
 * the row is the one-hot of x_u.  embed [D x V] row-major (bias [D] or NULL): width = D and out[r, d] = embed[d, x_u] + bias[d].  Rows
 * without an input (u > U_s, or x_u outside [0, V)) are zeros.  1 <= S <= 32, 0 <= Umax <= 1023, 1 <= V, D; bos in [0, V). */
klstm_status krnnt_pack(const int *labels_dev, const int *label_offsets_dev, int S, int Umax, int V, int bos, const float *embed,
                        const float *embed_bias, int D, float *out, int out_stride, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
