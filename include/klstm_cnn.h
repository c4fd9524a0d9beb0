/* include/klstm_cnn.h -- the kcnn_* entries of libklstm.so: nnet1's convolutional and max-pooling components and the two activations
 * that stand between them (the CLDNN front end under the LSTMs; the numpy yardsticks:
 * tests/cnn_ref.py).  A family of its own next to the klstm_* entries of klstm.h, like kdrop_* and knlm_*: the same library, the same
 * klstm_status, the same klstm_last_error().  [UPSTREAM-unvendored nnet-convolutional-component.h, nnet-max-pooling-component.h,
 * nnet-activation.h]: the definitions below are stated from nnet1's documented behaviour; the sources are not vendored.
 *
 * Rows are frames (any count, r = t * S + s as everywhere); everything is per row.  Strides are in floats.
 *
 * THE DEFINITION: ConvolutionalComponent.  Numbers (D_in, D_out, pd = PatchDim, ps = PatchStep, st = PatchStride):
 *     n = D_in / st   spliced blocks of st values           P = 1 + (st - pd) / ps   patches
 *     K = n * pd      values per patch                      F = D_out / P            filters
 * Refused: a number < 1, st does not divide D_in, pd > st, (st - pd) % ps != 0, P does not divide D_out.
 *     patch(r,p)[s*pd + d] = in[r, s*st + p*ps + d]                                   s < n, d < pd
 *     out[r, p*F + f]      = bias[f] + sum_k patch(r,p)[k] * filters[f,k]             filters: F x K, row-major, contiguous
 *     in_diff[r,c]         = sum over all (s,p,d) with s*st + p*ps + d = c of  sum_f out_diff[r, p*F+f] * filters[f, s*pd+d]
 *     filters_grad[f,k]    = sum_r sum_p out_diff[r, p*F+f] * patch(r,p)[k]
 *     bias_grad[f]         = sum_r sum_p out_diff[r, p*F+f]
 * The update is the affine rule of klstm_affine_update:  corr = momentum * corr + grad;  filters -= lr * corr;  bias -= lr_bias *
 * bias_corr  (at momentum 0 what upstream does).
 *
 * THE DEFINITION: MaxPoolingComponent.  Numbers (D_in, D_out, z = PoolSize, g = PoolStep, w = PoolStride):
 *     Pin = D_in / w  patches of w values                   Q = 1 + (Pin - z) / g   pools (rounded down)   D_out = Q * w
 * Refused: a number < 1, w does not divide D_in, z > Pin, D_out != Q * w.  (Pin - z) % g patches at the end lie in no pool.
 *     out[r, q*w + f] = the maximum of in[r, (q*g + j)*w + f] over j < z, computed as  m = first; if (v > m) m = v  in order of j
 *     in_diff[r, p*w + f] = (1 / c_p) * sum over the pools q that contain p of (in[r,p*w+f] == out[r,q*w+f]) ? out_diff[r,q*w+f] : 0
 * c_p is the number of pools that contain patch p; the sum runs in order of q from +0.0f; the factor is one float division 1.0f / c_p
 * applied last.  Tied inputs each receive the whole diff.  A patch that no pool contains gets +0.0f.  With g == z and no ties this is
 * the true gradient; with overlapping pools it is nnet1's rule (the equal-element mask and the compensation for the overlap) and NOT
 * the true gradient of the maximum.
 *
 * THE DEFINITION: <Sigmoid> and <Tanh>.  y = 1 / (1 + exp(-x)) or tanh(x) in the forms of the LSTM cell (klstm_math.h: the hardware
 * exp2 and rcp, <= 3e-7 absolute); backward from the OUTPUT: in_diff = out_diff * y * (1 - y) or out_diff * (1 - y * y).
 *
 * ALL ENTRIES.  Asynchronous on hip_stream.  Every argument error is KLSTM_ERR_ARG before the first HIP call, with the outputs
 * untouched.  rows == 0 is KLSTM_OK and launches nothing.  The columns from the width up to the stride are never written.  Any row
 * count, any F, any K: edge tiles are masked.  The products run on the f32-input matrix instruction (exact f32 products, f32
 * accumulation); no im2col matrix is ever in memory.  CAPACITY: the convolution kernels keep input rows and a tile of the filters in
 * LDS; a shape whose smallest tiling does not fit (16 K + 16 D_in + ... floats beyond 160 KB: K of several thousand) is refused
 * with KLSTM_ERR_ARG. */
#ifndef KLSTM_CNN_H_
#define KLSTM_CNN_H_

#include <stddef.h>

#include "klstm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KCNN_SIGMOID = 0, KCNN_TANH = 1 };

/* The numbers of the convolution, on the host.  KLSTM_ERR_ARG (outputs untouched) for numbers the definition refuses or a null. */
klstm_status kcnn_conv_plan(int in_dim, int out_dim, int patch_dim, int patch_step, int patch_stride, int *n, int *P, int *K, int *F);

/* The floats of device workspace kcnn_conv_gradient / kcnn_conv_update need for `rows` rows (0 for rows <= 0 or refused numbers): the
 * partial gradients of the fixed split (KCNN_GRAD_SPLIT_ROWS rows each), summed in fixed order by the second stage. */
enum { KCNN_GRAD_SPLIT_ROWS = 64 };
size_t kcnn_conv_workspace_floats(int rows, int in_dim, int out_dim, int patch_dim, int patch_step, int patch_stride);

klstm_status kcnn_conv_propagate(const float *in, int in_stride, int rows, int in_dim, int out_dim, int patch_dim, int patch_step,
                                 int patch_stride, const float *filters, const float *bias, float *out, int out_stride, void *hip_stream);

/* in_diff == NULL: not wanted (KLSTM_OK, nothing is launched). */
klstm_status kcnn_conv_backpropagate(const float *out_diff, int od_stride, int rows, int in_dim, int out_dim, int patch_dim, int patch_step,
                                     int patch_stride, const float *filters, float *in_diff, int id_stride, void *hip_stream);

/* The pure gradient into caller storage (filters_grad: F x K, bias_grad: F; overwritten).  Bit-identical from run to run and
 * independent of the strides and of the pointers' alignment.  ws: at least kcnn_conv_workspace_floats(...) floats on the device. */
klstm_status kcnn_conv_gradient(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim, int out_dim,
                                int patch_dim, int patch_step, int patch_stride, float *filters_grad, float *bias_grad, float *ws,
                                size_t ws_floats, void *hip_stream);

/* Gradient, momentum and step: the second stage applies them; no parameter is touched before every partial of the call exists. */
klstm_status kcnn_conv_update(const float *in, int in_stride, const float *out_diff, int od_stride, int rows, int in_dim, int out_dim,
                              int patch_dim, int patch_step, int patch_stride, float *filters, float *bias, float *filters_corr,
                              float *bias_corr, float lr, float lr_bias, float momentum, float *ws, size_t ws_floats, void *hip_stream);

klstm_status kcnn_pool_propagate(const float *in, int in_stride, int rows, int in_dim, int out_dim, int pool_size, int pool_step,
                                 int pool_stride, float *out, int out_stride, void *hip_stream);

/* in, out: what kcnn_pool_propagate read and wrote.  in_diff == NULL: not wanted. */
klstm_status kcnn_pool_backpropagate(const float *in, int in_stride, const float *out, int out_stride, const float *out_diff, int od_stride,
                                     int rows, int in_dim, int out_dim, int pool_size, int pool_step, int pool_stride, float *in_diff,
                                     int id_stride, void *hip_stream);

/* kind: KCNN_SIGMOID | KCNN_TANH.  in == out (one stride) is allowed. */
klstm_status kcnn_activation(int kind, const float *in, int in_stride, int rows, int cols, float *out, int out_stride, void *hip_stream);
/* out: the activation's OUTPUT.  in_diff == NULL: not wanted.  in_diff == out_diff (one stride) is allowed. */
klstm_status kcnn_activation_diff(int kind, const float *out, int out_stride, const float *out_diff, int od_stride, int rows, int cols,
                                  float *in_diff, int id_stride, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
