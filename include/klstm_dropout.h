/* include/klstm_dropout.h -- the kdrop_* entries of libklstm.so: forward-connection dropout with a counter-based mask (DESIGN.md 4v;
 * INTEGRATION.md 3p; the numpy twin: tests/dropout_ref.py).  A family of its own next to the klstm_* entries of klstm.h, like the
 * knlm_* entries of klstm_nlm.h: the same library, the same klstm_status, the same klstm_last_error().
 *
 * The operator of Zaremba, Sutskever and Vinyals ("Recurrent neural network regularization"): it acts on what goes UP between the
 * layers, never on what goes through time.  The reference left its own "LSTM forward dropout" switched off (commented-out lines in
 * bd-nnet-lstm-projected-streams.h, README FAQ Q4) and only declares Nnet::SetDropoutRetention; this is that operator with retention.
 *
 * THE DEFINITION.  Retention p is a float with 2^-32 <= p <= 1.
 *     thr   = min(floor((double)p * 2^32), 2^32 - 1)   as a uint32
 *     scale = 1.0f / p                                  one float division
 * For element (r, c) of a rows x cols block, with q = c >> 2 and j = c & 3:
 *     w[0..3] = Philox4x32-10(counter = (q, u, step, tag), key = (seed & 0xffffffff, seed >> 32))
 *     KDROP_ELEMENT:   u = r,                  tag = salt
 *     KDROP_SEQUENCE:  u = seq_id[r mod S],    tag = salt | 0x80000000,   step taken as 0
 * (rows are time-major, r = t * S + s: one mask per (stream, sequence) holds for every frame of that sequence, across the minibatches
 * of a truncated BPTT too).  salt < 2^31.  The element is KEPT iff w[j] < thr, and
 *     out = keep ? in * scale : +0.0f
 * The zero is written as such: a NaN or an Inf under a dropped element does not pass.  At p == 1 the call is a bit-for-bit copy
 * (nothing at all when in place) and draws no numbers.
 *
 * Philox4x32-10 is the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3"): ten rounds,
 * multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), the key bumped by the Weyl constants 0x9E3779B9 and
 * 0xBB67AE85 between rounds.  Known answers: counter 0 0 0 0, key 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ffffffff ->
 * 408f276d 41c83b0e a20bc7c6 6d5451fd; counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb
 * 5001e420 24126ea1.
 *
 * The mask depends on (seed, salt, step, row or sequence, column) and on nothing else: not on strides, alignment, launch geometry
 * or which code path ran.  The backward pass is the same call on out_diff with the same counters.  No mask is ever stored, nothing
 * is read back, and a training run can be replayed bit for bit from its seed.
 *
 * DEFAULT OFF.  The <Dropout> component of klstm_nnet.hpp is a copy until somebody switches it on (the four trainers do, for their
 * own duration, unless they cross-validate): a forgotten switch costs regularisation, never test accuracy.
 *
 * UNMEASURED.  8 bytes of traffic per element against roughly 40 quarter-rate integer multiplies per quad of four: by a paper
 * estimate about level with HBM.  What tools/dropout_probe.py measured stands in DESIGN.md 4v. */
#ifndef KLSTM_DROPOUT_H_
#define KLSTM_DROPOUT_H_

#include "klstm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KDROP_ELEMENT = 0, KDROP_SEQUENCE = 1 };

/* The two numbers of the definition, on the host (no device is touched).  A retention outside [2^-32, 1] or a NaN, or a null
 * pointer: KLSTM_ERR_ARG with the outputs untouched. */
klstm_status kdrop_threshold(float retention, unsigned *thr, float *scale);

/* out = dropout(in) over a rows x cols block of floats, rows in_stride / out_stride floats apart.  Asynchronous on hip_stream.
 * in == out (with one stride) is allowed; every other overlap of the two blocks' address ranges is refused.  mode: KDROP_ELEMENT or
 * KDROP_SEQUENCE; in KDROP_SEQUENCE num_stream = S >= 1 and seq_id_dev holds S unsigned ids on the device (both ignored in
 * KDROP_ELEMENT, as step is in KDROP_SEQUENCE).  The columns from cols up to the stride are never written.
 * KLSTM_ERR_ARG, before the first HIP call and with out untouched: rows or cols negative, a retention outside [2^-32, 1], salt >= 2^31,
 * an unknown mode, num_stream < 1 or a null seq_id_dev in KDROP_SEQUENCE; then, for a block that is not empty: a null in or out, a
 * stride below cols, an overlap.  rows == 0 or cols == 0 is KLSTM_OK and launches nothing. */
klstm_status kdrop_apply(const float *in, int in_stride, int rows, int cols, float *out, int out_stride, float retention,
                         unsigned long long seed, unsigned step, unsigned salt, int mode, int num_stream, const unsigned *seq_id_dev,
                         void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
