/* include/klstm_nlm.h -- the knlm_* entries of libklstm.so: rescoring of CTC n-best lists with an LSTM language model, the glue that
 * keeps that second pass on the device (the numpy twin: tests/ctc_nlm_ref.py).  A family of its own
 * next to the klstm_* entries of klstm.h: the same library, the same klstm_status, the same klstm_last_error().
 *
 * THE MODEL is run by the caller with calls of klstm.h: [an embedding Affine D x V] -> LstmProjectedStreams layers (engines of E
 * streams, klstm_propagate_inference) -> Affine V x R (klstm_affine_propagate).  V classes, V >= K: the classes 0 .. K - 1 are the
 * tokens of the CTC model, bos and eos are classes in [0, V) (eos < 0: no end term).  A Softmax behind the last Affine is folded
 * into knlm_score_rows: it takes the Affine's rows.
 *
 * THE LISTS are the arrays of klstm_ctc_nbest_rescore (klstm.h), read under the same contract: entry (s, q), se = s * list_n + q, is
 * LISTED when nbest_count[s] lies in [0, list_n] and q < nbest_count[s] (the slots beyond the count are never read), WELL FORMED
 * when it is listed, logp is finite, 0 <= len <= min(hyp_stride, max_len) and every token lies in [0, K); listed and not well
 * formed is DROPPED.
 *
 * THE SCORE of a well-formed entry with tokens y_0 .. y_{L-1}: inputs x_0 = bos, x_p = y_{p-1}; positions p = 0 .. L with an end
 * term (eos >= 0), p = 0 .. L - 1 without; targets tgt_p = y_p for p < L, eos at p = L; a_p the row of the last Affine after the net
 * has seen x_0 .. x_p from zero state;
 *     lp_p = (a_p[tgt_p] - max_j a_p[j]) - log(sum_j exp(a_p[j] - max))   as a float
 *     nlm_logp = sum_p (double)lp_p, p ascending;   units = L
 *     z = (double)am_scale * (double)logp + (double)nlm_scale * nlm_logp + (double)unit_bonus * units, left to right, then + 0.0
 * An entry whose nlm_logp is not finite is FORBIDDEN.  The entries that are neither dropped nor forbidden are ranked by z
 * descending, ties to the lower q.
 *
 * THE PLAN is fixed by numbers the host knows: the S * list_n flat entries go to the E streams in groups, group g holds the
 * entries se = g * E + e (first_entry = g * E); every group starts with all engine streams reset (klstm_reset) and runs
 * ceil((max_len + (eos >= 0)) / T) chunks of T positions, t0 = 0, T, 2 T, ...:
 *     knlm_pack -> klstm_propagate_inference per layer -> klstm_affine_propagate -> knlm_score_rows
 * and after the last group one knlm_rank.  An engine stream without an entry, a dropped or unlisted entry and every position past
 * an entry's last one get rows of zeros in and contribute nothing out.  Nothing is read back; no floating-point atomics; the
 * results are bit-identical from run to run.  All three calls are asynchronous on hip_stream.
 *
 * Limits: 1 <= S <= 32, 1 <= list_n <= 64, 0 <= max_len <= 1023, 2 <= K <= V <= 32768, 1 <= E <= 32, T >= 1, T * E <= 2^24,
 * 1 <= D <= 32768, 0 <= out_n <= list_n; beyond them KLSTM_ERR_SHAPE and nothing is launched (knlm_workspace_bytes answers 0).  A null
 * required pointer, a non-finite scale, bos or eos outside [0, V), first_entry outside [0, S * list_n), t0 < 0, a stride below its
 * row, a small or misaligned workspace: KLSTM_ERR_ARG with the outputs untouched.  Every check runs before the first HIP call. */
#ifndef KLSTM_NLM_H_
#define KLSTM_NLM_H_

#include "klstm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The engine input of one chunk.  Row t * E + e of out (T * E rows, out_stride floats apart) is position p = t0 + t of entry
 * first_entry + e: without an embedding (embed_W NULL) the one-hot of x_p over V columns; with embed_W [D x V] (row-major, Kaldi's
 * linearity_) and embed_bias [D] column x_p of embed_W plus the bias over D columns, a gather.  Rows without an input are zeros.
 * The columns beyond V (or D) are not touched. */
klstm_status knlm_pack(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                       int S, int list_n, int max_len, int K, int V, int bos, int eos, int first_entry, int E, int T, int t0,
                       const float *embed_W_dev, const float *embed_bias_dev, int D, float *out_dev, int out_stride, void *hip_stream);

/* The bytes knlm_score_rows needs for chunks of T positions of E streams (0 and a message beyond the limits). */
size_t knlm_workspace_bytes(int E, int T);

/* The rows a_dev [T * E x V] (a_stride floats apart) of the last Affine for the chunk knlm_pack made with the same entry arguments:
 * lp_p of every row whose position has a target, in one pass over the row that keeps its maximum, its sum and the target's value;
 * then, per entry, the chunk's values are added onto acc_dev [S * list_n] (doubles) with p ascending -- the chunk with t0 == 0 sets
 * the entry's accumulator instead (0 for an entry without a row).  positions_dev [S * list_n] (ints, may be NULL): the rows scored
 * of every entry, set and added likewise.  Entries outside this group are not touched. */
klstm_status knlm_score_rows(const float *a_dev, int a_stride, const int *hyp_dev, int hyp_stride, const int *hyp_len_dev,
                             const int *nbest_count_dev, const float *logp_dev, int S, int list_n, int max_len, int K, int V, int eos,
                             int first_entry, int E, int T, int t0, double *acc_dev, int *positions_dev, void *workspace,
                             size_t workspace_bytes, void *hip_stream);

/* The combination, the ranking and the re-ranked list.  acc_dev [S * list_n]: nlm_logp of every entry as knlm_score_rows left it.
 *   order_dev [S * list_n]       the entry of each rank; -1 from live_count[s] on
 *   live_count_dev [S]           the entries ranked
 *   score_dev [S * list_n]       float(z); -inf for a dropped, forbidden or unlisted entry
 *   nlm_logp_dev [S * list_n]    float(nlm_logp); -inf likewise (may be NULL)
 *   units_dev [S * list_n]       L of a well-formed entry, 0 otherwise (may be NULL)
 * With out_n > 0 the first min(live, out_n) entries of the ranking are gathered as klstm_ctc_nbest_rescore gathers them: out_hyp_dev
 * [S][out_n][out_stride], out_len_dev, out_score_dev [S][out_n], out_errors_dev (may be NULL; -1 without errors_dev), out_count_dev [S];
 * the slots beyond the count are left alone.  totals_dev (may be NULL): eight doubles the minibatch is ADDED to -- streams done,
 * streams idle or rejected, entries dropped, entries forbidden, streams whose 1-best changed, errors of the first pass's entry 0,
 * errors of the new 1-best, positions scored (L + (has_eos != 0) over the well-formed entries). */
klstm_status knlm_rank(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                       const int *errors_dev, int S, int list_n, int max_len, int K, const double *acc_dev, float am_scale,
                       float nlm_scale, float unit_bonus, int has_eos, int *order_dev, int *live_count_dev, float *score_dev,
                       float *nlm_logp_dev, int *units_dev, int out_n, int *out_hyp_dev, int out_stride, int *out_len_dev,
                       int *out_count_dev, float *out_score_dev, int *out_errors_dev, double *totals_dev, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
