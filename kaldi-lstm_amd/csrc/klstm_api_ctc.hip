// kaldi-lstm_amd/csrc/klstm_api_ctc.hip -- the klstm_ctc_* entries of include/klstm.h: the checks of every call, spelled once and fired
// in the order the tests pin, the notes about model blobs and MMI graphs kept per address, then one launcher of klstm_kernels.h each
// (the kernels are in klstm_ctc*.hip).
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>

#include "klstm_host.h"
#include "klstm_kernels.h"

using namespace klstm;

extern "C" {

// ---- the checks of the CTC entry points, spelled once; fn is the entry's name, which every message begins with ----
// the shape rule of the three workspace queries that take a label length (what: the entry's word for that length)
static bool ctc_query_ok(const char *fn, const char *what, int T, int S, int L) {
  if (T > 0 && S > 0 && S <= 32 && (long)T * S <= 65535 && L >= 0 && L <= 1023) return true;
  fail(KLSTM_ERR_SHAPE, "%s: T %d, streams %d, %s length %d outside T >= 1, 1 <= S <= 32, T * S <= 65535, L <= 1023", fn, T, S, what, L);
  return false;
}
// What the calls share, in the order it has always fired: sizes, limits (min_k: the fewest classes the call takes), the call's own
// finding about its pointers (null: none; where a call has several, the first to apply), blank, row stride (the smallest of the
// call's), its finding about aliasing, workspace alignment.
static klstm_status ctc_call_check(const char *fn, int T, int S, int K, int min_k, const char *pointers, int blank, int stride,
                                   const char *aliasing, const void *workspace) {
  if (T <= 0 || S <= 0 || K <= 0) return fail(KLSTM_ERR_ARG, "%s: bad size (T %d, streams %d, K %d)", fn, T, S, K);
  if (S > 32 || (long)T * S > 65535 || K < min_k || K > 32768)
    return fail(KLSTM_ERR_SHAPE, "%s: T %d, streams %d, K %d outside S <= 32, T * S <= 65535, %d <= K <= 32768", fn, T, S, K, min_k);
  if (pointers) return fail(KLSTM_ERR_ARG, "%s: %s", fn, pointers);
  if (blank < 0 || blank >= K) return fail(KLSTM_ERR_ARG, "%s: blank %d outside [0, %d)", fn, blank, K);
  if (stride < K) return fail(KLSTM_ERR_ARG, "%s: row stride below K (%d < %d)", fn, stride, K);
  if (aliasing) return fail(KLSTM_ERR_ARG, "%s: %s", fn, aliasing);
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: workspace must be 16-byte aligned", fn);
  return KLSTM_OK;
}
// the decoders' finding about their references: a pair, and what is counted against them needs them
static const char *ctc_refs_finding(const int *ref_labels_dev, const int *ref_offsets_dev, const int *errors_dev, const double *totals_dev) {
  if ((ref_labels_dev == nullptr) != (ref_offsets_dev == nullptr)) return "reference labels and offsets come together or not at all";
  if (!ref_labels_dev && (errors_dev || totals_dev)) return "errors / totals need reference labels";
  return nullptr;
}
size_t klstm_ctc_workspace_bytes(int T, int S, int max_label_len) {
  return ctc_query_ok("klstm_ctc_workspace_bytes", "label", T, S, max_label_len) ? ctc_workspace_bytes(T, S, max_label_len) : 0;
}
klstm_status klstm_ctc_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                            const int *label_offsets_dev, int blank, float *diff, int diff_stride, float *utt_loss_dev,
                            double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_eval";
  const bool null = !net_out || !lens_dev || !labels_dev || !label_offsets_dev || !diff || !utt_loss_dev || !workspace;
  const klstm_status st = ctc_call_check(fn, T, S, K, 1, null ? "null argument" : nullptr, blank, stride < diff_stride ? stride : diff_stride,
                                         net_out == diff ? "diff == net_out (the posteriors are read while diff is written)" : nullptr, workspace);
  if (st != KLSTM_OK) return st;
  const int lcap = ctc_label_capacity(T, S, workspace_bytes);
  if (lcap < 0) return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_workspace_bytes(%d, %d, 0)", fn, workspace_bytes, T, S);
  HIPCHK(launch_ctc(net_out, T, S, K, stride, lens_dev, labels_dev, label_offsets_dev, blank, diff, diff_stride, utt_loss_dev, totals_dev,
                    workspace, lcap, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
size_t klstm_ctc_decode_workspace_bytes(int T, int S, int max_ref_len) {
  return ctc_query_ok("klstm_ctc_decode_workspace_bytes", "reference", T, S, max_ref_len) ? ctc_decode_workspace_bytes(T, S) : 0;
}
klstm_status klstm_ctc_decode(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                              const float *class_weight_dev, int *hyp_dev, int *hyp_len_dev, float *score_dev, int *frame_class_dev,
                              const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev, double *totals_dev,
                              void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_decode";
  const char *pointers = ctc_refs_finding(ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev);
  if (!net_out || !lens_dev || !hyp_dev || !hyp_len_dev || !workspace) pointers = "null argument";
  const klstm_status st = ctc_call_check(fn, T, S, K, 2, pointers, blank, stride, nullptr, workspace);
  if (st != KLSTM_OK) return st;
  if (workspace_bytes < ctc_decode_workspace_bytes(T, S))
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_decode_workspace_bytes(%d, %d, .) = %zu", fn, workspace_bytes,
                T, S, ctc_decode_workspace_bytes(T, S));
  HIPCHK(launch_ctc_decode(net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, hyp_dev, hyp_len_dev, score_dev, frame_class_dev,
                           ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
static bool ctc_beam_shape_ok(int T, int S, int beam, int cands) {
  return T > 0 && S > 0 && S <= 32 && (long)T * S <= 65535 && beam >= 1 && beam <= 64 && cands >= 1 && cands <= 32;
}
size_t klstm_ctc_beam_workspace_bytes(int T, int S, int beam, int cands) {
  if (!ctc_beam_shape_ok(T, S, beam, cands)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_beam_workspace_bytes: T %d, streams %d, beam %d, candidates %d outside T >= 1, 1 <= S <= 32, T * S <= 65535, 1 <= beam <= 64, 1 <= candidates <= 32", T, S, beam, cands);
    return 0;
  }
  return ctc_beam_workspace_bytes(T, S, beam, cands);
}
// ---- sparse back-off models.  What a blob was built for is remembered per address, as for the MMI graphs below: the header lives
// on the device and the calls do not wait for it ----
struct SlmNote { int Q, A, K; size_t bytes; };
static std::mutex slm_mu;
static std::map<const void *, SlmNote> slm_blobs;
static bool ctc_slm_shape_ok(int states, int arcs, int K) {
  return states >= 1 && states <= (1 << 24) && arcs >= 1 && arcs <= (1 << 26) && K >= 2 && K <= 32768;
}
size_t klstm_ctc_slm_bytes(int states, int arcs, int K) {
  if (!ctc_slm_shape_ok(states, arcs, K)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_slm_bytes: %d states, %d arcs, %d classes outside 1 <= states <= 2^24, 1 <= arcs <= 2^26, 2 <= K <= 32768", states, arcs, K);
    return 0;
  }
  return ctc_slm_bytes(states, arcs);
}
klstm_status klstm_ctc_slm_build(int states, int arcs, int K, int blank, const int *arc_offsets_dev, const int *arc_labels_dev,
                                 const int *arc_next_dev, const float *arc_weight_dev, const int *backoff_dev, const float *backoff_weight_dev,
                                 void *slm, size_t slm_bytes, int *status_dev, void *hip_stream) {
  const char *fn = "klstm_ctc_slm_build";
  if (states <= 0 || arcs <= 0 || K <= 0) return fail(KLSTM_ERR_ARG, "%s: bad size (%d states, %d arcs, K %d)", fn, states, arcs, K);
  if (!ctc_slm_shape_ok(states, arcs, K))
    return fail(KLSTM_ERR_SHAPE, "%s: %d states, %d arcs, %d classes outside states <= 2^24, arcs <= 2^26, 2 <= K <= 32768", fn, states, arcs, K);
  if (!arc_offsets_dev || !arc_labels_dev || !arc_next_dev || !arc_weight_dev || !backoff_dev || !backoff_weight_dev || !slm)
    return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (blank < 0 || blank >= K) return fail(KLSTM_ERR_ARG, "%s: blank %d outside [0, %d)", fn, blank, K);
  if ((reinterpret_cast<uintptr_t>(slm) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: the model's buffer must be 16-byte aligned", fn);
  if (slm_bytes < ctc_slm_bytes(states, arcs))
    return fail(KLSTM_ERR_ARG, "%s: buffer of %zu bytes is below klstm_ctc_slm_bytes(%d, %d, %d) = %zu", fn, slm_bytes, states, arcs, K,
                ctc_slm_bytes(states, arcs));
  {
    std::lock_guard<std::mutex> lk(slm_mu);
    slm_blobs.erase(slm);
  }
  HIPCHK(launch_ctc_slm_build(states, arcs, K, blank, arc_offsets_dev, arc_labels_dev, arc_next_dev, arc_weight_dev, backoff_dev,
                              backoff_weight_dev, slm, status_dev, (hipStream_t)hip_stream));
  std::lock_guard<std::mutex> lk(slm_mu);
  slm_blobs[slm] = SlmNote{states, arcs, K, ctc_slm_bytes(states, arcs)};
  return KLSTM_OK;
}
// null: the blob serves a call with these sizes; else what is wrong with it
static const char *ctc_slm_finding(const void *slm, size_t slm_bytes, int lm_states, int K) {
  if (!slm) return "null sparse language model";
  std::lock_guard<std::mutex> lk(slm_mu);
  const auto it = slm_blobs.find(slm);
  if (it == slm_blobs.end()) return "no sparse language model was built at this address (klstm_ctc_slm_build)";
  if (it->second.Q != lm_states || it->second.K != K) return "the sparse language model was built for other states or classes";
  if (slm_bytes < it->second.bytes) return "the sparse language model's bytes are below klstm_ctc_slm_bytes";
  return nullptr;
}
// the checks and the launch behind klstm_ctc_beam_decode (Q = 0, no tables), klstm_ctc_beam_decode_lm (with_lm: 1 <= Q) and
// klstm_ctc_beam_decode_slm (slm_call: lm_next_dev is the blob, slm_bytes its size, 1 <= Q)
static klstm_status ctc_beam_decode_checked(const char *fn, bool with_lm, bool slm_call, size_t slm_bytes, const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                            const float *class_weight_dev, int beam, int cands, int nbest, int Q, const int *lm_next_dev,
                                            const float *lm_weight_dev, const float *lm_final_dev, int *hyp_dev, int *hyp_len_dev,
                                            int *nbest_count_dev, float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev,
                                            int *errors_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  if (T <= 0 || S <= 0 || K <= 0 || beam <= 0 || cands <= 0 || nbest <= 0)
    return fail(KLSTM_ERR_ARG, "%s: bad size (T %d, streams %d, K %d, beam %d, candidates %d, n-best %d)", fn, T, S, K, beam, cands, nbest);
  if (!ctc_beam_shape_ok(T, S, beam, cands) || K < 2 || K > 32768 || cands > K - 1 || nbest > beam)
    return fail(KLSTM_ERR_SHAPE, "%s: T %d, streams %d, K %d, beam %d, candidates %d, n-best %d outside S <= 32, T * S <= 65535, 2 <= K <= 32768, beam <= 64, candidates <= min(K - 1, 32), n-best <= beam",
                fn, T, S, K, beam, cands, nbest);
  if (slm_call && (Q < 1 || Q > (1 << 24)))
    return fail(KLSTM_ERR_SHAPE, "%s: %d language-model states outside 1 <= states <= 2^24", fn, Q);
  if (!slm_call && (Q < (with_lm ? 1 : 0) || (long)Q * K > (1L << 24)))
    return fail(KLSTM_ERR_SHAPE, "%s: %d language-model states of %d classes outside 1 <= states, states * K <= 2^24", fn, Q, K);
  const char *pointers = ctc_refs_finding(ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev);      // (the later one here fires first)
  if (slm_call) {
    const char *f = ctc_slm_finding(lm_next_dev, slm_bytes, Q, K);
    if (f) pointers = f;
  } else if (Q > 0 && (!lm_next_dev || !lm_weight_dev)) pointers = "the language model's next and weight tables come together";
  if (!net_out || !lens_dev || !hyp_dev || !hyp_len_dev || !nbest_count_dev || !workspace) pointers = "null argument";
  const klstm_status st = ctc_call_check(fn, T, S, K, 2, pointers, blank, stride, nullptr, workspace);
  if (st != KLSTM_OK) return st;
  if (workspace_bytes < ctc_beam_workspace_bytes(T, S, beam, cands))
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_beam_workspace_bytes(%d, %d, %d, %d) = %zu", fn, workspace_bytes,
                T, S, beam, cands, ctc_beam_workspace_bytes(T, S, beam, cands));
  if (slm_call) {
    HIPCHK(launch_ctc_beam_slm(net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, beam, cands, nbest, Q, lm_next_dev, lm_final_dev,
                               hyp_dev, hyp_len_dev, nbest_count_dev, score_dev, ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev,
                               workspace, (hipStream_t)hip_stream));
    return KLSTM_OK;
  }
  HIPCHK(launch_ctc_beam_lm(net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, beam, cands, nbest, Q, lm_next_dev, lm_weight_dev,
                            lm_final_dev, hyp_dev, hyp_len_dev, nbest_count_dev, score_dev, ref_labels_dev, ref_offsets_dev, errors_dev,
                            totals_dev, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_ctc_beam_decode(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                   const float *class_weight_dev, int beam, int cands, int nbest, int *hyp_dev, int *hyp_len_dev,
                                   int *nbest_count_dev, float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev,
                                   int *errors_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  return ctc_beam_decode_checked("klstm_ctc_beam_decode", false, false, 0, net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, beam, cands, nbest, 0,
                                 nullptr, nullptr, nullptr, hyp_dev, hyp_len_dev, nbest_count_dev, score_dev, ref_labels_dev, ref_offsets_dev,
                                 errors_dev, totals_dev, workspace, workspace_bytes, hip_stream);
}
klstm_status klstm_ctc_beam_decode_lm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                      const float *class_weight_dev, int beam, int cands, int nbest, int lm_states, const int *lm_next_dev,
                                      const float *lm_weight_dev, const float *lm_final_dev, int *hyp_dev, int *hyp_len_dev,
                                      int *nbest_count_dev, float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev,
                                      int *errors_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  return ctc_beam_decode_checked("klstm_ctc_beam_decode_lm", true, false, 0, net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, beam, cands, nbest,
                                 lm_states, lm_next_dev, lm_weight_dev, lm_final_dev, hyp_dev, hyp_len_dev, nbest_count_dev, score_dev,
                                 ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev, workspace, workspace_bytes, hip_stream);
}
klstm_status klstm_ctc_beam_decode_slm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank,
                                       const float *class_weight_dev, int beam, int cands, int nbest, const void *slm, size_t slm_bytes,
                                       int lm_states, const float *lm_final_dev, int *hyp_dev, int *hyp_len_dev, int *nbest_count_dev,
                                       float *score_dev, const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev,
                                       double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  return ctc_beam_decode_checked("klstm_ctc_beam_decode_slm", true, true, slm_bytes, net_out, T, S, K, stride, lens_dev, blank, class_weight_dev, beam,
                                 cands, nbest, lm_states, reinterpret_cast<const int *>(slm), nullptr, lm_final_dev, hyp_dev, hyp_len_dev,
                                 nbest_count_dev, score_dev, ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev, workspace, workspace_bytes,
                                 hip_stream);
}
int klstm_ctc_beam_lm_resident(int lm_states, int K, int beam, int cands) {
  if (lm_states < 1 || K < 2 || (long)lm_states * K > (1L << 24)) return 0;
  return ctc_beam_lm_resident(lm_states, K, beam, cands) ? 1 : 0;
}
static bool ctc_beam_stream_state_ok(int max_frames, int S, int beam) {
  return max_frames >= 1 && S >= 1 && S <= 32 && beam >= 1 && beam <= 64 && (long)max_frames * beam + 1 < (1L << 31);
}
size_t klstm_ctc_beam_stream_state_bytes(int max_frames, int S, int beam) {
  if (!ctc_beam_stream_state_ok(max_frames, S, beam)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_beam_stream_state_bytes: %d frames, streams %d, beam %d outside 1 <= frames, 1 <= S <= 32, 1 <= beam <= 64, frames * beam + 1 < 2^31", max_frames, S, beam);
    return 0;
  }
  return ctc_beam_stream_state_bytes(max_frames, S, beam);
}
size_t klstm_ctc_beam_stream_workspace_bytes(int T, int S, int cands, int nbest) {
  if (!ctc_beam_shape_ok(T, S, 1, cands) || nbest < 1 || nbest > 64) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_beam_stream_workspace_bytes: T %d, streams %d, candidates %d, n-best %d outside T >= 1, 1 <= S <= 32, T * S <= 65535, 1 <= candidates <= 32, 1 <= n-best <= 64", T, S, cands, nbest);
    return 0;
  }
  return ctc_beam_stream_workspace_bytes(T, S, cands, nbest);
}
// what step and emit check alike about the state
static klstm_status ctc_beam_stream_state_check(const char *fn, int S, int beam, const void *state, size_t state_bytes, int max_frames) {
  if (!ctc_beam_stream_state_ok(max_frames, S, beam))
    return fail(KLSTM_ERR_SHAPE, "%s: %d frames, streams %d, beam %d outside 1 <= frames, S <= 32, beam <= 64, frames * beam + 1 < 2^31", fn, max_frames, S, beam);
  if (!state) return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if ((reinterpret_cast<uintptr_t>(state) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: state must be 16-byte aligned", fn);
  if (state_bytes < ctc_beam_stream_state_bytes(max_frames, S, beam))
    return fail(KLSTM_ERR_ARG, "%s: state of %zu bytes is below klstm_ctc_beam_stream_state_bytes(%d, %d, %d) = %zu", fn, state_bytes, max_frames, S,
                beam, ctc_beam_stream_state_bytes(max_frames, S, beam));
  return KLSTM_OK;
}
// the checks and the launch behind klstm_ctc_beam_stream_step and klstm_ctc_beam_stream_step_slm (slm_call: lm_next_dev is the blob,
// slm_bytes its size, 1 <= lm_states)
static klstm_status ctc_beam_stream_step_checked(const char *fn, bool slm_call, size_t slm_bytes, const float *net_out, int T, int S, int K, int stride,
                                                 const int *lens_dev, const int *start_dev, int blank, const float *class_weight_dev, int beam,
                                                 int cands, int lm_states, const int *lm_next_dev, const float *lm_weight_dev, void *state,
                                                 size_t state_bytes, int max_frames, void *workspace, size_t workspace_bytes, void *hip_stream) {
  if (T <= 0 || S <= 0 || K <= 0 || beam <= 0 || cands <= 0)
    return fail(KLSTM_ERR_ARG, "%s: bad size (T %d, streams %d, K %d, beam %d, candidates %d)", fn, T, S, K, beam, cands);
  if (!ctc_beam_shape_ok(T, S, beam, cands) || K < 2 || K > 32768 || cands > K - 1)
    return fail(KLSTM_ERR_SHAPE, "%s: T %d, streams %d, K %d, beam %d, candidates %d outside S <= 32, T * S <= 65535, 2 <= K <= 32768, beam <= 64, candidates <= min(K - 1, 32)",
                fn, T, S, K, beam, cands);
  if (slm_call ? (lm_states < 1 || lm_states > (1 << 24)) : (lm_states < 0 || (long)lm_states * K > (1L << 24)))
    return fail(KLSTM_ERR_SHAPE, slm_call ? "%s: %d language-model states (%d classes) outside 1 <= states <= 2^24"
                                          : "%s: %d language-model states of %d classes outside 0 <= states, states * K <= 2^24", fn, lm_states, K);
  klstm_status st = ctc_beam_stream_state_check(fn, S, beam, state, state_bytes, max_frames);
  if (st != KLSTM_OK) return st;
  const char *pointers = nullptr;
  if (slm_call) pointers = ctc_slm_finding(lm_next_dev, slm_bytes, lm_states, K);
  else if (lm_states > 0 && (!lm_next_dev || !lm_weight_dev)) pointers = "the language model's next and weight tables come together";
  if (!net_out || !lens_dev || !workspace) pointers = "null argument";
  st = ctc_call_check(fn, T, S, K, 2, pointers, blank, stride, nullptr, workspace);
  if (st != KLSTM_OK) return st;
  if (workspace_bytes < ctc_beam_stream_workspace_bytes(T, S, cands, 1))
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_beam_stream_workspace_bytes(%d, %d, %d, .) = %zu", fn, workspace_bytes,
                T, S, cands, ctc_beam_stream_workspace_bytes(T, S, cands, 1));
  HIPCHK(launch_ctc_beam_stream_step(net_out, T, S, K, stride, lens_dev, start_dev, blank, class_weight_dev, beam, cands, lm_states, lm_next_dev,
                                     lm_weight_dev, slm_call, state, max_frames, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
klstm_status klstm_ctc_beam_stream_step(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *start_dev,
                                        int blank, const float *class_weight_dev, int beam, int cands, int lm_states,
                                        const int *lm_next_dev, const float *lm_weight_dev, void *state, size_t state_bytes, int max_frames,
                                        void *workspace, size_t workspace_bytes, void *hip_stream) {
  return ctc_beam_stream_step_checked("klstm_ctc_beam_stream_step", false, 0, net_out, T, S, K, stride, lens_dev, start_dev, blank, class_weight_dev,
                                      beam, cands, lm_states, lm_next_dev, lm_weight_dev, state, state_bytes, max_frames, workspace,
                                      workspace_bytes, hip_stream);
}
klstm_status klstm_ctc_beam_stream_step_slm(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *start_dev,
                                            int blank, const float *class_weight_dev, int beam, int cands, const void *slm, size_t slm_bytes,
                                            int lm_states, void *state, size_t state_bytes, int max_frames, void *workspace,
                                            size_t workspace_bytes, void *hip_stream) {
  return ctc_beam_stream_step_checked("klstm_ctc_beam_stream_step_slm", true, slm_bytes, net_out, T, S, K, stride, lens_dev, start_dev, blank,
                                      class_weight_dev, beam, cands, lm_states, reinterpret_cast<const int *>(slm), nullptr, state, state_bytes,
                                      max_frames, workspace, workspace_bytes, hip_stream);
}
klstm_status klstm_ctc_beam_stream_emit(int S, int K, int blank, int beam, int nbest, const int *mode_dev, int lm_states,
                                        const float *lm_final_dev, const void *state, size_t state_bytes, int max_frames, int *hyp_dev,
                                        int hyp_stride, int *hyp_len_dev, int *nbest_count_dev, float *score_dev, int *frames_dev,
                                        int *stable_len_dev, const int *ref_labels_dev, const int *ref_offsets_dev, int *errors_dev,
                                        double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_beam_stream_emit";
  if (S <= 0 || K <= 0 || beam <= 0 || nbest <= 0)
    return fail(KLSTM_ERR_ARG, "%s: bad size (streams %d, K %d, beam %d, n-best %d)", fn, S, K, beam, nbest);
  if (S > 32 || K < 2 || K > 32768 || beam > 64 || nbest > beam)
    return fail(KLSTM_ERR_SHAPE, "%s: streams %d, K %d, beam %d, n-best %d outside S <= 32, 2 <= K <= 32768, beam <= 64, n-best <= beam", fn, S, K, beam, nbest);
  if (lm_states < 0 || (long)lm_states * K > (1L << 24))
    return fail(KLSTM_ERR_SHAPE, "%s: %d language-model states of %d classes outside 0 <= states, states * K <= 2^24", fn, lm_states, K);
  if (ctc_beam_stream_state_ok(max_frames, S, beam) && hyp_stride < max_frames)      // (every limit before any pointer)
    return fail(KLSTM_ERR_SHAPE, "%s: hypothesis stride %d below the %d frames of the state", fn, hyp_stride, max_frames);
  klstm_status st = ctc_beam_stream_state_check(fn, S, beam, state, state_bytes, max_frames);
  if (st != KLSTM_OK) return st;
  const char *pointers = ctc_refs_finding(ref_labels_dev, ref_offsets_dev, errors_dev, totals_dev);
  if (!mode_dev || !hyp_dev || !hyp_len_dev || !nbest_count_dev || !workspace) pointers = "null argument";
  if (pointers) return fail(KLSTM_ERR_ARG, "%s: %s", fn, pointers);
  if (blank < 0 || blank >= K) return fail(KLSTM_ERR_ARG, "%s: blank %d outside [0, %d)", fn, blank, K);
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: workspace must be 16-byte aligned", fn);
  if (workspace_bytes < ctc_beam_stream_emit_workspace_bytes())
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_beam_stream_workspace_bytes(1, %d, 1, .) = %zu", fn, workspace_bytes, S,
                ctc_beam_stream_workspace_bytes(1, S, 1, 1));
  HIPCHK(launch_ctc_beam_stream_emit(S, K, blank, beam, nbest, mode_dev, lm_states, lm_final_dev, state, max_frames, hyp_dev, hyp_stride,
                                     hyp_len_dev, nbest_count_dev, score_dev, frames_dev, stable_len_dev, ref_labels_dev, ref_offsets_dev,
                                     errors_dev, totals_dev, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
static bool ctc_mbr_shape_ok(int T, int S, int list_n, int max_len) {
  return T > 0 && S > 0 && S <= 32 && (long)T * S <= 65535 && list_n >= 1 && list_n <= 16 && max_len >= 0 && max_len <= 1023;
}
size_t klstm_ctc_mbr_workspace_bytes(int T, int S, int list_n, int max_len, int with_ref) {
  if (!ctc_mbr_shape_ok(T, S, list_n, max_len)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_mbr_workspace_bytes: T %d, streams %d, list of %d, labelling length %d outside T >= 1, 1 <= S <= 32, T * S <= 65535, 1 <= list <= 16, L <= 1023", T, S, list_n, max_len);
    return 0;
  }
  return ctc_mbr_workspace_bytes(T, S, list_n, max_len, with_ref != 0);
}
klstm_status klstm_ctc_mbr_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, int blank, const int *hyp_dev,
                                int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const int *errors_dev, int list_n,
                                const int *ref_labels_dev, const int *ref_offsets_dev, float risk_scale, float ctc_weight, float *diff,
                                int diff_stride, float *risk_dev, float *hyp_logp_dev, float *hyp_post_dev, float *ref_loss_dev,
                                double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_mbr_eval";
  if (T <= 0 || S <= 0 || K <= 0 || list_n <= 0 || hyp_stride <= 0)
    return fail(KLSTM_ERR_ARG, "%s: bad size (T %d, streams %d, K %d, list of %d, hypothesis stride %d)", fn, T, S, K, list_n, hyp_stride);
  if (list_n > 16) return fail(KLSTM_ERR_SHAPE, "%s: list of %d outside 1 <= list <= 16", fn, list_n);
  if (!(risk_scale > 0.f) || !std::isfinite(risk_scale)) return fail(KLSTM_ERR_ARG, "%s: risk scale %g is not a finite number above 0", fn, (double)risk_scale);
  if (!(ctc_weight >= 0.f) || !std::isfinite(ctc_weight)) return fail(KLSTM_ERR_ARG, "%s: CTC weight %g is not a finite number >= 0", fn, (double)ctc_weight);
  const bool with_ref = ctc_weight > 0.f;
  const char *pointers = nullptr;
  if ((ref_labels_dev == nullptr) != (ref_offsets_dev == nullptr)) pointers = "reference labels and offsets come together or not at all";
  else if ((ref_labels_dev != nullptr) != with_ref) pointers = "the reference is given exactly when the CTC weight is above 0";
  if (!net_out || !lens_dev || !hyp_dev || !hyp_len_dev || !nbest_count_dev || !errors_dev || !diff || !risk_dev || !workspace) pointers = "null argument";
  const klstm_status st = ctc_call_check(fn, T, S, K, 2, pointers, blank, stride < diff_stride ? stride : diff_stride,
                                         net_out == diff ? "diff == net_out (the posteriors are read while diff is written)" : nullptr, workspace);
  if (st != KLSTM_OK) return st;
  const int lcap = ctc_mbr_label_capacity(T, S, list_n, with_ref, workspace_bytes);
  if (lcap < 0)
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_mbr_workspace_bytes(%d, %d, %d, 0, %d) = %zu", fn, workspace_bytes, T, S,
                list_n, (int)with_ref, ctc_mbr_workspace_bytes(T, S, list_n, 0, with_ref));
  HIPCHK(launch_ctc_mbr(net_out, T, S, K, stride, lens_dev, blank, hyp_dev, hyp_stride, hyp_len_dev, nbest_count_dev, errors_dev, list_n,
                        ref_labels_dev, ref_offsets_dev, risk_scale, ctc_weight, diff, diff_stride, risk_dev, hyp_logp_dev, hyp_post_dev,
                        ref_loss_dev, totals_dev, workspace, lcap, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
// ---- calls over n-best lists (the consensus, the rescoring): the checks they share, each fired from the place it always had ----
static bool ctc_nbest_shape_ok(int S, int list_n, int max_len) {
  return S >= 1 && S <= 32 && list_n >= 1 && list_n <= 64 && max_len >= 0 && max_len <= 1023;
}
struct CtcNbestCall {
  const char *fn; int S, list_n, max_len, hyp_stride;
  klstm_status shape() const {                                     // every limit before any pointer
    if (ctc_nbest_shape_ok(S, list_n, max_len)) return KLSTM_OK;
    return fail(KLSTM_ERR_SHAPE, "%s: streams %d, list of %d, length %d outside 1 <= S <= 32, 1 <= list <= 64, 0 <= L <= 1023", fn, S, list_n, max_len);
  }
  klstm_status strides(const char *what, int out_stride, bool written = true) const {      // of hyp, and of the output of whole entries
    if (hyp_stride > 0 && !(written && out_stride < (hyp_stride < max_len ? hyp_stride : max_len))) return KLSTM_OK;
    return fail(KLSTM_ERR_ARG, "%s: hypothesis stride %d, %s stride %d (at least min(hypothesis stride, length %d))", fn, hyp_stride, what, out_stride, max_len);
  }
  klstm_status workspace(const void *ws, size_t bytes, const char *size_fn, int word_mode, size_t need) const {      // alignment, then size
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: workspace must be 16-byte aligned", fn);
    if (bytes >= need) return KLSTM_OK;
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below %s(%d, %d, %d, %d) = %zu", fn, bytes, size_fn, S, list_n, max_len, word_mode, need);
  }
};
size_t klstm_ctc_consensus_workspace_bytes(int S, int list_n, int max_len, int word_mode) {
  if (!ctc_nbest_shape_ok(S, list_n, max_len)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_consensus_workspace_bytes: streams %d, list of %d, length %d outside 1 <= S <= 32, 1 <= list <= 64, 0 <= L <= 1023", S, list_n, max_len);
    return 0;
  }
  return ctc_consensus_workspace_bytes(S, list_n, max_len, word_mode != 0);
}
klstm_status klstm_ctc_consensus(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                                 const int *errors_dev, int S, int list_n, int max_len, float scale, int separator, int pivot_mode,
                                 int *pick_dev, int *map_dev, int *mbr_dev, float *post_dev, float *risk_dev, int *unit_len_dev,
                                 float *conf_dev, int conf_stride, int *dist_dev, double *totals_dev, void *workspace, size_t workspace_bytes,
                                 void *hip_stream) {
  const char *fn = "klstm_ctc_consensus";
  const CtcNbestCall call{fn, S, list_n, max_len, hyp_stride};
  if (klstm_status st = call.shape(); st != KLSTM_OK) return st;
  if (klstm_status st = call.strides("confidence", conf_stride); st != KLSTM_OK) return st;
  if (!(scale > 0.f) || !std::isfinite(scale)) return fail(KLSTM_ERR_ARG, "%s: scale %g is not a finite number above 0", fn, (double)scale);
  if (pivot_mode != 0 && pivot_mode != 1) return fail(KLSTM_ERR_ARG, "%s: pivot mode %d is neither 0 (MAP) nor 1 (MBR)", fn, pivot_mode);
  if (!hyp_dev || !hyp_len_dev || !nbest_count_dev || !logp_dev || !pick_dev || !map_dev || !mbr_dev || !post_dev || !risk_dev || !unit_len_dev ||
      !conf_dev || !workspace)
    return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (klstm_status st = call.workspace(workspace, workspace_bytes, "klstm_ctc_consensus_workspace_bytes", separator >= 0,
                                       ctc_consensus_workspace_bytes(S, list_n, max_len, separator >= 0)); st != KLSTM_OK) return st;
  HIPCHK(launch_ctc_consensus(hyp_dev, hyp_stride, hyp_len_dev, nbest_count_dev, logp_dev, errors_dev, S, list_n, max_len, scale, separator,
                              pivot_mode, pick_dev, map_dev, mbr_dev, post_dev, risk_dev, unit_len_dev, conf_dev, conf_stride, dist_dev,
                              totals_dev, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
// ---- second-pass rescoring of n-best lists.  The models are blobs of klstm_ctc_slm_build, known by their addresses ----
size_t klstm_ctc_rescore_workspace_bytes(int S, int list_n, int max_len, int word_mode) {
  if (!ctc_nbest_shape_ok(S, list_n, max_len)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_rescore_workspace_bytes: streams %d, list of %d, length %d outside 1 <= S <= 32, 1 <= list <= 64, 0 <= L <= 1023", S, list_n, max_len);
    return 0;
  }
  return ctc_rescore_workspace_bytes(S, list_n, max_len, word_mode != 0);
}
klstm_status klstm_ctc_nbest_rescore(const int *hyp_dev, int hyp_stride, const int *hyp_len_dev, const int *nbest_count_dev, const float *logp_dev,
                                     const int *errors_dev, int S, int list_n, int max_len, int K, const void *sub_slm, size_t sub_bytes,
                                     int sub_states, const float *sub_final_dev, const void *add_slm, size_t add_bytes, int add_states,
                                     int add_classes, const float *add_final_dev, const unsigned long long *word_keys_dev,
                                     const int *word_ids_dev, int num_words, int unk_id, int separator, int add_reserved, float am_scale,
                                     float add_scale, float unit_bonus, int *order_dev, int *live_count_dev, float *score_dev,
                                     float *add_logp_dev, float *sub_logp_dev, int *units_dev, int *oov_dev, int out_n, int *out_hyp_dev,
                                     int out_stride, int *out_len_dev, int *out_count_dev, float *out_score_dev, int *out_errors_dev,
                                     double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_nbest_rescore";
  const CtcNbestCall call{fn, S, list_n, max_len, hyp_stride};
  if (klstm_status st = call.shape(); st != KLSTM_OK) return st;
  if (K < 2 || K > 32768) return fail(KLSTM_ERR_SHAPE, "%s: %d classes outside 2 <= K <= 32768", fn, K);
  if (num_words < 0 || num_words > (1 << 24)) return fail(KLSTM_ERR_SHAPE, "%s: %d words outside 0 <= words <= 2^24", fn, num_words);
  if (out_n < 0 || out_n > list_n) return fail(KLSTM_ERR_SHAPE, "%s: a list of %d out of a list of %d", fn, out_n, list_n);
  if (!hyp_dev || !hyp_len_dev || !nbest_count_dev || !logp_dev || !order_dev || !live_count_dev || !score_dev || !workspace)
    return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (out_n >= 1 && (!out_hyp_dev || !out_len_dev || !out_count_dev || !out_score_dev))
    return fail(KLSTM_ERR_ARG, "%s: null list output with out_n %d", fn, out_n);
  if (klstm_status st = call.strides("output", out_stride, out_n >= 1); st != KLSTM_OK) return st;
  if (!std::isfinite(am_scale) || !std::isfinite(add_scale) || !std::isfinite(unit_bonus))
    return fail(KLSTM_ERR_ARG, "%s: scales %g, %g and bonus %g must be finite", fn, (double)am_scale, (double)add_scale, (double)unit_bonus);
  if (!sub_slm && !add_slm) return fail(KLSTM_ERR_ARG, "%s: neither a model to subtract nor one to add", fn);
  if (num_words > 0 && !add_slm) return fail(KLSTM_ERR_ARG, "%s: a word table without a model to add", fn);
  if (num_words > 0) {
    if (!word_keys_dev || !word_ids_dev) return fail(KLSTM_ERR_ARG, "%s: null word table", fn);
    if (separator < 0 || separator >= K) return fail(KLSTM_ERR_ARG, "%s: separator %d outside [0, %d)", fn, separator, K);
    if (add_reserved < 0 || add_reserved >= add_classes || unk_id >= add_classes || unk_id == add_reserved)
      return fail(KLSTM_ERR_ARG, "%s: reserved class %d, unknown-word class %d with %d word classes", fn, add_reserved, unk_id, add_classes);
  } else if (add_slm && add_classes != K) {
    return fail(KLSTM_ERR_ARG, "%s: a token-level model of %d classes over %d classes", fn, add_classes, K);
  }
  if (sub_slm) {
    const char *f = ctc_slm_finding(sub_slm, sub_bytes, sub_states, K);
    if (f) return fail(KLSTM_ERR_ARG, "%s: sub: %s", fn, f);
  }
  if (add_slm) {
    const char *f = ctc_slm_finding(add_slm, add_bytes, add_states, add_classes);
    if (f) return fail(KLSTM_ERR_ARG, "%s: add: %s", fn, f);
  }
  if (klstm_status st = call.workspace(workspace, workspace_bytes, "klstm_ctc_rescore_workspace_bytes", num_words > 0,
                                       ctc_rescore_workspace_bytes(S, list_n, max_len, num_words > 0)); st != KLSTM_OK) return st;
  HIPCHK(launch_ctc_rescore(hyp_dev, hyp_stride, hyp_len_dev, nbest_count_dev, logp_dev, errors_dev, S, list_n, max_len, K, sub_slm, sub_states,
                            sub_final_dev, add_slm, add_states, add_classes, add_final_dev, word_keys_dev, word_ids_dev, num_words, unk_id,
                            separator, add_reserved, am_scale, add_scale, unit_bonus, order_dev, live_count_dev, score_dev, add_logp_dev,
                            sub_logp_dev, units_dev, oov_dev, out_n, out_hyp_dev, out_stride, out_len_dev, out_count_dev, out_score_dev,
                            out_errors_dev, totals_dev, workspace, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
// ---- MMI against a label-LM denominator.  What a graph was built for is remembered per address: the header lives on the device and
// the calls do not wait for it, so klstm_ctc_mmi_eval knows a graph by where klstm_ctc_mmi_graph_build put it ----
struct MmiGraphNote { int Q, K, blank; };
static std::mutex mmi_graph_mu;
static std::map<const void *, MmiGraphNote> mmi_graphs;
static bool ctc_mmi_lm_ok(int lm_states, int K) { return lm_states >= 1 && K >= 2 && (long)lm_states * K <= 16384; }
size_t klstm_ctc_mmi_graph_bytes(int lm_states, int K) {
  if (!ctc_mmi_lm_ok(lm_states, K)) {
    fail(KLSTM_ERR_SHAPE, "klstm_ctc_mmi_graph_bytes: %d language-model states of %d classes outside 1 <= states, 2 <= K, states * K <= 16384", lm_states, K);
    return 0;
  }
  return ctc_mmi_graph_bytes(lm_states, K);
}
klstm_status klstm_ctc_mmi_graph_build(int lm_states, int K, int blank, const int *lm_next_dev, const float *lm_weight_dev,
                                       const float *lm_final_dev, void *graph, size_t graph_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_mmi_graph_build";
  if (lm_states <= 0 || K <= 0) return fail(KLSTM_ERR_ARG, "%s: bad size (%d language-model states, K %d)", fn, lm_states, K);
  if (!ctc_mmi_lm_ok(lm_states, K))
    return fail(KLSTM_ERR_SHAPE, "%s: %d language-model states of %d classes outside 2 <= K, states * K <= 16384", fn, lm_states, K);
  if (!lm_next_dev || !lm_weight_dev || !graph) return fail(KLSTM_ERR_ARG, "%s: null argument", fn);
  if (blank < 0 || blank >= K) return fail(KLSTM_ERR_ARG, "%s: blank %d outside [0, %d)", fn, blank, K);
  if ((reinterpret_cast<uintptr_t>(graph) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: graph must be 16-byte aligned", fn);
  if (graph_bytes < ctc_mmi_graph_bytes(lm_states, K))
    return fail(KLSTM_ERR_ARG, "%s: graph of %zu bytes is below klstm_ctc_mmi_graph_bytes(%d, %d) = %zu", fn, graph_bytes, lm_states, K,
                ctc_mmi_graph_bytes(lm_states, K));
  {
    std::lock_guard<std::mutex> lk(mmi_graph_mu);
    mmi_graphs.erase(graph);
  }
  HIPCHK(launch_ctc_mmi_graph(lm_states, K, blank, lm_next_dev, lm_weight_dev, lm_final_dev, graph, (hipStream_t)hip_stream));
  std::lock_guard<std::mutex> lk(mmi_graph_mu);
  mmi_graphs[graph] = MmiGraphNote{lm_states, K, blank};
  return KLSTM_OK;
}
size_t klstm_ctc_mmi_workspace_bytes(int T, int S, int K, int lm_states, int max_label_len) {
  const char *fn = "klstm_ctc_mmi_workspace_bytes";
  if (!ctc_query_ok(fn, "label", T, S, max_label_len)) return 0;
  if (!ctc_mmi_lm_ok(lm_states, K)) {
    fail(KLSTM_ERR_SHAPE, "%s: %d language-model states of %d classes outside 1 <= states, 2 <= K, states * K <= 16384", fn, lm_states, K);
    return 0;
  }
  return ctc_mmi_workspace_bytes(T, S, K, lm_states, max_label_len);
}
klstm_status klstm_ctc_mmi_eval(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                                const int *label_offsets_dev, int blank, const void *graph, size_t graph_bytes, int lm_states,
                                float ctc_weight, float *diff, int diff_stride, float *loss_dev, float *num_logp_dev, float *den_logz_dev,
                                float *lm_logw_dev, double *totals_dev, void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_mmi_eval";
  if (T <= 0 || S <= 0 || K <= 0 || lm_states <= 0) return fail(KLSTM_ERR_ARG, "%s: bad size (T %d, streams %d, K %d, %d language-model states)", fn, T, S, K, lm_states);
  if (!ctc_mmi_lm_ok(lm_states, K))
    return fail(KLSTM_ERR_SHAPE, "%s: %d language-model states of %d classes outside 2 <= K, states * K <= 16384", fn, lm_states, K);
  if (!(ctc_weight >= 0.f) || !std::isfinite(ctc_weight)) return fail(KLSTM_ERR_ARG, "%s: CTC weight %g is not a finite number >= 0", fn, (double)ctc_weight);
  const bool null = !net_out || !lens_dev || !labels_dev || !label_offsets_dev || !graph || !diff || !loss_dev || !workspace;
  const klstm_status st = ctc_call_check(fn, T, S, K, 2, null ? "null argument" : nullptr, blank, stride < diff_stride ? stride : diff_stride,
                                         net_out == diff ? "diff == net_out (the posteriors are read while diff is written)" : nullptr, workspace);
  if (st != KLSTM_OK) return st;
  if ((reinterpret_cast<uintptr_t>(graph) & 15) != 0) return fail(KLSTM_ERR_ARG, "%s: graph must be 16-byte aligned", fn);
  if (graph_bytes < ctc_mmi_graph_bytes(lm_states, K))
    return fail(KLSTM_ERR_ARG, "%s: graph of %zu bytes is below klstm_ctc_mmi_graph_bytes(%d, %d) = %zu", fn, graph_bytes, lm_states, K,
                ctc_mmi_graph_bytes(lm_states, K));
  {
    std::lock_guard<std::mutex> lk(mmi_graph_mu);
    const auto it = mmi_graphs.find(graph);
    if (it == mmi_graphs.end()) return fail(KLSTM_ERR_ARG, "%s: no graph was built at this address (klstm_ctc_mmi_graph_build)", fn);
    if (it->second.Q != lm_states || it->second.K != K || it->second.blank != blank)
      return fail(KLSTM_ERR_ARG, "%s: the graph was built for %d states, K %d, blank %d, not for %d states, K %d, blank %d", fn, it->second.Q,
                  it->second.K, it->second.blank, lm_states, K, blank);
  }
  const int lcap = ctc_mmi_label_capacity(T, S, K, lm_states, workspace_bytes);
  if (lcap < 0)
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_mmi_workspace_bytes(%d, %d, %d, %d, 0) = %zu", fn, workspace_bytes, T, S,
                K, lm_states, ctc_mmi_workspace_bytes(T, S, K, lm_states, 0));
  HIPCHK(launch_ctc_mmi(net_out, T, S, K, stride, lens_dev, labels_dev, label_offsets_dev, blank, graph, lm_states, ctc_weight, diff,
                        diff_stride, loss_dev, num_logp_dev, den_logz_dev, lm_logw_dev, totals_dev, workspace, lcap, (hipStream_t)hip_stream));
  return KLSTM_OK;
}
size_t klstm_ctc_align_workspace_bytes(int T, int S, int max_label_len) {
  return ctc_query_ok("klstm_ctc_align_workspace_bytes", "label", T, S, max_label_len) ? ctc_align_workspace_bytes(T, S, max_label_len) : 0;
}
klstm_status klstm_ctc_align(const float *net_out, int T, int S, int K, int stride, const int *lens_dev, const int *labels_dev,
                             const int *label_offsets_dev, int blank, const float *class_weight_dev, int *frame_class_dev,
                             int *frame_pos_dev, int *token_begin_dev, int *token_end_dev, float *score_dev, double *totals_dev,
                             void *workspace, size_t workspace_bytes, void *hip_stream) {
  const char *fn = "klstm_ctc_align";
  const char *pointers = (token_begin_dev == nullptr) != (token_end_dev == nullptr) ? "token begins and ends come together or not at all" : nullptr;
  if (!net_out || !lens_dev || !labels_dev || !label_offsets_dev || !frame_class_dev || !workspace) pointers = "null argument";
  const klstm_status st = ctc_call_check(fn, T, S, K, 2, pointers, blank, stride, nullptr, workspace);
  if (st != KLSTM_OK) return st;
  const int lcap = ctc_align_label_capacity(T, S, workspace_bytes);
  if (lcap < 0)
    return fail(KLSTM_ERR_ARG, "%s: workspace of %zu bytes is below klstm_ctc_align_workspace_bytes(%d, %d, 0) = %zu", fn, workspace_bytes, T, S,
                ctc_align_workspace_bytes(T, S, 0));
  HIPCHK(launch_ctc_align(net_out, T, S, K, stride, lens_dev, labels_dev, label_offsets_dev, blank, class_weight_dev, frame_class_dev,
                          frame_pos_dev, token_begin_dev, token_end_dev, score_dev, totals_dev, workspace, lcap, (hipStream_t)hip_stream));
  return KLSTM_OK;
}

}  // extern "C"
