// kaldi-lstm_amd/csrc/klstm_rnnt_decode.hip -- greedy (best-path) RNN-transducer decoding: the krnnt_greedy_* entries of
// include/klstm_rnnt.h (which states the algorithm; the torch yardstick: tests/rnnt_greedy_ref.py) and their kernels.
// The search is label-synchronous: in step u every live stream has emitted u labels, its predictor row is fixed, and ALL its remaining
// frames are scanned against that one row at once -- the 16 t x one u tile of joint_logits() (klstm_rnnt_dev.h), 16 frames per M-tile.
//   k_rnnt_greedy_begin    one wave, one thread per stream: status, t_s = 0, score 0, no labels, hit_chunk; the bos input rows.
//   k_rnnt_greedy_scan     grid (ceil(T / FB), S), 4 waves; FB = 64 frames per workgroup for J <= 512 (wave w owns frames 16 w .. 16 w +
//                          15), 32 for J > 512 (waves 2 and 3 only help to load the W panels: their products are discarded).  The
//                          chunk's enc rows and the stream's one pred row go to LDS once (rows of J + 2 floats); per pass of 128 classes
//                          a wave runs joint_logits<1>; the epilogue keeps per node the running max and sum (as k_rnnt_joint_fwd), the
//                          logit of blank and the running argmax as (value, class): `>` decides, so a tie goes to the lower class (a
//                          lane's classes ascend, the 16-lane butterfly prefers the lower class at equal value, a later pass wins only
//                          when strictly greater).  The per-frame results (class, log p(class), log p(blank)) go through a small LDS
//                          table; thread 0 walks the chunk's live frames in order, sums log p(blank) in double up to the first frame
//                          whose argmax is not blank, writes the chunk's record and lowers the stream's hit_chunk (integer atomicMin).
//                          A workgroup leaves at once when its stream is not live, when its chunk lies before t_s or behind T_s, or
//                          when a LOWER chunk has already reported a hit (thread 0 reads hit_chunk once for the whole workgroup): such
//                          a chunk's record is never read, so the race changes the work done, not the result.
//   k_rnnt_greedy_advance  one wave, one thread per stream: the lowest chunk with a hit wins; the blank sums of the chunks from t_s's up to
//                          the winner are added in chunk order, then the label's log-probability; label and frame are appended; t_s, the
//                          symbols-per-frame count and the flags are updated; then the wave writes the S next predictor input rows (the
//                          one-hot of the label or the gathered embedding column plus bias, as k_rnnt_pack; zeros for a stream that
//                          is not live) and the number of live streams.
// BOUNDS.  enc rows are read only under t < T_s <= T (k_rnnt_greedy_begin rejects anything else), LDS rows behind them are zero-filled;
// classes >= V are masked at the panel load and in the epilogue; records are indexed by (stream, blockIdx.x); a label is appended only
// while the length is below max_len (the stream is marked truncated when it gets there).  No floating-point atomics.
#include <climits>
#include <cstdint>

#include "../../include/klstm_rnnt.h"
#include "klstm_ctc_host.h"
#include "klstm_host.h"
#include "klstm_kernels.h"
#include "klstm_math.h"
#include "klstm_rnnt_dev.h"

namespace klstm {

constexpr int NOHIT = INT_MAX;
enum { GF_FINISHED = 1, GF_TRUNCATED = 2, GF_REJECTED = 4, GF_IDLE = 8 };

static int greedy_fb(int J) { return J <= 512 ? 64 : 32; }

struct GreedyState {                       // per stream, then per (stream, chunk)
  int *flags, *Ts, *ts, *nsym, *last_t, *len, *hit_chunk;
  double *score;
  int *rec_frame, *rec_label;
  float *rec_lpy;
  double *rec_blank;
};

static GreedyState greedy_carve(void *base, int T, int S, int J, size_t *bytes) {
  CtcCarver c(base);
  GreedyState g;
  const int fb = greedy_fb(J);
  const size_t nrec = (size_t)S * ((T + fb - 1) / fb);
  g.flags = c.take<int>(S); g.Ts = c.take<int>(S); g.ts = c.take<int>(S); g.nsym = c.take<int>(S); g.last_t = c.take<int>(S);
  g.len = c.take<int>(S); g.hit_chunk = c.take<int>(S);
  g.score = c.take<double>(S);
  g.rec_frame = c.take<int>(nrec); g.rec_label = c.take<int>(nrec); g.rec_lpy = c.take<float>(nrec);
  g.rec_blank = c.take<double>(nrec);
  *bytes = c.bytes();
  return g;
}

struct GreedyArgs {
  const float *enc, *pred, *W, *b;
  int enc_stride, pred_stride, T, S, J, V, blank, max_symbols, max_len, fb, nchunk;
  const float *embed, *embed_bias;
  int width;
  float *next_in;
  int next_in_stride;
  int *hyp, *hyp_len, *frame;
  float *score_out;
  int *flags_out, *live;
  GreedyState g;
};

// row s of next_in from x[s] (-1: zeros), by the whole wave
__device__ __forceinline__ void greedy_rows(const int *x, int S, int V, const float *embed, const float *bias, int width, float *out, int stride) {
  for (int s = 0; s < S; s++) {
    const int xs = x[s];
    for (int c = threadIdx.x; c < width; c += 64) {
      float v = 0.f;
      if (xs >= 0 && xs < V) v = embed ? embed[(size_t)c * V + xs] + (bias ? bias[c] : 0.f) : (c == xs ? 1.f : 0.f);
      out[(size_t)s * stride + c] = v;
    }
  }
}

__global__ __launch_bounds__(64) void k_rnnt_greedy_begin(GreedyState g, const int *lens, int T, int S, int V, int bos, const float *embed,
                                                          const float *bias, int width, float *next_in, int stride) {
  __shared__ int x[64];
  const int s = threadIdx.x;
  x[s] = -1;
  if (s < S) {
    const int Ts = lens[s];
    const int f = Ts == 0 ? GF_IDLE : (Ts < 0 || Ts > T) ? GF_REJECTED : 0;
    g.flags[s] = f; g.Ts[s] = f ? 0 : Ts; g.ts[s] = 0; g.nsym[s] = 0; g.last_t[s] = -1; g.len[s] = 0; g.hit_chunk[s] = NOHIT;
    g.score[s] = 0.0;
    if (!f) x[s] = bos;
  }
  __syncthreads();
  greedy_rows(x, S, V, embed, bias, width, next_in, stride);
}

__global__ __launch_bounds__(256) void k_rnnt_greedy_scan(GreedyArgs a) {
  extern __shared__ float lds[];
  __shared__ int go, f_cls[64];
  __shared__ float f_lpy[64], f_lpb[64];
  const int J = a.J, V = a.V, Jp = J + 2, FB = a.fb;
  float *encL = lds, *predL = encL + FB * Jp, *Wp = predL + Jp;
  const int s = blockIdx.y, c = blockIdx.x, t0 = c * FB, tid = threadIdx.x;
  if (a.g.flags[s] != 0) return;
  const int Ts = a.g.Ts[s], ts = a.g.ts[s];
  if (t0 + FB <= ts || t0 >= Ts) return;
  if (tid == 0) go = __hip_atomic_load(&a.g.hit_chunk[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= c;
  __syncthreads();
  if (!go) return;                                     // a lower chunk has the hit: nobody will read this chunk's record
  rnnt_stage(encL, Jp, a.enc, a.enc_stride, t0, FB, min(FB, Ts - t0), a.S, s, J);
  rnnt_stage(predL, Jp, a.pred, a.pred_stride, 0, 1, 1, a.S, s, J);      // row s of pred_rows
  const int lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kg = lane >> 4;
  const bool owns = wave * RT < FB;                    // FB = 32: waves 2 and 3 run the product of tiles 0 and 1 again and drop it
  const float *encW = encL + (owns ? wave : wave & 1) * RT * Jp;
  const float *const pl[1] = {predL};
  float mrun[4], srun[4], ab[4], bv[4];
  int bc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { mrun[j] = RLOG0; srun[j] = 0.f; ab[j] = 0.f; bv[j] = RLOG0; bc[j] = NOHIT; }
  for (int v0 = 0; v0 < V; v0 += VP) {
    const int nvt = (min(VP, V - v0) + 15) / 16;
    f32x4 acc[1][NVT];
    joint_logits<1>(encW, Jp, pl, a.W, J, V, v0, nvt, Wp, acc);
    float bias[NVT];
#pragma unroll
    for (int vt = 0; vt < NVT; vt++) {
      const int v = v0 + vt * 16 + i16;
      bias[vt] = (vt < nvt && v < V) ? a.b[v] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float x[NVT], pb = 0.f, lv = RLOG0;
      int lc = NOHIT;
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) {                // the lane's classes ascend with vt: `>` keeps the lower class of a tie
        const int v = v0 + vt * 16 + i16;
        x[vt] = (vt < nvt && v < V) ? acc[0][vt][j] + bias[vt] : RLOG0;
        pb += v == a.blank ? x[vt] : 0.f;
        if (x[vt] > lv) { lv = x[vt]; lc = v; }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {                // the same pair in all 16 lanes afterwards: the rule is symmetric
        const float ov = __shfl_xor(lv, o);
        const int oc = __shfl_xor(lc, o);
        if (ov > lv || (ov == lv && oc < lc)) { lv = ov; lc = oc; }
      }
      if (lv > bv[j]) { bv[j] = lv; bc[j] = lc; }      // a later pass (higher classes) only when strictly greater
      const float nm = fmaxf(mrun[j], lv);
      float sum = 0.f;
#pragma unroll
      for (int vt = 0; vt < NVT; vt++) sum += expf(x[vt] - nm);
      sum = red16_sum(sum);
      srun[j] = srun[j] * expf(mrun[j] - nm) + sum;
      mrun[j] = nm;
      ab[j] += red16_sum(pb);
    }
  }
  if (owns) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (i16 == j) {
        const int f = wave * RT + 4 * kg + j;
        const float lse = mrun[j] + logf(srun[j]);
        f_cls[f] = bc[j]; f_lpy[f] = bv[j] - lse; f_lpb[f] = ab[j] - lse;
      }
  }
  __syncthreads();
  if (tid == 0) {
    const int hi = min(FB, Ts - t0);
    double blanks = 0.0;
    int hit = -1, label = 0;
    float lpy = 0.f;
    for (int f = max(ts - t0, 0); f < hi; f++) {
      const int k = f_cls[f];
      if (k != a.blank && k >= 0 && k < V) { hit = t0 + f; label = k; lpy = f_lpy[f]; break; }
      blanks += (double)f_lpb[f];
    }
    const size_t r = (size_t)s * a.nchunk + c;
    a.g.rec_frame[r] = hit; a.g.rec_label[r] = label; a.g.rec_lpy[r] = lpy; a.g.rec_blank[r] = blanks;
    if (hit >= 0) atomicMin(&a.g.hit_chunk[s], c);
  }
}

__global__ __launch_bounds__(64) void k_rnnt_greedy_advance(GreedyArgs a) {
  __shared__ int x[64];
  const int s = threadIdx.x;
  x[s] = -1;
  bool live = false;
  if (s < a.S) {
    int f = a.g.flags[s], len = a.g.len[s];
    double score = a.g.score[s];
    if (f == 0) {
      const int Ts = a.g.Ts[s], ts = a.g.ts[s], win = a.g.hit_chunk[s];
      const int last = win == NOHIT ? (Ts - 1) / a.fb : win;
      const size_t r0 = (size_t)s * a.nchunk;
      for (int c = ts / a.fb; c <= last; c++) score += a.g.rec_blank[r0 + c];
      if (win == NOHIT) f = GF_FINISHED;
      else {
        const int t = a.g.rec_frame[r0 + win], y = a.g.rec_label[r0 + win];
        score += (double)a.g.rec_lpy[r0 + win];
        if (len < a.max_len) {                         // (always, unless the caller lowered max_len between two steps)
          a.hyp[(size_t)s * a.max_len + len] = y;
          if (a.frame) a.frame[(size_t)s * a.max_len + len] = t;
          len++;
        }
        const int nsym = t == a.g.last_t[s] ? a.g.nsym[s] + 1 : 1;
        const int next = nsym >= a.max_symbols ? t + 1 : t;      // max_symbols labels at one frame: the next scan starts behind it
        a.g.nsym[s] = nsym; a.g.last_t[s] = t; a.g.ts[s] = next; a.g.len[s] = len;
        if (len >= a.max_len) f = GF_TRUNCATED;
        else if (next >= Ts) f = GF_FINISHED;
        else x[s] = y;
        a.g.hit_chunk[s] = NOHIT;
      }
      a.g.flags[s] = f; a.g.score[s] = score;
    }
    live = f == 0;
    a.hyp_len[s] = len; a.score_out[s] = (float)score; a.flags_out[s] = f;
  }
  const int nlive = __popcll(__ballot(live));
  if (s == 0) *a.live = nlive;
  __syncthreads();
  greedy_rows(x, a.S, a.V, a.embed, a.embed_bias, a.width, a.next_in, a.next_in_stride);
}

static bool gal4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the limits of krnnt_eval on S, T, J (and V); null: inside them
static const char *greedy_limits(int T, int S, int J, int V) {
  if (S < 1 || S > 32) return "1 <= S <= 32";
  if (T < 1 || (long long)T * S > (1ll << 24)) return "1 <= T, T S <= 2^24";
  if (J < 16 || J > 1024 || J % 16 != 0) return "16 <= J <= 1024, J % 16 == 0";
  if (V < 2 || V > 4096) return "2 <= V <= 4096";
  return nullptr;
}

// what begin and step share: the input rows' arguments and the state
static klstm_status greedy_common(const char *who, int T, int S, int J, int V, const float *embed, const float *embed_bias, int D,
                                  const float *next_in, int next_in_stride, const void *state, size_t state_bytes) {
  if (const char *why = greedy_limits(T, S, J, V)) return fail(KLSTM_ERR_SHAPE, "%s: T %d, S %d, J %d, V %d: the limit is %s", who, T, S, J, V, why);
  if (embed && D < 1) return fail(KLSTM_ERR_SHAPE, "%s: an embedding of %d rows", who, D);
  if (!next_in || !state) return fail(KLSTM_ERR_ARG, "%s: null argument", who);
  if (next_in_stride < (embed ? D : V)) return fail(KLSTM_ERR_ARG, "%s: row stride %d below the width %d", who, next_in_stride, embed ? D : V);
  if (!gal4(next_in) || !gal4(embed) || !gal4(embed_bias)) return fail(KLSTM_ERR_ARG, "%s: misaligned pointer", who);
  size_t need = 0;
  greedy_carve(nullptr, T, S, J, &need);
  if (state_bytes < need) return fail(KLSTM_ERR_ARG, "%s: state of %zu bytes, %zu needed", who, state_bytes, need);
  if (reinterpret_cast<uintptr_t>(state) & 255) return fail(KLSTM_ERR_ARG, "%s: the state is not 256-byte aligned", who);
  return KLSTM_OK;
}

}  // namespace klstm

using namespace klstm;

extern "C" {

size_t krnnt_greedy_state_bytes(int T, int S, int J) {
  if (const char *why = greedy_limits(T, S, J, 2)) {
    fail(KLSTM_ERR_SHAPE, "krnnt_greedy_state_bytes: T %d, S %d, J %d: the limit is %s", T, S, J, why);
    return 0;
  }
  size_t bytes = 0;
  greedy_carve(nullptr, T, S, J, &bytes);
  return bytes;
}

klstm_status krnnt_greedy_begin(int T, int S, int J, int V, int bos, const int *lens_dev, const float *embed, const float *embed_bias, int D,
                                float *next_in, int next_in_stride, void *state, size_t state_bytes, void *hip_stream) {
  if (const klstm_status st = greedy_common("krnnt_greedy_begin", T, S, J, V, embed, embed_bias, D, next_in, next_in_stride, state, state_bytes)) return st;
  if (bos < 0 || bos >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_greedy_begin: bos %d outside [0, %d)", bos, V);
  if (!lens_dev) return fail(KLSTM_ERR_ARG, "krnnt_greedy_begin: null argument");
  size_t need = 0;
  const GreedyState g = greedy_carve(state, T, S, J, &need);
  HIPCHK(launch(k_rnnt_greedy_begin, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, LaunchProbe(), g, lens_dev, T, S, V, bos, embed, embed_bias,
                embed ? D : V, next_in, next_in_stride));
  return KLSTM_OK;
}

klstm_status krnnt_greedy_step(const float *enc, int enc_stride, const float *pred_rows, int pred_stride, const float *W, const float *b, int T,
                               int S, int J, int V, int blank, int max_symbols, int max_len, const float *embed, const float *embed_bias, int D,
                               float *next_in, int next_in_stride, int *hyp_dev, int *hyp_len_dev, int *frame_dev, float *score_dev,
                               int *flags_dev, int *live_dev, void *state, size_t state_bytes, void *hip_stream) {
  if (const klstm_status st = greedy_common("krnnt_greedy_step", T, S, J, V, embed, embed_bias, D, next_in, next_in_stride, state, state_bytes)) return st;
  if (blank < 0 || blank >= V) return fail(KLSTM_ERR_SHAPE, "krnnt_greedy_step: blank %d outside [0, %d)", blank, V);
  if (max_len < 1 || max_len > 1023 || max_symbols < 1)
    return fail(KLSTM_ERR_SHAPE, "krnnt_greedy_step: max_len %d, max_symbols %d: the limits are 1 <= max_len <= 1023, 1 <= max_symbols", max_len, max_symbols);
  if (!enc || !pred_rows || !W || !b || !hyp_dev || !hyp_len_dev || !score_dev || !flags_dev || !live_dev)
    return fail(KLSTM_ERR_ARG, "krnnt_greedy_step: null argument");
  if (enc_stride < J || pred_stride < J) return fail(KLSTM_ERR_ARG, "krnnt_greedy_step: row stride below the width %d (%d, %d)", J, enc_stride, pred_stride);
  if (!gal4(enc) || !gal4(pred_rows) || !gal4(W) || !gal4(b) || !gal4(hyp_dev) || !gal4(hyp_len_dev) || !gal4(frame_dev) || !gal4(score_dev) ||
      !gal4(flags_dev) || !gal4(live_dev))
    return fail(KLSTM_ERR_ARG, "krnnt_greedy_step: misaligned pointer");
  GreedyArgs a;
  size_t need = 0;
  a.g = greedy_carve(state, T, S, J, &need);
  a.enc = enc; a.pred = pred_rows; a.W = W; a.b = b; a.enc_stride = enc_stride; a.pred_stride = pred_stride;
  a.T = T; a.S = S; a.J = J; a.V = V; a.blank = blank; a.max_symbols = max_symbols; a.max_len = max_len;
  a.fb = greedy_fb(J); a.nchunk = (T + a.fb - 1) / a.fb;
  a.embed = embed; a.embed_bias = embed_bias; a.width = embed ? D : V; a.next_in = next_in; a.next_in_stride = next_in_stride;
  a.hyp = hyp_dev; a.hyp_len = hyp_len_dev; a.frame = frame_dev; a.score_out = score_dev; a.flags_out = flags_dev; a.live = live_dev;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t shm = ((size_t)(a.fb + 1) * (J + 2) + VP * WPS) * sizeof(float);
  HIPCHK(launch(k_rnnt_greedy_scan, dim3(a.nchunk, S), dim3(256), shm, st, LaunchProbe(), a));
  HIPCHK(launch(k_rnnt_greedy_advance, dim3(1), dim3(64), 0, st, LaunchProbe(), a));
  return KLSTM_OK;
}

}  // extern "C"
