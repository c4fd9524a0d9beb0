// kaldi-lstm_amd/csrc/klstm_ctc_align.hip -- CTC forced alignment (Viterbi) of whole utterances (klstm_ctc_align of include/klstm.h;
// DESIGN.md 4j): the single most probable alignment of a label sequence to the frames.  One launch, one workgroup per stream:
//   chain   the 2L+1 lattice states spread over the threads as in k_ctc_chain (state i on thread i % threads, the previous row in LDS,
//           double-buffered, one barrier per step).  The step is two LDS neighbour reads, two compare-selects and one add; the emission
//           gather runs AL_DEPTH steps ahead and the accurate logf is off the chain.  The back-pointer of a state (0 stay, 1 advance,
//           2 skip) is two bits: state i sits on lane i % 64, so two ballots per wave are the pointers of 64 states, stored by lanes 0
//           and 32 as (low bits, high bits) of 32 states each: 8 bytes per 32 states and frame.
//   trace   by the same workgroup, 256 frames at a time from the end.  The path descends by at most two states per frame, so a block
//           entered at state i touches the pointer columns [i - 512, i] only: at most 17 groups of 32 states.  The whole workgroup
//           loads that window into LDS (34 KB), one thread walks it there (a dependent LDS read per frame, never a trip to memory),
//           then the whole workgroup writes frame_class, frame_pos, the token boundaries and gathers the path's emissions.
//   totals  a second launch of one thread, only when the caller keeps totals.
// NUMBERS.  Sums of float32 logs in float32.  Every AL_NORM-th row's maximum is taken out of the next row's emissions (off the
// dependent chain): the values stay of the size of a few frames' log posteriors whatever the utterance's length, and since every
// state of a row gets the same offset, no comparison changes other than by rounding.  The score is summed afterwards, in double.
// DETERMINISM.  No floating-point atomics.  max and the compare-selects are exact, so the pointers do not depend on the geometry; the
// score is 256 partial sums (slot = frame % 256, frames in descending order) and a fixed tree over them, whatever the workgroup's size.
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "../../include/klstm.h"
#include "klstm_ctc_dev.h"
#include "klstm_ctc_host.h"
#include "klstm_kernels.h"

namespace klstm {

constexpr int AL_NORM = 8;             // a row maximum is taken out every AL_NORM steps, whatever the geometry: the same numbers from all
constexpr int AL_F = 256;              // frames per block of the trace
constexpr int AL_GW = 2 * AL_F / 32 + 1;   // groups of 32 states a block of the trace can touch

// stat [S][4]: status (0 idle, 1 aligned, 2 rejected), frames, blank frames, the bits of the float score.  bp: [S][T][W] words, per
// frame and group of 32 states the low and the high bit of the pointers.  W = 2 * ceil((2 Lcap + 1) / 32)
struct AlignWs { int *stat; unsigned *bp; int W, Lcap; };

// PHASES: 3 = the call; 1 = the chain only, 2 = the trace only over the pointers an earlier call left in the workspace (builds with
// KLSTM_ALIGN_PROBE, for tools/ctc_align_probe.py: what each part costs)
template <int NW, int P, int PHASES = 3>
__global__ __launch_bounds__(64 * NW) void k_ctc_align(const float *__restrict__ y, int T, int S, int K, int stride,
                                                       const int *__restrict__ lens, const int *__restrict__ labels,
                                                       const int *__restrict__ loff, int blank, const float *__restrict__ cw,
                                                       int *__restrict__ fclass, int *__restrict__ fpos, int *__restrict__ tbeg,
                                                       int *__restrict__ tend, float *__restrict__ score, AlignWs ws) {
  constexpr int NT = 64 * NW, CAP = NT * P;
  constexpr int AL_DEPTH = P == 1 ? 8 : 4;    // steps the emission gather runs ahead of the chain (two states per thread: the registers of 4)
  static_assert(AL_NORM % AL_DEPTH == 0, "a row maximum is taken out after the last step of a block");
  __shared__ float row[2][CAP + 4];           // state i at [i + 2]; two cells of CTC_NEG on either side
  __shared__ float pmax[NW];
  __shared__ uint2 win[AL_F * AL_GW];
  __shared__ int sstate[AL_F + 2];            // [q + 1]: the state at frame t0 + q of the block; [0]: at t0 - 1
  __shared__ double dsum[256];
  __shared__ int sm[2];
  __shared__ int s_entry, s_blanks;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o0 = loff[s], L = loff[s + 1] - o0, len = lens[s];
  const int *lab = labels + o0;
  const int st = ctc_status(len, T, L, ws.Lcap, lab, K, blank, sm);
  if (st != 1) {
    for (int t = tid; t < T; t += NT) {
      fclass[(size_t)t * S + s] = -1;
      if (fpos) fpos[(size_t)t * S + s] = -1;
    }
    if (tbeg)
      for (int j = tid; j < L; j += NT) { tbeg[o0 + j] = -1; tend[o0 + j] = -1; }
    if (tid == 0) {
      const float sc = st == 2 ? -INFINITY : 0.f;
      if (score) score[s] = sc;
      ws.stat[4 * s] = st; ws.stat[4 * s + 1] = 0; ws.stat[4 * s + 2] = 0; ws.stat[4 * s + 3] = __float_as_int(sc);
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------------------------------------------
  // the chain
  // ---------------------------------------------------------------------------------------------------------------------------------
  const int N = 2 * L + 1;
  const float *yp[P];
  bool act[P], allow2[P];
  float wgt[P], w[P];
#pragma unroll
  for (int k = 0; k < P; k++) {
    const int i = tid + k * NT;
    act[k] = i < N;
    const int cls = (act[k] && (i & 1)) ? lab[i >> 1] : blank;
    yp[k] = y + (size_t)s * stride + cls;
    wgt[k] = cw ? cw[cls] : 1.f;               // y * 1 is y, bit for bit
    allow2[k] = act[k] && (i & 1) && i >= 3 && lab[i >> 1] != lab[(i >> 1) - 1];
  }
  if (tid < 2) {
    row[0][tid] = CTC_NEG; row[1][tid] = CTC_NEG;
    row[0][CAP + 2 + tid] = CTC_NEG; row[1][CAP + 2 + tid] = CTC_NEG;
  }
  const size_t tstride = (size_t)S * stride;
  unsigned *bps = ws.bp + (size_t)s * T * ws.W;

  float en[AL_DEPTH][P];
#pragma unroll
  for (int d = 0; d < AL_DEPTH; d++)
#pragma unroll
    for (int k = 0; k < P; k++) en[d][k] = d < len ? yp[k][(size_t)d * tstride] : 1.f;

  // The log of a step's emissions is taken one step AHEAD, between that step's LDS reads and their use: it is not on the dependent chain
  // (LDS read, two compare-selects, add, LDS write, barrier), and in the slots where the wave waits for its reads it costs nothing.
  // Step 0 is a step like any other: its "previous row" is CTC_NEG but for the two start states, whose own value is 0.
  float M = 0.f, emn[P];                       // M: what the next row's emissions are lowered by; emn: the emissions of the step to come
  float ec[AL_DEPTH][P];
#pragma unroll
  for (int k = 0; k < P; k++) {
    const int i = tid + k * NT;
    emn[k] = logf(fmaxf(en[0][k] * wgt[k], FLT_MIN));                     // fmaxf(NaN, x) = x
    w[k] = i <= 1 ? 0.f : CTC_NEG;
    row[1][i + 2] = CTC_NEG;
  }
  __syncthreads();
  auto step = [&](int u, int d) {
    const int b = u & 1;
    float x1[P], x2[P], em[P];
#pragma unroll
    for (int k = 0; k < P; k++) {
      const int i = tid + k * NT;
      x1[k] = row[b ^ 1][i + 1];
      x2[k] = allow2[k] ? row[b ^ 1][i] : CTC_NEG;
      em[k] = d == 0 ? emn[k] - M : emn[k];    // a maximum is taken out after the last step of a block only (M = 0: none was)
    }
#pragma unroll
    for (int k = 0; k < P; k++) emn[k] = logf(fmaxf((d + 1 < AL_DEPTH ? ec[(d + 1) % AL_DEPTH][k] : en[0][k]) * wgt[k], FLT_MIN));
    float lmax = CTC_NEG;
    unsigned long long lo[P], hi[P];
#pragma unroll
    for (int k = 0; k < P; k++) {
      float base = w[k];
      int mv = 0;                              // ties: stay, then advance, then skip
      if (x1[k] > base) { base = x1[k]; mv = 1; }
      if (x2[k] > base) { base = x2[k]; mv = 2; }
      const float wk = act[k] ? base + em[k] : CTC_NEG;
      w[k] = wk;
      row[b][tid + k * NT + 2] = wk;
      lmax = fmaxf(lmax, wk);
      lo[k] = __ballot(mv & 1);
      hi[k] = __ballot(mv >> 1);
    }
    if ((lane & 31) == 0) {                    // behind the LDS write: the stores' issue overlaps its way to the barrier
#pragma unroll
      for (int k = 0; k < P; k++) {
        const int h = 2 * (k * NW + wv) + (lane >> 5);                    // this half wave's group of 32 states
        if (32 * h < N)
          *reinterpret_cast<uint2 *>(bps + (size_t)u * ws.W + 2 * h) =
              lane ? make_uint2((unsigned)(lo[k] >> 32), (unsigned)(hi[k] >> 32)) : make_uint2((unsigned)lo[k], (unsigned)hi[k]);
      }
    }
    const bool norm = d == AL_DEPTH - 1 && (u % AL_NORM) == AL_NORM - 1;  // uniform
    if (norm) {
      lmax = wave_max(lmax);
      if (NW > 1 && lane == 0) pmax[wv] = lmax;
    }
    __syncthreads();
    if (d == AL_DEPTH - 1) M = 0.f;
    if (norm) {
      if (NW > 1) {
        lmax = pmax[0];
#pragma unroll
        for (int q = 1; q < NW; q++) lmax = fmaxf(lmax, pmax[q]);
      }
      M = lmax;
    }
  };
  const int nsteps = (PHASES & 1) ? len : 0;
  int u0 = 0;
  for (; u0 + AL_DEPTH <= nsteps; u0 += AL_DEPTH) {                        // whole blocks: no branch inside
#pragma unroll
    for (int d = 0; d < AL_DEPTH; d++)
#pragma unroll
      for (int k = 0; k < P; k++) {
        ec[d][k] = en[d][k];
        const int un = u0 + AL_DEPTH + d;
        en[d][k] = un < len ? yp[k][(size_t)un * tstride] : 1.f;
      }
#pragma unroll
    for (int d = 0; d < AL_DEPTH; d++) step(u0 + d, d);
  }
#pragma unroll
  for (int d = 0; d < AL_DEPTH; d++)
#pragma unroll
    for (int k = 0; k < P; k++) { ec[d][k] = en[d][k]; en[d][k] = 1.f; }
#pragma unroll
  for (int d = 0; d < AL_DEPTH - 1; d++)
    if (u0 + d < nsteps) step(u0 + d, d);                                  // the last, partial block
  if (tid == 0) {                              // the end: state 2L unless 2L - 1 is strictly better
    const int b = (len - 1) & 1;
    const float a1 = row[b][N - 1 + 2], a2 = N > 1 ? row[b][N - 2 + 2] : CTC_NEG;
    s_entry = (PHASES & 1) && a2 > a1 ? N - 2 : N - 1;
    s_blanks = 0;
  }
  for (int q = tid; q < 256; q += NT) dsum[q] = 0.0;
  __syncthreads();                             // also: the pointers every wave stored are visible to the workgroup

  // ---------------------------------------------------------------------------------------------------------------------------------
  // the trace, blocks of AL_F frames from the end
  // ---------------------------------------------------------------------------------------------------------------------------------
  int carry = -1, nbl = 0;                     // carry: the state of the frame after the block (none after the last frame)
  for (int t0 = (PHASES & 2) ? (len - 1) / AL_F * AL_F : -1; t0 >= 0; t0 -= AL_F) {
    const int t1 = min(len, t0 + AL_F), nr = t1 - t0;
    const int entry = s_entry;                 // the state at frame t1 - 1
    const int gw0 = max(entry - 2 * AL_F, 0) >> 5, ng = (entry >> 5) - gw0 + 1;          // ng <= AL_GW, gw0 + ng <= W / 2
    for (int idx = tid; idx < nr * ng; idx += NT) {
      const int r = idx / ng, c = idx - r * ng, t = t0 + r;
      if (t > 0) win[r * AL_GW + c] = *reinterpret_cast<const uint2 *>(bps + (size_t)t * ws.W + 2 * (gw0 + c));
    }
    __syncthreads();
    if (tid == 0) {
      int cur = entry;
      for (int t = t1 - 1; t >= t0; t--) {
        sstate[t - t0 + 1] = cur;
        if (t > 0) {
          const uint2 wd = win[(t - t0) * AL_GW + ((cur >> 5) - gw0)];
          const int bit = cur & 31;
          cur -= ((wd.x >> bit) & 1u) + 2u * ((wd.y >> bit) & 1u);
        }
      }
      sstate[0] = cur;
      s_entry = cur;
    }
    __syncthreads();
    const int first = sstate[1];
    for (int q = tid; q < nr; q += NT) {
      const int t = t0 + q;
      const int cur = min(max(sstate[q + 1], 0), N - 1);                  // in range whatever the pointers held
      const int prev = t > 0 ? sstate[q] : -1, next = q + 1 < nr ? sstate[q + 2] : carry;
      const bool odd = cur & 1;
      const int pos = cur >> 1, cls = odd ? lab[pos] : blank;
      const size_t r = (size_t)t * S + s;
      fclass[r] = cls;
      if (fpos) fpos[r] = odd ? pos : -1;
      if (tbeg && odd) {
        if (prev != cur) tbeg[o0 + pos] = t;
        if (next != cur) tend[o0 + pos] = t + 1;
      }
      dsum[q] += (double)logf(fmaxf(y[r * stride + cls], FLT_MIN));       // slot q = t % 256: this thread's in every block
      nbl += !odd;
    }
    carry = first;
  }
  for (int t = len + tid; t < T; t += NT) {
    fclass[(size_t)t * S + s] = -1;
    if (fpos) fpos[(size_t)t * S + s] = -1;
  }
  if (nbl) atomicAdd(&s_blanks, nbl);          // integer
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {          // the same tree whatever the workgroup's size
    for (int q = tid; q < o; q += NT) dsum[q] += dsum[q + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float sc = (float)dsum[0];
    if (score) score[s] = sc;
    ws.stat[4 * s] = 1; ws.stat[4 * s + 1] = len; ws.stat[4 * s + 2] = s_blanks; ws.stat[4 * s + 3] = __float_as_int(sc);
  }
}

// the minibatch's statistics onto the totals, one thread, streams in order
__global__ __launch_bounds__(64) void k_ctc_align_totals(const int *__restrict__ stat, int S, double *__restrict__ totals) {
  if (threadIdx.x != 0) return;
  double sum = 0, cnt = 0, rej = 0, frames = 0, blanks = 0;
  for (int q = 0; q < S; q++) {
    const int *p = stat + 4 * q;
    if (p[0] == 1) { sum += (double)__int_as_float(p[3]); cnt += 1; frames += p[1]; blanks += p[2]; }
    else if (p[0] == 2) rej += 1;
  }
  totals[0] += sum; totals[1] += cnt; totals[2] += rej; totals[3] += frames; totals[4] += blanks;
}

constexpr size_t AL_HEAD = 512;                // stat [32][4]

static int align_words(int Lcap) { return 2 * ((2 * Lcap + 1 + 31) / 32); }

size_t ctc_align_workspace_bytes(int T, int S, int Lcap) {
  return AL_HEAD + ctc_up256((size_t)T * S * align_words(Lcap) * sizeof(unsigned));
}

int ctc_align_label_capacity(int T, int S, size_t bytes) {
  return ctc_label_capacity_of(bytes, [&](int Lcap) { return ctc_align_workspace_bytes(T, S, Lcap); });
}

hipError_t launch_ctc_align(const float *y, int T, int S, int K, int stride, const int *lens, const int *labels, const int *loff, int blank,
                            const float *cw, int *fclass, int *fpos, int *tbeg, int *tend, float *score, double *totals, void *workspace,
                            int Lcap, hipStream_t st) {
  AlignWs ws;
  ws.stat = reinterpret_cast<int *>(workspace);
  ws.bp = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(workspace) + AL_HEAD);
  ws.W = align_words(Lcap);
  ws.Lcap = Lcap;
  const int N = 2 * Lcap + 1;
  // 16 * waves + states per thread
  int plan = N <= 64 ? 16 * 1 + 1 : N <= 256 ? 16 * 4 + 1 : N <= 512 ? 16 * 8 + 1 : N <= 1024 ? 16 * 16 + 1 : 16 * 16 + 2;
  hipError_t err;
#define AL_CASE(NW, P, PH)                                                                                                          \
  case 1024 * PH + 16 * NW + P:                                                                                                     \
    err = launch(k_ctc_align<NW, P, PH>, dim3(S), dim3(64 * NW), 0, st, LaunchProbe{}, y, T, S, K, stride, lens, labels, loff, blank, \
                 cw, fclass, fpos, tbeg, tend, score, ws);                                                                          \
    break;
#ifdef KLSTM_ALIGN_PROBE
  const char *ep = getenv("KLSTM_ALIGN_PLAN"), *eh = getenv("KLSTM_ALIGN_PHASES");
  if (ep && atoi(ep) > 0) {
    const int nw = atoi(ep) / 16, p = atoi(ep) % 16;
    if (64 * nw * p < N) return hipErrorInvalidValue;
    plan = atoi(ep);
  }
  const int phases = eh && atoi(eh) > 0 ? atoi(eh) : 3;
#define AL_GEO(NW, P) AL_CASE(NW, P, 1) AL_CASE(NW, P, 2) AL_CASE(NW, P, 3)
  switch (1024 * phases + plan) {
    AL_GEO(1, 1) AL_GEO(1, 2) AL_GEO(1, 4) AL_GEO(2, 2) AL_GEO(4, 1) AL_GEO(4, 2) AL_GEO(4, 4) AL_GEO(8, 1) AL_GEO(8, 2) AL_GEO(8, 4)
    AL_GEO(16, 1) AL_GEO(16, 2)
    default: return hipErrorInvalidValue;
  }
#undef AL_GEO
#else
  switch (1024 * 3 + plan) {
    AL_CASE(1, 1, 3) AL_CASE(4, 1, 3) AL_CASE(8, 1, 3) AL_CASE(16, 1, 3) AL_CASE(16, 2, 3)
    default: return hipErrorInvalidValue;
  }
#endif
#undef AL_CASE
  if (err != hipSuccess || !totals) return err;
  return launch(k_ctc_align_totals, dim3(1), dim3(64), 0, st, LaunchProbe{}, (const int *)ws.stat, S, totals);
}

}  // namespace klstm
