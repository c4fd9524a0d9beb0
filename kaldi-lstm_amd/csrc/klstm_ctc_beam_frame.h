// kaldi-lstm_amd/csrc/klstm_ctc_beam_frame.h -- the frame body of the CTC prefix beam search, ONCE in source.  A FRAGMENT, not a header:
// no include guard, because klstm_ctc_beam.hip includes it several times INSIDE the bodies of k_ctc_beam<LM> and k_ctc_beam_stream<LM>,
// one part at a time, and nothing else may include it.  The two kernels get the same tokens, so each compiles to the instructions
// it had when the text stood in it twice; a shared __forceinline__ function did not.
//   #define KLSTM_BEAM_PART 1   storage: the LDS arrays, the registers of the prefetched LM factors, the views of the tables
//   #define KLSTM_BEAM_PART 2   lm_fetch: the lookup of the LM factors of a beam's extensions, a frame ahead
//   #define KLSTM_BEAM_PART 3   LM = 2: the staging of the resident tables into dynamic LDS (as a function it compiled differently)
//   #define KLSTM_BEAM_PART 4   the frame loop over t in [0, len)
// The part is undefined again at the end.  What a kernel has in scope by then -- part 1: K, lm; parts 2 and 3: tid, nt, C; part 4: y,
// w, S, s, stride, blank, B, len, topv, topi, npar, ntok, Bc, E and the prefetched nv, ni, neb -- and the two places where the kernels
// differ, as macros it defines before part 4 and undefines after it:
//   KLSTM_BEAM_FRAME      the index of frame t within the utterance: t, or (t0 + t) in a chunk that begins at frame t0
//   KLSTM_BEAM_NODE(n)    where node n of the stream's prefix tree lies in npar / ntok
#if !defined(KLSTM_BEAM_PART)
#error "klstm_ctc_beam_frame.h: define KLSTM_BEAM_PART (1 to 4) before every include"
#elif KLSTM_BEAM_PART == 1
  extern __shared__ __attribute__((aligned(16))) unsigned char beam_dyn[];     // LM = 2: weight [Q K] float, next [Q K] int
  __shared__ __attribute__((aligned(16))) u64 keys[BEAM_MAXLIST];
  __shared__ u64 sel[BEAM_MAXB];                                   // the new beam's keys, best first
  __shared__ u64 e_hash[BEAM_MAXB], e_ph[BEAM_MAXB];               // hash of the prefix, hash of the prefix without its last token
  __shared__ int e_node[BEAM_MAXB], e_tok[BEAM_MAXB], e_len[BEAM_MAXB];
  __shared__ float e_pb[BEAM_MAXB], e_pnb[BEAM_MAXB], s_pb[BEAM_MAXB], s_pnb[BEAM_MAXB];
  __shared__ float cvs[LM ? 2 * BEAM_MAXC : BEAM_MAXC];            // with an LM: the candidates of frame t in half t & 1
  __shared__ int cis[LM ? 2 * BEAM_MAXC : BEAM_MAXC];
  __shared__ unsigned char merged[BEAM_MAXB * BEAM_MAXC];          // extension (i, r) went into the stay entry of its prefix (LM: 1 + its slot)
  __shared__ int e_lm[LM ? 2 * BEAM_MAXB : 1];                     // LM state of the beam entries of frame t in half t & 1
  __shared__ int nq[LM ? BEAM_MAXB * BEAM_MAXC : 1];               // LM state an extension leads to
  float gw[BEAM_LMK];                                              // weight and next state of this thread's extensions, fetched a frame ahead
  int gn[BEAM_LMK];
  const float *const lw = reinterpret_cast<const float *>(beam_dyn);
  const int *const lnx = reinterpret_cast<const int *>(beam_dyn) + (LM == 2 ? lm.Q * K : 0);
  SlmView slm{};                                                   // LM = 3: the sections of the blob
  if constexpr (LM == 3) slm = slm_view(lm.next, lm.Q);
#elif KLSTM_BEAM_PART == 2
  // the table entries of the extensions q = tid + k nt < nbc of the beam and the candidates in half `half`
  auto lm_fetch = [&](int half, int nbc) {
#pragma unroll
    for (int k = 0; k < BEAM_LMK; k++) {
      gw[k] = 0.f; gn[k] = -1;
      const int q = tid + k * nt;
      if (q < nbc) {
        const int i = q / C, c = cis[half * BEAM_MAXC + q - i * C];
        if ((unsigned)c < (unsigned)K) {                            // -1: no candidate of that rank
          const int idx = e_lm[half * BEAM_MAXB + i] * K + c;      // states in e_lm lie inside [0, Q): only a checked `next` gets there
          if constexpr (LM == 3) slm_lookup(slm, e_lm[half * BEAM_MAXB + i], c, gw[k], gn[k]);
          else if constexpr (LM == 2) { gw[k] = lw[idx]; gn[k] = lnx[idx]; }
          else { gw[k] = lm.weight[idx]; gn[k] = lm.next[idx]; }
        }
      }
    }
  };
#elif KLSTM_BEAM_PART == 3
    if constexpr (LM == 2) {                                       // stage the tables: 16 bytes a load where the pointers allow it
      float *dw = reinterpret_cast<float *>(beam_dyn);
      int *dn = reinterpret_cast<int *>(beam_dyn) + lm.Q * K;
      const int nel = lm.Q * K;
      if (nel % 4 == 0 && ((reinterpret_cast<uintptr_t>(lm.weight) | reinterpret_cast<uintptr_t>(lm.next)) & 15) == 0) {
        const float4 *sw = reinterpret_cast<const float4 *>(lm.weight);
        const int4 *sn = reinterpret_cast<const int4 *>(lm.next);
#pragma unroll 4
        for (int q = tid; q < nel / 4; q += nt) {
          reinterpret_cast<float4 *>(dw)[q] = sw[q];
          reinterpret_cast<int4 *>(dn)[q] = sn[q];
        }
      } else {
#pragma unroll 4
        for (int q = tid; q < nel; q += nt) { dw[q] = lm.weight[q]; dn[q] = lm.next[q]; }
      }
    }
#elif KLSTM_BEAM_PART == 4
#if !defined(KLSTM_BEAM_FRAME) || !defined(KLSTM_BEAM_NODE)
#error "klstm_ctc_beam_frame.h: the frame loop needs KLSTM_BEAM_FRAME and KLSTM_BEAM_NODE(n)"
#endif
  for (int t = 0; t < len; t++) {
    const size_t r = (size_t)t * S + s;
    const float *yp = y + r * stride;
    float *const cv = cvs + (LM ? (t & 1) * BEAM_MAXC : 0);
    int *const ci = cis + (LM ? (t & 1) * BEAM_MAXC : 0);
    if constexpr (LM == 0)
      if (tid < C) { cv[tid] = nv; ci[tid] = ni; }
    const float eb = neb;
    if (tid < B) sel[tid] = 0;                                     // slots no key lands in: no entry
    if (t + 1 < len) {
      const size_t r1 = r + S;
      neb = beam_emit_at(y + r1 * stride, w, blank);
      if (tid < C) { nv = topv[r1 * C + tid]; ni = topi[r1 * C + tid]; }
    }
    __syncthreads();                                               // the candidates; the beam the frame before wrote
    if (tid < Bc) {                                                // stay entries
      const int j = tid, l = e_tok[j];
      const float tot = badd(e_pb[j], e_pnb[j]);
      const float spb = bmul(tot, eb);
      float spnb = 0.f;
      bool deferred = false;
      if (l >= 0) {
        spnb = bmul(e_pnb[j], beam_emit_at(yp, w, l));
        int pi = -1, rr = -1;
        for (int i = 0; i < Bc; i++)
          if (e_len[i] + 1 == e_len[j] && e_hash[i] == e_ph[j]) pi = i;
        for (int q = 0; q < C; q++)
          if (ci[q] == l && cv[q] > 0.f) rr = q;
        if (pi >= 0 && rr >= 0) {                                  // the extension of the parent by l IS this prefix
          if constexpr (LM == 0) {
            const float v = bmul(l == e_tok[pi] ? e_pb[pi] : badd(e_pb[pi], e_pnb[pi]), cv[rr]);
            spnb = badd(spnb, v);
            merged[pi * C + rr] = 1;
          } else {                                                 // the thread that holds the extension's factor adds it and writes the key
            merged[pi * C + rr] = (unsigned char)(j + 1);
            deferred = true;
          }
        }
      }
      s_pb[j] = spb; s_pnb[j] = spnb;
      if (!deferred) keys[j] = ((u64)__float_as_uint(badd(spb, spnb)) << 32) | (u64)(0xFFFFFFFFu - (unsigned)j);
    }
    __syncthreads();
    const int n = Bc * (C + 1);
    if constexpr (LM != 0) {                                       // extensions with the fused emission f in place of cv[rr]
#pragma unroll
      for (int k = 0; k < BEAM_LMK; k++) {
        const int q = tid + k * nt;
        if (q < Bc * C) {
          const int i = q / C, rr = q - i * C, pos = Bc + q, n1 = gn[k];
          float f = 0.f;
          if (cv[rr] > 0.f && (unsigned)n1 < (unsigned)lm.Q) f = beam_emit(bmul(cv[rr], beam_emit(gw[k])));
          const float v = bmul(ci[rr] == e_tok[i] ? e_pb[i] : badd(e_pb[i], e_pnb[i]), f);
          const int m = merged[q];
          u64 key = 0;
          if (m) {
            const int j = m - 1;
            const float spnb = badd(s_pnb[j], v);
            merged[q] = 0;
            s_pnb[j] = spnb;
            keys[j] = ((u64)__float_as_uint(badd(s_pb[j], spnb)) << 32) | (u64)(0xFFFFFFFFu - (unsigned)j);
          } else if (v > 0.f) key = ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - (unsigned)pos);
          keys[pos] = key;
          nq[q] = n1;
        }
      }
    } else {
      for (int pos = Bc + tid; pos < n; pos += nt) {               // extensions; key 0: no entry
        u64 key = 0;
        const int q = pos - Bc, i = q / C, rr = q - i * C;
        if (merged[q]) merged[q] = 0;
        else if (cv[rr] > 0.f) {
          const float v = bmul(ci[rr] == e_tok[i] ? e_pb[i] : badd(e_pb[i], e_pnb[i]), cv[rr]);
          if (v > 0.f) key = ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - (unsigned)pos);
        }
        keys[pos] = key;
      }
    }
    if (tid == 0) keys[n] = 0;                                     // the pair reads below may run one past an odd n
    __syncthreads();
    // selection by rank: the keys are distinct, so the number of larger keys IS the place in the new beam.  Every thread walks the
    // same addresses (LDS broadcasts, two keys a read); no sorting network, no barrier between its stages
    const ulonglong2 *k2 = reinterpret_cast<const ulonglong2 *>(keys);
    const int np = (n + 1) / 2;
    if (n <= nt) {                                                 // one key a thread
      const u64 key = tid < n ? keys[tid] : 0;
      int rank = 0;
#pragma unroll 8
      for (int j = 0; j < np; j++) {
        const ulonglong2 o = k2[j];
        rank += (o.x > key) + (o.y > key);
      }
      if (key && rank < B) sel[rank] = key;
    } else {                                                       // up to BEAM_KPT keys a thread, every read serves all of them
      u64 my[BEAM_KPT];
      int rank[BEAM_KPT];
#pragma unroll
      for (int e = 0; e < BEAM_KPT; e++) {
        const int pos = tid + e * nt;
        my[e] = pos < n ? keys[pos] : ~0ull;                        // nothing is above ~0: rank 0 for free, never stored
        rank[e] = 0;
      }
#pragma unroll 2
      for (int j = 0; j < np; j++) {
        const ulonglong2 o = k2[j];
#pragma unroll
        for (int e = 0; e < BEAM_KPT; e++) rank[e] += (o.x > my[e]) + (o.y > my[e]);
      }
#pragma unroll
      for (int e = 0; e < BEAM_KPT; e++)
        if (my[e] != ~0ull && my[e] && rank[e] < B) sel[rank[e]] = my[e];
    }
    __syncthreads();
    // the new beam: the first B keys that are entries
    const unsigned mbits = (unsigned)(sel[0] >> 32);
    const u64 key = tid < B ? sel[tid] : 0;
    int node = 0, tok = 0, ln = 0, lst = 0;
    u64 hs = 0, ph = 0;
    float pb = 0.f, pnb = 0.f;
    if (key) {
      const int pos = (int)(0xFFFFFFFFu - (unsigned)key);
      if (pos < Bc) {
        node = e_node[pos]; tok = e_tok[pos]; ln = e_len[pos]; hs = e_hash[pos]; ph = e_ph[pos]; pb = s_pb[pos]; pnb = s_pnb[pos];
        if constexpr (LM != 0) lst = e_lm[(t & 1) * BEAM_MAXB + pos];
      } else {
        const int q = pos - Bc, i = q / C, rr = q - i * C;
        node = 1 + KLSTM_BEAM_FRAME * B + tid; tok = ci[rr]; ln = e_len[i] + 1; ph = e_hash[i]; hs = beam_hash(ph, tok);
        pnb = __uint_as_float((unsigned)(key >> 32));
        npar[KLSTM_BEAM_NODE(node)] = e_node[i]; ntok[KLSTM_BEAM_NODE(node)] = tok;
        if constexpr (LM != 0) lst = nq[q];
      }
      if (mbits) {                                                 // M = m 2^k, m in [0.5, 1): times 2^-k, exact
        const int ex = (int)((mbits >> 23) & 0xffu);
        const float sc = __uint_as_float((unsigned)(253 - ex) << 23);
        pb = bmul(pb, sc); pnb = bmul(pnb, sc);
        pb = pb >= BEAM_TINY ? pb : 0.f; pnb = pnb >= BEAM_TINY ? pnb : 0.f;
      }
    }
    if constexpr (LM != 0) {                                       // the other halves: nobody reads them in this frame
      const int h1 = (t + 1) & 1;
      if (key) e_lm[h1 * BEAM_MAXB + tid] = lst;
      if (tid < C) { cvs[h1 * BEAM_MAXC + tid] = nv; cis[h1 * BEAM_MAXC + tid] = ni; }
    }
    Bc = __syncthreads_count(key != 0);                            // everybody has read the old beam
    if constexpr (LM != 0)
      if (t + 1 < len) lm_fetch((t + 1) & 1, Bc * C);              // in flight over the barrier and the stay entries of frame t + 1
    if (mbits) E += (int)((mbits >> 23) & 0xffu) - 126;
    if (key) { e_node[tid] = node; e_tok[tid] = tok; e_len[tid] = ln; e_hash[tid] = hs; e_ph[tid] = ph; e_pb[tid] = pb; e_pnb[tid] = pnb; }
  }
#else
#error "klstm_ctc_beam_frame.h: KLSTM_BEAM_PART must be 1 to 4"
#endif
#undef KLSTM_BEAM_PART
