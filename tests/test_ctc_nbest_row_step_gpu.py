"""The Levenshtein row step that the decoders and the n-best consensus share (KLSTM_ED_ROW_STEP of csrc/klstm_ctc_dev.h), seen from its
two sides on the device: k_ctc_beam_tail computes errors[s, q] = distance(entry q, reference) through edit_distance<P, false>, and the
consensus computes dist[s, q, r] for every pair of entries through its own rows.  With each stream's reference appended to its list as
entry N, dist[s, q, N] is the same distance by the other caller: the two must be equal, and equal to the host's (tests/nbest_ref.py).

References of 63, 64 and 65 tokens: in both callers the columns sit one per lane up to 63 of them and four per lane from 64, so the
three lengths stand on either side of that change of P and on it.  S = 2 holds two of them: two searches.  Integers: the bar is
equality.  Each case asserts that it is not vacuous: every list is full (so entry N is listed) and some listed entry has errors > 0."""
import numpy as np
import pytest
import torch

from tests import nbest_ref

pytestmark = pytest.mark.gpu
T, K, BEAM, N = 200, 12, 8, 4


@pytest.mark.parametrize("seed,ref_lens", [(11, (63, 64)), (12, (65, 63))])
def test_errors_of_the_search_are_the_distances_of_the_consensus(seed, ref_lens):
    import kaldi_lstm_amd as k
    from tests import ctc_mbr_ref as M
    S, lens = 2, [T, T - 7]
    refs = M.random_refs(seed, K, list(ref_lens))
    assert [len(r) for r in refs] == list(ref_lens)
    y = M.peaked(seed, T, K, lens, refs).reshape(T * S, K).cuda()
    nb = k.ctc_beam_decode(y, lens, beam=BEAM, cands=8, nbest=N, refs=refs)
    hyp, hyp_len, count = nb.hyp.cpu().numpy(), nb.hyp_len.cpu().numpy(), nb.nbest_count.cpu().numpy()
    errors, score = nb.errors.cpu().numpy(), nb.score.cpu().numpy()
    assert (count == N).all(), count                                   # every list is full: the appended entry N is listed
    stride = hyp.shape[2]
    assert stride >= max(ref_lens)
    hyp2 = np.full((S, N + 1, stride), 10 ** 6, np.int32)
    len2, logp2 = np.zeros((S, N + 1), np.int32), np.zeros((S, N + 1), np.float32)
    hyp2[:, :N], len2[:, :N], logp2[:, :N] = hyp, hyp_len, score
    for s, r in enumerate(refs):
        hyp2[s, N, :len(r)], len2[s, N], logp2[s, N] = r, len(r), -1.0
    assert np.isfinite(logp2).all()
    lists = tuple(torch.from_numpy(a).cuda() for a in (hyp2, len2, count + 1)) + (None,)
    r = k.ctc_nbest_consensus(lists, logp=torch.from_numpy(logp2).cuda(), want_dist=True)
    dist, unit_len = r.dist.cpu().numpy(), r.unit_len.cpu().numpy()
    assert np.array_equal(unit_len, len2)                              # nothing was dropped
    for s in range(S):
        for q in range(N):
            host = nbest_ref.levenshtein(hyp[s, q, :hyp_len[s, q]].tolist(), refs[s])
            print(f"stream {s} entry {q}: errors {errors[s, q]}, dist {dist[s, q, N]}, host {host}")
            assert dist[s, q, N] == errors[s, q] == host and dist[s, N, q] == host, (s, q)
    assert (errors > 0).any()
