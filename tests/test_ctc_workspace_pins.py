"""The workspace sizes of the calls whose layouts go through the carver of csrc/klstm_ctc_host.h (CtcCarver), and of the loss, pinned
byte for byte: klstm_ctc_consensus_workspace_bytes and klstm_ctc_rescore_workspace_bytes (token and word mode),
klstm_ctc_mbr_workspace_bytes (without and with a reference), klstm_ctc_mmi_workspace_bytes with klstm_ctc_mmi_graph_bytes, and
klstm_ctc_workspace_bytes.  A caller sizes its buffer once and keeps it: a layout that moves must say so here.

The numbers were read from the library of commit debc5b8 ("Add second-pass n-best rescoring with token and word back-off LMs"), the
last one whose layouts spelt every offset by hand.  The shapes hold S = 1 and 32, N = 1 and the largest list (64; 16 for the n-best
risk), and the lengths 0, 255, 256 (from there the consensus keeps its back-pointer table in the workspace) and 1023.  No device."""
import ctypes

import pytest

# ((S, N, max_len), consensus tokens, consensus words, rescore tokens, rescore words)
NBEST = [
    ((1, 1, 0), 2560, 2816, 1536, 1536),
    ((1, 64, 255), 35328, 165888, 1792, 1792),
    ((1, 64, 256), 4229632, 4360704, 1792, 1792),
    ((32, 1, 1023), 8417536, 8679424, 3328, 3328),
    ((32, 64, 1023), 539018240, 555779072, 35328, 35328),
    ((5, 7, 256), 2306560, 2378240, 2048, 2048),
    ((32, 16, 255), 178688, 1223168, 10752, 10752),
    ((3, 64, 0), 55040, 56576, 3840, 3840),
    ((2, 8, 100), 4352, 17152, 1536, 1536),
]
# ((T, S, N, max_len), without a reference, with one)
MBR = [
    ((1, 1, 1, 0), 132384, 132416),
    ((50, 32, 16, 255), 111149568, 117834752),
    ((50, 32, 16, 256), 111976960, 118713600),
    ((2047, 32, 1, 1023), 1077937152, 2151678464),
    ((100, 1, 16, 1023), 26608896, 28263680),
    ((37, 5, 7, 100), 2826656, 3136512),
    ((2000, 32, 16, 0), 36971008, 39019776),
    ((300, 3, 2, 511), 15189248, 22586624),
]
# ((T, S, K, lm_states, max_label_len), workspace, graph)
MMI = [
    ((1, 1, 2, 1, 0), 1088, 5120),
    ((50, 32, 64, 256, 255), 216335104, 922368),
    ((50, 32, 64, 256, 256), 216386560, 922368),
    ((2047, 32, 2, 1, 1023), 1075576576, 5120),
    ((100, 1, 128, 128, 1023), 14754816, 921344),
    ((37, 5, 7, 3, 100), 342560, 5120),
    ((2000, 32, 4096, 4, 0), 8390657024, 951808),
    ((300, 3, 30, 30, 511), 13866112, 55296),
]
# ((T, S, max_label_len), workspace)
CTC = [
    ((1, 1, 0), 288),
    ((50, 32, 255), 6619136),
    ((50, 32, 256), 6670592),
    ((2047, 32, 1023), 1073479680),
    ((100, 1, 1023), 1646592),
    ((37, 5, 100), 306016),
    ((2000, 32, 0), 2048256),
    ((300, 3, 511), 7385088),
]


@pytest.fixture(scope="module")
def lib():
    import kaldi_lstm_amd as k
    lib = k.load_library()
    for n in ("klstm_ctc_consensus_workspace_bytes", "klstm_ctc_rescore_workspace_bytes", "klstm_ctc_mbr_workspace_bytes",
              "klstm_ctc_mmi_workspace_bytes", "klstm_ctc_mmi_graph_bytes", "klstm_ctc_workspace_bytes"):
        assert getattr(lib, n).restype is ctypes.c_size_t, n
    return lib


def test_the_shapes_cover_the_edges():
    assert {s[0] for s, *_ in NBEST} >= {1, 32} and {s[1] for s, *_ in NBEST} >= {1, 64}
    assert {s[2] for s, *_ in NBEST} >= {0, 255, 256, 1023} and all(len(t) >= 8 for t in (NBEST, MBR, MMI, CTC))
    assert {s[1] for s, *_ in MBR} >= {1, 32} and {s[2] for s, *_ in MBR} >= {1, 16} and {s[3] for s, *_ in MBR} >= {0, 255, 256, 1023}


@pytest.mark.parametrize("shape,cons_tok,cons_word,resc_tok,resc_word", NBEST)
def test_consensus_and_rescore_workspace_bytes(lib, shape, cons_tok, cons_word, resc_tok, resc_word):
    assert [lib.klstm_ctc_consensus_workspace_bytes(*shape, w) for w in (0, 1)] == [cons_tok, cons_word]
    assert [lib.klstm_ctc_rescore_workspace_bytes(*shape, w) for w in (0, 1)] == [resc_tok, resc_word]


@pytest.mark.parametrize("shape,without_ref,with_ref", MBR)
def test_mbr_workspace_bytes(lib, shape, without_ref, with_ref):
    assert [lib.klstm_ctc_mbr_workspace_bytes(*shape, r) for r in (0, 1)] == [without_ref, with_ref]


@pytest.mark.parametrize("shape,workspace,graph", MMI)
def test_mmi_workspace_and_graph_bytes(lib, shape, workspace, graph):
    T, S, K, Q, L = shape
    assert lib.klstm_ctc_mmi_workspace_bytes(T, S, K, Q, L) == workspace and lib.klstm_ctc_mmi_graph_bytes(Q, K) == graph


@pytest.mark.parametrize("shape,workspace", CTC)
def test_ctc_workspace_bytes(lib, shape, workspace):
    assert lib.klstm_ctc_workspace_bytes(*shape) == workspace
