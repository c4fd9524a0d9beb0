"""kaldi-lstm_amd: MI355X-native LstmProjectedStreams forward/BPTT/update engine.

The product is the C-ABI shared library `libklstm.so` (include/klstm.h, hand-written gfx950
HIP kernels) plus the C++ mirror of the reference component (include/klstm_component.hpp).
This Python package is plumbing over that ABI for tests, bench.py and torch.distributed
launch; it contains no arithmetic and NO CPU fallback: if the library or a GPU is missing,
calls raise.
"""
from .binding import (Engine, KlstmError, RcclComm, OneshotAllreduce, lib_path, load_library, time_shift, affine_propagate,  # noqa: F401
                      affine_backpropagate, affine_update, affine_gradient, sgd_momentum_update, softmax,
                      xent_eval_masked, xent_eval_masked_post, softmax_xent_masked, debug_gemm_bf16_nt2, DEFER_MOMENTUM,
                      pack_streams, log_softmax_scatter, SCORE_POSTERIOR, SCORE_LOGPOST, SCORE_LOGLIKE,
                      reverse_streams, REVERSE_SET, REVERSE_ADD, REVERSE_ZERO_PAD, REVERSE_MASK_COPY)
from .batcher import MultiStreamBatcher  # noqa: F401,E402
from .blstm import BidirectionalLstm  # noqa: F401,E402
from .ctc import ctc_eval, ctc_workspace_bytes  # noqa: F401,E402
from .ctc import CtcDecodeResult, ctc_decode_workspace_bytes, ctc_greedy_decode, hypotheses_to_lists  # noqa: F401,E402
from .ctc import CtcAlignResult, alignments_to_lists, ctc_align, ctc_align_workspace_bytes  # noqa: F401,E402
from .ctc import CtcBeamResult, ctc_beam_decode, ctc_beam_workspace_bytes, nbest_to_lists  # noqa: F401,E402
from .ctc import CtcLabelLm, CtcSparseLabelLm  # noqa: F401,E402
from .ctc import CtcBeamStream, CtcStreamResult, ctc_beam_stream_state_bytes, ctc_beam_stream_workspace_bytes  # noqa: F401,E402
from .ctc import CtcMbrResult, ctc_mbr_eval, ctc_mbr_workspace_bytes  # noqa: F401,E402
from .ctc import CtcConsensusResult, consensus_to_lists, ctc_consensus_workspace_bytes, ctc_nbest_consensus  # noqa: F401,E402
from .ctc import CtcWordTable, ctc_nbest_rescore, ctc_rescore_workspace_bytes  # noqa: F401,E402
from .ctc import CtcMmiDenominator, CtcMmiResult, ctc_mmi_eval, ctc_mmi_workspace_bytes  # noqa: F401,E402
from .nlm import CtcNeuralLm, CtcNeuralRescoreResult, knlm_pack, knlm_rank, knlm_score_rows, knlm_workspace_bytes, lm_training_utterances  # noqa: F401,E402
from .dropout import DROPOUT_ELEMENT, DROPOUT_SEQUENCE, Dropout, dropout_apply, dropout_threshold  # noqa: F401,E402
from .cnn import (Convolutional, MaxPooling, Sigmoid, Tanh, activation, activation_diff, conv_backpropagate, conv_gradient,  # noqa: F401,E402
                  conv_plan, conv_propagate, conv_update, conv_workspace_floats, pool_backpropagate, pool_propagate)
from .lm import lexicon_label_lm, ngram_label_lm  # noqa: F401,E402
from .lm import dense_lm_to_sparse, word_key, word_sequences, word_table  # noqa: F401,E402
from .lm import SparseLm, arpa_label_lm, backoff_ngram_label_lm, sparse_lm_lookup, sparse_lm_to_dense, sparse_lm_validate  # noqa: F401,E402
from .dp import (DataParallelLstm, DataParallelNnet, LstmDP, AffineDP, SoftmaxXentDP,  # noqa: F401,E402
                 shard_time_major)
