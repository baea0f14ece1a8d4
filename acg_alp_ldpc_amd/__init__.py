"""acg_alp_ldpc_amd — MI355X-native batched LDPC decoding behind the reference's Decoder API.

Only the hot path of GreatDrake/acg-alp-ldpc is here: BP (algo/bp.h), QP-ADMM
(algo/qp_admm.h), the AWGN channel (utils/channel.h) and the Monte-Carlo loop (experiment.h),
implemented as hand-written HIP kernels for gfx950 in csrc/ behind the C ABI of include/acg_ldpc.h.
"""
from ._lib import (ENGINE_AUTO, ENGINE_FUSED, ENGINE_STREAMED, EVENT_NO_WORD, EVENT_NONCODEWORD, EVENT_PSEUDO, PREC_DEFAULT, PREC_F16, PREC_F32, PREC_F64,  # noqa: F401
                   SCHEDULE_FLOODING, SCHEDULE_LAYERED, LdpcError, build, lib)
from .channel import gen_random_codewords, llr, llr_variance, transmit_frames  # noqa: F401
from .code import ParityCheckMatrix  # noqa: F401
from .codes import regular_ldpc  # noqa: F401
from .decoder import (BeliefPropagationDecoder, CascadeDecoder, Decoder, MinSumDecoder, OSDDecoder, QPADMMDecoder, QuantConfig,  # noqa: F401
                      QuantizedMinSumDecoder, StreamedLayeredBPDecoder, StreamedLayeredMinSumDecoder, StreamedQuantizedMinSumDecoder)
from .experiment import (CodesEvaluator, ExperimentDetail, ExperimentResult, merge_cascade_results, merge_exp_details,  # noqa: F401
                         merge_exp_results, quant_structs, rate_match_pattern, run_experiment, run_experiment_cascade,
                         run_experiment_codes, run_experiment_detail, run_experiment_grid, run_experiment_inproc,
                         run_experiment_quants, run_experiment_rm, run_experiment_sharded, shard_range)


def read_pcm(path):
    """utils/parse_data.h:6-25 -> ParityCheckMatrix"""
    return ParityCheckMatrix.read_pcm(path)


def device_available():
    return bool(lib().acg_ldpc_device_available())
