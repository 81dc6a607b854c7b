"""ctypes binding of libsat_hip.so (C ABI: include/sat_hip.h).

The library is the product: there is NO CPU or eager-PyTorch fallback.  If it is missing or a kernel call
fails, a RuntimeError is raised -- nothing is computed another way.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAT_LIB") or os.path.join(_HERE, "libsat_hip.so")    # SAT_LIB: A/B another build of the same ABI

ABI_VERSION = 18
SAT_OK, SAT_ERR_ARG, SAT_ERR_WORKSPACE, SAT_ERR_UNSUPPORTED = 0, 1001, 1002, 1003     # include/sat_hip.h
SAT_F32, SAT_BF16 = 0, 1
OP_IMAGE_PREP, OP_CONV, OP_BN_FINALIZE, OP_BN_RELU, OP_BN_ADD_RELU, OP_BN_RELU_MAXPOOL, OP_AVGPOOL = 1, 2, 3, 4, 5, 6, 7

OP_BN_EVAL_BATCH = 8
OP_MAXPOOL2 = 9
OP_MAXPOOL3S2, OP_AVGPOOL3 = 10, 11
OP_GRAM, OP_GRAM_COV, OP_GEMM_BF16_NT, OP_BN_FROM_GRAM = 12, 13, 14, 15
CONV_PADW = 2
CONV_GROUP_TABLE = 4
CONV_IN_RESIDUAL = 8

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


class SatBnEvalItem(C.Structure):
    """mirror of `struct sat_bn_eval_item` (include/sat_hip.h)"""
    _fields_ = [("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp),
                ("scale_out", _vp), ("shift_out", _vp), ("C", C.c_int32), ("reserved", C.c_int32)]


class SatBnRunningItem(C.Structure):
    """mirror of `struct sat_bn_running_item` (include/sat_hip.h)"""
    _fields_ = [("running_mean", _vp), ("running_var", _vp), ("batch_mean", _vp), ("batch_var", _vp),
                ("C", C.c_int32), ("reserved", C.c_int32)]


class SatCiderCorpus(C.Structure):
    """mirror of `struct sat_cider_corpus` (include/sat_hip.h)"""
    _fields_ = [("table_keys", _vp), ("table_nodes", _vp), ("df", _vp), ("ref_tokens", _vp), ("ref_offsets", _vp),
                ("image_offsets", _vp), ("ref_norm", _vp), ("capacity", C.c_int64), ("n_tokens", C.c_int64),
                ("n_nodes", C.c_int32), ("n_refs", C.c_int32), ("n_images", C.c_int32), ("max_ref_tokens", C.c_int32)]


class SatRefCorpus(C.Structure):
    """mirror of `struct sat_ref_corpus` (include/sat_hip.h)"""
    _fields_ = [("ref_tokens", _vp), ("ref_offsets", _vp), ("image_offsets", _vp), ("n_tokens", C.c_int64),
                ("n_refs", C.c_int32), ("n_images", C.c_int32), ("max_ref_tokens", C.c_int32), ("reserved", C.c_int32)]


class SatBeamConstraints(C.Structure):
    """mirror of `sat_beam_constraints` (include/sat_hip.h)"""
    _fields_ = [("suppress_ids", _vp), ("n_suppress", C.c_int), ("min_length", C.c_int), ("no_repeat_ngram", C.c_int),
                ("block_repeat", C.c_int), ("length_penalty", C.c_float)]


class SatSampleConstraints(C.Structure):
    """mirror of `sat_sample_constraints` (include/sat_hip.h)"""
    _fields_ = [("suppress_ids", _vp), ("n_suppress", C.c_int), ("min_length", C.c_int), ("no_repeat_ngram", C.c_int),
                ("block_repeat", C.c_int), ("repetition_penalty", C.c_float), ("end_id", C.c_int64)]


class SatDecoderModel(C.Structure):
    """mirror of `sat_decoder_model` (include/sat_hip.h): one DecoderRNN of an ensemble, host struct of device pointers"""
    _fields_ = [("features", _vp), ("embed", _vp), ("lstm_w", C.POINTER(_vp)), ("num_layers", C.c_int), ("lin_w", _vp), ("lin_b", _vp),
                ("E", C.c_int), ("H", C.c_int)]


class SatOp(C.Structure):
    """mirror of `struct sat_op` (include/sat_hip.h); no instance attributes besides the fields, so a misspelt field raises"""
    __slots__ = ()
    _fields_ = [
        ("kind", C.c_int32), ("dtype", C.c_int32),
        ("in0", _vp), ("in1", _vp), ("out", _vp), ("w", _vp),
        ("scale0", _vp), ("shift0", _vp), ("scale1", _vp), ("shift1", _vp),
        ("stat_partial", _vp), ("gamma", _vp), ("beta", _vp),
        ("running_mean", _vp), ("running_var", _vp), ("scale_out", _vp), ("shift_out", _vp),
        ("N", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Cin", C.c_int32),
        ("Hout", C.c_int32), ("Wout", C.c_int32), ("Cout", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("training", C.c_int32), ("tiles_m", C.c_int32),
        ("sN", C.c_int64), ("sH", C.c_int64), ("sW", C.c_int64), ("count", C.c_int64),
        ("momentum", C.c_float), ("eps", C.c_float),
        ("variant", C.c_int32), ("flags", C.c_int32),
        ("stat_acc", _vp), ("stat_acc1", _vp), ("gamma1", _vp), ("beta1", _vp),
        ("running_mean1", _vp), ("running_var1", _vp), ("w_packed", _vp),
        ("reserved1", C.c_int32 * 2),
        ("pad_w", C.c_int32), ("groups", C.c_int32), ("ldc", C.c_int64), ("out1", C.c_void_p),
    ]


def op(kind, dtype, **fields):
    """one `SatOp`: tensors given for pointer fields stand for their `data_ptr()`; a name that is not a field raises"""
    return SatOp(kind=kind, dtype=dtype, **{k: v.data_ptr() if hasattr(v, "data_ptr") else v for k, v in fields.items()})


# name -> (restype, argtypes): every symbol include/sat_hip.h declares
SIGNATURES = {
    "sat_version": (_i, []),
    "sat_error_string": (C.c_char_p, [_i]),
    "sat_gemm_f32": (_i, [_i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i, _i, _i, _vp]),
    "sat_run_ops": (_i, [C.POINTER(SatOp), _i, _vp]),
    "sat_run_ops_parity": (_i, [C.POINTER(SatOp), _i, _i, _vp]),
    "sat_graph_create": (_i, [C.POINTER(SatOp), _i, _i, C.POINTER(_vp)]),
    "sat_graph_launch": (_i, [_vp, _vp]),
    "sat_graph_destroy": (_i, [_vp]),
    "sat_conv_bn_relu_fwd": (_i, [C.POINTER(SatOp), C.POINTER(SatOp), C.POINTER(SatOp), _vp]),
    "sat_conv_tiles_m": (_i, [_i64]),
    "sat_counter_add": (_i, [_vp, _i, _i64, _vp]),
    "sat_conv_variant_signature": (_i, [_i]),
    "sat_conv_variant_family": (_i, [_i]),
    "sat_gram_rows_per_slab": (_i, [_i64, _i]),
    "sat_gram_slabs": (_i, [_i64, _i]),
    "sat_gram_slab_floats": (_i64, [_i64, _i]),
    "sat_conv_num_variants": (_i, []),
    "sat_conv_default_variant": (_i, [C.POINTER(SatOp), _i]),
    "sat_conv_resolved_variant": (_i, [C.POINTER(SatOp)]),
    "sat_conv_pack_weights": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sat_conv_autotune": (_i, [C.POINTER(SatOp), _i, _i, _vp, _i64, _vp]),
    "sat_conv_autotune_topk": (_i, [C.POINTER(SatOp), _i, _i, _vp, _i64, _vp, _i, C.POINTER(C.c_int32)]),
    "sat_run_ops_timed": (_i, [C.POINTER(SatOp), _i, _i, _vp, C.POINTER(C.c_float)]),
    "sat_validate_ids": (_i, [_vp, _i64, _i, _i, _i64, _i64, _vp, _vp]),
    "sat_fc_bn1d_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_fc_bn1d_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_fc_bn1d_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_embed_concat_fwd": (_i, [_vp, _vp, _vp, _i64, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sat_embed_concat_bwd": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sat_pack_targets": (_i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
    "sat_lstm_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_lstm_mixed_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_lstm_fwd_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_lstm_bwd_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, _i,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_lstm_fwd_ws_bytes": (_i64, [_i, _i]),
    "sat_lstm_fwd_status_offset": (_i64, [_i, _i]),
    "sat_lstm_fwd_plan": (_i, [_i, _i, _i]),
    "sat_lstm_bwd_plan": (_i, [_i, _i, _i]),
    "sat_lstm_persist_enable": (_i, [_i]),
    "sat_lstm_bwd_ws_bytes": (_i64, [_i, _i]),
    "sat_lstm_bwd_ws_bytes_full": (_i64, [_i, _i, _i, _i]),
    "sat_lstm_bwd_status_offset": (_i64, [_i, _i, _i, _i]),
    "sat_lstm_bwd_ws_bytes_max": (_i64, [_i, _i, _i, _i]),
    "sat_lstm_ws_release": (_i, [_vp]),
    "sat_lstm_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, _i,
                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_vocab_logits_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "sat_ce_rows": (_i, [_vp, _i64, _vp, _i, _i, _f, _i, _vp, _vp, _vp]),
    "sat_vocab_ce_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp]),
    "sat_vocab_bf16_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_vocab_ce_fwd_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "sat_vocab_ce_bwd_bf16": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_gemm_bf16_nt": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i, _i, _i, _i64, _vp]),
    "sat_transpose_f32_bf16": (_i, [_vp, _i64, _i, _i, _vp, _i64, _vp]),
    "sat_vocab_ce_bwd": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_vocab_ce_bwd_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_gemm_f32_splitk": (_i, [_i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _i64, _vp]),
    "sat_gemm_f32x3_packed_bytes": (_i64, [_i, _i]),
    "sat_gemm_f32x3_pack": (_i, [_vp, _i, _i, _vp, _vp]),
    "sat_gemm_f32x3": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _i, _vp]),
    "sat_sum_slabs_f32": (_i, [_vp, _i, _i64, _i64, _vp, _vp]),
    "sat_skinny_gemm_f32": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_skinny_gemm_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_skinny_gemm2_f32": (_i, [_vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_vocab_argmax": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _i64, _vp]),
    "sat_vocab_argmax_ws_bytes": (_i64, [_i, _i]),
    "sat_lstm_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "sat_embed_rows": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp]),
    "sat_attention_fwd": (_i, [_vp, _vp, _vp, _i64, _vp, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_attention_bwd": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_attention_ws_bytes": (_i64, [_i, _i]),
    "sat_attention_coverage_ws_bytes": (_i64, [_i, _i]),
    "sat_attention_coverage": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_attention_bwd_ex": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i, _i, _vp, _vp, _vp, _vp,
                                  _vp, _i64, _vp]),
    "sat_bn_running_apply": (_i, [_vp, _i, _f, _vp]),
    "sat_pad_nhwc_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "sat_maxpool2_bwd_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sat_bcast_add_f32": (_i, [_vp, _i, _i, _i, _f, _vp, _vp]),
    "sat_lstmcell_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sat_rows_copy": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _i, _vp, _i64, _vp]),
    "sat_rows_sum": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp]),
    "sat_rows_add": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp, _i64, _vp]),
    "sat_pack_tokens": (_i, [_vp, _i64, _vp, _i, _i, _i, _vp, _vp]),
    "sat_scatter_rows_add": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sat_lstmcell_bwd_point": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "sat_collate_captions": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "sat_gather_rows_f32": (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    "sat_image_augment_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp]),
    "sat_beam_step": (_i, [_vp, _i64, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_beam_step_ws_bytes": (_i64, [_i, _i]),
    "sat_beam_gather_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sat_beam_backtrack": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "sat_beam_backtrack_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sat_kept_tokens": (_i, [_vp, _i64, _i, _i, _i64, _vp, _vp]),
    "sat_beam_decode_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "sat_beam_decode": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64, _vp, _vp, _vp, _i64, _vp]),
    "sat_beam_step_ex": (_i, [_vp, _i64, _vp, _vp, _i64, _i, _i, _i, C.POINTER(SatBeamConstraints), _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                              _i64, _vp]),
    "sat_beam_step_ex_ws_bytes": (_i64, [_i, _i, _i, _i]),
    "sat_beam_rerank": (_i, [_vp, _vp, _i, _i, _i, _i64, _f, _vp, _vp, _vp, _vp, _vp]),
    "sat_beam_decode_ex_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "sat_beam_decode_ex": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64, C.POINTER(SatBeamConstraints),
                                _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_beam_step_groups": (_i, [_vp, _i64, _vp, _vp, _i64, _i, _i, _i, C.POINTER(SatBeamConstraints), _vp, _vp, _i, _i, _i, _f, _vp, _vp,
                                  _vp, _vp, _i64, _vp]),
    "sat_beam_step_groups_ws_bytes": (_i64, [_i, _i, _i, _i]),
    "sat_beam_decode_groups_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "sat_beam_decode_groups": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64, C.POINTER(SatBeamConstraints),
                                    _i, _f, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_ensemble_logprobs": (_i, [C.POINTER(_vp), _i, _i64, C.POINTER(_f), _i, _i, _i, _vp, _i64, _vp]),
    "sat_beam_decode_ensemble_ws_bytes": (_i64, [C.POINTER(SatDecoderModel), _i, _i, _i, _i, _i]),
    "sat_beam_decode_ensemble": (_i, [C.POINTER(SatDecoderModel), _i, C.POINTER(_f), _i, _i, _i, _i, _i, _i64,
                                      C.POINTER(SatBeamConstraints), _i, _f, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_greedy_decode": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_ss_decoder_fwd_ws_bytes": (_i64, [_i, _i]),
    "sat_vocab_sample": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i64, _f, C.c_uint64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i, _vp,
                              _vp, _i64, _vp]),
    "sat_ss_decoder_fwd": (_i, [_vp, _vp, _vp, _i64, C.POINTER(C.c_int32), _vp, _i, _i, _i, C.POINTER(_vp), _i, _i, _vp, _vp,
                                C.POINTER(_vp), _vp, _vp, _i64, _f, C.c_uint64, _i, _vp, _i64, _vp, _i64, _vp]),
    "sat_ss_attend_fwd_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i]),
    "sat_ss_attend_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(C.c_int32), _vp, _i, _i, _i, _i, _i, _i, C.POINTER(_vp),
                               C.POINTER(_vp), _vp, _vp, _i64, _f, C.c_uint64, _i, _vp, _i64, _vp, _i64, _vp]),
    "sat_cider_table_insert": (_i, [_vp, _i, _vp, _vp, _i64, _vp, _vp]),
    "sat_cider_ref_stats": (_i, [C.POINTER(SatCiderCorpus), _vp, _vp]),
    "sat_cider_score": (_i, [C.POINTER(SatCiderCorpus), _vp, _i64, _i, _i, _vp, _i64, _vp, C.c_double, _vp, _vp, _vp]),
    "sat_consensus_ws_bytes": (_i64, [_i, _i]),
    "sat_consensus_rerank": (_i, [C.POINTER(SatCiderCorpus), _vp, _i64, _i64, _i, _i, _i, _vp, _i64, C.c_double, _vp, _vp, _vp, _vp, _vp,
                                  _i64, _vp]),
    "sat_bleu_comps": (_i, [C.POINTER(SatRefCorpus), _vp, _i64, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sat_bleu_finalize": (_i, [_vp, _vp, _vp]),
    "sat_rouge_l_score": (_i, [C.POINTER(SatRefCorpus), _vp, _i64, _i, _i, _vp, _i64, _vp, C.c_double, _vp, _vp, _vp]),
    "sat_rollout_decoder_fwd_ws_bytes": (_i64, [_i, _i]),
    "sat_rollout_decoder_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(_vp), _i, _i, _vp, _vp, C.POINTER(_vp), _vp, _vp, _i64,
                                     C.c_uint64, _i, _vp, _i64, _vp, _i64, _vp]),
    "sat_scst_weights": (_i, [_vp, _i64, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sat_ce_rows_weighted": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "sat_scst_weights_group": (_i, [_vp, _i64, _i, _i, _i, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sat_group_sum_rows": (_i, [_vp, _i64, _i, _i, _i64, _vp, _i64, _vp]),
    "sat_ce_rows_ls": (_i, [_vp, _i64, _vp, _i, _i, _f, _f, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "sat_vocab_ce_fwd_bf16_ls": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sat_ce_rows_ul": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sat_vocab_ce_fwd_bf16_ul": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _i64, _vp]),
    "sat_rollout_attend_fwd_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i]),
    "sat_rollout_attend_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _i64,
                                    _i, _i64, C.c_uint64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "sat_sample_filtered_ws_bytes": (_i64, [_i, _i]),
    "sat_sample_filtered": (_i, [_vp, _i64, _i, _i, _f, _i, _f, C.c_uint64, _i, _i, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "sat_sample_decode_ws_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "sat_sample_decode": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _f, C.c_uint64, _i, _vp, _vp, _vp,
                               _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "sat_sample_filtered_ex": (_i, [_vp, _i64, _i, _i, _f, _i, _f, C.c_uint64, _i, _i, _vp, _i64, _vp, _vp, C.POINTER(SatSampleConstraints),
                                    _vp, _i64, _vp, _i64, _vp]),
    "sat_sample_decode_ex_ws_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "sat_sample_decode_ex": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _f, C.c_uint64, _i, _vp, _vp, _vp,
                                  _vp, _vp, _i64, _vp, _vp, _vp, _i64, C.POINTER(SatSampleConstraints), _vp, _i64, _vp]),
    "sat_dropout_f32": (_i, [_vp, _i64, _vp, _i64, _i, _i, _f, C.c_uint64, _i, _i, _vp]),
    "sat_clamp_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp]),
    "sat_clamp_adam_step_guarded": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp, _vp]),
    "sat_step_fault_flag": (_i, [C.POINTER(_vp), _i, _vp, _vp, _vp]),
    "sat_grad_sumsq_partials": (_i, [_i64]),
    "sat_grad_sumsq_ws_bytes": (_i64, [_i64]),
    "sat_grad_sumsq": (_i, [_vp, _i64, _f, _vp, _i, _i, _vp]),
    "sat_adamw_step": (_i, [_vp, _vp, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _f, C.POINTER(_i64), _i, _f, _vp, _i, _vp, _vp, _vp]),
    "sat_ema_update": (_i, [_vp, _vp, _i64, _f, _vp, _vp, _vp]),
    "sat_swap_f32": (_i, [_vp, _vp, _i64, _vp]),
    "sat_grad_accumulate": (_i, [_vp, _vp, _i64, _f, _i, _vp]),
    "sat_colsum_f32": (_i, [_vp, _i64, _i, _i, _vp, _vp]),
    "sat_cast_f32_bf16": (_i, [_vp, _vp, _i64, _vp]),
    "sat_cast_bf16_f32": (_i, [_vp, _vp, _i64, _vp]),
    "sat_vocab_logp_ws_bytes": (_i64, [_i, _i, _i]),
    "sat_vocab_logp_ws_bytes_rows": (_i64, [_i, _i, _i, _i]),
    "sat_vocab_logp": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    "sat_caption_logp_sum": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    "sat_score_captions_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "sat_score_captions": (_i, [_vp, _vp, C.POINTER(_vp), _i, _vp, _vp, _vp, _i64, _i, _vp, _vp, C.POINTER(C.c_int32), _vp, _i, _i, _i, _i,
                                _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
}

# Symbols added since ABI_VERSION was last raised (additions do not raise it).  Another build of the same ABI version -- SAT_LIB,
# or a -DSAT_TESTHOOKS build made before the addition -- need not export them: they are bound where present, and a call through a
# library that lacks one raises AttributeError (nothing is computed another way).  The library built from this tree exports
# every one (tests/test_cabi_and_host.py, tests/test_conv_cases_host.py).
ADDED_WITHIN_ABI = ("sat_conv_resolved_variant", "sat_image_augment_u8", "sat_attention_coverage_ws_bytes", "sat_attention_coverage",
                    "sat_attention_bwd_ex", "sat_beam_backtrack_rows", "sat_cider_table_insert", "sat_cider_ref_stats", "sat_cider_score",
                    "sat_rollout_decoder_fwd_ws_bytes", "sat_rollout_decoder_fwd", "sat_scst_weights", "sat_ce_rows_weighted",
                    "sat_rollout_attend_fwd_ws_bytes", "sat_rollout_attend_fwd", "sat_bleu_comps", "sat_bleu_finalize",
                    "sat_rouge_l_score", "sat_sample_filtered_ws_bytes", "sat_sample_filtered", "sat_sample_decode_ws_bytes",
                    "sat_sample_decode", "sat_dropout_f32", "sat_beam_step_ex", "sat_beam_step_ex_ws_bytes", "sat_beam_rerank",
                    "sat_beam_decode_ex_ws_bytes", "sat_beam_decode_ex", "sat_beam_step_groups", "sat_beam_step_groups_ws_bytes",
                    "sat_beam_decode_groups_ws_bytes", "sat_beam_decode_groups", "sat_ce_rows_ls", "sat_vocab_ce_fwd_bf16_ls",
                    "sat_grad_sumsq_partials", "sat_grad_sumsq_ws_bytes", "sat_grad_sumsq", "sat_adamw_step",
                    "sat_ensemble_logprobs", "sat_beam_decode_ensemble_ws_bytes", "sat_beam_decode_ensemble",
                    "sat_consensus_ws_bytes", "sat_consensus_rerank", "sat_scst_weights_group", "sat_group_sum_rows",
                    "sat_sample_filtered_ex", "sat_sample_decode_ex_ws_bytes", "sat_sample_decode_ex", "sat_vocab_logp_ws_bytes",
                    "sat_vocab_logp_ws_bytes_rows", "sat_vocab_logp", "sat_caption_logp_sum", "sat_score_captions_ws_bytes",
                    "sat_score_captions", "sat_ce_rows_ul", "sat_vocab_ce_fwd_bf16_ul", "sat_ema_update", "sat_swap_f32",
                    "sat_grad_accumulate", "sat_lstm_fwd_plan", "sat_lstm_bwd_plan")

_lib = None


def open_library(path):
    """dlopen one build of the library and bind every declared symbol (tests bind the -DSAT_TESTHOOKS build this way)"""
    if not os.path.exists(path):
        raise RuntimeError(
            "show-and-tell_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if name in ADDED_WITHIN_ABI and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)       # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.sat_version() != ABI_VERSION:
        raise RuntimeError("%s: ABI version mismatch" % path)
    return lib


def load():
    """dlopen libsat_hip.so once; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH)
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = load().sat_error_string(rc)
        raise RuntimeError("libsat_hip %s failed: [%d] %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """device pointer of a torch tensor; None and a raw address pass through."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def rows(t, row0=0):
    """device pointer of row `row0` of a 2-D contiguous f32 tensor"""
    return t.data_ptr() + row0 * t.shape[1] * 4


def stream():
    """torch's current HIP stream as a raw hipStream_t: every kernel is launched on it."""
    import torch
    return torch.cuda.current_stream().cuda_stream


def pad4(n):
    """n rounded up to 4: the row length of logits and their gradients (rows padded to 4 floats, zero pad columns)"""
    return (n + 3) // 4 * 4


def logits_buffer(N, V, device):
    """f32 [N, pad4(V)] for N rows of V logits, the pad columns zero"""
    import torch
    return torch.zeros(N, pad4(V), device=device) if V % 4 else torch.empty(N, V, device=device)


def pad_rows4(d):
    """d f32 [N, V] as a contiguous [N, pad4(V)] with zero pad columns (an incoming d(loss)/d(logits))"""
    import torch
    V = d.shape[1]
    if V % 4 == 0:
        return d.contiguous()
    out = torch.zeros(d.shape[0], pad4(V), device=d.device)
    out[:, :V] = d
    return out


def workspace256(nbytes, device):
    """(uint8 tensor, address): `nbytes` of workspace whose address is a multiple of 256; the tensor keeps it alive"""
    import torch
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256


def require_gpu(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError("show-and-tell_amd: %s must live on the MI355X (got a %s tensor); the HIP path has no CPU fallback"
                           % (name, t.device))


def counter_add(t, value=1):
    """t += value for an int64 device tensor (BatchNorm's `num_batches_tracked`), through the library: no torch operator computes
    anything on the product path"""
    check(load().sat_counter_add(t.data_ptr(), t.numel(), value, stream()), "sat_counter_add")


_SKINNY_WS = {}
_SKINNY_ROWS = int(os.environ.get("SAT_SKINNY_ROWS", "128"))   # per-step GEMMs with at most this many rows take the split-K kernel


def gemm_splits_k(amode, bmode, lda, ldb, ldc, M, N, K, bias2=None):
    """whether `gemm` hands this call to sat_skinny_gemm_f32.  Its K split depends on M, so a row of its result does too; a row
    of sat_gemm_f32's does not (callers that encode a matrix once and repeat the result ask here)"""
    return amode == 0 and M <= _SKINNY_ROWS and bias2 is None and ldc == N and K % 4 == 0 and lda % 4 == 0 and (bmode == 1 or ldb % 4 == 0)


def gemm(lib, amode, bmode, A, lda, B, ldb, Cout, ldc, M, N, K, bias=None, bias2=None):
    """C[M,N] = op(A) op(B) + bias (+ bias2), f32; A, B, Cout: tensors or raw addresses.  A 64 x 64-tiled GEMM of a 64-row decode
    step runs on N/64 workgroups; those go to sat_skinny_gemm_f32, which splits K over waves and grid slices instead."""
    if gemm_splits_k(amode, bmode, lda, ldb, ldc, M, N, K, bias2):
        import torch
        need = lib.sat_skinny_gemm_ws_bytes(M, N, K)
        dev = torch.cuda.current_device()
        ws = _SKINNY_WS.get(dev)
        if ws is None or ws.numel() * 4 < need:
            ws = _SKINNY_WS[dev] = torch.empty(max(need // 4, 1 << 20), dtype=torch.float32, device="cuda")
        check(lib.sat_skinny_gemm_f32(ptr(A), lda, ptr(B), ldb, bmode, M, N, K, ptr(bias), ptr(Cout), ldc,
                                      ws.data_ptr(), ws.numel() * 4, stream()), "sat_skinny_gemm_f32")
        return
    check(lib.sat_gemm_f32(amode, bmode, ptr(A), lda, ptr(B), ldb, ptr(Cout), ldc, ptr(bias), ptr(bias2), M, N, K, stream()),
          "sat_gemm_f32")
