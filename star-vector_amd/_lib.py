"""ctypes binding of libstarvector_hip.so (include/starvector_hip.h: the product ABI; include/starvector_hip_debug.h: the test and
measurement surface of the same library).

The product path has NO fallback: if the HIP library is missing or fails to load this module raises,
and every public entry point of the package goes through it.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libstarvector_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "include", "starvector_hip.h"))
DEBUG_HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "include", "starvector_hip_debug.h"))

ABI_VERSION = 9
SV_DTYPE_BF16, SV_DTYPE_F32 = 0, 1
SV_NORM_LAYER, SV_NORM_BATCH = 0, 1
SV_ARCH_V1, SV_ARCH_V2 = 0, 1
ACT = {"none": 0, "quickgelu": 1, "swish": 2, "gelu_tanh": 3}


class SvConfig(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("vit_width", C.c_int32),
        ("vit_layers", C.c_int32), ("vit_heads", C.c_int32), ("adapter_norm", C.c_int32),
        ("hidden", C.c_int32), ("n_layer", C.c_int32), ("n_head", C.c_int32), ("n_inner", C.c_int32),
        ("vocab", C.c_int32), ("n_positions", C.c_int32), ("max_batch", C.c_int32),
        ("max_seq_len", C.c_int32), ("ln_eps", C.c_float), ("device", C.c_int32),
        ("arch", C.c_int32), ("n_kv_head", C.c_int32), ("rope_theta", C.c_float), ("vit_mlp", C.c_int32),
        ("vit_eps", C.c_float), ("sliding_window", C.c_int32), ("weight_dtype", C.c_int32), ("exclusive_device", C.c_int32),
    ]


class SvSampling(C.Structure):
    _fields_ = [
        ("do_sample", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
        ("max_length", C.c_int32), ("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32),
        ("n_stop", C.c_int32), ("stop_ids", C.POINTER(C.c_int32)), ("seed", C.c_uint64),
        ("sync_every", C.c_int32), ("repetition_penalty", C.c_float),
        ("num_beams", C.c_int32), ("length_penalty", C.c_float), ("early_stopping", C.c_int32),
        ("top_k", C.c_int32), ("on_tokens", C.c_void_p), ("user_data", C.c_void_p),
        ("min_new_tokens", C.c_int32),
    ]


TOKEN_CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32)


class SvCbRequest(C.Structure):
    _fields_ = [
        ("do_sample", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
        ("seed", C.c_uint64), ("max_new_tokens", C.c_int32), ("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32),
        ("min_new_tokens", C.c_int32), ("repetition_penalty", C.c_float), ("n_stop", C.c_int32),
        ("stop_ids", C.c_int32 * 16),
        # ABI 9: vLLM sampler semantics (semantics = 1); all zero = HF, as before
        ("semantics", C.c_int32), ("presence_penalty", C.c_float), ("frequency_penalty", C.c_float), ("min_p", C.c_float),
        ("n_prompt_ids", C.c_int32), ("prompt_ids", C.POINTER(C.c_int32)),
        ("n_logit_bias", C.c_int32), ("logit_bias_ids", C.POINTER(C.c_int32)), ("logit_bias_values", C.POINTER(C.c_float)),
        ("n_stop_any", C.c_int32), ("stop_any_ids", C.c_int32 * 8),
    ]

CB_MAX_LOGIT_BIAS, CB_MAX_STOP_ANY = 128, 8


class SvCbLogprobs(C.Structure):
    # sv_cb_admit_logprobs: what one request of a continuous batch records per emitted token (parallel to the sv_cb_request array)
    _fields_ = [("enable", C.c_int32), ("k", C.c_int32), ("source", C.c_int32)]



class SvBeamConfig(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("num_beams", C.c_int32), ("vocab", C.c_int32), ("max_new", C.c_int32),
        ("eos_token_id", C.c_int32), ("pad_token_id", C.c_int32), ("early_stopping", C.c_int32),
        ("length_penalty", C.c_float), ("repetition_penalty", C.c_float), ("n_stop", C.c_int32),
        ("stop_ids", C.POINTER(C.c_int32)), ("do_sample", C.c_int32), ("temperature", C.c_float),
        ("top_p", C.c_float), ("top_k", C.c_int32), ("seed", C.c_uint64), ("min_new_tokens", C.c_int32),
    ]


class SvGenerateOutputs(C.Structure):
    # sv_generate_ex: per-step outputs (HF output_scores / output_logits, beam search's sequences_scores / beam_indices)
    _fields_ = [
        ("dev_scores", C.c_void_p), ("dev_logits", C.c_void_p), ("ld", C.c_int64),
        ("host_sequences_scores", C.POINTER(C.c_float)), ("host_beam_indices", C.POINTER(C.c_int64)),
    ]


class SvLogitsProcessors(C.Structure):
    # sv_generate_processed: HF's no_repeat_ngram_size / bad_words_ids / min_p (all zero = none)
    _fields_ = [
        ("no_repeat_ngram_size", C.c_int32), ("n_bad_words", C.c_int32),
        ("bad_word_lens", C.POINTER(C.c_int32)), ("bad_word_ids", C.POINTER(C.c_int32)), ("min_p", C.c_float),
    ]

class SvTokenStats(C.Structure):
    # sv_generate_stats: per-token log-prob / processed log-prob / entropy of the roll-out, device fp32 [rows][ld] each (any may be NULL, not all)
    _fields_ = [
        ("dev_logprob", C.c_void_p), ("dev_logprob_processed", C.c_void_p), ("dev_entropy", C.c_void_p), ("ld", C.c_int64),
    ]


class SvTokenTopk(C.Structure):
    # sv_generate_topk: the k best ids / log-probs of every step, device [rows][ld][k], and the emitted token's rank [rows][ld] (may be NULL)
    _fields_ = [
        ("k", C.c_int32), ("source", C.c_int32), ("dev_ids", C.c_void_p), ("dev_logprobs", C.c_void_p), ("dev_rank", C.c_void_p),
        ("ld", C.c_int64),
    ]


class SvLookup(C.Structure):
    # sv_generate_lookup: K drafted tokens per sequence and step, from an n-gram lookup over the generated ids (0 = the default of a field)
    _fields_ = [("num_draft_tokens", C.c_int32), ("max_ngram", C.c_int32), ("min_ngram", C.c_int32)]


LOOKUP_MAX_DRAFT, LOOKUP_MAX_NGRAM = 15, 8      # SV_LOOKUP_MAX_DRAFT, SV_LOOKUP_MAX_NGRAM
TOPK_MAX = 32      # SV_TOPK_MAX
LP_MAX_NGRAM, LP_MAX_BAD_WORDS, LP_MAX_BAD_WORD_LEN = 8, 64, 8


_P = C.c_void_p
_I = C.c_int32
_F = C.c_float

# name -> (restype, argtypes): exactly the prototypes of include/starvector_hip.h
PRODUCT_PROTOTYPES = {
    "sv_abi_version": (_I, []),
    "sv_last_error": (C.c_char_p, []),
    "sv_config_default_1b": (None, [C.POINTER(SvConfig)]),
    "sv_config_default_8b": (None, [C.POINTER(SvConfig)]),
    "sv_create": (_I, [C.POINTER(SvConfig), C.POINTER(_P)]),
    "sv_destroy": (_I, [_P]),
    "sv_create_kv": (_I, [C.POINTER(SvConfig), _I, C.POINTER(_P)]),
    "sv_kv_info": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sv_load_weight": (_I, [_P, C.c_char_p, _P, _I, _I, C.POINTER(C.c_int64), _P]),
    "sv_weights_complete": (_I, [_P]),
    "sv_weight_count": (_I, [_P]),
    "sv_weight_info": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int64), C.POINTER(_I), C.POINTER(_I)]),
    "sv_encode_image": (_I, [_P, _P, _I, _P, _P]),
    "sv_adapter": (_I, [_P, _P, _I, _P, _P]),
    "sv_embed_tokens": (_I, [_P, _P, _I, _P, _P]),
    "sv_adapter_into": (_I, [_P, _P, _I, _P, _I, _P]),
    "sv_embed_tokens_into": (_I, [_P, _P, _I, _I, _P, _I, _I, _P]),
    "sv_preprocess_image": (_I, [_P, _I, _I, _I, _I, _I, C.POINTER(_F), C.POINTER(_F), _P, _P]),
    "sv_preprocess_workspace_bytes": (C.c_int64, [C.POINTER(_I), C.POINTER(_I), _I, _I, _I]),
    "sv_preprocess_images": (_I, [C.POINTER(_P), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I, _I, _I, C.POINTER(_F),
                                  C.POINTER(_F), _P, _P, C.c_int64, _P]),
    "sv_prefill": (_I, [_P, _P, _I, _I, _P, _P]),
    "sv_prefill_ragged": (_I, [_P, _P, _I, C.POINTER(_I), _P, _P]),
    "sv_prefill_open": (_I, [_P, _I, C.POINTER(_I)]),
    "sv_prefill_extend": (_I, [_P, _P, _I, C.POINTER(_I), C.POINTER(_I), _P, _P]),
    "sv_set_prefill_chunk": (_I, [_P, _I]),
    "sv_generate_ragged": (_I, [_P, _P, _I, C.POINTER(_I), C.POINTER(SvSampling), C.POINTER(SvGenerateOutputs), _P, C.POINTER(_I), _P]),
    "sv_generate_shared": (_I, [_P, _P, _I, C.POINTER(_I), _I, _I, C.POINTER(SvSampling), C.POINTER(SvGenerateOutputs), _P, C.POINTER(_I), _P]),
    "sv_generate_processed": (_I, [_P, _P, _I, C.POINTER(_I), _I, _I, C.POINTER(SvSampling), C.POINTER(SvLogitsProcessors),
                                   C.POINTER(SvGenerateOutputs), _P, C.POINTER(_I), _P]),
    "sv_generate_stats": (_I, [_P, _P, _I, C.POINTER(_I), _I, _I, C.POINTER(SvSampling), C.POINTER(SvLogitsProcessors),
                               C.POINTER(SvGenerateOutputs), C.POINTER(SvTokenStats), _P, C.POINTER(_I), _P]),
    "sv_generate_topk": (_I, [_P, _P, _I, C.POINTER(_I), _I, _I, C.POINTER(SvSampling), C.POINTER(SvLogitsProcessors),
                              C.POINTER(SvGenerateOutputs), C.POINTER(SvTokenStats), C.POINTER(SvTokenTopk), _P, C.POINTER(_I), _P]),
    "sv_generate_lookup": (_I, [_P, _P, _I, C.POINTER(_I), _I, C.POINTER(SvSampling), C.POINTER(SvLookup), _P, C.POINTER(_I), C.POINTER(_I), _P]),
    "sv_generate_lookup_sampled": (_I, [_P, _P, _I, C.POINTER(_I), _I, C.POINTER(SvSampling), C.POINTER(SvLookup), _P, C.POINTER(_I), C.POINTER(_I),
                                        _P]),
    "sv_forward_topk": (_I, [_P, _P, _I, _I, _I, _P, _F, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "sv_forward_logprobs_ragged": (_I, [_P, _P, _I, C.POINTER(_I), C.POINTER(_I), _P, _F, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "sv_forward_logprobs_prefixed": (_I, [_P, _P, _I, C.POINTER(_I), _P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _P, _F, _P, _P, _P, _P, _I,
                                          _P, _P, _P, _P]),
    "sv_cb_admit_shared": (_I, [_P, _P, _I, C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(SvCbRequest), C.POINTER(_I), _P]),
    "sv_cb_admit_ragged": (_I, [_P, _P, _I, C.POINTER(_I), C.POINTER(SvCbRequest), C.POINTER(_I), _P]),
    "sv_forward_logits": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "sv_forward_logprobs": (_I, [_P, _P, _I, _I, _I, _P, _F, _P, _P, _P, _P, _P]),
    "sv_decode_step": (_I, [_P, _P, _I, _P, _P]),
    "sv_generate": (_I, [_P, _P, _I, _I, C.POINTER(SvSampling), _P, C.POINTER(_I), _P]),
    "sv_generate_ex": (_I, [_P, _P, _I, _I, C.POINTER(SvSampling), C.POINTER(SvGenerateOutputs), _P, C.POINTER(_I), _P]),
    "sv_cb_admit": (_I, [_P, _P, _I, _I, C.POINTER(SvCbRequest), C.POINTER(_I), _P]),
    "sv_cb_step": (_I, [_P, _I, C.POINTER(_I), _P]),
    "sv_cb_poll": (_I, [_P, C.POINTER(_I), C.POINTER(_I), _I]),
    "sv_cb_read": (_I, [_P, _I, _I, _I, C.POINTER(C.c_int64)]),
    "sv_cb_release": (_I, [_P, _I]),
    "sv_cb_reset": (_I, [_P]),
    "sv_cb_admit_logprobs": (_I, [_P, _P, _I, C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(SvCbRequest), C.POINTER(SvCbLogprobs), C.POINTER(_I), _P]),
    "sv_cb_read_logprobs": (_I, [_P, _I, _I, _I, C.POINTER(_F), C.POINTER(_I), C.POINTER(_I), C.POINTER(_F)]),
    "sv_cb_set_lookup": (_I, [_P, C.POINTER(SvLookup)]),
    "sv_cb_lookup_counts": (_I, [_P, _I, C.POINTER(_I)]),
    "sv_cb_set_prefix_cache": (_I, [_P, _I]),
    "sv_cb_prefix_cache_info": (_I, [_P, C.POINTER(C.c_int64)]),
    "sv_beam_create": (_I, [C.POINTER(SvBeamConfig), C.POINTER(_P)]),
    "sv_beam_destroy": (_I, [_P]),
    "sv_beam_step": (_I, [_P, _P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _P]),
    "sv_beam_finalize": (_I, [_P, C.POINTER(C.c_int64), C.POINTER(_I), C.POINTER(_F), _P]),
    "sv_beam_history": (_I, [_P, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I)]),
    "sv_last_timing": (_I, [_P, C.POINTER(C.c_double)]),
}

# the test / measurement surface: include/starvector_hip_debug.h (same library)
DEBUG_PROTOTYPES = {
    "sv_debug_resample_coeffs": (_I, [_I, _I, C.POINTER(_I), C.POINTER(_I), _I]),
    "sv_debug_gemm_plan": (_I, [_I, _I, _I, _I, C.POINTER(_I)]),
    "sv_debug_skinny_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "sv_debug_set_exp": (_I, [_P, _I]),
    "sv_debug_exp_known": (_I, []),
    "sv_debug_set_col_tiles": (_I, [_I]),
    "sv_debug_set_skinny_form": (_I, [_I]),
    "sv_debug_skinny_form": (_I, []),
    "sv_debug_tailsplit_launches": (_I, [C.POINTER(C.c_int64)]),
    "sv_debug_cols_rowhalf_launches": (_I, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sv_debug_set_gemm_form": (_I, [_I]),
    "sv_debug_set_linear_seq_rows": (_I, [_I]),
    "sv_debug_gemm_seq_form": (_I, [_I, _I, _I, _I]),
    "sv_debug_ragged_plan": (_I, [C.POINTER(_I), _I, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I)]),
    "sv_debug_prefix_plan": (_I, [C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), _I, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I,
                                  C.POINTER(_I)]),
    "sv_debug_prompt_passes": (_I, [_P, C.POINTER(C.c_int64)]),
    "sv_debug_extend_plan": (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I)]),
    "sv_debug_kv_gather": (_I, [_P, _I, _I, _I, _P, _P]),
    "sv_debug_page_digests": (_I, [_P, _I, C.POINTER(_I), _I, _I, _I, C.POINTER(C.c_uint64), _P]),
    "sv_debug_prefix_hit": (_I, [C.POINTER(C.c_uint64), _I, _I, C.POINTER(C.c_uint64), _I, C.POINTER(C.c_uint64), C.POINTER(_I)]),
    "sv_debug_shared_plan": (_I, [C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_int64)]),
    "sv_debug_block_table": (_I, [_P, _I, C.POINTER(_I), _I]),
    "sv_debug_free_pages": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "sv_debug_attn_plan": (_I, [_I, _I, _I, C.POINTER(_I)]),
    "sv_debug_rowln_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I)]),
    "sv_debug_rowln_occupancy": (_I, [_I, C.POINTER(_I)]),
    "sv_debug_step_plan": (_I, [_P, C.POINTER(_I)]),
    "sv_debug_attn_trace": (_I, [_P, C.POINTER(C.c_int64), _I]),
    "sv_debug_mlp_trace": (_I, [_P, C.POINTER(C.c_int64), _I]),
    "sv_debug_xcc_map": (_I, [_P, _I, _I, C.POINTER(_I)]),
    "sv_debug_occupy_cus": (_I, [_P, _I, _I, _I]),
    "sv_debug_gemm_trace": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int64), _I]),
    "sv_debug_kv_load": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "sv_debug_kv_read": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "sv_debug_attn_decode": (_I, [_P, _I, _P, _I, _P, _I, _P]),
    "sv_debug_attn_decode_slabs": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P]),
    "sv_debug_attn_decode_draft": (_I, [_P, _I, _P, _I, _P, _I, _I, _P, _P]),
    "sv_debug_set_lookup_drafts": (_I, [_P, C.POINTER(_I), _I, _I]),
    "sv_op_lookup_accept": (_I, [C.POINTER(_I), C.POINTER(_I), _I, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I,
                                 _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _P]),
    "sv_op_lookup_draft": (_I, [C.POINTER(_I), _I, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _P]),
    "sv_op_lookup_hold": (_I, [_P, _I, _I, _I, _I, _I, C.POINTER(_I), _P]),
    "sv_op_lookup_sample": (_I, [_P, _I, _I, _I, _I, C.POINTER(_I), _F, _I, _F, C.c_uint64, C.POINTER(C.c_uint32), _I, _F, C.POINTER(_I),
                                 C.POINTER(_F), C.POINTER(_I), _P]),
    "sv_op_lookup_seen": (_I, [C.POINTER(_I), _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(C.c_uint32),
                               C.POINTER(C.c_uint32), _P]),
    "sv_debug_decode_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "sv_profile_decode_step": (_I, [_P, _I, _I, C.POINTER(C.c_double), _P]),
    "sv_profile_ttft": (_I, [_P, _P, _I, _P, _I, _I, C.POINTER(C.c_double), _P]),
    "sv_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "sv_op_linear": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_op_linear_skinny": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sv_op_linear_skinny_fp8": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sv_op_linear_skinny_epi": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_op_linear_skinny_epi_fp8": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_op_linear_fp8": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_op_pack_weight_fp8": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "sv_op_pack_weight_mxfp4": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "sv_op_linear_skinny_mxfp4": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_op_linear_skinny_epi_mxfp4": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sv_op_lm_head_argmax": (_I, [_P, _P, _P, C.POINTER(_I), _I, _I, _I, _P]),
    "sv_op_decode_proj_fold": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sv_bench_linear": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _P]),
    "sv_bench_decode_linear": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_double), _P]),
    "sv_op_cvt_bf16_hw": (_I, [_P, _P, C.c_int64, _P]),
    "sv_op_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P]),
    "sv_op_attention_prefill": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, C.POINTER(_I), _I, _I, _I, _I, _F, _I, _I, _P]),
    "sv_op_attn_prefill_prefixed": (_I, [_P, _I, _I, _I, _I, _P, _I, C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), _I, _I, _I, _F, _I, _P]),
    "sv_op_plane_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "sv_op_plane_layernorm_strided": (_I, [_P, _P, _P, _P, _I, _I, _F, C.c_int64, _P]),
    "sv_op_im2col": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sv_op_vit_embed_lnpre": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "sv_op_dec_embed": (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    "sv_op_gather_rows": (_I, [_P, _P, _P, _I, _I, _I, C.c_int64, _P]),
    "sv_op_gather_last_rows": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "sv_op_gather_tail_rows": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sv_op_gather_tail_rows_ragged": (_I, [_P, _P, _I, _I, _P, _I, _P]),
    "sv_op_gather_listed_rows": (_I, [_P, _I, _P, _I, _P, _I, _P]),
    "sv_op_ragged_row_pos": (_I, [_P, _I, _P, _P]),
    "sv_op_ragged_positions": (_I, [_P, _P, _I, _I, _I, _P]),
    "sv_op_token_batchnorm": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, C.c_int64, _P]),
    "sv_op_layernorm_packed": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "sv_op_pack_rows": (_I, [_P, _I, _P, _I, _I, _P]),
    "sv_op_unpack_rows": (_I, [_P, _P, _I, _I, _I, _P]),
    "sv_op_row_update_ln": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _P]),
    "sv_op_argmax": (_I, [_P, _I, _I, _I, _P, _P]),
    "sv_op_sample_top_p": (_I, [_P, _I, _I, _I, _F, _F, C.c_uint64, _I, _P, _P]),
    "sv_op_sample": (_I, [_P, _I, _I, _I, _F, _I, _F, C.c_uint64, _I, _P, _P]),
    "sv_op_capture_rows": (_I, [_P, _I, _I, _I, _P, _I, _F, _I, _I, _I, _F, _I, _F, _F, _P, _P, C.c_int64, _P]),
    "sv_debug_beam_set_capture": (_I, [_P, _P, _P, C.c_int64, _I]),
    "sv_op_logprob_rows": (_I, [_P, _I, _I, _I, _P, _F, _P, _P, _P, _P, C.POINTER(_I), _P]),
    "sv_debug_set_score_chunk_rows": (_I, [_P, _I]),
    "sv_op_topk_rows_bf16": (_I, [_P, _I, _I, _I, _P, _F, _P, _I, _P, _P, _P, _P]),
    "sv_op_token_topk": (_I, [_P, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P]),
    "sv_op_ban_tokens": (_I, [_P, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(SvLogitsProcessors), _P]),
    "sv_op_cb_select": (_I, [_P, _I, _I, _I, C.POINTER(SvCbRequest), C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I), _P]),
    "sv_op_cb_logprobs": (_I, [_P, _I, _I, _I, C.POINTER(SvCbRequest), C.POINTER(SvCbLogprobs), C.POINTER(_I), _I, C.POINTER(_I), C.POINTER(_I),
                               C.POINTER(_F), C.POINTER(_I), C.POINTER(_I), C.POINTER(_F), _I, _P]),
    "sv_debug_cb_set_lookup_drafts": (_I, [_P, C.POINTER(_I), _I, _I]),
    "sv_op_cb_lookup_step": (_I, [_P, _I, _I, _I, _I, C.POINTER(SvCbRequest), C.POINTER(SvCbLogprobs), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I,
                                  C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I), _I, _I, C.POINTER(_I),
                                  C.POINTER(_I), C.POINTER(_F), C.POINTER(_I), _P]),
}

PROTOTYPES = {**PRODUCT_PROTOTYPES, **DEBUG_PROTOTYPES}

_lib = None


class StarVectorHipError(RuntimeError):
    pass


class StarVectorBusy(StarVectorHipError):
    """sv_cb_admit: no free slot / KV pages right now (SV_EBUSY); release finished requests and retry."""


def load() -> C.CDLL:
    """Load the HIP library or raise.  Never falls back to another implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StarVectorHipError(
            f"{LIB_PATH} is missing: the HIP engine has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `python star-vector_amd/build.py`); "
            "there is no CPU/PyTorch fallback for this path.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise StarVectorHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise StarVectorHipError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.sv_abi_version() != ABI_VERSION:
        raise StarVectorHipError(f"ABI version mismatch: library {lib.sv_abi_version()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    """Map C return codes onto the exceptions the reference's callers already catch
    (serve/model_worker.py:183-207 handles ValueError / RuntimeError)."""
    if rc == 0:
        return
    msg = load().sv_last_error().decode("utf-8", "replace")
    text = f"{what}: {msg}" if what else msg
    if rc == -22:
        raise ValueError(text)
    if rc == -2:
        raise KeyError(text)
    if rc == -95:
        raise NotImplementedError(text)
    if rc == -16:
        raise StarVectorBusy(text)
    raise StarVectorHipError(f"{text} (code {rc})")
