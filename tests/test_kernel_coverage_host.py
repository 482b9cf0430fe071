"""CPU: every __global__ kernel under star-vector_amd/csrc is accounted for.

COVERAGE maps each kernel name to either
  * a tuple of tests, "file::function" under tests/, that hold it to a reference -- for a kernel that is only held to the BITS of
    another kernel (rowln_cattn_kernel, mlp_fused_kernel, the mt2 / mt2x decode GEMMs) the test of that identity first, then a test that
    holds the kernel it is compared with to a reference; or
  * a one-line reason (a string) why no test holds it to a reference.
The test fails when a kernel of the sources is missing here, when an entry names a kernel that is gone, or when a named test does not
exist (the test files are parsed with ast: nothing is imported, no GPU is needed).  "(engine)" marks a kernel without an operator-level
entry point: the named tests reach it through the engine and would fail if it were wrong, but do not isolate it."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "star-vector_amd", "csrc")

OPS = "test_gpu_ops.py::"
ROWS = "test_gpu_row_kernels.py::"
E2E = "test_gpu_e2e.py::"
BEAM = "test_gpu_beam.py::"
LONG = "test_gpu_long_context.py::"
DH64 = "test_gpu_decoder_head_dim64.py::"
FP8 = "test_gpu_fp8_ops.py::"
KEPT = "test_gpu_warper_kept_set.py::"                             # the warper's kept set, exactly, against float64 (tests/warp_rows.py)

_ROW_UPDATE = (ROWS + "test_row_update_residual_mode_sums_the_slabs_in_order", ROWS + "test_row_update_embedding_mode", ROWS + "test_eps_row_update")
_BIG_M = (OPS + "test_linear_mfma", OPS + "test_linear_big_m_kernels_agree_bitwise",
          OPS + "test_linear_tile_kernels_and_the_tuned_choice_agree_at_the_prefill_shapes")
_SKINNY = (OPS + "test_linear_skinny_weight_streaming", OPS + "test_linear_skinny_fused_activation_epilogue", OPS + "test_linear_skinny_logits_epilogue")
# fp8 weights: the quantiser's images, the big-M kernels' column-scale epilogues (bits of the bf16 operator on exactly quantisable weights +
# float64 on dequant(quant(W))), the decode GEMM's c_fc / lm_head epilogues in every kernel form
_FP8_QUANT = (FP8 + "test_quantiser_images_are_torchs_cast_in_the_stated_layouts",)
_FP8_BIG_M = (FP8 + "test_big_m_kernels_apply_the_column_scale", FP8 + "test_big_m_tuned_choice_with_the_column_scale")
_FP8_DECODE = (FP8 + "test_decode_epilogues_with_fp8_weights_small_shapes", FP8 + "test_decode_epilogues_with_fp8_weights_engine_shapes")
_FOLD = (OPS + "test_decode_output_projection_and_folded_layernorm", OPS + "test_folded_layernorm_with_a_large_common_offset_per_row",
         ROWS + "test_eps_folded_layernorm_of_the_six_launch_layer")
_BEAM_STEP = (BEAM + "test_beam_scorer_matches_oracle", BEAM + "test_beam_scorer_full_vocab_penalty_and_pad_zero")
_BEAM_KV = (BEAM + "test_generate_beam_replay_through_oracle", LONG + "test_beam_search_kv_reindex_across_the_4096_boundary")
_FORK = ("test_gpu_shared_prompt.py::test_sampling_shared_equals_repeated_prompts", "test_gpu_shared_prompt.py::test_page_structure_outputs_and_streaming")
_PREPROCESS = (OPS + "test_preprocess_image_bit_exact", OPS + "test_preprocess_image_siglip_recipe_bit_exact",
               OPS + "test_preprocess_images_batched_stateless_bit_exact")
_KV_LOAD = (LONG + "test_decode_attention_needle_on_every_page", DH64 + "test_decode_attention_needle_on_every_page")

COVERAGE = {
    # ---- attention.hip
    "attn_prefill_kernel": (OPS + "test_attention_prefill", OPS + "test_attention_online_softmax_rescale_branch",
                            "test_gpu_prefill_attention.py::test_window_against_the_reference", "test_gpu_prefill_attention.py::test_ragged_form"),
    "kv_write_prefill_kernel": _KV_LOAD,                                  # sv_debug_kv_load writes the pages the attention then reads
    "rope_prefill_kernel": (DH64 + "test_teacher_forced_logits_against_the_oracle",          # (engine)
                            DH64 + "test_ragged_prompt_pass_writes_the_pages_the_rectangular_one_writes"),
    "attn_decode_kernel": (LONG + "test_decode_attention_1b_geometry_contexts", LONG + "test_decode_attention_8b_geometry_sliding_window_4096",
                           DH64 + "test_decode_attention_mqa_contexts", DH64 + "test_decode_attention_window_edge_is_exact_to_the_key"),
    "xcc_probe_kernel": "measurement tool: reports the XCD of each block (sv_debug_xcc_map), computes nothing of the path",
    "occupy_kernel": "test tool: the foreign tenant of tests/test_gpu_safety.py, pins LDS for a while and computes nothing",
    # ---- beam.hip
    "beam_row_stats_kernel": _BEAM_STEP,
    "beam_row_topk_kernel": _BEAM_STEP,
    "beam_merge_kernel": _BEAM_STEP,
    "beam_update_kernel": _BEAM_STEP + (BEAM + "test_beam_scorer_row0_stop_sequence",),
    "beam_reset_kernel": _BEAM_STEP,
    "beam_seen_gather_kernel": (BEAM + "test_beam_scorer_full_vocab_penalty_and_pad_zero",),
    "beam_row_warp_kernel": (KEPT + "test_beam_sample_forms_keep_exactly_the_reference_set", BEAM + "test_beam_sample_scorer_distribution",
                             BEAM + "test_beam_sample_warper_selection_path_at_full_vocabulary"),
    "beam_capture_kernel": (KEPT + "test_beam_sample_forms_keep_exactly_the_reference_set", "test_gpu_generate_outputs.py::test_beam_search_outputs"),
    "beam_table_reorder_kernel": _BEAM_KV,                                # (engine)
    "beam_tail_copy_kernel": _BEAM_KV,                                    # (engine)
    # ---- decode_cols.hip
    "gemm_cols_resid_kernel": _FOLD,
    "fold_prepare_kernel": _FOLD,
    # ---- engine_core.hip
    "fill_i32_kernel": _KV_LOAD,                                          # (engine) sv_debug_kv_load sets every row's position with it
    "add_i32_kernel": (LONG + "test_decode_attention_1b_geometry_walk_across_the_64_page_boundary",),      # (engine) advances the positions of a walk
    "suppress_token_kernel": ("test_gpu_minlen.py::test_min_length_holds_eos_back",),                      # (engine)
    "tokens_to_i64_kernel": (E2E + "test_generate_semantics_eos_pad_stop_on_device",),                     # (engine)
    "gen_state_init_kernel": (E2E + "test_generate_semantics_eos_pad_stop_on_device",                      # (engine)
                              E2E + "test_generate_is_deterministic_graph_equals_eager_and_batch_invariant"),
    "fill_random_bf16_kernel": "measurement tool: operands of sv_bench_linear / sv_debug_gemm_trace",
    "pack_rows_kernel": (ROWS + "test_pack_rows_and_unpack_rows_follow_the_stated_fragment_layout",),
    "unpack_rows_kernel": (ROWS + "test_pack_rows_and_unpack_rows_follow_the_stated_fragment_layout",),
    "reduce_partials_kernel": (OPS + "test_linear_skinny_weight_streaming",),                              # the slab sum behind sv_op_linear_skinny
    # ---- engine_forward.hip
    "ragged_positions_kernel": (ROWS + "test_ragged_row_pos_and_ragged_positions",),
    # ---- fork.hip
    "fork_tail_copy_kernel": _FORK,                                       # (engine)
    "fork_logits_kernel": _FORK,                                          # (engine)
    # ---- gemm_pack.hip
    "pack_weight_kernel": (OPS + "test_linear_mfma", OPS + "test_linear_transpose_detecting"),
    "convert_bf16_kernel": (E2E + "test_against_reference_goldens",),     # (engine) sv_load_weight
    "fp8_row_scale_kernel": _FP8_QUANT + ("test_gpu_fp8.py::test_fp8_skinny_gemm_matches_torch_fake_quant",),
    "pack_weight_fp8_kernel": _FP8_QUANT + ("test_gpu_fp8.py::test_fp8_skinny_gemm_matches_torch_fake_quant",),
    "cvt_bf16_hw_kernel": (OPS + "test_bf16_rounding_is_rne",),
    # ---- gemm.hip
    "gemm_bf16_kernel": _BIG_M + _FP8_BIG_M,
    "gemm256_kernel": _BIG_M + _FP8_BIG_M,
    "gemm_tail_kernel": (OPS + "test_remainder_row_kernels_agree_with_the_tile_kernels_bitwise",) + _BIG_M + _FP8_BIG_M[:1] +
                        (OPS + "test_linear_every_row_through_the_one_wave_per_tile_kernel_is_bitwise_the_tile_kernel",),
    "gemm_tailk_kernel": (OPS + "test_linear_rows_a_sequence_leaves_over_its_tiles",
                          FP8 + "test_big_m_rows_a_sequence_leaves_over_its_tiles_with_the_column_scale",
                          OPS + "test_linear_every_row_through_the_one_wave_per_tile_kernel_is_bitwise_the_tile_kernel"),
    "gemm_skinny_kernel": _SKINNY,
    "gemm_skinny_fp8_kernel": _FP8_DECODE + ("test_gpu_fp8.py::test_fp8_skinny_gemm_matches_torch_fake_quant",),
    "gemm_head_persist_kernel": (OPS + "test_lm_head_persistent_blocks_bit_identical_to_one_tile_blocks", OPS + "test_lm_head_persistent_blocks_two_row_tiles",
                                 OPS + "test_lm_head_with_folded_greedy_selection"),
    "gemm_skinny_tailsplit_kernel": (OPS + "test_linear_skinny_tail_split_gives_the_one_launch_bits",) + _SKINNY,
    "gemm_skinny_mt2_kernel": (OPS + "test_linear_skinny_two_row_tiles_per_block_is_bitwise_the_one_tile_kernel",) + _SKINNY + _FP8_DECODE,
    "gemm_skinny_mt2x_kernel": (OPS + "test_linear_skinny_two_row_tiles_per_block_is_bitwise_the_one_tile_kernel",) + _SKINNY + _FP8_DECODE,
    # ---- mlp_fused.hip
    "mlp_fused_kernel": (E2E + "test_fused_mlp_launch_equals_the_two_launches_bit_for_bit",) + _SKINNY,
    # ---- preprocess.hip
    "pp_tables_kernel": _PREPROCESS,
    "pp_horizontal_kernel": _PREPROCESS,
    "pp_vertical_kernel": _PREPROCESS,
    # ---- processors.hip
    "ban_tokens_kernel": ("test_gpu_logits_processors.py::test_ban_kernel_is_the_restatement",
                          "test_gpu_logits_processors.py::test_ban_kernel_without_any_processor_changes_nothing"),
    # ---- rowops.hip
    "layernorm_rows_kernel": (OPS + "test_layernorm_rows", ROWS + "test_layernorm_rows_packed_output", ROWS + "test_eps_layernorm_rows"),
    "row_update_ln_kernel": _ROW_UPDATE,
    "rowln_cattn_kernel": (E2E + "test_row_update_and_c_attn_as_one_launch_bit_for_bit",
                           E2E + "test_row_update_and_c_attn_as_one_launch_at_starvector_8b_widths") + _ROW_UPDATE + _SKINNY[:1],
    "im2col_kernel": (ROWS + "test_im2col_is_unfold_with_zero_padding_columns",),
    "vit_embed_lnpre_kernel": (ROWS + "test_vit_embed_lnpre", ROWS + "test_eps_vit_embed_lnpre", ROWS + "test_vit_embed_lnpre_refuses_rows_wider_than_its_registers"),
    "dec_embed_kernel": (ROWS + "test_dec_embed_adds_the_position_of_a_row_inside_its_sequence", ROWS + "test_dec_embed_ragged_rows_take_their_listed_positions"),
    "gather_rows_kernel": (ROWS + "test_gather_rows_plain_and_behind_the_visual_rows_of_a_prompt_buffer",),
    "gather_last_rows_kernel": (ROWS + "test_gather_last_rows_rectangular_and_ragged",),
    "gather_tail_rows_kernel": (ROWS + "test_gather_tail_rows",),
    "gather_listed_rows_kernel": (ROWS + "test_gather_listed_rows_unordered_repeated_from_strided_rows",),
    "ragged_row_pos_kernel": (ROWS + "test_ragged_row_pos_and_ragged_positions",),
    "plane_layernorm_kernel": (OPS + "test_plane_layernorm", ROWS + "test_plane_layernorm_into_a_strided_prompt_buffer", ROWS + "test_eps_plane_layernorm"),
    "token_batchnorm_kernel": (ROWS + "test_token_batchnorm_running_statistics_per_token", ROWS + "test_eps_token_batchnorm"),
    # ---- sampling.hip
    "argmax_kernel": (OPS + "test_argmax_lowest_index_on_ties",),
    "argmax_merge_kernel": (OPS + "test_argmax_lowest_index_on_ties",),
    "sample_top_p_kernel": (OPS + "test_top_p_sampler_distribution", BEAM + "test_sampler_top_k_then_top_p_distribution",
                            BEAM + "test_sampler_top_k_selection_at_full_vocabulary", KEPT + "test_sampler_forms_draw_exactly_the_reference_set",
                            KEPT + "test_drawn_support_captured_support_and_reference_are_one_set"),
    "capture_warp_kernel": (KEPT + "test_capture_forms_keep_exactly_the_reference_set", KEPT + "test_capture_processors_in_front_of_the_warper",
                            "test_gpu_generate_outputs.py::test_sampling_topk_topp_graph_and_eager"),
    "capture_write_kernel": (KEPT + "test_capture_forms_keep_exactly_the_reference_set", KEPT + "test_capture_processors_in_front_of_the_warper",
                             "test_gpu_generate_outputs.py::test_greedy_penalty_min_length_eos_and_stop",
                             "test_gpu_generate_outputs.py::test_sampling_topk_topp_graph_and_eager"),
    "token_stats_kernel": ("test_gpu_token_stats.py::test_tokens_unaffected_and_values_match_the_capture",  # (engine)
                           "test_gpu_token_stats.py::test_agrees_with_the_scoring_forward"),
    "token_topk_kernel": ("test_gpu_token_topk.py::test_engine_greedy_raw", "test_gpu_token_topk.py::test_engine_sampling_processed"),     # (engine)
    "token_topk_rows_kernel": ("test_gpu_token_topk.py::test_operator_fp32_random_rows", "test_gpu_token_topk.py::test_operator_designed_rows"),
    "finish_step_kernel": (E2E + "test_step_bookkeeping_inside_the_lm_head_launch_equals_the_finish_launch",                               # (engine)
                           E2E + "test_generate_semantics_eos_pad_stop_on_device"),
    "cb_step_kernel": ("test_gpu_vllm_sampling.py::test_op_greedy_processors_match_the_restatement",
                       "test_gpu_vllm_sampling.py::test_op_distribution_matches_the_restatement", "test_gpu_cb_logprobs.py::test_operator_mixed_rows",
                       KEPT + "test_every_kernel_that_draws_through_sample_row_draws_the_reference_set"),
    # ---- score.hip
    "logprob_rows_kernel": ("test_gpu_token_logprobs.py::test_logprob_rows_operator",),
    "topk_rows_bf16_kernel": ("test_gpu_token_topk.py::test_operator_bf16_rows",),
}


def kernel_names():
    """The names behind __global__ in csrc/*.hip: attributes and launch bounds skipped, template arguments never part of the name."""
    names = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        text = open(path).read()
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?([A-Za-z_]\w*)\s*(?:<[^>(]*>\s*)?\(", text):
            names.setdefault(m.group(1), os.path.basename(path))
        assert len(re.findall(r"__global__", text)) == len(re.findall(r"__global__[^;{]*?\bvoid\s", text)), path
    return names


def _test_functions(filename, cache={}):
    if filename not in cache:
        tree = ast.parse(open(os.path.join(ROOT, "tests", filename)).read())
        cache[filename] = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
    return cache[filename]


def check_table(table, names):
    """The list of what is wrong with `table` for the kernels `names` (empty: nothing)."""
    wrong = [f"{k} ({names[k]}) has no entry in COVERAGE" for k in sorted(set(names) - set(table))]
    wrong += [f"COVERAGE names {k}, which no source defines" for k in sorted(set(table) - set(names))]
    for k, v in sorted(table.items()):
        if isinstance(v, str):
            if len(v.strip()) < 10 or "\n" in v:
                wrong.append(f"{k}: the reason must be one line that says something")
            continue
        if not isinstance(v, tuple) or not v:
            wrong.append(f"{k}: an entry is a non-empty tuple of tests or a reason")
            continue
        for t in v:
            fn, _, func = t.partition("::")
            if not func or not os.path.exists(os.path.join(ROOT, "tests", fn)):
                wrong.append(f"{k}: {t!r} is not file::function under tests/")
            elif func not in _test_functions(fn):
                wrong.append(f"{k}: {fn} has no function {func}")
    return wrong


def test_every_kernel_is_accounted_for():
    names = kernel_names()
    assert len(names) >= 75, sorted(names)                       # the parse itself: 75 kernels when this table was written
    wrong = check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)


def test_the_check_notices_each_kind_of_gap():
    names = kernel_names()
    for k in COVERAGE:                                           # deleting any one entry fails
        assert check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k
    assert check_table({**COVERAGE, "gone_kernel": "a kernel that no source defines"}, names)
    assert check_table({**COVERAGE, "im2col_kernel": (ROWS + "test_that_does_not_exist",)}, names)
    assert check_table({**COVERAGE, "im2col_kernel": ("no_such_file.py::test_x",)}, names)
    assert check_table({**COVERAGE, "im2col_kernel": ()}, names)
