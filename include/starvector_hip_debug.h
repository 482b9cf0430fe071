/*
 * libstarvector_hip.so - TEST AND MEASUREMENT surface of the MI355X StarVector engine (not needed to run the path).
 *
 * Compiled into the same shared object as the product ABI (include/starvector_hip.h, included below), kept apart so that a
 * reference-side binding sees only what it has to bind:
 *   sv_op_*                 single operators, one per row of SURVEY.md section 8a: the parity tests put each HIP kernel next to the
 *                           oracle through them (tests/test_gpu_ops.py, tests/test_gpu_row_kernels.py, tests/test_gpu_fp8.py); the fp8-weight
 *                           forms (sv_op_pack_weight_fp8, sv_op_linear_fp8, sv_op_linear_skinny_epi_fp8: the quantiser's raw images, the big-M
 *                           kernels' column-scale epilogues, the decode GEMM's c_fc / lm_head epilogues) in tests/test_gpu_fp8_ops.py
 *   sv_debug_*_plan,
 *   sv_debug_resample_coeffs  host-side decisions of the library (dispatch, split-K, context splits, Pillow's tap tables), callable
 *                           WITHOUT a GPU: the CPU suite pins them
 *   sv_debug_kv_load / sv_debug_attn_decode   the decode attention alone over an engine's real paged pool (tests/test_gpu_long_context.py)
 *   sv_debug_*_trace, sv_debug_xcc_map        in-kernel wall-clock traces and block placement (tools/*_trace.py)
 *   sv_bench_*, sv_profile_decode_step        micro-benchmarks and the HIP-event profile bench.py's roofline leg reads
 *   sv_debug_set_exp / sv_debug_set_col_tiles / sv_debug_set_gemm_form / sv_debug_set_linear_seq_rows
 *                           A/B switches: they CHANGE which kernels a live engine (set_exp) or the process (the other two) launches
 *                           from then on -- every form computes the same bits (tests), but a product deployment has no reason to
 *                           call them.  The environment variable SV_EXP sets the same mask at sv_create.
 * Conventions as in starvector_hip.h.
 */
#ifndef STARVECTOR_HIP_DEBUG_H
#define STARVECTOR_HIP_DEBUG_H

#include "starvector_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-side decisions of the library, callable WITHOUT a GPU (the CPU test suite pins them):
 *   sv_debug_resample_coeffs  the fixed-point table sv_preprocess_image feeds its two passes = Pillow's
 *                             precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for BICUBIC, box (0, in_size):
 *                             bounds [out_size][2] = (first input index, tap count), taps [out_size][cap]; returns ksize
 *                             (> 0) or SV_EINVAL when cap < ksize
 *   sv_debug_gemm_plan        what the big-M GEMM dispatch does with an M x N x K problem: out5 = {peel the row remainder,
 *                             remainder rows, remainder as a 128^2 tile row (else one wave per 32x32 tile), main part on the
 *                             256^2 kernel, modelled time in us}; every choice computes the same bits */
/*   sv_debug_skinny_plan      how a decode GEMM (rows <= 64, W [N][K], split-K `splitk`, weights of format `wfmt` = SV_WEIGHT_*) is launched:
 *                             out2 = {waves per block = how K is cut inside a block, i.e. the order in which a row's partial
 *                             sums are added -- a function of the GEMM only, never of `rows`; 1 when a block carries two
 *                             32-row tiles (33..64 rows: the weights are streamed once; never with MXFP4 weights, whose kernel puts
 *                             the row tiles on grid.z); waves 0: no kernel cuts this K (fp8, MXFP4)} */
int  sv_debug_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* taps, int32_t cap);
int  sv_debug_skinny_plan(int32_t rows, int32_t N, int32_t K, int32_t splitk, int32_t wfmt, int32_t* out2);
/* The A/B switches of an engine: one bit each of the mask that the environment variable SV_EXP sets at sv_create and sv_debug_set_exp sets
 * on a live engine.  Mask 0 is the product path; every switch computes the same tokens unless its line says otherwise.
 * The values are stable: logs under profiles/ name them by number.  star-vector_amd/engine.py mirrors the enum as the IntFlag `Exp`. */
enum sv_exp_bits {
    SV_EXP_NO_LN_FOLD        = 2,        /* the 7-launch decode layer where the 6-launch one (ln_2 folded into c_fc) is the default; the fold re-rounds
                                            gamma * W, so logits move within bf16 noise (test_gpu_e2e: test_seven_launch_layer_mask_matches_the_golden) */
    SV_EXP_MLP_FUSED_FORCE   = 128,      /* c_fc + down projection as ONE launch without exclusive_device (test_fused_mlp_launch_equals_the_two_launches_bit_for_bit) */
    SV_EXP_MLP_FUSED_OFF     = 512,      /* never that launch (test_gpu_safety: test_continuous_batching_on_an_engine_that_owns_its_gpu_equals_solo_runs) */
    SV_EXP_SEPARATE_ARGMAX   = 1024,     /* greedy selection as its own launch, not in the lm_head epilogue (test_folded_greedy_selection_equals_the_argmax_launch_token_for_token) */
    SV_EXP_ROWLN_CATTN_OFF   = 8192,     /* never the row update + c_attn as one launch (test_gpu_safety, the same test as SV_EXP_MLP_FUSED_OFF) */
    SV_EXP_ROWLN_CATTN_FORCE = 16384,    /* that launch without exclusive_device (test_row_update_and_c_attn_as_one_launch_bit_for_bit) */
    SV_EXP_NO_PRUNE_LAST     = 32768,    /* the last prompt layer over all rows, not the last row of each sequence
                                            (test_prompts_of_259_rows_are_batch_independent_with_the_per_sequence_remainder) */
    SV_EXP_BATCH_REMAINDER   = 4194304,  /* big-M GEMMs peel the row remainder of the batch, not of each sequence: other kernels for those rows,
                                            so their bits may move (the same test as SV_EXP_NO_PRUNE_LAST) */
    SV_EXP_KNOWN = SV_EXP_NO_LN_FOLD | SV_EXP_MLP_FUSED_FORCE | SV_EXP_MLP_FUSED_OFF | SV_EXP_SEPARATE_ARGMAX | SV_EXP_ROWLN_CATTN_OFF |
                   SV_EXP_ROWLN_CATTN_FORCE | SV_EXP_NO_PRUNE_LAST | SV_EXP_BATCH_REMAINDER
};
/*   sv_debug_set_exp          sets that mask on a live engine (in-process A/B runs: tools/ab_exp.py).  A mask with a bit outside SV_EXP_KNOWN
 *                             is SV_EINVAL (the message names the bits) and leaves the engine as it was; sv_create fails the same way on such
 *                             an SV_EXP.  A removed switch is therefore an error, never a silent comparison of the default with itself.
 *   sv_debug_exp_known        SV_EXP_KNOWN of this build; host only, no GPU */
int  sv_debug_set_exp(sv_engine* e, int32_t mask);
int  sv_debug_exp_known(void);
int  sv_debug_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t act, int32_t* out5);
/*   sv_debug_decode_plan      what sv_create decides for a decoder Linear W [N][K] when the engine decodes `rows` (<= 64) rows at a
 *                             time on a GPU with `num_cus` CUs: out2 = {split-K factor (1 when whole_k: c_fc / lm_head keep the whole
 *                             K for their epilogue), column tiles per block of the two-row-tile kernel (1 for rows <= 32) or, for
 *                             wfmt = SV_WEIGHT_MXFP4, of the MXFP4 decode kernel (1, 2 or 4 at any row count)} -- plain
 *                             host arithmetic (engine_core.hip: pick_splitk / pick_decode_plan), pinned by the CPU tests */
int  sv_debug_decode_plan(int32_t rows, int32_t N, int32_t K, int32_t wfmt, int32_t whole_k, int32_t num_cus, int32_t* out2);
/*   sv_debug_attn_plan        the decode attention's context-split constants of an engine: out2 = {the most blocks a sequence's context
 *                             is split over (so that rows x KV heads x splits covers the CUs, <= 8), 32-key groups a block takes
 *                             before another split joins (8 where rows x KV heads alone cover the CUs, else 4)} -- functions of the
 *                             engine's max_batch / KV heads only, never of the call's batch (a row's bits do not depend on its batch) */
int  sv_debug_attn_plan(int32_t max_batch, int32_t n_kv_head, int32_t num_cus, int32_t* out2);
/*   sv_debug_rowln_plan       whether (and how) an engine that owns its GPU runs a decode layer's row update and c_attn projection as ONE
 *                             launch (rowops.hip rowln_cattn_kernel): hidden size D, the projection W [N][D] with
 *                             split-K `splitk`, `splitk_ru` slabs summed by the row update in front, a GPU with `num_cus` CUs;
 *                             out3 = {1 if the shapes fit, k-steps a GEMM wave holds in registers (4: StarVector-1B, 9: StarVector-8B), blocks of
 *                             the launch = 32 row blocks + (N / 32) * splitk} -- narrow rows (D <= 2048) need every block resident at once
 *                             (two per CU), wide rows rely on the row blocks being dispatched first.  Host arithmetic, pinned by the CPU tests */
int  sv_debug_rowln_plan(int32_t D, int32_t N, int32_t splitk, int32_t splitk_ru, int32_t num_cus, int32_t* out3);
/*   sv_debug_rowln_occupancy  blocks of that launch a CU of the current device holds at once (hipOccupancyMaxActiveBlocksPerMultiprocessor of
 *                             rowln_cattn_kernel<4, false> / <9, true> for wide != 0): sv_create turns the fused launch off below 2 / 3;
 *                             needs a GPU */
int  sv_debug_rowln_occupancy(int32_t wide, int32_t* blocks_per_cu);
/*   sv_debug_step_plan        what the LAST sv_generate call's decode step actually was, from the engine itself (bench.py's `launches_per_step`
 *                             and roofline captions; ADVICE r05: not re-derived from the configuration): out4 = {kernel nodes of the captured
 *                             decode-step graph (0: no graph, plain launches), 1 if the layers' row update + c_attn ran as one launch,
 *                             1 if the greedy selection rode in the lm_head launch, 1 if c_fc + down-projection ran as one launch} */
int  sv_debug_step_plan(sv_engine* e, int32_t* out4);
/*   sv_debug_set_col_tiles    column tiles per block (1..3; 0 = the launcher's own choice) the OP-LEVEL decode GEMM entry points
 *                             (sv_op_linear_skinny*, 33..64 rows) launch with from now on, process-wide: lets the parity tests put
 *                             every variant of the two-row-tile kernel next to the one-tile kernels (all bit-identical).  An engine's
 *                             decode loop is not affected (it carries its own plan per Linear). */
int  sv_debug_set_col_tiles(int32_t col_tiles);
/*   sv_debug_set_skinny_form  which kernel the 33..64-row decode GEMMs take from now on, process-wide (all forms are bit-identical; the choice is speed):
 *                             0 = gemm_skinny_mt2_kernel (both operands of the stream in registers, rounds 2-5), 1 = gemm_skinny_mt2x_kernel
 *                             (activations through a wave-private LDS ring, weights by hand-counted register loads; chunk depth by block
 *                             count: the default), 2 / 3 = that kernel's two-blocks-per-CU / one-block-per-CU form wherever the shape allows.
 *                             This call is the only handle on the form: it holds until the next call, across sv_create and sv_debug_set_exp
 *                             (which used to reset it from mask bits 131072 / 262144 / 524288, now removed).
 *   sv_debug_skinny_form      the form in force (0..3); host only */
int  sv_debug_set_skinny_form(int32_t form);
int  sv_debug_skinny_form(void);
/*   sv_debug_tailsplit_launches  how many times, process-wide since the library was loaded, a decode GEMM took the tail split (gemm.hip
 *                             gemm_skinny_tailsplit_kernel: StarVector-8B's c_fc at <= 32 rows); counted on the host at launch (a captured
 *                             graph counts once, at capture).  Lets a test prove which kernel ran. */
int  sv_debug_tailsplit_launches(int64_t* count);
/*   sv_debug_cols_rowhalf_launches  how many times, process-wide since the library was loaded, the decode output projection took its row-half
 *                             form (decode_cols.hip gemm_cols_resid_kernel: 16 rows x 16 columns per block; SV_COLS_ROWHALF=0 = never), and how many
 *                             row halves those launches ran (one for a step of at most 16 rows, else two); counted on the host at launch (a
 *                             captured graph counts once, at capture).  Lets a test prove which form ran. */
int  sv_debug_cols_rowhalf_launches(int64_t* launches, int64_t* halves);
/*   sv_debug_set_gemm_form    process-wide: every big-M GEMM launch takes ONE form -- 0 = 128x128 tiles, 1 = 256x256 tiles (rows not peeled),
     2 = 256x256 tiles + the row remainder over a multiple of 256 through the one-wave-per-tile tail kernel, 3 = every row through that tail
     kernel (with a sequence structure: the full 256-row tiles' rows of every sequence; the rows a sequence leaves over take the split-K
     remainder kernel as in every form); -1 = the tuned choice (default).
     The forms give the same bits; the tests compare them through this switch. */
int  sv_debug_set_gemm_form(int32_t form);
/*   sv_debug_set_linear_seq_rows  process-wide: the sequence structure sv_op_linear / sv_bench_linear hand to the big-M dispatch from now on --
     S > 0: the M rows are M / S sequences of S rows.  Where S leaves 1..3 rows over its 256-row tiles (a 259-row prompt, a 257-token image:
     starvector_base.py:131-170, clip_model.py:140-155 produce exactly those row counts) AND the dispatch's cost model peels the remainder of a
     32-sequence batch for this projection, the tile kernels cover the full tiles of EVERY sequence and gemm_tailk_kernel (8 waves per 32 x 32
     tile, K split over the waves) the rows left over -- what the engine's prompt pass and vision tower launch; S < 0: the M rows are the LAST
     rows of sequences of |S| rows (the pruned last prompt layer) and take the kernel they take inside the full problem; 0 = none (default). */
int  sv_debug_set_linear_seq_rows(int32_t seq_rows);
/*   sv_debug_gemm_seq_form    1 / 0: does the projection (N, K, act) take that per-sequence form for sequences of S rows?  Host arithmetic only
     (callable without a GPU); a function of S and the projection alone, never of the batch: a sequence's tokens do not depend on its neighbours. */
int  sv_debug_gemm_seq_form(int32_t S, int32_t N, int32_t K, int32_t act);
/*   sv_debug_ragged_plan      what the RAGGED prompt pass (sv_prefill_ragged and friends) decides for B sequences of lengths lens[0..B), packed back
     to back, at the projection (N, K, act).  Host arithmetic only.  rows_out [capacity]: the packed row indices (ascending) that go through the
     split-K remainder kernel -- the last S % 256 rows of every sequence for which sv_debug_gemm_seq_form(S, N, K, act) holds; every other row takes an
     ascending-k kernel.  last_out [capacity]: the sequences whose LAST row is such a row (the compact rows of the pruned last layer).  out4 =
     {rows listed, sequences listed, attention blocks of q_tile query rows counted from each sequence's first row, 32-token KV-write blocks}.
     capacity >= 3 * B; q_tile 32 or 128 (grouped-query heads in fours / one head per block). */
int  sv_debug_ragged_plan(const int32_t* lens, int32_t B, int32_t N, int32_t K, int32_t act, int32_t q_tile, int32_t* rows_out,
                          int32_t* last_out, int32_t capacity, int32_t* out4);
/*   sv_debug_prefix_plan      what the shared-prefix scoring pass (sv_forward_logprobs_prefixed) decides for P prefixes of lengths prefix_lens[0..P)
     and B sequences of own lengths lens[0..B) with prefix prefix_of[b], packed prefixes first, at the projection (N, K, act).  Host arithmetic
     only.  row_pos_out [packed rows]: every packed row's index in its SOLO sequence (j in a prefix, Pl + j in own rows: wpe and RoPE).  rows_out:
     the packed rows (ascending) that go through the split-K remainder kernel -- own rows only, those with solo index >= T - T % 256 where
     sv_debug_gemm_seq_form(T, N, K, act) holds for T = Pl + len; a prefix is never listed, not by its own length either.  blocks_out: the
     {sequence, query tile} pairs of the prefixed attention launch, tiles of q_tile rows counted from solo index 0, from the tile that holds row
     Pl on.  out4 = {rows listed, blocks listed, the first sequence whose remainder rows would reach into its prefix (len < T % 256 where the form
     holds: the entry point refuses the call) or -1, packed rows}.  capacity (of each of the three arrays) >= max(packed rows, 3 * B, 2 * blocks).
     SV_EINVAL for the shapes sv_forward_logprobs_prefixed refuses: P or B out of order, a length < 1, a prefix_of out of range, an unused prefix. */
int  sv_debug_prefix_plan(const int32_t* prefix_lens, int32_t P, const int32_t* lens, const int32_t* prefix_of, int32_t B, int32_t N,
                          int32_t K, int32_t act, int32_t q_tile, int32_t* row_pos_out, int32_t* rows_out, int32_t* blocks_out,
                          int32_t capacity, int32_t* out4);
/*   sv_debug_extend_plan      what an extension call (sv_prefill_extend, or a prompt pass under sv_set_prefill_chunk) decides for B sequences with
     ctx[b] cached tokens, lens[b] >= 0 new rows and total lengths totals[b] >= ctx + len (NULL: ctx + len), at the projection (N, K, act), under a
     row budget (0: one pass).  Host arithmetic only.  out [capacity] int32, *out_n = the values written (or needed, when SV_EINVAL says capacity):
       n_passes, then per pass:  n_seq, {b, ctx, len, first packed row} x n_seq        the sequences that take part, their context BEFORE the pass
                                 n_rows, packed row x n_rows                             rows through the split-K remainder kernel: the own rows with solo
                                                                                         index >= total - total % 256 where sv_debug_gemm_seq_form(total, ..) holds
                                 n_tiles, {b, tile} x n_tiles                            attention tiles of q_tile rows counted from solo index 0, from the
                                                                                         tile that holds row ctx on (context-free sequences first)
                                 n_groups, {b, 32-token group} x n_groups                page groups the writer touches: ctx / 32 .. (ctx + len - 1) / 32
                                 n_fin, b x n_fin                                        sequences that reach their total: last layer in full + logits */
int  sv_debug_extend_plan(const int32_t* ctx, const int32_t* lens, const int32_t* totals, int32_t B, int32_t budget, int32_t N, int32_t K,
                          int32_t act, int32_t q_tile, int32_t* out, int32_t capacity, int32_t* out_n);
/*   sv_debug_shared_plan      the page plan of a shared prompt pass (sv_generate_shared, sv_cb_admit_shared): n requests over n_prompts prompts of
     lengths lens[u], request i samples prompt group[i] with a budget of budgets[i] new tokens.  Host arithmetic only.  shared_out [n]: the leading
     block-table entries of request i that are its prompt's full pages, lens[group[i]] / 64, held ONCE per prompt; private_out [n]: the pages the
     request owns, ceil((len + budget) / 64) - len / 64 (the prompt's partially filled tail page included); *total_out = the pages the admit takes =
     sum over prompts of len / 64 + sum over requests of private.  SV_EINVAL for the arguments sv_cb_admit_shared rejects: a length or budget < 1,
     group[i] outside [0, n_prompts), prompts not numbered in the order their first request appears, a prompt no request references.
     sv_debug_block_table      the block-table row of a decode row / slot as the device holds it -> host_out [capacity >= pages per sequence]; returns
     the number of entries (> 0).  Needs a GPU.
     sv_debug_free_pages       pages on the host allocator's free list / pages of the pool, after the last generate call or admit / release */
int  sv_debug_shared_plan(const int32_t* lens, int32_t n_prompts, const int32_t* group, const int32_t* budgets, int32_t n,
                          int32_t* shared_out, int32_t* private_out, int64_t* total_out);
int  sv_debug_block_table(sv_engine* e, int32_t row, int32_t* host_out, int32_t capacity);
int  sv_debug_free_pages(sv_engine* e, int32_t* free_out, int32_t* total_out);
/*   sv_debug_prompt_passes    prompt passes (rectangular and ragged, continuous-batching admits included) this engine has run so far */
int  sv_debug_prompt_passes(sv_engine* e, int64_t* out);
/* The decode attention (gpt_bigcode/modeling_gpt_bigcode.py:151-285, llm/starcoder2.py:22-27 sliding window) on
 * its own, over the engine's real paged KV pool, block table and context-split plan.  Test surface: the caller chooses q / K / V.
 *   sv_debug_kv_load     dev_kv bf16 [B][S][2*n_kv*head_dim] (k heads | v heads, K as cached = after RoPE) -> pages of `layer`;
 *                        positions[b] = S for every row, or dev_lens[b] (int32 [B], <= S; NULL = S): a ragged batch
 *   sv_debug_attn_decode dev_qkv_f32 fp32 [B][n_head*head_dim + 2*n_kv*head_dim] (the new token's c_attn output, before RoPE) ->
 *                        dev_out bf16 [B][n_head*head_dim]; appends the new K/V row at positions[b]; advance != 0: positions += 1
 *   sv_debug_attn_decode_slabs  the same launch fed as a decode step feeds it: dev_slabs_f32 fp32 [splitk][B][QKV], the split-K slabs of
 *                        the c_attn GEMM (splitk 1, 2, 4 or 8), and dev_bias bf16 [QKV] (NULL = zero); the kernel sums the slabs in slab
 *                        order in fp32, then adds the bias */
/*   sv_debug_mlp_trace   (engine created with SV_MLP_TRACE=1) 100 MHz wall-clock stamps of the fused MLP launch (SV_EXP_MLP_FUSED_FORCE) of the
 *                        middle layer of the last decode step: host_out [blocks][8] = {start, c_fc loop done, tile published, slice
 *                        complete, end, XCC id, 0, 0}; returns the block count or a negative error code */
/*   sv_debug_attn_trace  (engine created with SV_ATTN_TRACE=1) the same for the decode attention launch of the middle layer: host_out
 *                        [rows * kv heads * context splits][16] = {start, first KV group requested, q in LDS, key groups processed,
 *                        partial stored + drained, ticket drawn, end (0 unless the merging block), active splits, key groups, 0...} */
int  sv_debug_attn_trace(sv_engine* e, int64_t* host_out, int32_t capacity_rows);
int  sv_debug_mlp_trace(sv_engine* e, int64_t* host_out, int32_t capacity_blocks);
/*   sv_debug_xcc_map     the XCD (XCC_ID) each block of a 1-D launch of `blocks` 8-wave blocks ran on, into host_out[blocks]; heavy = 1 gives
     the blocks the decode attention's LDS footprint and 10 us of residence (a grid above the CU count then runs in rounds, like a 64-row
     attention launch).  Evidence for the XCD-aware block -> tile mappings (block L runs on XCD (L + c) % 8): DESIGN.md sections 3c / 3f. */
int  sv_debug_xcc_map(sv_engine* e, int32_t blocks, int32_t heavy, int32_t* host_out);
/*   sv_debug_occupy_cus  a foreign tenant for the safety test of exclusive_device (tests/test_gpu_safety.py): `blocks` 4-wave blocks on a stream
     of their own, each pinning `lds_bytes` of a CU's LDS for `ms` milliseconds; returns at once.  With 144 KiB per block no block of the
     fused MLP / fused row-update launch fits beside one: those CUs are taken the way another process's kernels would take them, and a decode
     call made meanwhile has to END WITH AN ERROR (give-up code 3 / 4), never hang and never return tokens. */
int  sv_debug_occupy_cus(sv_engine* e, int32_t blocks, int32_t lds_bytes, int32_t ms);
/*   sv_debug_gemm_trace  the 256x256 big-M GEMM kernel (prefill / ViT) on random operands of the given shape, one launch with wall-clock
     stamps (form = 1): host_out [blocks * 2][8] = {start, K-tile 0 staged, K loop done, epilogue stored, tile m, tile n, wave, 0}
     (tools/gemm_trace.py).  Needs no engine.  Returns the number of blocks. */
int  sv_debug_gemm_trace(int32_t M, int32_t N, int32_t K, int32_t act, int32_t form, int64_t* host_out, int32_t capacity_blocks);
int  sv_debug_kv_load(sv_engine* e, int32_t layer, const void* dev_kv, int32_t B, int32_t S, const int32_t* dev_lens,
                      sv_stream stream);
/*   sv_debug_kv_read     tokens [first, first + count) of decode row `row` of `layer` as the attention will see them: dev_out_bf16
     [count][2*n_kv*head_dim] (k heads | v heads, the layout sv_debug_kv_load takes).  Works for both KV formats: the bf16 pool's stored bits,
     the e4m3 pool's deq(quant(.)) through the attention's own widening. */
int  sv_debug_kv_read(sv_engine* e, int32_t layer, int32_t row, int32_t first, int32_t count, void* dev_out_bf16, sv_stream stream);
/*   sv_debug_kv_gather   tokens [0, count) of decode row `row` of `layer` through the extension pass's pages -> rows launch (kv_gather_kernel, whole
     1 KiB fragment loads) -> dev_out_bf16 [count][2*n_kv*head_dim]: bit for bit what sv_debug_kv_read returns for them, either format.  Blocks. */
int  sv_debug_kv_gather(sv_engine* e, int32_t layer, int32_t row, int32_t count, void* dev_out_bf16, sv_stream stream);
/*   sv_debug_page_digests  the prefix cache's digest launch on its own (page_digest_kernel; no engine): n prompts of bf16 rows of `hidden`
     elements packed back to back in dev_embeds_packed (16-byte aligned), host_lens [n] their lengths or NULL = n x S0 rows; host_out
     [n][max_pages][2] uint64 = the digest of page k of prompt u for k < len_u / 64, zeros beyond.  Blocks.
     sv_debug_prefix_hit    host arithmetic, no device: chains the n_pages = L / 64 digests host_digests [n_pages][2] of a prompt of L rows into its
     keys (host_keys_out [n_pages][2], may be NULL) and returns in *h_out the pages an admit reuses against a table holding the n_table keys
     host_table_keys [n_table][2]: min(leading keys found, (L - 1) / 64). */
int  sv_debug_page_digests(const void* dev_embeds_packed, int32_t n, const int32_t* host_lens, int32_t S0, int32_t hidden, int32_t max_pages,
                           uint64_t* host_out, sv_stream stream);
int  sv_debug_prefix_hit(const uint64_t* host_digests, int32_t n_pages, int32_t L, const uint64_t* host_table_keys, int32_t n_table,
                         uint64_t* host_keys_out, int32_t* h_out);
int  sv_debug_attn_decode(sv_engine* e, int32_t layer, const float* dev_qkv_f32, int32_t B, void* dev_out, int32_t advance,
                          sv_stream stream);
int  sv_debug_attn_decode_slabs(sv_engine* e, int32_t layer, const float* dev_slabs_f32, int32_t splitk, const void* dev_bias, int32_t B,
                                void* dev_out, int32_t advance, sv_stream stream);
/* Prompt-lookup decoding (sv_generate_lookup), piece by piece.
 *   sv_debug_attn_decode_draft  what a verification step does around ONE attention launch, on the real paged cache: after sv_debug_kv_load of
 *                        n_seq sequences, the block table and the positions are expanded to n_seq x K1 rows (row s * K1 + j: sequence s's pages,
 *                        position pos_s + j), every row's k_new | v_new is pre-written into its page slot (lookup_kv_write_kernel) and the attention
 *                        runs over all rows; dev_slabs_f32 fp32 [splitk][n_seq * K1][QKV], dev_out bf16 [n_seq * K1][n_head*head_dim].
 *                        Afterwards the engine is back in the n_seq-row layout with every position advanced by K1 -- the state K1 calls of
 *                        sv_debug_attn_decode_slabs(..., advance = 1) leave, which must give the same bits.
 *   sv_debug_set_lookup_drafts  draft j of sequence b is host_stream[b][n_emit_b + j] (ids inside the vocabulary) instead of the lookup, for
 *                        every sv_generate_lookup call that follows with that B; NULL clears it.
 *   sv_op_lookup_accept  one lookup_step_kernel launch on given state, no engine: host_winners [n_seq * (K + 1)] = the id every row chose,
 *                        host_rows the ids the rows carried (d_0 .. d_K per sequence); in / out: host_hist [n_seq][ld] generated ids,
 *                        host_state [n_seq][4] = {n_emit, finished, prompt length, live drafts}, host_call [8] = {limit, done, n_emitted, bad,
 *                        steps, drafted, accepted, 0}, host_next_positions [n_seq * (K + 1)] the rows' positions (a finished sequence keeps its rows);
 *                        out: host_next_rows, the next step's ids.  A winner outside [0, vocab) stands for a row without a finite logit.
 *   sv_op_lookup_draft   the lookup alone on one history host_hist [L]: the drafts (at most K, and at most max_new - L - 1) and their count.
 *   sv_op_lookup_hold    the min-length hold on caller-given rows: dev_logits fp32 [rows][ld], row r belongs to sequence r / K1 with
 *                        host_n_emit [rows / K1] ids emitted; logits[r][eos] = -inf while n_emit + r % K1 < min_new.
 *   sv_op_lookup_sample  one lookup_sample_kernel launch (sv_generate_lookup_sampled's draw) on caller-given rows: dev_logits fp32 [rows][ld],
 *                        row r = s * K1 + j draws with (seed, host_n_emit[s] + j, s) -- what sv_op_sample draws for that row placed at row
 *                        index s with step = host_n_emit[s] + j.  host_seen (may be NULL) [rows][seen_words]: one bitmap per ROW, with penalty.
 *                        Out: host_tokens [rows], the id lookup_step_kernel reads from the row's slices (0x7fffffff: no finite score), and,
 *                        if not NULL, the slices themselves host_pval8 / host_pidx8 [rows][8].
 *   sv_op_lookup_seen    one lookup_seen_kernel launch on given state: host_hist [n_seq][ld] generated ids, in / out host_seq_seen
 *                        [n_seq][words] = the sequences' bitmaps over columns [0, L_before), host_L_before / host_L_after [n_seq] the columns
 *                        in front of and behind the step, host_n_draft [n_seq] and host_rows [n_seq * K1] the NEXT step's live drafts and ids.
 *                        Out: host_row_seen [n_seq * K1][words], row s * K1 + j = the sequence's set plus rows 1 .. j (dead rows: row 0's).
 *                        sv_debug_set_lookup_drafts applies to sv_generate_lookup_sampled as it does to sv_generate_lookup. */
int  sv_debug_attn_decode_draft(sv_engine* e, int32_t layer, const float* dev_slabs_f32, int32_t splitk, const void* dev_bias, int32_t n_seq,
                                int32_t K1, void* dev_out, sv_stream stream);
int  sv_debug_set_lookup_drafts(sv_engine* e, const int32_t* host_stream, int32_t B, int32_t ld);
int  sv_op_lookup_accept(const int32_t* host_winners, const int32_t* host_rows, int32_t n_seq, int32_t K, int32_t max_ngram, int32_t min_ngram,
                         int32_t* host_hist, int32_t ld, int32_t* host_state, int32_t* host_call, const int32_t* stop_ids, int32_t n_stop,
                         int32_t eos, int32_t pad, int32_t max_new, int32_t vocab, int32_t* host_next_rows, int32_t* host_next_positions,
                         sv_stream stream);
int  sv_op_lookup_draft(const int32_t* host_hist, int32_t L, int32_t K, int32_t max_ngram, int32_t min_ngram, int32_t max_new,
                        int32_t* host_drafts, int32_t* n_drafts, sv_stream stream);
int  sv_op_lookup_hold(float* dev_logits, int32_t ld, int32_t rows, int32_t K1, int32_t eos, int32_t min_new, const int32_t* host_n_emit,
                       sv_stream stream);
int  sv_op_lookup_sample(const float* dev_logits, int32_t rows, int32_t V, int32_t ld, int32_t K1, const int32_t* host_n_emit, float temperature,
                         int32_t top_k, float top_p, uint64_t seed, const uint32_t* host_seen, int32_t seen_words, float penalty,
                         int32_t* host_tokens, float* host_pval8, int32_t* host_pidx8, sv_stream stream);
int  sv_op_lookup_seen(const int32_t* host_hist, int32_t ld, int32_t n_seq, int32_t K1, int32_t words, const int32_t* host_L_before,
                       const int32_t* host_L_after, const int32_t* host_n_draft, const int32_t* host_rows, uint32_t* host_seq_seen,
                       uint32_t* host_row_seen, sv_stream stream);

/* HIP-event timing of one decode step by kernel class, on the cache state left by the last
 * sv_generate / sv_prefill (bench.py roofline leg).  out: 10 doubles, [2k] = ms per step in class k
 * (event deltas minus the empty event-pair time), [2k+1] = launches per step; k = 0 skinny
 * weight-streaming GEMM, 1 paged decode attention, 2 residual+LayerNorm row update;
 * [6] = ms between two back-to-back events with no kernel; [7] = ms per step of the step's GEMM launches
 * enqueued back to back between ONE event pair (dispatch-to-dispatch); [8] = the same for every OTHER kernel
 * of the step (no GEMMs): step - [8] = what the GEMMs cost in situ; [9] reserved. */
int  sv_profile_decode_step(sv_engine* e, int32_t B, int32_t iters, double* out10, sv_stream stream);

/* Where the time to first token goes: one pass image -> encoder -> adapter -> prompt rows -> prompt pass -> lm_head -> first greedy
 * token with a HIP event in front of every launch (group), averaged over `iters` passes after one warm-up pass.
 * dev_image bf16 [B,3,S,S] (NULL for text2svg: no encoder / adapter), dev_ids int64 [B][P].  out24: [2k] = ms per pass in stage k,
 * [2k+1] = launches (groups) per pass; k = 0 encoder GEMMs, 1 encoder attention, 2 encoder row kernels, 3 adapter GEMMs, 4 adapter
 * norm + prompt-token gather, 5 decoder prompt-pass GEMMs (tile launches), 6 remainder-row launches of peeled GEMMs (all towers),
 * 7 prompt-pass attention (+ RoPE, KV scatter), 8 prompt-pass row kernels (positions, LayerNorms, last-row gather, ln_f), 9 lm_head,
 * 10 first-token selection; [22] = the event-pair overhead subtracted from every interval (ms); [23] = first event -> last event, raw.
 * Leaves the KV cache filled like sv_prefill(B, P or T + P). */
int  sv_profile_ttft(sv_engine* e, const void* dev_image, int32_t B, const int64_t* dev_ids, int32_t P, int32_t iters,
                     double* out24, sv_stream stream);

/* ---- single operators (parity tests; all device pointers, bf16 unless noted) ------------------ */
int  sv_op_layernorm(const void* x, const void* gamma, const void* beta, void* y, int32_t M, int32_t D,
                     float eps, sv_stream stream);
/* y[M,N] = act(x[M,K] . W[N,K]^T + bias) (+ residual); W/bias/residual reference layouts */
int  sv_op_linear(const void* x, const void* W, const void* bias, const void* residual, void* y,
                  int32_t M, int32_t N, int32_t K, int32_t act, int32_t out_f32, sv_stream stream);
/* the decode-path (M<=32 per tile, weight-streaming) implementation of the same contraction */
int  sv_op_linear_skinny(const void* x, const void* W, const void* bias, void* y_f32, int32_t M, int32_t N,
                         int32_t K, int32_t splitk, sv_stream stream);
/* the same contraction with the weight quantised to fp8 e4m3 (one scale per output row, as weight_dtype = SV_WEIGHT_FP8_E4M3
 * does at load): y = x . dequant(quant(W))^T + bias, fp32; scale_out [N] (device, optional) receives the row scales */
int  sv_op_linear_skinny_fp8(const void* x, const void* W, const void* bias, void* y_f32, float* scale_out, int32_t M,
                             int32_t N, int32_t K, int32_t splitk, sv_stream stream);
/* the decode GEMM's fused epilogues on their own (split-K 1): out_f32 == 0: y[M,N] = act(bf16(x W^T + bias)) as bf16 rows
 * (the c_fc form, N %% 8 == 0); out_f32 != 0: float32 rows of x W^T holding bf16-rounded values, bias ignored (the lm_head form) */
int  sv_op_linear_skinny_epi(const void* x, const void* W, const void* bias, void* y, int32_t M, int32_t N, int32_t K,
                             int32_t act, int32_t out_f32, sv_stream stream);
/* sv_op_linear_skinny_epi with the weight quantised to fp8 e4m3 as in sv_op_linear_skinny_fp8 (the SkinnyArgs of an fp8 engine's c_fc and
 * lm_head launches); K % 64 == 0; scale_out [N] (device, optional) receives the row scales.  Honours sv_debug_set_col_tiles /
 * sv_debug_set_skinny_form like its bf16 sibling. */
int  sv_op_linear_skinny_epi_fp8(const void* x, const void* W, const void* bias, void* y, float* scale_out, int32_t M, int32_t N, int32_t K,
                                 int32_t act, int32_t out_f32, sv_stream stream);
/* sv_op_linear with the weight quantised the same way: the big-M kernels run on the bf16 image of the quantised values and apply the row
 * scales to the accumulator (GemmArgs::cscale), as an fp8 engine's prompt pass does; K % 64 == 0; scale_out [N] optional.  Honours
 * sv_debug_set_gemm_form and sv_debug_set_linear_seq_rows like sv_op_linear. */
int  sv_op_linear_fp8(const void* x, const void* W, const void* bias, const void* residual, void* y, float* scale_out, int32_t M, int32_t N,
                      int32_t K, int32_t act, int32_t out_f32, sv_stream stream);
/* the fp8 quantiser on its own, as sv_load_weight runs it: W [N][K] row-major (bf16; fp32 when w_is_f32 != 0), K % 64 == 0, Npad = N rounded
 * up to 32.  scale_out fp32 [Npad]: max_k |W[n][k]| / 448, 1 for an all-zero row and for rows >= N.  wq_out [Npad * K] bytes: the decode image
 * [Npad/32][K/32][64 lanes][16 B] -- lane l of tile nt holds row nt*32 + (l & 31), bytes 8h .. 8h+7 = k = 32*ks2 + 16*h + 8*(l >> 5) + 0..7.
 * wp_out bf16 [Npad * K]: the same values in the packed layout of the bf16 weights [Npad/32][K/16][64 lanes][8] -- lane l, k-step ks:
 * k = 16*ks + 8*(l >> 5) + 0..7.  Rows >= N are zero in both images. */
int  sv_op_pack_weight_fp8(const void* W, int32_t w_is_f32, int32_t N, int32_t K, float* scale_out, void* wq_out, void* wp_out,
                           sv_stream stream);
/* MXFP4 weights (weight_dtype = SV_WEIGHT_MXFP4, the format stated at sv_config.weight_dtype).  The quantiser on its own, as sv_load_weight runs
 * it: W [N][K] row-major (bf16; fp32 when w_is_f32 != 0), K % 64 == 0, Npad = N rounded up to 32.  scale_out uint8 [Npad][K/32]: the e8m0 bytes
 * (127 for all-zero blocks and rows >= N).  w4_out [Npad/32 * K/64 * 1088] bytes: the decode image, groups [Npad/32][K/64] of 1088 bytes --
 * bytes 0..1023 = [64 lanes][16 B], lane 32*((k/8)&1) + n%32, 32-bit word (k/16)&3 of the lane, code k%8 in nibble k%8 of the word (bits 4*(k%8)..+3:
 * sign, then the e2m1 index); bytes 1024..1087 = [32 rows][2] scale bytes, row n%32, byte (k/32)&1.  wp_out bf16 [Npad * K]: the dequantised
 * values in the packed layout of the bf16 weights. */
int  sv_op_pack_weight_mxfp4(const void* W, int32_t w_is_f32, int32_t N, int32_t K, void* scale_out, void* w4_out, void* wp_out,
                             sv_stream stream);
/* sv_op_linear_skinny with the weight quantised that way: y = x . dequant(quant(W))^T + bias, fp32, through gemm_skinny_mxfp4_kernel and fp32
 * slabs; (K/16/splitk) % 8 == 0; col_tiles = column tiles per block (1, 2, 4: identical bits; 0 = the launcher's default); scale_out uint8
 * [N][K/32] (device, optional) receives the scale bytes.  M may exceed 32: row tiles ride on grid.z. */
int  sv_op_linear_skinny_mxfp4(const void* x, const void* W, const void* bias, void* y_f32, void* scale_out, int32_t M, int32_t N, int32_t K,
                               int32_t splitk, int32_t col_tiles, sv_stream stream);
/* sv_op_linear_skinny_epi with the weight quantised that way (the SkinnyArgs of an mxfp4 engine's c_fc and lm_head launches); K % 128 == 0 */
int  sv_op_linear_skinny_epi_mxfp4(const void* x, const void* W, const void* bias, void* y, void* scale_out, int32_t M, int32_t N, int32_t K,
                                   int32_t act, int32_t out_f32, int32_t col_tiles, sv_stream stream);
/* the lm_head form with the greedy selection folded into its epilogue (what a plain greedy sv_generate runs per decode step): y_f32 [M][N]
 * (optional, device) = bf16-rounded fp32 logits, host_idx [M] (HOST) = arg-max column per row -- lowest index on ties, NaN never wins,
 * 0x7fffffff when a row has no comparable score; M <= 32 */
int  sv_op_lm_head_argmax(const void* x, const void* W, void* y_f32, int32_t* host_idx, int32_t M, int32_t N, int32_t K, sv_stream stream);
/* the two kernels of the 6-launch decode layer (csrc/decode_cols.hip; gpt_bigcode/modeling_gpt_bigcode.py:694-755) as one op, M <= 32:
 *   h2 = bf16(h + bf16(x[M,Kp] . Wp[D,Kp]^T + bp))                      attention output projection, whole K per block, in place
 *   y  = act(bf16(LayerNorm(h2; gamma, beta, eps) . Wf[F,D]^T + bf))    c_fc on the raw h2, ln_2 folded into weights / epilogue */
int  sv_op_decode_proj_fold(const void* x, const void* Wp, const void* bp, const void* h, const void* gamma, const void* beta, float eps,
                            const void* Wf, const void* bf, void* h2_out, void* y_out, int32_t M, int32_t D, int32_t Kp, int32_t F,
                            int32_t act, sv_stream stream);
/* micro-benchmark of the big-M MFMA GEMM alone (pseudo-random operands): average microseconds per launch */
int  sv_bench_linear(int32_t M, int32_t N, int32_t K, int32_t act, int32_t residual, int32_t iters, double* avg_us,
                     sv_stream stream);
/* micro-benchmark of the decode GEMM kernel alone: average microseconds per launch over `iters` back-to-back launches (HIP
 * events); mode = 0 fp32 slabs (split-K `splitk`), 1 bias + GELU -> fragment order, 2 fp32 logits (modes 1, 2: splitk == 1) */
int  sv_bench_decode_linear(int32_t M, int32_t N, int32_t K, int32_t splitk, int32_t mode, int32_t iters, double* avg_us,
                            sv_stream stream);
/* f32 -> bf16 through the hardware convert used inside the kernels (rounding-mode check) */
int  sv_op_cvt_bf16_hw(const float* x, void* y, int64_t n, sv_stream stream);
/* q,k,v token-major [B,S,H*D] / [B,S,Hkv*D]; out [B,S,H*D] */
int  sv_op_attention(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t S,
                     int32_t H, int32_t Hkv, int32_t head_dim, int32_t causal, float scale,
                     sv_stream stream);
/* The same kernel in the forms the engine's prompt pass launches: q, k, v are the column ranges [q_off, q_off + H*D), [k_off, k_off + Hkv*D),
 * [v_off, v_off + Hkv*D) of ONE bf16 token-major buffer qkv [rows][row_stride] (offsets and stride in elements, multiples of 8; MQA reads its
 * single KV head with head stride 0); out [rows][H*D].  window > 0 (causal only): query i sees keys i - window < j <= i.  host_lens == NULL:
 * B sequences of S rows, last_rows > 0 launches only the query tiles that hold the last `last_rows` rows of every sequence (the other rows of
 * `out` are not written).  host_lens != NULL (HOST array of B lengths >= 1, causal only; S ignored): the ragged form over packed rows, block
 * lists from the engine's own planner, last_rows > 0 = each sequence's last query tile alone.  Every argument is checked before any device
 * work (SV_EINVAL). */
int  sv_op_attention_prefill(const void* qkv, int32_t q_off, int32_t k_off, int32_t v_off, int32_t row_stride, void* out, int32_t B,
                             int32_t S, const int32_t* host_lens, int32_t H, int32_t Hkv, int32_t head_dim, int32_t causal,
                             float scale, int32_t window, int32_t last_rows, sv_stream stream);
/* The PREFIXED form of that kernel on its own (the shared-prefix scoring pass): the packed rows are P prefixes of host_prefix_lens[u] rows
 * followed by the own rows of B sequences (host_lens[b] >= 1, prefix host_prefix_of[b]); sequence b attends as the solo sequence
 * concat(prefix, own rows).  Causal, block list from the engine's own planner (the tiles from the one that holds row Pl on).  Only the OWN rows of
 * `out` [packed rows][H*D] are written: the prefix rows belong to the prefixes' ordinary ragged launch, which this operator does not make.
 * Every argument is checked before any device work (SV_EINVAL). */
int  sv_op_attn_prefill_prefixed(const void* qkv, int32_t q_off, int32_t k_off, int32_t v_off, int32_t row_stride, void* out, int32_t P,
                                 const int32_t* host_prefix_lens, int32_t B, const int32_t* host_lens, const int32_t* host_prefix_of,
                                 int32_t H, int32_t Hkv, int32_t head_dim, float scale, int32_t window, sv_stream stream);
int  sv_op_plane_layernorm(const void* x, const void* gamma, const void* beta, void* y, int32_t B,
                           int32_t QD, float eps, sv_stream stream);
/* the same kernel writing plane b at y + b * y_batch_stride (elements, a multiple of 8, >= QD): the form the engine launches, straight
 * into a [B][S0][D] prompt buffer.  Nothing between the planes is written. */
int  sv_op_plane_layernorm_strided(const void* x, const void* gamma, const void* beta, void* y, int32_t B, int32_t QD, float eps,
                                   int64_t y_batch_stride, sv_stream stream);
/* ---- the row kernels that assemble the prompt and carry the decode residual stream, each on its own (tests/test_gpu_row_kernels.py).
 * Device pointers, bf16 unless noted.  Shapes a kernel cannot do are SV_EINVAL; the sizes of the caller's buffers cannot be checked here:
 * each line says what the call reads and writes.
 *   sv_op_im2col            img [B][3][S][S] -> out [B * (S/P)^2][Kpad], column k = c*P*P + ky*P + kx, columns 3*P*P .. Kpad-1 zero (Kpad % 8 == 0)
 *   sv_op_vit_embed_lnpre   CLIP token assembly + ln_pre: x [B][NP+1][Dv] = LN(bf16(cat(cls [Dv], patch_out [B*NP][ldp]) + pos [NP+1][Dv])); Dv % 8 == 0, Dv <= 2048
 *   sv_op_dec_embed         h [B*S0][D] = bf16(emb + table[t]), t = row % S0, or dev_row_pos[row] (int32 [B*S0]) when given
 *   sv_op_gather_rows       out row r = table[dev_ids[r]] (int64 [n]); per_seq > 0: row r goes to out + (r / per_seq) * seq_stride + (r % per_seq) * D
 *   sv_op_gather_last_rows  out [B][D] = row b*S0 + S0-1 of h, or row first + len - 1 with descriptors dev_rag_seq int32 [B][2] = {first packed row, length}
 *   sv_op_gather_tail_rows  out [B*n_keep][D] = the last n_keep rows of each of the B sequences of S0 rows of h
 *   sv_op_gather_tail_rows_ragged  the same kernel over packed sequences of different lengths, each keeping its own number of rows: descriptors
 *                           dev_rag_keep int32 [B][4] = {first packed row, length, keep, first output row} with keep in 1..length and first output
 *                           row = the sum of the keeps in front; out [total_keep][D], total_keep = sum(keep): rows first + length - keep ..
 *                           first + length - 1 of sequence b go to output rows first output row ..
 *   sv_op_gather_listed_rows  out [n][D] = x[dev_rows[i]] (int32 [n]), x rows ldx elements apart
 *   sv_op_ragged_row_pos    dev_row_pos[first + j] = j for j < len, for each of the B descriptors {first packed row, length}
 *   sv_op_ragged_positions  dev_positions[i] = length of descriptor i / rep, + delta, for i < B * rep
 *   sv_op_token_batchnorm   nn.BatchNorm1d(Q) in eval over x [B][Q][D] (w, b, running_mean, running_var: [Q]); batch b at y + b * y_batch_stride
 *   sv_op_layernorm_packed  sv_op_layernorm with y in fragment order ("xp", csrc/common.h): ceil(M/32) tiles of 32 x D, rows >= M not written; D % 16 == 0
 *   sv_op_pack_rows / sv_op_unpack_rows   row-major [M][ldx] <-> fragment order, K % 16 == 0
 *   sv_op_row_update_ln     the decode row update (csrc/kernels.h RowUpdateArgs, field for field).  ws == NULL: h = bf16(wte[tok] + wpe[pos]) (wpe NULL:
 *                           wte[tok]); else h = bf16(h + bf16(sum over the splitk slabs ws [splitk][rows_ws][ldws] fp32, in slab order, + bias)).  h is row-major
 *                           [M][ldh] or, ldh == 0, fragment order; xp_out = LN(h) in fragment order.  D % 16 == 0; 256 threads per row up to D = 2048,
 *                           1024 above */
int  sv_op_im2col(const void* img, void* out, int32_t B, int32_t img_size, int32_t patch, int32_t Kpad, sv_stream stream);
int  sv_op_vit_embed_lnpre(const void* patch_out, int32_t ldp, const void* cls, const void* pos, const void* gamma, const void* beta,
                           void* x, int32_t B, int32_t NP, int32_t Dv, float eps, sv_stream stream);
int  sv_op_dec_embed(const void* emb, const void* table, void* h, int32_t B, int32_t S0, int32_t D, const int32_t* dev_row_pos,
                     sv_stream stream);
int  sv_op_gather_rows(const void* table, const int64_t* dev_ids, void* out, int32_t n, int32_t D, int32_t per_seq, int64_t seq_stride,
                       sv_stream stream);
int  sv_op_gather_last_rows(const void* h, void* out, int32_t B, int32_t S0, int32_t D, const int32_t* dev_rag_seq, sv_stream stream);
int  sv_op_gather_tail_rows(const void* h, void* out, int32_t B, int32_t S0, int32_t n_keep, int32_t D, sv_stream stream);
int  sv_op_gather_tail_rows_ragged(const void* h, void* out, int32_t B, int32_t D, const int32_t* dev_rag_keep, int32_t total_keep,
                                   sv_stream stream);
int  sv_op_gather_listed_rows(const void* x, int32_t ldx, const int32_t* dev_rows, int32_t n, void* out, int32_t D, sv_stream stream);
int  sv_op_ragged_row_pos(const int32_t* dev_rag_seq, int32_t B, int32_t* dev_row_pos, sv_stream stream);
int  sv_op_ragged_positions(int32_t* dev_positions, const int32_t* dev_rag_seq, int32_t B, int32_t rep, int32_t delta, sv_stream stream);
int  sv_op_token_batchnorm(const void* x, const void* w, const void* b, const void* running_mean, const void* running_var, void* y,
                           int32_t B, int32_t Q, int32_t D, float eps, int64_t y_batch_stride, sv_stream stream);
int  sv_op_layernorm_packed(const void* x, const void* gamma, const void* beta, void* y_xp, int32_t M, int32_t D, float eps,
                            sv_stream stream);
int  sv_op_pack_rows(const void* x, int32_t ldx, void* xp, int32_t M, int32_t K, sv_stream stream);
int  sv_op_unpack_rows(const void* xp, void* x, int32_t ldx, int32_t M, int32_t K, sv_stream stream);
int  sv_op_row_update_ln(const float* ws, int32_t splitk, int32_t ldws, int32_t rows_ws, const void* bias, void* h, int32_t ldh,
                         const void* wte, const void* wpe, const int32_t* dev_tokens, const int32_t* dev_positions, const void* gamma,
                         const void* beta, float eps, void* xp_out, int32_t M, int32_t D, sv_stream stream);
int  sv_op_argmax(const float* logits, int32_t B, int32_t V, int32_t ld, int32_t* out, sv_stream stream);
int  sv_op_sample_top_p(const float* logits, int32_t B, int32_t V, int32_t ld, float temperature,
                        float top_p, uint64_t seed, int32_t step, int32_t* out, sv_stream stream);
/* the continuous-batching selection (cb_step_kernel, the same device code) on caller-given rows: row b of dev_logits [B][ld]
 * (ld a multiple of 4; not modified: the kernel works on a copy) is request reqs[b] after host_hist_len[b] output tokens
 * host_history[b][0 .. host_hist_len[b]) (row stride ld_hist): that is its step (random stream, min_new_tokens hold), its output
 * counts and, with the prompt ids, its repetition set.  host_out [B] = the token each row takes. */
int  sv_op_cb_select(const float* dev_logits, int32_t B, int32_t V, int32_t ld, const sv_cb_request* reqs,
                     const int32_t* host_history, int32_t ld_hist, const int32_t* host_hist_len, int32_t* host_out, sv_stream stream);
/* sv_op_cb_select plus one sv_cb_logprobs per row (the recording form of cb_step_kernel: the device code behind sv_cb_admit_logprobs): row b
 * records what lps[b] asks.  Host outputs: host_out [B] tokens (those of sv_op_cb_select on the same rows), host_logprob / host_rank [B],
 * host_ids / host_lps [B][ld_k] with ld_k >= every enabled row's k -- row b's first k entries are its list, the rest (-1, -inf); a row with
 * enable = 0 reads log-prob NaN, rank 0 and an empty list. */
int  sv_op_cb_logprobs(const float* dev_logits, int32_t B, int32_t V, int32_t ld, const sv_cb_request* reqs, const sv_cb_logprobs* lps,
                       const int32_t* host_history, int32_t ld_hist, const int32_t* host_hist_len, int32_t* host_out, float* host_logprob,
                       int32_t* host_rank, int32_t* host_ids, float* host_lps, int32_t ld_k, sv_stream stream);
/* Drafting in the continuous batch (sv_cb_set_lookup), test surface.
 *   sv_debug_cb_set_lookup_drafts  draft j of slot s < n is host_ids[s][step_s + j] (row stride ld, ids inside the vocabulary; nothing beyond
 *                                  column ld) instead of the lookup; slots >= n draft by the lookup.  host_ids NULL: cleared.  Set before the
 *                                  admit, while no continuous batch is active (SV_ESTATE otherwise); the kept step graphs are dropped.
 *   sv_op_cb_lookup_step           ONE launch of cb_lookup_step_kernel (cb_lookup/cb_lookup.hip, the same device code) over n slots of K + 1
 *                                  rows each on caller-given state.  dev_logits [n * (K + 1)][ld] fp32 (ld a multiple of 4; not modified: the
 *                                  kernel works on a copy), row s * (K + 1) + j is slot s's row j.  Slot s is request reqs[s] with prompt
 *                                  length host_base[s], live flag host_live[s] and host_hist_len[s] emitted ids host_history[s][0 ..) (row
 *                                  stride ld_hist, which must leave room for K + 1 more): its step, counts and repetition set.  host_rows /
 *                                  host_positions [n * (K + 1)] and host_n_draft [n] are the step in flight (lk_write_rows' layout).
 *                                  host_forced (may be NULL) [forced_n][forced_ld] as sv_debug_cb_set_lookup_drafts.  All host arrays but
 *                                  reqs / host_base / host_forced are updated in place; host_counts [n][3] = each slot's {steps, drafted,
 *                                  accepted} of this launch, host_flags3 = {finished slots, 0, bad}.
 *                                  lps (may be NULL) [n]: what each slot records; host_logprob / host_rank [n][K + 1] then receive the record
 *                                  of the columns this launch emitted (NaN / 0 behind them), lists are not returned. */
int  sv_debug_cb_set_lookup_drafts(sv_engine* e, const int32_t* host_ids, int32_t n, int32_t ld);
int  sv_op_cb_lookup_step(const float* dev_logits, int32_t n, int32_t K, int32_t V, int32_t ld, const sv_cb_request* reqs,
                          const sv_cb_logprobs* lps, const int32_t* host_base, int32_t* host_live, int32_t* host_history, int32_t ld_hist,
                          int32_t* host_hist_len, int32_t* host_rows, int32_t* host_positions, int32_t* host_n_draft, int32_t max_ngram,
                          int32_t min_ngram, const int32_t* host_forced, int32_t forced_n, int32_t forced_ld, int32_t* host_counts,
                          int32_t* host_flags3, float* host_logprob, int32_t* host_rank, sv_stream stream);
/* the kernel of sv_generate_processed's token bans (processors.hip ban_tokens_kernel) on caller-given rows: row b of dev_logits [B][ld] fp32
 * (device, V valid columns) is a row whose generated ids so far are host_hist[b][0 .. host_hist_len[b]) (HOST, row stride ld_hist, ids inside
 * the vocabulary).  The ids lp->no_repeat_ngram_size and lp's bad words ban at that point are set to -inf IN PLACE; every other value is left
 * as it is.  lp->min_p is ignored (it is no ban).  The limits of sv_logits_processors apply (SV_EINVAL before any device work). */
int  sv_op_ban_tokens(float* dev_logits, int32_t B, int32_t V, int32_t ld, const int32_t* host_hist, int32_t ld_hist,
                      const int32_t* host_hist_len, const sv_logits_processors* lp, sv_stream stream);
/* the kernel of sv_forward_logprobs (score.hip logprob_rows_kernel) on caller-given rows: dev_logits_bf16 [R][ld] bf16 (16-byte aligned,
 * ld a multiple of 8), V valid columns, dev_targets int32 [R] (-100 = ignore: logprob 0).  fp32 over x_i = float(logit_i) / temperature:
 * logsumexp, logprob = x_target - logsumexp, entropy of softmax(x) (an x_i = -inf adds 0), argmax = the lowest index holding the maximum.
 * Outputs are device arrays [R]; each may be NULL.  host_flag2 (optional, HOST int32[2]): [0] = 1 if a target was outside [0, V) and not
 * -100 (its logprob is NaN) | 2 if a row had no finite logit (its outputs are NaN, argmax -1), [1] = the first such row, -1 if none. */
int  sv_op_logprob_rows(const void* dev_logits_bf16, int32_t R, int32_t V, int32_t ld, const int32_t* dev_targets, float temperature,
                        float* dev_logprob, float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t* host_flag2,
                        sv_stream stream);
/* the kernel of sv_forward_topk (score.hip topk_rows_bf16_kernel) on the same rows: dev_logsumexp [R] is what sv_op_logprob_rows returned for
 * them at the same temperature.  dev_topk_ids int32 / dev_topk_logprobs fp32 [R][k], 1 <= k <= SV_TOPK_MAX; dev_rank int32 [R] or NULL: the
 * rank of dev_targets[r] (dev_targets NULL or -100: 0). */
int  sv_op_topk_rows_bf16(const void* dev_logits_bf16, int32_t R, int32_t V, int32_t ld, const int32_t* dev_targets, float temperature,
                          const float* dev_logsumexp, int32_t k, int32_t* dev_topk_ids, float* dev_topk_logprobs, int32_t* dev_rank,
                          sv_stream stream);
/* sv_generate_topk's source 0 on caller-given rows (sampling.hip token_topk_rows_kernel, the row function of the decode step): dev_logits
 * [B][ld] fp32, V valid columns, one token per row (dev_tokens int32 [B]; NULL or an entry < 0: no rank, 0 is written).  Outputs: dev_ids int32 /
 * dev_logprobs fp32 [B][k] = the k best ids of log_softmax(row / temperature) and their log-probs, dev_rank int32 [B] or NULL. */
int  sv_op_token_topk(const float* dev_logits, int32_t B, int32_t V, int32_t ld, float temperature, const int32_t* dev_tokens, int32_t k,
                      int32_t* dev_ids, float* dev_logprobs, int32_t* dev_rank, sv_stream stream);
/*   sv_debug_set_score_chunk_rows  sv_forward_logprobs runs its lm_head over `rows` rows at a time from the next call on (a multiple of 256;
     0 = the default, 4096): lets a test force many chunks on a tiny model.  The outputs do not depend on it, bit for bit. */
int  sv_debug_set_score_chunk_rows(sv_engine* e, int32_t rows);
/* temperature -> top-k (0 = off) -> top-p -> one multinomial draw per row */
int  sv_op_sample(const float* logits, int32_t B, int32_t V, int32_t ld, float temperature, int32_t top_k,
                  float top_p, uint64_t seed, int32_t step, int32_t* out, sv_stream stream);
/* The per-step output launch of sv_generate_ex (sampling.hip launch_capture_rows: capture_warp_kernel + capture_write_kernel) on caller-given
 * rows, as step 0 of a one-step call: dev_rows fp32 [B][ld], V valid columns.  dev_seen (may be NULL) uint32 [B][seen_words] with `penalty`:
 * the repetition set of each row; hold_eos != 0: the min-length hold, eos_token_id at -inf.  do_sample != 0: temperature -> top_k (<= 0: off)
 * -> top_p -> min_p (0: off) with min_tokens_to_keep 1.  Outputs, each [B][ld_out] fp32 and optional (at least one): dev_logits_out = the raw
 * row, dev_scores_out = the processed row as HF reports it -- kept ids s / temperature, the rest -inf.  Columns >= V and rows >= B are not
 * written.  Every argument is checked before any device work (SV_EINVAL). */
int  sv_op_capture_rows(const float* dev_rows, int32_t B, int32_t V, int32_t ld, const uint32_t* dev_seen, int32_t seen_words, float penalty,
                        int32_t eos_token_id, int32_t hold_eos, int32_t do_sample, float temperature, int32_t top_k, float top_p, float min_p,
                        float* dev_scores_out, float* dev_logits_out, int64_t ld_out, sv_stream stream);
/* The sv_beam_step calls that follow also launch beam_capture_kernel (beam.hip) into the caller's slabs, through the BeamScorer::cap / cap_temp
 * sv_generate_ex sets: dev_scores / dev_logits fp32 [max_new][batch * num_beams][ld] (each optional), step t writes slab t -- the raw rows and
 * the processed log-probs the scorer ranks (beam-sample: kept ids lp / temperature with min_tokens_to_keep 2, the rest -inf).  Both NULL:
 * cleared.  ld >= vocab and 1 <= max_new <= the scorer's (SV_EINVAL); steps >= max_new write nothing.  The slabs must outlive the steps. */
int  sv_debug_beam_set_capture(sv_beam* b, float* dev_scores, float* dev_logits, int64_t ld, int32_t max_new);

#ifdef __cplusplus
}
#endif
#endif /* STARVECTOR_HIP_DEBUG_H */
