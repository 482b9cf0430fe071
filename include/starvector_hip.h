/*
 * libstarvector_hip.so - C ABI of the MI355X (gfx950) StarVector im2svg inference engine.
 *
 * Drop-in boundary for the hot path of joanrod/star-vector (paths below are relative to the
 * reference checkout):
 *
 *   sv_encode_image        replaces  ImageEncoder.forward, clip branch
 *                                    starvector/model/image_encoder/image_encoder.py:91-94
 *                                    (VisionTransformer.forward, .../clip_model.py:181-191)
 *   sv_adapter             replaces  Adapter.forward  starvector/model/adapters/adapter.py:33-39
 *   sv_embed_tokens        replaces  StarVectorStarCoder._get_embeddings (wte lookup)
 *                                    starvector/model/models/starvector_v1.py:16-18
 *   sv_prefill / sv_decode_step
 *                          replace   GPTBigCodeForCausalLM.forward as called by HF generate
 *                                    (restated in starvector/model/gpt_bigcode/modeling_gpt_bigcode.py:930-1134,1241-1258)
 *   sv_generate            replaces  svg_transformer.transformer.generate(**generation_kwargs)
 *                                    starvector/model/models/starvector_base.py:228-241,255
 *                                    incl. StoppingCriteriaSub (starvector_base.py:9-20)
 *   sv_generate_processed  the same call with the HF generate arguments the reference's callers add for a decoder that loops or emits
 *                                    a forbidden token: no_repeat_ngram_size, bad_words_ids, min_p (sv_logits_processors below)
 *   sv_generate_stats      the same call, also returning each generated token's log-prob, processed log-prob and entropy (what a GRPO
 *                                    trainer otherwise gets from a second pass over prompt + completion; sv_token_stats below)
 *   sv_generate_topk       the same call, also returning the k most likely ids of every step, their log-probs and the emitted token's rank
 *                                    (sv_token_topk below); sv_forward_topk does the same for the scoring pass
 *   sv_load_weight         ingests the reference state_dict keys (train/util.py:71 naming;
 *                          SURVEY.md section 8b "Weight names")
 *
 * This header is the PRODUCT ABI: what a reference-side binding needs -- engine life cycle, weights,
 * the forward entry points, generate, continuous batching, the beam scorer, image pre-processing.  The test / measurement surface
 * (sv_op_* single operators, sv_debug_* plans and traces, sv_bench_*, sv_profile_*) is compiled into the same library but declared
 * in include/starvector_hip_debug.h: nothing there is needed to run the path, and three of its switches change which kernels a live
 * engine launches (A/B measurements only).
 *
 * Conventions: every pointer named dev_* / documented "device" is a HIP device pointer owned by the
 * caller (PyTorch-ROCm tensor.data_ptr()); `stream` is a hipStream_t passed as void* (0 = default
 * stream); all work is enqueued on it.  Functions return 0 on success or a negative SV_E* code;
 * sv_last_error() returns the message of the calling thread's last failure.  One in-flight call
 * per engine handle (internal mutex); handles are independent.  bf16 = IEEE bfloat16 bits.
 */
#ifndef STARVECTOR_HIP_H
#define STARVECTOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_ABI_VERSION 9
#define SV_WEIGHT_BF16 0
#define SV_WEIGHT_FP8_E4M3 1
#define SV_WEIGHT_MXFP4 2

enum {
    SV_OK = 0,
    SV_EINVAL = -22,      /* bad argument / shape */
    SV_ENOMEM = -12,      /* device allocation failed */
    SV_ENOENT = -2,       /* unknown weight name / missing weight */
    SV_EHIP = -5,         /* HIP runtime error */
    SV_ESTATE = -1,       /* call order (e.g. generate before weights are complete) */
    SV_ENOTSUP = -95,     /* a combination the engine does not implement (says which) */
    SV_EBUSY = -16        /* continuous batching: no free slot / KV pages for the request right now (release finished slots, retry) */
};

enum { SV_DTYPE_BF16 = 0, SV_DTYPE_F32 = 1 };
enum { SV_ARCH_V1 = 0, SV_ARCH_V2 = 1 };
enum { SV_NORM_LAYER = 0, SV_NORM_BATCH = 1 };          /* adapter_norm (adapter.py:25-28) */
enum { SV_ACT_NONE = 0, SV_ACT_QUICKGELU = 1, SV_ACT_SWISH = 2, SV_ACT_GELU_TANH = 3 };

typedef struct sv_engine sv_engine;
typedef void* sv_stream;

/* Shapes of StarVector-1B unless overridden (StarVectorConfig, starvector_arch.py:96-131) */
typedef struct sv_config {
    int32_t image_size;        /* 224 */
    int32_t patch_size;        /* 14  */
    int32_t vit_width;         /* 1024 */
    int32_t vit_layers;        /* 23 (image_encoder.py:52-58) */
    int32_t vit_heads;         /* 16 */
    int32_t adapter_norm;      /* SV_NORM_LAYER */
    int32_t hidden;            /* 2048 */
    int32_t n_layer;           /* 24 */
    int32_t n_head;            /* 16 */
    int32_t n_inner;           /* 8192 */
    int32_t vocab;             /* 49156 */
    int32_t n_positions;       /* 8192 */
    int32_t max_batch;         /* sequences per generate call (KV pool + workspace sizing) */
    int32_t max_seq_len;       /* prompt + generated tokens per sequence (<= n_positions) */
    float   ln_eps;            /* 1e-5 */
    int32_t device;            /* HIP device ordinal */
    /* StarVector-8B; sv_config_default_1b() zeroes / defaults them */
    int32_t arch;              /* SV_ARCH_V1: CLIP + GPTBigCode (MQA, learned positions)
                                  SV_ARCH_V2: SigLIP tower + StarCoder2 (RoPE, GQA)   */
    int32_t n_kv_head;         /* v2: key/value heads (v1: 1) */
    float   rope_theta;        /* v2: rotary base (1e6 for bigcode/starcoder2-7b) */
    int32_t vit_mlp;           /* v2: SigLIP intermediate size (v1: 4 * vit_width) */
    float   vit_eps;           /* v2: SigLIP layer_norm_eps 1e-6 (v1: ln_eps) */
    int32_t sliding_window;    /* v2: a query sees the last `sliding_window` keys, itself included (4096 for
                                  bigcode/starcoder2-7b; HF's eager/sdpa mask `kv > q - W`); 0 = full attention.
                                  The prompt must fit inside the window. */
    int32_t weight_dtype;      /* SV_WEIGHT_BF16 (reference precision) or SV_WEIGHT_FP8_E4M3: decoder Linear weights and the
                                  lm_head are quantised at load to OCP e4m3 with one scale per output row (BASELINE config 5,
                                  "fp8 weights"): the decode step streams half the bytes; activations, accumulation and every
                                  other tensor stay as they are.  Not a reference numerics mode: see DESIGN.md.
                                  SV_WEIGHT_MXFP4: the same tensors quantised at load to OCP MXFP4 -- per output row, blocks of 32
                                  consecutive k (K zero-padded), one e8m0 scale byte E + 127 per block with E = floor(log2(amax)) - 2
                                  clamped to [-125, 125] (E = 0, codes 0 for an all-zero block), e2m1 codes = W / 2^E rounded to
                                  {0, .5, 1, 1.5, 2, 3, 4, 6} with its sign, ties to the even mantissa bit, magnitudes above 6
                                  saturating; amax is taken from the tensor as handed (fp32 sources are not rounded to bf16 first).
                                  The decode step streams 4.25 bits per weight.  Every dequantised weight is exactly a bf16 number:
                                  the engine computes what a bf16 engine computes over dequant(quant(W)), except for the K-summation
                                  order of the decode GEMMs.  Every decoder K must be a multiple of 128 (else sv_create: SV_ENOTSUP,
                                  naming the Linear).  Embedding lookups keep the bf16 table.  Not a reference numerics mode. */
    int32_t exclusive_device;  /* != 0: this engine is the only thing launching kernels on its GPU while it decodes (the deployment the
                                  path is built for: one process per GPU).  Enables the decode launches that need ALL their
                                  workgroups resident at once (mlp_fused_kernel: the MLP half of a layer as one launch, 256 blocks, one
                                  per CU, in-launch hand-off; rowln_cattn_kernel: the row update and the c_attn projection as one
                                  launch).  Results are bit-identical either way.  With ANOTHER process or engine decoding on the same
                                  GPU such a launch can find its blocks only partly resident: the waiting blocks then give up after
                                  a wall-clock bound (5 ms) and the call -- sv_generate, beam search, sv_decode_step, sv_cb_step --
                                  fails with SV_EHIP and a message naming the launch (never a hang, never tokens; executed by
                                  tests/test_gpu_safety.py); the next call starts clean.  Leave it 0 there.  Default 0.
                                  2 = OPTIMISTIC: as 1 until a fused launch gives up for the first time; the engine then switches those launches
                                  off for the rest of its life (one line on stderr) and sv_generate runs the failed call again without them -- the
                                  kernels are bit-identical either way, so the caller sees the same tokens, late by the failed attempt (<= 80 ms
                                  in the safety test), and a streaming callback gets every column exactly once; sv_decode_step / sv_cb_step report
                                  that one failure and are clean from the next call on.  What the Python wrapper passes by default. */
} sv_config;

/* Streaming: called on the host with the tokens that became final since the last call -- tokens [batch][n_cols] int32
 * row-major, covering output columns first_col .. first_col + n_cols - 1 -- every `sync_every` steps and once at the end
 * (what a HF `streamer` gets through put(); the reference's serve worker builds one, serve/model_worker.py:129,170, but its
 * kwargs whitelist never lets it reach generate). */
typedef void (*sv_token_callback)(void* user, const int32_t* tokens, int32_t batch, int32_t first_col, int32_t n_cols);

/* generate(...) arguments that reach HF generate through starvector_base.py:228-241 */
typedef struct sv_sampling {
    int32_t do_sample;         /* 0 = greedy argmax */
    float   temperature;       /* used when do_sample */
    float   top_p;             /* used when do_sample */
    int32_t max_length;        /* HF semantics: INCLUDES the prompt rows (budget = max_length - S0) */
    int32_t eos_token_id;
    int32_t pad_token_id;
    int32_t n_stop;            /* length of the row-0 stop sequence ("</svg>" ids), 0 = none */
    const int32_t* stop_ids;   /* host pointer, n_stop entries */
    uint64_t seed;             /* sampling RNG seed */
    int32_t sync_every;        /* host polls the device "done" flag every this many steps (0 = 32) */
    float   repetition_penalty;/* HF RepetitionPenaltyLogitsProcessor over the generated ids; 0 or 1 = off */
    int32_t num_beams;         /* 0 or 1 = greedy / sampling; 2..8 = HF beam search (the reference's default is 2,
                                  starvector_base.py:234); batch * num_beams <= max_batch; with do_sample: beam-sample */
    float   length_penalty;    /* beam search: hypothesis score = sum log-probs / len ** length_penalty (:238) */
    int32_t early_stopping;    /* beam search: 0 False (HF default), 1 True (:293), 2 "never" */
    int32_t top_k;             /* used when do_sample: HF TopKLogitsWarper before top-p; 0 = off.  The reference never
                                  passes it, but its pinned transformers==4.49.0 defaults GenerationConfig.top_k to 50 */
    sv_token_callback on_tokens; /* optional streaming callback (NULL = off); not with num_beams > 1 (as in HF) */
    void*   user_data;
    int32_t min_new_tokens;    /* HF MinLengthLogitsProcessor: the EOS logit is held at -inf while fewer than this many tokens
                                  have been generated.  The caller passes max(min_length - S0, 0) (HF subtracts the prompt
                                  length when generating from inputs_embeds; starvector_base.py:236 passes min_length).
                                  0 = off.  With num_beams > 1 HF applies it to the log-probabilities: so does the scorer */
} sv_sampling;

/* HF beam search bookkeeping as a standalone device-side scorer (what transformers' _beam_search does between two
 * forward passes): feed it the [batch * num_beams][vocab] fp32 logits of each step.  sv_generate drives the same
 * object internally; this handle exists so the parity tests can check it against the oracle on synthetic logits. */
typedef struct sv_beam sv_beam;
typedef struct sv_beam_config {
    int32_t batch, num_beams, vocab, max_new;
    int32_t eos_token_id, pad_token_id;
    int32_t early_stopping;    /* 0 False, 1 True, 2 "never" */
    float   length_penalty;
    float   repetition_penalty;
    int32_t n_stop;            /* the reference's row-0 stop sequence (starvector_base.py:9-20) */
    const int32_t* stop_ids;   /* host pointer */
    int32_t do_sample;         /* beam-sample: warpers (temperature, top_k, top_p; min_tokens_to_keep 2) on the log-probs,
                                  then 2*num_beams draws without replacement from softmax(accumulated scores) */
    float   temperature, top_p;
    int32_t top_k;
    uint64_t seed;
    int32_t min_new_tokens;    /* HF MinLengthLogitsProcessor on the log-probabilities (as _beam_search applies processors) */
} sv_beam_config;

int  sv_abi_version(void);
const char* sv_last_error(void);
void sv_config_default_1b(sv_config* cfg);
void sv_config_default_8b(sv_config* cfg);    /* siglip_384 + starcoder2-7b shapes, max_batch 16 */

int  sv_create(const sv_config* cfg, sv_engine** out);
int  sv_destroy(sv_engine* e);

/* The KV-cache format, chosen at engine creation (entry points appended; SV_ABI_VERSION and sv_config are unchanged).  sv_create is
 * sv_create_kv with SV_KV_BF16.
 *
 * SV_KV_FP8_E4M3.  For every (token, KV head), K (after RoPE) and V are quantised separately to one scale byte and head_dim one-byte
 * OCP e4m3 codes.  The rule:
 *   - amax is taken over the finite ones of the head_dim bf16 values the bf16 cache would have stored;
 *   - E = floor(log2(amax)) - 7, clamped to [-120, 120]; the scale byte is E + 127.  The scaled maximum then lies in [128, 256): no code
 *     saturates (the clamp at 120 can let an element above 248 * 2^120 dequantise to 2^128, which bf16 spells Inf);
 *   - amax = 0 gives E = 0 and codes 0;
 *   - code = e4m3_rne(x * 2^-E), round to nearest even; the multiply is exact;
 *   - a non-finite element becomes the NaN code (a request with NaN inputs still ends with SV_EHIP);
 *   - every dequantised element 2^E * e4m3 is exactly a bf16 number.
 * The engine computes exactly what the bf16-KV engine computes over a cache holding deq(quant(.)), with one exception: a token's own pass
 * sees its unquantised K / V -- the prompt pass attends over the unquantised prompt, a decode step takes the new token's K / V in bf16 --
 * and every later step reads the quantised row.  Slots behind a sequence's position contribute exactly zero whatever codes and scale
 * bytes they hold.  A page is 64 * head_dim * 2 + 128 bytes (head_dim 128: 16,512 against 32,768) and the pool is sized from that.
 * Everything an engine serves it serves with either format, and with every weight format, except prompt-lookup drafting:
 * sv_generate_lookup, sv_generate_lookup_sampled and sv_cb_set_lookup (with drafts) answer SV_ENOTSUP on an SV_KV_FP8_E4M3 engine.
 * Not a reference numerics mode: the reference keeps its cache in bf16. */
#define SV_KV_BF16 0
#define SV_KV_FP8_E4M3 1
int  sv_create_kv(const sv_config* cfg, int32_t kv_dtype, sv_engine** out);
/* the engine's KV format, the bytes of one page (64 tokens, one layer, one KV head) and of the whole pool; any pointer may be NULL */
int  sv_kv_info(sv_engine* e, int32_t* kv_dtype, int64_t* page_bytes, int64_t* pool_bytes);

/* Ingest one tensor of the reference state_dict (device pointer, dtype SV_DTYPE_*).  Linear weights
 * are repacked into MFMA fragment order in library-owned memory; the caller's tensor is only read. */
int  sv_load_weight(sv_engine* e, const char* name, const void* dev_ptr, int32_t dtype, int32_t ndim,
                    const int64_t* shape, sv_stream stream);
/* 0 when every tensor the path needs has been loaded; otherwise SV_ENOENT and sv_last_error() names
 * the first missing key. */
int  sv_weights_complete(sv_engine* e);
/* The tensors an engine of this configuration expects, sorted by name: reference state_dict key (train/util.py:71 names), element
 * count, whether sv_weights_complete insists on it (the tied lm_head is optional) and whether it has been loaded.
 * sv_weight_count returns the number of entries (>= 0) or a negative error code. */
int  sv_weight_count(sv_engine* e);
int  sv_weight_info(sv_engine* e, int32_t index, char* name, int32_t name_cap, int64_t* numel, int32_t* required, int32_t* loaded);

/* image [B,3,S,S] bf16 (device) -> out [B, T, vit_width] bf16, T = (S/patch)^2 + 1 */
int  sv_encode_image(sv_engine* e, const void* dev_image, int32_t B, void* dev_out, sv_stream stream);
/* in [B,T,vit_width] bf16 -> out [B,T,hidden] bf16 */
int  sv_adapter(sv_engine* e, const void* dev_in, int32_t B, void* dev_out, sv_stream stream);
/* ids [n] int64 (device) -> out [n, hidden] bf16 */
int  sv_embed_tokens(sv_engine* e, const int64_t* dev_ids, int32_t n, void* dev_out, sv_stream stream);
/* The same two ops writing STRAIGHT into the inputs_embeds buffer [B][S0][hidden] that sv_prefill / sv_generate read (starvector_base.py:
 * 203-221 without the torch.cat): image b's visual rows -> rows 0 .. T-1 of its block; the P token rows of sequence b -> rows
 * row0 .. row0 + P - 1 (row0 = T for im2svg).  dev_ids: int64 [B][P]. */
int  sv_adapter_into(sv_engine* e, const void* dev_in, int32_t B, void* dev_embeds, int32_t S0, sv_stream stream);
int  sv_embed_tokens_into(sv_engine* e, const int64_t* dev_ids, int32_t B, int32_t P, void* dev_embeds, int32_t S0, int32_t row0,
                          sv_stream stream);

/* Image pre-processing on device = `ImageTrainProcessor.__call__` (starvector/data/util.py:40-68):
 * dev_pixels uint8 [height][width][channels] (3 = RGB, 4 = RGBA composited on white) -> white pad to square -> Pillow's
 * antialiased BICUBIC resize to out_size -> /255 -> (x - mean) / std.  dev_out float32 [3][out_size][out_size], bit for bit
 * the tensor the reference computes with Pillow + torchvision.  Needs no engine handle.
 * recipe 0: the above (clip branch).  recipe 1: the SigLIP tower's HF image processor (image_encoder.py:45-48,116-117):
 * alpha dropped (`convert("RGB")`), the image STRETCHED to out_size x out_size by the same resampler, rescale by 1/255 in
 * double, then (x - mean) / std (mean = std = 0.5 for google/siglip-large-patch16-384). */
int  sv_preprocess_image(const uint8_t* dev_pixels, int32_t width, int32_t height, int32_t channels, int32_t out_size,
                         int32_t recipe, const float* mean3, const float* std3, float* dev_out, sv_stream stream);

/* The same recipe for a BATCH of images of any sizes (the serving TTFT path: one call, three launches per 32 images):
 * dev_pixels / widths / heights / channels are HOST arrays of n entries (device pointers in dev_pixels); dev_out is float32
 * [n][3][out_size][out_size].  Stateless: the caller owns the workspace (sv_preprocess_workspace_bytes, a host computation),
 * the fixed-point tap tables are computed on device into it, every per-image parameter travels in the kernel arguments --
 * no host copy, no lock, no stream synchronisation, no library-owned buffer. */
int64_t sv_preprocess_workspace_bytes(const int32_t* widths, const int32_t* heights, int32_t n, int32_t out_size, int32_t recipe);
int  sv_preprocess_images(const uint8_t* const* dev_pixels, const int32_t* widths, const int32_t* heights,
                          const int32_t* channels, int32_t n, int32_t out_size, int32_t recipe, const float* mean3,
                          const float* std3, float* dev_out, void* dev_workspace, int64_t workspace_bytes, sv_stream stream);

/* Prompt pass over inputs_embeds [B,S0,hidden] bf16 (all-ones attention mask): fills the paged KV
 * cache and writes the last-row logits [B, vocab] fp32 (bf16-rounded values, as the reference's
 * bf16 lm_head produces). */
int  sv_prefill(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, float* dev_logits,
                sv_stream stream);
/* ---- ragged prompt pass: B sequences of DIFFERENT lengths in one pass.  dev_embeds_packed: the sequences' inputs_embeds back to back,
 * [sum(host_lens)][hidden] bf16 -- no padding row is computed or stored; host_lens: int32 [B] on the host, each in 1 .. max_seq_len.
 * Contract: for every sequence the last-row logits, the K / V entries in its pages and every token generated afterwards are BIT-IDENTICAL
 * to the same sequence alone through the rectangular entry point with S0 = host_lens[b]; with all lengths equal the ragged entry points
 * return exactly what the rectangular ones return.
 *   sv_prefill_ragged    sv_prefill: logits [B, vocab] fp32 of every sequence's last row; sv_decode_step continues every row at its own position
 *   sv_generate_ragged   sv_generate_ex with HF's padded-batch semantics: sp->max_length counts from the LONGEST prompt (HF counts the budget
 *                        from the padded length), so every row gets max_new = max_length - max(host_lens) new tokens.  Greedy, sampling,
 *                        repetition_penalty, the row-0 stop, EOS / pad, streaming, outs, and num_beams 2..8 (beam search / beam-sample; the
 *                        shared prompt pages and the cached length are per request).  outs may be NULL.
 *   sv_cb_admit_ragged   sv_cb_admit for n requests of prompt lengths host_lens[i] in ONE prompt pass; SV_EBUSY (nothing admitted) when
 *                        slots or KV pages are short.
 *   sv_forward_logprobs_ragged   sv_forward_topk (below) over sequences of different lengths, each with its own number of kept rows: host_keep
 *                        int32 [B] on the host, host_keep[b] in 1 .. host_lens[b] = the LAST rows of sequence b that are scored.  dev_targets and
 *                        every output are packed [sum(host_keep)], the lists [sum(host_keep)][k]: each sequence's kept rows are contiguous, in
 *                        sequence order.  Target -100, temperature, the outputs that may be NULL, k (0 = no lists), the order / ties / (-1, -inf)
 *                        tail / rank of the lists and the two failures (a target outside the vocabulary: SV_EINVAL; a row without a finite
 *                        logit: SV_EHIP -- the message names the sequence and the kept position inside it) are those of sv_forward_topk.  No
 *                        padding row goes through a layer or the lm_head.  Blocks until the pass has finished; leaves the engine as
 *                        sv_prefill_ragged does (sv_decode_step continues every row at its own position).
 *                        Contract: for every sequence b every output of its kept rows is BIT-IDENTICAL to sv_forward_topk on that sequence
 *                        alone (B = 1, S = host_lens[b], n_keep = host_keep[b]), whatever the other sequences, their order and the lm_head
 *                        chunk size.  (Not to the rows of a PADDED rectangular call: there a row takes its GEMM kernels by the padded S.)
 * SV_EINVAL before any device work for null pointers, B out of range, a length < 1 or > max_seq_len, max(len) + max_new > max_seq_len, a keep
 * outside 1 .. its length. */
int  sv_prefill_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, float* dev_logits,
                       sv_stream stream);
int  sv_forward_logprobs_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_keep,
                                const int32_t* dev_targets, float temperature, float* dev_logprob, float* dev_logsumexp, float* dev_entropy,
                                int32_t* dev_argmax, int32_t k, int32_t* dev_topk_ids, float* dev_topk_logprobs, int32_t* dev_rank, sv_stream stream);
/* ---- prompt rows behind a CACHED context: a second turn, a teacher-forced suffix, a long prompt in bounded pieces.  The engine keeps, on the
 * host, the number of tokens cached for every row of the cache.  It is known behind sv_prefill, sv_prefill_ragged, sv_prefill_open and
 * sv_prefill_extend, grows by one per sv_decode_step, and is UNKNOWN behind every other call that assigns pages or runs a prompt pass
 * (sv_generate*, beam search, the scoring forwards, continuous batching).
 *   sv_prefill_open      assigns pages for B sequences of host_total_lens[b] (1 .. max_seq_len) tokens each; every context becomes 0; nothing
 *                        is computed.  Returns when the table is on the device.
 *   sv_prefill_extend    appends host_lens[b] >= 0 rows to sequence b of the B cached sequences; dev_embeds_packed: the new rows back to back,
 *                        [sum(host_lens)][hidden] bf16; at least one length > 0, a 0 leaves the sequence and its logits row untouched.  The new
 *                        rows take positions ctx_b + j; they see the cache for everything before them (an e4m3 cache: its dequantised values)
 *                        and the unquantised K / V of the rows of this call, as the rows of a one-shot pass see each other.
 *                        host_total_lens[b] >= ctx_b + host_lens[b] (NULL: exactly that, the free extension) states the length of the sequence
 *                        the rows belong to: a row takes the GEMM kernel it takes in a one-shot pass over a sequence of THAT many rows.  The
 *                        last layer's rows and the last-row logits are computed for the sequences this call brings to their total length:
 *                        dev_logits [B][vocab] fp32 receives their rows, as sv_prefill_ragged writes them; the rows of the others are untouched.
 *                        Afterwards sv_decode_step and further extensions continue every row at its own position.
 *                        Contract (bf16 cache): a sequence fed through sv_prefill_open and any number of sv_prefill_extend calls with the same
 *                        total is BIT-IDENTICAL to sv_prefill_ragged over the whole sequence -- last-row logits, every K / V entry of its
 *                        pages, every token generated afterwards --, whatever the boundaries and whatever shares the passes.  A free extension is
 *                        bit-identical to the one-shot pass of the concatenation whenever both send the same rows through the split-K
 *                        remainder kernel (always, for lengths that leave no 1..3 rows over a multiple of 256).
 *                        SV_EINVAL before any device work for null pointers, B other than the cached sequences, a negative length, all
 *                        lengths 0, ctx + len > total, a total beyond the sequence's pages or max_seq_len; SV_ESTATE for unknown contexts or an
 *                        active continuous batch.
 *   sv_set_prefill_chunk rows = 0 (the default): off, every call issues the launches it always issued.  rows > 0: a row budget for every prompt
 *                        pass with a generate tail -- sv_prefill, sv_prefill_ragged, sv_generate*, the shared prompt pass, sv_cb_admit*.  A pass
 *                        of more packed rows runs as several extension passes of at most `rows` own rows: the sequences are walked in order,
 *                        each takes what the budget leaves, every sequence's total is its prompt length.  Same logits, same pages, same tokens
 *                        (bf16 cache: bit for bit; e4m3 cache: a later piece sees the dequantised cache of the earlier ones).  The prompt-pass
 *                        workspaces are sized by the budget; only the K | V rows gathered from the pages grow with the context.  The scoring
 *                        forwards are not chunked. */
int  sv_prefill_open(sv_engine* e, int32_t B, const int32_t* host_total_lens);
int  sv_prefill_extend(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_total_lens,
                       float* dev_logits, sv_stream stream);
int  sv_set_prefill_chunk(sv_engine* e, int32_t rows);
/* sv_forward_logprobs_ragged over sequences that SHARE PREFIXES (GRPO's log-prob pass: G completions per image): every prefix goes through
 * the decoder once, not once per sequence.  dev_prefix_packed: the P prefixes back to back, [sum(host_prefix_lens)][hidden] bf16;
 * dev_embeds_packed: the B sequences' OWN rows back to back, [sum(host_lens)][hidden] bf16.  Sequence b stands for the solo sequence
 * concat(prefix[host_prefix_of[b]], own rows of b) of T_b = Pl + host_lens[b] rows.  host_keep[b] in 1 .. host_lens[b] + 1 = the LAST rows
 * of that solo sequence that are scored; host_lens[b] + 1 reaches the prefix's last row, the row that predicts the first own token.
 * dev_targets, the outputs ([sum(host_keep)], lists [sum(host_keep)][k], in sequence order), -100, temperature, k, ties, ranks and the two
 * failures are those of sv_forward_logprobs_ragged.  Blocks until the pass has finished, under the same lock.
 * Contract: every output of sequence b's kept rows is BIT-IDENTICAL to sv_forward_topk on the concatenated sequence alone (B = 1,
 * S = T_b, n_keep = host_keep[b]), whatever the other sequences, their order, the number of sequences per prefix and the lm_head chunk size.
 * Refusal rule: where a solo run of T_b rows sends its last T_b % 256 (1..3, T_b > 256) rows through the split-K remainder kernel for any of
 * the four decoder projections and host_lens[b] is smaller than that, a PREFIX row would need different bits for different sharers:
 * SV_EINVAL naming the sequence, before any device work (score that sequence with sv_forward_logprobs_ragged on its concatenation).
 * KV cache: no page is assigned or written; afterwards sv_decode_step refuses (SV_ESTATE) until the next prompt pass, which behaves as on
 * a fresh engine.  The last layer runs over the prefix rows as well (their c_proj / MLP work there is not skipped).
 * SV_EINVAL before any device work for null pointers, P or B out of range (1 <= P <= B <= max_batch), a host_prefix_of outside 0 .. P - 1,
 * a prefix no sequence uses, a length < 1, T_b > max_seq_len, a keep outside 1 .. host_lens[b] + 1, and the temperature / k / output rules of
 * sv_forward_logprobs_ragged.  SV_ESTATE while continuous-batch slots are live.  Weight formats: bf16, fp8 (e4m3) and mxfp4 engines alike
 * (the contract is against the same engine's solo run); there is no format the call answers with SV_ENOTSUP. */
int  sv_forward_logprobs_prefixed(sv_engine* e, const void* dev_prefix_packed, int32_t P, const int32_t* host_prefix_lens,
                                  const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_prefix_of,
                                  const int32_t* host_keep, const int32_t* dev_targets, float temperature, float* dev_logprob,
                                  float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t k, int32_t* dev_topk_ids,
                                  float* dev_topk_logprobs, int32_t* dev_rank, sv_stream stream);
/* Scoring forward =`StarVectorForCausalLM.forward(vision_embeds, input_ids, ..., num_logits_to_keep)`
 * (starvector_arch.py:161-184; GRPO's log-prob pass, inference mode): the decoder over inputs_embeds [B,S,hidden] bf16
 * (all-ones mask) and the lm_head over the LAST n_keep positions of every sequence.
 * dev_logits_bf16: [B, n_keep, vocab] bf16, the dtype the reference's bf16 lm_head returns.  Also leaves the KV cache
 * filled like sv_prefill. */
int  sv_forward_logits(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep,
                       void* dev_logits_bf16, sv_stream stream);
/* Scoring forward that keeps no logits: the decoder over inputs_embeds [B,S,hidden] bf16 exactly as sv_forward_logits,
 * then for row (b, j), j < n_keep, = position S - n_keep + j: the log-probability of dev_targets[b][j] under
 * softmax(logits / temperature), where logits are the bf16 values sv_forward_logits would have returned for that row
 * (fp32 arithmetic over them).  dev_targets int32 [B][n_keep]; -100 = ignore (logprob 0).  Outputs fp32 / int32
 * [B][n_keep], each may be NULL (not all): logprob, logsumexp of logits / temperature, entropy of the softmax, argmax =
 * the lowest index holding the row's maximum.  temperature > 0.  The lm_head runs over the rows in chunks: device
 * memory does not grow with B x n_keep x vocab.  A target outside [0, vocab) that is not -100: SV_EINVAL naming the
 * row (its logprob is NaN, everything else is written).  Blocks until the pass has finished.  KV side effects as
 * sv_forward_logits. */
int  sv_forward_logprobs(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep,
                         const int32_t* dev_targets, float temperature, float* dev_logprob, float* dev_logsumexp,
                         float* dev_entropy, int32_t* dev_argmax, sv_stream stream);

/* One autoregressive step for tokens [B] int32 (device) appended after the cached context. */
int  sv_decode_step(sv_engine* e, const int32_t* dev_tokens, int32_t B, float* dev_logits, sv_stream stream);

/* Full generation.  out_tokens [B, max_new] int64 (device, max_new = max_length - S0) receives the
 * NEW tokens only (HF semantics); *n_generated = number of columns produced (<= max_new); trailing
 * columns are left untouched.  Blocks until generation has finished (polls a device flag). */
int  sv_generate(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, const sv_sampling* sp,
                 int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);

/* Per-step outputs of a generate call (HF return_dict_in_generate with output_scores / output_logits, transformers 4.49
 * generation/utils.py _sample and _beam_search).  rows = batch for greedy / sampling, batch * num_beams for beam search; step t
 * of row r lives at slab[(t * rows + r) * ld].  Only the first *n_generated steps are written; the rest are left untouched.
 *   dev_logits   raw fp32 logits of each step, before any processor (the bf16-rounded values of the lm_head)
 *   dev_scores   greedy / sampling: RepetitionPenalty -> MinLength hold -> (do_sample) s / temperature, TopK, TopP with the
 *                removed tokens at -inf;  beam search: log_softmax -> RepetitionPenalty -> MinLength -> (beam-sample) the warpers
 *                with min_tokens_to_keep = 2: the processed log-probs the scorer ranks
 *   host_sequences_scores   [batch]: the best hypothesis' length-penalised score (beam search only)
 *   host_beam_indices       [batch][max_new]: the flat row (b * num_beams + beam) of step t's scores the hypothesis took its
 *                           token from, -1 after the hypothesis ends (beam search only)
 * Every pointer may be NULL.  Capturing costs 2 x rows x vocab fp32 stores per decode step; with the slabs NULL no extra kernel runs. */
typedef struct sv_generate_outputs {
    float*   dev_scores;             /* [max_new][rows][ld] fp32, or NULL */
    float*   dev_logits;             /* [max_new][rows][ld] fp32, or NULL */
    int64_t  ld;                     /* >= vocab */
    float*   host_sequences_scores;  /* [batch], beam search only, or NULL */
    int64_t* host_beam_indices;      /* [batch][max_new], beam search only, or NULL */
} sv_generate_outputs;

/* sv_generate with per-step outputs; sv_generate(...) == sv_generate_ex(..., outs = NULL, ...).  SV_EINVAL for ld < vocab with a
 * slab, and for the beam-only pointers without num_beams > 1. */
int  sv_generate_ex(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, const sv_sampling* sp,
                    const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);
int  sv_generate_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const sv_sampling* sp,
                        const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);
/* ---- several samples of ONE prompt from one prompt pass (GRPO roll-outs: num_return_sequences = G; vLLM: SamplingParams.n).
 * sv_generate_shared: B prompts -- host_lens NULL: dev_embeds_packed is [B][S0][hidden]; otherwise the ragged form, prompts of host_lens[b] rows
 * packed back to back (S0 ignored) -- and n_samples continuations of each: B * n_samples <= max_batch decode rows, row b * n_samples + j = sample j
 * of prompt b, the row order of repeat_interleave.  The prompt pass runs over the B prompts only; the rows of a prompt share its full 64-token KV
 * pages through the block table and own every page from the prompt's partially filled tail page on (copied once, on device, before the first
 * token).  Contract: tokens, *n_generated and the per-step outputs are BIT-IDENTICAL to sv_generate_ex / sv_generate_ragged over the prompts
 * repeated n_samples times each (the sampler draws from (seed, step, row)).  dev_out_tokens [B * n_samples][max_new]; outs rows = B * n_samples;
 * streaming delivers B * n_samples rows; n_samples = 1 is sv_generate_ex / sv_generate_ragged.  num_beams > 1 with n_samples > 1: SV_ENOTSUP.
 * sv_cb_admit_shared: the group admit of a continuous batch -- n_prompts prompts (ragged, packed), n requests, request i samples prompt
 * host_group[i] and keeps its own sv_cb_request (seed, budget, sampler, stop ids).  Prompts are numbered in the order their first request appears
 * (host_group[0] = 0, host_group[i] <= max(host_group[0..i)) + 1, every prompt used).  One prompt pass over the prompts; each request's tokens are
 * those of its solo sv_cb_admit.  A prompt's full pages are held once and reference-counted: sv_cb_release of a sample returns its own pages at once
 * and a shared page when its last holder lets go.  SV_EBUSY (nothing admitted) when n slots or
 * sum_u len_u / 64 + sum_i (ceil((len + budget_i) / 64) - len / 64) pages are not free.  SV_EINVAL before any device work for null pointers,
 * n_samples < 1, a length < 1, host_group[i] out of range or out of order. */
int  sv_generate_shared(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                        const sv_sampling* sp, const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);
/* ---- HF logits processors that change tokens, on device (transformers 4.49 generation/logits_process.py): what HF generate's
 * no_repeat_ngram_size, bad_words_ids and min_p arguments do.  The history g[0 .. t-1] of a row is its GENERATED ids only (with inputs_embeds
 * HF's input_ids start empty); a finished row keeps receiving pads and they count, as in HF.
 *   no_repeat_ngram_size n   NoRepeatNGramLogitsProcessor: at step t every id g[j+n-1], 0 <= j <= t-n, with g[j .. j+n-2] == g[t-n+1 .. t-1] is
 *                            banned (nothing while t < n-1; n = 1 bans every earlier id)
 *   bad words                NoBadWordsLogitsProcessor: a sequence of one id is always banned; the last id of a sequence of L > 1 ids is banned
 *                            when t >= L and g[t-L+1 .. t-1] are its first L-1 ids (HF ignores a sequence "longer than the context", L > t).
 *                            At most 64 sequences of at most 8 ids, every id inside the vocabulary: anything else is SV_EINVAL, nothing is
 *                            truncated
 *   min_p                    MinPLogitsWarper, after temperature, top-k and top-p: tokens with p < min_p * p_max are dropped, the maximum
 *                            always stays; used when do_sample only; 0 = off, at most 1
 * A banned id's score is -inf in the fp32 logits row before the repetition penalty, the min-length hold and the selection see it; of the
 * per-step outputs dev_logits stays raw and dev_scores shows the -inf, as in HF.
 * sv_generate_processed = sv_generate_shared (rectangular or ragged prompts through host_lens, n_samples continuations of each) with such a set.
 * lp NULL or all zero: exactly sv_generate_shared, the same captured decode step.  An active ban adds one launch per step (ban_tokens_kernel,
 * inside the captured step, and in front of the first selection after the prompt pass) and takes the separate selection launch, like a
 * repetition penalty.  num_beams > 1 with any processor set: SV_EINVAL (beam rows reorder their histories; not built).  The host arrays are
 * read during the call only. */
typedef struct sv_logits_processors {
    int32_t no_repeat_ngram_size;      /* 0 = off, 1..8 */
    int32_t n_bad_words;               /* 0..64 */
    const int32_t* bad_word_lens;      /* host [n_bad_words], each 1..8 */
    const int32_t* bad_word_ids;       /* host, the sequences back to back: sum(bad_word_lens) ids */
    float min_p;                       /* 0 = off, (0, 1] */
} sv_logits_processors;
int  sv_generate_processed(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                           const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs, int64_t* dev_out_tokens,
                           int32_t* n_generated, sv_stream stream);
/* ---- per-token statistics of a roll-out, from the decode loop itself (GRPO's old-policy log-probs, best-of-n reranking, confidence filters):
 * sv_generate_stats = sv_generate_processed plus, for the token tok that row r emits in column t, three fp32 values at [r][t] of the caller's
 * device buffers ([rows][ld] each, rows = B * n_samples, ld >= max_new = max_length - prompt length; any may be NULL, not all three):
 *   dev_logprob            log_softmax(x / T)[tok]; x = the step's raw lm_head row (what sv_generate_outputs.dev_logits holds: before bans, the
 *                          min-length hold and the repetition penalty), T = temperature when do_sample, else 1 -- the quantity
 *                          sv_forward_logprobs(..., temperature = T) returns for that position
 *   dev_entropy            entropy of softmax(x / T)
 *   dev_logprob_processed  log_softmax(s)[tok]; s = the processed row (what dev_scores holds: bans -> repetition penalty -> min-length hold ->
 *                          with do_sample / T, top-k, top-p, min_p, removed ids at -inf; the kept set is the one dev_scores shows) -- HF's
 *                          compute_transition_scores(..., normalize_logits = True)
 * A row that had finished before column t gets 0 in all three (columns >= *n_generated are not written).  No [rows][vocab] output exists: the
 * cost is one launch per step (one 1024-thread block per row, fp32 reductions) between the selection and the bookkeeping, two when the step
 * rewrites the raw row in place (a token ban, the min-length hold: the raw row's sums are then taken in front of the rewrite).  A call with
 * statistics takes the separate selection launch, like a repetition penalty or a capture; its captured step is keyed on the statistics, so a
 * plain call afterwards replays the plain step and the other way round, and a kept graph writes each call's own buffers (device descriptor).
 * Tokens and *n_generated are those of sv_generate_processed bit for bit.  stats NULL: exactly sv_generate_processed, the same captured step.
 * SV_EINVAL before any device work for ld < max_new, for all three pointers NULL and for num_beams > 1 (beam search reports
 * sequences_scores; beam rows reorder). */
typedef struct sv_token_stats {
    float* dev_logprob;                /* [rows][ld] fp32, or NULL */
    float* dev_logprob_processed;      /* [rows][ld] fp32, or NULL */
    float* dev_entropy;                /* [rows][ld] fp32, or NULL */
    int64_t ld;                        /* >= max_new */
} sv_token_stats;
int  sv_generate_stats(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                       const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs, const sv_token_stats* stats,
                       int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);
/* ---- the k most likely ids of every step's distribution, their log-probs, and the rank of the emitted token (distillation from roll-outs,
 * a confidence read-out, best-of-n diagnostics) without a [steps][rows][vocab] slab: sv_generate_topk = sv_generate_stats plus, for the token
 * that row r emits in column t, k ids and k fp32 log-probs at [r][t][0..k) and the token's rank at [r][t] of the caller's device buffers.
 *   source 0  the distribution of sv_token_stats.dev_logprob: log_softmax(x / T) over the step's raw row
 *   source 1  the distribution of dev_logprob_processed: the processed row, the ids outside the kept set at -inf (they are never listed)
 * Order: descending by value, equal values by ascending id (slot 0 is what greedy selection picks).  The key is the value BEFORE the division
 * by T, so rounding after it never reorders or merges entries.  NaN and -inf never enter; with fewer than k ids that do (vocab < k, a kept
 * set smaller than k) the tail slots hold id -1 and log-prob -inf.  A slot's log-prob is the expression that yields dev_logprob /
 * dev_logprob_processed: the slot of the emitted id equals that statistic bit for bit.  rank = 1 + #{ i : x_i > x_tok } (vLLM's definition,
 * NaN compares false).  A row that had finished before column t: ids -1, log-probs 0, rank 0.  A row without a comparable value: ids -1,
 * rank 0, log-probs NaN.  A row's output depends on that row alone: the same bits in any batch and launch.
 * Cost: one launch per step (one 1024-thread block per row) beside the statistics launch; with source 0 on a step that rewrites the raw row in
 * place (a token ban, the min-length hold) it runs in front of the rewrite, where the token is not yet known -- dev_rank with source 0 and such a
 * processor is SV_EINVAL (use source 1, or pass no dev_rank).  The captured step is keyed on (k, source, rank asked for); the buffers travel
 * through a device descriptor, so a kept graph writes each call's own buffers and a plain or statistics call afterwards replays its own step.
 * Tokens, *n_generated and the statistics are those of sv_generate_stats bit for bit.  topk NULL: exactly sv_generate_stats (stats may be
 * NULL as well: sv_generate_processed).  SV_EINVAL before any device work for k outside 1..SV_TOPK_MAX, a NULL dev_ids / dev_logprobs,
 * ld < max_new, num_beams > 1, source outside {0, 1} and the rank combination above. */
#define SV_TOPK_MAX 32
typedef struct sv_token_topk {
    int32_t  k;              /* 1..SV_TOPK_MAX */
    int32_t  source;         /* 0 = log_softmax(raw / T), 1 = processed scores */
    int32_t* dev_ids;        /* [rows][ld][k] */
    float*   dev_logprobs;   /* [rows][ld][k] */
    int32_t* dev_rank;       /* [rows][ld], or NULL */
    int64_t  ld;             /* >= max_new */
} sv_token_topk;
int  sv_generate_topk(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                      const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs, const sv_token_stats* stats,
                      const sv_token_topk* topk, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream);
/* ---- prompt-lookup speculative decoding for greedy generate (HF's generate(..., prompt_lookup_num_tokens = K); entry point appended,
 * SV_ABI_VERSION unchanged).  A decode step costs the same for 1 row as for 32, so one step VERIFIES K drafted tokens of every sequence: B x (K + 1)
 * rows, row j of a sequence carrying its j-th draft at position ctx + j, all of them on the sequence's own KV pages.  The drafts come from an
 * n-gram lookup over the ids the sequence has generated so far (for n = max_ngram .. min_ngram: the latest earlier occurrence of the last n
 * ids, then the ids that followed it) -- no draft model.  A step emits the accepted drafts and one token more.  Greedy verification is
 * exact: tokens and *n_generated are those of sv_generate / sv_generate_ragged BIT FOR BIT, for every B, including the reference's row-0 stop
 * sequence (which ends the batch at row 0's column for every row), EOS / pad and min_new_tokens.
 * host_counts3 (may be NULL): {verification steps, drafts verified, drafts accepted}.  lookup NULL or num_draft_tokens == 0: this IS
 * sv_generate_ragged (host_lens given) / sv_generate.  Streaming works with B == 1.
 * SV_EINVAL before any device work: NULL arguments, num_draft_tokens outside 0..SV_LOOKUP_MAX_DRAFT, max_ngram outside 0..SV_LOOKUP_MAX_NGRAM,
 * min_ngram outside 0..max_ngram.  SV_ENOTSUP, naming the offender: do_sample, num_beams > 1, repetition_penalty != 1, streaming with
 * B > 1, B x (K + 1) > max_batch.  Continuous batching (sv_cb_*) drafts per request once sv_cb_set_lookup has switched it on. */
#define SV_LOOKUP_MAX_DRAFT 15
#define SV_LOOKUP_MAX_NGRAM 8
typedef struct sv_lookup {
    int32_t num_draft_tokens;   /* K: 1..SV_LOOKUP_MAX_DRAFT (0: a plain call) */
    int32_t max_ngram;          /* 1..SV_LOOKUP_MAX_NGRAM, 0 = 3 */
    int32_t min_ngram;          /* 1..max_ngram, 0 = 1 */
} sv_lookup;
int  sv_generate_lookup(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, const sv_sampling* sp,
                        const sv_lookup* lookup, int64_t* dev_out_tokens, int32_t* n_generated, int32_t* host_counts3, sv_stream stream);
/* sv_generate_lookup with the selection the call's sv_sampling asks for (entry point appended, SV_ABI_VERSION unchanged): do_sample 0 or 1 with
 * temperature / top_k / top_p / seed, and any repetition_penalty.  Still token-exact, per seed: the sampler's random number is a pure function
 * of (seed, step, row), so row j of sequence s draws with the triple sv_generate uses at column n_emit_s + j of row s, over the same logits
 * bits; a draft is accepted when it equals the token DRAWN in front of it (what HF does for do_sample with prompt_lookup_num_tokens: draw at
 * every position, match against the drafts).  The repetition penalty of row j sees the sequence's generated ids plus the drafts d_1 .. d_j in
 * front of the row -- the plain call's set at that column once those drafts are accepted.  Tokens and *n_generated are those of
 * sv_generate / sv_generate_ragged with the same sv_sampling, BIT FOR BIT; rectangular and ragged prompts, EOS / pad, min_new_tokens, the row-0
 * stop sequence, streaming with B == 1.  lookup NULL or num_draft_tokens == 0: the plain call.
 * SV_ENOTSUP, naming the offender: num_beams > 1, streaming with B > 1, B x (K + 1) > max_batch, live continuous-batching slots (SV_ESTATE as
 * every generate call).  The signature carries no n_samples, processors, per-step outputs, statistics or top-k lists: none is built with it. */
int  sv_generate_lookup_sampled(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, const sv_sampling* sp,
                                const sv_lookup* lookup, int64_t* dev_out_tokens, int32_t* n_generated, int32_t* host_counts3, sv_stream stream);
/* sv_forward_logprobs plus, for every kept position, the k best ids of softmax(logits / temperature) over the bf16 row, their log-probs
 * (dev_topk_ids int32 / dev_topk_logprobs fp32, [B][n_keep][k]) and the rank of the target (dev_rank int32 [B][n_keep], may be NULL; target
 * -100: rank 0).  Order, ties, the (-1, -inf) tail and the rank as in sv_generate_topk, keyed on the bf16 logit; a slot holds
 * float(logit) * (1 / temperature) - logsumexp, the expression behind dev_logprob: the slot of the target equals dev_logprob bit for bit and
 * slot 0's id is dev_argmax.  Computed chunk by chunk from the lm_head workspace like the log-probs: device memory does not grow with
 * B x n_keep x vocab.  k = 0: exactly sv_forward_logprobs (the three new pointers are ignored).  The four outputs of sv_forward_logprobs may
 * all be NULL when k > 0.  SV_EINVAL before any device work for k outside 0..SV_TOPK_MAX and for k > 0 with a NULL dev_topk_ids /
 * dev_topk_logprobs. */
int  sv_forward_topk(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep, const int32_t* dev_targets, float temperature,
                     float* dev_logprob, float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t k, int32_t* dev_topk_ids,
                     float* dev_topk_logprobs, int32_t* dev_rank, sv_stream stream);
/* ---- continuous batching (the reference worker's 5 concurrent requests, serve/model_worker.py:161-172,
 * 216-229, as ONE decode loop).  Every row ("slot") of the engine's batch is an independent request: own sampling parameters,
 * budget, EOS, stop sequence (the reference's row-0 stop, starvector_base.py:9-20, is right for one request per generate call
 * and becomes each request's own stop here) and random stream.  A request yields the same tokens as when it runs alone through
 * sv_generate.  While a continuous batch is active the classic entry points (sv_prefill / sv_generate / ...) return SV_ESTATE.
 *   sv_cb_admit    prompt pass of n new requests of equal prompt length S0 (dev_embeds [n][S0][hidden] bf16) into free slots --
 *                  the live slots keep their KV pages -- and their first token; slots_out [n] = the slots taken.
 *                  SV_EBUSY when slots or KV pages are short (nothing is admitted then).
 *   sv_cb_step     n_steps decode steps for all live slots (one captured hipGraph per row bucket, kept on the engine);
 *                  *n_live = slots still generating afterwards.  Finished slots idle until released.
 *   sv_cb_poll     per slot: live flag and number of tokens emitted so far (host arrays of `capacity` >= max_batch entries)
 *   sv_cb_read     tokens [first, first + count) of a slot -> host int64
 *   sv_cb_release  frees a slot and its KV pages (stops it if it is still generating)
 *   sv_cb_reset    releases everything; the engine is back to the classic entry points
 * The batch drafts per request when sv_cb_set_lookup (below) has switched it on: a slot then owns K + 1 rows, a step emits 1 .. K + 1
 * tokens per live slot, the batch holds max_batch / (K + 1) slots -- and every request's tokens stay exactly what they are without it. */
typedef struct sv_cb_request {
    int32_t do_sample; float temperature; float top_p; int32_t top_k;     /* as in sv_sampling */
    uint64_t seed;
    int32_t max_new_tokens;    /* new-token budget of THIS request (HF: max_length - prompt length) */
    int32_t eos_token_id, pad_token_id;
    int32_t min_new_tokens;
    float   repetition_penalty;
    int32_t n_stop;            /* 0..16 */
    int32_t stop_ids[16];
    /* ABI 9, appended.  All zero = the fields above alone (HF semantics, unchanged).  semantics = 1 selects vLLM 0.5.5's
     * sampler for this request: logit_bias -> min_tokens hold (eos_token_id and stop_any_ids -> -inf while fewer than
     * min_new_tokens were emitted) -> repetition_penalty over prompt_ids and the output ids (l > 0 ? l / rp : l * rp) ->
     * frequency_penalty * count -> presence_penalty * (count > 0), counts over the output ids only -> greedy argmax when
     * do_sample = 0, else temperature -> top-k -> top-p -> min_p -> one draw.  Every field below is rejected (SV_EINVAL) unless
     * semantics = 1, so none is lost silently.  Host arrays are read during sv_cb_admit only. */
    int32_t semantics;         /* 0 = HF, 1 = vLLM */
    float   presence_penalty, frequency_penalty, min_p;      /* min_p in [0, 1], 0 = off */
    int32_t n_prompt_ids; const int32_t* prompt_ids;          /* token ids of the text prompt: seed the repetition set */
    int32_t n_logit_bias;      /* 0..128, distinct ids; values clamped to [-100, 100] */
    const int32_t* logit_bias_ids; const float* logit_bias_values;
    int32_t n_stop_any;        /* 0..8: emitting any one of these ids ends the request */
    int32_t stop_any_ids[8];
} sv_cb_request;
int  sv_cb_admit(sv_engine* e, const void* dev_embeds, int32_t n, int32_t S0, const sv_cb_request* reqs, int32_t* slots_out,
                 sv_stream stream);
int  sv_cb_admit_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t n, const int32_t* host_lens, const sv_cb_request* reqs,
                        int32_t* slots_out, sv_stream stream);
int  sv_cb_admit_shared(sv_engine* e, const void* dev_embeds_packed, int32_t n_prompts, const int32_t* host_lens, int32_t n,
                        const int32_t* host_group, const sv_cb_request* reqs, int32_t* slots_out, sv_stream stream);
int  sv_cb_step(sv_engine* e, int32_t n_steps, int32_t* n_live, sv_stream stream);
int  sv_cb_poll(sv_engine* e, int32_t* host_live, int32_t* host_steps, int32_t capacity);
int  sv_cb_read(sv_engine* e, int32_t slot, int32_t first, int32_t count, int64_t* host_tokens);
int  sv_cb_release(sv_engine* e, int32_t slot);
int  sv_cb_reset(sv_engine* e);
/* Per-request log-probs on the continuous batch (entry points appended; SV_ABI_VERSION and sv_cb_request are unchanged).
 * sv_cb_admit_logprobs is sv_cb_admit_shared -- packed prompts, request i samples prompt host_group[i] -- plus lps [n], parallel to reqs: what
 * request i records for every token it emits, the first one (selected inside the admit from the prompt's logits) being column 0.  lps NULL or
 * every enable 0: exactly sv_cb_admit_shared, same tokens and launches.  A recording slot keeps, per column, the emitted token's log-prob and
 * rank and the k best ids with their log-probs; the definitions are sv_generate_topk's for the same k and source (descending by the value before
 * the division by T, equal values by ascending id, tail (-1, -inf), rank = 1 + #{ x_i > x_tok }, the slot of the emitted id equals the token's
 * log-prob bit for bit, a row without a comparable value reads ids -1 / rank 0 / log-probs NaN), and an HF-semantics slot's record equals its
 * solo sv_generate_topk output bit for bit:
 *   source 0   log_softmax(raw / T), T = the slot's temperature when it samples, else 1.  HF slots only: a vLLM-semantics slot has rewritten
 *              its raw row in place by then (SV_EINVAL at admit)
 *   source 1   the processed row.  HF: repetition penalty, the min-length hold of EOS, the sampler's kept set, removed ids at -inf.  vLLM: what
 *              vLLM 0.5.5's Sampler reports -- log_softmax over the row after logit_bias, the min_tokens hold and the repetition / frequency /
 *              presence penalties; a sampling slot divides by its temperature and applies its top-k / top-p / min_p masks first, a greedy
 *              slot uses T = 1 and no mask.  The rank is taken over the same vector.
 * The record is written inside the slot's own selection block (after the token is known, before the slot's repetition set and counts take it),
 * so it depends on that slot alone: the same bits whether other slots record or not, in any row bucket, however many steps a sv_cb_step call
 * runs.  A batch with a recording slot runs the recording form of the selection kernel (its captured step graphs are kept beside the plain
 * ones); a batch in which nobody records replays exactly the graphs it replayed before.
 * Memory: the first admit that asks allocates, for the life of the engine, max_batch x max_seq_len x (8 + 8 x SV_TOPK_MAX) bytes = 264 B per
 * slot column (64 slots x 8192 columns: 138 MB); an engine that never asks allocates nothing.
 * sv_cb_read_logprobs copies columns [first, first + count) of a slot to the host: host_logprob / host_rank [count], host_ids / host_lps
 * [count][k] with the slot's own k (each may be NULL).  Only columns the slot has emitted (< its steps in sv_cb_poll) exist: anything beyond, a
 * slot admitted without enable and a slot not in use are SV_EINVAL -- a reused slot never shows its predecessor's columns.
 * SV_EINVAL before any device work for an enabled entry with k outside 0..SV_TOPK_MAX, a source outside {0, 1}, or source 0 with semantics 1. */
typedef struct sv_cb_logprobs {
    int32_t enable;            /* 0: this request records nothing and costs nothing */
    int32_t k;                 /* 0..SV_TOPK_MAX: 0 = the emitted token's log-prob and rank only */
    int32_t source;            /* 0 raw, 1 processed */
} sv_cb_logprobs;
int  sv_cb_admit_logprobs(sv_engine* e, const void* dev_embeds_packed, int32_t n_prompts, const int32_t* host_lens, int32_t n,
                          const int32_t* host_group, const sv_cb_request* reqs, const sv_cb_logprobs* lps, int32_t* slots_out, sv_stream stream);
int  sv_cb_read_logprobs(sv_engine* e, int32_t slot, int32_t first, int32_t count, float* host_logprob, int32_t* host_rank, int32_t* host_ids,
                         float* host_lps);
/* Prompt-lookup drafting for the continuous batch (entry points appended; SV_ABI_VERSION and sv_cb_request are unchanged).  With
 * num_draft_tokens = K > 0 a slot owns K + 1 decode rows -- rows slot * (K + 1) + j of the step, row j carrying the slot's j-th draft on the
 * slot's own KV pages, as in sv_generate_lookup -- and a sv_cb_step step is a VERIFICATION step: every live slot emits 1 .. K + 1 tokens, and
 * sv_cb_poll's step counts advance by that much.  The drafts come from the n-gram lookup over the ids the slot has emitted; a slot never drafts
 * past its own budget.  The slot's rows are verified one after the other inside the slot's selection block with the plain step's own code
 * against the slot's current state, so every request's tokens, its finish and its log-prob record are those of the same request in a batch
 * with drafting off, BIT FOR BIT: greedy and sampled (the draw at a column uses (seed, column) as always), repetition penalty, min_new_tokens,
 * stop sequence, vLLM semantics with penalties, logit_bias, min_p and stop_any_ids, every admit form.  The cost: the batch holds
 * max_batch / (K + 1) slots (sv_cb_admit* return SV_EBUSY beyond that, as when slots are short); slot ids, sv_cb_poll's arrays, sv_cb_read and
 * sv_cb_release stay indexed by slot; the KV pages a request needs are unchanged.
 * lookup NULL or num_draft_tokens == 0: off (the default; every sv_cb_* call is then exactly what it is without this entry point).
 * Only while no continuous batch is active (before the first admit, or after sv_cb_reset): SV_ESTATE otherwise.  The setting stays on the engine
 * across sv_cb_reset.  Defaults and ranges of sv_lookup as in sv_generate_lookup (max_ngram 0 = 3, min_ngram 0 = 1); SV_EINVAL before any device work
 * for values outside them; SV_ENOTSUP when max_batch / (K + 1) < 1. */
int  sv_cb_set_lookup(sv_engine* e, const sv_lookup* lookup);
/* {verification steps, drafts verified, drafts accepted} of a slot since its admit; slot = -1: totals since the batch began (steps summed over
 * the slots: one per live slot and step).  Host array of 3.  All zero while drafting is off. */
int  sv_cb_lookup_counts(sv_engine* e, int32_t slot, int32_t* host_counts3);
/* A prefix cache for the continuous batch (entry points appended; SV_ABI_VERSION and every struct are unchanged).  Off by default; with it off
 * every sv_cb_* call issues exactly the launches and takes exactly the pages it takes without these entry points.  With it on, every admit form
 * (sv_cb_admit, _ragged, _shared, _logprobs; with or without sv_cb_set_lookup and sv_set_prefill_chunk) first digests the full 64-row pages of its
 * prompts on the device (one launch, one copy to the host), chains the digests into keys -- a key stands for "these exact rows at these exact
 * positions behind exactly this prefix" -- and looks them up in a table of the prompt pages earlier admits of this batch computed.  A prompt of L
 * rows reuses h = min(leading pages found, (L - 1) / 64) pages: they enter the block-table rows of its slots read-only (held once per slot, as
 * shared prompt pages are), only the other pages leave the free list, and the prompt pass computes rows 64 h .. L - 1 behind the cached context.
 * After the pass every full prompt page, computed or reused, stands in the table under its key (a key already present keeps its page; the partial
 * tail page never enters).  A released slot's cached pages stay resident while no admit needs them: pages without a holder are evicted least
 * recently released first when the free list is short, pages with a holder never; SV_EBUSY only when free + evictable pages are short, so an
 * admit never fails with the cache on where it succeeds with it off.  A failed admit registers nothing and gives back the holders it added.
 * The contract: on a bf16-KV engine everything of a request -- every token, its finish, its log-prob record, the K / V bytes of its own pages --
 * is bit for bit what the same request returns with the cache off, whatever was cached before and whatever is evicted meanwhile.
 * Keys are 128 bits and a hit is not verified against the rows.  The table lives until sv_cb_reset (sv_load_weight drops it too).
 * sv_cb_set_prefix_cache: only while no continuous batch is active (SV_ESTATE otherwise); the setting stays across sv_cb_reset.  SV_ENOTSUP on an
 * fp8_e4m3 KV engine (a pass behind cached pages sees the dequantised cache, a one-shot pass the unquantised rows: the tokens could differ) and
 * while the A/B arm SV_EXP_BATCH_REMAINDER is selected.
 * sv_cb_prefix_cache_info: host array of 5 = {full prompt pages looked up, pages reused, pages resident in the table, of those without a holder,
 * evictions} since the batch began; all 0 while off. */
int  sv_cb_set_prefix_cache(sv_engine* e, int32_t enable);
int  sv_cb_prefix_cache_info(sv_engine* e, int64_t* host_out5);

/* beam scorer: one step consumes dev_logits [batch * num_beams][ld] (row r = request r / num_beams, beam r % num_beams)
 * and reports (host arrays, each batch * num_beams long, may be NULL) the flat parent row, the token and the running
 * score of every beam that continues; *done = 1 once HF's loop would stop.  sv_beam_finalize returns the best
 * hypothesis per request: host_tokens [batch][max_new] (filled with pad-or-eos), *n_generated = common length. */
int  sv_beam_create(const sv_beam_config* cfg, sv_beam** out);
int  sv_beam_destroy(sv_beam* b);
int  sv_beam_step(sv_beam* b, const float* dev_logits, int32_t ld, int32_t* done, int32_t* host_parent,
                  int32_t* host_tokens, float* host_scores, sv_stream stream);
int  sv_beam_finalize(sv_beam* b, int64_t* host_tokens, int32_t* n_generated, float* host_scores, sv_stream stream);

/* Search trace of the last beam-search sv_generate on this engine (parity tests replay it through the oracle):
 * host_parent / host_tok [n_steps][rows], rows = batch * num_beams; entry (t, r) = the beam (index inside its request)
 * that running beam r descended from at step t, and the token it took.  NULL arrays: only *n_steps / *rows. */
int  sv_beam_history(sv_engine* e, int32_t* host_parent, int32_t* host_tok, int32_t capacity_steps, int32_t* n_steps,
                     int32_t* rows);

/* host wall-clock of the last sv_generate, 4 doubles: [0] ms prefill + first token (TTFT),
 * [1] ms decode loop, [2] decode steps enqueued, [3] decode steps per hipGraph launch (0: plain launches, 1: one step per replay,
 * > 1: the step captured that many times into one graph for calls long enough to pay for it -- SV_GRAPH_STEPS, default 32, 1 = off) */
int  sv_last_timing(sv_engine* e, double* out4);

#ifdef __cplusplus
}
#endif
#endif /* STARVECTOR_HIP_H */
