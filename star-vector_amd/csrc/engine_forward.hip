// Host driver, part 2 of 5: the op graphs -- vision tower, adapter, prompt pass, one decode step -- and the forward entry
// points of the C ABI (sv_encode_image, sv_adapter, sv_embed_tokens, sv_prefill, sv_forward_logits, sv_forward_logprobs, sv_forward_logprobs_ragged,
// sv_forward_logprobs_prefixed, sv_decode_step).  The prompt pass is two layer loops: prefill_forward (rectangular, B x S0 rows) and
// prefill_forward_packed (sequences of different lengths, ragged or behind shared prefixes, driven by the lists of one PackedPlan); the fragments that
// are the same in both -- attention arguments, GEMM arguments, last-row logits, the log-prob tail -- are functions in front of them.  Every scoring
// entry point with log-probs goes through one ScoreCall / check_score_call / score_pass.
#include <algorithm>
#include <cmath>
#include "engine_internal.h"

namespace sveng {
// record an event in front of the next launch (tagged with its kind); durations = event deltas
void prof_mark(sv_engine* e, int kind, hipStream_t st) {
    if (!e->prof_on) return;
    if (e->prof_used == e->prof_ev.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        e->prof_ev.push_back(ev);
        e->prof_kind.push_back(kind);
    }
    e->prof_kind[e->prof_used] = kind;
    (void)hipEventRecord(e->prof_ev[e->prof_used++], st);
}
}  // namespace sveng

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
// `kind`: the stage this GEMM belongs to in a time-to-first-token profile (sv_profile_ttft; prof_mark is a no-op otherwise); the
// remainder-row launch of a peeled GEMM is marked PK_GEMM_TAIL through the launcher's hook
static void tail_mark_cb(void* e, hipStream_t st) { prof_mark(static_cast<sv_engine*>(e), PK_GEMM_TAIL, st); }
// the stage mark and the arguments every engine GEMM shares: C [M][l.N] = act(A l.W + bias) + R, bf16 out
static GemmArgs gemm_args(sv_engine* e, int kind, const bf16_t* A, int lda, const Linear& l, const bf16_t* R, int ldr, void* C, int ldc, int M,
                          int act, hipStream_t st) {
    prof_mark(e, kind, st);
    GemmArgs g;
    if (e->prof_on) { g.tail_mark = tail_mark_cb; g.tail_ctx = e; }
    g.A = A; g.lda = lda; g.Wp = l.Wp; g.bias = l.bias; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc;
    g.M = M; g.N = l.N; g.K = l.Kpad; g.act = act; g.out_f32 = 0;
    g.cscale = l.wfmt == SV_WFMT_FP8 ? l.wscale : nullptr;
    return g;
}
// seq_rows: the M rows are whole sequences of that many rows (vision tokens of an image, prompt rows of a request): where gemm_seq_form holds
// the rows a sequence leaves over its 256-row tiles go through the split-K remainder kernel (gemm.hip); last_rows: the M rows are the LAST
// rows of such sequences (compact) and take the kernel they take inside the full problem
static void gemm(sv_engine* e, int kind, const bf16_t* A, int lda, const Linear& l, const bf16_t* R, int ldr, void* C, int ldc, int M,
                 int act, int out_f32, hipStream_t st, int seq_rows = 0, int last_rows = 0, int tune_in_place = 0) {
    GemmArgs g = gemm_args(e, kind, A, lda, l, R, ldr, C, ldc, M, act, st);
    g.out_f32 = out_f32;
    g.seq_rows = (e->exp & SV_EXP_BATCH_REMAINDER) ? 0 : seq_rows;          // A/B: the batch-level remainder of rounds 2-5
    g.splitk_rows = (e->exp & SV_EXP_BATCH_REMAINDER) ? 0 : last_rows;
    g.tune_in_place = tune_in_place;
    launch_gemm(g, st);
}
// the same GEMM over packed rows of sequences of different lengths: `rows` (device, n_rows of them) take the split-K remainder kernel (launch_gemm_ragged)
static void gemm_ragged(sv_engine* e, int kind, const bf16_t* A, int lda, const Linear& l, const bf16_t* R, int ldr, void* C, int ldc, int M,
                        int act, hipStream_t st, const int32_t* rows, int n_rows) {
    launch_gemm_ragged(gemm_args(e, kind, A, lda, l, R, ldr, C, ldc, M, act, st), rows, n_rows, e->rag_rsave, st);
}

// Context splits of the decode attention: a constant of the engine (sized for the engine's max_batch), NOT of the batch of the
// call, so that a sequence's partial results are merged in the same grouping whatever shares the batch with it: a row is
// bit-identical alone, inside a batch and inside a continuous batch at any context length.
int sveng::attn_max_splits_of(int max_batch, int nkv, int num_cus) {
    const int rows = (max_batch < 32 ? max_batch : 32) * nkv;
    const int ms = num_cus / (rows < 1 ? 1 : rows);
    return ms < 1 ? 1 : (ms > 8 ? 8 : ms);
}
static int attn_max_splits(const sv_engine* e) { return attn_max_splits_of(e->cfg.max_batch, e->nkv, e->num_cus); }

// 32-key groups a block takes before another context split joins.  Where the engine's rows x KV heads already give every CU a block
// (StarVector-8B at 64 rows: 256 (row, KV head) pairs), a context of <= 8 groups stays in ONE block (one group per wave: no partial
// results, no ticket, no merge); otherwise 4 (measured best where the splits are what fills the chip,
// profiles/attention_r03_groups_per_block_ab.log).  A constant of the engine like the split cap (same reason).
int sveng::attn_groups_per_block_of(int max_batch, int nkv, int num_cus) {
    return (max_batch < 64 ? max_batch : 64) * nkv >= num_cus ? 8 : 4;
}
static int attn_groups_per_block(const sv_engine* e) { return attn_groups_per_block_of(e->cfg.max_batch, e->nkv, e->num_cus); }

static int vision_forward(sv_engine* e, const bf16_t* img, int B, bf16_t* out, hipStream_t st) {
    const sv_config& c = e->cfg;
    const int Dv = c.vit_width, T = e->T, NP = e->NP, M = B * T, Fv = e->vit_F;
    const float eps = e->v2 ? c.vit_eps : c.ln_eps;
    const int act = e->v2 ? ACT_GELU_TANH : ACT_QUICKGELU;       // SigLIP gelu_pytorch_tanh | CLIP QuickGELU
    prof_mark(e, PK_VIT_ROWS, st);
    launch_im2col(img, e->patches, B, c.image_size, c.patch_size, e->conv1.Kpad, st);
    gemm(e, PK_VIT_GEMM, e->patches, e->conv1.Kpad, e->conv1, nullptr, 0, e->patch_out, Dv, B * NP, ACT_NONE, 0, st);
    prof_mark(e, PK_VIT_ROWS, st);
    if (e->v2)      // SigLIP: patches (+conv bias) + learned positions, no class token, no ln_pre
        launch_dec_embed(e->patch_out, e->pos, e->vx, B, NP, Dv, st);
    else
        launch_vit_embed_lnpre(e->patch_out, Dv, e->cls, e->pos, e->ln_pre.g, e->ln_pre.b, e->vx, B, NP, Dv,
                               c.ln_eps, st);
    AttnPrefillArgs at;
    at.q = e->vqkv; at.k = e->vqkv + Dv; at.v = e->vqkv + 2 * Dv;
    at.q_row_stride = 3 * Dv; at.kv_row_stride = 3 * Dv; at.q_head_stride = e->vdh; at.kv_head_stride = e->vdh;
    at.o = e->vattn; at.o_row_stride = Dv; at.B = B; at.S = T; at.H = c.vit_heads; at.head_dim = e->vdh;
    at.kv_group = 1; at.causal = 0; at.scale = 1.0f / sqrtf((float)e->vdh);
    for (int i = 0; i < c.vit_layers; ++i) {
        VitLayer& L = e->vit[i];
        prof_mark(e, PK_VIT_ROWS, st);
        launch_layernorm_rows(e->vx, Dv, L.ln1.g, L.ln1.b, e->vln, Dv, M, Dv, eps, st);
        gemm(e, PK_VIT_GEMM, e->vln, Dv, L.in_proj, nullptr, 0, e->vqkv, 3 * Dv, M, ACT_NONE, 0, st, T);
        prof_mark(e, PK_VIT_ATTN, st);
        launch_attn_prefill(at, st);
        gemm(e, PK_VIT_GEMM, e->vattn, Dv, L.out_proj, e->vx, Dv, e->vx, Dv, M, ACT_NONE, 0, st, T);
        prof_mark(e, PK_VIT_ROWS, st);
        launch_layernorm_rows(e->vx, Dv, L.ln2.g, L.ln2.b, e->vln, Dv, M, Dv, eps, st);
        gemm(e, PK_VIT_GEMM, e->vln, Dv, L.c_fc, nullptr, 0, e->vmlp, Fv, M, act, 0, st, T);
        gemm(e, PK_VIT_GEMM, e->vmlp, Fv, L.c_proj, e->vx, Dv, e->vx, Dv, M, ACT_NONE, 0, st, T);
    }
    prof_mark(e, PK_VIT_ROWS, st);
    launch_layernorm_rows(e->vx, Dv, e->ln_vision.g, e->ln_vision.b, out, Dv, M, Dv, eps, st);
    return 0;
}

// out_batch_stride (elements; 0 = T * D): image b's T visual rows go to out + b * stride, e.g. the head of its [S0][D] prompt block
static int adapter_forward(sv_engine* e, const bf16_t* in, int B, bf16_t* out, hipStream_t st, size_t out_batch_stride = 0) {
    const sv_config& c = e->cfg;
    const int Dv = c.vit_width, D = c.hidden, T = e->T, M = B * T;
    gemm(e, PK_AD_GEMM, in, Dv, e->ad_fc, nullptr, 0, e->a1, 2 * Dv, M, ACT_SWISH, 0, st, T);
    gemm(e, PK_AD_GEMM, e->a1, 2 * Dv, e->ad_proj, nullptr, 0, e->a2, D, M, ACT_NONE, 0, st, T);
    prof_mark(e, PK_AD_NORM, st);
    if (c.adapter_norm == SV_NORM_LAYER)
        launch_plane_layernorm(e->a2, e->ad_w, e->ad_b, out, B, T * D, c.ln_eps, st, out_batch_stride);
    else
        launch_token_batchnorm(e->a2, e->ad_w, e->ad_b, e->ad_rm, e->ad_rv, out, B, T, D, c.ln_eps, st, out_batch_stride);
    return 0;
}

static int ensure_prefill_ws(sv_engine* e, size_t rows) {
    if (rows <= e->pf_rows) return 0;
    const sv_config& c = e->cfg;
    const int D = c.hidden;
    // previous buffers stay in e->allocs (freed at destroy); growth is rare (max_batch * S0)
    SVCHECK(dalloc(e, &e->ph, rows * D));
    SVCHECK(dalloc(e, &e->pln, rows * D));
    // 128 zeroed rows in front of the c_attn output: the query tile of an extension pass that straddles a context's end reads up to q_tile - 1 Q rows
    // in front of a sequence's first own row (extend/extend.hip)
    SVCHECK(dalloc(e, &e->pqkv, (rows + 128) * (size_t)e->QKV));
    e->pqkv += (size_t)128 * e->QKV;
    SVCHECK(dalloc(e, &e->pattn, rows * D));
    SVCHECK(dalloc(e, &e->pmlp, rows * c.n_inner));
    e->pf_rows = rows;
    return 0;
}

void sveng::reset_free_pages(sv_engine* e) {
    e->free_pages.clear();
    for (int p = e->num_pages - 1; p >= 0; --p) e->free_pages.push_back(p);
}
// page allocator: hand every sequence the pages for its whole budget up front (the decode loop runs without host round-trips, so pages cannot be
// added mid-flight): lens[b] + extra tokens for sequence b (lens == nullptr: extra tokens each; extra < 0: the whole max_seq_len, as sv_prefill hands out)
int sveng::assign_pages_ragged(sv_engine* e, int B, const int32_t* lens, int extra, hipStream_t st) {
    reset_free_pages(e);
    e->ctx_known = false;
    // The table goes up from a PINNED host image without a stream synchronise (the pageable copy + hipStreamSynchronize of rounds 1-5 drained the
    // stream in front of every prompt pass: ~25 us of idle GPU on the way to the first token); the image is rewritten only after the upload
    // before it has completed (an event, normally long past).
    if (e->table_pending) { HIPCHECK(hipEventSynchronize(e->table_ev)); e->table_pending = false; }
    const size_t n = (size_t)e->cfg.max_batch * e->pages_per_seq;
    int32_t* table = e->h_table;
    memset(table, 0, n * sizeof(int32_t));
    for (int b = 0; b < B; ++b) {
        const int total = extra < 0 ? e->cfg.max_seq_len : (lens ? lens[b] : 0) + extra;
        const int need = (total + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS;
        if (need > e->pages_per_seq) return fail(SV_EINVAL, "sequence length %d exceeds max_seq_len %d", total, e->cfg.max_seq_len);
        for (int i = 0; i < need; ++i) {
            table[(size_t)b * e->pages_per_seq + i] = e->free_pages.back();
            e->free_pages.pop_back();
        }
    }
    HIPCHECK(hipMemcpyAsync(e->block_table, table, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(e->table_ev, st));
    e->table_pending = true;
    return 0;
}
int sveng::assign_pages(sv_engine* e, int B, int total_len, hipStream_t st) {
    // (a common length that does not fit is refused before the free list is touched)
    if ((total_len + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS > e->pages_per_seq)
        return fail(SV_EINVAL, "sequence length %d exceeds max_seq_len %d", total_len, e->cfg.max_seq_len);
    return assign_pages_ragged(e, B, nullptr, total_len, st);
}

// lm_head -> e->logits; xp holds ln_f(h) in fragment order
// The fused row-update + c_attn launch (rowops.hip) is on for this engine: then xp_a -- the LayerNorm output buffer its GEMM blocks poll --
// is touched ONLY with write-through stores / L1-bypassing loads (row role, the attention launch's and the lm_head launch's pattern
// stores, the GEMM role's polls), and ln_f's output lives in xp_f.  Invariant: behind every lm_head launch xp_a carries the pattern.
// (First form: a memset node at the head of the step + the prompt pass's ln_f through xp_a with plain stores -- NaN logits in the third
//  sv_generate call of bench.py: a stale line of the buffer in some XCD's L2.)
static bool rc_enabled(const sv_engine* e) {
    // the 6-launch layer (fold6: residual stream in fragment order) or the 7-launch layer of the wide model (row-major residual stream)
    const bool layer_ok = e->fold6 ? (e->fold_ready && !(e->exp & SV_EXP_NO_LN_FOLD)) : e->cfg.hidden > 2048;
    return layer_ok && e->rc_fused_ok && !(e->exp & SV_EXP_ROWLN_CATTN_OFF) && (e->cfg.exclusive_device || (e->exp & SV_EXP_ROWLN_CATTN_FORCE)) && !e->fused_off;
}
// the lm_head launch stores the pattern 16 bytes per thread from its first blocks: its grid must cover the buffer (a tiny-vocabulary
// configuration would arm only part of it: then layer 0 of the next step takes the two launches)
static bool lm_head_covers(const sv_engine* e, unsigned bytes) {
    return (size_t)(e->lm_head.Npad / 32 / 3) * 128 * 16 >= bytes;      // at least: three column tiles per block, two waves
}
static void lm_head_logits(sv_engine* e, int MT, const bf16_t* xp, hipStream_t st) {
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    if (rc_enabled(e) && MT == 1 && xp != e->xp_a) { a.poison = e->xp_a; a.poison_bytes = (unsigned)((size_t)(e->cfg.hidden / 16) * 1024); }
    e->xpa_armed = a.poison != nullptr && lm_head_covers(e, a.poison_bytes);
    a.xp = xp; a.Wp = e->lm_head.Wp; a.Wq = e->lm_head.Wq; a.wscale = e->lm_head.wscale; a.MT = MT;      // (mxfp4: the prompt pass runs the bf16 image, W4 stays null)
 a.Npad = e->lm_head.Npad; a.K = e->lm_head.Kpad;
    a.splitk = 1; a.out_mode = SK_OUT_F32; a.out_f32 = e->logits; a.ldo = e->Vpad; a.round_bf16 = 1;
    a.N = e->lm_head.N;
    a.col_tiles = e->lm_head.col_tiles;      // the engine's own plan: sv_debug_set_col_tiles never reaches an engine launch
    launch_gemm_skinny(a, st);
}

// scoring workspace for `rows` kept rows: [rows][D] hidden, [rows][D] ln_f, [rows][Vpad] logits -- the log-prob form keeps its logits in the chunk
// workspace instead
static int ensure_score_ws(sv_engine* e, size_t rows, bool with_logits) {
    const size_t need = rows * (size_t)e->cfg.hidden * 2 + (with_logits ? rows * (size_t)e->Vpad : 0);
    if (need > e->score_elems) {
        if (e->score_ws) (void)hipFree(e->score_ws);
        e->score_ws = nullptr; e->score_elems = 0;
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->score_ws), need * sizeof(bf16_t)));
        e->score_elems = need;
    }
    return 0;
}
// sv_forward_logprobs: the lm_head over the ln_f rows hn [rows][D], `chunk` rows at a time into a workspace that does not grow
// with rows x vocab, logprob_rows over each chunk while it is still in the last-level cache.  The logits underneath are the
// bits sv_forward_logits returns whatever the chunk size: this call hands the dispatch no sequence structure, so a chunk can
// only reach the tile kernels and the one-wave-per-tile kernel, which compute a row with the same MFMA, operand roles and
// ascending k (tests/test_gpu_ops.py::test_linear_big_m_kernels_agree_bitwise); the split-K remainder kernels with their own
// K order are never chosen here.  Chunks are multiples of 256 rows: the rows in front of a boundary are whole tiles.  For the
// same reason a row's outputs do not depend on the rows around it: the ragged scoring pass runs this loop over sum(keep) rows.
static int score_logprob_chunks(sv_engine* e, const bf16_t* hn, size_t rows, const ScoreLogprobs* lp, hipStream_t st) {
    const sv_config& c = e->cfg;
    const int D = c.hidden;
    const int chunk = e->score_chunk_rows > 0 ? e->score_chunk_rows : SV_SCORE_CHUNK_ROWS;
    if (e->score_chunk_alloc != chunk) {
        if (e->score_chunk_ws) (void)hipFree(e->score_chunk_ws);
        e->score_chunk_ws = nullptr; e->score_chunk_alloc = 0;
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->score_chunk_ws), (size_t)chunk * e->Vpad * sizeof(bf16_t) + 16));
        e->score_chunk_alloc = chunk;
    }
    if (lp->k > 0 && !lp->lse && e->score_lse_alloc < chunk) {     // the chunk's lse travels from logprob_rows to topk_rows through this
        if (e->score_lse_ws) (void)hipFree(e->score_lse_ws);
        e->score_lse_ws = nullptr; e->score_lse_alloc = 0;
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->score_lse_ws), (size_t)chunk * sizeof(float)));
        e->score_lse_alloc = chunk;
    }
    int32_t* flag = reinterpret_cast<int32_t*>(e->score_chunk_ws + (size_t)chunk * e->Vpad);
    fill_i32(flag, 0, 1, st);
    fill_i32(flag + 1, 0x7fffffff, 1, st);
    for (size_t r0 = 0; r0 < rows; r0 += (size_t)chunk) {
        const int n = (int)std::min<size_t>((size_t)chunk, rows - r0);
        gemm(e, PK_PF_GEMM, hn + r0 * D, D, e->lm_head, nullptr, 0, e->score_chunk_ws, e->Vpad, n, ACT_NONE, 0, st, 0, 0, 1);
        LogprobArgs a;
        a.logits = e->score_chunk_ws; a.ld = e->Vpad; a.V = c.vocab; a.R = n; a.inv_t = lp->inv_t;
        a.targets = lp->targets + r0;
        a.logprob = lp->logprob ? lp->logprob + r0 : nullptr; a.lse = lp->lse ? lp->lse + r0 : nullptr;
        a.entropy = lp->entropy ? lp->entropy + r0 : nullptr; a.argmax = lp->argmax ? lp->argmax + r0 : nullptr;
        a.bad = flag; a.row0 = (int)r0;
        if (lp->k > 0 && !a.lse) a.lse = e->score_lse_ws;
        prof_mark(e, PK_PF_ROWS, st);
        launch_logprob_rows(a, st);
        if (lp->k > 0) {                 // sv_forward_topk: the list and the rank from the same chunk, with the lse just written
            TopkRowsArgs tk;
            tk.logits = e->score_chunk_ws; tk.ld = e->Vpad; tk.V = c.vocab; tk.R = n; tk.targets = lp->targets + r0; tk.inv_t = lp->inv_t;
            tk.lse = a.lse; tk.k = lp->k; tk.ids = lp->topk_ids + r0 * (size_t)lp->k; tk.logprobs = lp->topk_logprobs + r0 * (size_t)lp->k;
            tk.rank = lp->rank ? lp->rank + r0 : nullptr;
            launch_topk_rows_bf16(tk, st);
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The prompt pass: two layer loops.  prefill_forward runs the rectangular pass over B x S0 rows with the launchers' arithmetic forms (seq_rows /
// last_rows, launch_kv_write_prefill, at.S); prefill_forward_packed runs packed sequences of different lengths -- ragged or with shared prefixes --
// from the lists of a PackedPlan.  What is identical in both is stated once, here.
// ------------------------------------------------------------------------------------------------
// the prompt-pass attention over the engine's fused q | k | v rows; the call site adds B / S or the ragged fields
static AttnPrefillArgs attn_prefill_args(const sv_engine* e) {
    const sv_config& c = e->cfg;
    const int dh = e->dh, QKV = e->QKV, nkv = e->nkv, QD = c.n_head * dh;      // QD: width of the query block (= hidden for both model families)
    AttnPrefillArgs at;
    at.q = e->pqkv; at.k = e->pqkv + QD; at.v = e->pqkv + QD + nkv * dh;
    at.q_row_stride = QKV; at.kv_row_stride = QKV; at.q_head_stride = dh; at.kv_head_stride = nkv > 1 ? dh : 0;
    at.o = e->pattn; at.o_row_stride = QD; at.B = 0; at.S = 0; at.H = c.n_head; at.head_dim = dh;
    at.kv_group = c.n_head / nkv; at.causal = 1; at.scale = 1.0f / sqrtf((float)dh);
    at.window = c.sliding_window > 0 ? c.sliding_window : 0;      // StarCoder2: also inside the prompt pass (prompts longer than the window)
    return at;
}
// only the last prompt row of every sequence feeds ln_f + lm_head (HF computes all rows; same result).  gathered: e->hl holds those rows already
// (the pruned last layer); otherwise they come from the residual stream -- rows S0 - 1 of B sequences of S0 rows, or by rag_seq
static void last_row_logits(sv_engine* e, int B, int S0, const int32_t* rag_seq, bool gathered, hipStream_t st) {
    const int D = e->cfg.hidden;
    prof_mark(e, PK_PF_ROWS, st);
    if (!gathered) launch_gather_last_rows(e->ph, e->hl, B, S0, D, st, rag_seq);
    launch_layernorm_rows_packed(e->hl, D, e->ln_f.g, e->ln_f.b, e->xp_f, B, D, e->cfg.ln_eps, st);
    prof_mark(e, PK_PF_LMHEAD, st);
    lm_head_logits(e, (B + 31) / 32, e->xp_f, st);
}
// the log-prob tail of every scoring pass: `rows` kept rows, gathered into the first half of score_ws, through ln_f and the chunked lm_head
static int score_kept_rows(sv_engine* e, size_t rows, const ScoreLogprobs* lp, hipStream_t st) {
    const int D = e->cfg.hidden;
    bf16_t* hn = e->score_ws + rows * D;
    launch_layernorm_rows(e->score_ws, D, e->ln_f.g, e->ln_f.b, hn, D, (int)rows, D, e->cfg.ln_eps, st);
    return score_logprob_chunks(e, hn, rows, lp, st);
}

// sv_set_prefill_chunk: a generate-tail prompt pass of more packed rows than the budget runs as extension passes.  (SV_EXP_BATCH_REMAINDER, the A/B
// arm whose remainder rows depend on the batch, has no per-sequence routing to keep: it stays one pass.)
static bool chunk_applies(const sv_engine* e, long long rows) {
    return e->prefill_chunk > 0 && rows > e->prefill_chunk && !(e->exp & SV_EXP_BATCH_REMAINDER);
}

int sveng::prefill_forward(sv_engine* e, const bf16_t* embeds, int B, int S0, hipStream_t st, int n_keep,
                           bf16_t* dev_scores, const int32_t* table, const ScoreLogprobs* lp) {
    if (!table) table = e->block_table;           // continuous batching prefills NEW requests through a table of their slots' pages
    e->ctx_known = false;
    if (n_keep == 0 && chunk_applies(e, (long long)B * S0)) {      // sv_set_prefill_chunk: the same bits from passes of at most that many rows
        const std::vector<int32_t> lens((size_t)B, S0);
        return prefill_chunked(e, embeds, B, lens.data(), table, st);
    }
    const sv_config& c = e->cfg;
    const int D = c.hidden, dh = e->dh, F = c.n_inner, M = B * S0, QKV = e->QKV, nkv = e->nkv;
    const int QD = c.n_head * dh;                      // width of the query block (= D for both model families)
    SVCHECK(ensure_prefill_ws(e, (size_t)M));
    ++e->prompt_passes;
    prof_mark(e, PK_PF_ROWS, st);
    if (e->v2)      // StarCoder2: no learned positions (rotary), hidden = inputs_embeds
        HIPCHECK(hipMemcpyAsync(e->ph, embeds, (size_t)M * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    else
        launch_dec_embed(embeds, e->wpe, e->ph, B, S0, D, st);
    AttnPrefillArgs at = attn_prefill_args(e);
    at.B = B; at.S = S0;
    // The LAST layer of a generation prompt pass (n_keep == 0) is only needed for (a) its K / V rows and (b) the residual stream of
    // the last prompt row, which alone feeds ln_f + lm_head.  So after its attention only the last row of every sequence goes on:
    // attention over the last query tile, then c_proj / ln_2 / c_fc / down-proj on B rows instead of B * S0 (HF computes all rows and
    // reads logits[:, -1]; a row's GEMM / attention result does not depend on the rows around it: bit-identical, test_gpu_e2e.py).
    // SV_EXP_NO_PRUNE_LAST = off (A/B).
    const bool prune_last = n_keep == 0 && S0 >= 2 && !(e->exp & SV_EXP_NO_PRUNE_LAST);
    // the last prompt row may be one of the rows its sequence leaves over its 256-row tiles: the launcher gives it the kernel it takes in the full layers
    for (int i = 0; i < c.n_layer; ++i) {
        DecLayer& L = e->dec[i];
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln1.g, L.ln1.b, e->pln, D, M, D, c.ln_eps, st);
        gemm(e, PK_PF_GEMM, e->pln, D, L.c_attn, nullptr, 0, e->pqkv, QKV, M, ACT_NONE, 0, st, S0);
        prof_mark(e, PK_PF_ATTN, st);                      // RoPE + KV scatter + flash attention
        if (e->v2) launch_rope_prefill(e->pqkv, QKV, M, S0, c.n_head + nkv, dh, e->rope_cos, e->rope_sin, st);
        for (int kh = 0; kh < nkv; ++kh)
            launch_kv_write_prefill(e->pqkv, QKV, QD + kh * dh, QD + nkv * dh + kh * dh,
                                    e->kv_pool + (size_t)i * e->layer_stride + (size_t)kh * e->kv_head_stride,
                                    table, e->pages_per_seq, B, S0, dh, st, e->kv_dtype);
        if (prune_last && i + 1 == c.n_layer) {
            at.last_rows = 1;
            launch_attn_prefill(at, st);
            at.last_rows = 0;
            // compact buffers inside the (now free) LayerNorm workspace: [B][QD] attention rows | [B][D] ln_2 rows; the MLP rows in pmlp
            bf16_t* pa_l = e->pln;
            bf16_t* ln_l = e->pln + (size_t)B * QD;
            prof_mark(e, PK_PF_ROWS, st);
            launch_gather_last_rows(e->pattn, pa_l, B, S0, QD, st);
            launch_gather_last_rows(e->ph, e->hl, B, S0, D, st);
            gemm(e, PK_PF_GEMM, pa_l, QD, L.c_proj, e->hl, D, e->hl, D, B, ACT_NONE, 0, st, S0, 1);
            prof_mark(e, PK_PF_ROWS, st);
            launch_layernorm_rows(e->hl, D, L.ln2.g, L.ln2.b, ln_l, D, B, D, c.ln_eps, st);
            gemm(e, PK_PF_GEMM, ln_l, D, L.c_fc, nullptr, 0, e->pmlp, F, B, ACT_GELU_TANH, 0, st, S0, 1);
            gemm(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->hl, D, e->hl, D, B, ACT_NONE, 0, st, S0, 1);
            last_row_logits(e, B, S0, nullptr, true, st);
            return 0;
        }
        launch_attn_prefill(at, st);
        gemm(e, PK_PF_GEMM, e->pattn, QD, L.c_proj, e->ph, D, e->ph, D, M, ACT_NONE, 0, st, S0);
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln2.g, L.ln2.b, e->pln, D, M, D, c.ln_eps, st);
        gemm(e, PK_PF_GEMM, e->pln, D, L.c_fc, nullptr, 0, e->pmlp, F, M, ACT_GELU_TANH, 0, st, S0);
        gemm(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->ph, D, e->ph, D, M, ACT_NONE, 0, st, S0);
    }
    if (n_keep > 0) {
        // scoring forward (starvector_arch.py:161-184): ln_f + lm_head over the last n_keep rows of every sequence, as one
        // big-M GEMM; bf16 logits like the reference's bf16 lm_head.  The GEMM writes rows of Vpad columns (the packed
        // weight's padding), the caller's tensor has `vocab` columns.
        const size_t rows = (size_t)B * n_keep;
        SVCHECK(ensure_score_ws(e, rows, !lp));
        bf16_t* hk = e->score_ws;
        prof_mark(e, PK_PF_ROWS, st);
        launch_gather_tail_rows(e->ph, hk, B, S0, n_keep, D, st);
        if (lp) {
            SVCHECK(score_kept_rows(e, rows, lp, st));
        } else {
            bf16_t* hn = hk + rows * D;
            bf16_t* lg = hn + rows * D;
            launch_layernorm_rows(hk, D, e->ln_f.g, e->ln_f.b, hn, D, (int)rows, D, c.ln_eps, st);
            gemm(e, PK_PF_GEMM, hn, D, e->lm_head, nullptr, 0, lg, e->Vpad, (int)rows, ACT_NONE, 0, st);
            HIPCHECK(hipMemcpy2DAsync(dev_scores, (size_t)c.vocab * sizeof(bf16_t), lg, (size_t)e->Vpad * sizeof(bf16_t),
                                      (size_t)c.vocab * sizeof(bf16_t), rows, hipMemcpyDeviceToDevice, st));
        }
    }
    last_row_logits(e, B, S0, nullptr, false, st);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The packed prompt pass, ragged form: B sequences of lengths lens[b], embeddings packed [sum(lens)][hidden], no padding row computed or stored.
// (The prefixed form and why its bits hold: prefix/prefix.hip.)  Contract: for every sequence the last-row logits and every K / V entry are BIT-IDENTICAL to the sequence alone through prefill_forward
// with S0 = lens[b].  Per stage: LayerNorm is per row; the GEMMs send a row to the split-K remainder kernel exactly when its solo run
// does (ragged_gemm_rows) and to an ascending-k kernel otherwise; the attention keeps query-tile and key-tile origins at the sequence's
// first row (ragged_blocks); positions, pages and slots come from the row's own sequence.
// ------------------------------------------------------------------------------------------------
// one projection's PL_ROWS pair
static void ragged_gemm_rows(const int32_t* lens, int B, int N, int K, int act, std::vector<int32_t>& rows, std::vector<int32_t>& last) {
    rows.clear(); last.clear();
    int r0 = 0;
    for (int b = 0; b < B; ++b) {
        const int S = lens[b], r = seq_peel_rows(S);
        if (r > 0 && gemm_seq_form(S, N, K, act)) {
            for (int j = S - r; j < S; ++j) rows.push_back(r0 + j);
            last.push_back(b);
        }
        r0 += S;
    }
}
void sveng::ragged_blocks(const int32_t* lens, int B, int tile, bool last_only, std::vector<int32_t>& out) {
    out.clear();
    for (int b = 0; b < B; ++b) {
        const int n = (lens[b] + tile - 1) / tile;
        for (int t = last_only ? n - 1 : 0; t < n; ++t) { out.push_back(b); out.push_back(t); }
    }
}
int sveng::ragged_check_lens(const sv_engine* e, const int32_t* lens, int B, const char* who, int* max_len, long long* total) {
    int mx = 0;
    long long sum = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > e->cfg.max_seq_len)
            return fail(SV_EINVAL, "%s: length %d of sequence %d out of range (1..max_seq_len %d)", who, lens[b], b, e->cfg.max_seq_len);
        mx = lens[b] > mx ? lens[b] : mx;
        sum += lens[b];
    }
    if (max_len) *max_len = mx;
    if (total) *total = sum;
    return 0;
}

// the row-position buffer and the plan image (pinned host + device) of the ragged passes, grown on demand
static int rag_reserve_row_pos(sv_engine* e, size_t rows) {
    if (rows <= e->rag_pos_rows) return 0;
    if (e->rag_row_pos) (void)hipFree(e->rag_row_pos);
    e->rag_row_pos = nullptr; e->rag_pos_rows = 0;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->rag_row_pos), rows * sizeof(int32_t)));
    e->rag_pos_rows = rows;
    return 0;
}
static int rag_reserve_plan(sv_engine* e, size_t need) {
    if (need > e->rag_cap) {
        if (e->rag_pending) { HIPCHECK(hipEventSynchronize(e->rag_ev)); e->rag_pending = false; }
        if (e->h_rag) (void)hipHostFree(e->h_rag);
        if (e->d_rag) (void)hipFree(e->d_rag);
        e->h_rag = nullptr; e->d_rag = nullptr; e->rag_cap = 0;
        const size_t cap = need + need / 2 + 256;
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_rag), cap * sizeof(int32_t), hipHostMallocDefault));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->d_rag), cap * sizeof(int32_t)));
        if (!e->rag_ev) HIPCHECK(hipEventCreateWithFlags(&e->rag_ev, hipEventDisableTiming));
        e->rag_cap = cap;
    }
    // pinned image, no stream synchronise: rewritten only after its last upload has completed (an event, normally long past)
    if (e->rag_pending) { HIPCHECK(hipEventSynchronize(e->rag_ev)); e->rag_pending = false; }
    return 0;
}

__global__ void ragged_positions_kernel(int32_t* positions, const int32_t* rag_seq, int n, int rep, int delta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) positions[i] = rag_seq[2 * (i / rep) + 1] + delta;
}
void sveng::ragged_positions(sv_engine* e, int B, int rep, int delta, hipStream_t st) {
    launch_ragged_positions(e->positions, e->d_rag, B * rep, rep, delta, st);
}
void sveng::launch_ragged_positions(int32_t* positions, const int32_t* rag_seq, int n, int rep, int delta, hipStream_t st) {
    ragged_positions_kernel<<<(n + 63) / 64, 64, 0, st>>>(positions, rag_seq, n, rep, delta);
}

void sveng::ragged_plan(const int32_t* lens, int B, int q_tile, const PlanProj* proj, int n_proj, const int32_t* keep, PackedPlan& out) {
    out = PackedPlan();
    out.B = B; out.tail = keep ? PackedPlan::SCORE_TAIL_ROWS : PackedPlan::GENERATE;
    int r0 = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t d[4] = {r0, lens[b], keep ? keep[b] : 0, out.kept};
        out.list[PL_DESC].insert(out.list[PL_DESC].end(), d, d + 2);
        if (keep) { out.list[PL_KEPT].insert(out.list[PL_KEPT].end(), d, d + 4); out.kept += keep[b]; }
        r0 += lens[b];
    }
    out.M = out.src_rows[0] = r0;
    ragged_blocks(lens, B, q_tile, false, out.list[PL_BLOCKS0]);
    if (!keep) ragged_blocks(lens, B, q_tile, true, out.list[PL_LAST_TILES]);
    ragged_blocks(lens, B, 32, false, out.list[PL_KV_BLOCKS]);
    for (int i = 0; i < n_proj; ++i) ragged_gemm_rows(lens, B, proj[i].N, proj[i].K, proj[i].act, out.rows(i), out.last(i));
}
// the decoder's four projections as a plan builder asks for them (every layer has the same shapes); returns how many of them get per-sequence
// remainder rows: none under SV_EXP_BATCH_REMAINDER (as in the rectangular pass: nothing to list and, with prefixes, nothing to refuse)
static int plan_proj(const sv_engine* e, PlanProj pj[4]) {
    const DecLayer& L = e->dec[0];
    pj[0] = {L.c_attn.N, L.c_attn.Kpad, ACT_NONE}; pj[1] = {L.c_proj.N, L.c_proj.Kpad, ACT_NONE};
    pj[2] = {L.c_fc.N, L.c_fc.Kpad, ACT_GELU_TANH}; pj[3] = {L.c_proj2.N, L.c_proj2.Kpad, ACT_NONE};
    return (e->exp & SV_EXP_BATCH_REMAINDER) ? 0 : 4;
}
// every list of the plan, concatenated in list order into the pinned image, in one upload; off[i] = where list i begins in d_rag
static int rag_upload_lists(sv_engine* e, const std::vector<int32_t>* list, int n, size_t* off, hipStream_t st) {
    size_t need = 0;
    for (int i = 0; i < n; ++i) { off[i] = need; need += list[i].size(); }
    SVCHECK(rag_reserve_plan(e, need));
    for (int i = 0; i < n; ++i)
        if (!list[i].empty()) memcpy(e->h_rag + off[i], list[i].data(), list[i].size() * sizeof(int32_t));
    HIPCHECK(hipMemcpyAsync(e->d_rag, e->h_rag, need * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(e->rag_ev, st));
    e->rag_pending = true;
    return 0;
}
static int rag_upload_plan(sv_engine* e, const PackedPlan& p, size_t off[PL_COUNT], hipStream_t st) { return rag_upload_lists(e, p.list, PL_COUNT, off, st); }

// The packed pass over p.M rows.  A scoring tail (lp) runs the last layer on all packed rows with the per-sequence remainder rows of the layers in
// front -- a solo scoring pass never prunes it either --, gathers the kept rows into [p.kept][D] and sends them through ln_f and the chunked lm_head +
// logprob_rows (+ topk_rows) of the rectangular pass.  With prefixes the attention runs as two launches (the prefixes as ordinary ragged sequences,
// then the prefixed form over the sequences' tiles from the straddling one on); the prefix rows' c_proj / MLP work in the last layer is not skipped.
int sveng::prefill_forward_packed(sv_engine* e, const PackedPlan& p, const int32_t* table, const ScoreLogprobs* lp, hipStream_t st) {
    if (!table) table = e->block_table;
    e->ctx_known = false;
    const sv_config& c = e->cfg;
    const int D = c.hidden, dh = e->dh, F = c.n_inner, QKV = e->QKV, nkv = e->nkv;
    const int QD = c.n_head * dh, M = p.M, B = p.B;
    // (the pruned last layer keeps [B][QD] + [B][D] compact rows inside the LayerNorm workspace: at least 2 B rows)
    SVCHECK(ensure_prefill_ws(e, (size_t)std::max(M, 2 * B)));
    ++e->prompt_passes;
    if (!e->rag_rsave) SVCHECK(dalloc(e, &e->rag_rsave, (size_t)3 * c.max_batch * D));
    SVCHECK(rag_reserve_row_pos(e, (size_t)M));
    size_t off[PL_COUNT];
    SVCHECK(rag_upload_plan(e, p, off, st));
    const auto dev = [&](int i) -> const int32_t* { return e->d_rag + off[i]; };
    const auto len = [&](int i) { return (int)p.list[i].size(); };
    const int32_t* d_desc = dev(PL_DESC);

    prof_mark(e, PK_PF_ROWS, st);
    // a row's position is its index in its solo sequence: learned positions (v1) and RoPE (v2).  (Every form keeps the launch order it has always
    // had: the ragged v2 pass copies its rows first.)
    const auto row_pos = [&] {
        if (p.n_seg > 0) launch_prefix_row_pos(d_desc, p.n_seg, e->rag_row_pos, st);
        else launch_ragged_row_pos(d_desc, B, e->rag_row_pos, st);
    };
    const bool pos_first = !e->v2 || p.n_seg > 0;
    if (pos_first) row_pos();
    for (int s = 0, r = 0; s < 2 && p.src_rows[s] > 0; r += p.src_rows[s++]) {
        if (e->v2)      // StarCoder2: no learned positions (rotary), hidden = inputs_embeds
            HIPCHECK(hipMemcpyAsync(e->ph + (size_t)r * D, p.src[s], (size_t)p.src_rows[s] * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
        else
            launch_dec_embed(p.src[s], e->wpe, e->ph + (size_t)r * D, 1, p.src_rows[s], D, st, e->rag_row_pos + r);
    }
    if (!pos_first) row_pos();
    AttnPrefillArgs at = attn_prefill_args(e);
    at.B = B;
    const bool prune_last = p.tail == PackedPlan::GENERATE && !(e->exp & SV_EXP_NO_PRUNE_LAST);
    for (int i = 0; i < c.n_layer; ++i) {
        DecLayer& L = e->dec[i];
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln1.g, L.ln1.b, e->pln, D, M, D, c.ln_eps, st);
        gemm_ragged(e, PK_PF_GEMM, e->pln, D, L.c_attn, nullptr, 0, e->pqkv, QKV, M, ACT_NONE, st, dev(pl_rows(0)), len(pl_rows(0)));
        prof_mark(e, PK_PF_ATTN, st);
        if (e->v2) launch_rope_prefill(e->pqkv, QKV, M, M, c.n_head + nkv, dh, e->rope_cos, e->rope_sin, st, e->rag_row_pos);
        for (int kh = 0; kh < (len(PL_KV_BLOCKS) > 0 ? nkv : 0); ++kh)      // (no blocks: the pass writes no page)
            launch_kv_write_prefill_ragged(e->pqkv, QKV, QD + kh * dh, QD + nkv * dh + kh * dh,
                                           e->kv_pool + (size_t)i * e->layer_stride + (size_t)kh * e->kv_head_stride,
                                           table, e->pages_per_seq, d_desc, dev(PL_KV_BLOCKS), len(PL_KV_BLOCKS) / 2, dh, st, e->kv_dtype);
        if (prune_last && i + 1 == c.n_layer) {
            // only the last row of every sequence goes on (see prefill_forward): its query tile, then B compact rows
            at.rag_seq = d_desc; at.rag_blocks = dev(PL_LAST_TILES); at.rag_nblocks = len(PL_LAST_TILES) / 2;
            launch_attn_prefill(at, st);
            bf16_t* pa_l = e->pln;
            bf16_t* ln_l = e->pln + (size_t)B * QD;
            prof_mark(e, PK_PF_ROWS, st);
            launch_gather_last_rows(e->pattn, pa_l, B, 0, QD, st, d_desc);
            launch_gather_last_rows(e->ph, e->hl, B, 0, D, st, d_desc);
            gemm_ragged(e, PK_PF_GEMM, pa_l, QD, L.c_proj, e->hl, D, e->hl, D, B, ACT_NONE, st, dev(pl_last(1)), len(pl_last(1)));
            prof_mark(e, PK_PF_ROWS, st);
            launch_layernorm_rows(e->hl, D, L.ln2.g, L.ln2.b, ln_l, D, B, D, c.ln_eps, st);
            gemm_ragged(e, PK_PF_GEMM, ln_l, D, L.c_fc, nullptr, 0, e->pmlp, F, B, ACT_GELU_TANH, st, dev(pl_last(2)), len(pl_last(2)));
            gemm_ragged(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->hl, D, e->hl, D, B, ACT_NONE, st, dev(pl_last(3)), len(pl_last(3)));
            last_row_logits(e, B, 0, d_desc, true, st);
            return 0;
        }
        for (int j = 0; j < p.n_attn; ++j) {
            const int seq = PL_SEQ0 + 2 * j, blocks = PL_BLOCKS0 + 2 * j;
            at.rag_prefixed = j; at.rag_seq = len(seq) > 0 ? dev(seq) : d_desc; at.rag_blocks = dev(blocks); at.rag_nblocks = len(blocks) / 2;
            launch_attn_prefill(at, st);
        }
        gemm_ragged(e, PK_PF_GEMM, e->pattn, QD, L.c_proj, e->ph, D, e->ph, D, M, ACT_NONE, st, dev(pl_rows(1)), len(pl_rows(1)));
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln2.g, L.ln2.b, e->pln, D, M, D, c.ln_eps, st);
        gemm_ragged(e, PK_PF_GEMM, e->pln, D, L.c_fc, nullptr, 0, e->pmlp, F, M, ACT_GELU_TANH, st, dev(pl_rows(2)), len(pl_rows(2)));
        gemm_ragged(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->ph, D, e->ph, D, M, ACT_NONE, st, dev(pl_rows(3)), len(pl_rows(3)));
    }
    if (p.tail != PackedPlan::GENERATE) {
        SVCHECK(ensure_score_ws(e, (size_t)p.kept, false));
        prof_mark(e, PK_PF_ROWS, st);
        if (p.tail == PackedPlan::SCORE_TAIL_ROWS)
            launch_gather_tail_rows(e->ph, e->score_ws, B, 0, 0, D, st, dev(PL_KEPT), p.kept);
        else      // (keep = len + 1: the prefix's last row, then the own rows -- not contiguous)
            launch_gather_listed_rows(e->ph, D, dev(PL_KEPT), p.kept, e->score_ws, D, st);
        SVCHECK(score_kept_rows(e, (size_t)p.kept, lp, st));
        if (p.tail == PackedPlan::SCORE_LISTED_ROWS) return 0;
    }
    last_row_logits(e, B, 0, d_desc, false, st);
    return 0;
}

int sveng::prefill_forward_ragged(sv_engine* e, const bf16_t* embeds, int B, const int32_t* lens, hipStream_t st, const int32_t* table,
                                  const int32_t* keep, const ScoreLogprobs* lp) {
    if (!keep) {
        long long rows = 0;
        for (int b = 0; b < B; ++b) rows += lens[b];
        if (chunk_applies(e, rows)) return prefill_chunked(e, embeds, B, lens, table ? table : e->block_table, st);
    }
    PlanProj pj[4];
    const int n_proj = plan_proj(e, pj);
    PackedPlan p;
    ragged_plan(lens, B, attn_prefill_q_tile(e->cfg.n_head, e->nkv), pj, n_proj, keep, p);
    p.src[0] = embeds;
    return prefill_forward_packed(e, p, table, lp, st);
}

// ------------------------------------------------------------------------------------------------
// The extension pass: own rows behind a cached context (the plan and why the bits hold: extend/extend.hip)
// ------------------------------------------------------------------------------------------------
ExtKvArgs sveng::extend_kv_args(sv_engine* e, int layer, const int32_t* table, const int32_t* xseq, const int32_t* blocks, int n_blocks, bf16_t* gkv) {
    const int dh = e->dh, nkv = e->nkv, QD = e->cfg.n_head * dh;
    ExtKvArgs a;
    a.qkv = e->pqkv; a.row_stride = e->QKV; a.k_off = QD; a.v_off = QD + nkv * dh;
    a.pool_layer = e->kv_pool + (size_t)layer * e->layer_stride; a.kv_head_stride = e->kv_head_stride; a.table = table; a.max_pages = e->pages_per_seq;
    a.xseq = xseq; a.blocks = blocks; a.n_blocks = n_blocks; a.head_dim = dh; a.n_kv = nkv; a.kv_fmt = e->kv_dtype;
    a.gkv = gkv; a.gkv_stride = 2 * nkv * dh;
    return a;
}

// the K | V rows of the sequences with a context: the one buffer of an extension pass that grows with the context (hipFree waits for the launches
// that still read the old one)
static int reserve_gkv(sv_engine* e, size_t rows) {
    if (rows <= e->gkv_rows) return 0;
    if (e->gkv) (void)hipFree(e->gkv);
    e->gkv = nullptr; e->gkv_rows = 0;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->gkv), rows * 2 * e->nkv * e->dh * sizeof(bf16_t)));
    e->gkv_rows = rows;
    return 0;
}

int sveng::extend_forward(sv_engine* e, ExtendPass& p, const bf16_t* embeds, const int32_t* table, hipStream_t st) {
    if (!table) table = e->block_table;
    const sv_config& c = e->cfg;
    const int D = c.hidden, dh = e->dh, F = c.n_inner, QKV = e->QKV, nkv = e->nkv;
    const int QD = c.n_head * dh, M = p.M, NF = (int)p.fin.size(), KW = 2 * nkv * dh;
    SVCHECK(ensure_prefill_ws(e, (size_t)std::max(M, 2 * NF)));
    SVCHECK(reserve_gkv(e, (size_t)p.gkv_rows));
    ++e->prompt_passes;
    if (!e->rag_rsave) SVCHECK(dalloc(e, &e->rag_rsave, (size_t)3 * c.max_batch * D));
    SVCHECK(rag_reserve_row_pos(e, (size_t)M));
    size_t off[XL_COUNT];
    SVCHECK(rag_upload_lists(e, p.list, XL_COUNT, off, st));
    const auto dev = [&](int i) -> const int32_t* { return e->d_rag + off[i]; };
    const auto len = [&](int i) { return (int)p.list[i].size(); };
    const auto rows = [&](int i) { return XL_ROWS + 2 * i; };
    const auto last = [&](int i) { return XL_ROWS + 2 * i + 1; };

    prof_mark(e, PK_PF_ROWS, st);
    launch_prefix_row_pos(dev(XL_SEG), len(XL_SEG) / 3, e->rag_row_pos, st);      // a row's position is its solo index ctx + j
    if (e->v2) HIPCHECK(hipMemcpyAsync(e->ph, embeds, (size_t)M * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    else launch_dec_embed(embeds, e->wpe, e->ph, 1, M, D, st, e->rag_row_pos);
    AttnPrefillArgs at = attn_prefill_args(e);
    // the attention of the sequences with a context: one prefixed launch each over {0, tile} entries, K | V from the sequence's region of gkv -- the
    // kernel's row index of solo index s is (R - ctx) + s, so the region's row 0 lies at index R - ctx
    const auto attn_ctx = [&](bool last_only) {
        AttnPrefillArgs ac = at;
        ac.rag_prefixed = 1; ac.kv_row_stride = KW; ac.kv_head_stride = nkv > 1 ? dh : 0;
        for (const ExtendPass::CtxSeq& cs : p.ctx_seqs) {
            if (last_only && !cs.fin) continue;
            const bf16_t* kb = e->gkv + ((long long)cs.region - cs.index_row0) * KW;
            ac.k = kb; ac.v = kb + nkv * dh;
            ac.rag_seq = dev(XL_CTX_SEQ) + cs.seq_off;
            ac.rag_blocks = dev(XL_CTX_BLOCKS) + cs.blocks_off + (last_only ? 2 * (cs.n_blocks - 1) : 0);
            ac.rag_nblocks = last_only ? 1 : cs.n_blocks;
            launch_attn_prefill(ac, st);
        }
    };
    for (int i = 0; i < c.n_layer; ++i) {
        DecLayer& L = e->dec[i];
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln1.g, L.ln1.b, e->pln, D, M, D, c.ln_eps, st);
        gemm_ragged(e, PK_PF_GEMM, e->pln, D, L.c_attn, nullptr, 0, e->pqkv, QKV, M, ACT_NONE, st, dev(rows(0)), len(rows(0)));
        prof_mark(e, PK_PF_ATTN, st);
        if (e->v2) launch_rope_prefill(e->pqkv, QKV, M, M, c.n_head + nkv, dh, e->rope_cos, e->rope_sin, st, e->rag_row_pos);
        launch_kv_write_extend(extend_kv_args(e, i, table, dev(XL_XSEQ), dev(XL_WRITE), len(XL_WRITE) / 2, e->gkv), st);
        const bool last_layer = i + 1 == c.n_layer;
        if (last_layer && NF == 0) break;      // no sequence reaches its total: the last layer owes its K / V rows and nothing else
        launch_kv_gather(extend_kv_args(e, i, table, dev(XL_XSEQ), dev(XL_GATHER), len(XL_GATHER) / 2, e->gkv), st);
        at.rag_prefixed = 0; at.rag_seq = dev(XL_PLAIN_SEQ);
        if (last_layer) {
            // only the last row of every finishing sequence goes on (see prefill_forward): its query tile, then NF compact rows
            at.rag_blocks = dev(XL_PLAIN_LAST); at.rag_nblocks = len(XL_PLAIN_LAST) / 2;
            launch_attn_prefill(at, st);
            attn_ctx(true);
            const int32_t* d_fin = dev(XL_FIN);
            bf16_t* pa_l = e->pln;
            bf16_t* ln_l = e->pln + (size_t)NF * QD;
            prof_mark(e, PK_PF_ROWS, st);
            launch_gather_last_rows(e->pattn, pa_l, NF, 0, QD, st, d_fin);
            launch_gather_last_rows(e->ph, e->hl, NF, 0, D, st, d_fin);
            gemm_ragged(e, PK_PF_GEMM, pa_l, QD, L.c_proj, e->hl, D, e->hl, D, NF, ACT_NONE, st, dev(last(1)), len(last(1)));
            prof_mark(e, PK_PF_ROWS, st);
            launch_layernorm_rows(e->hl, D, L.ln2.g, L.ln2.b, ln_l, D, NF, D, c.ln_eps, st);
            gemm_ragged(e, PK_PF_GEMM, ln_l, D, L.c_fc, nullptr, 0, e->pmlp, F, NF, ACT_GELU_TANH, st, dev(last(2)), len(last(2)));
            gemm_ragged(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->hl, D, e->hl, D, NF, ACT_NONE, st, dev(last(3)), len(last(3)));
            last_row_logits(e, NF, 0, d_fin, true, st);
            return 0;
        }
        at.rag_blocks = dev(XL_PLAIN_BLOCKS); at.rag_nblocks = len(XL_PLAIN_BLOCKS) / 2;
        launch_attn_prefill(at, st);
        attn_ctx(false);
        gemm_ragged(e, PK_PF_GEMM, e->pattn, QD, L.c_proj, e->ph, D, e->ph, D, M, ACT_NONE, st, dev(rows(1)), len(rows(1)));
        prof_mark(e, PK_PF_ROWS, st);
        launch_layernorm_rows(e->ph, D, L.ln2.g, L.ln2.b, e->pln, D, M, D, c.ln_eps, st);
        gemm_ragged(e, PK_PF_GEMM, e->pln, D, L.c_fc, nullptr, 0, e->pmlp, F, M, ACT_GELU_TANH, st, dev(rows(2)), len(rows(2)));
        gemm_ragged(e, PK_PF_GEMM, e->pmlp, F, L.c_proj2, e->ph, D, e->ph, D, M, ACT_NONE, st, dev(rows(3)), len(rows(3)));
    }
    e->xpa_armed = false;                       // no lm_head launch in front of the step that follows
    return 0;
}

int sveng::prefill_chunked(sv_engine* e, const bf16_t* embeds, int B, const int32_t* lens, const int32_t* table, hipStream_t st, const int32_t* ctx0) {
    PlanProj pj[4];
    const int n_proj = plan_proj(e, pj), q_tile = attn_prefill_q_tile(e->cfg.n_head, e->nkv), D = e->cfg.hidden;
    // the own rows of every sequence: all of it, or what lies behind its cached context (ctx0: the prefix cache's reused pages)
    std::vector<int32_t> own(lens, lens + B), desc, at((size_t)B, 0);
    long long rows = 0;
    size_t region = 0;
    int longest = 0;
    for (int b = 0, r0 = 0; b < B; r0 += own[b++]) {
        if (ctx0) { own[b] -= ctx0[b]; at[b] = ctx0[b]; if (ctx0[b] > 0) region += (size_t)lens[b]; }
        desc.push_back(r0); desc.push_back(lens[b]); longest = std::max(longest, lens[b]); rows += own[b];
    }
    std::vector<std::vector<int32_t>> take;
    extend_schedule(own.data(), B, chunk_applies(e, rows) ? e->prefill_chunk : 0, take);
    const bool stash = take.size() > 1;        // one pass: every sequence finishes in it, compact row i is sequence i
    if (stash && !e->logit_stash) SVCHECK(dalloc(e, &e->logit_stash, (size_t)e->cfg.max_batch * e->Vpad, false));
    SVCHECK(reserve_gkv(e, region + (size_t)longest));      // (a pass continues the sequences that came with a context and at most one more: the one the pass in front cut)
    size_t row0 = 0;
    std::vector<ExtendSeq> seqs((size_t)B);
    for (size_t k = 0; k < take.size(); ++k) {
        for (int b = 0; b < B; ++b) seqs[b] = {at[b], take[k][b], lens[b]};
        ExtendPass p;
        extend_plan(seqs.data(), B, q_tile, pj, n_proj, p);
        p.list[XL_DESC] = desc;
        SVCHECK(extend_forward(e, p, embeds + row0 * D, table, st));
        for (size_t i = 0; stash && i < p.fin.size(); ++i)
            HIPCHECK(hipMemcpyAsync(e->logit_stash + (size_t)p.fin[i] * e->Vpad, e->logits + i * e->Vpad, (size_t)e->Vpad * sizeof(float),
                                    hipMemcpyDeviceToDevice, st));
        row0 += (size_t)p.M;
        for (int b = 0; b < B; ++b) at[b] += take[k][b];
    }
    if (stash) HIPCHECK(hipMemcpyAsync(e->logits, e->logit_stash, (size_t)B * e->Vpad * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

// Arguments of the decode attention of layer `layer` over the engine's KV pool / block table / positions: the c_attn output
// arrives as `splitk` fp32 slabs `ws` (+ bias, summed by the kernel), the result goes to `out_xp` in fragment order.
void sveng::attn_decode_args(sv_engine* e, int layer, int B, const float* ws, int splitk, const bf16_t* bias, bf16_t* out_xp,
                             AttnDecodeArgs& ad) {
    const sv_config& c = e->cfg;
    const int MT = (B + 31) / 32;
    memset(&ad, 0, sizeof(ad));
    ad.ws = ws; ad.splitk = splitk; ad.ldws = e->ldws; ad.rows_ws = MT * 32; ad.bias = bias;
    ad.pool_layer = e->kv_pool + (size_t)layer * e->layer_stride; ad.block_table = e->block_table;
    ad.max_pages = e->pages_per_seq; ad.positions = e->positions; ad.out_xp = out_xp; ad.out_KS = c.n_head * e->dh / 16;
    ad.window = c.sliding_window;
    ad.B = B; ad.H = c.n_head; ad.head_dim = e->dh; ad.scale = 1.0f / sqrtf((float)e->dh);
    ad.part = e->attn_part; ad.counters = e->attn_cnt;
    ad.max_splits = attn_max_splits(e);
    ad.groups_per_block = attn_groups_per_block(e);
    ad.n_kv = e->nkv; ad.kv_head_stride = e->kv_head_stride; ad.rope_cos = e->rope_cos; ad.rope_sin = e->rope_sin;
    ad.kv_fmt = e->kv_dtype;
}

// the K / V pre-write of a verification step (lookup/lookup.hip) over exactly what the attention launch `ad` reads
LookupKvArgs sveng::lookup_kv_args(const AttnDecodeArgs& ad) {
    LookupKvArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.ws = ad.ws; ka.splitk = ad.splitk; ka.ldws = ad.ldws; ka.rows_ws = ad.rows_ws; ka.bias = ad.bias;
    ka.pool_layer = ad.pool_layer; ka.block_table = ad.block_table; ka.max_pages = ad.max_pages; ka.positions = ad.positions;
    ka.rows = ad.B; ka.H = ad.H; ka.head_dim = ad.head_dim; ka.n_kv = ad.n_kv; ka.kv_head_stride = ad.kv_head_stride;
    ka.rope_cos = ad.rope_cos; ka.rope_sin = ad.rope_sin;
    return ka;
}

// One autoregressive step: consumes cur_tok / positions, leaves logits in e->logits.  6 launches per layer + 2 (bf16 weights,
// <= 32 rows):
//   row update (embedding | + bias + residual of the previous down-proj, LN1) | c_attn -> fp32 slabs | attention (sums the
//   slabs, + bias) | c_proj over the whole K: h += ..., partial row statistics | c_fc on the raw h (ln_2 folded, bias + GELU
//   epilogue) | down-proj -> slabs ... | row update (ln_f) | lm_head
// fp8 weights / more than one row tile: 7 launches per layer (c_proj -> slabs | row update (+ bias, + residual, LN2) | c_fc).
void sveng::decode_forward(sv_engine* e, int B, hipStream_t st) {
    const sv_config& c = e->cfg;
    const int D = c.hidden, dh = e->dh, F = c.n_inner, MT = (B + 31) / 32;
    // slab double buffer: A = c_attn slabs (read by attention); B = c_proj / down-proj slabs (read by the row update)
    float* wsA = e->ws;
    float* wsB = e->ws2;
    RowUpdateArgs ru;
    memset(&ru, 0, sizeof(ru));
    const bool fold6 = e->fold6 && e->fold_ready && !(e->exp & SV_EXP_NO_LN_FOLD);
    // Row update + c_attn as ONE launch (rowops.hip rowln_cattn_kernel): on when the engine owns its GPU (like the fused MLP launch: its
    // blocks wait for blocks of the same launch); SV_EXP_ROWLN_CATTN_OFF = off, SV_EXP_ROWLN_CATTN_FORCE = on without exclusive_device (A/B).  The GEMM blocks
    // recognise unwritten activations by the 0xFFFF'FFFF pattern: xp_a gets it from the lm_head launch of the step (or prompt pass) before
    // (layer 0) and from the attention launch of layer i for layer i + 1 -- which must have room for it: 16 bytes per thread of its grid
    // (B >= 10 at StarVector-1B's shapes).  Not inside the profiling legs (they time the row updates and the GEMMs apart).  A call that
    // cannot fuse on an engine that does (see rc_enabled) keeps its LayerNorm outputs out of xp_a.
    const size_t attn_threads_bytes = (size_t)B * e->nkv * attn_max_splits(e) * 512 * 16;
    const bool mlp_pattern = fold6 && e->mlp_fused_ok;          // the attention launch may also have to arm the fused MLP launch's buffer
    // (xpa_armed: the launch that arms layer 0's buffer really ran in front of this step -- not after sv_create, sv_debug_set_exp or
    //  sv_debug_kv_load, whose first step takes the two launches and arms the next one)
    // (round 6, third session: a batch below 10 rows has an attention grid too small for the patterns -- B * 8 splits * 512 threads * 16 bytes -- and ran
    //  the two launches, 123 launches per step instead of 99: slower at batch 1 than at batch 16.  On the 6-launch layer the attention output projection,
    //  256 blocks of 1024 threads whatever the batch, arms the buffers instead: ColsArgs::poison / ::poison2)
    const bool attn_room = (size_t)(D / 16) * 1024 + (mlp_pattern ? (size_t)(F / 16) * 1024 : 0u) <= attn_threads_bytes;
    const bool rc = rc_enabled(e) && e->xpa_armed && MT == 1 && !e->only_skinny && !e->skip_skinny && !e->prof_on && (attn_room || fold6);
    const unsigned xpa_bytes = (unsigned)((size_t)(D / 16) * 1024);
    e->step_rc = false; e->step_mlp = false; e->step_sel = e->greedy_fused;
    bf16_t* const xp_ln = (rc_enabled(e) && !rc) ? e->xp_f : e->xp_a;      // LayerNorm(ln_1) output = the c_attn operand

    ru.h = fold6 ? e->h_xp : e->h_dec; ru.ldh = fold6 ? 0 : D;        // 6-launch layer: the residual stream lives in fragment order
    ru.M = B; ru.D = D; ru.eps = c.ln_eps; ru.xp_out = xp_ln;
    ru.ldws = e->ldws; ru.rows_ws = MT * 32;
    ru.ws = nullptr; ru.wte = e->wte; ru.wpe = e->wpe; ru.tokens = e->cur_tok; ru.positions = e->positions;
    ru.g = e->dec[0].ln1.g; ru.b = e->dec[0].ln1.b;
    auto row_update = [&]() {
        if (e->only_skinny) return;
        prof_mark(e, PK_ROWLN, st);
        launch_row_update_ln(ru, st);
    };
    auto skinny = [&](const bf16_t* xp, const Linear& l, int out_mode, float* ws) {
        SkinnyArgs a;
        memset(&a, 0, sizeof(a));
        a.xp = xp; a.Wp = l.Wp; a.Wq = l.Wq; a.wscale = l.wscale; a.W4 = l.W4; a.MT = MT; a.Npad = l.Npad; a.K = l.Kpad; a.N = l.N;
        a.out_mode = out_mode; a.col_tiles = l.col_tiles;
        if (out_mode == SK_OUT_PARTIAL) {
            a.splitk = l.splitk; a.ws = ws; a.ldws = e->ldws;
            const int NT = l.Npad / 32;
            // XCD-aware (tile, K slice) assignment: every XCD pulls one K slice of the activations into its L2, not all of them
            // (profiles/skinny_r03_xcd_slice_remap_ab.log: 1121 -> 1110 us per step, tokens identical)
            a.xcd_remap = (MT == 1 && l.splitk > 1 && 8 % l.splitk == 0 && (NT * l.splitk) % 8 == 0 &&
                           NT % (8 / l.splitk) == 0) ? 1 : 0;
        }
        else if (out_mode == SK_OUT_PACKED_ACT) { a.splitk = 1; a.bias = l.bias; a.act = ACT_GELU_TANH; a.out_xp = e->xp_mlp; a.out_KS = F / 16;
                                                  a.tail_ws = e->tail_ws; a.tail_cnt = e->tail_cnt; }
        else {
            a.splitk = 1; a.out_f32 = e->logits; a.ldo = e->Vpad; a.round_bf16 = 1;
            if (e->greedy_fused) { a.amax = e->amax; a.amax_rows = B; }      // greedy selection inside the lm_head launch (sv_generate)
            if (e->greedy_fused && e->fin_fold) { a.finish = &e->fin_args; a.fin_cnt = e->fin_cnt; }     // ... and the step's bookkeeping behind it
                    if (rc_enabled(e) && MT == 1 && xp != e->xp_a) { a.poison = e->xp_a; a.poison_bytes = xpa_bytes; }      // the next step's layer 0
            if (!e->skip_skinny) e->xpa_armed = a.poison != nullptr && lm_head_covers(e, xpa_bytes);
        }
        if (e->skip_skinny) return;
        if (out_mode == SK_OUT_F32) e->fin_folded = skinny_head_folds_finish(a);
        prof_mark(e, PK_SKINNY, st);
        launch_gemm_skinny(a, st);
    };
    for (int i = 0; i < c.n_layer; ++i) {
        DecLayer& L = e->dec[i];
        bool rc_done = false;
        if (rc) {
            SkinnyArgs a;
            memset(&a, 0, sizeof(a));
            a.xp = e->xp_a; a.Wp = L.c_attn.Wp; a.MT = MT; a.Npad = L.c_attn.Npad; a.K = L.c_attn.Kpad; a.N = L.c_attn.N;
            a.out_mode = SK_OUT_PARTIAL; a.splitk = L.c_attn.splitk; a.ws = wsA; a.ldws = e->ldws;
            prof_mark(e, PK_SKINNY, st);
            rc_done = launch_rowln_cattn(ru, a, e->d_bad, 500000, st, e->rc_delay, e->rc_dbg, i, e->num_cus) == 0;      // 5 ms budget; a refusal takes the two launches
            e->step_rc = e->step_rc || rc_done;
        }
        if (!rc_done) {
            bf16_t* const xo = rc ? e->xp_f : xp_ln;             // a refused fused launch must not reach the polled buffer with plain stores / loads
            ru.xp_out = xo;
            row_update();                                        // embedding or the previous layer's down-proj -> LN1(h)
            skinny(xo, L.c_attn, SK_OUT_PARTIAL, wsA);
            ru.xp_out = xp_ln;
        }
        // c_fc + down projection in ONE launch (mlp_fused.hip mlp_fused_kernel): on when the engine owns its GPU (sv_config.exclusive_device);
        // SV_EXP_MLP_FUSED_FORCE forces it on, SV_EXP_MLP_FUSED_OFF off (in-process A/B, tools/ab_exp.py).  It recognises unwritten activations by a pattern
        // that an EARLIER launch of the layer leaves in the buffer: the attention launch (16 bytes per thread: free in a latency-bound
        // kernel), or -- grid too small, or the profiling leg without attention -- the projection kernel (+0.5 us there)
        const bool fused = fold6 && e->mlp_fused_ok && !(e->exp & SV_EXP_MLP_FUSED_OFF) && (c.exclusive_device || (e->exp & SV_EXP_MLP_FUSED_FORCE)) && !e->fused_off;
        const size_t pat_bytes = (size_t)(F / 16) * 1024;
        const size_t poison_cap = (size_t)B * e->nkv * attn_max_splits(e) * 512 * 16;      // 16 bytes per thread of the attention launch
        const bool attn_poisons = fused && !e->only_skinny && pat_bytes + (rc ? xpa_bytes : 0u) <= poison_cap;
        const bool attn_poisons_xpa = rc && i + 1 < c.n_layer && (fused ? attn_poisons : xpa_bytes <= poison_cap);
        const bool cols_poisons_xpa = rc && fold6 && i + 1 < c.n_layer && !attn_poisons_xpa;      // (rc without room in the attention grid implies fold6: see above)
        if (!e->only_skinny) {
            AttnDecodeArgs ad;
            attn_decode_args(e, i, B, wsA, L.c_attn.splitk, L.c_attn.bias, e->xp_attn, ad);
            if (i == c.n_layer / 2) ad.trace = e->attn_trace;             // SV_ATTN_TRACE=1: one layer in the middle of the step
            if (attn_poisons) { ad.poison = e->xp_mlp; ad.poison_bytes = (unsigned)pat_bytes; }
            if (attn_poisons_xpa) { ad.poison2 = e->xp_a; ad.poison2_bytes = xpa_bytes; }     // the next layer's rowln_cattn launch
            if (e->lookup_on) launch_lookup_kv_write(lookup_kv_args(ad), st);      // sv_generate_lookup: the rows of a sequence see their siblings' K / V through the cache
            prof_mark(e, PK_ATTN, st);
            launch_attn_decode(ad, st);
        }
        if (fold6) {
            // attention output projection over the whole K per block: h += bf(x W^T + b) in place (+ partial row statistics), then
            // c_fc on the raw h with ln_2 folded into its weights / epilogue: no slabs, no row-update launch (decode_cols.hip)
            ColsArgs ca;
            memset(&ca, 0, sizeof(ca));
            ca.xp = e->xp_attn; ca.Wp = L.c_proj.Wp; ca.bias = L.c_proj.bias; ca.MT = MT; ca.M = B; ca.N = L.c_proj.N; ca.K = L.c_proj.Kpad;
            ca.cpb = L.c_proj.cpb; ca.h_xp = e->h_xp; ca.out_KS = D / 16;
            if (fused && !attn_poisons) { ca.poison = e->xp_mlp; ca.poison_bytes = (unsigned)pat_bytes; }
            if (cols_poisons_xpa) { ca.poison2 = e->xp_a; ca.poison2_bytes = xpa_bytes; }
            if (!e->skip_skinny) { prof_mark(e, PK_SKINNY, st); launch_gemm_cols(ca, st); }
            if (fused) {
                MlpFusedArgs ma;
                memset(&ma, 0, sizeof(ma));
                ma.W1 = L.c_fc.Wf; ma.x1 = e->h_xp; ma.N1 = L.c_fc.N; ma.N1pad = L.c_fc.Npad; ma.K1 = L.c_fc.Kpad;
                ma.fold_c1 = L.c_fc.c1; ma.fold_c2 = L.c_fc.c2; ma.fold_D = D; ma.fold_eps = c.ln_eps; ma.act = ACT_GELU_TANH;
                ma.out_xp = e->xp_mlp; ma.out_KS = F / 16;
                ma.W2 = L.c_proj2.Wp; ma.N2 = L.c_proj2.N; ma.N2pad = L.c_proj2.Npad; ma.K2 = L.c_proj2.Kpad; ma.splitk = L.c_proj2.splitk;
                ma.ws = wsB; ma.ldws = e->ldws; ma.rows_ws = MT * 32; ma.err = e->d_bad; ma.spin_ticks = 500000;     // 5 ms at 100 MHz
                ma.trace = (i == c.n_layer / 2) ? e->mlp_trace : nullptr;        // one layer in the middle of the step
                // the launcher re-checks the shapes of THIS layer (sv_create looked at layer 0): a layer it refuses takes the two launches
                // below -- never a silently skipped MLP
                bool done = e->skip_skinny;
                if (!done) { prof_mark(e, PK_SKINNY, st); done = launch_mlp_fused(ma, st) == 0; }
                if (done) {
                    e->step_mlp = e->step_mlp || !e->skip_skinny;
                    const LNp& nx = (i + 1 < c.n_layer) ? e->dec[i + 1].ln1 : e->ln_f;
                    ru.ws = wsB; ru.splitk = L.c_proj2.splitk; ru.bias = L.c_proj2.bias; ru.g = nx.g; ru.b = nx.b;
                    continue;
                }
            }
            SkinnyArgs a;
            memset(&a, 0, sizeof(a));
            a.xp = e->h_xp; a.Wp = L.c_fc.Wf; a.MT = MT; a.Npad = L.c_fc.Npad; a.K = L.c_fc.Kpad; a.N = L.c_fc.N; a.splitk = 1;
            a.out_mode = SK_OUT_PACKED_ACT; a.act = ACT_GELU_TANH; a.out_xp = e->xp_mlp; a.out_KS = F / 16;
            a.fold_c1 = L.c_fc.c1; a.fold_c2 = L.c_fc.c2; a.fold_D = D; a.fold_eps = c.ln_eps;
            if (!e->skip_skinny) { prof_mark(e, PK_SKINNY, st); launch_gemm_skinny(a, st); }
        } else {
            skinny(e->xp_attn, L.c_proj, SK_OUT_PARTIAL, wsB);
            ru.ws = wsB; ru.splitk = L.c_proj.splitk; ru.bias = L.c_proj.bias; ru.g = L.ln2.g; ru.b = L.ln2.b;
            bf16_t* const x2 = rc_enabled(e) ? e->xp_f : e->xp_a;      // an engine with the fused launch keeps xp_a for it alone (write-through / L1-bypass only)
            ru.xp_out = x2;
            row_update();                                        // + bias + residual, LN2
            skinny(x2, L.c_fc, SK_OUT_PACKED_ACT, nullptr);
            ru.xp_out = xp_ln;
        }
        skinny(e->xp_mlp, L.c_proj2, SK_OUT_PARTIAL, wsB);
        const LNp& nxt = (i + 1 < c.n_layer) ? e->dec[i + 1].ln1 : e->ln_f;
        ru.ws = wsB; ru.splitk = L.c_proj2.splitk; ru.bias = L.c_proj2.bias; ru.g = nxt.g; ru.b = nxt.b;
    }
    bf16_t* xp_last = rc_enabled(e) ? e->xp_f : e->xp_a;         // (an engine with the fused launch keeps xp_a for it alone: see rc_enabled)
    ru.xp_out = xp_last;
    row_update();                                                // + bias + residual, ln_f
    skinny(xp_last, e->lm_head, SK_OUT_F32, nullptr);
    prof_mark(e, PK_SAMPLE, st);      // closes the lm_head interval; whatever follows is sampling
}

int sveng::check_ready(sv_engine* e) {
    if (!e) return fail(SV_EINVAL, "null engine");
    int r = sv_weights_complete(e);
    if (r) return fail(SV_ESTATE, "weights incomplete: %s", g_err.c_str());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: forward entry points
// ------------------------------------------------------------------------------------------------
extern "C" int sv_encode_image(sv_engine* e, const void* dev_image, int32_t B, void* dev_out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_image || !dev_out || B < 1 || B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_encode_image: bad B=%d (max_batch %d) or null pointer", B, e->cfg.max_batch);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    SVCHECK(vision_forward(e, (const bf16_t*)dev_image, B, (bf16_t*)dev_out, (hipStream_t)stream));
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_adapter(sv_engine* e, const void* dev_in, int32_t B, void* dev_out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_in || !dev_out || B < 1 || B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_adapter: bad B=%d or null pointer", B);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    SVCHECK(adapter_forward(e, (const bf16_t*)dev_in, B, (bf16_t*)dev_out, (hipStream_t)stream));
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_embed_tokens(sv_engine* e, const int64_t* dev_ids, int32_t n, void* dev_out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_ids || !dev_out || n < 0) return fail(SV_EINVAL, "sv_embed_tokens: bad argument");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    launch_gather_rows(e->wte, dev_ids, (bf16_t*)dev_out, n, e->cfg.hidden, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

// a1 (starvector_base.py:203-221) without the torch.cat: the adapter's visual rows and the prompt's token rows are written straight into
// the caller's [B][T + P][D] inputs_embeds buffer (the one sv_prefill / sv_generate read)
extern "C" int sv_adapter_into(sv_engine* e, const void* dev_in, int32_t B, void* dev_embeds, int32_t S0, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_in || !dev_embeds || B < 1 || B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_adapter_into: bad B=%d or null pointer", B);
    if (S0 < e->T) return fail(SV_EINVAL, "sv_adapter_into: S0=%d is shorter than the %d visual rows", S0, e->T);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    SVCHECK(adapter_forward(e, (const bf16_t*)dev_in, B, (bf16_t*)dev_embeds, (hipStream_t)stream, (size_t)S0 * e->cfg.hidden));
    HIPCHECK(hipGetLastError());
    return 0;
}
extern "C" int sv_embed_tokens_into(sv_engine* e, const int64_t* dev_ids, int32_t B, int32_t P, void* dev_embeds, int32_t S0, int32_t row0,
                                    sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_ids || !dev_embeds || B < 1 || P < 0 || row0 < 0 || row0 + P > S0) return fail(SV_EINVAL, "sv_embed_tokens_into: bad argument (rows %d..%d of %d)", row0, row0 + P, S0);
    if (P == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    const int D = e->cfg.hidden;
    launch_gather_rows(e->wte, dev_ids, (bf16_t*)dev_embeds + (size_t)row0 * D, B * P, D, (hipStream_t)stream, P, (size_t)S0 * D);
    HIPCHECK(hipGetLastError());
    return 0;
}

static int copy_logits_out(sv_engine* e, int B, float* dev_logits, hipStream_t st) {
    HIPCHECK(hipMemcpy2DAsync(dev_logits, (size_t)e->cfg.vocab * sizeof(float), e->logits,
                              (size_t)e->Vpad * sizeof(float), (size_t)e->cfg.vocab * sizeof(float), B,
                              hipMemcpyDeviceToDevice, st));
    return 0;
}

int sveng::cb_guard(sv_engine* e, const char* who) {
    if (e->cb_active) return fail(SV_ESTATE, "%s: a continuous batch holds the KV cache of this engine (sv_cb_reset first)", who);
    return 0;
}

// the host-side contexts behind a call that leaves them known: lens[b] (nullptr: `len` each) tokens cached, pages for `cap` tokens
static void set_contexts(sv_engine* e, int B, const int32_t* lens, int len, int cap) {
    e->ctx_len.assign((size_t)e->cfg.max_batch, 0);
    e->ctx_cap.assign((size_t)e->cfg.max_batch, 0);
    for (int b = 0; b < B; ++b) { e->ctx_len[b] = lens ? lens[b] : len; e->ctx_cap[b] = cap; }
    e->ctx_known = true;
}

int sveng::prefill_locked(sv_engine* e, const void* dev_embeds, int B, int S0, int total_len, hipStream_t st, bool set_positions) {
    SVCHECK(cb_guard(e, "prefill"));
    if (!dev_embeds || B < 1 || B > e->cfg.max_batch) return fail(SV_EINVAL, "prefill: bad B=%d (max_batch %d)", B, e->cfg.max_batch);
    if (S0 < 1 || S0 > e->cfg.max_seq_len) return fail(SV_EINVAL, "prefill: S0=%d out of range (max_seq_len %d)", S0, e->cfg.max_seq_len);
    SVCHECK(assign_pages(e, B, total_len, st));
    SVCHECK(prefill_forward(e, (const bf16_t*)dev_embeds, B, S0, st));
    if (set_positions) fill_i32(e->positions, S0, B, st);          // (sv_generate sets its own generation state in one launch)
    e->cached_B = B;
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_prefill(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, float* dev_logits,
                          sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_logits) return fail(SV_EINVAL, "sv_prefill: null logits pointer");
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    SVCHECK(prefill_locked(e, dev_embeds, B, S0, e->cfg.max_seq_len, st));
    SVCHECK(copy_logits_out(e, B, dev_logits, st));
    set_contexts(e, B, nullptr, S0, e->cfg.max_seq_len);
    return 0;
}

extern "C" int sv_prefill_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, float* dev_logits,
                                 sv_stream stream) {
    // (the checks that need no engine come first: they are the same on a machine without a GPU)
    if (!dev_embeds_packed || !host_lens || !dev_logits) return fail(SV_EINVAL, "sv_prefill_ragged: null embeds / lengths / logits pointer");
    if (B < 1) return fail(SV_EINVAL, "sv_prefill_ragged: bad B=%d", B);
    for (int b = 0; b < B; ++b)
        if (host_lens[b] < 1) return fail(SV_EINVAL, "sv_prefill_ragged: length %d of sequence %d (must be >= 1)", host_lens[b], b);
    SVCHECK(check_ready(e));
    if (B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_prefill_ragged: bad B=%d (max_batch %d)", B, e->cfg.max_batch);
    SVCHECK(ragged_check_lens(e, host_lens, B, "sv_prefill_ragged", nullptr, nullptr));
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    SVCHECK(cb_guard(e, "sv_prefill_ragged"));
    SVCHECK(assign_pages_ragged(e, B, host_lens, -1, st));
    SVCHECK(prefill_forward_ragged(e, (const bf16_t*)dev_embeds_packed, B, host_lens, st));
    ragged_positions(e, B, 1, 0, st);
    e->cached_B = B;
    HIPCHECK(hipGetLastError());
    SVCHECK(copy_logits_out(e, B, dev_logits, st));
    set_contexts(e, B, host_lens, 0, e->cfg.max_seq_len);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: many rows behind a cached context (include/starvector_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int sv_set_prefill_chunk(sv_engine* e, int32_t rows) {
    if (!e) return fail(SV_EINVAL, "sv_set_prefill_chunk: null engine");
    if (rows < 0) return fail(SV_EINVAL, "sv_set_prefill_chunk: rows %d (0 = off, or a row budget >= 1)", rows);
    std::lock_guard<std::mutex> lk(e->mu);
    e->prefill_chunk = rows;
    return 0;
}

extern "C" int sv_prefill_open(sv_engine* e, int32_t B, const int32_t* host_total_lens) {
    if (!host_total_lens) return fail(SV_EINVAL, "sv_prefill_open: null lengths pointer");
    if (B < 1) return fail(SV_EINVAL, "sv_prefill_open: bad B=%d", B);
    for (int b = 0; b < B; ++b)
        if (host_total_lens[b] < 1) return fail(SV_EINVAL, "sv_prefill_open: total length %d of sequence %d (must be >= 1)", host_total_lens[b], b);
    SVCHECK(check_ready(e));
    if (B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_prefill_open: bad B=%d (max_batch %d)", B, e->cfg.max_batch);
    SVCHECK(ragged_check_lens(e, host_total_lens, B, "sv_prefill_open", nullptr, nullptr));
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = nullptr;                   // (no device work but the table upload and the positions: done when the call returns)
    SVCHECK(cb_guard(e, "sv_prefill_open"));
    SVCHECK(assign_pages_ragged(e, B, host_total_lens, 0, st));
    fill_i32(e->positions, 0, B, st);
    e->cached_B = B;
    e->xpa_armed = false;
    e->dbg_pos_hi = 0;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    set_contexts(e, B, nullptr, 0, 0);
    for (int b = 0; b < B; ++b) e->ctx_cap[b] = (host_total_lens[b] + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS * SV_PAGE_TOKENS;
    return 0;
}

extern "C" int sv_prefill_extend(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_total_lens,
                                 float* dev_logits, sv_stream stream) {
    const char* who = "sv_prefill_extend";
    // (the checks that need no engine come first: they are the same on a machine without a GPU)
    if (!dev_embeds_packed || !host_lens || !dev_logits) return fail(SV_EINVAL, "%s: null embeds / lengths / logits pointer", who);
    if (B < 1) return fail(SV_EINVAL, "%s: bad B=%d", who, B);
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        if (host_lens[b] < 0) return fail(SV_EINVAL, "%s: length %d of sequence %d (must be >= 0)", who, host_lens[b], b);
        if (host_total_lens && host_total_lens[b] < host_lens[b])
            return fail(SV_EINVAL, "%s: total length %d of sequence %d is below its %d new rows", who, host_total_lens[b], b, host_lens[b]);
        rows += host_lens[b];
    }
    if (rows == 0) return fail(SV_EINVAL, "%s: every length is 0: nothing to append", who);
    SVCHECK(check_ready(e));
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, who));
    if (B != e->cached_B) return fail(SV_EINVAL, "%s: B=%d but the cache holds %d sequences", who, B, e->cached_B);
    if (!e->ctx_known)
        return fail(SV_ESTATE, "%s: the context lengths of the cache are unknown (they are known behind sv_prefill, sv_prefill_ragged, sv_prefill_open, "
                    "sv_prefill_extend and sv_decode_step)", who);
    std::vector<ExtendSeq> seqs((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int ctx = e->ctx_len[b], T = ctx + host_lens[b], total = host_total_lens ? host_total_lens[b] : T;
        if (T > total) return fail(SV_EINVAL, "%s: context %d + length %d of sequence %d exceeds its total length %d", who, ctx, host_lens[b], b, total);
        if (total > e->ctx_cap[b] || total > e->cfg.max_seq_len)
            return fail(SV_EINVAL, "%s: total length %d of sequence %d exceeds its pages (%d tokens) or max_seq_len %d", who, total, b, e->ctx_cap[b], e->cfg.max_seq_len);
        seqs[b] = {ctx, host_lens[b], total};
    }
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    PlanProj pj[4];
    const int n_proj = plan_proj(e, pj);
    ExtendPass p;
    extend_plan(seqs.data(), B, attn_prefill_q_tile(e->cfg.n_head, e->nkv), pj, n_proj, p);
    for (int b = 0; b < B; ++b) p.list[XL_POS].push_back(seqs[b].ctx + seqs[b].len);
    SVCHECK(extend_forward(e, p, (const bf16_t*)dev_embeds_packed, nullptr, st));
    size_t pos_off = 0;
    for (int i = 0; i < XL_POS; ++i) pos_off += p.list[i].size();
    HIPCHECK(hipMemcpyAsync(e->positions, e->d_rag + pos_off, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    for (size_t i = 0; i < p.fin.size(); ++i)
        HIPCHECK(hipMemcpyAsync(dev_logits + (size_t)p.fin[i] * e->cfg.vocab, e->logits + i * e->Vpad, (size_t)e->cfg.vocab * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipGetLastError());
    for (int b = 0; b < B; ++b) e->ctx_len[b] += host_lens[b];
    e->dbg_pos_hi = *std::max_element(e->ctx_len.begin(), e->ctx_len.begin() + B);
    return 0;
}

// A scoring call, as sv_forward_logits / sv_forward_logprobs / sv_forward_topk (B sequences of S rows, the last n_keep kept), sv_forward_logprobs_ragged
// (lens, keep) or sv_forward_logprobs_prefixed (P prefixes in front of lens, prefix_of, keep) describes it
struct ScoreCall {
    const char* who;
    enum Form { RECT, RAGGED, PREFIXED } form;
    const void* embeds;
    int32_t B, S, n_keep;
    const int32_t *lens, *keep;
    float temperature;
    ScoreLogprobs lp;
    const void* prefixes = nullptr;
    int32_t P = 0;
    const int32_t *prefix_lens = nullptr, *prefix_of = nullptr;
};
// The checks of a call with a ScoreLogprobs that need no engine (they come first: they are the same on a machine without a GPU).  Every check is
// stated once; the rectangular and the packed forms have always asked in different orders, and which of two violations is reported is part of each
// one's contract.
static int check_score_call(const ScoreCall& c) {
    const char* who = c.who;
    const auto nulls = [&]() -> int {
        if (c.form == ScoreCall::PREFIXED && (!c.prefixes || !c.prefix_lens || !c.embeds || !c.lens || !c.prefix_of || !c.keep || !c.lp.targets))
            return fail(SV_EINVAL, "%s: null prefixes / embeds / lengths / prefix_of / keep / targets pointer", who);
        if (c.form == ScoreCall::RAGGED && (!c.embeds || !c.lens || !c.keep || !c.lp.targets)) return fail(SV_EINVAL, "%s: null embeds / lengths / keep / targets pointer", who);
        if (!c.embeds || !c.lp.targets) return fail(SV_EINVAL, "%s: null embeds / targets", who);
        return 0;
    };
    const auto shape = [&]() -> int {
        if (c.form == ScoreCall::RECT) return (c.S < 1 || c.n_keep < 1 || c.n_keep > c.S) ? fail(SV_EINVAL, "%s: n_keep=%d must be in 1..S (S=%d)", who, c.n_keep, c.S) : 0;
        if (c.form == ScoreCall::PREFIXED) return prefix_check(who, c.prefix_lens, c.P, c.lens, c.prefix_of, c.B, c.keep);
        if (c.B < 1) return fail(SV_EINVAL, "%s: bad B=%d", who, c.B);
        for (int b = 0; b < c.B; ++b) {
            if (c.lens[b] < 1) return fail(SV_EINVAL, "%s: length %d of sequence %d (must be >= 1)", who, c.lens[b], b);
            if (c.keep[b] < 1 || c.keep[b] > c.lens[b])
                return fail(SV_EINVAL, "%s: keep %d of sequence %d must be in 1..its length %d", who, c.keep[b], b, c.lens[b]);
        }
        return 0;
    };
    const auto temperature = [&]() -> int {
        return (!(c.temperature > 0.f) || !std::isfinite(c.temperature)) ? fail(SV_EINVAL, "%s: temperature must be finite and > 0", who) : 0;
    };
    const auto lists = [&]() -> int {
        if (c.lp.k < 0 || c.lp.k > SV_TOPK_MAX) return fail(SV_EINVAL, "%s: k=%d must be in 0..%d", who, c.lp.k, SV_TOPK_MAX);
        if (c.lp.k > 0 && (!c.lp.topk_ids || !c.lp.topk_logprobs)) return fail(SV_EINVAL, "%s: k=%d with a null dev_topk_ids / dev_topk_logprobs", who, c.lp.k);
        return 0;
    };
    const auto outputs = [&]() -> int {
        if (c.lp.k == 0 && !c.lp.logprob && !c.lp.lse && !c.lp.entropy && !c.lp.argmax) return fail(SV_EINVAL, "%s: every output pointer is null", who);
        return 0;
    };
    if (c.form != ScoreCall::RECT) { SVCHECK(nulls()); SVCHECK(shape()); SVCHECK(temperature()); SVCHECK(lists()); return outputs(); }
    SVCHECK(lists()); SVCHECK(nulls()); SVCHECK(outputs()); SVCHECK(temperature()); return shape();
}

// the packed kept row a scoring kernel flagged -> (sequence, kept position): n_keep rows per sequence, or the prefix sums of keep
static void score_row_owner(int row, int B, int n_keep, const int32_t* keep, int* seq, int* pos) {
    int b = 0, first = 0;
    if (!keep) { b = row / n_keep; first = b * n_keep; }
    else while (b + 1 < B && first + keep[b] <= row) first += keep[b++];
    *seq = b; *pos = row - first;
}
// the scoring kernels' flag: a target outside the vocabulary (its logprob is NaN) / a row without a finite logit (all of its outputs are NaN)
static int score_flag_report(sv_engine* e, const char* who, int B, int n_keep, const int32_t* keep, hipStream_t st) {
    int32_t flag[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(flag, e->score_chunk_ws + (size_t)e->score_chunk_alloc * e->Vpad, sizeof(flag), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (!(flag[0] & 3)) return 0;
    int seq = 0, pos = 0;
    score_row_owner(flag[1], B, n_keep, keep, &seq, &pos);
    if (flag[0] & 2)
        return fail(SV_EHIP, "%s: a row of logits had no finite value (NaN / Inf in the weights or inputs?); first at row %d "
                             "(sequence %d, kept position %d)", who, flag[1], seq, pos);
    return fail(SV_EINVAL, "%s: a target id outside [0, %d) that is not -100; first at row %d (sequence %d, kept position %d)",
                who, e->cfg.vocab, flag[1], seq, pos);
}
// One scoring-mode prompt pass under the engine lock, and -- unless the logits go to dev_scores -- the kernels' flag.  The rectangular and the ragged
// form assign pages for exactly the rows given and leave positions = the lengths.  The prefixed form (`prefixed`: its plan) assigns no page and writes
// none: whatever the cache held is void for sv_decode_step from here on (cached_B = 0: SV_ESTATE).
static int score_pass(sv_engine* e, const ScoreCall& c, bf16_t* dev_scores, const PackedPlan* prefixed, hipStream_t st) {
    const ScoreLogprobs* lp = dev_scores ? nullptr : &c.lp;
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    SVCHECK(cb_guard(e, c.who));
    if (c.form == ScoreCall::PREFIXED) {
        e->cached_B = 0;
        SVCHECK(prefill_forward_packed(e, *prefixed, nullptr, lp, st));
    } else if (c.form == ScoreCall::RAGGED) {
        SVCHECK(assign_pages_ragged(e, c.B, c.lens, 0, st));
        SVCHECK(prefill_forward_ragged(e, (const bf16_t*)c.embeds, c.B, c.lens, st, nullptr, c.keep, lp));
        ragged_positions(e, c.B, 1, 0, st);
        e->cached_B = c.B;
    } else {
        SVCHECK(assign_pages(e, c.B, c.S, st));
        SVCHECK(prefill_forward(e, (const bf16_t*)c.embeds, c.B, c.S, st, c.n_keep, dev_scores, nullptr, lp));
        fill_i32(e->positions, c.S, c.B, st);
        e->cached_B = c.B;
    }
    HIPCHECK(hipGetLastError());
    if (!lp) return 0;
    return score_flag_report(e, c.who, c.B, c.n_keep, c.form == ScoreCall::RECT ? nullptr : c.keep, st);
}

extern "C" int sv_forward_logits(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep,
                                 void* dev_logits_bf16, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_embeds || !dev_logits_bf16) return fail(SV_EINVAL, "sv_forward_logits: null argument");
    if (B < 1 || B > e->cfg.max_batch) return fail(SV_EINVAL, "sv_forward_logits: bad B=%d (max_batch %d)", B, e->cfg.max_batch);
    if (S < 1 || S > e->cfg.max_seq_len) return fail(SV_EINVAL, "sv_forward_logits: S=%d out of range (max_seq_len %d)", S, e->cfg.max_seq_len);
    if (n_keep < 1 || n_keep > S) return fail(SV_EINVAL, "sv_forward_logits: n_keep=%d must be in 1..S", n_keep);
    return score_pass(e, {"sv_forward_logits", ScoreCall::RECT, dev_embeds, B, S, n_keep, nullptr, nullptr, 0.f, {}}, (bf16_t*)dev_logits_bf16, nullptr,
                      (hipStream_t)stream);
}

// The engine's side of a prefixed call: every solo sequence fits, and none is refused (prefix/prefix.hip).  Every weight format: the pass is the ragged
// pass's launches -- fp8's column-scale epilogue and the bf16 image of an mxfp4 engine are per row and per column --, and
// tests/test_gpu_prefix_scoring.py holds each format to the contract.
static int prefixed_plan(sv_engine* e, const ScoreCall& c, PackedPlan& plan) {
    for (int b = 0; b < c.B; ++b) {
        const long long T = (long long)c.prefix_lens[c.prefix_of[b]] + c.lens[b];
        if (T > e->cfg.max_seq_len)
            return fail(SV_EINVAL, "%s: length %lld of sequence %d (prefix %d + own %d) out of range (1..max_seq_len %d)", c.who, T, b,
                        c.prefix_lens[c.prefix_of[b]], c.lens[b], e->cfg.max_seq_len);
    }
    static const char* const proj_name[4] = {"c_attn", "attention c_proj", "c_fc", "MLP c_proj"};
    PlanProj pj[4];
    const int n_proj = plan_proj(e, pj);
    prefix_plan(c.prefix_lens, c.P, c.lens, c.prefix_of, c.B, attn_prefill_q_tile(e->cfg.n_head, e->nkv), pj, n_proj, c.keep, plan);
    if (plan.refused >= 0) {
        const int b = plan.refused, pl = c.prefix_lens[c.prefix_of[b]];
        return fail(SV_EINVAL, "%s: sequence %d (prefix %d + own %d rows): the %d remainder rows of its %d-row solo run at %s would reach into the "
                    "shared prefix (score it alone: sv_forward_logprobs_ragged on the concatenation)", c.who, b, pl, c.lens[b],
                    seq_peel_rows(pl + c.lens[b]), pl + c.lens[b], proj_name[plan.refused_proj]);
    }
    plan.src[0] = (const bf16_t*)c.prefixes; plan.src[1] = (const bf16_t*)c.embeds;
    return 0;
}
static int score_call(sv_engine* e, ScoreCall c, sv_stream stream) {
    SVCHECK(check_score_call(c));
    SVCHECK(check_ready(e));
    if (c.B < 1 || c.B > e->cfg.max_batch) return fail(SV_EINVAL, "%s: bad B=%d (max_batch %d)", c.who, c.B, e->cfg.max_batch);
    PackedPlan prefixed;
    if (c.form == ScoreCall::PREFIXED) SVCHECK(prefixed_plan(e, c, prefixed));
    else if (c.form == ScoreCall::RAGGED) SVCHECK(ragged_check_lens(e, c.lens, c.B, c.who, nullptr, nullptr));
    else if (c.S > e->cfg.max_seq_len) return fail(SV_EINVAL, "%s: S=%d out of range (max_seq_len %d)", c.who, c.S, e->cfg.max_seq_len);
    if (c.lp.k == 0) { c.lp.topk_ids = nullptr; c.lp.topk_logprobs = nullptr; c.lp.rank = nullptr; }
    return score_pass(e, c, nullptr, &prefixed, (hipStream_t)stream);
}

extern "C" int sv_forward_logprobs(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep,
                                   const int32_t* dev_targets, float temperature, float* dev_logprob, float* dev_logsumexp,
                                   float* dev_entropy, int32_t* dev_argmax, sv_stream stream) {
    return score_call(e, {"sv_forward_logprobs", ScoreCall::RECT, dev_embeds, B, S, n_keep, nullptr, nullptr, temperature,
                          {dev_targets, 1.0f / temperature, dev_logprob, dev_logsumexp, dev_entropy, dev_argmax}}, stream);
}
// k == 0 is sv_forward_logprobs, to the letter
extern "C" int sv_forward_topk(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S, int32_t n_keep, const int32_t* dev_targets,
                               float temperature, float* dev_logprob, float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t k,
                               int32_t* dev_topk_ids, float* dev_topk_logprobs, int32_t* dev_rank, sv_stream stream) {
    return score_call(e, {k == 0 ? "sv_forward_logprobs" : "sv_forward_topk", ScoreCall::RECT, dev_embeds, B, S, n_keep, nullptr, nullptr, temperature,
                          {dev_targets, 1.0f / temperature, dev_logprob, dev_logsumexp, dev_entropy, dev_argmax, k, dev_topk_ids, dev_topk_logprobs, dev_rank}},
                      stream);
}
// sv_forward_topk over packed sequences of different lengths, each keeping its own number of rows
extern "C" int sv_forward_logprobs_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_keep,
                                          const int32_t* dev_targets, float temperature, float* dev_logprob, float* dev_logsumexp, float* dev_entropy,
                                          int32_t* dev_argmax, int32_t k, int32_t* dev_topk_ids, float* dev_topk_logprobs, int32_t* dev_rank,
                                          sv_stream stream) {
    return score_call(e, {"sv_forward_logprobs_ragged", ScoreCall::RAGGED, dev_embeds_packed, B, 0, 0, host_lens, host_keep, temperature,
                          {dev_targets, 1.0f / temperature, dev_logprob, dev_logsumexp, dev_entropy, dev_argmax, k, dev_topk_ids, dev_topk_logprobs, dev_rank}},
                      stream);
}
// sv_forward_logprobs_ragged over sequences that share prefixes: every prefix goes through the decoder once
extern "C" int sv_forward_logprobs_prefixed(sv_engine* e, const void* dev_prefix_packed, int32_t P, const int32_t* host_prefix_lens,
                                            const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const int32_t* host_prefix_of,
                                            const int32_t* host_keep, const int32_t* dev_targets, float temperature, float* dev_logprob,
                                            float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t k, int32_t* dev_topk_ids,
                                            float* dev_topk_logprobs, int32_t* dev_rank, sv_stream stream) {
    return score_call(e, {"sv_forward_logprobs_prefixed", ScoreCall::PREFIXED, dev_embeds_packed, B, 0, 0, host_lens, host_keep, temperature,
                          {dev_targets, 1.0f / temperature, dev_logprob, dev_logsumexp, dev_entropy, dev_argmax, k, dev_topk_ids, dev_topk_logprobs, dev_rank},
                          dev_prefix_packed, P, host_prefix_lens, host_prefix_of},
                      stream);
}

extern "C" int sv_decode_step(sv_engine* e, const int32_t* dev_tokens, int32_t B, float* dev_logits, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_tokens || !dev_logits) return fail(SV_EINVAL, "sv_decode_step: null pointer");
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, "sv_decode_step"));
    if (B != e->cached_B) return fail(SV_ESTATE, "sv_decode_step: B=%d but the cache holds %d sequences", B, e->cached_B);
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHECK(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), st));         // a flag left by an earlier, failed call is not this call's
    HIPCHECK(hipMemcpyAsync(e->cur_tok, dev_tokens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    decode_forward(e, B, st);
    add_i32(e->positions, 1, B, st);
    if (e->ctx_known) for (int b = 0; b < B; ++b) ++e->ctx_len[b];
    SVCHECK(copy_logits_out(e, B, dev_logits, st));
    HIPCHECK(hipGetLastError());
    // the fused MLP launch reports a give-up through d_bad (code 3): logits computed from its unwritten activations are void
    if (e->mlp_fused_ok || e->rc_fused_ok) SVCHECK(check_finite_logits(e, st, "sv_decode_step"));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI (measurement surface): where the time to first token goes.  One pass image -> encoder -> adapter -> prompt rows -> prompt
// pass -> lm_head -> first greedy token, with a HIP event in front of every launch (group); out[2k] = ms per pass in stage k,
// out[2k + 1] = launches (groups) per pass, k = 0 encoder GEMMs, 1 encoder attention, 2 encoder row kernels (im2col, embedding +
// ln_pre, LayerNorms), 3 adapter GEMMs, 4 adapter norm + prompt-token gather, 5 decoder prompt-pass GEMMs (tile launches),
// 6 remainder-row launches of peeled GEMMs (encoder, adapter and decoder), 7 prompt-pass attention (+ RoPE, KV scatter), 8 prompt-pass
// row kernels (position embedding, LayerNorms, last-row gather, ln_f), 9 lm_head, 10 first-token selection; out[22] = the
// event-pair overhead subtracted from every interval (ms), out[23] = first event -> last event, raw (ms).  The events themselves
// open gaps between launches, so the stages sum to a little more than an unprofiled TTFT: bench.py prints both.
// dev_image NULL (text2svg): no encoder / adapter; the prompt is dev_ids [B][P] alone.
// ------------------------------------------------------------------------------------------------
extern "C" int sv_profile_ttft(sv_engine* e, const void* dev_image, int32_t B, const int64_t* dev_ids, int32_t P, int32_t iters,
                               double* out24, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!out24 || !dev_ids || iters < 1 || B < 1 || B > e->cfg.max_batch || P < 1) return fail(SV_EINVAL, "sv_profile_ttft: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, "sv_profile_ttft"));
    const sv_config& c = e->cfg;
    const int D = c.hidden, T = dev_image ? e->T : 0, S0 = T + P;
    if (S0 + 1 > c.max_seq_len) return fail(SV_EINVAL, "sv_profile_ttft: prompt of %d rows does not fit max_seq_len %d", S0, c.max_seq_len);
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    struct Bufs { bf16_t* enc = nullptr; bf16_t* emb = nullptr; ~Bufs() { if (enc) (void)hipFree(enc); if (emb) (void)hipFree(emb); } } bufs;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&bufs.emb), (size_t)B * S0 * D * sizeof(bf16_t)));
    if (dev_image) HIPCHECK(hipMalloc(reinterpret_cast<void**>(&bufs.enc), (size_t)B * e->T * c.vit_width * sizeof(bf16_t)));
    SVCHECK(assign_pages(e, B, S0 + 1, st));
    for (int k = 0; k < 24; ++k) out24[k] = 0.0;
    double overhead_ms = 0.0;
    {
        struct EvPair { hipEvent_t a = nullptr, b = nullptr; ~EvPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
        HIPCHECK(hipEventCreate(&ev.a)); HIPCHECK(hipEventCreate(&ev.b));
        float acc = 0.f;
        for (int i = 0; i < 20; ++i) {
            HIPCHECK(hipEventRecord(ev.a, st)); HIPCHECK(hipEventRecord(ev.b, st));
            HIPCHECK(hipEventSynchronize(ev.b));
            float ms = 0.f; HIPCHECK(hipEventElapsedTime(&ms, ev.a, ev.b)); acc += ms;
        }
        overhead_ms = acc / 20.0;
    }
    struct ProfGuard { sv_engine* e; ~ProfGuard() { e->prof_on = false; } } pg{e};
    for (int it = 0; it < iters + 1; ++it) {
        e->prof_on = true; e->prof_used = 0;
        if (dev_image) {
            SVCHECK(vision_forward(e, (const bf16_t*)dev_image, B, bufs.enc, st));
            SVCHECK(adapter_forward(e, bufs.enc, B, bufs.emb, st, (size_t)S0 * D));
        }
        prof_mark(e, PK_AD_NORM, st);                     // the prompt-token gather travels with the adapter stage (a1)
        launch_gather_rows(e->wte, dev_ids, bufs.emb + (size_t)T * D, B * P, D, st, P, (size_t)S0 * D);
        SVCHECK(prefill_forward(e, bufs.emb, B, S0, st));
        prof_mark(e, PK_FIRST_SAMPLE, st);
        launch_argmax_partial(e->logits, e->Vpad, c.vocab, e->am_val, e->am_idx, B, nullptr, e->seen_words, 1.f, st);
        prof_mark(e, PK_END, st);
        e->prof_on = false;
        HIPCHECK(hipStreamSynchronize(st));
        HIPCHECK(hipGetLastError());
        if (it == 0) continue;                            // warm-up pass (creates the events, lets the big-M tuner settle)
        for (size_t i = 0; i + 1 < e->prof_used; ++i) {
            const int k = e->prof_kind[i] - PK_TTFT_FIRST;
            if (k < 0 || k >= PK_TTFT_COUNT) continue;
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]));
            double d = (double)ms - overhead_ms;
            out24[2 * k] += d > 0 ? d : 0;
            out24[2 * k + 1] += 1.0;
        }
        float total = 0.f;
        HIPCHECK(hipEventElapsedTime(&total, e->prof_ev[0], e->prof_ev[e->prof_used - 1]));
        out24[23] += total;
    }
    for (int k = 0; k < 2 * PK_TTFT_COUNT; ++k) out24[k] /= (double)iters;
    out24[23] /= (double)iters;
    out24[22] = overhead_ms;
    fill_i32(e->positions, S0, B, st);
    e->cached_B = B;
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}
