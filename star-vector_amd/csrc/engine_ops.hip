// Host driver, part 5 of 5: host-side planning probes (callable without a GPU), the pre-processing ABI, decode-step profiling
// and the single-operator test surfaces (sv_op_*, sv_bench_*).
#include <cmath>
#include "engine_internal.h"

struct TmpBufs {
    std::vector<void*> p;
    ~TmpBufs() { for (void* q : p) (void)hipFree(q); }
    template <typename T> int get(T** out, size_t count) {
        hipError_t r = hipMalloc(reinterpret_cast<void**>(out), count * sizeof(T));
        if (r != hipSuccess) return fail(SV_ENOMEM, "hipMalloc: %s", hipGetErrorString(r));
        p.push_back(*out);
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// C ABI: host-side decisions, callable without a GPU (CPU tests)
// ------------------------------------------------------------------------------------------------
// A/B tool surface (tools/ab_exp.py): change the experiment mask of a live engine; captured graphs are keyed on it
extern "C" int sv_debug_set_exp(sv_engine* e, int32_t mask) {
    if (!e) return fail(SV_EINVAL, "null engine");
    SVCHECK(check_exp_mask(mask, "sv_debug_set_exp"));
    std::lock_guard<std::mutex> lk(e->mu);
    e->exp = mask;
    e->xpa_armed = false;                    // another mask may have run plain stores through xp_a: the next step re-arms it
    cb_drop_graphs(e);                       // the continuous-batching step graphs were captured with the old mask
    return 0;
}

extern "C" int sv_debug_exp_known(void) { return SV_EXP_KNOWN; }

extern "C" int sv_debug_step_plan(sv_engine* e, int32_t* out4) {
    if (!e || !out4) return fail(SV_EINVAL, "sv_debug_step_plan: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    out4[0] = e->gen_step.x ? e->step_nodes : 0;
    out4[1] = e->step_rc ? 1 : 0; out4[2] = e->step_sel ? 1 : 0; out4[3] = e->step_mlp ? 1 : 0;
    return 0;
}

extern "C" int sv_debug_rowln_plan(int32_t D, int32_t N, int32_t splitk, int32_t splitk_ru, int32_t num_cus, int32_t* out3) {
    if (!out3 || D < 16 || N < 1 || splitk < 1 || splitk_ru < 1 || num_cus < 1) return fail(SV_EINVAL, "sv_debug_rowln_plan: bad argument");
    const int Npad = round_up(N, 32);
    const bool fits = rowln_cattn_fits(D, Npad, D, splitk, splitk_ru, num_cus);
    out3[0] = fits ? 1 : 0;
    out3[1] = fits ? D / 16 / splitk / 8 : 0;
    out3[2] = 32 + (Npad / 32) * splitk;
    return 0;
}

extern "C" int sv_debug_skinny_plan(int32_t rows, int32_t N, int32_t K, int32_t splitk, int32_t wfmt, int32_t* out2) {
    if (!out2 || rows < 1 || N < 1 || K < 16 || K % 16 || splitk < 1 || (K / 16) % splitk || wfmt < 0 || wfmt > SV_WFMT_MXFP4)
        return fail(SV_EINVAL, "sv_debug_skinny_plan: bad argument");
    int waves = 0, two = 0;
    skinny_plan(round_up(N, 32), K, splitk, wfmt, (rows + 31) / 32, &waves, &two);
    out2[0] = waves; out2[1] = two;
    return 0;
}

extern "C" int sv_debug_decode_plan(int32_t rows, int32_t N, int32_t K, int32_t wfmt, int32_t whole_k, int32_t num_cus, int32_t* out2) {
    const bool fp8 = wfmt == SV_WFMT_FP8;
    if (!out2 || rows < 1 || rows > 64 || N < 1 || K < 16 || K % 16 || num_cus < 1 || wfmt < 0 || wfmt > SV_WFMT_MXFP4)
        return fail(SV_EINVAL, "sv_debug_decode_plan: bad argument");
    Linear l;
    l.N = N; l.K = K; l.Npad = round_up(N, 32); l.Kpad = K;
    int sk = 1, ct = 1;
    pick_decode_plan(l, (rows + 31) / 32, num_cus, wfmt, whole_k != 0, &sk, &ct);
    if (wfmt == SV_WFMT_MXFP4) while (sk > 1 && !skinny_waves_mxfp4(K / 16, sk)) --sk;                  // as sv_create does
    if (fp8) while (sk > 1 && ((K / 16) % sk != 0 || ((K / 16) / sk) % 4 != 0)) --sk;          // as sv_create does
    out2[0] = sk; out2[1] = ct;
    return 0;
}

extern "C" int sv_debug_rowln_occupancy(int32_t wide, int32_t* blocks_per_cu) {
    if (!blocks_per_cu) return fail(SV_EINVAL, "sv_debug_rowln_occupancy: null argument");
    *blocks_per_cu = rowln_cattn_blocks_per_cu(wide != 0);
    return 0;
}

extern "C" int sv_debug_attn_plan(int32_t max_batch, int32_t n_kv_head, int32_t num_cus, int32_t* out2) {
    if (!out2 || max_batch < 1 || n_kv_head < 1 || num_cus < 1) return fail(SV_EINVAL, "sv_debug_attn_plan: bad argument");
    out2[0] = attn_max_splits_of(max_batch, n_kv_head, num_cus);
    out2[1] = attn_groups_per_block_of(max_batch, n_kv_head, num_cus);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: the decode attention on its own, over an engine's REAL paged KV pool / block table / split plan.
// The e2e parity tests cannot discriminate at long contexts (with random weights the attention of thousands of keys is a few
// per cent of the residual stream); here the test chooses q / K / V itself (peaked softmax, needles on chosen pages).
// ------------------------------------------------------------------------------------------------
// dev_kv: bf16 [B][S][2 * n_kv * head_dim] rows (k heads | v heads) for tokens 0..S-1 of `layer` (K as it sits in the cache, i.e. already
// rotated for StarCoder2).  Assigns every row the pages of the whole max_seq_len, writes the rows, sets positions[b] = S -- or
// dev_lens[b] (int32 [B], each <= S) when given: a ragged batch, as continuous batching runs it.
extern "C" int sv_debug_kv_load(sv_engine* e, int32_t layer, const void* dev_kv, int32_t B, int32_t S, const int32_t* dev_lens,
                                sv_stream stream) {
    if (!e || (!dev_kv && S > 0)) return fail(SV_EINVAL, "sv_debug_kv_load: null argument");
    const sv_config& c = e->cfg;
    if (layer < 0 || layer >= c.n_layer || B < 1 || B > c.max_batch || S < 0 || S >= c.max_seq_len)
        return fail(SV_EINVAL, "sv_debug_kv_load: bad layer %d / B %d / S %d (max_batch %d, max_seq_len %d)", layer, B, S, c.max_batch, c.max_seq_len);
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, "sv_debug_kv_load"));
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    SVCHECK(assign_pages(e, B, c.max_seq_len, st));
    const int dh = e->dh, nkv = e->nkv;
    if (S > 0)
        for (int kh = 0; kh < nkv; ++kh)
            launch_kv_write_prefill((const bf16_t*)dev_kv, 2 * nkv * dh, kh * dh, nkv * dh + kh * dh,
                                    e->kv_pool + (size_t)layer * e->layer_stride + (size_t)kh * e->kv_head_stride,
                                    e->block_table, e->pages_per_seq, B, S, dh, st, e->kv_dtype);
    if (dev_lens) HIPCHECK(hipMemcpyAsync(e->positions, dev_lens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    else fill_i32(e->positions, S, B, st);
    e->cached_B = B;
    e->xpa_armed = false;                       // no lm_head launch in front of the step that follows
    e->dbg_pos_hi = S;                          // dev_lens[b] <= S by contract
    if (!dev_lens) {                            // (lengths on the device: the host does not know the contexts)
        e->ctx_len.assign((size_t)c.max_batch, 0); e->ctx_cap.assign((size_t)c.max_batch, 0);
        for (int b = 0; b < B; ++b) { e->ctx_len[b] = S; e->ctx_cap[b] = c.max_seq_len; }
        e->ctx_known = true;
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// dev_qkv_f32: fp32 [B][n_head*head_dim + 2*n_kv*head_dim] = the c_attn output of the NEW token (q heads | k heads | v heads, bias
// included, before RoPE); dev_out: bf16 [B][n_head*head_dim].  Runs attn_decode_kernel of `layer` exactly as a decode step does
// (same grid, split cap, groups per block, window, RoPE tables; the new K/V row is appended to the cache at positions[b]);
// advance != 0 steps positions[b] afterwards, so consecutive calls walk a sequence across page boundaries.
// One body for the two entries: `splitk` slabs dev_slabs fp32 [splitk][B][QKV] and an optional bf16 bias [QKV] (nullptr: zero).
static int debug_attn_decode(sv_engine* e, const char* who, int32_t layer, const float* dev_slabs, int32_t splitk, const void* dev_bias, int32_t B,
                             void* dev_out, int32_t advance, sv_stream stream) {
    if (!e || !dev_slabs || !dev_out) return fail(SV_EINVAL, "%s: null argument", who);
    const sv_config& c = e->cfg;
    if (layer < 0 || layer >= c.n_layer) return fail(SV_EINVAL, "%s: bad layer %d", who, layer);
    if (splitk != 1 && splitk != 2 && splitk != 4 && splitk != 8) return fail(SV_EINVAL, "%s: splitk %d is not 1, 2, 4 or 8", who, splitk);
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, who));
    if (B != e->cached_B) return fail(SV_ESTATE, "%s: B=%d but the cache holds %d sequences", who, B, e->cached_B);
    // the kernel appends the new K/V row at positions[b] and indexes the block table with it: repeated advancing calls must not walk
    // past the sequence's allocation
    if (e->dbg_pos_hi >= c.max_seq_len)
        return fail(SV_EINVAL, "%s: position %d would reach max_seq_len %d", who, e->dbg_pos_hi, c.max_seq_len);
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    bf16_t* bias;
    SVCHECK(tmp.get(&bias, (size_t)e->ldws));
    HIPCHECK(hipMemsetAsync(bias, 0, (size_t)e->ldws * sizeof(bf16_t), st));
    if (dev_bias) HIPCHECK(hipMemcpyAsync(bias, dev_bias, (size_t)e->QKV * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    // e->ws holds 8 slabs of rows_ws x ldws floats (sv_create): slab s of the caller lands where the c_attn GEMM's K slice s writes
    const int rows_ws = ((B + 31) / 32) * 32;
    for (int s = 0; s < splitk; ++s)
        HIPCHECK(hipMemcpy2DAsync(e->ws + (size_t)s * rows_ws * e->ldws, (size_t)e->ldws * sizeof(float), dev_slabs + (size_t)s * B * e->QKV,
                                  (size_t)e->QKV * sizeof(float), (size_t)e->QKV * sizeof(float), B, hipMemcpyDeviceToDevice, st));
    AttnDecodeArgs ad;
    attn_decode_args(e, layer, B, e->ws, splitk, bias, e->xp_attn, ad);
    launch_attn_decode(ad, st);
    unpack_rows(e->xp_attn, (bf16_t*)dev_out, c.n_head * e->dh, B, c.n_head * e->dh, st);
    if (advance) { add_i32(e->positions, 1, B, st); e->dbg_pos_hi += 1; e->ctx_known = false; }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));          // `bias` is freed on return
    return 0;
}

// tokens [first, first + count) of decode row `row` of `layer`, as the attention will see them: bf16 [count][2 * n_kv * head_dim] (k heads | v heads),
// from a pool of either format
extern "C" int sv_debug_kv_read(sv_engine* e, int32_t layer, int32_t row, int32_t first, int32_t count, void* dev_out_bf16, sv_stream stream) {
    if (!e || (!dev_out_bf16 && count > 0)) return fail(SV_EINVAL, "sv_debug_kv_read: null argument");
    const sv_config& c = e->cfg;
    if (layer < 0 || layer >= c.n_layer || row < 0 || row >= c.max_batch || first < 0 || count < 0 || (long long)first + count > c.max_seq_len)
        return fail(SV_EINVAL, "sv_debug_kv_read: bad layer %d / row %d / tokens [%d, %d + %d) (max_batch %d, max_seq_len %d)", layer, row, first, first, count,
                    c.max_batch, c.max_seq_len);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    KvReadArgs a;
    a.pool_layer = e->kv_pool + (size_t)layer * e->layer_stride; a.kv_head_stride = e->kv_head_stride;
    a.table_row = e->block_table + (size_t)row * e->pages_per_seq;
    a.n_kv = e->nkv; a.head_dim = e->dh; a.first = first; a.count = count; a.kv_fmt = e->kv_dtype; a.out = (bf16_t*)dev_out_bf16;
    launch_kv_read(a, st);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_debug_attn_decode(sv_engine* e, int32_t layer, const float* dev_qkv_f32, int32_t B, void* dev_out, int32_t advance,
                                    sv_stream stream) {
    return debug_attn_decode(e, "sv_debug_attn_decode", layer, dev_qkv_f32, 1, nullptr, B, dev_out, advance, stream);
}

// The same launch fed as a decode step feeds it: dev_slabs_f32 fp32 [splitk][B][QKV] = the split-K slabs of the c_attn GEMM (splitk 1, 2, 4
// or 8) and dev_bias bf16 [QKV] (NULL: zero); the kernel sums the slabs in slab order, then adds the bias.
extern "C" int sv_debug_attn_decode_slabs(sv_engine* e, int32_t layer, const float* dev_slabs_f32, int32_t splitk, const void* dev_bias, int32_t B,
                                          void* dev_out, int32_t advance, sv_stream stream) {
    return debug_attn_decode(e, "sv_debug_attn_decode_slabs", layer, dev_slabs_f32, splitk, dev_bias, B, dev_out, advance, stream);
}

// ------------------------------------------------------------------------------------------------
// Prompt-lookup decoding piece by piece (include/starvector_hip_debug.h)
// ------------------------------------------------------------------------------------------------
// What a verification step does around one attention launch, on the cache sv_debug_kv_load left: n_seq sequences -> n_seq x K1 rows (table rows
// copied, positions pos_s + j), the pre-write, ONE attention launch; then back to n_seq rows with every position advanced by K1.
extern "C" int sv_debug_attn_decode_draft(sv_engine* e, int32_t layer, const float* dev_slabs, int32_t splitk, const void* dev_bias, int32_t n_seq,
                                          int32_t K1, void* dev_out, sv_stream stream) {
    const char* who = "sv_debug_attn_decode_draft";
    if (!e || !dev_slabs || !dev_out) return fail(SV_EINVAL, "%s: null argument", who);
    if (e->kv_dtype != SV_KV_BF16) return fail(SV_ENOTSUP, "%s: the K / V pre-write of a verification step is not built for the fp8_e4m3 KV cache", who);
    const sv_config& c = e->cfg;
    if (layer < 0 || layer >= c.n_layer) return fail(SV_EINVAL, "%s: bad layer %d", who, layer);
    if (splitk != 1 && splitk != 2 && splitk != 4 && splitk != 8) return fail(SV_EINVAL, "%s: splitk %d is not 1, 2, 4 or 8", who, splitk);
    if (n_seq < 1 || K1 < 1 || K1 > SV_LOOKUP_MAX_DRAFT + 1 || (long long)n_seq * K1 > c.max_batch)
        return fail(SV_EINVAL, "%s: n_seq %d x K1 %d rows (K1 1..%d, max_batch %d)", who, n_seq, K1, SV_LOOKUP_MAX_DRAFT + 1, c.max_batch);
    std::lock_guard<std::mutex> lk(e->mu);
    SVCHECK(cb_guard(e, who));
    if (n_seq != e->cached_B) return fail(SV_ESTATE, "%s: n_seq=%d but the cache holds %d sequences", who, n_seq, e->cached_B);
    if (e->dbg_pos_hi + K1 > c.max_seq_len) return fail(SV_EINVAL, "%s: position %d would reach max_seq_len %d", who, e->dbg_pos_hi + K1 - 1, c.max_seq_len);
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    const int rows = n_seq * K1;
    const size_t mp = (size_t)e->pages_per_seq;
    if (e->table_pending) { HIPCHECK(hipEventSynchronize(e->table_ev)); e->table_pending = false; }
    std::vector<int32_t> table((size_t)rows * mp), pos0((size_t)n_seq), pos((size_t)rows);
    HIPCHECK(hipMemcpyAsync(pos0.data(), e->positions, (size_t)n_seq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int r = 0; r < rows; ++r) {
        memcpy(table.data() + (size_t)r * mp, e->h_table + (size_t)(r / K1) * mp, mp * sizeof(int32_t));
        pos[r] = pos0[r / K1] + r % K1;
        if (pos[r] < 0 || pos[r] >= c.max_seq_len) return fail(SV_ESTATE, "%s: position %d of row %d outside the sequence's pages", who, pos[r], r);
    }
    for (int s = 0; s < n_seq; ++s) pos0[s] += K1;
    HIPCHECK(hipMemcpyAsync(e->block_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(e->positions, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    TmpBufs tmp;
    bf16_t* bias;
    SVCHECK(tmp.get(&bias, (size_t)e->ldws));
    HIPCHECK(hipMemsetAsync(bias, 0, (size_t)e->ldws * sizeof(bf16_t), st));
    if (dev_bias) HIPCHECK(hipMemcpyAsync(bias, dev_bias, (size_t)e->QKV * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    const int rows_ws = ((rows + 31) / 32) * 32;
    for (int s = 0; s < splitk; ++s)
        HIPCHECK(hipMemcpy2DAsync(e->ws + (size_t)s * rows_ws * e->ldws, (size_t)e->ldws * sizeof(float), dev_slabs + (size_t)s * rows * e->QKV,
                                  (size_t)e->QKV * sizeof(float), (size_t)e->QKV * sizeof(float), rows, hipMemcpyDeviceToDevice, st));
    AttnDecodeArgs ad;
    attn_decode_args(e, layer, rows, e->ws, splitk, bias, e->xp_attn, ad);
    launch_lookup_kv_write(lookup_kv_args(ad), st);
    launch_attn_decode(ad, st);
    unpack_rows(e->xp_attn, (bf16_t*)dev_out, c.n_head * e->dh, rows, c.n_head * e->dh, st);
    // back to the n_seq-row layout (the host image still holds it), K1 positions further
    HIPCHECK(hipMemcpyAsync(e->block_table, e->h_table, (size_t)rows * mp * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(e->positions, pos0.data(), (size_t)n_seq * sizeof(int32_t), hipMemcpyHostToDevice, st));
    e->dbg_pos_hi += K1;
    e->ctx_known = false;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int sv_debug_set_lookup_drafts(sv_engine* e, const int32_t* host_stream, int32_t B, int32_t ld) {
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipDeviceSynchronize());                // no step in flight reads the buffer that goes
    e->lk_forced_B = 0; e->lk_forced_ld = 0;         // (the buffer stays: a kept graph of a forced call names its address)
    if (!host_stream) return 0;
    if (B < 1 || B > e->cfg.max_batch || ld < 1 || ld > e->cfg.max_seq_len)
        return fail(SV_EINVAL, "sv_debug_set_lookup_drafts: bad B %d / ld %d (max_batch %d, max_seq_len %d)", B, ld, e->cfg.max_batch, e->cfg.max_seq_len);
    for (size_t i = 0; i < (size_t)B * ld; ++i)      // a draft is fed to the embedding table
        if (host_stream[i] < 0 || host_stream[i] >= e->cfg.vocab)
            return fail(SV_EINVAL, "sv_debug_set_lookup_drafts: id %d outside the vocabulary (%d)", host_stream[i], e->cfg.vocab);
    if (!e->lk_forced) SVCHECK(dalloc(e, &e->lk_forced, (size_t)e->cfg.max_batch * e->cfg.max_seq_len));
    HIPCHECK(hipMemcpy(e->lk_forced, host_stream, (size_t)B * ld * sizeof(int32_t), hipMemcpyHostToDevice));
    e->lk_forced_B = B; e->lk_forced_ld = ld;
    return 0;
}
extern "C" int sv_op_lookup_accept(const int32_t* host_winners, const int32_t* host_rows, int32_t n_seq, int32_t K, int32_t max_ngram,
                                   int32_t min_ngram, int32_t* host_hist, int32_t ld, int32_t* host_state, int32_t* host_call,
                                   const int32_t* stop_ids, int32_t n_stop, int32_t eos, int32_t pad, int32_t max_new, int32_t vocab,
                                   int32_t* host_next_rows, int32_t* host_next_positions, sv_stream stream) {
    const char* who = "sv_op_lookup_accept";
    if (!host_winners || !host_rows || !host_hist || !host_state || !host_call || !host_next_rows || !host_next_positions)
        return fail(SV_EINVAL, "%s: null argument", who);
    if (n_seq < 1 || n_seq > 64 || K < 0 || K > SV_LOOKUP_MAX_DRAFT || max_ngram < 1 || max_ngram > SV_LOOKUP_MAX_NGRAM || min_ngram < 1 ||
        min_ngram > max_ngram || max_new < 1 || ld < max_new || vocab < 1 || n_stop < 0 || n_stop > 16 || (n_stop > 0 && !stop_ids))
        return fail(SV_EINVAL, "%s: bad shape (n_seq %d, K %d, n-grams %d..%d, max_new %d, ld %d, vocab %d, n_stop %d)", who, n_seq, K, min_ngram,
                    max_ngram, max_new, ld, vocab, n_stop);
    const int K1 = K + 1, rows = n_seq * K1;
    for (int s = 0; s < n_seq; ++s) {
        const int32_t* q = host_state + 4 * s;
        if (q[0] < 0 || q[0] > max_new || q[3] < 0 || q[3] > K || (!q[1] && q[0] + q[3] + 1 > max_new))
            return fail(SV_EINVAL, "%s: sequence %d: n_emit %d with %d live drafts does not fit max_new %d", who, s, q[0], q[3], max_new);
    }
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t *d_i;
    float* d_val;
    // one int32 block: state (counts[3] | n_emit | fin | base | n_draft | limit | ticket) | call {step, done, n_emitted, bad} | rows | positions | pidx | hist | stop
    const size_t o_call = 4 * (size_t)n_seq + 8, o_rows = o_call + 4, o_pos = o_rows + rows, o_idx = o_pos + rows, o_hist = o_idx + (size_t)rows * 8,
                 o_stop = o_hist + (size_t)n_seq * ld, total = o_stop + 16;
    SVCHECK(tmp.get(&d_i, total));
    SVCHECK(tmp.get(&d_val, (size_t)rows * 8));
    std::vector<int32_t> h(total, 0);
    std::vector<float> hv((size_t)rows * 8, -INFINITY);
    int32_t* n_emit = h.data() + 3;
    for (int s = 0; s < n_seq; ++s) {
        n_emit[s] = host_state[4 * s]; n_emit[n_seq + s] = host_state[4 * s + 1]; n_emit[2 * n_seq + s] = host_state[4 * s + 2];
        n_emit[3 * n_seq + s] = host_state[4 * s + 3];
    }
    h[0] = host_call[4]; h[1] = host_call[5]; h[2] = host_call[6];
    h[3 + 4 * (size_t)n_seq] = host_call[0];
    h[o_call + 1] = host_call[1]; h[o_call + 2] = host_call[2]; h[o_call + 3] = host_call[3];
    for (int r = 0; r < rows; ++r) {
        h[o_rows + r] = host_rows[r];
        h[o_pos + r] = host_next_positions[r];          // in / out: a sequence that is finished keeps its rows as they are
        for (int i = 0; i < 8; ++i) h[o_idx + (size_t)r * 8 + i] = 0x7fffffff;
        h[o_idx + (size_t)r * 8 + (r & 7)] = host_winners[r];          // the winner sits in some slice, the others hold nothing
        hv[(size_t)r * 8 + (r & 7)] = 1.f;
    }
    memcpy(h.data() + o_hist, host_hist, (size_t)n_seq * ld * sizeof(int32_t));
    for (int i = 0; i < n_stop; ++i) h[o_stop + i] = stop_ids[i];
    HIPCHECK(hipMemcpyAsync(d_i, h.data(), total * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_val, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice, st));
    LookupArgs a;
    memset(&a, 0, sizeof(a));
    a.counts = d_i; a.n_emit = d_i + 3; a.fin = a.n_emit + n_seq; a.base = a.fin + n_seq; a.n_draft = a.base + n_seq; a.limit = a.n_draft + n_seq;
    a.ticket = reinterpret_cast<unsigned*>(a.limit + 1);
    a.n_seq = n_seq; a.K = K; a.max_ngram = max_ngram; a.min_ngram = min_ngram;
    a.cur_tok = d_i + o_rows; a.positions = d_i + o_pos; a.out_tok = d_i + o_hist; a.ld_out = ld; a.pval = d_val; a.pidx = d_i + o_idx;
    a.done = d_i + o_call + 1; a.n_emitted = d_i + o_call + 2; a.bad = d_i + o_call + 3;
    a.stop_ids = d_i + o_stop; a.n_stop = n_stop; a.eos = eos; a.pad = pad; a.max_new = max_new; a.V = vocab;
    launch_lookup_step(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(h.data(), d_i, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int s = 0; s < n_seq; ++s) {
        host_state[4 * s] = n_emit[s]; host_state[4 * s + 1] = n_emit[n_seq + s]; host_state[4 * s + 2] = n_emit[2 * n_seq + s];
        host_state[4 * s + 3] = n_emit[3 * n_seq + s];
    }
    host_call[0] = h[3 + 4 * (size_t)n_seq]; host_call[1] = h[o_call + 1]; host_call[2] = h[o_call + 2]; host_call[3] = h[o_call + 3];
    host_call[4] = h[0]; host_call[5] = h[1]; host_call[6] = h[2]; host_call[7] = 0;
    memcpy(host_next_rows, h.data() + o_rows, (size_t)rows * sizeof(int32_t));
    memcpy(host_next_positions, h.data() + o_pos, (size_t)rows * sizeof(int32_t));
    memcpy(host_hist, h.data() + o_hist, (size_t)n_seq * ld * sizeof(int32_t));
    return 0;
}
// the lookup alone: one step that re-emits the history's last id with no draft in flight, then drafts behind the L ids
extern "C" int sv_op_lookup_draft(const int32_t* host_hist, int32_t L, int32_t K, int32_t max_ngram, int32_t min_ngram, int32_t max_new,
                                  int32_t* host_drafts, int32_t* n_drafts, sv_stream stream) {
    if (!host_hist || !host_drafts || !n_drafts) return fail(SV_EINVAL, "sv_op_lookup_draft: null argument");
    if (L < 1 || L > max_new || K < 1 || K > SV_LOOKUP_MAX_DRAFT) return fail(SV_EINVAL, "sv_op_lookup_draft: bad L %d / K %d (max_new %d)", L, K, max_new);
    std::vector<int32_t> hist(host_hist, host_hist + L), win((size_t)K + 1, host_hist[L - 1]), rows((size_t)K + 1, 0), nrows((size_t)K + 1), npos((size_t)K + 1);
    hist.resize((size_t)max_new, 0);
    int32_t state[4] = {L - 1, 0, 0, 0}, call[8] = {max_new, 0, 0, 0, 0, 0, 0, 0};
    SVCHECK(sv_op_lookup_accept(win.data(), rows.data(), 1, K, max_ngram, min_ngram, hist.data(), max_new, state, call, nullptr, 0, -1, 0, max_new,
                                0x7fffffff, nrows.data(), npos.data(), stream));
    *n_drafts = state[3];
    for (int j = 0; j < state[3]; ++j) host_drafts[j] = nrows[(size_t)j + 1];
    return 0;
}
extern "C" int sv_op_lookup_hold(float* dev_logits, int32_t ld, int32_t rows, int32_t K1, int32_t eos, int32_t min_new, const int32_t* host_n_emit,
                                 sv_stream stream) {
    if (!dev_logits || !host_n_emit) return fail(SV_EINVAL, "sv_op_lookup_hold: null argument");
    if (rows < 1 || K1 < 1 || rows % K1 != 0 || eos < 0 || eos >= ld) return fail(SV_EINVAL, "sv_op_lookup_hold: bad rows %d / K1 %d / eos %d (ld %d)", rows, K1, eos, ld);
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t* d_n;
    SVCHECK(tmp.get(&d_n, (size_t)(rows / K1)));
    HIPCHECK(hipMemcpyAsync(d_n, host_n_emit, (size_t)(rows / K1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    launch_lookup_hold_eos(dev_logits, ld, eos, d_n, K1, min_new, rows, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}
// sv_generate_lookup_sampled's draw on caller-given rows (lookup_sampled/lookup_sampled.hip)
extern "C" int sv_op_lookup_sample(const float* dev_logits, int32_t rows, int32_t V, int32_t ld, int32_t K1, const int32_t* host_n_emit, float temperature,
                                   int32_t top_k, float top_p, uint64_t seed, const uint32_t* host_seen, int32_t seen_words, float penalty,
                                   int32_t* host_tokens, float* host_pval8, int32_t* host_pidx8, sv_stream stream) {
    const char* who = "sv_op_lookup_sample";
    if (!dev_logits || !host_n_emit || !host_tokens) return fail(SV_EINVAL, "%s: null argument", who);
    if (rows < 1 || rows > (1 << 16) || K1 < 1 || K1 > SV_LOOKUP_MAX_DRAFT + 1 || rows % K1 != 0 || V < 1 || ld < V)
        return fail(SV_EINVAL, "%s: bad rows %d / K1 %d / V %d (ld %d)", who, rows, K1, V, ld);
    if (!(temperature > 0.f) || !(top_p > 0.f)) return fail(SV_EINVAL, "%s: temperature and top_p must be > 0", who);
    if (host_seen && (seen_words < (V + 31) / 32 || !(penalty > 0.f))) return fail(SV_EINVAL, "%s: seen_words %d below vocab / 32, or penalty <= 0", who, seen_words);
    const int n_seq = rows / K1;
    for (int s = 0; s < n_seq; ++s)
        if (host_n_emit[s] < 0) return fail(SV_EINVAL, "%s: n_emit %d of sequence %d", who, host_n_emit[s], s);
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t *d_n, *d_idx;
    float* d_val;
    uint32_t* d_seen = nullptr;
    SVCHECK(tmp.get(&d_n, (size_t)n_seq));
    SVCHECK(tmp.get(&d_idx, (size_t)rows * 8));
    SVCHECK(tmp.get(&d_val, (size_t)rows * 8));
    HIPCHECK(hipMemcpyAsync(d_n, host_n_emit, (size_t)n_seq * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (host_seen) {
        SVCHECK(tmp.get(&d_seen, (size_t)rows * seen_words));
        HIPCHECK(hipMemcpyAsync(d_seen, host_seen, (size_t)rows * seen_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    LookupSampleArgs a;
    a.logits = dev_logits; a.ld = ld; a.V = V; a.rows = rows; a.K1 = K1; a.n_emit = d_n; a.done = nullptr;
    a.temperature = temperature; a.top_p = top_p; a.top_k = top_k; a.seed = seed;
    a.seen = d_seen; a.seen_words = seen_words; a.penalty = host_seen ? penalty : 1.f; a.pval = d_val; a.pidx = d_idx;
    launch_lookup_sample(a, st);
    HIPCHECK(hipGetLastError());
    std::vector<float> hv((size_t)rows * 8);
    std::vector<int32_t> hi((size_t)rows * 8);
    HIPCHECK(hipMemcpyAsync(hv.data(), d_val, hv.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(hi.data(), d_idx, hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int r = 0; r < rows; ++r) {                 // lookup_step_kernel's merge: the largest value, the lowest index on a tie
        float best = -INFINITY;
        int32_t nxt = 0x7fffffff;
        for (int i = 0; i < 8; ++i) {
            const float ov = hv[(size_t)r * 8 + i];
            const int32_t oi = hi[(size_t)r * 8 + i];
            if (ov > best || (ov == best && oi < nxt)) { best = ov; nxt = oi; }
        }
        host_tokens[r] = nxt;
    }
    if (host_pval8) memcpy(host_pval8, hv.data(), hv.size() * sizeof(float));
    if (host_pidx8) memcpy(host_pidx8, hi.data(), hi.size() * sizeof(int32_t));
    return 0;
}
// the seen sets of a verification step on given state (lookup_seen_kernel)
extern "C" int sv_op_lookup_seen(const int32_t* host_hist, int32_t ld, int32_t n_seq, int32_t K1, int32_t words, const int32_t* host_L_before,
                                 const int32_t* host_L_after, const int32_t* host_n_draft, const int32_t* host_rows, uint32_t* host_seq_seen,
                                 uint32_t* host_row_seen, sv_stream stream) {
    const char* who = "sv_op_lookup_seen";
    if (!host_hist || !host_L_before || !host_L_after || !host_n_draft || !host_rows || !host_seq_seen || !host_row_seen)
        return fail(SV_EINVAL, "%s: null argument", who);
    if (n_seq < 1 || n_seq > 64 || K1 < 1 || K1 > SV_LOOKUP_MAX_DRAFT + 1 || words < 1 || words > 16384 || ld < 1)
        return fail(SV_EINVAL, "%s: bad shape (n_seq %d, K1 %d, words %d, ld %d)", who, n_seq, K1, words, ld);
    for (int s = 0; s < n_seq; ++s)
        if (host_L_before[s] < 0 || host_L_after[s] < host_L_before[s] || host_L_after[s] > ld || host_n_draft[s] < 0 || host_n_draft[s] > K1 - 1)
            return fail(SV_EINVAL, "%s: sequence %d: columns %d..%d of %d, %d live drafts of %d", who, s, host_L_before[s], host_L_after[s], ld,
                        host_n_draft[s], K1 - 1);
    hipStream_t st = (hipStream_t)stream;
    const int rows = n_seq * K1;
    TmpBufs tmp;
    int32_t* d_i;      // cols | n_emit | n_draft | rows | hist
    uint32_t *d_seq, *d_row;
    const size_t o_emit = (size_t)n_seq, o_nd = 2 * (size_t)n_seq, o_rows = 3 * (size_t)n_seq, o_hist = o_rows + rows, total = o_hist + (size_t)n_seq * ld;
    SVCHECK(tmp.get(&d_i, total));
    SVCHECK(tmp.get(&d_seq, (size_t)n_seq * words));
    SVCHECK(tmp.get(&d_row, (size_t)rows * words));
    std::vector<int32_t> h(total);
    for (int s = 0; s < n_seq; ++s) { h[s] = host_L_before[s]; h[o_emit + s] = host_L_after[s]; h[o_nd + s] = host_n_draft[s]; }
    memcpy(h.data() + o_rows, host_rows, (size_t)rows * sizeof(int32_t));
    memcpy(h.data() + o_hist, host_hist, (size_t)n_seq * ld * sizeof(int32_t));
    HIPCHECK(hipMemcpyAsync(d_i, h.data(), total * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_seq, host_seq_seen, (size_t)n_seq * words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(d_row, 0, (size_t)rows * words * sizeof(uint32_t), st));
    LookupSeenArgs a;
    a.seq_seen = d_seq; a.seq_cols = d_i; a.row_seen = d_row; a.words = words; a.n_seq = n_seq; a.K1 = K1; a.begin = 0;
    a.n_emit = d_i + o_emit; a.n_draft = d_i + o_nd; a.cur_tok = d_i + o_rows; a.out_tok = d_i + o_hist; a.ld_out = ld; a.done = nullptr;
    launch_lookup_seen(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(host_seq_seen, d_seq, (size_t)n_seq * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(host_row_seen, d_row, (size_t)rows * words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// SV_MLP_TRACE=1 at sv_create: wall-clock stamps (100 MHz ticks) of the fused MLP launch of the middle layer of the LAST decode step,
// host_out [blocks][8] = {start, c_fc loop done, tile published, slice complete, end, XCC id, 0, 0}; returns the number of blocks
extern "C" int sv_debug_mlp_trace(sv_engine* e, int64_t* host_out, int32_t capacity_blocks) {
    if (!e || !host_out) return fail(SV_EINVAL, "sv_debug_mlp_trace: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->mlp_trace) return fail(SV_ESTATE, "sv_debug_mlp_trace: the engine was not created with SV_MLP_TRACE=1 (or the fused MLP launch does not fit it)");
    const int T1 = e->dec[0].c_fc.Npad / 32;
    if (capacity_blocks < T1) return fail(SV_EINVAL, "sv_debug_mlp_trace: capacity %d < %d blocks", capacity_blocks, T1);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(host_out, e->mlp_trace, (size_t)T1 * 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return T1;
}

// SV_ATTN_TRACE=1 at sv_create: wall-clock stamps (100 MHz ticks) of the decode attention launch of the middle layer of the LAST decode step,
// host_out [rows * kv heads * splits][16] = {start, first KV group requested, q in LDS, key groups processed, partial stored + drained, ticket
// drawn, end (0: not the merging block), active splits, key groups, 0...}; an all-zero row = an inactive split.  Returns the number of rows.
extern "C" int sv_debug_attn_trace(sv_engine* e, int64_t* host_out, int32_t capacity_rows) {
    if (!e || !host_out) return fail(SV_EINVAL, "sv_debug_attn_trace: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->attn_trace) return fail(SV_ESTATE, "sv_debug_attn_trace: the engine was not created with SV_ATTN_TRACE=1");
    const int rows = e->cached_B * e->nkv * attn_max_splits_of(e->cfg.max_batch, e->nkv, e->num_cus);
    if (rows < 1 || capacity_rows < rows) return fail(SV_EINVAL, "sv_debug_attn_trace: capacity %d < %d rows", capacity_rows, rows);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(host_out, e->attn_trace, (size_t)rows * 16 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return rows;
}

// host_out[blocks]: the XCC_ID each block of a 1-D launch of 8-wave blocks ran on (heavy = 1: with the decode attention's LDS footprint and
// 10 us of residence, so that a grid above the CU count is dispatched in rounds).
extern "C" int sv_debug_xcc_map(sv_engine* e, int32_t blocks, int32_t heavy, int32_t* host_out) {
    if (!e || !host_out || blocks < 1 || blocks > (1 << 16)) return fail(SV_EINVAL, "sv_debug_xcc_map: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    int32_t* d = nullptr;
    HIPCHECK(hipMalloc((void**)&d, (size_t)blocks * 4));
    int rc = launch_xcc_probe(d, blocks, heavy, nullptr);
    if (!rc && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_out, d, (size_t)blocks * 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    (void)hipFree(d);
    if (rc) return fail(SV_EHIP, "sv_debug_xcc_map: probe launch failed");
    return 0;
}

// A foreign tenant for the safety tests: `blocks` blocks that each pin `lds_bytes` of LDS on a CU for `ms` milliseconds, launched on a
// stream of their own; returns at once.  The caller then decodes on the same GPU.
extern "C" int sv_debug_occupy_cus(sv_engine* e, int32_t blocks, int32_t lds_bytes, int32_t ms) {
    if (!e || blocks < 1 || blocks > 4096 || lds_bytes < 1024 || lds_bytes > 160 * 1024 || ms < 1 || ms > 5000)
        return fail(SV_EINVAL, "sv_debug_occupy_cus: blocks 1..4096, lds_bytes 1 KiB..160 KiB, ms 1..5000");
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    if (!e->tenant_stream) HIPCHECK(hipStreamCreateWithFlags(&e->tenant_stream, hipStreamNonBlocking));      // kept: hipStreamDestroy would wait for the kernel
    const int rc = launch_occupy(blocks, lds_bytes, ms * 100000, e->tenant_stream);
    if (rc) return fail(SV_EHIP, "sv_debug_occupy_cus: launch failed (%d)", rc);
    return 0;
}

extern "C" int sv_debug_set_gemm_form(int32_t form) {
    if (form < -1 || form > 3) return fail(SV_EINVAL, "sv_debug_set_gemm_form: -1 (tuned), 0 .. 3");
    set_gemm_form(form);
    return 0;
}

// sequence structure sv_op_linear / sv_bench_linear hand to the big-M dispatch (GemmArgs::seq_rows; 0 = none): the test surface of
// the per-sequence remainder (gemm_tailk_kernel)
static std::atomic<int> g_op_seq_rows{0};
extern "C" int sv_debug_set_linear_seq_rows(int32_t seq_rows) {
    if (seq_rows < -65536 || seq_rows > 65536) return fail(SV_EINVAL, "sv_debug_set_linear_seq_rows: |S| <= 65536");
    g_op_seq_rows = seq_rows;
    return 0;
}

extern "C" int sv_debug_set_col_tiles(int32_t col_tiles) {
    if (col_tiles < 0 || col_tiles > 3) return fail(SV_EINVAL, "sv_debug_set_col_tiles: 0..3");
    g_op_col_tiles = col_tiles;
    return 0;
}

extern "C" int sv_debug_cols_rowhalf_launches(int64_t* launches, int64_t* halves) {
    if (!launches || !halves) return fail(SV_EINVAL, "sv_debug_cols_rowhalf_launches: null argument");
    long long l = 0, h = 0;
    cols_rowhalf_launches(&l, &h);
    *launches = (int64_t)l; *halves = (int64_t)h;
    return 0;
}
extern "C" int sv_debug_tailsplit_launches(int64_t* count) {
    if (!count) return fail(SV_EINVAL, "sv_debug_tailsplit_launches: null argument");
    *count = (int64_t)tailsplit_launches();
    return 0;
}

extern "C" int sv_debug_set_skinny_form(int32_t form) {
    if (form < 0 || form > 3) return fail(SV_EINVAL, "sv_debug_set_skinny_form: 0..3");
    set_mt2x(form);
    return 0;
}
extern "C" int sv_debug_skinny_form(void) { return get_mt2x(); }

// 1 / 0: does the projection (N, K, act) take the per-sequence remainder form for sequences of S rows (host arithmetic only; < 0: bad argument)
extern "C" int sv_debug_gemm_seq_form(int32_t S, int32_t N, int32_t K, int32_t act) {
    if (S < 1 || N < 1 || K < 1) return fail(SV_EINVAL, "sv_debug_gemm_seq_form: bad argument");
    return gemm_seq_form(S, N, K, act) ? 1 : 0;
}

extern "C" int sv_debug_ragged_plan(const int32_t* lens, int32_t B, int32_t N, int32_t K, int32_t act, int32_t q_tile, int32_t* rows_out,
                                    int32_t* last_out, int32_t capacity, int32_t* out4) {
    if (!lens || !rows_out || !last_out || !out4) return fail(SV_EINVAL, "sv_debug_ragged_plan: null argument");
    if (B < 1 || N < 1 || K < 1 || (q_tile != 32 && q_tile != 128)) return fail(SV_EINVAL, "sv_debug_ragged_plan: bad argument (B %d, N %d, K %d, q_tile %d)", B, N, K, q_tile);
    if (capacity < 3 * B) return fail(SV_EINVAL, "sv_debug_ragged_plan: capacity %d < 3 * B", capacity);
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1) return fail(SV_EINVAL, "sv_debug_ragged_plan: length %d of sequence %d", lens[b], b);
    PackedPlan pp;
    const PlanProj pj{N, K, act};
    ragged_plan(lens, B, q_tile, &pj, 1, nullptr, pp);
    std::copy(pp.rows(0).begin(), pp.rows(0).end(), rows_out);
    std::copy(pp.last(0).begin(), pp.last(0).end(), last_out);
    out4[0] = (int32_t)pp.rows(0).size(); out4[1] = (int32_t)pp.last(0).size();
    out4[2] = (int32_t)pp.list[PL_BLOCKS0].size() / 2; out4[3] = (int32_t)pp.list[PL_KV_BLOCKS].size() / 2;
    return 0;
}
extern "C" int sv_debug_prompt_passes(sv_engine* e, int64_t* out) {
    if (!e || !out) return fail(SV_EINVAL, "sv_debug_prompt_passes: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    *out = e->prompt_passes;
    return 0;
}

extern "C" int sv_debug_shared_plan(const int32_t* lens, int32_t n_prompts, const int32_t* group, const int32_t* budgets, int32_t n,
                                    int32_t* shared_out, int32_t* private_out, int64_t* total_out) {
    if (!budgets || !shared_out || !private_out || !total_out) return fail(SV_EINVAL, "sv_debug_shared_plan: null argument");
    SVCHECK(shared_check_group("sv_debug_shared_plan", lens, n_prompts, group, n));
    for (int i = 0; i < n; ++i)
        if (budgets[i] < 1) return fail(SV_EINVAL, "sv_debug_shared_plan: budgets[%d] = %d (must be >= 1)", i, budgets[i]);
    *total_out = shared_page_plan(lens, n_prompts, group, budgets, n, shared_out, private_out);
    return 0;
}
extern "C" int sv_debug_block_table(sv_engine* e, int32_t row, int32_t* host_out, int32_t capacity) {
    if (!e || !host_out) return fail(SV_EINVAL, "sv_debug_block_table: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (row < 0 || row >= e->cfg.max_batch) return fail(SV_EINVAL, "sv_debug_block_table: row %d outside [0, max_batch %d)", row, e->cfg.max_batch);
    if (capacity < e->pages_per_seq) return fail(SV_EINVAL, "sv_debug_block_table: capacity %d < %d pages per sequence", capacity, e->pages_per_seq);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipMemcpyAsync(host_out, e->block_table + (size_t)row * e->pages_per_seq, e->pages_per_seq * sizeof(int32_t), hipMemcpyDeviceToHost, e->gen_stream));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    return e->pages_per_seq;
}
extern "C" int sv_debug_free_pages(sv_engine* e, int32_t* free_out, int32_t* total_out) {
    if (!e || !free_out || !total_out) return fail(SV_EINVAL, "sv_debug_free_pages: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    *free_out = (int32_t)e->free_pages.size();
    *total_out = e->num_pages;
    return 0;
}

extern "C" int sv_debug_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t act, int32_t* out5) {
    if (!out5 || M < 1 || N < 1 || K < 1) return fail(SV_EINVAL, "sv_debug_gemm_plan: bad argument");
    const GemmPlan pl = gemm_plan(M, N, K, act, 1);
    out5[0] = pl.peel; out5[1] = pl.tail_rows; out5[2] = pl.tail_by_tiles; out5[3] = pl.main_256;
    out5[4] = (int32_t)(pl.est_us + 0.5);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: image pre-processing on device (no engine handle: it depends on nothing but the pixels)
// ------------------------------------------------------------------------------------------------
extern "C" int sv_preprocess_image(const uint8_t* dev_pixels, int32_t width, int32_t height, int32_t channels,
                                   int32_t out_size, int32_t recipe, const float* mean3, const float* std3,
                                   float* dev_out, sv_stream stream) {
    if (recipe != 0 && recipe != 1) return fail(SV_EINVAL, "sv_preprocess_image: recipe must be 0 (ImageTrainProcessor) or 1 (SigLIP processor)");
    if (!dev_pixels || !dev_out || !mean3 || !std3) return fail(SV_EINVAL, "sv_preprocess_image: null argument");
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(SV_EINVAL, "sv_preprocess_image: bad image size %dx%d", width, height);
    if (channels != 3 && channels != 4) return fail(SV_EINVAL, "sv_preprocess_image: channels must be 3 (RGB) or 4 (RGBA), got %d", channels);
    if (out_size < 1 || out_size > 4096) return fail(SV_EINVAL, "sv_preprocess_image: bad output size %d", out_size);
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] > 0.f)) return fail(SV_EINVAL, "sv_preprocess_image: std must be positive");
    const int r = preprocess_image(dev_pixels, width, height, channels, out_size, recipe, mean3, std3, dev_out, (hipStream_t)stream);
    if (r) return fail(SV_EHIP, "sv_preprocess_image: %s", hipGetErrorString((hipError_t)r));
    return 0;
}

extern "C" int64_t sv_preprocess_workspace_bytes(const int32_t* widths, const int32_t* heights, int32_t n, int32_t out_size,
                                                 int32_t recipe) {
    if (!widths || !heights || n < 1 || out_size < 1 || out_size > 4096 || (recipe != 0 && recipe != 1)) return fail(SV_EINVAL, "sv_preprocess_workspace_bytes: bad argument");
    for (int i = 0; i < n; ++i)
        if (widths[i] < 1 || heights[i] < 1 || widths[i] > 16384 || heights[i] > 16384) return fail(SV_EINVAL, "sv_preprocess_workspace_bytes: bad image size %dx%d", widths[i], heights[i]);
    return (int64_t)preprocess_workspace_bytes(widths, heights, n, out_size, recipe);
}

extern "C" int sv_preprocess_images(const uint8_t* const* dev_pixels, const int32_t* widths, const int32_t* heights,
                                    const int32_t* channels, int32_t n, int32_t out_size, int32_t recipe, const float* mean3,
                                    const float* std3, float* dev_out, void* dev_workspace, int64_t workspace_bytes,
                                    sv_stream stream) {
    if (recipe != 0 && recipe != 1) return fail(SV_EINVAL, "sv_preprocess_images: recipe must be 0 (ImageTrainProcessor) or 1 (SigLIP processor)");
    if (!dev_pixels || !widths || !heights || !channels || !dev_out || !mean3 || !std3 || n < 1) return fail(SV_EINVAL, "sv_preprocess_images: null argument or empty batch");
    if (out_size < 1 || out_size > 4096) return fail(SV_EINVAL, "sv_preprocess_images: bad output size %d", out_size);
    for (int i = 0; i < n; ++i) {
        if (!dev_pixels[i]) return fail(SV_EINVAL, "sv_preprocess_images: image %d is null", i);
        if (widths[i] < 1 || heights[i] < 1 || widths[i] > 16384 || heights[i] > 16384) return fail(SV_EINVAL, "sv_preprocess_images: bad image size %dx%d", widths[i], heights[i]);
        if (channels[i] != 3 && channels[i] != 4) return fail(SV_EINVAL, "sv_preprocess_images: channels must be 3 (RGB) or 4 (RGBA), got %d", channels[i]);
    }
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] > 0.f)) return fail(SV_EINVAL, "sv_preprocess_images: std must be positive");
    const size_t need = preprocess_workspace_bytes(widths, heights, n, out_size, recipe);
    if (workspace_bytes < 0 || (size_t)workspace_bytes < need || (!dev_workspace && need > 256))
        return fail(SV_EINVAL, "sv_preprocess_images: workspace of %lld bytes, %zu needed (sv_preprocess_workspace_bytes)", (long long)workspace_bytes, need);
    const int r = preprocess_images(dev_pixels, widths, heights, channels, n, out_size, recipe, mean3, std3, dev_out, dev_workspace,
                                    (size_t)workspace_bytes, (hipStream_t)stream);
    if (r) return fail(SV_EHIP, "sv_preprocess_images: %s", r < 0 ? "workspace too small" : hipGetErrorString((hipError_t)r));
    return 0;
}

// Per-kernel timing of the decode step with HIP events on the engine stream (eager launches of the
// same kernels the graph replays).  Uses the KV cache / positions left by the last generate or prefill.
// out[2*k] = milliseconds per step spent in kernel class k, out[2*k+1] = launches per step,
// k in {0: skinny GEMM, 1: decode attention, 2: row update + LayerNorm, 3: lm_head-to-end marker}.
extern "C" int sv_profile_decode_step(sv_engine* e, int32_t B, int32_t iters, double* out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!out || iters < 1) return fail(SV_EINVAL, "sv_profile_decode_step: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (B != e->cached_B) return fail(SV_ESTATE, "sv_profile_decode_step: B=%d but the cache holds %d sequences", B, e->cached_B);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipEventRecord(e->gen_event, (hipStream_t)stream));
    hipStream_t st = e->gen_stream;
    HIPCHECK(hipStreamWaitEvent(st, e->gen_event, 0));
    // positions may sit one past the budget after a full generate: step back so the probe stays in range
    add_i32(e->positions, -1, B, st);
    struct PosGuard { sv_engine* e; int B; hipStream_t st; ~PosGuard() { add_i32(e->positions, 1, B, st); (void)hipStreamSynchronize(st); } } pg{e, B, st};
    for (int k = 0; k < 2 * PK_COUNT + 2; ++k) out[k] = 0.0;
    // event-pair overhead: two back-to-back events with nothing in between
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
    for (int it = 0; it < iters + 1; ++it) {
        e->prof_on = true; e->prof_used = 0;
        decode_forward(e, B, st);
        e->prof_on = false;                  // (no HIP call that can return sits between the two assignments)
        HIPCHECK(hipStreamSynchronize(st));
        if (it == 0) continue;              // warm-up pass (also creates the events)
        for (size_t i = 0; i + 1 < e->prof_used; ++i) {
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]));
            double d = (double)ms - overhead_ms;      // an event pair with nothing in between costs ~4 us
            if (d < 0) d = 0;
            out[2 * e->prof_kind[i]] += d;
            out[2 * e->prof_kind[i] + 1] += 1.0;
        }
    }
    for (int k = 0; k < 2 * PK_COUNT; ++k) out[k] /= (double)iters;
    out[2 * PK_SAMPLE] = overhead_ms;         // slot 6: time between two back-to-back events with no kernel
    // slot 7: the step's weight-streaming GEMMs alone, back to back between ONE event pair: average
    // dispatch-to-dispatch time per launch (what rocprofv3's kernel trace calls the kernel duration)
    // slot 8: the complement -- every other kernel of the step (row updates, attention) back to back, no GEMMs.  The step
    // minus this chain is what the GEMMs cost IN SITU (bench.py's roofline.avg_launch_us)
    // The two filters are engine state read by decode_forward: the guard clears them and destroys the events on EVERY exit,
    // so a failed HIP call in here can never leave a live engine that silently skips its GEMMs.
    struct ChainGuard {
        sv_engine* e; hipEvent_t a = nullptr, b = nullptr;
        ~ChainGuard() { e->only_skinny = false; e->skip_skinny = false; if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } cg{e};
    HIPCHECK(hipEventCreate(&cg.a)); HIPCHECK(hipEventCreate(&cg.b));
    for (int leg = 0; leg < 2; ++leg) {
        e->only_skinny = leg == 0;
        e->skip_skinny = leg == 1;
        decode_forward(e, B, st);
        HIPCHECK(hipEventRecord(cg.a, st));
        for (int it = 0; it < iters; ++it) decode_forward(e, B, st);
        HIPCHECK(hipEventRecord(cg.b, st));
        e->only_skinny = false; e->skip_skinny = false;
        HIPCHECK(hipEventSynchronize(cg.b));
        float ms = 0.f; HIPCHECK(hipEventElapsedTime(&ms, cg.a, cg.b));
        out[leg == 0 ? 2 * PK_SAMPLE + 1 : 2 * PK_COUNT] = (double)ms / iters;       // ms per step for the chain
    }
    return 0;           // ~PosGuard steps the positions forward again and drains the stream
}

extern "C" int sv_last_timing(sv_engine* e, double* out3) {   /* 4 doubles */
    if (!e || !out3) return fail(SV_EINVAL, "null argument");
    out3[0] = e->timing[0]; out3[1] = e->timing[1]; out3[2] = e->timing[2]; out3[3] = e->timing_graph;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI: single operators (test surface)
// ------------------------------------------------------------------------------------------------

extern "C" int sv_op_layernorm(const void* x, const void* gamma, const void* beta, void* y, int32_t M, int32_t D,
                               float eps, sv_stream stream) {
    if (!x || !gamma || !beta || !y || M < 1 || D < 8 || D % 8) return fail(SV_EINVAL, "sv_op_layernorm: bad argument");
    launch_layernorm_rows((const bf16_t*)x, D, (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, D, M, D, eps,
                          (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

// the big-M Linear behind sv_op_linear (fp8 == 0) and sv_op_linear_fp8 (fp8 != 0: the weight quantised as sv_load_weight does it, the GEMM on the
// bf16 image of the quantised values with the row scales as GemmArgs::cscale -- what an fp8 engine's prompt pass launches)
static int op_linear_run(const void* x, const void* W, const void* bias, const void* residual, void* y, float* scale_out, int M, int N, int K,
                         int act, int out_f32, bool fp8, hipStream_t st) {
    TmpBufs tmp;
    const int Npad = round_up(N, 32), Kpad = round_up(K, 64);
    bf16_t* Wp;
    float* sc = nullptr;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * Kpad));
    if (fp8) {
        uint8_t* Wq;
        SVCHECK(tmp.get(&Wq, (size_t)Npad * Kpad));
        SVCHECK(tmp.get(&sc, (size_t)Npad));
        launch_pack_weight_fp8(W, 0, Wp, Wq, sc, N, K, Npad, Kpad, st);
    } else launch_pack_weight(W, 0, Wp, N, K, Npad, Kpad, st);
    const bf16_t* A = (const bf16_t*)x;
    int lda = K;
    if (Kpad != K) {
        bf16_t* xpd;
        SVCHECK(tmp.get(&xpd, (size_t)M * Kpad));
        HIPCHECK(hipMemsetAsync(xpd, 0, (size_t)M * Kpad * 2, st));
        HIPCHECK(hipMemcpy2DAsync(xpd, (size_t)Kpad * 2, x, (size_t)K * 2, (size_t)K * 2, M, hipMemcpyDeviceToDevice, st));
        A = xpd; lda = Kpad;
    }
    GemmArgs g;
    g.A = A; g.lda = lda; g.Wp = Wp; g.bias = (const bf16_t*)bias; g.R = (const bf16_t*)residual; g.ldr = N;
    g.C = y; g.ldc = N; g.M = M; g.N = N; g.K = Kpad; g.act = act; g.out_f32 = out_f32;
    g.cscale = sc;
    g.seq_rows = g_op_seq_rows.load();
    if (g.seq_rows < 0) { g.seq_rows = -g.seq_rows; g.splitk_rows = 1; }      // the rows are the last rows of sequences of |S| rows
    launch_gemm(g, st);
    if (scale_out) HIPCHECK(hipMemcpyAsync(scale_out, sc, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sv_op_linear(const void* x, const void* W, const void* bias, const void* residual, void* y, int32_t M,
                            int32_t N, int32_t K, int32_t act, int32_t out_f32, sv_stream stream) {
    if (!x || !W || !y || M < 1 || N < 4 || N % 4 || K < 1) return fail(SV_EINVAL, "sv_op_linear: bad argument");
    return op_linear_run(x, W, bias, residual, y, nullptr, M, N, K, act, out_f32, false, (hipStream_t)stream);
}

// sv_op_linear with fp8 (e4m3) weights: the six cscale sites of the big-M kernels (gemm_bf16_kernel / gemm256_kernel: LDS strip and register
// epilogue; gemm_tail_kernel; gemm_tailk_kernel) on their own.  scale_out [N] (optional) returns the row scales.
extern "C" int sv_op_linear_fp8(const void* x, const void* W, const void* bias, const void* residual, void* y, float* scale_out, int32_t M,
                                int32_t N, int32_t K, int32_t act, int32_t out_f32, sv_stream stream) {
    if (!x || !W || !y || M < 1 || N < 4 || N % 4 || K < 64 || K % 64)
        return fail(SV_EINVAL, "sv_op_linear_fp8: bad argument (N %% 4 == 0 and K %% 64 == 0 required)");
    return op_linear_run(x, W, bias, residual, y, scale_out, M, N, K, act, out_f32, true, (hipStream_t)stream);
}

// the fp8 quantiser on its own, exactly as sv_load_weight calls it: W [N][K] (bf16, or fp32 when w_is_f32) -> scale_out fp32 [Npad] (Npad = N rounded up
// to 32; 1 for an all-zero row and for the padding rows), wq_out [Npad * K] bytes (the decode image: [Npad/32][K/32][64 lanes][16 B], a lane's two
// consecutive k-steps of 8 e4m3 codes each) and wp_out bf16 [Npad * K] (the SAME values in the packed layout of the bf16 weights: [Npad/32][K/16][64][8]).
extern "C" int sv_op_pack_weight_fp8(const void* W, int32_t w_is_f32, int32_t N, int32_t K, float* scale_out, void* wq_out, void* wp_out,
                                     sv_stream stream) {
    if (!W || !scale_out || !wq_out || !wp_out || N < 1 || K < 64 || K % 64)
        return fail(SV_EINVAL, "sv_op_pack_weight_fp8: bad argument (K %% 64 == 0 required)");
    hipStream_t st = (hipStream_t)stream;
    launch_pack_weight_fp8(W, w_is_f32 != 0, (bf16_t*)wp_out, (uint8_t*)wq_out, scale_out, N, K, round_up(N, 32), K, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// Micro-benchmark of the big-M MFMA GEMM alone (zero-filled... no: uniform random bf16 operands, HIP events)
extern "C" int sv_bench_linear(int32_t M, int32_t N, int32_t K, int32_t act, int32_t residual, int32_t iters,
                               double* avg_us, sv_stream stream) {
    if (!avg_us || M < 1 || N < 32 || N % 4 || K < 64 || K % 64 || iters < 1) return fail(SV_EINVAL, "sv_bench_linear: bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Npad = round_up(N, 32);
    bf16_t *Wp, *A, *C, *bias, *Wsrc;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&Wsrc, (size_t)N * K));
    SVCHECK(tmp.get(&A, (size_t)M * K));
    SVCHECK(tmp.get(&C, (size_t)M * N));
    SVCHECK(tmp.get(&bias, (size_t)N));
    // pseudo-random operands in [-1, 1): zero-filled data would clock ~20 % higher (cdna guide, rule 25)
    fill_random_bf16(A, (size_t)M * K, 1u, 4096, st);
    fill_random_bf16(Wsrc, (size_t)N * K, 2u, 4096, st);
    fill_random_bf16(bias, (size_t)N, 3u, 64, st);
    fill_random_bf16(C, (size_t)M * N, 4u, 4096, st);
    launch_pack_weight(Wsrc, 0, Wp, N, K, Npad, K, st);
    if (const char* fill = getenv("SV_BENCH_FILL")) {
        // evidence for the ceiling claim (cdna guide rule 25): the SAME kernel on zero-filled operands clocks ~20 % higher (DVFS), so a
        // quoted TF/s must say which fill it ran on.  "zero": everything zero; default: uniform random in [-1, 1)
        if (!strcmp(fill, "zero")) {
            HIPCHECK(hipMemsetAsync(A, 0, (size_t)M * K * 2, st));
            HIPCHECK(hipMemsetAsync(Wp, 0, (size_t)Npad * K * 2, st));
            HIPCHECK(hipMemsetAsync(C, 0, (size_t)M * N * 2, st));
            HIPCHECK(hipMemsetAsync(bias, 0, (size_t)N * 2, st));
        }
    }
    GemmArgs g;
    g.A = A; g.lda = K; g.Wp = Wp; g.bias = bias; g.R = residual ? C : nullptr; g.ldr = N; g.C = C; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.act = act; g.out_f32 = 0;
    g.seq_rows = g_op_seq_rows.load() > 0 ? g_op_seq_rows.load() : 0;
    // SV_BENCH_GEMM_FORM = 0 / 1: one fixed form (128^2 tiles, 256^2 tiles; rows not peeled) instead of the tuned choice
    const char* form_s = getenv("SV_BENCH_GEMM_FORM");
    const int form = form_s ? atoi(form_s) : -1;
    auto run1 = [&]() { if (form >= 0) launch_gemm_fixed(g, form, 0, st); else launch_gemm(g, st); };
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) run1();
    HIPCHECK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) run1();
    HIPCHECK(hipEventRecord(e1, st));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = (double)ms * 1e3 / iters;
    HIPCHECK(hipGetLastError());
    return 0;
}

// The 256^2 big-M kernel on its own over random operands, one launch with wall-clock stamps (100 MHz): host_out [blocks * 2][8] =
// {start, K-tile 0 staged, K loop done, epilogue stored and drained, tile m, tile n, wave (0 / 7: one wave of each ping-pong group), 0}.
// form: 1 (round 4's persistent stream-K kernel was form 2: profiles/gemm_trace_r04.log).  Returns the number of blocks (tools/gemm_trace.py:
// where the time of a prefill GEMM goes).
extern "C" int sv_debug_gemm_trace(int32_t M, int32_t N, int32_t K, int32_t act, int32_t form, int64_t* host_out, int32_t capacity_blocks) {
    if (!host_out || M < 256 || N < 256 || N % 8 || K < 64 || K % 64 || form != 1) return fail(SV_EINVAL, "sv_debug_gemm_trace: bad argument (form: 1)");
    const int blocks = ((M + 255) / 256) * ((N + 255) / 256);
    if (capacity_blocks < blocks) return fail(SV_EINVAL, "sv_debug_gemm_trace: capacity %d < %d blocks", capacity_blocks, blocks);
    hipStream_t st = nullptr;
    TmpBufs tmp;
    const int Npad = round_up(N, 32);
    bf16_t *Wp, *A, *C, *bias, *Wsrc;
    long long* tr;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&Wsrc, (size_t)N * K));
    SVCHECK(tmp.get(&A, (size_t)M * K));
    SVCHECK(tmp.get(&C, (size_t)M * N));
    SVCHECK(tmp.get(&bias, (size_t)N));
    SVCHECK(tmp.get(&tr, (size_t)blocks * 16));
    fill_random_bf16(A, (size_t)M * K, 1u, 4096, st);
    fill_random_bf16(Wsrc, (size_t)N * K, 2u, 4096, st);
    fill_random_bf16(bias, (size_t)N, 3u, 64, st);
    launch_pack_weight(Wsrc, 0, Wp, N, K, Npad, K, st);
    HIPCHECK(hipMemsetAsync(tr, 0, (size_t)blocks * 16 * sizeof(long long), st));
    GemmArgs g;
    g.A = A; g.lda = K; g.Wp = Wp; g.bias = bias; g.R = nullptr; g.ldr = N; g.C = C; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.act = act; g.out_f32 = 0;
    for (int i = 0; i < 20; ++i) launch_gemm_fixed(g, form, 0, st);          // clocks and caches as in a running prefill
    g.trace = tr;
    launch_gemm_fixed(g, form, 0, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipMemcpy(host_out, tr, (size_t)blocks * 16 * sizeof(long long), hipMemcpyDeviceToHost));
    return blocks;
}

extern "C" int sv_op_linear_skinny(const void* x, const void* W, const void* bias, void* y_f32, int32_t M, int32_t N,
                                   int32_t K, int32_t splitk, sv_stream stream) {
    if (!x || !W || !y_f32 || M < 1 || N < 1 || K < 16 || K % 16 || splitk < 1 || (K / 16) % splitk)
        return fail(SV_EINVAL, "sv_op_linear_skinny: bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Npad = round_up(N, 32), MT = (M + 31) / 32;
    bf16_t *Wp, *xp;
    float* ws;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&xp, (size_t)MT * 32 * K));
    SVCHECK(tmp.get(&ws, (size_t)splitk * MT * 32 * Npad));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)MT * 32 * K * 2, st));
    launch_pack_weight(W, 0, Wp, N, K, Npad, K, st);
    pack_rows((const bf16_t*)x, K, xp, M, K, st);
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.MT = MT; a.Npad = Npad; a.K = K; a.splitk = splitk; a.out_mode = SK_OUT_PARTIAL;
    a.ws = ws; a.ldws = Npad; a.N = N;
    launch_gemm_skinny(a, st);
    reduce_partials(ws, splitk, MT * 32, Npad, (const bf16_t*)bias,
                                                                 (float*)y_f32, M, N, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// the fp8-weight decode GEMM on its own: W [N][K] bf16 is quantised like sv_load_weight does it with weight_dtype = fp8
// (one e4m3 scale per row), y = x . dequant(quant(W))^T + bias in fp32; scale_out [N] (optional) returns the row scales
extern "C" int sv_op_linear_skinny_fp8(const void* x, const void* W, const void* bias, void* y_f32, float* scale_out,
                                       int32_t M, int32_t N, int32_t K, int32_t splitk, sv_stream stream) {
    if (!x || !W || !y_f32 || M < 1 || N < 1 || K < 64 || K % 64 || splitk < 1 || (K / 16) % splitk || ((K / 16) / splitk) % 4)
        return fail(SV_EINVAL, "sv_op_linear_skinny_fp8: bad argument (K %% 64 == 0 and (K/16/splitk) %% 4 == 0 required)");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Npad = round_up(N, 32), MT = (M + 31) / 32;
    bf16_t *Wp, *xp;
    uint8_t* Wq;
    float *ws, *sc;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&Wq, (size_t)Npad * K));
    SVCHECK(tmp.get(&sc, (size_t)Npad));
    SVCHECK(tmp.get(&xp, (size_t)MT * 32 * K));
    SVCHECK(tmp.get(&ws, (size_t)splitk * MT * 32 * Npad));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)MT * 32 * K * 2, st));
    launch_pack_weight_fp8(W, 0, Wp, Wq, sc, N, K, Npad, K, st);
    pack_rows((const bf16_t*)x, K, xp, M, K, st);
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.Wq = Wq; a.wscale = sc; a.MT = MT; a.Npad = Npad; a.K = K; a.splitk = splitk;
    a.out_mode = SK_OUT_PARTIAL; a.ws = ws; a.ldws = Npad; a.N = N;
    launch_gemm_skinny(a, st);
    reduce_partials(ws, splitk, MT * 32, Npad, (const bf16_t*)bias,
                                                                 (float*)y_f32, M, N, st);
    if (scale_out) HIPCHECK(hipMemcpyAsync(scale_out, sc, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// the decode GEMM's two fused epilogues on their own (split-K 1): out_f32 == 0: y[M,N] = act(bf16(x W^T + bias)) as bf16 rows
// (c_fc: N %% 8 == 0); out_f32 != 0: fp32 rows of x W^T rounded to bf16 values, no bias (lm_head)
static int op_linear_skinny_epi_run(const void* x, const void* W, const void* bias, void* y, float* scale_out, int M, int N, int K, int act,
                                    int out_f32, bool fp8, hipStream_t st) {
    TmpBufs tmp;
    const int Npad = round_up(N, 32), MT = (M + 31) / 32, R = MT * 32;
    bf16_t *Wp, *xp, *oxp;
    uint8_t* Wq = nullptr;
    float *of, *sc = nullptr;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&xp, (size_t)R * K));
    SVCHECK(tmp.get(&oxp, (size_t)R * Npad));
    SVCHECK(tmp.get(&of, (size_t)R * Npad));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)R * K * 2, st));
    if (fp8) {
        SVCHECK(tmp.get(&Wq, (size_t)Npad * K));
        SVCHECK(tmp.get(&sc, (size_t)Npad));
        launch_pack_weight_fp8(W, 0, Wp, Wq, sc, N, K, Npad, K, st);
    } else launch_pack_weight(W, 0, Wp, N, K, Npad, K, st);
    pack_rows((const bf16_t*)x, K, xp, M, K, st);
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.Wq = Wq; a.wscale = sc; a.MT = MT; a.Npad = Npad; a.K = K; a.splitk = 1; a.N = N;
    if (out_f32) { a.out_mode = SK_OUT_F32; a.out_f32 = of; a.ldo = Npad; a.round_bf16 = 1; }
    else {
        a.out_mode = SK_OUT_PACKED_ACT; a.bias = (const bf16_t*)bias; a.act = act; a.out_xp = oxp; a.out_KS = Npad / 16;
        // the engine's scratch for the tiles beyond the first round of blocks (gemm_skinny_tailsplit_kernel; taken only where launch_gemm_skinny's rule says so)
        float* tws; unsigned* tcnt;
        SVCHECK(tmp.get(&tws, (size_t)SV_TAIL_TILES * 8 * 16 * 64));
        SVCHECK(tmp.get(&tcnt, (size_t)SV_TAIL_TILES));
        HIPCHECK(hipMemsetAsync(tcnt, 0, (size_t)SV_TAIL_TILES * sizeof(unsigned), st));
        a.tail_ws = tws; a.tail_cnt = tcnt;
    }
    launch_gemm_skinny(a, st);
    if (out_f32) HIPCHECK(hipMemcpy2DAsync(y, (size_t)N * 4, of, (size_t)Npad * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, st));
    else if (N == Npad) unpack_rows(oxp, (bf16_t*)y, N, M, N, st);
    else {
        // the kernel wrote row tiles of out_KS = Npad / 16 k-steps: unpack that width (unpacking N columns would look for the second row tile
        // at 32 * N elements instead of 32 * Npad), then keep the N valid columns
        bf16_t* yp;
        SVCHECK(tmp.get(&yp, (size_t)M * Npad));
        unpack_rows(oxp, yp, Npad, M, Npad, st);
        HIPCHECK(hipMemcpy2DAsync(y, (size_t)N * 2, yp, (size_t)Npad * 2, (size_t)N * 2, M, hipMemcpyDeviceToDevice, st));
    }
    if (scale_out) HIPCHECK(hipMemcpyAsync(scale_out, sc, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sv_op_linear_skinny_epi(const void* x, const void* W, const void* bias, void* y, int32_t M, int32_t N, int32_t K,
                                       int32_t act, int32_t out_f32, sv_stream stream) {
    if (!x || !W || !y || M < 1 || N < 1 || K < 16 || K % 16) return fail(SV_EINVAL, "sv_op_linear_skinny_epi: bad argument");
    if (!out_f32 && N % 8) return fail(SV_EINVAL, "bf16 output needs N %% 8 == 0");
    return op_linear_skinny_epi_run(x, W, bias, y, nullptr, M, N, K, act, out_f32, false, (hipStream_t)stream);
}

// the same two epilogues with fp8 (e4m3) weights, the SkinnyArgs of an fp8 engine's c_fc and lm_head (engine_forward.hip): the weight quantised as
// sv_load_weight does it, Wq / wscale set; scale_out [N] (optional) returns the row scales
extern "C" int sv_op_linear_skinny_epi_fp8(const void* x, const void* W, const void* bias, void* y, float* scale_out, int32_t M, int32_t N,
                                           int32_t K, int32_t act, int32_t out_f32, sv_stream stream) {
    if (!x || !W || !y || M < 1 || N < 1 || K < 64 || K % 64)
        return fail(SV_EINVAL, "sv_op_linear_skinny_epi_fp8: bad argument (K %% 64 == 0 required)");
    if (!out_f32 && N % 8) return fail(SV_EINVAL, "sv_op_linear_skinny_epi_fp8: bf16 output needs N %% 8 == 0");
    return op_linear_skinny_epi_run(x, W, bias, y, scale_out, M, N, K, act, out_f32, true, (hipStream_t)stream);
}

// ---- MXFP4 weights (csrc/mxfp4/mxfp4.hip; the format: kernels.h launch_pack_weight_mxfp4) ----
// the quantiser on its own, exactly as sv_load_weight calls it: W [N][K] (bf16, or fp32 when w_is_f32) -> scale_out uint8 [Npad][K/32] (the e8m0
// bytes, Npad = N rounded up to 32), w4_out = the raw decode image (Npad/32 * K/64 * 1088 bytes), wp_out bf16 [Npad * K] = the raw bf16 image
extern "C" int sv_op_pack_weight_mxfp4(const void* W, int32_t w_is_f32, int32_t N, int32_t K, void* scale_out, void* w4_out, void* wp_out,
                                       sv_stream stream) {
    if (!W || !scale_out || !w4_out || !wp_out || N < 1 || K < 64 || K % 64)
        return fail(SV_EINVAL, "sv_op_pack_weight_mxfp4: bad argument (K %% 64 == 0 required)");
    hipStream_t st = (hipStream_t)stream;
    launch_pack_weight_mxfp4(W, w_is_f32 != 0, (bf16_t*)wp_out, (uint8_t*)w4_out, (uint8_t*)scale_out, N, K, round_up(N, 32), K, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// the MXFP4 decode GEMM through launch_gemm_skinny, the SkinnyArgs an mxfp4 engine builds: out_mode SK_OUT_PARTIAL (slabs, reduced here with the
// bias), SK_OUT_PACKED_ACT or SK_OUT_F32 (split-K 1).  col_tiles 0 = the launcher's default.
static int op_linear_skinny_mxfp4_run(const void* x, const void* W, const void* bias, void* y, void* scale_out, int M, int N, int K, int splitk,
                                      int col_tiles, int out_mode, int act, hipStream_t st) {
    TmpBufs tmp;
    const int Npad = round_up(N, 32), MT = (M + 31) / 32, R = MT * 32;
    bf16_t *Wp, *xp, *oxp = nullptr;
    uint8_t *W4, *sc;
    float* of;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&W4, mxfp4_image_bytes(Npad, K)));
    SVCHECK(tmp.get(&sc, (size_t)Npad * (K / 32)));
    SVCHECK(tmp.get(&xp, (size_t)R * K));
    SVCHECK(tmp.get(&of, (size_t)(out_mode == SK_OUT_PARTIAL ? splitk : 1) * R * Npad));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)R * K * 2, st));
    launch_pack_weight_mxfp4(W, 0, Wp, W4, sc, N, K, Npad, K, st);
    pack_rows((const bf16_t*)x, K, xp, M, K, st);
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.W4 = W4; a.MT = MT; a.Npad = Npad; a.K = K; a.splitk = splitk; a.N = N; a.col_tiles = col_tiles; a.out_mode = out_mode;
    if (out_mode == SK_OUT_PARTIAL) { a.ws = of; a.ldws = Npad; }
    else if (out_mode == SK_OUT_F32) { a.out_f32 = of; a.ldo = Npad; a.round_bf16 = 1; }
    else {
        SVCHECK(tmp.get(&oxp, (size_t)R * Npad));
        a.bias = (const bf16_t*)bias; a.act = act; a.out_xp = oxp; a.out_KS = Npad / 16;
    }
    if (!launch_gemm_skinny_mxfp4(a, st)) return fail(SV_ENOTSUP, "mxfp4 decode GEMM: K=%d with split-K %d has no kernel", K, splitk);
    if (out_mode == SK_OUT_PARTIAL) reduce_partials(of, splitk, R, Npad, (const bf16_t*)bias, (float*)y, M, N, st);
    else if (out_mode == SK_OUT_F32) HIPCHECK(hipMemcpy2DAsync(y, (size_t)N * 4, of, (size_t)Npad * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, st));
    else if (N == Npad) unpack_rows(oxp, (bf16_t*)y, N, M, N, st);
    else {
        bf16_t* yp;                                   // (row tiles of Npad / 16 k-steps: see op_linear_skinny_epi_run)
        SVCHECK(tmp.get(&yp, (size_t)M * Npad));
        unpack_rows(oxp, yp, Npad, M, Npad, st);
        HIPCHECK(hipMemcpy2DAsync(y, (size_t)N * 2, yp, (size_t)Npad * 2, (size_t)N * 2, M, hipMemcpyDeviceToDevice, st));
    }
    if (scale_out) HIPCHECK(hipMemcpyAsync(scale_out, sc, (size_t)N * (K / 32), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// y fp32 [M][N] = x . dequant(quant(W))^T + bias through fp32 slabs; scale_out uint8 [N][K/32] (optional) returns the scale bytes
extern "C" int sv_op_linear_skinny_mxfp4(const void* x, const void* W, const void* bias, void* y_f32, void* scale_out, int32_t M, int32_t N,
                                         int32_t K, int32_t splitk, int32_t col_tiles, sv_stream stream) {
    if (!x || !W || !y_f32 || M < 1 || N < 1 || K < 64 || K % 64 || splitk < 1 || splitk > 8 || !skinny_waves_mxfp4(K / 16, splitk) ||
        !(col_tiles == 0 || col_tiles == 1 || col_tiles == 2 || col_tiles == 4))
        return fail(SV_EINVAL, "sv_op_linear_skinny_mxfp4: bad argument (K %% 64 == 0, (K/16/splitk) %% 8 == 0, col_tiles 0, 1, 2 or 4 required)");
    return op_linear_skinny_mxfp4_run(x, W, bias, y_f32, scale_out, M, N, K, splitk, col_tiles, SK_OUT_PARTIAL, 0, (hipStream_t)stream);
}

// the two fused epilogues (split-K 1) as sv_op_linear_skinny_epi states them, the SkinnyArgs of an mxfp4 engine's c_fc and lm_head
extern "C" int sv_op_linear_skinny_epi_mxfp4(const void* x, const void* W, const void* bias, void* y, void* scale_out, int32_t M, int32_t N,
                                             int32_t K, int32_t act, int32_t out_f32, int32_t col_tiles, sv_stream stream) {
    if (!x || !W || !y || M < 1 || N < 1 || K < 64 || K % 64 || !skinny_waves_mxfp4(K / 16, 1) ||
        !(col_tiles == 0 || col_tiles == 1 || col_tiles == 2 || col_tiles == 4))
        return fail(SV_EINVAL, "sv_op_linear_skinny_epi_mxfp4: bad argument (K %% 128 == 0, col_tiles 0, 1, 2 or 4 required)");
    if (!out_f32 && N % 8) return fail(SV_EINVAL, "sv_op_linear_skinny_epi_mxfp4: bf16 output needs N %% 8 == 0");
    return op_linear_skinny_mxfp4_run(x, W, bias, y, scale_out, M, N, K, 1, col_tiles, out_f32 ? SK_OUT_F32 : SK_OUT_PACKED_ACT, act, (hipStream_t)stream);
}

// the lm_head form of the decode GEMM with the greedy selection folded into its epilogue (gemm.hip, SkinnyArgs::amax): y_f32 [M][N]
// (optional) = the bf16-rounded fp32 logits x W^T, host_idx [M] = the arg-max column of every row as finish_step_kernel decodes it
// (lowest index on ties, NaN never wins; 0x7fffffff for a row without a single comparable score).  M <= 32.
extern "C" int sv_op_lm_head_argmax(const void* x, const void* W, void* y_f32, int32_t* host_idx, int32_t M, int32_t N, int32_t K,
                                    sv_stream stream) {
    if (!x || !W || !host_idx || M < 1 || M > 32 || N < 1 || K < 32 || K % 32) return fail(SV_EINVAL, "sv_op_lm_head_argmax: bad argument (M <= 32, K %% 32 == 0)");
    if (int ar = init_gemm_kernels()) return fail(SV_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString((hipError_t)ar));
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Npad = round_up(N, 32);
    int waves = 1, two = 0;
    skinny_plan(Npad, K, 1, 0, 1, &waves, &two);
    if (waves < 2) return fail(SV_ENOTSUP, "sv_op_lm_head_argmax: K = %d leaves one wave per block (the fold needs the K split over waves)", K);
    bf16_t *Wp, *xp;
    float* of;
    unsigned long long* keys;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&xp, (size_t)32 * K));
    SVCHECK(tmp.get(&of, (size_t)32 * Npad));
    SVCHECK(tmp.get(&keys, (size_t)32 * SV_AMAX_STRIDE));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)32 * K * 2, st));
    HIPCHECK(hipMemsetAsync(keys, 0, (size_t)32 * SV_AMAX_STRIDE * 8, st));
    launch_pack_weight(W, 0, Wp, N, K, Npad, K, st);
    pack_rows((const bf16_t*)x, K, xp, M, K, st);
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.MT = 1; a.Npad = Npad; a.K = K; a.splitk = 1; a.N = N;
    a.out_mode = SK_OUT_F32; a.out_f32 = of; a.ldo = Npad; a.round_bf16 = 1; a.amax = keys; a.amax_rows = M;
    launch_gemm_skinny(a, st);
    if (y_f32) HIPCHECK(hipMemcpy2DAsync(y_f32, (size_t)N * 4, of, (size_t)Npad * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, st));
    std::vector<unsigned long long> h((size_t)32 * SV_AMAX_STRIDE);
    HIPCHECK(hipMemcpyAsync(h.data(), keys, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    for (int m = 0; m < M; ++m) host_idx[m] = sv_amax_index(h[(size_t)m * SV_AMAX_STRIDE]);
    return 0;
}

// The 6-launch layer's two kernels as one op (decode_cols.hip): h2 = bf16(h + bf16(x Wp^T + bp)) by the slab-free output projection
// (whole K per block, partial row statistics), then y = act(bf16(LN(h2; gamma, beta) Wf^T + bf)) by the decode GEMM on the RAW h2
// with the LayerNorm folded into its weights / epilogue.  Row-major in / out; M <= 32.
extern "C" int sv_op_decode_proj_fold(const void* x, const void* Wp_, const void* bp, const void* h, const void* gamma, const void* beta,
                                      float eps, const void* Wf_, const void* bf_, void* h2_out, void* y_out, int32_t M, int32_t D,
                                      int32_t Kp, int32_t F, int32_t act, sv_stream stream) {
    if (!x || !Wp_ || !h || !gamma || !beta || !Wf_ || !h2_out || !y_out || M < 1 || M > 32 || D < 32 || D % 32 || Kp < 32 || Kp % 32 ||
        F < 8 || F % 8)
        return fail(SV_EINVAL, "sv_op_decode_proj_fold: bad argument (M <= 32, D %% 32 == 0, Kp %% 32 == 0, F %% 8 == 0)");
    if (int ar = init_cols_kernels()) return fail(SV_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString((hipError_t)ar));
    if (int ar = init_gemm_kernels()) return fail(SV_EHIP, "hipFuncSetAttribute: %s", hipGetErrorString((hipError_t)ar));
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Fpad = round_up(F, 32), cpb = cols_pick_cpb(D, Kp);
    bf16_t *Wpp, *Wfp, *Wff, *xp, *hxp, *yxp;
    float *c1, *c2;
    SVCHECK(tmp.get(&Wpp, (size_t)D * Kp));
    SVCHECK(tmp.get(&Wfp, (size_t)Fpad * D));
    SVCHECK(tmp.get(&Wff, (size_t)Fpad * D));
    SVCHECK(tmp.get(&xp, (size_t)32 * Kp));
    SVCHECK(tmp.get(&hxp, (size_t)32 * D));
    SVCHECK(tmp.get(&yxp, (size_t)32 * Fpad));
    SVCHECK(tmp.get(&c1, (size_t)Fpad));
    SVCHECK(tmp.get(&c2, (size_t)Fpad));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)32 * Kp * 2, st));
    HIPCHECK(hipMemsetAsync(hxp, 0, (size_t)32 * D * 2, st));
    launch_pack_weight(Wp_, 0, Wpp, D, Kp, D, Kp, st);
    launch_pack_weight(Wf_, 0, Wfp, F, D, Fpad, D, st);
    pack_rows((const bf16_t*)x, Kp, xp, M, Kp, st);
    pack_rows((const bf16_t*)h, D, hxp, M, D, st);
    launch_fold_prepare(Wfp, (const bf16_t*)gamma, (const bf16_t*)beta, (const bf16_t*)bf_, Wff, c1, c2, F, Fpad, D, st);
    ColsArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.xp = xp; ca.Wp = Wpp; ca.bias = (const bf16_t*)bp; ca.MT = 1; ca.M = M; ca.N = D; ca.K = Kp; ca.cpb = cpb; ca.h_xp = hxp; ca.out_KS = D / 16;
    if (launch_gemm_cols(ca, st)) return fail(SV_ENOTSUP, "sv_op_decode_proj_fold: no kernel for this shape");
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = hxp; a.Wp = Wff; a.MT = 1; a.Npad = Fpad; a.K = D; a.N = F; a.splitk = 1; a.out_mode = SK_OUT_PACKED_ACT; a.act = act;
    a.out_xp = yxp; a.out_KS = Fpad / 16; a.fold_c1 = c1; a.fold_c2 = c2; a.fold_D = D;
    a.fold_eps = eps;
    launch_gemm_skinny(a, st);
    unpack_rows(hxp, (bf16_t*)h2_out, D, M, D, st);
    unpack_rows(yxp, (bf16_t*)y_out, F, M, F, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// Micro-benchmark of the decode GEMM kernel alone (HIP events, `iters` back-to-back launches on one stream):
// mode 0 = fp32 slabs (split-K `splitk`), 1 = bias + GELU -> fragment order, 2 = fp32 rows rounded to bf16 values (lm_head).
// Weights / activations are zero-filled device buffers (bandwidth only).  NOTE: back-to-back launches of ONE GEMM re-read
// the same weights, so anything below ~200 MB is served by the Infinity Cache / L2 -- an upper bound, not the in-situ time.
extern "C" int sv_bench_decode_linear(int32_t M, int32_t N, int32_t K, int32_t splitk, int32_t mode, int32_t iters, double* avg_us,
                                      sv_stream stream) {
    if (!avg_us || M < 1 || N < 32 || K < 32 || K % 32 || splitk < 1 || (K / 16) % splitk || iters < 1 || mode < 0 || mode > 2)
        return fail(SV_EINVAL, "sv_bench_decode_linear: bad argument");
    if (mode != 0 && splitk != 1) return fail(SV_EINVAL, "sv_bench_decode_linear: modes 1 and 2 need splitk == 1");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    const int Npad = round_up(N, 32), MT = (M + 31) / 32, R = MT * 32;
    bf16_t *Wp, *xp, *oxp, *bias;
    float* ws;
    SVCHECK(tmp.get(&Wp, (size_t)Npad * K));
    SVCHECK(tmp.get(&xp, (size_t)R * K));
    SVCHECK(tmp.get(&oxp, (size_t)R * Npad));
    SVCHECK(tmp.get(&bias, (size_t)Npad));
    SVCHECK(tmp.get(&ws, (size_t)splitk * R * Npad));
    HIPCHECK(hipMemsetAsync(Wp, 0, (size_t)Npad * K * 2, st));
    HIPCHECK(hipMemsetAsync(xp, 0, (size_t)R * K * 2, st));
    HIPCHECK(hipMemsetAsync(bias, 0, (size_t)Npad * 2, st));
    SkinnyArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = xp; a.Wp = Wp; a.bias = bias; a.MT = MT; a.Npad = Npad; a.K = K; a.splitk = splitk; a.N = N;
    a.out_mode = mode; a.act = mode == 1 ? ACT_GELU_TANH : ACT_NONE;
    a.ws = ws; a.ldws = Npad; a.out_xp = oxp; a.out_KS = Npad / 16; a.out_f32 = ws; a.ldo = Npad; a.round_bf16 = 1;
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch_gemm_skinny(a, st);
    HIPCHECK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) launch_gemm_skinny(a, st);
    HIPCHECK(hipEventRecord(e1, st));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_us = (double)ms * 1e3 / iters;
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_cvt_bf16_hw(const float* x, void* y, int64_t n, sv_stream stream) {
    if (!x || !y || n < 1) return fail(SV_EINVAL, "sv_op_cvt_bf16_hw: bad argument");
    launch_cvt_bf16_hw(x, (bf16_t*)y, (size_t)n, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_attention(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t S, int32_t H,
                               int32_t Hkv, int32_t head_dim, int32_t causal, float scale, sv_stream stream) {
    if (!q || !k || !v || !out || B < 1 || S < 1 || H < 1 || Hkv < 1 || H % Hkv) return fail(SV_EINVAL, "sv_op_attention: bad argument");
    if (head_dim != 64 && head_dim != 128) return fail(SV_EINVAL, "head_dim %d unsupported (64|128)", head_dim);
    AttnPrefillArgs a;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v;
    a.q_row_stride = H * head_dim; a.kv_row_stride = Hkv * head_dim; a.q_head_stride = head_dim;
    a.kv_head_stride = head_dim; a.o = (bf16_t*)out; a.o_row_stride = H * head_dim; a.B = B; a.S = S; a.H = H;
    a.head_dim = head_dim; a.kv_group = H / Hkv; a.causal = causal; a.scale = scale;
    launch_attn_prefill(a, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

// attn_prefill_kernel in the forms the engine launches it: q / k / v as column ranges of ONE token-major buffer (the c_attn output), MQA with
// kv_head_stride 0, the sliding window, the trailing query tiles alone (last_rows) and the ragged form (host_lens).  The arguments are filled
// as prefill_forward / prefill_forward_ragged fill them; everything is checked on the host first, so that what passes keeps every access of
// the kernel inside rows * row_stride elements of `qkv` and rows * H * head_dim elements of `out` (the kernel clamps rows to the last row of
// their sequence, a 16-byte load starts at a multiple of 8 elements inside its head, and an output row is written only when it exists).
extern "C" int sv_op_attention_prefill(const void* qkv, int32_t q_off, int32_t k_off, int32_t v_off, int32_t row_stride, void* out, int32_t B,
                                       int32_t S, const int32_t* host_lens, int32_t H, int32_t Hkv, int32_t head_dim, int32_t causal,
                                       float scale, int32_t window, int32_t last_rows, sv_stream stream) {
    const char* who = "sv_op_attention_prefill";
    if (!qkv || !out) return fail(SV_EINVAL, "%s: null pointer", who);
    if (B < 1 || H < 1 || Hkv < 1 || H > 4096) return fail(SV_EINVAL, "%s: bad shape (B %d, H %d, Hkv %d)", who, B, H, Hkv);
    if (H % Hkv) return fail(SV_EINVAL, "%s: %d query heads are not a multiple of %d KV heads", who, H, Hkv);
    if (head_dim != 64 && head_dim != 128) return fail(SV_EINVAL, "%s: head_dim %d unsupported (64|128)", who, head_dim);
    if (q_off < 0 || k_off < 0 || v_off < 0 || row_stride < 8 || (q_off | k_off | v_off | row_stride) % 8)
        return fail(SV_EINVAL, "%s: offsets %d / %d / %d and row stride %d must be non-negative multiples of 8 elements (16-byte loads)", who,
                    q_off, k_off, v_off, row_stride);
    if ((long long)q_off + (long long)H * head_dim > row_stride || (long long)k_off + (long long)Hkv * head_dim > row_stride ||
        (long long)v_off + (long long)Hkv * head_dim > row_stride)
        return fail(SV_EINVAL, "%s: q / k / v columns (%d + %d x %d, %d + %d x %d, %d + %d x %d) reach beyond the row stride %d", who, q_off,
                    H, head_dim, k_off, Hkv, head_dim, v_off, Hkv, head_dim, row_stride);
    if (!(scale > 0.f) || std::isinf(scale)) return fail(SV_EINVAL, "%s: scale must be positive and finite", who);
    if (window < 0) return fail(SV_EINVAL, "%s: window %d < 0", who, window);
    if (window > 0 && !causal) return fail(SV_EINVAL, "%s: a window needs causal = 1", who);
    if (host_lens && !causal) return fail(SV_EINVAL, "%s: the ragged form (lengths) needs causal = 1", who);
    if (last_rows < 0) return fail(SV_EINVAL, "%s: last_rows %d < 0", who, last_rows);
    long long rows = 0;
    if (host_lens) {
        for (int b = 0; b < B; ++b) {
            if (host_lens[b] < 1) return fail(SV_EINVAL, "%s: length %d of sequence %d (must be >= 1)", who, host_lens[b], b);
            rows += host_lens[b];
        }
    } else {
        if (S < 1) return fail(SV_EINVAL, "%s: S %d < 1", who, S);
        rows = (long long)B * S;
    }
    if (rows > (1 << 24) || B > 65535) return fail(SV_EINVAL, "%s: %lld rows / %d sequences: more than this test surface takes", who, rows, B);

    hipStream_t st = (hipStream_t)stream;
    AttnPrefillArgs a;
    a.q = (const bf16_t*)qkv + q_off; a.k = (const bf16_t*)qkv + k_off; a.v = (const bf16_t*)qkv + v_off;
    a.q_row_stride = row_stride; a.kv_row_stride = row_stride; a.q_head_stride = head_dim; a.kv_head_stride = Hkv > 1 ? head_dim : 0;
    a.o = (bf16_t*)out; a.o_row_stride = H * head_dim; a.B = B; a.S = host_lens ? 0 : S; a.H = H; a.head_dim = head_dim;
    a.kv_group = H / Hkv; a.causal = causal ? 1 : 0; a.scale = scale; a.window = window;
    TmpBufs tmp;
    if (host_lens) {
        // descriptors {first packed row, length} | the engine's own block list (every query tile, or each sequence's last one)
        std::vector<int32_t> plan((size_t)2 * B), blocks;
        int r0 = 0;
        for (int b = 0; b < B; ++b) { plan[2 * b] = r0; plan[2 * b + 1] = host_lens[b]; r0 += host_lens[b]; }
        ragged_blocks(host_lens, B, attn_prefill_q_tile(H, Hkv), last_rows > 0, blocks);
        plan.insert(plan.end(), blocks.begin(), blocks.end());
        int32_t* d_plan;
        SVCHECK(tmp.get(&d_plan, plan.size()));
        HIPCHECK(hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        a.rag_seq = d_plan; a.rag_blocks = d_plan + (size_t)2 * B; a.rag_nblocks = (int)blocks.size() / 2;
    } else {
        a.last_rows = last_rows;
    }
    launch_attn_prefill(a, st);
    HIPCHECK(hipGetLastError());
    if (host_lens) HIPCHECK(hipStreamSynchronize(st));          // the plan is freed on return
    return 0;
}

// attn_prefill_kernel's prefixed form alone, with the descriptors and the block list of the shared-prefix scoring pass (prefix_plan).  As above every
// access stays inside packed rows * row_stride elements of `qkv` and packed rows * H * head_dim elements of `out`: a solo index below T maps to a row
// of the sequence's prefix or to one of its own rows, and only own rows are stored.
extern "C" int sv_op_attn_prefill_prefixed(const void* qkv, int32_t q_off, int32_t k_off, int32_t v_off, int32_t row_stride, void* out, int32_t P,
                                           const int32_t* host_prefix_lens, int32_t B, const int32_t* host_lens, const int32_t* host_prefix_of,
                                           int32_t H, int32_t Hkv, int32_t head_dim, float scale, int32_t window, sv_stream stream) {
    const char* who = "sv_op_attn_prefill_prefixed";
    if (!qkv || !out || !host_prefix_lens || !host_lens || !host_prefix_of) return fail(SV_EINVAL, "%s: null pointer", who);
    if (H < 1 || Hkv < 1 || H > 4096) return fail(SV_EINVAL, "%s: bad shape (H %d, Hkv %d)", who, H, Hkv);
    if (H % Hkv) return fail(SV_EINVAL, "%s: %d query heads are not a multiple of %d KV heads", who, H, Hkv);
    if (head_dim != 64 && head_dim != 128) return fail(SV_EINVAL, "%s: head_dim %d unsupported (64|128)", who, head_dim);
    if (q_off < 0 || k_off < 0 || v_off < 0 || row_stride < 8 || (q_off | k_off | v_off | row_stride) % 8)
        return fail(SV_EINVAL, "%s: offsets %d / %d / %d and row stride %d must be non-negative multiples of 8 elements (16-byte loads)", who,
                    q_off, k_off, v_off, row_stride);
    if ((long long)q_off + (long long)H * head_dim > row_stride || (long long)k_off + (long long)Hkv * head_dim > row_stride ||
        (long long)v_off + (long long)Hkv * head_dim > row_stride)
        return fail(SV_EINVAL, "%s: q / k / v columns reach beyond the row stride %d", who, row_stride);
    if (!(scale > 0.f) || std::isinf(scale)) return fail(SV_EINVAL, "%s: scale must be positive and finite", who);
    if (window < 0) return fail(SV_EINVAL, "%s: window %d < 0", who, window);
    SVCHECK(prefix_check(who, host_prefix_lens, P, host_lens, host_prefix_of, B, nullptr));
    long long rows = 0;
    for (int u = 0; u < P; ++u) rows += host_prefix_lens[u];
    for (int b = 0; b < B; ++b) rows += host_lens[b];
    if (rows > (1 << 24) || B > 65535) return fail(SV_EINVAL, "%s: %lld rows / %d sequences: more than this test surface takes", who, rows, B);

    hipStream_t st = (hipStream_t)stream;
    PackedPlan pp;
    prefix_plan(host_prefix_lens, P, host_lens, host_prefix_of, B, attn_prefill_q_tile(H, Hkv), nullptr, 0, nullptr, pp);
    const std::vector<int32_t>&sseq = pp.list[PL_SEQ1], &sblocks = pp.list[PL_BLOCKS1];
    std::vector<int32_t> plan(sseq);
    plan.insert(plan.end(), sblocks.begin(), sblocks.end());
    TmpBufs tmp;
    int32_t* d_plan;
    SVCHECK(tmp.get(&d_plan, plan.size()));
    HIPCHECK(hipMemcpyAsync(d_plan, plan.data(), plan.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AttnPrefillArgs a;
    a.q = (const bf16_t*)qkv + q_off; a.k = (const bf16_t*)qkv + k_off; a.v = (const bf16_t*)qkv + v_off;
    a.q_row_stride = row_stride; a.kv_row_stride = row_stride; a.q_head_stride = head_dim; a.kv_head_stride = Hkv > 1 ? head_dim : 0;
    a.o = (bf16_t*)out; a.o_row_stride = H * head_dim; a.B = B; a.S = 0; a.H = H; a.head_dim = head_dim;
    a.kv_group = H / Hkv; a.causal = 1; a.scale = scale; a.window = window;
    a.rag_seq = d_plan; a.rag_blocks = d_plan + sseq.size(); a.rag_nblocks = (int)sblocks.size() / 2; a.rag_prefixed = 1;
    launch_attn_prefill(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));          // the plan is freed on return
    return 0;
}

extern "C" int sv_op_plane_layernorm(const void* x, const void* gamma, const void* beta, void* y, int32_t B, int32_t QD,
                                     float eps, sv_stream stream) {
    if (!x || !gamma || !beta || !y || B < 1 || QD < 8 || QD % 8) return fail(SV_EINVAL, "sv_op_plane_layernorm: bad argument");
    launch_plane_layernorm((const bf16_t*)x, (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, B, QD, eps,
                           (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_plane_layernorm_strided(const void* x, const void* gamma, const void* beta, void* y, int32_t B, int32_t QD, float eps,
                                             int64_t y_batch_stride, sv_stream stream) {
    if (!x || !gamma || !beta || !y || B < 1 || QD < 8 || QD % 8) return fail(SV_EINVAL, "sv_op_plane_layernorm_strided: bad argument");
    if (y_batch_stride < QD || y_batch_stride % 8)
        return fail(SV_EINVAL, "sv_op_plane_layernorm_strided: y_batch_stride %lld must be a multiple of 8 and >= QD %d", (long long)y_batch_stride, QD);
    launch_plane_layernorm((const bf16_t*)x, (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, B, QD, eps, (hipStream_t)stream,
                           (size_t)y_batch_stride);
    HIPCHECK(hipGetLastError());
    return 0;
}

// ---- the row kernels that assemble the prompt and carry the decode residual stream, each on its own (tests/test_gpu_row_kernels.py).
// The entry points check shapes only: the caller's buffers must hold what the comment in the header says each call addresses.
static bool rows_ok(int64_t rows) { return rows >= 1 && rows <= (1 << 24); }

extern "C" int sv_op_im2col(const void* img, void* out, int32_t B, int32_t img_size, int32_t patch, int32_t Kpad, sv_stream stream) {
    if (!img || !out || B < 1 || patch < 1 || img_size < patch || img_size > 4096) return fail(SV_EINVAL, "sv_op_im2col: bad argument");
    if (img_size % patch) return fail(SV_EINVAL, "sv_op_im2col: image_size %d %% patch %d != 0", img_size, patch);
    if (Kpad % 8 || Kpad < 3 * patch * patch) return fail(SV_EINVAL, "sv_op_im2col: Kpad %d must be a multiple of 8 and >= 3 * patch^2 = %d", Kpad, 3 * patch * patch);
    if (!rows_ok((int64_t)B * (img_size / patch) * (img_size / patch))) return fail(SV_EINVAL, "sv_op_im2col: too many patch rows");
    launch_im2col((const bf16_t*)img, (bf16_t*)out, B, img_size, patch, Kpad, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_vit_embed_lnpre(const void* patch_out, int32_t ldp, const void* cls, const void* pos, const void* gamma, const void* beta,
                                     void* x, int32_t B, int32_t NP, int32_t Dv, float eps, sv_stream stream) {
    if (!patch_out || !cls || !pos || !gamma || !beta || !x || B < 1 || NP < 1) return fail(SV_EINVAL, "sv_op_vit_embed_lnpre: bad argument");
    if (Dv < 8 || Dv % 8 || Dv > 2048) return fail(SV_EINVAL, "sv_op_vit_embed_lnpre: Dv %d must be a multiple of 8 in 8..2048 (4 chunks of 8 columns per lane)", Dv);
    if (ldp < Dv || ldp % 8) return fail(SV_EINVAL, "sv_op_vit_embed_lnpre: ldp %d must be a multiple of 8 and >= Dv %d", ldp, Dv);
    if (!rows_ok((int64_t)B * (NP + 1))) return fail(SV_EINVAL, "sv_op_vit_embed_lnpre: too many rows");
    launch_vit_embed_lnpre((const bf16_t*)patch_out, ldp, (const bf16_t*)cls, (const bf16_t*)pos, (const bf16_t*)gamma, (const bf16_t*)beta,
                           (bf16_t*)x, B, NP, Dv, eps, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_dec_embed(const void* emb, const void* table, void* h, int32_t B, int32_t S0, int32_t D, const int32_t* dev_row_pos,
                               sv_stream stream) {
    if (!emb || !table || !h || B < 1 || S0 < 1 || D < 8 || D % 8 || !rows_ok((int64_t)B * S0)) return fail(SV_EINVAL, "sv_op_dec_embed: bad argument (D %% 8 == 0)");
    launch_dec_embed((const bf16_t*)emb, (const bf16_t*)table, (bf16_t*)h, B, S0, D, (hipStream_t)stream, dev_row_pos);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_gather_rows(const void* table, const int64_t* dev_ids, void* out, int32_t n, int32_t D, int32_t per_seq, int64_t seq_stride,
                                 sv_stream stream) {
    if (!table || !dev_ids || !out || !rows_ok(n) || D < 8 || D % 8 || per_seq < 0) return fail(SV_EINVAL, "sv_op_gather_rows: bad argument (D %% 8 == 0)");
    if (per_seq > 0 && (n % per_seq || seq_stride < (int64_t)per_seq * D || seq_stride % 8))
        return fail(SV_EINVAL, "sv_op_gather_rows: n %d must be a multiple of per_seq %d, seq_stride %lld a multiple of 8 and >= per_seq * D", n, per_seq,
                    (long long)seq_stride);
    launch_gather_rows((const bf16_t*)table, dev_ids, (bf16_t*)out, n, D, (hipStream_t)stream, per_seq, (size_t)(per_seq > 0 ? seq_stride : 0));
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_gather_last_rows(const void* h, void* out, int32_t B, int32_t S0, int32_t D, const int32_t* dev_rag_seq, sv_stream stream) {
    if (!h || !out || B < 1 || D < 8 || D % 8 || (!dev_rag_seq && S0 < 1) || !rows_ok((int64_t)B * (S0 > 0 ? S0 : 1)))
        return fail(SV_EINVAL, "sv_op_gather_last_rows: bad argument (D %% 8 == 0, S0 >= 1 without descriptors)");
    launch_gather_last_rows((const bf16_t*)h, (bf16_t*)out, B, S0, D, (hipStream_t)stream, dev_rag_seq);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_gather_tail_rows(const void* h, void* out, int32_t B, int32_t S0, int32_t n_keep, int32_t D, sv_stream stream) {
    if (!h || !out || B < 1 || S0 < 1 || n_keep < 1 || n_keep > S0 || D < 8 || D % 8 || !rows_ok((int64_t)B * S0))
        return fail(SV_EINVAL, "sv_op_gather_tail_rows: bad argument (1 <= n_keep <= S0, D %% 8 == 0)");
    launch_gather_tail_rows((const bf16_t*)h, (bf16_t*)out, B, S0, n_keep, D, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_gather_tail_rows_ragged(const void* h, void* out, int32_t B, int32_t D, const int32_t* dev_rag_keep, int32_t total_keep,
                                             sv_stream stream) {
    if (!h || !out || !dev_rag_keep || B < 1 || total_keep < B || D < 8 || D % 8 || !rows_ok(total_keep))
        return fail(SV_EINVAL, "sv_op_gather_tail_rows_ragged: bad argument (descriptors given, B >= 1, total_keep >= B, D %% 8 == 0)");
    launch_gather_tail_rows((const bf16_t*)h, (bf16_t*)out, B, 0, 0, D, (hipStream_t)stream, dev_rag_keep, total_keep);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_gather_listed_rows(const void* x, int32_t ldx, const int32_t* dev_rows, int32_t n, void* out, int32_t D, sv_stream stream) {
    if (!x || !dev_rows || !out || !rows_ok(n) || D < 8 || D % 8 || ldx < D || ldx % 8)
        return fail(SV_EINVAL, "sv_op_gather_listed_rows: bad argument (D %% 8 == 0, ldx %% 8 == 0, ldx >= D)");
    launch_gather_listed_rows((const bf16_t*)x, ldx, dev_rows, n, (bf16_t*)out, D, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_ragged_row_pos(const int32_t* dev_rag_seq, int32_t B, int32_t* dev_row_pos, sv_stream stream) {
    if (!dev_rag_seq || !dev_row_pos || B < 1 || B > 65535) return fail(SV_EINVAL, "sv_op_ragged_row_pos: bad argument");
    launch_ragged_row_pos(dev_rag_seq, B, dev_row_pos, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_ragged_positions(int32_t* dev_positions, const int32_t* dev_rag_seq, int32_t B, int32_t rep, int32_t delta, sv_stream stream) {
    if (!dev_positions || !dev_rag_seq || B < 1 || rep < 1 || !rows_ok((int64_t)B * rep)) return fail(SV_EINVAL, "sv_op_ragged_positions: bad argument");
    launch_ragged_positions(dev_positions, dev_rag_seq, B * rep, rep, delta, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_token_batchnorm(const void* x, const void* w, const void* b, const void* running_mean, const void* running_var, void* y,
                                     int32_t B, int32_t Q, int32_t D, float eps, int64_t y_batch_stride, sv_stream stream) {
    if (!x || !w || !b || !running_mean || !running_var || !y || B < 1 || Q < 1 || D < 8 || D % 8 || !rows_ok((int64_t)B * Q))
        return fail(SV_EINVAL, "sv_op_token_batchnorm: bad argument (D %% 8 == 0)");
    if (y_batch_stride < (int64_t)Q * D || y_batch_stride % 8)
        return fail(SV_EINVAL, "sv_op_token_batchnorm: y_batch_stride %lld must be a multiple of 8 and >= Q * D", (long long)y_batch_stride);
    launch_token_batchnorm((const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (const bf16_t*)running_mean, (const bf16_t*)running_var,
                           (bf16_t*)y, B, Q, D, eps, (hipStream_t)stream, (size_t)y_batch_stride);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_layernorm_packed(const void* x, const void* gamma, const void* beta, void* y_xp, int32_t M, int32_t D, float eps,
                                      sv_stream stream) {
    if (!x || !gamma || !beta || !y_xp || !rows_ok(M) || D < 16 || D % 16) return fail(SV_EINVAL, "sv_op_layernorm_packed: bad argument (D %% 16 == 0)");
    launch_layernorm_rows_packed((const bf16_t*)x, D, (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y_xp, M, D, eps, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_pack_rows(const void* x, int32_t ldx, void* xp, int32_t M, int32_t K, sv_stream stream) {
    if (!x || !xp || !rows_ok(M) || K < 16 || K % 16 || ldx < K || ldx % 8 || (int64_t)M * (K / 8) > INT32_MAX)
        return fail(SV_EINVAL, "sv_op_pack_rows: bad argument (K %% 16 == 0, ldx %% 8 == 0, ldx >= K)");
    pack_rows((const bf16_t*)x, ldx, (bf16_t*)xp, M, K, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_unpack_rows(const void* xp, void* x, int32_t ldx, int32_t M, int32_t K, sv_stream stream) {
    if (!x || !xp || !rows_ok(M) || K < 16 || K % 16 || ldx < K || ldx % 8 || (int64_t)M * (K / 8) > INT32_MAX)
        return fail(SV_EINVAL, "sv_op_unpack_rows: bad argument (K %% 16 == 0, ldx %% 8 == 0, ldx >= K)");
    unpack_rows((const bf16_t*)xp, (bf16_t*)x, ldx, M, K, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

// row_update_ln_kernel<256> (D <= 2048) / <1024>: the fields of RowUpdateArgs; ws == NULL selects the embedding mode
extern "C" int sv_op_row_update_ln(const float* ws, int32_t splitk, int32_t ldws, int32_t rows_ws, const void* bias, void* h, int32_t ldh,
                                   const void* wte, const void* wpe, const int32_t* dev_tokens, const int32_t* dev_positions, const void* gamma,
                                   const void* beta, float eps, void* xp_out, int32_t M, int32_t D, sv_stream stream) {
    if (!h || !gamma || !beta || !xp_out || M < 1 || M > 65535) return fail(SV_EINVAL, "sv_op_row_update_ln: bad argument");
    if (D < 16 || D % 16 || D > 12288) return fail(SV_EINVAL, "sv_op_row_update_ln: D %d must be a multiple of 16 in 16..12288 (the row sits in LDS as fp32: 48 KiB)", D);
    if (ldh != 0 && (ldh < D || ldh % 8)) return fail(SV_EINVAL, "sv_op_row_update_ln: ldh %d must be 0 (fragment order) or a multiple of 8 and >= D", ldh);
    if (ws) {
        if (!bias || splitk < 1 || splitk > 64 || rows_ws < M || ldws < D || ldws % 4)
            return fail(SV_EINVAL, "sv_op_row_update_ln: residual mode needs a bias, 1 <= splitk <= 64, rows_ws >= M, ldws %% 4 == 0 and ldws >= D");
    } else if (!wte || !dev_tokens || !dev_positions) {
        return fail(SV_EINVAL, "sv_op_row_update_ln: embedding mode needs wte, tokens and positions");
    }
    RowUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.ws = ws; a.splitk = splitk; a.ldws = ldws; a.rows_ws = rows_ws; a.bias = (const bf16_t*)bias; a.h = (bf16_t*)h; a.ldh = ldh;
    a.wte = (const bf16_t*)wte; a.wpe = (const bf16_t*)wpe; a.tokens = dev_tokens; a.positions = dev_positions;
    a.g = (const bf16_t*)gamma; a.b = (const bf16_t*)beta; a.eps = eps; a.xp_out = (bf16_t*)xp_out; a.M = M; a.D = D;
    launch_row_update_ln(a, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_op_argmax(const float* logits, int32_t B, int32_t V, int32_t ld, int32_t* out, sv_stream stream) {
    if (!logits || !out || B < 1 || V < 1 || ld < V || ld % 4) return fail(SV_EINVAL, "sv_op_argmax: bad argument (ld must be a multiple of 4)");
    TmpBufs tmp;
    float* pv; int32_t* pi;
    SVCHECK(tmp.get(&pv, (size_t)B * 8));
    SVCHECK(tmp.get(&pi, (size_t)B * 8));
    launch_argmax(logits, ld, V, out, pv, pi, B, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// the continuous-batching selection on caller-given rows: cb_step_kernel itself, one block per row (slot b = row b), on a copy of the
// logits (vLLM-mode rows are rewritten in place) with each row's step, output counts and repetition set rebuilt from its history
// lps != nullptr (sv_op_cb_logprobs): row b records what lps[b] asks, one column, into out_logprob / out_rank [B] and out_ids / out_lps [B][ld_k]
static int op_cb_select_impl(const char* who, const float* logits, int32_t B, int32_t V, int32_t ld, const sv_cb_request* reqs,
                             const int32_t* history, int32_t ld_hist, const int32_t* hist_len, int32_t* out, const sv_cb_logprobs* lps,
                             float* out_logprob, int32_t* out_rank, int32_t* out_ids, float* out_lps, int32_t ld_k, sv_stream stream) {
    if (!logits || !reqs || !hist_len || !out || B < 1 || B > 4096 || V < 1 || ld < V || (ld & 3) || ld_hist < 0)
        return fail(SV_EINVAL, "%s: bad argument", who);
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        if (hist_len[b] < 0 || hist_len[b] > ld_hist || (hist_len[b] > 0 && !history))
            return fail(SV_EINVAL, "%s: row %d: history length %d (ld_hist %d)", who, b, hist_len[b], ld_hist);
        for (int t = 0; t < hist_len[b]; ++t)
            if (history[(size_t)b * ld_hist + t] < 0 || history[(size_t)b * ld_hist + t] >= V)
                return fail(SV_EINVAL, "%s: row %d: history id outside the vocabulary", who, b);
        max_len = std::max(max_len, (int)hist_len[b]);
        SVCHECK(cb_check_request(reqs[b], V, b, who));
    }
    if (lps) {
        if (!out_logprob || !out_rank || !out_ids || !out_lps || ld_k < 1) return fail(SV_EINVAL, "%s: null output or ld_k < 1", who);
        SVCHECK(cb_check_logprobs(reqs, lps, B, who));
        for (int b = 0; b < B; ++b)
            if (lps[b].enable && lps[b].k > ld_k) return fail(SV_EINVAL, "%s: row %d: k=%d exceeds ld_k=%d", who, b, lps[b].k, ld_k);
    }
    const int words = (ld + 31) / 32, ld_out = max_len + 1;
    std::vector<CbSlot> hs(B);
    std::vector<CbBias> hb(B);
    std::vector<uint32_t> seen((size_t)B * words, 0u), row;
    std::vector<uint16_t> counts((size_t)B * ld, 0);
    for (int b = 0; b < B; ++b) {
        const sv_cb_request& r = reqs[b];
        cb_fill_slot(r, hs[b], hb[b], row, words);
        hs[b].step = hist_len[b];
        const bool track = r.semantics == 1 || (r.repetition_penalty > 0.f && r.repetition_penalty != 1.0f);
        for (int t = 0; t < hist_len[b]; ++t) {
            const int id = history[(size_t)b * ld_hist + t];
            if (track) row[id >> 5] |= 1u << (id & 31);
            if (r.semantics == 1) counts[(size_t)b * ld + id] += 1;
        }
        std::copy(row.begin(), row.end(), seen.begin() + (size_t)b * words);
    }
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    float* lg;
    CbSlot* dslots;
    CbBias* dbias;
    uint32_t* dseen;
    uint16_t* dcounts;
    int32_t *dout, *dcur, *dpos, *dctr;
    SVCHECK(tmp.get(&lg, (size_t)B * ld));
    SVCHECK(tmp.get(&dslots, (size_t)B));
    SVCHECK(tmp.get(&dbias, (size_t)B));
    SVCHECK(tmp.get(&dseen, seen.size()));
    SVCHECK(tmp.get(&dcounts, counts.size()));
    SVCHECK(tmp.get(&dout, (size_t)B * ld_out));
    SVCHECK(tmp.get(&dcur, (size_t)B));
    SVCHECK(tmp.get(&dpos, (size_t)B));
    SVCHECK(tmp.get(&dctr, 3));
    HIPCHECK(hipMemcpyAsync(lg, logits, (size_t)B * ld * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemcpyAsync(dslots, hs.data(), hs.size() * sizeof(CbSlot), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dbias, hb.data(), hb.size() * sizeof(CbBias), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dseen, seen.data(), seen.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dcounts, counts.data(), counts.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(dout, 0, (size_t)B * ld_out * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(dcur, 0, (size_t)B * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(dpos, 0, (size_t)B * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(dctr, 0, 3 * sizeof(int32_t), st));
    CbStepArgs a;
    a.logits = lg; a.ld = ld; a.V = V; a.slots = dslots; a.slot_map = nullptr;
    a.cur_tok = dcur; a.positions = dpos; a.out_tokens = dout; a.ld_out = ld_out;
    a.seen = dseen; a.seen_words = words; a.n_live = dctr; a.events = dctr + 1; a.bad = dctr + 2;
    a.counts = dcounts; a.ld_counts = ld; a.bias = dbias;
    // the record of row b: column hist_len[b] (its step) of buffers that hold ld_out columns per row, as the engine's hold out_ld
    CbLogprobs* dlp = nullptr;
    float *dlogprob = nullptr, *dlps = nullptr;
    int32_t *drank = nullptr, *dids = nullptr;
    if (lps) {
        const size_t cols = (size_t)B * ld_out;
        SVCHECK(tmp.get(&dlp, (size_t)B));
        SVCHECK(tmp.get(&dlogprob, cols));
        SVCHECK(tmp.get(&drank, cols));
        SVCHECK(tmp.get(&dids, cols * SV_TOPK_MAX));
        SVCHECK(tmp.get(&dlps, cols * SV_TOPK_MAX));
        std::vector<CbLogprobs> hl(B);
        for (int b = 0; b < B; ++b) {
            CbLogprobs& h = hl[b];
            h.enable = lps[b].enable ? 1 : 0; h.k = h.enable ? lps[b].k : 0; h.source = h.enable ? lps[b].source : 0; h.pad_ = 0;
            h.logprob = dlogprob + (size_t)b * ld_out; h.rank = drank + (size_t)b * ld_out;
            h.ids = dids + (size_t)b * ld_out * SV_TOPK_MAX; h.lps = dlps + (size_t)b * ld_out * SV_TOPK_MAX;
        }
        HIPCHECK(hipMemcpyAsync(dlp, hl.data(), hl.size() * sizeof(CbLogprobs), hipMemcpyHostToDevice, st));
        HIPCHECK(hipStreamSynchronize(st));                 // `hl` is a host temporary
        a.lp = dlp;
    }
    launch_cb_step(a, B, st);
    HIPCHECK(hipGetLastError());
    std::vector<int32_t> ho((size_t)B * ld_out);
    HIPCHECK(hipMemcpyAsync(ho.data(), dout, ho.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) out[b] = ho[(size_t)b * ld_out + hist_len[b]];
    if (!lps) return 0;
    for (int b = 0; b < B; ++b) {                           // a row that records nothing reads (NaN, 0) and an empty list
        out_logprob[b] = std::nanf(""); out_rank[b] = 0;
        for (int j = 0; j < ld_k; ++j) { out_ids[(size_t)b * ld_k + j] = -1; out_lps[(size_t)b * ld_k + j] = -INFINITY; }
        if (!lps[b].enable) continue;
        const size_t t = (size_t)hist_len[b], k = (size_t)lps[b].k;
        HIPCHECK(hipMemcpy(out_logprob + b, dlogprob + (size_t)b * ld_out + t, sizeof(float), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(out_rank + b, drank + (size_t)b * ld_out + t, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (!k) continue;
        HIPCHECK(hipMemcpy(out_ids + (size_t)b * ld_k, dids + (size_t)b * ld_out * SV_TOPK_MAX + t * k, k * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(out_lps + (size_t)b * ld_k, dlps + (size_t)b * ld_out * SV_TOPK_MAX + t * k, k * sizeof(float), hipMemcpyDeviceToHost));
    }
    return 0;
}
extern "C" int sv_op_cb_select(const float* logits, int32_t B, int32_t V, int32_t ld, const sv_cb_request* reqs,
                               const int32_t* history, int32_t ld_hist, const int32_t* hist_len, int32_t* out, sv_stream stream) {
    return op_cb_select_impl("sv_op_cb_select", logits, B, V, ld, reqs, history, ld_hist, hist_len, out, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                             stream);
}
// sv_op_cb_select plus one sv_cb_logprobs per row: the recording form of cb_step_kernel, the device code of sv_cb_admit_logprobs' slots
extern "C" int sv_op_cb_logprobs(const float* logits, int32_t B, int32_t V, int32_t ld, const sv_cb_request* reqs, const sv_cb_logprobs* lps,
                                 const int32_t* history, int32_t ld_hist, const int32_t* hist_len, int32_t* out, float* out_logprob,
                                 int32_t* out_rank, int32_t* out_ids, float* out_lps, int32_t ld_k, sv_stream stream) {
    if (!lps) return fail(SV_EINVAL, "sv_op_cb_logprobs: null lps");
    return op_cb_select_impl("sv_op_cb_logprobs", logits, B, V, ld, reqs, history, ld_hist, hist_len, out, lps, out_logprob, out_rank, out_ids, out_lps,
                             ld_k, stream);
}

// ---- drafting in the continuous batch (sv_cb_set_lookup): forced drafts, and cb_lookup_step_kernel on caller-given state ----
extern "C" int sv_debug_cb_set_lookup_drafts(sv_engine* e, const int32_t* host_ids, int32_t n, int32_t ld) {
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->cb_active) return fail(SV_ESTATE, "sv_debug_cb_set_lookup_drafts: a continuous batch is active (set the drafts before the first admit)");
    if (host_ids) {
        if (n < 1 || n > e->cfg.max_batch || ld < 1 || ld > e->cfg.max_seq_len)
            return fail(SV_EINVAL, "sv_debug_cb_set_lookup_drafts: bad n %d / ld %d (max_batch %d, max_seq_len %d)", n, ld, e->cfg.max_batch, e->cfg.max_seq_len);
        for (size_t i = 0; i < (size_t)n * ld; ++i)      // a draft is fed to the embedding table
            if (host_ids[i] < 0 || host_ids[i] >= e->cfg.vocab)
                return fail(SV_EINVAL, "sv_debug_cb_set_lookup_drafts: id %d outside the vocabulary (%d)", host_ids[i], e->cfg.vocab);
    }
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipDeviceSynchronize());                // no step in flight reads the buffer
    cb_drop_graphs(e);                               // the kept steps carry the buffer and its shape by value
    e->cb_lk_forced_n = 0; e->cb_lk_forced_ld = 0;
    if (!host_ids) return 0;
    if (!e->cb_lk_forced) SVCHECK(dalloc(e, &e->cb_lk_forced, (size_t)e->cfg.max_batch * e->cfg.max_seq_len));
    HIPCHECK(hipMemcpy(e->cb_lk_forced, host_ids, (size_t)n * ld * sizeof(int32_t), hipMemcpyHostToDevice));
    e->cb_lk_forced_n = n; e->cb_lk_forced_ld = ld;
    return 0;
}

extern "C" int sv_op_cb_lookup_step(const float* logits, int32_t n, int32_t K, int32_t V, int32_t ld, const sv_cb_request* reqs,
                                    const sv_cb_logprobs* lps, const int32_t* base, int32_t* live, int32_t* history, int32_t ld_hist,
                                    int32_t* hist_len, int32_t* rows, int32_t* positions, int32_t* n_draft, int32_t max_ngram, int32_t min_ngram,
                                    const int32_t* forced, int32_t forced_n, int32_t forced_ld, int32_t* counts, int32_t* flags3,
                                    float* out_logprob, int32_t* out_rank, sv_stream stream) {
    const char* who = "sv_op_cb_lookup_step";
    if (!logits || !reqs || !base || !live || !history || !hist_len || !rows || !positions || !n_draft || !counts || !flags3)
        return fail(SV_EINVAL, "%s: null argument", who);
    if (n < 1 || n > 256 || V < 1 || ld < V || (ld & 3) || ld_hist < 1) return fail(SV_EINVAL, "%s: bad argument", who);
    sv_lookup lk_in{K, max_ngram, min_ngram}, lk;
    SVCHECK(cb_check_lookup(who, &lk_in, lk));
    if (K < 1) return fail(SV_EINVAL, "%s: num_draft_tokens %d (1..%d)", who, K, SV_LOOKUP_MAX_DRAFT);
    const int K1 = K + 1;
    if (forced && (forced_n < 1 || forced_ld < 1)) return fail(SV_EINVAL, "%s: bad forced_n %d / forced_ld %d", who, forced_n, forced_ld);
    if (lps && (!out_logprob || !out_rank)) return fail(SV_EINVAL, "%s: lps without host_logprob / host_rank", who);
    if (lps) SVCHECK(cb_check_logprobs(reqs, lps, n, who));
    for (int s = 0; s < n; ++s) {
        SVCHECK(cb_check_request(reqs[s], V, s, who));
        if (hist_len[s] < 0 || hist_len[s] + K1 > ld_hist)
            return fail(SV_EINVAL, "%s: slot %d: history length %d + %d rows exceed ld_hist %d", who, s, hist_len[s], K1, ld_hist);
        if (live[s] && hist_len[s] >= reqs[s].max_new_tokens) return fail(SV_EINVAL, "%s: slot %d: live with its budget %d spent", who, s, reqs[s].max_new_tokens);
        if (n_draft[s] < 0 || n_draft[s] > K) return fail(SV_EINVAL, "%s: slot %d: n_draft %d outside 0..%d", who, s, n_draft[s], K);
        for (int t = 0; t < hist_len[s]; ++t)
            if (history[(size_t)s * ld_hist + t] < 0 || history[(size_t)s * ld_hist + t] >= V) return fail(SV_EINVAL, "%s: slot %d: history id outside the vocabulary", who, s);
        for (int j = 0; j < K1; ++j)
            if (rows[s * K1 + j] < 0 || rows[s * K1 + j] >= V) return fail(SV_EINVAL, "%s: slot %d: row id outside the vocabulary", who, s);
    }
    for (size_t i = 0; forced && i < (size_t)std::min(n, forced_n) * forced_ld; ++i)
        if (forced[i] < 0 || forced[i] >= V) return fail(SV_EINVAL, "%s: forced id outside the vocabulary", who);
    const int words = (ld + 31) / 32, R = n * K1;
    std::vector<CbSlot> hs(n);
    std::vector<CbBias> hb(n);
    std::vector<uint32_t> seen((size_t)n * words, 0u), row;
    std::vector<uint16_t> cnt((size_t)n * ld, 0);
    for (int s = 0; s < n; ++s) {
        const sv_cb_request& r = reqs[s];
        cb_fill_slot(r, hs[s], hb[s], row, words);
        hs[s].step = hist_len[s]; hs[s].live = live[s] ? 1 : 0; hs[s].base = base[s];
        const bool track = r.semantics == 1 || (r.repetition_penalty > 0.f && r.repetition_penalty != 1.0f);
        for (int t = 0; t < hist_len[s]; ++t) {
            const int id = history[(size_t)s * ld_hist + t];
            if (track) row[id >> 5] |= 1u << (id & 31);
            if (r.semantics == 1) cnt[(size_t)s * ld + id] += 1;
        }
        std::copy(row.begin(), row.end(), seen.begin() + (size_t)s * words);
    }
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    float *lg, *dlogprob = nullptr, *dlps = nullptr;
    CbSlot* dslots; CbBias* dbias; uint32_t* dseen; uint16_t* dcnt; CbLogprobs* dlp = nullptr;
    int32_t *dout, *dcur, *dpos, *dctr, *dstate, *dforced = nullptr, *drank = nullptr, *dids = nullptr;
    SVCHECK(tmp.get(&lg, (size_t)R * ld));
    SVCHECK(tmp.get(&dslots, (size_t)n));
    SVCHECK(tmp.get(&dbias, (size_t)n));
    SVCHECK(tmp.get(&dseen, seen.size()));
    SVCHECK(tmp.get(&dcnt, cnt.size()));
    SVCHECK(tmp.get(&dout, (size_t)n * ld_hist));
    SVCHECK(tmp.get(&dcur, (size_t)R));
    SVCHECK(tmp.get(&dpos, (size_t)R));
    SVCHECK(tmp.get(&dctr, 3));
    SVCHECK(tmp.get(&dstate, (size_t)4 * n + 3));        // n_draft [n] | counts [n][3] | totals [3]
    if (forced) SVCHECK(tmp.get(&dforced, (size_t)forced_n * forced_ld));
    HIPCHECK(hipMemcpyAsync(lg, logits, (size_t)R * ld * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemcpyAsync(dslots, hs.data(), hs.size() * sizeof(CbSlot), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dbias, hb.data(), hb.size() * sizeof(CbBias), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dseen, seen.data(), seen.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dcnt, cnt.data(), cnt.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dout, history, (size_t)n * ld_hist * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dcur, rows, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dpos, positions, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(dctr, 0, 3 * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(dstate, 0, ((size_t)4 * n + 3) * sizeof(int32_t), st));
    HIPCHECK(hipMemcpyAsync(dstate, n_draft, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (forced) HIPCHECK(hipMemcpyAsync(dforced, forced, (size_t)forced_n * forced_ld * sizeof(int32_t), hipMemcpyHostToDevice, st));
    CbLookupArgs q;
    CbStepArgs& a = q.st;
    a.logits = lg; a.ld = ld; a.V = V; a.slots = dslots; a.slot_map = nullptr;
    a.cur_tok = dcur; a.positions = dpos; a.out_tokens = dout; a.ld_out = ld_hist;
    a.seen = dseen; a.seen_words = words; a.n_live = dctr; a.events = dctr + 1; a.bad = dctr + 2;
    a.counts = dcnt; a.ld_counts = ld; a.bias = dbias;
    q.K = K; q.max_ngram = lk.max_ngram; q.min_ngram = lk.min_ngram; q.first = 0;
    q.n_draft = dstate; q.counts = dstate + n; q.totals = q.counts + 3 * n;
    q.forced = dforced; q.forced_n = forced ? forced_n : 0; q.forced_ld = forced_ld;
    std::vector<CbLogprobs> hl;
    if (lps) {
        const size_t cols = (size_t)n * ld_hist;
        SVCHECK(tmp.get(&dlp, (size_t)n));
        SVCHECK(tmp.get(&dlogprob, cols));
        SVCHECK(tmp.get(&drank, cols));
        SVCHECK(tmp.get(&dids, cols * SV_TOPK_MAX));
        SVCHECK(tmp.get(&dlps, cols * SV_TOPK_MAX));
        hl.resize(n);
        for (int s = 0; s < n; ++s) {
            CbLogprobs& h = hl[s];
            h.enable = lps[s].enable ? 1 : 0; h.k = h.enable ? lps[s].k : 0; h.source = h.enable ? lps[s].source : 0; h.pad_ = 0;
            h.logprob = dlogprob + (size_t)s * ld_hist; h.rank = drank + (size_t)s * ld_hist;
            h.ids = dids + (size_t)s * ld_hist * SV_TOPK_MAX; h.lps = dlps + (size_t)s * ld_hist * SV_TOPK_MAX;
        }
        HIPCHECK(hipMemcpyAsync(dlp, hl.data(), hl.size() * sizeof(CbLogprobs), hipMemcpyHostToDevice, st));
        a.lp = dlp;
    }
    launch_cb_lookup_step(q, n, st);
    HIPCHECK(hipGetLastError());
    std::vector<int32_t> ctr(3), state((size_t)4 * n + 3);
    std::vector<CbSlot> after(n);
    HIPCHECK(hipMemcpyAsync(history, dout, (size_t)n * ld_hist * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(rows, dcur, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(positions, dpos, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(ctr.data(), dctr, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(state.data(), dstate, state.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(after.data(), dslots, after.size() * sizeof(CbSlot), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int s = 0; s < n; ++s) {
        const int L0 = hist_len[s], L1 = after[s].step;
        if (lps) {
            for (int j = 0; j < K1; ++j) { out_logprob[s * K1 + j] = std::nanf(""); out_rank[s * K1 + j] = 0; }
            if (lps[s].enable && L1 > L0) {
                HIPCHECK(hipMemcpy(out_logprob + s * K1, dlogprob + (size_t)s * ld_hist + L0, (size_t)(L1 - L0) * sizeof(float), hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(out_rank + s * K1, drank + (size_t)s * ld_hist + L0, (size_t)(L1 - L0) * sizeof(int32_t), hipMemcpyDeviceToHost));
            }
        }
        live[s] = after[s].live; hist_len[s] = L1; n_draft[s] = state[s];
        for (int k = 0; k < 3; ++k) counts[3 * s + k] = state[n + 3 * s + k];
    }
    flags3[0] = -ctr[0]; flags3[1] = 0; flags3[2] = ctr[2];
    return 0;
}

// ban_tokens_kernel (processors.hip) on caller-given rows and histories: rewrites dev_logits in place
extern "C" int sv_op_ban_tokens(float* dev_logits, int32_t B, int32_t V, int32_t ld, const int32_t* hist, int32_t ld_hist, const int32_t* hist_len,
                                const sv_logits_processors* lp, sv_stream stream) {
    if (!dev_logits || !hist_len || !lp || B < 1 || B > 4096 || V < 1 || ld < V || ld_hist < 0) return fail(SV_EINVAL, "sv_op_ban_tokens: bad argument");
    SVCHECK(check_logits_processors(lp, V, "sv_op_ban_tokens"));
    for (int b = 0; b < B; ++b) {
        if (hist_len[b] < 0 || hist_len[b] > ld_hist || (hist_len[b] > 0 && !hist))
            return fail(SV_EINVAL, "sv_op_ban_tokens: row %d: history length %d (ld_hist %d)", b, hist_len[b], ld_hist);
        for (int t = 0; t < hist_len[b]; ++t)
            if (hist[(size_t)b * ld_hist + t] < 0 || hist[(size_t)b * ld_hist + t] >= V)
                return fail(SV_EINVAL, "sv_op_ban_tokens: row %d: history id outside the vocabulary", b);
    }
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t *dhist, *dlen;
    BanWord* dwords;
    std::vector<BanWord> words;
    ban_word_table(*lp, words);
    const size_t nh = (size_t)B * (size_t)(ld_hist > 0 ? ld_hist : 1);
    SVCHECK(tmp.get(&dhist, nh));
    SVCHECK(tmp.get(&dlen, (size_t)B));
    SVCHECK(tmp.get(&dwords, words.size()));
    if (ld_hist > 0 && hist) HIPCHECK(hipMemcpyAsync(dhist, hist, (size_t)B * ld_hist * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dlen, hist_len, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(dwords, words.data(), words.size() * sizeof(BanWord), hipMemcpyHostToDevice, st));
    BanArgs a;
    a.logits = dev_logits; a.ld = ld; a.V = V; a.B = B;
    a.hist = dhist; a.ld_hist = ld_hist; a.step = nullptr; a.hist_len = dlen; a.done = nullptr;
    a.ngram = lp->no_repeat_ngram_size; a.words = dwords; a.n_words = lp->n_bad_words;
    launch_ban_tokens(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// sv_forward_logprobs runs its lm_head over `rows` rows at a time (0 = the default); the workspace follows at the next call
extern "C" int sv_debug_set_score_chunk_rows(sv_engine* e, int32_t rows) {
    if (rows < 0 || rows > 65536 || rows % 256) return fail(SV_EINVAL, "sv_debug_set_score_chunk_rows: rows=%d must be 0 or a multiple of 256 up to 65536", rows);
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    e->score_chunk_rows = rows;
    return 0;
}

// logprob_rows_kernel (score.hip) on caller-given rows
extern "C" int sv_op_logprob_rows(const void* dev_logits_bf16, int32_t R, int32_t V, int32_t ld, const int32_t* dev_targets, float temperature,
                                  float* dev_logprob, float* dev_logsumexp, float* dev_entropy, int32_t* dev_argmax, int32_t* host_flag2,
                                  sv_stream stream) {
    if (!dev_logits_bf16 || R < 1 || R > (1 << 22) || V < 1 || ld < V || (ld & 7) || ((uintptr_t)dev_logits_bf16 & 15))
        return fail(SV_EINVAL, "sv_op_logprob_rows: bad argument (rows 16-byte aligned, ld a multiple of 8 and >= V)");
    if (!dev_logprob && !dev_logsumexp && !dev_entropy && !dev_argmax) return fail(SV_EINVAL, "sv_op_logprob_rows: every output pointer is null");
    if (dev_logprob && !dev_targets) return fail(SV_EINVAL, "sv_op_logprob_rows: logprob asked for without targets");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(SV_EINVAL, "sv_op_logprob_rows: temperature must be finite and > 0");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t* flag;
    SVCHECK(tmp.get(&flag, 2));
    const int32_t flag0[2] = {0, 0x7fffffff};
    HIPCHECK(hipMemcpy(flag, flag0, sizeof(flag0), hipMemcpyHostToDevice));
    LogprobArgs a;
    a.logits = (const bf16_t*)dev_logits_bf16; a.ld = ld; a.V = V; a.R = R; a.targets = dev_targets; a.inv_t = 1.0f / temperature;
    a.logprob = dev_logprob; a.lse = dev_logsumexp; a.entropy = dev_entropy; a.argmax = dev_argmax; a.bad = flag; a.row0 = 0;
    launch_logprob_rows(a, st);
    HIPCHECK(hipGetLastError());
    int32_t hf[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(hf, flag, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (host_flag2) { host_flag2[0] = hf[0]; host_flag2[1] = hf[0] ? hf[1] : -1; }
    return 0;
}

// topk_rows_bf16_kernel (score.hip) on caller-given rows and the lse sv_op_logprob_rows left for them
extern "C" int sv_op_topk_rows_bf16(const void* dev_logits_bf16, int32_t R, int32_t V, int32_t ld, const int32_t* dev_targets, float temperature,
                                    const float* dev_logsumexp, int32_t k, int32_t* dev_topk_ids, float* dev_topk_logprobs, int32_t* dev_rank,
                                    sv_stream stream) {
    if (!dev_logits_bf16 || R < 1 || R > (1 << 22) || V < 1 || ld < V || (ld & 7) || ((uintptr_t)dev_logits_bf16 & 15))
        return fail(SV_EINVAL, "sv_op_topk_rows_bf16: bad argument (rows 16-byte aligned, ld a multiple of 8 and >= V)");
    if (k < 1 || k > SV_TOPK_MAX) return fail(SV_EINVAL, "sv_op_topk_rows_bf16: k=%d must be in 1..%d", k, SV_TOPK_MAX);
    if (!dev_logsumexp || !dev_topk_ids || !dev_topk_logprobs) return fail(SV_EINVAL, "sv_op_topk_rows_bf16: null dev_logsumexp / dev_topk_ids / dev_topk_logprobs");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(SV_EINVAL, "sv_op_topk_rows_bf16: temperature must be finite and > 0");
    hipStream_t st = (hipStream_t)stream;
    TopkRowsArgs a;
    a.logits = (const bf16_t*)dev_logits_bf16; a.ld = ld; a.V = V; a.R = R; a.targets = dev_targets; a.inv_t = 1.0f / temperature;
    a.lse = dev_logsumexp; a.k = k; a.ids = dev_topk_ids; a.logprobs = dev_topk_logprobs; a.rank = dev_rank;
    launch_topk_rows_bf16(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}
// token_topk_rows_kernel (sampling.hip): the source-0 row function of sv_generate_topk on caller-given rows
extern "C" int sv_op_token_topk(const float* dev_logits, int32_t B, int32_t V, int32_t ld, float temperature, const int32_t* dev_tokens, int32_t k,
                                int32_t* dev_ids, float* dev_logprobs, int32_t* dev_rank, sv_stream stream) {
    if (!dev_logits || B < 1 || B > (1 << 22) || V < 1 || ld < V) return fail(SV_EINVAL, "sv_op_token_topk: bad argument (B >= 1, V >= 1, ld >= V)");
    if (k < 1 || k > SV_TOPK_MAX) return fail(SV_EINVAL, "sv_op_token_topk: k=%d must be in 1..%d", k, SV_TOPK_MAX);
    if (!dev_ids || !dev_logprobs) return fail(SV_EINVAL, "sv_op_token_topk: null dev_ids / dev_logprobs");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(SV_EINVAL, "sv_op_token_topk: temperature must be finite and > 0");
    hipStream_t st = (hipStream_t)stream;
    TokenTopkRowsArgs a;
    a.rows = dev_logits; a.ld = ld; a.V = V; a.B = B; a.temperature = temperature; a.tokens = dev_tokens; a.k = k;
    a.ids = dev_ids; a.logprobs = dev_logprobs; a.rank = dev_rank;
    launch_token_topk_rows(a, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

extern "C" int sv_op_sample(const float* logits, int32_t B, int32_t V, int32_t ld, float temperature, int32_t top_k,
                            float top_p, uint64_t seed, int32_t step, int32_t* out, sv_stream stream);
extern "C" int sv_op_sample_top_p(const float* logits, int32_t B, int32_t V, int32_t ld, float temperature, float top_p,
                                  uint64_t seed, int32_t step, int32_t* out, sv_stream stream) {
    return sv_op_sample(logits, B, V, ld, temperature, 0, top_p, seed, step, out, stream);
}
extern "C" int sv_op_sample(const float* logits, int32_t B, int32_t V, int32_t ld, float temperature, int32_t top_k,
                            float top_p, uint64_t seed, int32_t step, int32_t* out, sv_stream stream) {
    if (!logits || !out || B < 1 || V < 1 || ld < V || !(temperature > 0.f) || !(top_p > 0.f))
        return fail(SV_EINVAL, "sv_op_sample: bad argument");
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    int32_t* dstep;
    SVCHECK(tmp.get(&dstep, 1));
    HIPCHECK(hipMemcpyAsync(dstep, &step, sizeof(int32_t), hipMemcpyHostToDevice, st));
    SampleArgs sa;
    sa.logits = logits; sa.ld = ld; sa.V = V; sa.B = B; sa.temperature = temperature; sa.top_p = top_p; sa.top_k = top_k; sa.seed = seed;
    sa.step = dstep; sa.out = out; sa.scratch = nullptr; sa.seen = nullptr; sa.seen_words = 0; sa.penalty = 1.f;
    launch_sample_top_p(sa, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

// launch_capture_rows (capture_warp_kernel + capture_write_kernel, sampling.hip) on caller-given rows: the launch sv_generate_ex makes per step,
// at device step 0 of a one-step call.  The descriptor, the step / done scalars and the per-row thresholds live in temporaries of this call.
extern "C" int sv_op_capture_rows(const float* dev_rows, int32_t B, int32_t V, int32_t ld, const uint32_t* dev_seen, int32_t seen_words,
                                  float penalty, int32_t eos_token_id, int32_t hold_eos, int32_t do_sample, float temperature, int32_t top_k,
                                  float top_p, float min_p, float* dev_scores_out, float* dev_logits_out, int64_t ld_out, sv_stream stream) {
    const char* who = "sv_op_capture_rows";
    if (!dev_rows || (!dev_scores_out && !dev_logits_out)) return fail(SV_EINVAL, "%s: null dev_rows, or neither output given", who);
    if (B < 1 || B > 65535 || V < 1 || ld < V || ld_out < V)
        return fail(SV_EINVAL, "%s: bad shape (B %d in 1..65535, V %d >= 1, ld %d and ld_out %lld >= V)", who, B, V, ld, (long long)ld_out);
    if (dev_seen && (seen_words < (V + 31) / 32 || !(penalty > 0.f) || !std::isfinite(penalty)))
        return fail(SV_EINVAL, "%s: a seen bitmap needs seen_words >= ceil(V / 32) and a finite penalty > 0", who);
    if (hold_eos && eos_token_id >= V) return fail(SV_EINVAL, "%s: eos_token_id %d outside the vocabulary", who, eos_token_id);
    if (do_sample && (!(temperature > 0.f) || !std::isfinite(temperature) || !(top_p > 0.f) || !(top_p <= 1.f) || !(min_p >= 0.f) || !(min_p <= 1.f)))
        return fail(SV_EINVAL, "%s: temperature must be finite and > 0, top_p in (0, 1], min_p in [0, 1]", who);
    hipStream_t st = (hipStream_t)stream;
    TmpBufs tmp;
    CaptureDesc* ddesc;
    int32_t* scalars;                                                // {step, done}
    float* warp;
    SVCHECK(tmp.get(&ddesc, 1));
    SVCHECK(tmp.get(&scalars, 2));
    SVCHECK(tmp.get(&warp, (size_t)B * 8));
    CaptureDesc hd;
    hd.scores = dev_scores_out; hd.logits = dev_logits_out; hd.ld = ld_out; hd.rows = B; hd.max_new = 1;
    HIPCHECK(hipMemcpyAsync(ddesc, &hd, sizeof(hd), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(scalars, 0, 2 * sizeof(int32_t), st));
    CaptureArgs c;
    c.desc = ddesc; c.src = dev_rows; c.ld_src = ld; c.V = V; c.B = B; c.step = scalars; c.done = scalars + 1;
    c.seen = dev_seen; c.seen_words = dev_seen ? seen_words : 0; c.penalty = dev_seen ? penalty : 1.f;
    c.eos = eos_token_id; c.min_new = hold_eos ? 1 : 0;
    c.do_sample = do_sample ? 1 : 0; c.temperature = do_sample ? temperature : 1.f; c.top_p = do_sample ? top_p : 1.f; c.top_k = top_k;
    c.warp = (do_sample && dev_scores_out) ? warp : nullptr;
    c.minp_log = (do_sample && min_p > 0.f) ? logf(min_p) : -INFINITY; c.what = 3;
    launch_capture_rows(c, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));                              // hd and the temporaries are this call's
    return 0;
}
