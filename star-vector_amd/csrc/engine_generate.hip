// Host driver, part 3 of 5: sv_generate* -- the stop state lives on the device, one decode step is captured as a hipGraph and replayed.
//   sel_mode / sample_and_finish   the selection a call's sv_sampling asks for, and the launches of one step behind the lm_head
//   generate_beam                  beam search over the same decode step (its graph is a GraphSlot of the call)
//   GenCall / check_gen_call       one validator behind the C ABI entry points; generate_retry = the optimistic-ownership second attempt
//   GenFrame                       the call frame of the two non-beam drivers: budget checks, lock + stream ordering + cb_guard, prompt pass + state +
//                                  first token + its one round trip, the streaming helper, the poll of the device block, report + tokens + timing
//   lookup_attempt                 B x (K + 1) aliased rows, verification step, kept in e->lk_step; polls after every chunk of 8
//   generate_attempt               B x G rows, the plain step, kept in e->gen_step (+ e->gen_multi: U steps per launch); polls only when something can end the call
// and the standalone beam scorer's C ABI (sv_beam_*).  The kept graphs are GraphSlots (engine_internal.h): dropping and replacing is theirs.
#include "engine_internal.h"

// What a call's sv_sampling asks of the selection, derived once: the repetition penalty is on for a factor > 0 other than 1 (seen = the engine's
// bitmap then), the min-length hold for min_new_tokens > 0 with an EOS id inside the vocabulary (min_new = 0 when it is off)
struct SelMode { bool pen; int min_new; uint32_t* seen; };
static SelMode sel_mode(const sv_engine* e, const sv_sampling& sp) {
    const bool pen = sp.repetition_penalty > 0.f && sp.repetition_penalty != 1.0f;
    const bool hold = sp.min_new_tokens > 0 && sp.eos_token_id >= 0 && sp.eos_token_id < e->cfg.vocab;
    return {pen, hold ? sp.min_new_tokens : 0, pen ? e->seen : nullptr};
}
// sample from e->logits into next_tok, then the bookkeeping kernel
// fused: the lm_head launch in front has already left every row's best (value, lowest index) in e->amax (gemm.hip, SkinnyArgs::amax):
// no argmax launch, finish_step_kernel decodes the keys
static FinishArgs make_finish_args(sv_engine* e, int B, const sv_sampling& sp, int max_new, bool fused) {
    FinishArgs f;
    f.pval = sp.do_sample ? nullptr : e->am_val; f.pidx = sp.do_sample ? nullptr : e->am_idx;
    f.amax = fused ? e->amax : nullptr;
    f.next = e->next_tok; f.cur_tok = e->cur_tok; f.unfinished = e->unfinished; f.positions = e->positions;
    f.out_tokens = e->out_tok; f.ld_out = e->out_ld; f.step = e->d_step; f.done = e->d_done; f.n_emitted = e->d_nemit;
    f.stop_ids = e->d_stop; f.n_stop = sp.n_stop; f.eos = sp.eos_token_id; f.pad = sp.pad_token_id; f.B = B;
    f.max_new = max_new;
    f.seen = sel_mode(e, sp).seen; f.seen_words = e->seen_words;
    f.V = e->cfg.vocab; f.bad = e->d_bad;
    return f;
}
// sv_generate_ex outputs: the step's raw row and processed row, BEFORE suppress_token rewrites the EOS logit in place
// what: 1 = the raw row, 2 = the processed row, 3 = both (CaptureArgs::what)
static void capture_step(sv_engine* e, int B, const sv_sampling& sp, hipStream_t st, int what = 3) {
    const SelMode m = sel_mode(e, sp);
    CaptureArgs c;
    c.desc = e->cap_desc; c.src = e->logits; c.ld_src = e->Vpad; c.V = e->cfg.vocab; c.B = B;
    c.step = e->d_step; c.done = e->d_done;
    c.seen = m.seen; c.seen_words = e->seen_words; c.penalty = sp.repetition_penalty;
    c.eos = sp.eos_token_id;
    c.min_new = m.min_new;
    c.do_sample = sp.do_sample ? 1 : 0; c.temperature = sp.temperature; c.top_p = sp.top_p; c.top_k = sp.top_k;
    c.warp = (sp.do_sample && e->cap_host.scores) ? e->cap_warp : nullptr;
    c.minp_log = e->minp_log; c.what = what;
    launch_capture_rows(c, st);
}
// sv_generate_stats: the statistics of the token this step emits (TokenStatsArgs::what: 1 = the raw row's sums, 2 = the outputs, 3 = both)
static void token_stats_step(sv_engine* e, int B, const sv_sampling& sp, hipStream_t st, int what) {
    const SelMode m = sel_mode(e, sp);
    TokenStatsArgs a;
    a.desc = e->ts_desc; a.src = e->logits; a.ld_src = e->Vpad; a.V = e->cfg.vocab; a.B = B;
    a.step = e->d_step; a.done = e->d_done; a.unfinished = e->unfinished;
    a.next = e->next_tok; a.pval = sp.do_sample ? nullptr : e->am_val; a.pidx = sp.do_sample ? nullptr : e->am_idx;
    a.seen = m.seen; a.seen_words = e->seen_words; a.penalty = sp.repetition_penalty;
    a.eos = sp.eos_token_id;
    a.min_new = m.min_new;
    a.do_sample = sp.do_sample ? 1 : 0; a.temperature = sp.temperature; a.top_p = sp.top_p; a.top_k = sp.top_k;
    a.minp_log = e->minp_log; a.raw = e->ts_raw; a.what = what;
    launch_token_stats(a, st);
}
// sv_generate_topk: the k best ids of this step's distribution and the rank of the emitted token (TokenTopkArgs, kernels.h)
static_assert(SV_TOPK_MAX == SV_TOPK_MAX_DEV, "topk.h's list length is the ABI's");
static void token_topk_step(sv_engine* e, int B, const sv_sampling& sp, hipStream_t st, bool want_rank) {
    const SelMode m = sel_mode(e, sp);
    TokenTopkArgs a;
    a.desc = e->tk_desc; a.src = e->logits; a.ld_src = e->Vpad; a.V = e->cfg.vocab; a.B = B;
    a.step = e->d_step; a.done = e->d_done; a.unfinished = e->unfinished;
    a.next = e->next_tok; a.pval = sp.do_sample ? nullptr : e->am_val; a.pidx = sp.do_sample ? nullptr : e->am_idx;
    a.seen = m.seen; a.seen_words = e->seen_words; a.penalty = sp.repetition_penalty;
    a.eos = sp.eos_token_id;
    a.min_new = m.min_new;
    a.do_sample = sp.do_sample ? 1 : 0; a.temperature = sp.temperature; a.top_p = sp.top_p; a.top_k = sp.top_k;
    a.minp_log = e->minp_log; a.k = e->tk_k; a.source = e->tk_source; a.want_rank = want_rank ? 1 : 0;
    launch_token_topk(a, st);
}
static void sample_and_finish(sv_engine* e, int B, const sv_sampling& sp, int max_new, hipStream_t st, bool fused = false) {
    if (fused && e->fin_folded) { e->fin_folded = false; return; }      // the lm_head launch in front did the selection AND the bookkeeping (SkinnyArgs::finish)
    // sv_generate_stats: one launch between the selection and the bookkeeping; a step that rewrites the raw row in place (a ban, the min-length
    // hold) takes the raw row's sums in a launch of their own in front of the rewrite (a statistics call never folds: fused is off for it)
    const SelMode m = sel_mode(e, sp);
    const bool rewrite = e->ban_ngram > 0 || e->ban_nwords > 0 || m.min_new > 0;
    const bool ts_split = e->ts_on && rewrite;
    if (ts_split) token_stats_step(e, B, sp, st, 1);
    // sv_generate_topk, source 0 on such a step: the raw list is taken here as well, without the rank (the token is not known yet; a request for
    // it was refused before the call began)
    const bool tk_front = e->tk_on && e->tk_source == 0 && rewrite;
    if (tk_front) token_topk_step(e, B, sp, st, false);
    if (e->ban_ngram > 0 || e->ban_nwords > 0) {
        // sv_generate_processed with a ban: the raw row goes out first, the banned ids become -inf in e->logits, then everything below -- the score
        // capture, the min-length hold, the repetition penalty, the selection -- reads the banned row (-inf stays -inf through all of them)
        if (e->cap_on && e->cap_host.logits) capture_step(e, B, sp, st, 1);
        BanArgs ba;
        ba.logits = e->logits; ba.ld = e->Vpad; ba.V = e->cfg.vocab; ba.B = B;
        ba.hist = e->out_tok; ba.ld_hist = e->out_ld; ba.step = e->d_step; ba.hist_len = nullptr; ba.done = e->d_done;
        ba.ngram = e->ban_ngram; ba.words = e->ban_words; ba.n_words = e->ban_nwords;
        launch_ban_tokens(ba, st);
        if (e->cap_on && e->cap_host.scores) capture_step(e, B, sp, st, 2);
    } else if (e->cap_on) capture_step(e, B, sp, st);                   // (a capturing call never folds: fused is off for it)
    if (m.min_new > 0) suppress_token(e->logits, e->Vpad, sp.eos_token_id, e->d_step, m.min_new, B, st);
    if (sp.do_sample) {
        SampleArgs sa;
        sa.logits = e->logits; sa.ld = e->Vpad; sa.V = e->cfg.vocab; sa.B = B; sa.temperature = sp.temperature;
        sa.top_p = sp.top_p; sa.top_k = sp.top_k; sa.seed = sp.seed; sa.step = e->d_step; sa.out = e->next_tok; sa.scratch = e->sample_scratch;
        sa.seen = m.seen; sa.seen_words = e->seen_words; sa.penalty = sp.repetition_penalty;
        sa.minp_log = e->minp_log;
        launch_sample_top_p(sa, st);
    } else if (!fused) {
        launch_argmax_partial(e->logits, e->Vpad, e->cfg.vocab, e->am_val, e->am_idx, B, m.seen, e->seen_words,
                              sp.repetition_penalty, st);
    }
    if (e->ts_on) token_stats_step(e, B, sp, st, ts_split ? 2 : 3);
    if (e->tk_on && !tk_front) token_topk_step(e, B, sp, st, e->tk_rank);
    const FinishArgs f = make_finish_args(e, B, sp, max_new, fused);
    launch_finish_step(f, st);
}

// timing[0] = prompt pass + first token, [1] = the rest of the call (it ends now), [2] = decode steps, timing_graph = steps per graph launch (0: no graph)
using GenClock = std::chrono::steady_clock;
static void set_timing(sv_engine* e, GenClock::time_point t0, GenClock::time_point t1, double steps, double per_launch) {
    e->timing[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->timing[1] = std::chrono::duration<double, std::milli>(GenClock::now() - t1).count();
    e->timing[2] = steps;
    e->timing_graph = per_launch;
}

// ------------------------------------------------------------------------------------------------
// beam search (num_beams > 1): HF _beam_search restated on device (beam.hip).  The prompt is prefilled ONCE per
// request: its full KV pages are shared by all beams through the block table, only the partially filled tail page
// is private to a beam (HF expands the prompt to B * num_beams rows and prefills every copy).
// ------------------------------------------------------------------------------------------------
// lens (ragged prompt pass): the prompt pages the beams of request b share are lens[b] / SV_PAGE_TOKENS instead of shared_pages
static int upload_beam_table(sv_engine* e, int B, int nb, int need, int shared_pages, bool prefill_rows, hipStream_t st, const int32_t* lens = nullptr) {
    std::vector<int32_t> table((size_t)e->cfg.max_batch * e->pages_per_seq, 0);
    if (prefill_rows) {
        for (int b = 0; b < B; ++b)             // request b writes its prompt into the pages of beam row b * nb
            for (int i = 0; i < need; ++i) table[(size_t)b * e->pages_per_seq + i] = (b * nb) * need + i;
    } else {
        for (int r = 0; r < B * nb; ++r)
            for (int i = 0; i < need; ++i)
                table[(size_t)r * e->pages_per_seq + i] = (i < (lens ? lens[r / nb] / SV_PAGE_TOKENS : shared_pages) ? (r / nb) * nb : r) * need + i;
    }
    HIPCHECK(hipMemcpyAsync(e->block_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

static void beam_step(sv_engine* e, const BeamKvArgs& kv, int logit_div, hipStream_t st) {
    e->beam.enqueue_step(e->logits, e->Vpad, logit_div, st);
    launch_beam_table_reorder(kv, st);
    launch_beam_tail_copy(kv, st);
}

// lens != nullptr: the ragged form (sv_generate_ragged) -- S0 is the longest prompt, request b has lens[b] prompt rows
static int generate_beam(sv_engine* e, const void* dev_embeds, int B, int S0, const int32_t* lens, const sv_sampling* sp, int max_new,
                         const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, hipStream_t st) {
    const sv_config& c = e->cfg;
    const int nb = sp->num_beams, R = B * nb;
    if (nb > BM_MAXNB) return fail(SV_EINVAL, "num_beams %d unsupported (2..%d)", nb, BM_MAXNB);
    if (R > c.max_batch) return fail(SV_EINVAL, "batch %d x num_beams %d exceeds engine max_batch %d", B, nb, c.max_batch);
    if (sp->early_stopping < 0 || sp->early_stopping > 2) return fail(SV_EINVAL, "early_stopping must be 0 (False), 1 (True) or 2 (\"never\")");
    if (!dev_embeds || B < 1) return fail(SV_EINVAL, "generate: bad batch %d", B);
    if (S0 < 1) return fail(SV_EINVAL, "generate: bad prompt length %d", S0);
    const int need = (S0 + max_new + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS;
    if (need > e->pages_per_seq) return fail(SV_EINVAL, "sequence length %d exceeds max_seq_len %d", S0 + max_new, c.max_seq_len);

    auto t0 = GenClock::now();
    HIPCHECK(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), st));         // a flag left by an earlier, failed call is not this call's
    BeamConfig bc;
    bc.B = B; bc.nb = nb; bc.V = c.vocab; bc.max_new = max_new; bc.eos = sp->eos_token_id; bc.pad = sp->pad_token_id;
    bc.early = sp->early_stopping; bc.length_penalty = sp->length_penalty;
    bc.penalty = sp->repetition_penalty > 0.f ? sp->repetition_penalty : 1.f;
    bc.n_stop = sp->n_stop;
    for (int i = 0; i < sp->n_stop; ++i) bc.stop[i] = sp->stop_ids[i];
    bc.do_sample = sp->do_sample ? 1 : 0; bc.temperature = sp->temperature; bc.top_p = sp->top_p; bc.top_k = sp->top_k;
    bc.seed = sp->seed;
    bc.min_new = sp->min_new_tokens > 0 ? sp->min_new_tokens : 0;
    if (!e->beam.matches(bc)) {
        int r = e->beam.init(bc, e->cur_tok, e->positions, e->d_step, e->d_done);
        if (r) return fail(SV_ENOMEM, "beam scorer allocation failed (hip error %d)", r);
    }
    e->beam.c = bc;
    struct BeamCap { BeamScorer* s; ~BeamCap() { s->cap = nullptr; } } beam_cap{&e->beam};
    e->beam.cap = e->cap_on ? e->cap_desc : nullptr;           // every beam_step below (eager and captured) writes the outputs
    e->beam.cap_temp = sp->temperature;
    // prompt pass over the B requests, written into the pages of each request's first beam row
    SVCHECK(upload_beam_table(e, B, nb, need, 0, true, st));
    if (lens) SVCHECK(prefill_forward_ragged(e, (const bf16_t*)dev_embeds, B, lens, st));
    else SVCHECK(prefill_forward(e, (const bf16_t*)dev_embeds, B, S0, st));
    SVCHECK(upload_beam_table(e, B, nb, need, S0 / SV_PAGE_TOKENS, false, st, lens));
    e->cached_B = R;
    {
        int r = e->beam.reset(st);
        if (r) return fail(SV_EHIP, "beam scorer reset failed (hip error %d)", r);
    }
    if (lens) ragged_positions(e, B, nb, -1, st);
    else fill_i32(e->positions, S0 - 1, R, st);      // beam_update adds 1
    BeamKvArgs kv;
    kv.block_table = e->block_table; kv.max_pages = e->pages_per_seq; kv.need = need; kv.parent = e->beam.d.parent;
    kv.step = e->d_step; kv.done = e->d_done; kv.S0 = S0; kv.L_fixed = S0; kv.B = B; kv.nb = nb;
    kv.rag_seq = lens ? e->d_rag : nullptr;     // (the descriptors prefill_forward_ragged uploaded: they live until the next ragged pass)
    kv.kv_pool = e->kv_pool; kv.layer_stride = e->layer_stride; kv.kv_head_stride = e->kv_head_stride;
    kv.n_layer = c.n_layer; kv.n_kv = e->nkv; kv.page_bytes = e->page_bytes;
    launch_beam_tail_copy(kv, st);              // the prompt's tail page fans out to beams 1.. (parent = first beam row)
    kv.L_fixed = -1;
    beam_step(e, kv, nb, st);                   // first token: every beam of a request reads the request's logits row
    HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_DONE], e->d_done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    auto t1 = GenClock::now();

    int steps = 0;
    const int chunk = sp->sync_every > 0 ? sp->sync_every : 32;
    GraphSlot step;                             // this call's own (kv travels by value in it): released on every way out
    const auto one_step = [&]() { decode_forward(e, R, st); beam_step(e, kv, 1, st); };
    if (!e->h_flags[HF_DONE] && graph_enabled()) SVCHECK(step.use("", st, 1, one_step));
    while (!e->h_flags[HF_DONE]) {
        int n = max_new - 1 - steps;
        if (n <= 0) break;
        if (n > chunk) n = chunk;
        for (int i = 0; i < n; ++i) {
            if (step.x) HIPCHECK(hipGraphLaunch(step.x, st));
            else one_step();
        }
        steps += n;
        HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_DONE], e->d_done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
    }
    const double gexec_used = step.x ? 1.0 : 0.0;
    step.drop();
    // the decode steps of a beam search run the fused MLP launch too: its give-up code must not come back as rc 0 with hypotheses
    // built from void logits
    SVCHECK(check_finite_logits(e, st, "sv_generate (beam search)"));
    if (!e->h_flags[HF_DONE]) return fail(SV_EHIP, "beam search did not terminate within its budget");
    std::vector<int64_t> toks, bidx;
    std::vector<float> scores;
    int L = 0;
    const bool want_bidx = outs && outs->host_beam_indices;
    {
        int r = e->beam.finalize(st, toks, L, scores, want_bidx ? &bidx : nullptr);
        if (r) return fail(SV_EHIP, "beam search bookkeeping failed (code %d)", r);
    }
    if (want_bidx) memcpy(outs->host_beam_indices, bidx.data(), bidx.size() * sizeof(int64_t));
    if (outs && outs->host_sequences_scores) memcpy(outs->host_sequences_scores, scores.data(), scores.size() * sizeof(float));
    HIPCHECK(hipMemcpy2DAsync(dev_out_tokens, (size_t)max_new * sizeof(int64_t), toks.data(), (size_t)max_new * sizeof(int64_t),
                              (size_t)L * sizeof(int64_t), B, hipMemcpyHostToDevice, st));
    HIPCHECK(hipStreamSynchronize(st));
    set_timing(e, t0, t1, (double)steps, gexec_used);
    *n_generated = L;
    return 0;
}

// The selection kernels raise a device flag when a row had no finite logit (a numeric failure upstream: the token they emit
// is then 0 instead of the out-of-range sentinel, so nothing indexes the embedding table out of bounds); the entry points
// turn it into an error instead of returning made-up tokens.
int sveng::check_finite_logits(sv_engine* e, hipStream_t st, const char* who) {
    HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_BAD], e->d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return report_bad_logits(e, st, who, e->h_flags[HF_BAD]);
}
int sveng::report_bad_logits(sv_engine* e, hipStream_t st, const char* who, int what) {
    if (!what) return 0;
    HIPCHECK(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), st));
    // (The failed steps may have appended non-finite K / V rows to their pages.  Nothing is scrubbed here: the decode attention clears the stale
    //  V columns of a sequence's current key group itself -- attention.hip, process() -- so a page's next owner never multiplies them.)
    HIPCHECK(hipStreamSynchronize(st));
    if (what == 4 && e->rc_dbg) {
        long long d[8] = {0};
        int32_t stepv = -1;
        (void)hipMemcpy(d, e->rc_dbg, sizeof(d), hipMemcpyDeviceToHost);
        (void)hipMemcpy(&stepv, e->d_step, sizeof(stepv), hipMemcpyDeviceToHost);
        (void)hipMemset(e->rc_dbg, 0, sizeof(d));
        fprintf(stderr, "[sv] rowln_cattn give-up: block %lld wave %lld ks0 %lld waited %lld ticks, x0 %016llx, layer %lld, rows %lld; device step %d\n",
                d[0], d[1], d[2], d[3], (unsigned long long)d[4], d[5], d[6], stepv);
    }
    if (what == 3 || what == 4) {
        e->last_giveup = what;
        if (e->cfg.exclusive_device == 2 && !e->fused_off) {
            // optimistic ownership (sv_config.exclusive_device = 2) did not hold: from here on this engine decodes without the launches that need
            // every block resident.  sv_generate runs the failed call again (below); the step-wise entry points report this one failure.
            e->fused_off = true;
            e->xpa_armed = false;
            cb_drop_graphs(e);                   // the continuous-batching step graphs were captured with the fused launches (sv_generate's carry the flag in their key)
            fprintf(stderr, "[starvector_amd] a fused decode launch gave up waiting (code %d): this GPU is shared -- the engine continues WITHOUT the all-blocks-resident "
                            "launches (same tokens, ~8 %% more time per step); create it with exclusive_device = 0 to start that way\n", what);
        }
    }
    if (what == 3 || what == 4)
        return fail(SV_EHIP, "%s: a block of a fused decode launch (code %d: 3 = MLP pair, 4 = row update + c_attn) gave up waiting for its producers (its blocks were not all resident at "
                             "once?  another process or engine on this GPU?); the tokens of this call are void -- create the engine with "
                             "exclusive_device = 0 (SV_EXP_MLP_FUSED_OFF) there", who, what);
    {
        int32_t stepv = -1;
        (void)hipMemcpy(&stepv, e->d_step, sizeof(stepv), hipMemcpyDeviceToHost);
        return fail(SV_EHIP, "%s: a row of logits had no finite value (NaN / Inf in the weights or inputs?) [code %d, device step %d]", who, what, stepv);
    }
}

// One generate call as its entry point describes it (internal: the public header knows nothing of it).  `who` is the entry point whose checks run
// and whose name their messages carry: a call handed over (topk NULL -> sv_generate_stats, stats NULL -> sv_generate_processed, an all-zero lp ->
// sv_generate_shared) is described again by the entry point that takes it.
enum : unsigned {
    GC_ARGS = 1,         // the checks that need no engine run (sv_generate_ex: none, everything is the engine's)
    GC_LENS = 2,         // host_lens is required (sv_generate_ragged)
    GC_LP_FIRST = 4,     // the processors are checked right behind the pointers (sv_generate_processed), not last (sv_generate_stats / _topk)
};
struct GenCall {
    const char* who;
    unsigned checks;
    const void* embeds;
    int32_t B, S0;                    // behind check_gen_call S0 is the longest prompt: the budget counts from it
    const int32_t* lens;              // nullptr: B prompts of S0 rows each
    int32_t n_samples;                // G: samples per prompt -- one prompt pass over the B prompts, B * G decode rows
    const sv_sampling* sp;
    const sv_logits_processors* lp;   // nullptr unless some processor is set
    const sv_generate_outputs* outs;
    const sv_token_stats* stats;
    const sv_token_topk* topk;
    int64_t* dev_out_tokens;
    int32_t* n_generated;
    sv_stream stream;
    const sv_lookup* lookup = nullptr;      // sv_generate_lookup: the call verifies drafts (lookup_attempt), defaults resolved
    int32_t* counts3 = nullptr;             //   its {steps, drafted, accepted}, or nullptr
};
static bool lp_any(const sv_logits_processors* lp) { return lp && (lp->no_repeat_ngram_size != 0 || lp->n_bad_words != 0 || lp->min_p != 0.f); }
static int check_token_topk(const sv_sampling* sp, const sv_logits_processors* lp, const sv_token_topk* tk, int max_new);
// The checks that need no engine (they come first: they are the same on a machine without a GPU), in the order the entry points have always
// run them, and the longest prompt.  max_new <= 0 is refused later, by the call itself.
static int check_gen_call(GenCall& c) {
    if (!(c.checks & GC_ARGS)) return 0;
    const char* who = c.who;
    const sv_sampling* sp = c.sp;
    if (!c.embeds || ((c.checks & GC_LENS) && !c.lens) || !sp || !c.dev_out_tokens || !c.n_generated) return fail(SV_EINVAL, "%s: null argument", who);
    if (c.stats && !c.stats->dev_logprob && !c.stats->dev_logprob_processed && !c.stats->dev_entropy)
        return fail(SV_EINVAL, "%s: dev_logprob, dev_logprob_processed and dev_entropy are all NULL (pass stats = NULL for a call without statistics)", who);
    if (c.checks & GC_LP_FIRST) SVCHECK(check_logits_processors(c.lp, 0, who));
    if (sp->num_beams > 1 && !c.topk) {      // (a top-k call refuses beams among its own checks, below)
        if (c.stats)
            return fail(SV_EINVAL, "%s: token statistics with num_beams %d are not built (beam search reports sequences_scores; beam rows reorder)", who,
                        sp->num_beams);
        if (c.lp)
            return fail(SV_EINVAL, "%s: no_repeat_ngram_size / bad words / min_p with num_beams %d is not built (beam rows reorder their histories)", who,
                        sp->num_beams);
    }
    if (c.B < 1) return fail(SV_EINVAL, "%s: bad B=%d", who, c.B);
    if (c.n_samples < 1) return fail(SV_EINVAL, "%s: bad n_samples=%d (must be >= 1)", who, c.n_samples);
    int longest = c.S0;
    if (c.lens) {
        longest = 0;
        for (int b = 0; b < c.B; ++b) {
            if (c.lens[b] < 1) return fail(SV_EINVAL, "%s: length %d of sequence %d (must be >= 1)", who, c.lens[b], b);
            longest = c.lens[b] > longest ? c.lens[b] : longest;
        }
    } else if (c.S0 < 1) {
        return fail(SV_EINVAL, "%s: bad S0=%d", who, c.S0);
    }
    const int max_new = sp->max_length - longest;
    if (c.topk) SVCHECK(check_token_topk(sp, c.lp, c.topk, max_new));
    if (c.stats && max_new > 0 && c.stats->ld < (int64_t)max_new)
        return fail(SV_EINVAL, "%s: %sld %lld must be >= max_new %d (max_length %d - prompt length %d)", who, c.topk ? "stats " : "", (long long)c.stats->ld,
                    max_new, sp->max_length, longest);
    if (!(c.checks & GC_LP_FIRST)) SVCHECK(check_logits_processors(c.lp, 0, who));
    c.S0 = longest;
    return 0;
}

static int generate_attempt(sv_engine* e, const GenCall& c);
static int generate_retry(sv_engine* e, const GenCall& c) {
    if (e) { e->last_giveup = 0; e->stream_skip = 0; }
    int rc = generate_attempt(e, c);
    if (rc != 0 && e && e->cfg.exclusive_device == 2 && e->last_giveup && e->fused_off) {
        e->last_giveup = 0;      // (the second attempt runs every step again: the statistics columns are rewritten completely, like the capture slabs)
        rc = generate_attempt(e, c);
    }
    if (e) e->stream_skip = 0;
    return rc;
}

// sv_config.exclusive_device = 2: OPTIMISTIC ownership.  The fused launches run as if the engine owned its GPU; if one gives up (another process
// holds CUs: the bounded wait of rowops.hip / mlp_fused.hip, never a hang, never tokens) the engine switches them off for good (report_bad_logits) and
// THIS call is run again from its prompt pass.  The kernels with and without the fused launches are bit-identical (tests/test_gpu_e2e.py), the
// sampler's random stream is a function of (seed, step, row): the second attempt re-derives exactly the columns the first one had already handed
// to a streaming callback, and skips them.
// (the second attempt runs every step again: the capture slabs of sv_generate_ex are rewritten completely)
extern "C" int sv_generate_ex(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, const sv_sampling* sp,
                              const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    GenCall c{"sv_generate_ex", 0, dev_embeds, B, S0, nullptr, 1, sp, nullptr, outs, nullptr, nullptr, dev_out_tokens, n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}
// The ragged form: sequences of lengths host_lens[b], packed.  HF's padded-batch semantics: the budget counts from the longest prompt.
extern "C" int sv_generate_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, const sv_sampling* sp,
                                  const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    GenCall c{"sv_generate_ragged", GC_ARGS | GC_LENS, dev_embeds_packed, B, 0, host_lens, 1, sp, nullptr, outs, nullptr, nullptr, dev_out_tokens,
              n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}
// n_samples continuations of every prompt from ONE prompt pass.  host_lens == NULL: B prompts of S0 rows each; otherwise the ragged form (S0 unused).
// Row b * n_samples + j of the outputs is sample j of prompt b: the rows, tokens and random draws of sv_generate / sv_generate_ragged over the
// prompts repeated n_samples times each.
extern "C" int sv_generate_shared(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                                  const sv_sampling* sp, const sv_generate_outputs* outs, int64_t* dev_out_tokens, int32_t* n_generated,
                                  sv_stream stream) {
    GenCall c{"sv_generate_shared", GC_ARGS, dev_embeds_packed, B, S0, host_lens, n_samples, sp, nullptr, outs, nullptr, nullptr, dev_out_tokens,
              n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}
extern "C" int sv_generate(sv_engine* e, const void* dev_embeds, int32_t B, int32_t S0, const sv_sampling* sp,
                           int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    return sv_generate_ex(e, dev_embeds, B, S0, sp, nullptr, dev_out_tokens, n_generated, stream);
}

// ------------------------------------------------------------------------------------------------
// sv_generate_processed: HF's no_repeat_ngram_size / bad_words_ids / min_p
// ------------------------------------------------------------------------------------------------
int sveng::check_logits_processors(const sv_logits_processors* lp, int V, const char* who) {
    if (!lp) return 0;
    if (lp->no_repeat_ngram_size < 0 || lp->no_repeat_ngram_size > SV_BAN_MAXNGRAM)
        return fail(SV_EINVAL, "%s: no_repeat_ngram_size %d unsupported (0..%d)", who, lp->no_repeat_ngram_size, SV_BAN_MAXNGRAM);
    if (lp->n_bad_words < 0 || lp->n_bad_words > SV_BAN_MAXWORDS)
        return fail(SV_EINVAL, "%s: %d bad-word sequences (at most %d)", who, lp->n_bad_words, SV_BAN_MAXWORDS);
    if (lp->n_bad_words > 0 && (!lp->bad_word_lens || !lp->bad_word_ids)) return fail(SV_EINVAL, "%s: n_bad_words > 0 but bad_word_lens / bad_word_ids is null", who);
    if (!(lp->min_p >= 0.f && lp->min_p <= 1.f)) return fail(SV_EINVAL, "%s: min_p must lie in [0, 1]", who);
    size_t off = 0;
    for (int i = 0; i < lp->n_bad_words; ++i) {
        const int L = lp->bad_word_lens[i];
        if (L < 1 || L > SV_BAN_MAXLEN) return fail(SV_EINVAL, "%s: bad-word sequence %d has %d ids (1..%d)", who, i, L, SV_BAN_MAXLEN);
        for (int k = 0; k < L; ++k) {
            const int id = lp->bad_word_ids[off + k];
            if (id < 0 || (V > 0 && id >= V)) return fail(SV_EINVAL, "%s: bad-word sequence %d: id %d outside the vocabulary", who, i, id);
        }
        off += (size_t)L;
    }
    return 0;
}
void sveng::ban_word_table(const sv_logits_processors& lp, std::vector<BanWord>& out) {
    out.assign((size_t)(lp.n_bad_words > 0 ? lp.n_bad_words : 1), BanWord{});
    size_t off = 0;
    for (int i = 0; i < lp.n_bad_words; ++i) {
        out[i].len = lp.bad_word_lens[i];
        for (int k = 0; k < out[i].len; ++k) out[i].id[k] = lp.bad_word_ids[off + k];
        off += (size_t)out[i].len;
    }
}
// the call's processors into the engine (cleared again by generate_attempt's guard); the ids are checked against the engine's vocabulary here
static int setup_processors(sv_engine* e, const sv_sampling* sp, const sv_logits_processors* lp, hipStream_t st) {
    if (!lp) return 0;
    SVCHECK(check_logits_processors(lp, e->cfg.vocab, "sv_generate_processed"));
    if (lp->n_bad_words > 0) {
        if (!e->ban_words) SVCHECK(dalloc(e, &e->ban_words, (size_t)SV_BAN_MAXWORDS));
        ban_word_table(*lp, e->ban_host);
        HIPCHECK(hipMemcpyAsync(e->ban_words, e->ban_host.data(), (size_t)lp->n_bad_words * sizeof(BanWord), hipMemcpyHostToDevice, st));
    }
    e->ban_ngram = lp->no_repeat_ngram_size;
    e->ban_nwords = lp->n_bad_words;
    e->minp_log = (sp->do_sample && lp->min_p > 0.f) ? logf(lp->min_p) : -INFINITY;
    return 0;
}
extern "C" int sv_generate_processed(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                                     const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs,
                                     int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    if (!lp_any(lp)) return sv_generate_shared(e, dev_embeds_packed, B, host_lens, S0, n_samples, sp, outs, dev_out_tokens, n_generated, stream);
    GenCall c{"sv_generate_processed", GC_ARGS | GC_LP_FIRST, dev_embeds_packed, B, S0, host_lens, n_samples, sp, lp, outs, nullptr, nullptr,
              dev_out_tokens, n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}

// validation of sv_generate_ex's outputs, and the descriptor of the call's slabs (allocated on first use, rewritten on the call's stream in front
// of everything the call enqueues: a kept graph reads the new slab addresses)
static int setup_capture(sv_engine* e, const sv_sampling* sp, const sv_generate_outputs* outs, int rows, int max_new, hipStream_t st) {
    e->cap_on = false;
    if (!outs) return 0;
    const bool beam = sp->num_beams > 1;
    if (!beam && (outs->host_sequences_scores || outs->host_beam_indices))
        return fail(SV_EINVAL, "sv_generate_ex: host_sequences_scores / host_beam_indices are beam-search outputs (num_beams > 1)");
    if (!outs->dev_scores && !outs->dev_logits) return 0;
    if (outs->ld < e->cfg.vocab || outs->ld > ((int64_t)1 << 31))
        return fail(SV_EINVAL, "sv_generate_ex: ld %lld must be >= vocab %d", (long long)outs->ld, e->cfg.vocab);
    if (!e->cap_desc) {
        SVCHECK(dalloc(e, &e->cap_desc, 1));
        SVCHECK(dalloc(e, &e->cap_warp, (size_t)e->cfg.max_batch * 8));
    }
    e->cap_host.scores = outs->dev_scores; e->cap_host.logits = outs->dev_logits; e->cap_host.ld = (long long)outs->ld;
    e->cap_host.rows = rows; e->cap_host.max_new = max_new;
    HIPCHECK(hipMemcpyAsync(e->cap_desc, &e->cap_host, sizeof(CaptureDesc), hipMemcpyHostToDevice, st));
    e->cap_on = true;
    return 0;
}

// sv_generate_stats: the descriptor of the call's three buffers (allocated on first use, rewritten on the call's stream in front of everything the
// call enqueues: a kept graph reads the new addresses).  The argument checks that need no engine are sv_generate_stats's own.
static int setup_token_stats(sv_engine* e, const sv_sampling* sp, const sv_token_stats* ts, int rows, int max_new, hipStream_t st) {
    e->ts_on = false;
    if (!ts) return 0;
    if (sp->num_beams > 1) return fail(SV_EINVAL, "sv_generate_stats: token statistics with num_beams %d are not built", sp->num_beams);
    if (ts->ld < max_new) return fail(SV_EINVAL, "sv_generate_stats: ld %lld must be >= max_new %d", (long long)ts->ld, max_new);
    if (!e->ts_desc) {
        SVCHECK(dalloc(e, &e->ts_desc, 1));
        SVCHECK(dalloc(e, &e->ts_raw, (size_t)e->cfg.max_batch * 4));
    }
    e->ts_host.logprob = ts->dev_logprob; e->ts_host.processed = ts->dev_logprob_processed; e->ts_host.entropy = ts->dev_entropy;
    e->ts_host.ld = (long long)ts->ld; e->ts_host.rows = rows; e->ts_host.max_new = max_new;
    HIPCHECK(hipMemcpyAsync(e->ts_desc, &e->ts_host, sizeof(TokenStatsDesc), hipMemcpyHostToDevice, st));
    e->ts_on = true;
    return 0;
}
// sv_generate_processed plus the per-token statistics of the roll-out (include/starvector_hip.h): stats NULL = exactly sv_generate_processed.
extern "C" int sv_generate_stats(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                                 const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs, const sv_token_stats* stats,
                                 int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    if (!stats) return sv_generate_processed(e, dev_embeds_packed, B, host_lens, S0, n_samples, sp, lp, outs, dev_out_tokens, n_generated, stream);
    GenCall c{"sv_generate_stats", GC_ARGS, dev_embeds_packed, B, S0, host_lens, n_samples, sp, lp_any(lp) ? lp : nullptr, outs, stats, nullptr,
              dev_out_tokens, n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}

// sv_generate_topk: the checks that need no engine (the same on a machine without a GPU); max_new <= 0 is refused later, by the call itself
static int check_token_topk(const sv_sampling* sp, const sv_logits_processors* lp, const sv_token_topk* tk, int max_new) {
    if (tk->k < 1 || tk->k > SV_TOPK_MAX) return fail(SV_EINVAL, "sv_generate_topk: k=%d must be in 1..%d", tk->k, SV_TOPK_MAX);
    if (tk->source != 0 && tk->source != 1)
        return fail(SV_EINVAL, "sv_generate_topk: source=%d must be 0 (log_softmax(raw / T)) or 1 (the processed scores)", tk->source);
    if (!tk->dev_ids || !tk->dev_logprobs) return fail(SV_EINVAL, "sv_generate_topk: dev_ids / dev_logprobs is NULL (pass topk = NULL for a call without the lists)");
    if (sp->num_beams > 1)
        return fail(SV_EINVAL, "sv_generate_topk: top-k lists with num_beams %d are not built (beam search reports sequences_scores; beam rows reorder)",
                    sp->num_beams);
    if (max_new > 0 && tk->ld < (int64_t)max_new)
        return fail(SV_EINVAL, "sv_generate_topk: ld %lld must be >= max_new %d", (long long)tk->ld, max_new);
    // (no engine here, so no vocabulary bound: sample_and_finish holds the EOS id only when it is < vocab, and a min_new_tokens call whose
    //  EOS id lies outside the vocabulary is refused its raw rank although nothing would be rewritten -- conservative, and such a call has no EOS)
    const bool rewrite = (lp && (lp->no_repeat_ngram_size != 0 || lp->n_bad_words != 0)) || (sp->min_new_tokens > 0 && sp->eos_token_id >= 0);
    if (tk->source == 0 && tk->dev_rank && rewrite)
        return fail(SV_EINVAL, "sv_generate_topk: dev_rank with source 0 and a processor that rewrites the raw row (no_repeat_ngram_size, bad words, "
                               "min_new_tokens): the raw list is taken in front of the rewrite, where the token is not known yet -- use source 1, or pass no dev_rank");
    return 0;
}
static int setup_token_topk(sv_engine* e, const sv_sampling* sp, const sv_token_topk* tk, int rows, int max_new, hipStream_t st) {
    e->tk_on = false;
    if (!tk) return 0;
    SVCHECK(check_token_topk(sp, nullptr, tk, max_new));
    if (!e->tk_desc) SVCHECK(dalloc(e, &e->tk_desc, 1));
    e->tk_host.ids = tk->dev_ids; e->tk_host.logprobs = tk->dev_logprobs; e->tk_host.rank = tk->dev_rank;
    e->tk_host.ld = (long long)tk->ld; e->tk_host.rows = rows; e->tk_host.max_new = max_new;
    HIPCHECK(hipMemcpyAsync(e->tk_desc, &e->tk_host, sizeof(TokenTopkDesc), hipMemcpyHostToDevice, st));
    e->tk_k = tk->k; e->tk_source = tk->source; e->tk_rank = tk->dev_rank != nullptr;
    e->tk_on = true;
    return 0;
}
// sv_generate_stats plus the top-k lists (include/starvector_hip.h): topk NULL = exactly sv_generate_stats.
extern "C" int sv_generate_topk(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, int32_t n_samples,
                                const sv_sampling* sp, const sv_logits_processors* lp, const sv_generate_outputs* outs, const sv_token_stats* stats,
                                const sv_token_topk* topk, int64_t* dev_out_tokens, int32_t* n_generated, sv_stream stream) {
    if (!topk) return sv_generate_stats(e, dev_embeds_packed, B, host_lens, S0, n_samples, sp, lp, outs, stats, dev_out_tokens, n_generated, stream);
    GenCall c{"sv_generate_topk", GC_ARGS, dev_embeds_packed, B, S0, host_lens, n_samples, sp, lp_any(lp) ? lp : nullptr, outs, stats, topk,
              dev_out_tokens, n_generated, stream};
    SVCHECK(check_gen_call(c));
    return generate_retry(e, c);
}

// ------------------------------------------------------------------------------------------------
// Shared prompt pass (sv_generate_shared): B prompts, G samples each, ONE prompt pass over the B prompts.
// ------------------------------------------------------------------------------------------------
static int ensure_fork_buffers(sv_engine* e) {
    const size_t mb = (size_t)e->cfg.max_batch;
    if (!e->h_fork) HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_fork), (mb * e->pages_per_seq + 6 * mb) * sizeof(int32_t), hipHostMallocDefault));
    return e->fork_desc ? 0 : dalloc(e, &e->fork_desc, 6 * mb);      // (the group admit of a continuous batch may have allocated the device side)
}
void sveng::fork_args(sv_engine* e, int n_prompts, int n_rows, ForkArgs& f) {
    const int mb = e->cfg.max_batch;
    f.prompts = e->fork_desc; f.dst_rows = e->fork_desc + 4 * mb; f.lsrc = e->fork_desc + 5 * mb; f.n_prompts = n_prompts; f.n_rows = n_rows;
    f.block_table = e->block_table; f.max_pages = e->pages_per_seq;
    f.kv_pool = e->kv_pool; f.layer_stride = e->layer_stride; f.kv_head_stride = e->kv_head_stride; f.n_layer = e->cfg.n_layer; f.n_kv = e->nkv;
    f.page_bytes = e->page_bytes; f.logits = e->logits; f.ld = e->Vpad;
}
// The page plan (static, like the beam path's): the G rows of prompt b share block-table entries 0 .. len_b / 64 - 1 -- the prompt's FULL pages,
// written by the prompt pass through the table of row b * G and by nobody afterwards: a decode step writes K / V at its row's own position only,
// which lies in a page from len_b / 64 on, and the decode attention clears the stale rows of a key group in registers (attention.hip, process()),
// never in memory.  From entry len_b / 64 (the partially filled tail page, if any) up to the end of the budget every row owns its pages; the fork
// launch copies the tail page from row b * G to the other rows and hands every row its prompt's logits.  No host round trip in between.
static int shared_prefill_fork(sv_engine* e, const void* dev_embeds, int B, int G, int S0, const int32_t* lens, int max_new, hipStream_t st) {
    const sv_config& c = e->cfg;
    const int R = B * G, mp = e->pages_per_seq, mb = c.max_batch;
    if (!dev_embeds) return fail(SV_EINVAL, "sv_generate_shared: null inputs_embeds");
    if (S0 < 1 || S0 > c.max_seq_len) return fail(SV_EINVAL, "sv_generate_shared: S0=%d out of range (max_seq_len %d)", S0, c.max_seq_len);
    SVCHECK(ensure_fork_buffers(e));
    reset_free_pages(e);
    if (e->table_pending) { HIPCHECK(hipEventSynchronize(e->table_ev)); e->table_pending = false; }      // (guards both pinned images)
    int32_t* table = e->h_table;                       // decode rows
    int32_t* pf = e->h_fork;                           // prompt pass: row b = the pages of decode row b * G
    int32_t* desc = e->h_fork + (size_t)mb * mp;
    memset(table, 0, (size_t)mb * mp * sizeof(int32_t));
    memset(pf, 0, ((size_t)mb * mp + 6 * (size_t)mb) * sizeof(int32_t));
    for (int b = 0; b < B; ++b) {
        const int len = lens ? lens[b] : S0, sh = len / SV_PAGE_TOKENS;
        const int need = (len + max_new + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS;
        if (need > mp) return fail(SV_EINVAL, "sequence length %d exceeds max_seq_len %d", len + max_new, c.max_seq_len);
        const int32_t* first = table + (size_t)b * G * mp;
        for (int j = 0; j < G; ++j) {
            int32_t* row = table + (size_t)(b * G + j) * mp;
            for (int i = 0; i < need; ++i) {
                if (j > 0 && i < sh) { row[i] = first[i]; continue; }
                row[i] = e->free_pages.back();
                e->free_pages.pop_back();
            }
            desc[5 * mb + b * G + j] = b;              // logits row of the prompt
            if (j > 0) desc[4 * mb + b * (G - 1) + j - 1] = b * G + j;
        }
        for (int i = 0; i < (len + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS; ++i) pf[(size_t)b * mp + i] = first[i];
        desc[4 * b] = b * G; desc[4 * b + 1] = len; desc[4 * b + 2] = b * (G - 1); desc[4 * b + 3] = G - 1;
    }
    HIPCHECK(hipMemcpyAsync(e->block_table, table, (size_t)mb * mp * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(e->cb_table_pf, pf, (size_t)mb * mp * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(e->fork_desc, desc, 6 * (size_t)mb * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(e->table_ev, st));
    e->table_pending = true;
    if (lens) SVCHECK(prefill_forward_ragged(e, (const bf16_t*)dev_embeds, B, lens, st, e->cb_table_pf));
    else SVCHECK(prefill_forward(e, (const bf16_t*)dev_embeds, B, S0, st, 0, nullptr, e->cb_table_pf));
    ForkArgs f;
    fork_args(e, B, R, f);
    launch_fork_prompt(f, st);
    e->cached_B = R;
    HIPCHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The call frame of the two non-beam drivers (generate_attempt, lookup_attempt): what both do around their decode loops, once.  A driver
// runs budget(), enter(), its own setup, start(), its loop over poll(), then report() and finish(); the rows it decodes, its step, the key of
// its kept graph and when it polls are its own.
// ------------------------------------------------------------------------------------------------
struct GenFrame {
    sv_engine* const e;
    const GenCall& c;
    const sv_sampling* const sp;
    const char* const who;            // the name cb_guard and the bad-logits report carry: "sv_generate" (plain) or c.who (lookup)
    const int B;                      // rows of the prompt pass's layout, of the outputs and of the streaming callback: c.B * c.n_samples
    const SelMode sel;
    int max_new = 0;
    hipStream_t st = nullptr;
    std::unique_lock<std::mutex> lock;
    GenClock::time_point t0, t1;
    // streaming: the columns below `streamed` have been handed to sp->on_tokens -- by this attempt or, for an optimistic call's second attempt, by
    // its first (e->stream_skip comes in through enter() and is written back on every way out; generate_retry resets it)
    int streamed = 0;
    std::vector<int32_t> stream_buf;

    GenFrame(sv_engine* e_, const GenCall& c_, const char* who_) : e(e_), c(c_), sp(c_.sp), who(who_), B(c_.B * c_.n_samples), sel(sel_mode(e_, *c_.sp)) {}
    ~GenFrame() { if (lock.owns_lock()) e->stream_skip = streamed; }
    const int32_t* block() const { return e->h_flags + HF_BLOCK; }      // the last poll()'s {step, done, n_emitted, bad}
    bool done() const { return e->h_flags[HF_DONE] != 0; }

    // the budget checks (no engine state is touched); stop_ids_now: the null check of stop_ids is made here, not by start() behind the prompt pass
    int budget(bool stop_ids_now) {
        max_new = sp->max_length - c.S0;     // HF: with inputs_embeds, max_length includes the prompt
        if (max_new <= 0) return fail(SV_EINVAL, "max_length (%d) must exceed the prompt length (%d)", sp->max_length, c.S0);
        if (c.S0 + max_new > e->cfg.max_seq_len) return fail(SV_EINVAL, "max_length %d exceeds engine max_seq_len %d", sp->max_length, e->cfg.max_seq_len);
        if (sp->n_stop < 0 || sp->n_stop > 16) return fail(SV_EINVAL, "stop sequence length %d unsupported (0..16)", sp->n_stop);
        if (stop_ids_now && sp->n_stop > 0 && !sp->stop_ids) return fail(SV_EINVAL, "n_stop > 0 but stop_ids is null");
        if (sp->do_sample && !(sp->temperature > 0.f && sp->top_p > 0.f)) return fail(SV_EINVAL, "temperature and top_p must be > 0");
        return 0;
    }
    // the engine's lock for the rest of the call; the engine stream ordered after everything already queued on the caller's
    int enter() {
        lock = std::unique_lock<std::mutex>(e->mu);
        streamed = e->stream_skip;
        HIPCHECK(hipSetDevice(e->cfg.device));
        HIPCHECK(hipEventRecord(e->gen_event, (hipStream_t)c.stream));
        st = e->gen_stream;
        HIPCHECK(hipStreamWaitEvent(st, e->gen_event, 0));
        return cb_guard(e, who);
    }
    // one copy of the device's {step, done, n_emitted, bad} block -- with lk_state's four words in the same synchronise when a lookup call asks
    int poll(const int32_t* lk_state = nullptr) {
        HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_BLOCK], e->d_step, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (lk_state) HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_LOOKUP], lk_state, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        e->h_flags[HF_DONE] = block()[BLK_DONE];
        return 0;
    }
    // The prompt pass, the generation state and the first token (from the prompt pass's logits, by the plain step's own launches), then ONE copy
    // of the device block: a call that is over after its first token (budget 1, EOS) has everything it needs from this round trip and takes no
    // other before the tokens go out.  n_amax: the key slots of a folded greedy selection to clear (0: none).
    int start(int n_amax) {
        const int32_t Bp = c.B, G = c.n_samples, S0 = c.S0;
        const int32_t* lens = c.lens;
        t0 = GenClock::now();
        HIPCHECK(hipMemsetAsync(e->d_bad, 0, sizeof(int32_t), st));         // a flag left by an earlier, failed call is not this call's
        if (G > 1) {                             // one prompt pass over the Bp prompts, then the fork launch: B rows from here on
            SVCHECK(shared_prefill_fork(e, c.embeds, Bp, G, S0, lens, max_new, st));
        } else if (lens) {                       // pages per sequence for lens[b] + max_new, one ragged prompt pass
            SVCHECK(assign_pages_ragged(e, B, lens, max_new, st));
            SVCHECK(prefill_forward_ragged(e, (const bf16_t*)c.embeds, B, lens, st));
            if (!c.lookup) e->cached_B = B;      // (a lookup call aliases the table below: it says so itself, there)
            HIPCHECK(hipGetLastError());
        } else {
            SVCHECK(prefill_locked(e, c.embeds, B, S0, S0 + max_new, st, false));
        }
        // generation state, one launch: positions = S0 - 1 (finish_step adds 1), unfinished = 1, {step, done, n_emitted} = 0, the folded selection's key slots = 0
        gen_state_init(e->positions, S0 - 1, e->unfinished, B, e->d_step, e->amax, n_amax, st);
        if (lens) ragged_positions(e, Bp, G, -1, st);        // every row continues at its own prompt's length
        if (sel.pen) HIPCHECK(hipMemsetAsync(e->seen, 0, (size_t)((B + 31) / 32) * 32 * e->seen_words * sizeof(uint32_t), st));
        if (sp->n_stop > 0) {
            if (!sp->stop_ids) return fail(SV_EINVAL, "n_stop > 0 but stop_ids is null");
            HIPCHECK(hipMemcpyAsync(e->d_stop, sp->stop_ids, sp->n_stop * sizeof(int32_t), hipMemcpyHostToDevice, st));
        }
        sample_and_finish(e, B, *sp, max_new, st);
        SVCHECK(poll());
        t1 = GenClock::now();
        return 0;
    }
    // streaming: hand the callback the columns [streamed, n_cols_final) of all B rows
    int stream_upto(int n_cols_final) {
        if (!sp->on_tokens || n_cols_final <= streamed) return 0;
        const int n = n_cols_final - streamed;
        stream_buf.resize((size_t)B * n);
        HIPCHECK(hipMemcpy2DAsync(stream_buf.data(), (size_t)n * sizeof(int32_t), e->out_tok + streamed,
                                  (size_t)e->out_ld * sizeof(int32_t), (size_t)n * sizeof(int32_t), B, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        sp->on_tokens(sp->user_data, stream_buf.data(), B, streamed, n);
        streamed = n_cols_final;
        return 0;
    }
    // the verdict on the block the last poll() read: a give-up or a non-finite row voids the call (before the last columns go out: a void call
    // streams nothing more)
    int report() {
        e->h_flags[HF_NEMIT] = block()[BLK_NEMIT];
        return report_bad_logits(e, st, who, block()[BLK_BAD]);
    }
    // the rest of the columns to the callback, the tokens to the caller, the timing
    int finish(double steps, double per_launch) {
        const int n_emit = e->h_flags[HF_NEMIT];
        if (n_emit < 1 || n_emit > max_new) return fail(SV_EHIP, "generation bookkeeping failed (n_emitted=%d)", n_emit);
        SVCHECK(stream_upto(n_emit));
        tokens_to_i64(e->out_tok, e->out_ld, c.dev_out_tokens, B, n_emit, max_new, st);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(st));
        set_timing(e, t0, t1, steps, per_launch);
        *c.n_generated = n_emit;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// sv_generate_lookup: greedy generate that verifies K drafted tokens per sequence and step (lookup/lookup.hip; DESIGN.md "Prompt-lookup decoding")
// ------------------------------------------------------------------------------------------------
static void lookup_args(sv_engine* e, int n_seq, const sv_lookup& lk, const sv_sampling& sp, int max_new, LookupArgs& a) {
    const int mb = e->cfg.max_batch;
    memset(&a, 0, sizeof(a));
    a.counts = e->lk_state; a.n_emit = a.counts + 3; a.fin = a.n_emit + mb; a.base = a.fin + mb; a.n_draft = a.base + mb;
    a.limit = a.n_draft + mb; a.ticket = reinterpret_cast<unsigned*>(a.limit + 1);
    a.n_seq = n_seq; a.K = lk.num_draft_tokens; a.max_ngram = lk.max_ngram; a.min_ngram = lk.min_ngram;
    a.cur_tok = e->cur_tok; a.positions = e->positions; a.unfinished = e->unfinished;
    a.out_tok = e->out_tok; a.ld_out = e->out_ld; a.pval = e->am_val; a.pidx = e->am_idx;
    a.done = e->d_done; a.n_emitted = e->d_nemit; a.bad = e->d_bad;
    a.stop_ids = e->d_stop; a.n_stop = sp.n_stop; a.eos = sp.eos_token_id; a.pad = sp.pad_token_id; a.max_new = max_new; a.V = e->cfg.vocab;
    if (e->lk_forced && e->lk_forced_B == n_seq) { a.forced = e->lk_forced; a.forced_ld = e->lk_forced_ld; }
}
// The driver beside generate_attempt (same GenCall, same retry): prompt pass and first token exactly as the plain call takes them, then
// verification steps -- decode_forward over B x (K + 1) rows with the K / V pre-write in front of every attention launch, the min-length
// hold, the slice argmax, lookup_step_kernel -- captured once and replayed.
// sv_generate_lookup_sampled comes through here with the selection switch: do_sample replaces the slice argmax by lookup_sample_kernel (the
// plain sampler's code with the plain call's (seed, column, sequence) triple, handed over as slice winners), a repetition penalty gives every
// ROW its own bitmap in e->seen (lookup_seen_kernel behind lookup_step_kernel) and both selections read it by row.  The sampler's stream does
// not depend on the attempt: the rerun after an ownership fall-back returns the same tokens.
static int lookup_attempt(sv_engine* e, const GenCall& c) {
    const sv_sampling* sp = c.sp;
    const sv_lookup& lk = *c.lookup;
    const int32_t B = c.B, K1 = lk.num_draft_tokens + 1;
    const int32_t* lens = c.lens;
    SVCHECK(check_ready(e));
    if ((long long)B * K1 > e->cfg.max_batch || B > 64)
        return fail(SV_ENOTSUP, "%s: B %d x (num_draft_tokens %d + 1) rows exceed engine max_batch %d", c.who, B, K1 - 1, e->cfg.max_batch);
    const int rows = B * K1;
    if (lens) SVCHECK(ragged_check_lens(e, lens, B, c.who, nullptr, nullptr));
    GenFrame f(e, c, c.who);
    SVCHECK(f.budget(true));
    // sv_generate_lookup_sampled: the selection the call asks for (sv_generate_lookup refuses both in front of this driver)
    const bool sample = sp->do_sample != 0, pen = f.sel.pen;
    const int max_new = f.max_new;
    if (pen && (size_t)e->seen_words * sizeof(uint32_t) > 65536)
        return fail(SV_ENOTSUP, "%s: repetition_penalty with a vocabulary of %d ids is not built (a sequence's bitmap must fit 64 KB of LDS)", c.who, e->cfg.vocab);
    SVCHECK(f.enter());
    hipStream_t st = f.st;
    if (!e->lk_state) SVCHECK(dalloc(e, &e->lk_state, (size_t)4 * e->cfg.max_batch + 8));
    if (pen && !e->lk_seen) {
        SVCHECK(dalloc(e, &e->lk_seen, (size_t)64 * e->seen_words));
        SVCHECK(dalloc(e, &e->lk_seen_cols, (size_t)64));
    }
    SVCHECK(f.start(0));
    int32_t* const lkh = e->h_flags + HF_LOOKUP;      // {steps, drafted, accepted, n_emit[0]} as the last poll read them
    lkh[0] = lkh[1] = lkh[2] = 0; lkh[3] = 1;

    struct LookupOff { sv_engine* e; ~LookupOff() { e->lookup_on = false; } } lookup_off{e};
    int steps = 0;
    hipGraphExec_t gexec = nullptr;
    if (!f.done()) {
        // rows s * K1 + j of the block table = sequence s's row: the K1 rows of a sequence alias the same pages, tail page included (descending:
        // a row is read before it is overwritten)
        if (e->table_pending) { HIPCHECK(hipEventSynchronize(e->table_ev)); e->table_pending = false; }
        const size_t mp = (size_t)e->pages_per_seq;
        for (int r = rows - 1; r > 0; --r)
            if (r / K1 != r) memcpy(e->h_table + (size_t)r * mp, e->h_table + (size_t)(r / K1) * mp, mp * sizeof(int32_t));
        HIPCHECK(hipMemcpyAsync(e->block_table, e->h_table, (size_t)rows * mp * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHECK(hipEventRecord(e->table_ev, st));
        e->table_pending = true;
        e->cached_B = 0;                         // the cache is in no layout sv_decode_step could continue
        LookupArgs la;
        lookup_args(e, B, lk, *sp, max_new, la);
        // the penalty's seen sets: row b of the B-row layout holds what the first token's bookkeeping left; they go to the per-sequence buffer
        // BEFORE any row of the B x K1 layout is written (rows b and s * K1 overlap), then every row gets its sequence's set plus its drafts
        if (pen) HIPCHECK(hipMemcpyAsync(e->lk_seen, e->seen, (size_t)B * e->seen_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        launch_lookup_begin(la, st);
        LookupSeenArgs ls;
        ls.seq_seen = e->lk_seen; ls.seq_cols = e->lk_seen_cols; ls.row_seen = e->seen; ls.words = e->seen_words; ls.n_seq = B; ls.K1 = K1; ls.begin = 1;
        ls.n_emit = la.n_emit; ls.n_draft = la.n_draft; ls.cur_tok = la.cur_tok; ls.out_tok = la.out_tok; ls.ld_out = la.ld_out; ls.done = la.done;
        if (pen) launch_lookup_seen(ls, st);
        ls.begin = 0;
        e->lookup_on = true;
        const int min_new = f.sel.min_new;
        const uint32_t* seen = f.sel.seen;
        const float penalty = pen ? sp->repetition_penalty : 1.f;
        LookupSampleArgs sa;
        sa.logits = e->logits; sa.ld = e->Vpad; sa.V = e->cfg.vocab; sa.rows = rows; sa.K1 = K1; sa.n_emit = la.n_emit; sa.done = la.done;
        sa.temperature = sp->temperature; sa.top_p = sp->top_p; sa.top_k = sp->top_k; sa.seed = sp->seed;
        sa.seen = seen; sa.seen_words = e->seen_words; sa.penalty = penalty; sa.pval = e->am_val; sa.pidx = e->am_idx;
        const auto one_step = [&]() {
            decode_forward(e, rows, st);
            if (min_new > 0) launch_lookup_hold_eos(e->logits, e->Vpad, sp->eos_token_id, la.n_emit, K1, min_new, rows, st);
            if (sample) launch_lookup_sample(sa, st);
            else launch_argmax_partial(e->logits, e->Vpad, e->cfg.vocab, e->am_val, e->am_idx, rows, seen, e->seen_words, penalty, st);
            launch_lookup_step(la, st);
            if (pen) launch_lookup_seen(ls, st);
        };
        if (graph_enabled()) {
            char key[480];
            int kn = snprintf(key, sizeof(key), "B%d|K%d|ng%d.%d|n%d|eos%d|pad%d|ns%d|mn%d|x%d|fo%d|f%p.%d", B, K1 - 1, lk.max_ngram, lk.min_ngram, max_new,
                              sp->eos_token_id, sp->pad_token_id, sp->n_stop, sp->min_new_tokens, e->exp, e->fused_off ? 1 : 0, (const void*)la.forced, la.forced_ld);
            // the selection of sv_generate_lookup_sampled is part of the captured step (the seed travels by value in the sampler's arguments)
            if (sample) kn += snprintf(key + kn, sizeof(key) - kn, "|s.T%a.k%d.p%a.sd%llu", (double)sp->temperature, sp->top_k, (double)sp->top_p, (unsigned long long)sp->seed);
            if (pen) snprintf(key + kn, sizeof(key) - kn, "|r%a", (double)sp->repetition_penalty);
            SVCHECK(e->lk_step.use(key, st, 1, one_step));       // a slot of its own: the plain call's kept graphs stay
            gexec = e->lk_step.x;
        }
        // The end is data-dependent (a step emits 1 .. K + 1 tokens per sequence), so the device block is polled after EVERY chunk.  Chunk length
        // 8 unless sync_every says otherwise: the steps a chunk runs past the end of the call are wasted (they find *done set and change
        // nothing) -- at most 7 of ~1 ms, where the plain loop's 32 would waste up to 31 -- while a poll idles the GPU for ~0.1 ms, ~1 % of 8 steps.
        // Never more steps than the budget has tokens left: every step emits at least one token per live sequence.
        const int chunk = sp->sync_every > 0 ? sp->sync_every : 8;
        while (!f.done()) {
            int n = max_new - 1 - steps;
            if (n <= 0) break;
            if (n > chunk) n = chunk;
            for (int i = 0; i < n; ++i) {
                if (gexec) HIPCHECK(hipGraphLaunch(gexec, st));
                else one_step();
            }
            steps += n;
            SVCHECK(f.poll(e->lk_state));
            if (f.block()[BLK_BAD]) break;
            if (!f.done() && B == 1) SVCHECK(f.stream_upto(lkh[3]));      // (B == 1: the columns below n_emit[0] are final)
        }
    }
    SVCHECK(f.report());
    if (!f.done()) return fail(SV_EHIP, "%s: the call did not end within its budget (%d steps)", c.who, steps);
    SVCHECK(f.finish((double)lkh[0], gexec ? 1.0 : 0.0));         // (timing[2]: the device's count of steps)
    if (c.counts3) { c.counts3[0] = lkh[0]; c.counts3[1] = lkh[1]; c.counts3[2] = lkh[2]; }
    return 0;
}
// sampled = false: sv_generate_lookup (greedy, no penalty); true: sv_generate_lookup_sampled (the selection of the call's sv_sampling)
static int lookup_call(const char* who, bool sampled, sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0,
                       const sv_sampling* sp, const sv_lookup* lookup, int64_t* dev_out_tokens, int32_t* n_generated, int32_t* host_counts3, sv_stream stream) {
    if (!lookup || lookup->num_draft_tokens == 0) {
        if (host_counts3) host_counts3[0] = host_counts3[1] = host_counts3[2] = 0;
        if (host_lens) return sv_generate_ragged(e, dev_embeds_packed, B, host_lens, sp, nullptr, dev_out_tokens, n_generated, stream);
        return sv_generate(e, dev_embeds_packed, B, S0, sp, dev_out_tokens, n_generated, stream);
    }
    sv_lookup lk = *lookup;
    if (lk.num_draft_tokens < 0 || lk.num_draft_tokens > SV_LOOKUP_MAX_DRAFT)
        return fail(SV_EINVAL, "%s: num_draft_tokens %d unsupported (0..%d)", who, lk.num_draft_tokens, SV_LOOKUP_MAX_DRAFT);
    if (lk.max_ngram < 0 || lk.max_ngram > SV_LOOKUP_MAX_NGRAM)
        return fail(SV_EINVAL, "%s: max_ngram %d unsupported (1..%d, 0 = 3)", who, lk.max_ngram, SV_LOOKUP_MAX_NGRAM);
    if (lk.max_ngram == 0) lk.max_ngram = 3;
    if (lk.min_ngram < 0 || lk.min_ngram > lk.max_ngram)
        return fail(SV_EINVAL, "%s: min_ngram %d must lie in 1..max_ngram %d (0 = 1)", who, lk.min_ngram, lk.max_ngram);
    if (lk.min_ngram == 0) lk.min_ngram = 1;
    GenCall c{who, GC_ARGS, dev_embeds_packed, B, S0, host_lens, 1, sp, nullptr, nullptr, nullptr, nullptr, dev_out_tokens, n_generated, stream};
    SVCHECK(check_gen_call(c));
    if (e && e->kv_dtype != SV_KV_BF16) return fail(SV_ENOTSUP, "%s: prompt-lookup drafting is not built for the fp8_e4m3 KV cache (the drafts' K / V pre-write is bf16)", who);
    if (sp->do_sample && !sampled) return fail(SV_ENOTSUP, "%s: do_sample is not built (verification is greedy: the drafts are compared with the arg-max)", who);
    if (sp->num_beams > 1) return fail(SV_ENOTSUP, "%s: num_beams %d is not built (beam rows reorder their caches)", who, sp->num_beams);
    if (!sampled && sp->repetition_penalty > 0.f && sp->repetition_penalty != 1.0f)
        return fail(SV_ENOTSUP, "%s: repetition_penalty %g is not built (a draft row's penalty depends on the drafts in front of it)", who, sp->repetition_penalty);
    if (sp->on_tokens && B > 1) return fail(SV_ENOTSUP, "%s: streaming (on_tokens) with B %d > 1 is not built (the sequences advance at different rates)", who, B);
    c.lookup = &lk;
    c.counts3 = host_counts3;
    return generate_retry(e, c);
}
extern "C" int sv_generate_lookup(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0, const sv_sampling* sp,
                                  const sv_lookup* lookup, int64_t* dev_out_tokens, int32_t* n_generated, int32_t* host_counts3, sv_stream stream) {
    return lookup_call("sv_generate_lookup", false, e, dev_embeds_packed, B, host_lens, S0, sp, lookup, dev_out_tokens, n_generated, host_counts3, stream);
}
// The same call with the selection its sv_sampling asks for: do_sample with temperature / top_k / top_p / seed, any repetition_penalty.  Row j of
// sequence s draws with (seed, n_emit_s + j, s) -- the plain call's triple at that column -- over the plain call's logits bits, against the
// plain call's seen set once the drafts in front of it are accepted: the tokens are sv_generate's / sv_generate_ragged's, bit for bit.
extern "C" int sv_generate_lookup_sampled(sv_engine* e, const void* dev_embeds_packed, int32_t B, const int32_t* host_lens, int32_t S0,
                                          const sv_sampling* sp, const sv_lookup* lookup, int64_t* dev_out_tokens, int32_t* n_generated,
                                          int32_t* host_counts3, sv_stream stream) {
    return lookup_call("sv_generate_lookup_sampled", true, e, dev_embeds_packed, B, host_lens, S0, sp, lookup, dev_out_tokens, n_generated, host_counts3,
                       stream);
}

// lens != nullptr: the ragged form -- S0 is the longest prompt (the budget counts from it), sequence b has lens[b] rows
static int generate_attempt(sv_engine* e, const GenCall& c) {
    if (c.lookup) return lookup_attempt(e, c);
    const int32_t Bp = c.B, G = c.n_samples;
    const int32_t* lens = c.lens;
    const sv_sampling* sp = c.sp;
    SVCHECK(check_ready(e));
    const bool shared = G > 1;
    if (shared && (Bp < 1 || (long long)Bp * G > e->cfg.max_batch))
        return fail(SV_EINVAL, "sv_generate_shared: B %d x n_samples %d exceeds engine max_batch %d", Bp, G, e->cfg.max_batch);
    const int B = Bp * G;        // decode rows: row b * G + j is sample j of prompt b (the row order of repeat_interleave)
    if (lens) {
        if (Bp > e->cfg.max_batch) return fail(SV_EINVAL, "sv_generate_ragged: bad B=%d (max_batch %d)", Bp, e->cfg.max_batch);
        SVCHECK(ragged_check_lens(e, lens, Bp, shared ? "sv_generate_shared" : "sv_generate_ragged", nullptr, nullptr));
    }
    if (!sp || !c.dev_out_tokens || !c.n_generated) return fail(SV_EINVAL, "sv_generate: null argument");
    GenFrame f(e, c, "sv_generate");
    SVCHECK(f.budget(false));
    const int max_new = f.max_new;
    if (sp->num_beams < 0) return fail(SV_EINVAL, "num_beams must be >= 1");
    if (sp->num_beams > 1 && shared)
        return fail(SV_ENOTSUP, "sv_generate_shared: n_samples %d with num_beams %d is not built (several returned sequences under beam search)", G, sp->num_beams);
    SVCHECK(f.enter());
    hipStream_t st = f.st;
    struct ProcOff { sv_engine* e; ~ProcOff() { e->ban_ngram = 0; e->ban_nwords = 0; e->minp_log = -INFINITY; } } proc_off{e};
    SVCHECK(setup_processors(e, sp, c.lp, st));
    const bool ban = e->ban_ngram > 0 || e->ban_nwords > 0;
    struct CapOff { sv_engine* e; ~CapOff() { e->cap_on = false; } } cap_off{e};
    SVCHECK(setup_capture(e, sp, c.outs, sp->num_beams > 1 ? B * sp->num_beams : B, max_new, st));
    struct StatsOff { sv_engine* e; ~StatsOff() { e->ts_on = false; } } stats_off{e};
    SVCHECK(setup_token_stats(e, sp, c.stats, B, max_new, st));
    struct TopkOff { sv_engine* e; ~TopkOff() { e->tk_on = false; } } topk_off{e};
    SVCHECK(setup_token_topk(e, sp, c.topk, B, max_new, st));
    if (sp->num_beams > 1) {
        if (sp->on_tokens) return fail(SV_EINVAL, "streaming is not supported with beam search (hypotheses are only final at the end; HF refuses too)");
        if (sp->n_stop > 0 && !sp->stop_ids) return fail(SV_EINVAL, "n_stop > 0 but stop_ids is null");
        return generate_beam(e, c.embeds, B, c.S0, lens, sp, max_new, c.outs, c.dev_out_tokens, c.n_generated, st);
    }

    // Plain greedy decode (no repetition penalty, no min_length hold, one row tile, bf16 lm_head with the K split over the waves of a
    // block): the selection rides in the lm_head epilogue of every decode step -- one launch less per step, same tokens bit for bit.
    // SV_EXP_SEPARATE_ARGMAX = the separate argmax launch (A/B).
    bool fused_sel = false;
    {
        int waves = 1, two = 0;
        skinny_plan(e->lm_head.Npad, e->lm_head.Kpad, 1, e->lm_head.wfmt, (B + 31) / 32, &waves, &two);
        // a capturing call (sv_generate_ex) takes the separate selection launch: the capture must read the logits row between the lm_head and
        // the selection, and the tokens are bit-identical either way (tests/test_gpu_e2e.py)
        // (a ban rewrites the logits row between the lm_head and the selection: the separate launch as well)
        fused_sel = !sp->do_sample && !f.sel.pen && sp->min_new_tokens <= 0 && B <= 32 && e->lm_head.wfmt == SV_WFMT_BF16 && waves > 1 && !two && !(e->exp & SV_EXP_SEPARATE_ARGMAX) &&
                    !e->cap_on && !ban && !e->ts_on && !e->tk_on;      // (the statistics / top-k launches read the row and the slice winners between the lm_head and the bookkeeping)
    }
    SVCHECK(f.start(fused_sel ? 64 * SV_AMAX_STRIDE : 0));
    struct FusedSel { sv_engine* e; ~FusedSel() { e->greedy_fused = false; e->fin_fold = false; e->fin_folded = false; } } fused_guard{e};
    if (fused_sel) {
        e->greedy_fused = true;                      // read by decode_forward (capture and eager launches below); cleared on every exit
        const char* ff = getenv("SV_FINISH_FOLD");   // 0 = the bookkeeping as its own launch (A/B)
        e->fin_fold = !(ff && atoi(ff) == 0);
        e->fin_args = make_finish_args(e, B, *sp, max_new, true);
    }

    int steps = 0;
    const int chunk = sp->sync_every > 0 ? sp->sync_every : 32;
    hipGraphExec_t gexec = nullptr;
    const auto one_step = [&]() { decode_forward(e, B, st); sample_and_finish(e, B, *sp, max_new, st, fused_sel); };
    if (!f.done() && graph_enabled()) {
        // One decode step is captured as a hipGraph (all kernel arguments are stable device pointers; the step index,
        // positions and stop state live in device memory) and replayed every step.  The instantiated graph is KEPT on the
        // engine and reused by the next call whose batch, budget and sampling parameters are the same (a serving request
        // stream, the benchmark), so a short request does not pay a 172-node capture + instantiate; a call with other
        // parameters replaces it.  Owned by the engine: no early return below can leak it.
        char key[384];
        snprintf(key, sizeof(key), "B%d|n%d|ds%d|T%a|p%a|k%d|seed%llu|eos%d|pad%d|ns%d|rp%a|mn%d|x%d|fo%d|ff%d", B, max_new, sp->do_sample,
                 sp->temperature, sp->top_p, sp->top_k, (unsigned long long)sp->seed, sp->eos_token_id, sp->pad_token_id, sp->n_stop,
                 sp->repetition_penalty, sp->min_new_tokens, e->exp, e->fused_off ? 1 : 0, e->fin_fold ? 1 : 0);
        if (e->cap_on)       // capturing steps carry more launches (never the same graph as a plain call's); the slabs are read through cap_desc
            snprintf(key + strlen(key), sizeof(key) - strlen(key), "|cap%d", (e->cap_host.scores ? 1 : 0) | (e->cap_host.logits ? 2 : 0));
        if (ban || e->minp_log > -INFINITY)      // the ban launch / the sampler's min_p argument (the bad-word ids live in device memory, not in the graph);
            snprintf(key + strlen(key), sizeof(key) - strlen(key), "|ng%d|bw%d|mp%a", e->ban_ngram, e->ban_nwords, e->minp_log);      // neither: the plain call's key and graph
        if (e->ts_on)        // a statistics step carries one or two launches more; the buffers (and which of them are asked for) are read through ts_desc
            snprintf(key + strlen(key), sizeof(key) - strlen(key), "|ts");
        if (e->tk_on)        // the top-k launch: k, the source and whether the rank is taken are launch arguments; the buffers are read through tk_desc
            snprintf(key + strlen(key), sizeof(key) - strlen(key), "|tk%d.%d.%d", e->tk_k, e->tk_source, e->tk_rank ? 1 : 0);
        const bool kept = e->gen_step.holds(key);
        if (!kept) e->gen_multi.drop();          // the multi-step graph is the same step: it goes with the one it copies
        SVCHECK(e->gen_step.use(key, st, 1, one_step));
        gexec = e->gen_step.x;                   // (nullptr: plain launches of the SAME kernels)
        if (gexec && !kept) {
            size_t nn = 0;                       // sv_debug_step_plan: the step's launches, counted on the freshly captured graph itself
            e->step_nodes = 0;
            if (hipGraphGetNodes(e->gen_step.g, nullptr, &nn) == hipSuccess && nn > 0) {
                std::vector<hipGraphNode_t> nodes(nn);
                if (hipGraphGetNodes(e->gen_step.g, nodes.data(), &nn) == hipSuccess)
                    for (size_t i = 0; i < nn; ++i) {
                        hipGraphNodeType ty;
                        if (hipGraphNodeGetType(nodes[i], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel) ++e->step_nodes;
                    }
            }
        }
    }
    // Several steps per graph launch.  Inside a replayed graph a kernel follows its predecessor with no measurable gap; from one hipGraphLaunch to
    // the next the GPU idles 8.6 us (rocprofv3 kernel trace of the bench: finish_step_kernel of step i -> the first kernel of step i + 1,
    // profiles/step_gaps_r06.log) -- 0.9 % of StarVector-1B's step.  So the SAME step is captured U times into a second graph (every kernel argument
    // is a stable device pointer and the step index lives on the device: U copies of the node list ARE U consecutive steps) and a chunk of the loop
    // below launches it while at least U steps of the chunk are left, the one-step graph for the rest.  U = the polling chunk (sync_every, at most
    // SV_GRAPH_STEPS = 32 by default; 1 = off): nothing runs that did not run before -- the loop already issues a whole chunk before it looks at the
    // done flag.  Built only for calls with at least 4 U steps in front of them (instantiating 32 x 99 nodes costs milliseconds), kept on the
    // engine with the one-step graph (same key).
    hipGraphExec_t gexec_multi = nullptr;
    int U = 0;
    if (gexec) {
        U = chunk < graph_steps_cap() ? chunk : graph_steps_cap();
        if (U >= 2 && max_new - 1 >= 4 * U) {
            // (not required: on a failure the one-step graph carries the call, whatever SV_REQUIRE_GRAPH says)
            (void)e->gen_multi.use(std::to_string(U), st, U, one_step, false);
            gexec_multi = e->gen_multi.x;
        }
    }
    // The host looks at the device's done flag after every chunk -- a round trip that leaves the GPU idle for ~0.1 ms -- only when something can
    // END the call before its budget (an EOS id inside the vocabulary, a stop sequence) or wants the columns as they become final (streaming).
    // A fixed-length call (the benchmark's EOS-disabled workload, fixed-length rollouts) has nothing to poll for.
    const bool poll = (sp->eos_token_id >= 0 && sp->eos_token_id < e->cfg.vocab) || sp->n_stop > 0 || sp->on_tokens != nullptr;
    while (!f.done()) {
        int n = max_new - 1 - steps;
        if (n <= 0) break;                       // budget exhausted: the device flag is already set
        if (n > chunk) n = chunk;
        for (int i = 0; i < n;) {
            if (gexec_multi && n - i >= U) {
                HIPCHECK(hipGraphLaunch(gexec_multi, st));
                i += U;
            } else if (gexec) {
                HIPCHECK(hipGraphLaunch(gexec, st));
                ++i;
            } else {
                one_step();
                ++i;
            }
        }
        steps += n;
        if (!poll) continue;                     // nothing can end this call before its budget: the next chunk follows without a host round trip
        SVCHECK(f.poll());
        if (f.block()[BLK_BAD]) break;           // a void step (give-up, non-finite row): nothing of this chunk is handed on; the error is raised below
        if (!f.done()) SVCHECK(f.stream_upto(steps + 1));      // still running: columns [0, steps] are final (a finished batch may have fewer: n_emitted caps it)
    }
    if (steps > 0) SVCHECK(f.poll());            // (a call that ended at its first token has the block already)
    SVCHECK(f.report());
    return f.finish((double)steps, gexec_multi ? (double)U : gexec ? 1.0 : 0.0);       // steps per graph launch
}

// ------------------------------------------------------------------------------------------------
// C ABI: the beam scorer on its own (parity tests drive it with synthetic logits)
// ------------------------------------------------------------------------------------------------
struct sv_beam { BeamScorer s; int device = 0; CaptureDesc* cap_desc = nullptr; };

extern "C" int sv_beam_create(const sv_beam_config* cfg, sv_beam** out) {
    if (!cfg || !out) return fail(SV_EINVAL, "sv_beam_create: null argument");
    if (cfg->batch < 1 || cfg->num_beams < 1 || cfg->num_beams > BM_MAXNB || cfg->vocab < 2 * cfg->num_beams || cfg->max_new < 1)
        return fail(SV_EINVAL, "sv_beam_create: bad shape (batch %d, num_beams %d, vocab %d, max_new %d)", cfg->batch,
                    cfg->num_beams, cfg->vocab, cfg->max_new);
    if (cfg->batch > 1024) return fail(SV_EINVAL, "sv_beam_create: batch > 1024");
    if (cfg->n_stop < 0 || cfg->n_stop > BM_MAXSTOP || (cfg->n_stop > 0 && !cfg->stop_ids)) return fail(SV_EINVAL, "sv_beam_create: bad stop sequence");
    if (cfg->early_stopping < 0 || cfg->early_stopping > 2) return fail(SV_EINVAL, "sv_beam_create: early_stopping must be 0, 1 or 2");
    BeamConfig bc;
    bc.B = cfg->batch; bc.nb = cfg->num_beams; bc.V = cfg->vocab; bc.max_new = cfg->max_new; bc.eos = cfg->eos_token_id;
    bc.pad = cfg->pad_token_id; bc.early = cfg->early_stopping; bc.length_penalty = cfg->length_penalty;
    bc.penalty = cfg->repetition_penalty > 0.f ? cfg->repetition_penalty : 1.f; bc.n_stop = cfg->n_stop;
    for (int i = 0; i < cfg->n_stop; ++i) bc.stop[i] = cfg->stop_ids[i];
    if (cfg->do_sample && !(cfg->temperature > 0.f && cfg->top_p > 0.f)) return fail(SV_EINVAL, "sv_beam_create: temperature and top_p must be > 0");
    bc.do_sample = cfg->do_sample ? 1 : 0; bc.temperature = cfg->do_sample ? cfg->temperature : 1.f;
    bc.top_p = cfg->do_sample ? cfg->top_p : 1.f; bc.top_k = cfg->top_k; bc.seed = cfg->seed;
    bc.min_new = cfg->min_new_tokens > 0 ? cfg->min_new_tokens : 0;
    sv_beam* h = new sv_beam();
    int r = h->s.init(bc, nullptr, nullptr, nullptr, nullptr);
    if (!r) r = h->s.reset(nullptr);
    if (r) { h->s.destroy(); delete h; return fail(SV_EHIP, "sv_beam_create: hip error %d", r); }
    *out = h;
    return 0;
}
extern "C" int sv_beam_destroy(sv_beam* h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    h->s.destroy();
    if (h->cap_desc) (void)hipFree(h->cap_desc);
    delete h;
    return 0;
}
// test surface (include/starvector_hip_debug.h): the sv_beam_step calls that follow also launch beam_capture_kernel into the caller's slabs,
// through the BeamScorer::cap / cap_temp the engine sets for sv_generate_ex
extern "C" int sv_debug_beam_set_capture(sv_beam* h, float* dev_scores, float* dev_logits, int64_t ld, int32_t max_new) {
    if (!h) return fail(SV_EINVAL, "sv_debug_beam_set_capture: null scorer");
    if (!dev_scores && !dev_logits) { h->s.cap = nullptr; h->s.cap_temp = 1.f; return 0; }
    if (ld < h->s.c.V) return fail(SV_EINVAL, "sv_debug_beam_set_capture: ld %lld < vocab %d", (long long)ld, h->s.c.V);
    if (max_new < 1 || max_new > h->s.c.max_new)
        return fail(SV_EINVAL, "sv_debug_beam_set_capture: max_new %d outside 1..%d (the scorer's)", max_new, h->s.c.max_new);
    if (!h->cap_desc) HIPCHECK(hipMalloc(reinterpret_cast<void**>(&h->cap_desc), sizeof(CaptureDesc)));
    CaptureDesc hd;
    hd.scores = dev_scores; hd.logits = dev_logits; hd.ld = ld; hd.rows = h->s.R; hd.max_new = max_new;
    HIPCHECK(hipMemcpy(h->cap_desc, &hd, sizeof(hd), hipMemcpyHostToDevice));
    h->s.cap = h->cap_desc;
    h->s.cap_temp = h->s.c.temperature;
    return 0;
}
extern "C" int sv_beam_step(sv_beam* h, const float* dev_logits, int32_t ld, int32_t* done, int32_t* host_parent,
                            int32_t* host_tokens, float* host_scores, sv_stream stream) {
    if (!h || !dev_logits || !done) return fail(SV_EINVAL, "sv_beam_step: null argument");
    if (ld < h->s.c.V) return fail(SV_EINVAL, "sv_beam_step: ld %d < vocab %d", ld, h->s.c.V);
    hipStream_t st = (hipStream_t)stream;
    h->s.enqueue_step(dev_logits, ld, 1, st);
    HIPCHECK(hipGetLastError());
    const size_t R = (size_t)h->s.R;
    HIPCHECK(hipMemcpyAsync(done, h->s.d.done, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_parent) HIPCHECK(hipMemcpyAsync(host_parent, h->s.d.parent, R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_tokens) HIPCHECK(hipMemcpyAsync(host_tokens, h->s.d.cur_tok, R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_scores) HIPCHECK(hipMemcpyAsync(host_scores, h->s.d.run_score, R * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}
// the (parent beam, token) columns of the last beam-search sv_generate: [n_steps][batch * num_beams] each
extern "C" int sv_beam_history(sv_engine* e, int32_t* host_parent, int32_t* host_tok, int32_t capacity_steps,
                               int32_t* n_steps, int32_t* rows) {
    if (!e || !n_steps || !rows) return fail(SV_EINVAL, "sv_beam_history: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->beam.R <= 0) return fail(SV_ESTATE, "sv_beam_history: no beam search has run on this engine");
    HIPCHECK(hipSetDevice(e->cfg.device));
    int32_t n = 0;
    HIPCHECK(hipMemcpy(&n, e->beam.d.step, sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_steps = n;
    *rows = e->beam.R;
    if (!host_parent || !host_tok) return 0;
    if (n > capacity_steps) return fail(SV_EINVAL, "sv_beam_history: %d steps recorded, capacity %d", n, capacity_steps);
    HIPCHECK(hipMemcpy(host_parent, e->beam.d.hist_parent, (size_t)n * e->beam.R * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(host_tok, e->beam.d.hist_tok, (size_t)n * e->beam.R * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int sv_beam_finalize(sv_beam* h, int64_t* host_tokens, int32_t* n_generated, float* host_scores, sv_stream stream) {
    if (!h || !host_tokens || !n_generated) return fail(SV_EINVAL, "sv_beam_finalize: null argument");
    std::vector<int64_t> toks;
    std::vector<float> sc;
    int L = 0;
    int r = h->s.finalize((hipStream_t)stream, toks, L, sc);
    if (r) return fail(SV_EHIP, "sv_beam_finalize: bookkeeping failed (code %d)", r);
    memcpy(host_tokens, toks.data(), toks.size() * sizeof(int64_t));
    if (host_scores) memcpy(host_scores, sc.data(), sc.size() * sizeof(float));
    *n_generated = L;
    return 0;
}
