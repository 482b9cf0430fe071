// Host driver, part 4 of 5: continuous batching (sv_cb_*): requests are rows ("slots") of one decode loop.
#include <algorithm>
#include <cmath>
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------------
// C ABI: continuous batching.  The reference's worker admits up to 5 concurrent requests
// (serve/model_worker.py:161-172,216-229) and runs each as its own HF generate; here they share ONE decode loop: every
// row ("slot") of the batch is a request with its own sampling parameters, budget, EOS and stop sequence, requests join
// (prefill into free slots while the others keep their KV pages) and leave at any step, and the captured decode step is kept
// per row bucket.  A request produces the same tokens as when it runs alone through sv_generate.
// sv_cb_set_lookup (at the end of this file) makes the batch draft: a slot then owns cb_K + 1 decode rows and the step's selection is
// cb_lookup_step_kernel (cb_lookup/cb_lookup.hip) -- the tokens of every request stay what they are.
// ------------------------------------------------------------------------------------------------
// Drafting (sv_cb_set_lookup): a slot owns K1 = cb_K + 1 decode rows, the batch holds max_batch / K1 slots, the bucket is counted in ROWS
static inline int cb_k1(const sv_engine* e) { return e->cb_K + 1; }
static inline int cb_slot_cap(const sv_engine* e) { return e->cfg.max_batch / cb_k1(e); }
static int cb_bucket(const sv_engine* e) {
    int hi = 0;
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2) if (e->cb_used[s2]) hi = s2 + 1;
    hi *= cb_k1(e);
    int b = 8;
    while (b < hi) b <<= 1;
    return b > e->cfg.max_batch ? e->cfg.max_batch : b;
}

// record: some slot of the launch records log-probs (the recording kernel; the descriptors decide per slot)
static void cb_step_args(sv_engine* e, CbStepArgs& a, const int32_t* map, bool record) {
    a.logits = e->logits; a.ld = e->Vpad; a.V = e->cfg.vocab; a.slots = e->cb_slots; a.slot_map = map;
    a.cur_tok = e->cur_tok; a.positions = e->positions; a.out_tokens = e->out_tok; a.ld_out = e->out_ld;
    a.seen = e->seen; a.seen_words = e->seen_words; a.n_live = e->cb_nlive; a.events = e->cb_events; a.bad = e->d_bad;
    a.counts = e->cb_counts; a.ld_counts = e->Vpad; a.bias = e->cb_bias;
    a.lp = record ? e->cb_lp : nullptr;
}
// the drafting batch's selection: first = the first token of new requests (block b = slot map[b] on logits row b), else a verification step
static void cb_lookup_args(sv_engine* e, CbLookupArgs& q, const int32_t* map, bool record, bool first) {
    const int mb = e->cfg.max_batch;
    cb_step_args(e, q.st, map, record);
    q.K = e->cb_K; q.max_ngram = e->cb_max_ngram; q.min_ngram = e->cb_min_ngram; q.first = first ? 1 : 0;
    q.n_draft = e->cb_lk_state; q.counts = q.n_draft + mb; q.totals = q.counts + 3 * mb;
    q.forced = e->cb_lk_forced_n > 0 ? e->cb_lk_forced : nullptr; q.forced_n = e->cb_lk_forced_n; q.forced_ld = e->cb_lk_forced_ld;
}

// ---- per-slot log-prob records (sv_cb_admit_logprobs / sv_cb_read_logprobs) ----
// a slot in use that records: the step of such a batch is the recording kernel, under a graph key of its own (a finished slot that has not been
// released yet still counts: the host learns of the finish at the next poll)
static bool cb_any_records(const sv_engine* e) {
    if (!e->cb_lp) return false;
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2) if (e->cb_used[s2] && e->cb_lp_host[s2].enable) return true;
    return false;
}
// first use: the descriptors and the four buffers; slot s2 owns columns [s2 * out_ld, (s2 + 1) * out_ld) of each
static int cb_lp_alloc(sv_engine* e) {
    if (e->cb_lp) return 0;
    const size_t mb = (size_t)e->cfg.max_batch, cols = mb * (size_t)e->out_ld;
    float *lp = nullptr, *lps = nullptr;
    int32_t *rank = nullptr, *ids = nullptr;
    CbLogprobs* d = nullptr;
    SVCHECK(dalloc(e, &lp, cols, false));
    SVCHECK(dalloc(e, &rank, cols, false));
    SVCHECK(dalloc(e, &ids, cols * SV_TOPK_MAX, false));
    SVCHECK(dalloc(e, &lps, cols * SV_TOPK_MAX, false));
    SVCHECK(dalloc(e, &d, mb));
    e->cb_lp_host.assign(mb, CbLogprobs{});
    for (size_t s2 = 0; s2 < mb; ++s2) {
        CbLogprobs& h = e->cb_lp_host[s2];
        h.logprob = lp + s2 * e->out_ld; h.rank = rank + s2 * e->out_ld;
        h.ids = ids + s2 * e->out_ld * SV_TOPK_MAX; h.lps = lps + s2 * e->out_ld * SV_TOPK_MAX;
    }
    e->cb_lp = d;
    return 0;
}
// the descriptor of slot s2 <- what request i asks (lp == nullptr: nothing); the host image is a member, so the copy may stay in flight
static int cb_lp_set(sv_engine* e, int s2, const sv_cb_logprobs* lp, hipStream_t st) {
    if (!e->cb_lp) return 0;
    CbLogprobs& h = e->cb_lp_host[s2];
    const bool on = lp && lp->enable;
    if (!on && !h.enable) return 0;                          // off on both sides already
    h.enable = on ? 1 : 0; h.k = on ? lp->k : 0; h.source = on ? lp->source : 0;
    HIPCHECK(hipMemcpyAsync(e->cb_lp + s2, &h, sizeof(CbLogprobs), hipMemcpyHostToDevice, st));
    return 0;
}

namespace sveng {
int cb_check_request(const sv_cb_request& r, int V, int i, const char* who) {
    if (r.semantics != 0 && r.semantics != 1) return fail(SV_EINVAL, "%s: request %d: semantics %d (0 = HF, 1 = vLLM)", who, i, r.semantics);
    if (r.n_stop < 0 || r.n_stop > SV_CB_MAXSTOP) return fail(SV_EINVAL, "%s: request %d: stop sequence length %d unsupported (0..%d)", who, i, r.n_stop, SV_CB_MAXSTOP);
    if (r.do_sample && !(r.temperature > 0.f && r.top_p > 0.f)) return fail(SV_EINVAL, "%s: request %d: temperature and top_p must be > 0", who, i);
    if (r.semantics == 0) {
        // the vLLM fields act in vLLM mode only: a caller that set one under HF semantics would lose it silently
        const char* set = r.presence_penalty != 0.f ? "presence_penalty" : r.frequency_penalty != 0.f ? "frequency_penalty"
                        : r.min_p != 0.f ? "min_p" : (r.n_prompt_ids || r.prompt_ids) ? "prompt_ids"
                        : (r.n_logit_bias || r.logit_bias_ids || r.logit_bias_values) ? "logit_bias" : r.n_stop_any ? "stop_any_ids" : nullptr;
        if (set) return fail(SV_EINVAL, "%s: request %d: %s is a vLLM-semantics field (set semantics = 1)", who, i, set);
        return 0;
    }
    if (!std::isfinite(r.presence_penalty) || !std::isfinite(r.frequency_penalty))
        return fail(SV_EINVAL, "%s: request %d: presence / frequency penalty must be finite", who, i);
    if (!(r.min_p >= 0.f && r.min_p <= 1.f)) return fail(SV_EINVAL, "%s: request %d: min_p %g outside [0, 1]", who, i, (double)r.min_p);
    if (!(r.repetition_penalty >= 0.f) || !std::isfinite(r.repetition_penalty))
        return fail(SV_EINVAL, "%s: request %d: repetition_penalty must be > 0 (0 = off)", who, i);
    if (r.eos_token_id >= V) return fail(SV_EINVAL, "%s: request %d: eos_token_id %d outside the vocabulary (%d; negative = none)", who, i, r.eos_token_id, V);
    if (r.max_new_tokens > 65535) return fail(SV_EINVAL, "%s: request %d: max_new_tokens %d: vLLM mode counts tokens in 16 bits (< 65536)", who, i, r.max_new_tokens);
    if (r.n_prompt_ids < 0 || (r.n_prompt_ids > 0 && !r.prompt_ids)) return fail(SV_EINVAL, "%s: request %d: bad prompt_ids", who, i);
    for (int k = 0; k < r.n_prompt_ids; ++k)
        if (r.prompt_ids[k] < 0 || r.prompt_ids[k] >= V) return fail(SV_EINVAL, "%s: request %d: prompt id %d outside the vocabulary (%d)", who, i, r.prompt_ids[k], V);
    if (r.n_logit_bias < 0 || r.n_logit_bias > SV_CB_MAXBIAS) return fail(SV_EINVAL, "%s: request %d: %d logit_bias entries (0..%d)", who, i, r.n_logit_bias, SV_CB_MAXBIAS);
    if (r.n_logit_bias > 0 && (!r.logit_bias_ids || !r.logit_bias_values)) return fail(SV_EINVAL, "%s: request %d: null logit_bias arrays", who, i);
    for (int k = 0; k < r.n_logit_bias; ++k) {
        const int id = r.logit_bias_ids[k];
        if (id < 0 || id >= V) return fail(SV_EINVAL, "%s: request %d: logit_bias id %d outside the vocabulary (%d)", who, i, id, V);
        if (std::isnan(r.logit_bias_values[k])) return fail(SV_EINVAL, "%s: request %d: logit_bias value of id %d is NaN", who, i, id);
        for (int j = 0; j < k; ++j)
            if (r.logit_bias_ids[j] == id) return fail(SV_EINVAL, "%s: request %d: logit_bias id %d given twice", who, i, id);
    }
    if (r.n_stop_any < 0 || r.n_stop_any > SV_CB_MAXANY) return fail(SV_EINVAL, "%s: request %d: %d stop_any_ids (0..%d)", who, i, r.n_stop_any, SV_CB_MAXANY);
    for (int k = 0; k < r.n_stop_any; ++k)
        if (r.stop_any_ids[k] < 0 || r.stop_any_ids[k] >= V) return fail(SV_EINVAL, "%s: request %d: stop id %d outside the vocabulary (%d)", who, i, r.stop_any_ids[k], V);
    return 0;
}

int cb_check_logprobs(const sv_cb_request* reqs, const sv_cb_logprobs* lps, int n, const char* who) {
    for (int i = 0; lps && i < n; ++i) {
        const sv_cb_logprobs& l = lps[i];
        if (!l.enable) continue;
        if (l.k < 0 || l.k > SV_TOPK_MAX) return fail(SV_EINVAL, "%s: request %d: logprobs k=%d must be in 0..%d", who, i, l.k, SV_TOPK_MAX);
        if (l.source != 0 && l.source != 1)
            return fail(SV_EINVAL, "%s: request %d: logprobs source=%d must be 0 (log_softmax(raw / T)) or 1 (the processed row)", who, i, l.source);
        if (reqs[i].semantics == 1 && l.source == 0)
            return fail(SV_EINVAL, "%s: request %d: logprobs source 0 on a vLLM-semantics request (its processors rewrite the raw row in place: use source 1)",
                        who, i);
    }
    return 0;
}

void cb_fill_slot(const sv_cb_request& r, CbSlot& h, CbBias& bias, std::vector<uint32_t>& seen_row, int seen_words) {
    memset(&h, 0, sizeof(h));
    memset(&bias, 0, sizeof(bias));
    h.live = 1; h.step = 0; h.budget = r.max_new_tokens; h.do_sample = r.do_sample ? 1 : 0; h.temperature = r.temperature;
    h.top_p = r.top_p; h.top_k = r.top_k; h.eos = r.eos_token_id; h.pad = r.pad_token_id; h.min_new = r.min_new_tokens;
    h.penalty = r.repetition_penalty > 0.f ? r.repetition_penalty : 1.0f; h.n_stop = r.n_stop; h.seed = r.seed;
    for (int k = 0; k < r.n_stop; ++k) h.stop[k] = r.stop_ids[k];
    seen_row.assign(seen_words, 0u);
    if (r.semantics != 1) return;
    h.vllm = 1; h.presence = r.presence_penalty; h.frequency = r.frequency_penalty; h.min_p = r.min_p;
    h.n_bias = r.n_logit_bias; h.n_any = r.n_stop_any;
    for (int k = 0; k < r.n_stop_any; ++k) h.any[k] = r.stop_any_ids[k];
    for (int k = 0; k < r.n_logit_bias; ++k) {
        bias.id[k] = r.logit_bias_ids[k];
        bias.val[k] = std::min(100.f, std::max(-100.f, r.logit_bias_values[k]));      // the OpenAI server's clamp
    }
    for (int k = 0; k < r.n_prompt_ids; ++k) seen_row[r.prompt_ids[k] >> 5] |= 1u << (r.prompt_ids[k] & 31);
}
}  // namespace sveng

// ------------------------------------------------------------------------------------------------
// The prefix cache (sv_cb_set_prefix_cache; keys and digests: prefix_cache/prefix_cache.hip).  Host bookkeeping over the page pool:
//   * pc_table maps the chained key of a full prompt page to the page that holds its K / V.  A registered page's page_refs entry is its exact
//     holder count (a private page, 0 elsewhere, becomes 1 when it is registered; cb_release_locked treats both alike).
//   * a registered page whose last holder lets go joins the back of pc_lru instead of the free list; an admit that is short of free pages evicts
//     from the front.  Pages with a holder are never evicted.
//   * nothing here touches the device: a cached page is read by later prompt passes and never written (kv_write_extend_kernel starts at ctx).
// ------------------------------------------------------------------------------------------------
static void pc_lru_remove(sv_engine* e, int pg) {
    if (!e->pc_in_lru[pg]) return;
    e->pc_lru.erase(e->pc_lru_it[pg]);
    e->pc_in_lru[pg] = 0;
}
static void pc_lru_push(sv_engine* e, int pg) {
    e->pc_lru.push_back(pg);
    e->pc_lru_it[pg] = std::prev(e->pc_lru.end());
    e->pc_in_lru[pg] = 1;
}
static void pc_unregister(sv_engine* e, int pg) {
    e->pc_table.erase(e->pc_key_of[pg]);
    e->pc_reg[pg] = 0;
}
void sveng::pc_drop(sv_engine* e) {
    // (pages nobody holds are free again; held ones simply stop being findable and go to the free list when their slots release them)
    for (int pg : e->pc_lru) { e->pc_in_lru[pg] = 0; e->free_pages.push_back(pg); }
    e->pc_lru.clear();
    e->pc_table.clear();
    std::fill(e->pc_reg.begin(), e->pc_reg.end(), 0);
}

// What the cache decides for the U prompts of an admit, before any page moves: the keys of every full page and the pages found in the table as
// it stood before the call.
struct PcAdmit {
    std::vector<std::vector<PcKey>> keys;            // [U][len / 64]
    std::vector<std::vector<int>> pages;             // [U][h]: the reused pages
    std::vector<int> holders;                        // a page once per holder this admit added (a failed admit takes them back)
    bool any_hit = false;
    int h(int u) const { return (int)pages[u].size(); }
};

// the digest launch over the admit's prompts, the copy to the host (the admit is synchronous anyway), the chains and the walk
static int pc_lookup(sv_engine* e, const void* dev_embeds, int U, int S0_all, const int32_t* lens, PcAdmit& pc, hipStream_t st) {
    const int mp = e->pages_per_seq;
    pc.keys.assign(U, {}); pc.pages.assign(U, {});
    int most = 0;
    std::vector<int32_t> desc;
    for (int u = 0, r0 = 0; u < U; ++u) {
        const int len = lens ? lens[u] : S0_all;
        most = std::max(most, len / SV_PAGE_TOKENS);
        desc.push_back(r0); desc.push_back(len);
        r0 += len;
    }
    if (most == 0) return 0;      // no prompt has a full page
    if (lens) HIPCHECK(hipMemcpyAsync(e->pc_desc, desc.data(), desc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    SVCHECK(pc_launch_digests((const bf16_t*)dev_embeds, U, lens ? e->pc_desc : nullptr, S0_all, e->cfg.hidden, mp, e->pc_dig, st));
    std::vector<uint64_t> dig((size_t)U * mp * 2);
    HIPCHECK(hipMemcpyAsync(dig.data(), e->pc_dig, dig.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int u = 0; u < U; ++u) {
        const int len = lens ? lens[u] : S0_all;
        PcKey key = pc_key0();
        int matched = 0;
        std::vector<int> found;
        for (int k = 0; k < len / SV_PAGE_TOKENS; ++k) {
            const uint64_t* d = dig.data() + 2 * ((size_t)u * mp + k);
            key = pc_chain(key, PcKey{d[0], d[1]});
            pc.keys[u].push_back(key);
            if (matched != k) continue;
            const auto it = e->pc_table.find(key);
            if (it != e->pc_table.end()) { ++matched; found.push_back(it->second); }
        }
        found.resize((size_t)pc_hit_pages(matched, len));
        pc.pages[u] = std::move(found);
        pc.any_hit = pc.any_hit || !pc.pages[u].empty();
    }
    return 0;
}

// Room for an admit that takes `need` pages from the free list and reuses pc's pages: SV_EBUSY -- nothing has moved -- when the free pages and the
// evictable ones (cached, no holder, not reused by this admit) are short; otherwise the reused pages leave the LRU list and the oldest others are
// evicted until the free list holds `need`.  pc == nullptr (the cache is off): the free list alone decides, as ever.
static bool pc_make_room(sv_engine* e, size_t need, const PcAdmit* pc) {
    if (!pc) return need <= e->free_pages.size();
    size_t keep = 0;
    std::vector<char> seen((size_t)e->num_pages + 1, 0);
    for (const std::vector<int>& v : pc->pages)
        for (int pg : v) if (e->pc_in_lru[pg] && !seen[pg]) { seen[pg] = 1; ++keep; }
    if (e->free_pages.size() + (e->pc_lru.size() - keep) < need) return false;
    for (const std::vector<int>& v : pc->pages) for (int pg : v) pc_lru_remove(e, pg);
    while (e->free_pages.size() < need) {
        const int pg = e->pc_lru.front();
        pc_lru_remove(e, pg);
        pc_unregister(e, pg);
        e->free_pages.push_back(pg);
        ++e->pc_evictions;
    }
    return true;
}

// after a successful prompt pass: every full prompt page, computed or reused, under its key -- a key already present keeps its page
static void pc_register(sv_engine* e, const PcAdmit& pc, const std::vector<int32_t>& pf) {
    const int mp = e->pages_per_seq;
    for (size_t u = 0; u < pc.keys.size(); ++u) {
        e->pc_lookups += (long long)pc.keys[u].size();
        e->pc_reused += pc.h((int)u);
        for (size_t k = 0; k < pc.keys[u].size(); ++k) {
            const int pg = pf[u * mp + k];
            if (!e->pc_table.emplace(pc.keys[u][k], pg).second) continue;
            e->pc_key_of[pg] = pc.keys[u][k];
            e->pc_reg[pg] = 1;
            if (e->page_refs[pg] == 0) e->page_refs[pg] = 1;      // a private page: its one slot is its holder
        }
    }
}

static int cb_begin(sv_engine* e, hipStream_t st) {
    if (e->cb_active) return 0;
    reset_free_pages(e);
    e->pc_table.clear(); e->pc_lru.clear();
    e->pc_key_of.assign((size_t)e->num_pages + 1, PcKey{0, 0});
    e->pc_reg.assign((size_t)e->num_pages + 1, 0);
    e->pc_in_lru.assign((size_t)e->num_pages + 1, 0);
    e->pc_lru_it.assign((size_t)e->num_pages + 1, e->pc_lru.end());
    e->pc_lookups = e->pc_reused = e->pc_evictions = 0;
    std::fill(e->cb_used.begin(), e->cb_used.end(), 0);
    for (auto& v : e->cb_pages) v.clear();
    e->page_refs.assign((size_t)e->num_pages + 1, 0);
    const size_t R = (size_t)e->MT * 32;
    std::vector<int32_t> table((size_t)e->cfg.max_batch * e->pages_per_seq, e->trash_page);
    HIPCHECK(hipMemcpyAsync(e->block_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(e->cb_slots, 0, R * sizeof(CbSlot), st));
    HIPCHECK(hipMemsetAsync(e->positions, 0, R * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(e->cur_tok, 0, R * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(e->cb_nlive, 0, sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(e->cb_events, 0, sizeof(int32_t), st));
    if (e->cb_K) HIPCHECK(hipMemsetAsync(e->cb_lk_state, 0, ((size_t)4 * e->cfg.max_batch + 3) * sizeof(int32_t), st));      // no drafts in flight, the totals from zero
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2) SVCHECK(cb_lp_set(e, s2, nullptr, st));      // (every slot is free: nobody records)
    HIPCHECK(hipStreamSynchronize(st));                  // `table` is a host temporary
    e->cb_active = true;
    e->cached_B = 0;
    return 0;
}

// What an admit stages on the host for its n requests before anything goes to the device.  The two plans below fill the page side -- they take
// pages from the free list in different orders, which block_table_row and free_pages show --, cb_admit_impl the rest.
struct AdmitPlan {
    std::vector<int> slots;                          // request i -> its slot (lowest free first: keeps the row bucket of the decode graph small)
    std::vector<int32_t> rows;                       // [n][pages_per_seq]: the block-table rows of the slots
    std::vector<int32_t> pf;                         // the prompt pass's table, one row per prompt
    std::vector<int> taken;                          // the pages in the order they left the free list (a failed admit puts them back in reverse)
    std::vector<int32_t> map, pos;                   // slot and last prompt position of request i
    std::vector<int32_t> fork;                       // the fork launch's descriptor (group admit); empty: no fork launch
    std::vector<CbSlot> hs;
    std::vector<CbBias> hb;
    std::vector<std::vector<uint32_t>> seen_rows;
    bool record = false;                             // some request records log-probs
    PcAdmit* pc = nullptr;                           // the prefix cache's decisions for the prompts (nullptr: the cache is off)
    // page k of prompt u comes from the cache: it gets one more holder
    int reuse(sv_engine* e, int u, int k) { const int pg = pc->pages[u][k]; ++e->page_refs[pg]; pc->holders.push_back(pg); return pg; }
    int take(sv_engine* e) { const int pg = e->free_pages.back(); e->free_pages.pop_back(); taken.push_back(pg); return pg; }
};

// sv_cb_admit / sv_cb_admit_ragged: every request owns the pages of its whole budget, taken request by request (lens == nullptr: all prompts S0_all rows)
static int plan_plain(sv_engine* e, int n, int S0_all, const int32_t* lens, const sv_cb_request* reqs, AdmitPlan& p) {
    const int mp = e->pages_per_seq;
    auto need_of = [&](int i) { return ((lens ? lens[i] : S0_all) + reqs[i].max_new_tokens + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS; };
    const auto hit_of = [&](int i) { return p.pc ? p.pc->h(i) : 0; };      // leading pages the cache supplies
    size_t need_pages = 0;
    for (int i = 0; i < n; ++i) need_pages += (size_t)(need_of(i) - hit_of(i));
    if ((int)p.slots.size() < n || !pc_make_room(e, need_pages, p.pc))
        return fail(SV_EBUSY, "sv_cb_admit: %d requests need %d slots / %zu KV pages, %zu / %zu are free (release finished slots first)",
                    n, n, need_pages, p.slots.size(), e->free_pages.size() + e->pc_lru.size());
    for (int i = 0; i < n; ++i) {
        p.pos[i] = (lens ? lens[i] : S0_all) - 1;
        std::vector<int>& held = e->cb_pages[p.slots[i]];
        held.clear();
        for (int k = 0; k < need_of(i); ++k) held.push_back(p.rows[(size_t)i * mp + k] = k < hit_of(i) ? p.reuse(e, i, k) : p.take(e));
    }
    p.pf = p.rows;      // prompt i is written through the pages of request i
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Group admit (sv_cb_admit_shared): n requests over n_prompts prompts, request i samples prompt group[i].  One ragged prompt pass over the
// PROMPTS, the fork launch into the n slots (fork.hip), the first-token step.  Page plan as sv_generate_shared's: the slots of a prompt share its
// full pages (held once, reference-counted in page_refs), every slot owns its pages from the prompt's tail page on.  Shared pages are never written
// after the prompt pass: a decode step writes at its slot's own position, i.e. into a private page.
// ------------------------------------------------------------------------------------------------
namespace sveng {
// Prompts are numbered in the order their first request appears: group[0] = 0, group[i] <= max(group[0..i)) + 1, every prompt used -- so that
// group[i] <= i, which the in-place fan-out of the logits rows needs (fork.hip).
int shared_check_group(const char* who, const int32_t* lens, int n_prompts, const int32_t* group, int n) {
    if (!lens || !group) return fail(SV_EINVAL, "%s: null host_lens / host_group", who);
    if (n_prompts < 1 || n < 1 || n_prompts > n) return fail(SV_EINVAL, "%s: bad n_prompts=%d / n=%d (1 <= n_prompts <= n)", who, n_prompts, n);
    for (int u = 0; u < n_prompts; ++u)
        if (lens[u] < 1) return fail(SV_EINVAL, "%s: prompt %d: bad prompt length %d", who, u, lens[u]);
    int hi = -1;
    for (int i = 0; i < n; ++i) {
        if (group[i] < 0 || group[i] >= n_prompts) return fail(SV_EINVAL, "%s: group[%d] = %d outside [0, n_prompts = %d)", who, i, group[i], n_prompts);
        if (group[i] > hi + 1)
            return fail(SV_EINVAL, "%s: group[%d] = %d: prompts are numbered in the order their first request appears (prompt %d has none before it)", who, i,
                        group[i], hi + 1);
        hi = group[i] > hi ? group[i] : hi;
    }
    if (hi + 1 != n_prompts) return fail(SV_EINVAL, "%s: prompt %d is referenced by no request", who, hi + 1);
    return 0;
}
// pages of request i: the first shared[i] entries of its block-table row are its prompt's (held once per prompt), private_[i] are its own;
// returns what the admit takes from the free list: sum over prompts of len / 64 + sum over requests of ceil((len + budget) / 64) - len / 64
long long shared_page_plan(const int32_t* lens, int n_prompts, const int32_t* group, const int32_t* budgets, int n, int32_t* shared, int32_t* private_) {
    long long total = 0;
    for (int u = 0; u < n_prompts; ++u) total += lens[u] / SV_PAGE_TOKENS;
    for (int i = 0; i < n; ++i) {
        const int len = lens[group[i]], sh = len / SV_PAGE_TOKENS;
        const int pv = (len + budgets[i] + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS - sh;
        if (shared) shared[i] = sh;
        if (private_) private_[i] = pv;
        total += pv;
    }
    return total;
}
}  // namespace sveng

// sv_cb_admit_shared / sv_cb_admit_logprobs: every prompt's shared pages first (held once, counted in page_refs), then each request's private ones
static int plan_group(sv_engine* e, int U, const int32_t* lens, int n, const int32_t* group, const sv_cb_request* reqs, AdmitPlan& p) {
    const int mp = e->pages_per_seq, mb = e->cfg.max_batch;
    std::vector<int32_t> budgets(n), n_sh(n), n_pv(n);
    for (int i = 0; i < n; ++i) budgets[i] = reqs[i].max_new_tokens;
    size_t need_pages = (size_t)shared_page_plan(lens, U, group, budgets.data(), n, n_sh.data(), n_pv.data());
    for (int u = 0; p.pc && u < U; ++u) need_pages -= (size_t)p.pc->h(u);      // the leading pages the cache supplies
    if ((int)p.slots.size() < n || !pc_make_room(e, need_pages, p.pc))
        return fail(SV_EBUSY, "sv_cb_admit_shared: %d requests over %d prompts need %d slots / %zu KV pages, %zu / %zu are free (release finished slots first)",
                    n, U, n, need_pages, p.slots.size(), e->free_pages.size() + e->pc_lru.size());
    p.pf.assign((size_t)U * mp, e->trash_page);
    p.fork.assign(6 * (size_t)mb, 0);
    std::vector<std::vector<int>> prompt_pages(U);
    std::vector<int> owner(U, -1), n_dst(U, 0);
    for (int u = 0; u < U; ++u)
        for (int k = 0; k < lens[u] / SV_PAGE_TOKENS; ++k) prompt_pages[u].push_back(p.pc && k < p.pc->h(u) ? p.pc->pages[u][k] : p.take(e));
    for (int i = 0; i < n; ++i) {
        const int u = group[i];
        std::vector<int>& held = e->cb_pages[p.slots[i]];
        held.clear();
        for (int k = 0; k < n_sh[i]; ++k) {
            held.push_back(p.rows[(size_t)i * mp + k] = prompt_pages[u][k]);
            ++e->page_refs[prompt_pages[u][k]];
            if (p.pc && k < p.pc->h(u)) p.pc->holders.push_back(prompt_pages[u][k]);
        }
        for (int k = 0; k < n_pv[i]; ++k) held.push_back(p.rows[(size_t)i * mp + n_sh[i] + k] = p.take(e));
        if (owner[u] < 0) owner[u] = i;          // the prompt pass writes prompt u through the pages of its first request
        else ++n_dst[u];
        p.pos[i] = lens[u] - 1;
        p.fork[5 * (size_t)mb + i] = u;          // logits row of the prompt (u <= i: shared_check_group)
    }
    const int K1 = cb_k1(e);             // the fork launch indexes block-table ROWS: a slot's first (its K1 rows are copies of one another)
    for (int u = 0, d0 = 0; u < U; ++u) {
        const int o = owner[u];
        for (int k = 0; k < (lens[u] + SV_PAGE_TOKENS - 1) / SV_PAGE_TOKENS; ++k) p.pf[(size_t)u * mp + k] = p.rows[(size_t)o * mp + k];
        p.fork[4 * u] = p.slots[o] * K1; p.fork[4 * u + 1] = lens[u]; p.fork[4 * u + 2] = d0; p.fork[4 * u + 3] = n_dst[u];
        for (int i = 0; i < n; ++i) if (group[i] == u && i != o) p.fork[4 * (size_t)mb + d0++] = p.slots[i] * K1;
    }
    return 0;
}

// The prompt pass of an admit in which the cache supplies the first h_u pages of some prompts: prompt u runs as an extension with ctx = 64 h_u,
// len = L_u - 64 h_u, total = L_u (h_u = 0: as a sequence without a context, the bits of the one-shot pass) through cb_table_pf.  The own rows are
// no longer contiguous in the caller's buffer: they are compacted into pc_ws, one copy per prompt.  The chunk budget, if set, counts own rows.
static int pc_prompt_pass(sv_engine* e, const bf16_t* embeds, int U, int S0_all, const int32_t* lens, const PcAdmit& pc, hipStream_t st) {
    const size_t D = (size_t)e->cfg.hidden;
    std::vector<int32_t> L((size_t)U), ctx((size_t)U);
    size_t own = 0;
    for (int u = 0; u < U; ++u) { L[u] = lens ? lens[u] : S0_all; ctx[u] = SV_PAGE_TOKENS * pc.h(u); own += (size_t)(L[u] - ctx[u]); }
    if (own > e->pc_ws_rows) {
        if (e->pc_ws) (void)hipFree(e->pc_ws);      // (waits for the launches that still read it)
        e->pc_ws = nullptr; e->pc_ws_rows = 0;
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&e->pc_ws), own * D * sizeof(bf16_t)));
        e->pc_ws_rows = own;
    }
    for (size_t u = 0, src = 0, dst = 0; u < (size_t)U; src += L[u], dst += L[u] - ctx[u], ++u)
        HIPCHECK(hipMemcpyAsync(e->pc_ws + dst * D, embeds + (src + ctx[u]) * D, (size_t)(L[u] - ctx[u]) * D * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
    e->ctx_known = false;
    return prefill_chunked(e, e->pc_ws, U, L.data(), e->cb_table_pf, st, ctx.data());
}

// The device side of an admit: the slots' state, ONE prompt pass over the U new prompts (their pages through cb_table_pf; rectangular when
// lens == nullptr), the fork launch when the plan has a descriptor (tail pages to the other slots of each prompt, logits row i <- row group[i]) and
// the first-token step; the live slots keep decoding afterwards.  Any failure rolls the host bookkeeping back (slots, pages) and parks the slots'
// device state, so a failed admit leaks nothing and the caller may simply retry: the slots it was told about are NOT in use on error.
static int cb_admit_commit(sv_engine* e, const void* dev_embeds, int U, int S0_all, const int32_t* lens, const sv_cb_request* reqs,
                           const sv_cb_logprobs* lps, const AdmitPlan& p, int32_t* slots_out, hipStream_t st) {
    const int n = (int)p.slots.size(), mp = e->pages_per_seq;
    const bool any_pen = [&] { for (int i = 0; i < n; ++i) if (reqs[i].repetition_penalty > 0.f && reqs[i].repetition_penalty != 1.0f) return true; return false; }();
    bool nlive_added = false;
    const int K1 = cb_k1(e);
    const int rc = [&]() -> int {
    for (int i = 0; i < n; ++i) {
        const int s2 = p.slots[i];
        // drafting: the slot's K1 block-table rows are copies of one another; its rows of cur_tok / positions are written by the first-token launch
        // from the prompt length kept in the slot (CbSlot::base)
        for (int j = 0; j < K1; ++j)
            HIPCHECK(hipMemcpyAsync(e->block_table + ((size_t)s2 * K1 + j) * mp, p.rows.data() + (size_t)i * mp, mp * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(e->cb_slots + s2, &p.hs[i], sizeof(CbSlot), hipMemcpyHostToDevice, st));
        if (!e->cb_K) HIPCHECK(hipMemcpyAsync(e->positions + s2, &p.pos[i], sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (reqs[i].semantics == 1) {
            // vLLM mode: the repetition set starts as the prompt ids, the output counts at zero -- before the first-token step below
            HIPCHECK(hipMemcpyAsync(e->seen + (size_t)s2 * e->seen_words, p.seen_rows[i].data(), e->seen_words * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemsetAsync(e->cb_counts + (size_t)s2 * e->Vpad, 0, (size_t)e->Vpad * sizeof(uint16_t), st));
            if (p.hs[i].n_bias) HIPCHECK(hipMemcpyAsync(e->cb_bias + s2, &p.hb[i], sizeof(CbBias), hipMemcpyHostToDevice, st));
        } else if (any_pen) {
            HIPCHECK(hipMemsetAsync(e->seen + (size_t)s2 * e->seen_words, 0, e->seen_words * sizeof(uint32_t), st));
        }
        if (p.record) SVCHECK(cb_lp_set(e, s2, lps + i, st));
    }
    HIPCHECK(hipMemcpyAsync(e->cb_table_pf, p.pf.data(), p.pf.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(e->cb_map, p.map.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!p.fork.empty()) HIPCHECK(hipMemcpyAsync(e->fork_desc, p.fork.data(), p.fork.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    add_i32(e->cb_nlive, n, 1, st);
    nlive_added = true;
    if (p.pc && p.pc->any_hit) SVCHECK(pc_prompt_pass(e, (const bf16_t*)dev_embeds, U, S0_all, lens, *p.pc, st));
    else if (lens) SVCHECK(prefill_forward_ragged(e, (const bf16_t*)dev_embeds, U, lens, st, e->cb_table_pf));
    else SVCHECK(prefill_forward(e, (const bf16_t*)dev_embeds, U, S0_all, st, 0, nullptr, e->cb_table_pf));
    if (!p.fork.empty()) {
        ForkArgs f;
        fork_args(e, U, n, f);
        launch_fork_prompt(f, st);
    }
    // first token of every new request, from its prompt's logits (column 0 of its record)
    if (e->cb_K) {
        CbLookupArgs q;                                    // the plain kernel would write cur_tok[slot] / positions[slot]: another slot's rows in this layout
        cb_lookup_args(e, q, e->cb_map, p.record, true);
        launch_cb_lookup_step(q, n, st);
    } else {
        CbStepArgs a;
        cb_step_args(e, a, e->cb_map, p.record);
        launch_cb_step(a, n, st);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));                    // the plan's vectors are host temporaries
    return 0;
    }();
    if (!rc) {
        if (p.pc) pc_register(e, *p.pc, p.pf);
        return 0;
    }
    const std::string why = g_err;                          // keep the first error's text
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    std::vector<int32_t> trash(mp, e->trash_page);
    for (int i = n - 1; i >= 0; --i) {
        const int s2 = p.slots[i];
        e->cb_pages[s2].clear();
        e->cb_used[s2] = 0;
        slots_out[i] = -1;
        // best effort on the device: the slot is dead, records nothing and its block-table row points at the trash page again
        (void)hipMemsetAsync(e->cb_slots + s2, 0, sizeof(CbSlot), st);
        for (int j = 0; j < K1; ++j)
            (void)hipMemcpyAsync(e->block_table + ((size_t)s2 * K1 + j) * mp, trash.data(), trash.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
        (void)cb_lp_set(e, s2, nullptr, st);
    }
    for (size_t k = p.taken.size(); k-- > 0;) {             // pages go back in reverse order, no holder left: the free list is as it was
        e->page_refs[p.taken[k]] = 0;
        e->free_pages.push_back(p.taken[k]);
    }
    for (size_t k = 0; p.pc && k < p.pc->holders.size(); ++k) {      // the reused pages lose the holders this admit added
        const int pg = p.pc->holders[k];
        if (--e->page_refs[pg] == 0 && e->pc_reg[pg]) pc_lru_push(e, pg);
    }
    if (nlive_added) add_i32(e->cb_nlive, -n, 1, st);
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    g_err = why;
    return rc;
}

// group == nullptr: n requests, one prompt each (U == n; lens == nullptr: the common length S0_all and the rectangular prompt pass); otherwise the
// group admit: request i samples prompt group[i] of the U prompts.  lps: what each request records (sv_cb_admit_logprobs), nullptr = nothing.
static int cb_admit_impl(sv_engine* e, const void* dev_embeds, int32_t U, int32_t S0_all, const int32_t* lens, int32_t n, const int32_t* group,
                         const sv_cb_request* reqs, const sv_cb_logprobs* lps, int32_t* slots_out, sv_stream stream) {
    const int mp = e->pages_per_seq, mb = e->cfg.max_batch;
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(e->cfg.device));
    HIPCHECK(hipEventRecord(e->gen_event, (hipStream_t)stream));
    hipStream_t st = e->gen_stream;
    HIPCHECK(hipStreamWaitEvent(st, e->gen_event, 0));
    SVCHECK(cb_begin(e, st));
    if (group && !e->fork_desc) SVCHECK(dalloc(e, &e->fork_desc, 6 * (size_t)mb));
    PcAdmit pc;
    AdmitPlan p;
    if (e->pc_on) {
        if (e->exp & SV_EXP_BATCH_REMAINDER)
            return fail(SV_ENOTSUP, "sv_cb_admit: the prefix cache is on and the A/B arm SV_EXP_BATCH_REMAINDER is selected (its remainder rows depend on the batch)");
        if (((uintptr_t)dev_embeds & 15) != 0) return fail(SV_EINVAL, "sv_cb_admit: the prefix cache reads the prompt rows in 16-byte pieces: align dev_embeds to 16 bytes");
        SVCHECK(pc_lookup(e, dev_embeds, U, S0_all, lens, pc, st));
        p.pc = &pc;
    }
    p.record = [&] { for (int i = 0; lps && i < n; ++i) if (lps[i].enable) return true; return false; }();
    if (p.record) SVCHECK(cb_lp_alloc(e));
    for (int s2 = 0; s2 < cb_slot_cap(e) && (int)p.slots.size() < n; ++s2) if (!e->cb_used[s2]) p.slots.push_back(s2);
    p.rows.assign((size_t)n * mp, e->trash_page);
    p.map.resize(n); p.pos.resize(n); p.hs.resize(n); p.hb.resize(n); p.seen_rows.resize(n);
    SVCHECK(group ? plan_group(e, U, lens, n, group, reqs, p) : plan_plain(e, n, S0_all, lens, reqs, p));
    for (int i = 0; i < n; ++i) {
        const int s2 = p.slots[i];
        e->cb_used[s2] = 1;
        cb_fill_slot(reqs[i], p.hs[i], p.hb[i], p.seen_rows[i], e->seen_words);
        if (e->cb_K) p.hs[i].base = p.pos[i] + 1;        // the prompt length: the drafting selection places the slot's rows from it
        p.map[i] = s2;
        slots_out[i] = s2;
    }
    return cb_admit_commit(e, dev_embeds, U, S0_all, lens, reqs, lps, p, slots_out, st);
}

// the per-request checks behind the engine check: the budget against max_seq_len and the request itself; len_of(i) = the prompt rows of request i
template <class LenOf>
static int cb_check_requests(const sv_engine* e, const char* who, int n, const sv_cb_request* reqs, LenOf len_of) {
    const sv_config& c = e->cfg;
    for (int i = 0; i < n; ++i) {
        const sv_cb_request& r = reqs[i];
        const int len = len_of(i);
        if (r.max_new_tokens < 1 || len > c.max_seq_len || len + r.max_new_tokens > c.max_seq_len)
            return fail(SV_EINVAL, "%s: request %d: prompt %d + max_new_tokens %d out of range (max_seq_len %d)", who, i, len, r.max_new_tokens, c.max_seq_len);
        SVCHECK(cb_check_request(r, c.vocab, i, who));
    }
    return 0;
}

extern "C" int sv_cb_admit(sv_engine* e, const void* dev_embeds, int32_t n, int32_t S0, const sv_cb_request* reqs,
                           int32_t* slots_out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (!dev_embeds || !reqs || !slots_out || n < 1) return fail(SV_EINVAL, "sv_cb_admit: null argument or empty batch");
    if (n > e->cfg.max_batch) return fail(SV_EINVAL, "sv_cb_admit: %d requests exceed max_batch %d", n, e->cfg.max_batch);
    if (S0 < 1) return fail(SV_EINVAL, "sv_cb_admit: bad prompt length %d", S0);
    SVCHECK(cb_check_requests(e, "sv_cb_admit", n, reqs, [&](int) { return S0; }));
    return cb_admit_impl(e, dev_embeds, n, S0, nullptr, n, nullptr, reqs, nullptr, slots_out, stream);
}

extern "C" int sv_cb_admit_ragged(sv_engine* e, const void* dev_embeds_packed, int32_t n, const int32_t* host_lens, const sv_cb_request* reqs,
                                  int32_t* slots_out, sv_stream stream) {
    // (the checks that need no engine come first: they are the same on a machine without a GPU)
    if (!dev_embeds_packed || !host_lens || !reqs || !slots_out || n < 1) return fail(SV_EINVAL, "sv_cb_admit_ragged: null argument or empty batch");
    for (int i = 0; i < n; ++i)
        if (host_lens[i] < 1) return fail(SV_EINVAL, "sv_cb_admit_ragged: request %d: bad prompt length %d", i, host_lens[i]);
    SVCHECK(check_ready(e));
    if (n > e->cfg.max_batch) return fail(SV_EINVAL, "sv_cb_admit_ragged: %d requests exceed max_batch %d", n, e->cfg.max_batch);
    SVCHECK(cb_check_requests(e, "sv_cb_admit_ragged", n, reqs, [&](int i) { return host_lens[i]; }));
    return cb_admit_impl(e, dev_embeds_packed, n, 0, host_lens, n, nullptr, reqs, nullptr, slots_out, stream);
}

// sv_cb_admit_shared, and sv_cb_admit_logprobs = that plus what each request records (lps == NULL or every enable == 0: sv_cb_admit_shared's tokens
// and launches)
static int cb_admit_group(const char* who, sv_engine* e, const void* dev_embeds_packed, int32_t n_prompts, const int32_t* host_lens, int32_t n,
                          const int32_t* host_group, const sv_cb_request* reqs, const sv_cb_logprobs* lps, int32_t* slots_out, sv_stream stream) {
    // (the checks that need no engine come first: they are the same on a machine without a GPU)
    if (!dev_embeds_packed || !host_lens || !host_group || !reqs || !slots_out) return fail(SV_EINVAL, "%s: null argument", who);
    SVCHECK(shared_check_group(who, host_lens, n_prompts, host_group, n));
    SVCHECK(cb_check_logprobs(reqs, lps, n, who));
    SVCHECK(check_ready(e));
    if (n > e->cfg.max_batch) return fail(SV_EINVAL, "%s: %d requests exceed max_batch %d", who, n, e->cfg.max_batch);
    SVCHECK(cb_check_requests(e, who, n, reqs, [&](int i) { return host_lens[host_group[i]]; }));
    return cb_admit_impl(e, dev_embeds_packed, n_prompts, 0, host_lens, n, host_group, reqs, lps, slots_out, stream);
}
extern "C" int sv_cb_admit_shared(sv_engine* e, const void* dev_embeds_packed, int32_t n_prompts, const int32_t* host_lens, int32_t n,
                                  const int32_t* host_group, const sv_cb_request* reqs, int32_t* slots_out, sv_stream stream) {
    return cb_admit_group("sv_cb_admit_shared", e, dev_embeds_packed, n_prompts, host_lens, n, host_group, reqs, nullptr, slots_out, stream);
}
extern "C" int sv_cb_admit_logprobs(sv_engine* e, const void* dev_embeds_packed, int32_t n_prompts, const int32_t* host_lens, int32_t n,
                                    const int32_t* host_group, const sv_cb_request* reqs, const sv_cb_logprobs* lps, int32_t* slots_out,
                                    sv_stream stream) {
    return cb_admit_group("sv_cb_admit_logprobs", e, dev_embeds_packed, n_prompts, host_lens, n, host_group, reqs, lps, slots_out, stream);
}

extern "C" int sv_cb_step(sv_engine* e, int32_t n_steps, int32_t* n_live_out, sv_stream stream) {
    SVCHECK(check_ready(e));
    if (n_steps < 1 || !n_live_out) return fail(SV_EINVAL, "sv_cb_step: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->cb_active) return fail(SV_ESTATE, "sv_cb_step: no continuous batch (sv_cb_admit first)");
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->gen_stream;
    const int Bb = cb_bucket(e);
    const bool record = cb_any_records(e);
    hipGraphExec_t gexec = nullptr;
    int per_launch = 1;
    // drafting: a verification step -- decode_forward over the row bucket with the K / V pre-write in front of every attention launch (the rows
    // of a slot see their siblings through the cache, as in sv_generate_lookup), then the per-slot selection over the bucket's Bb / K1 slots.
    // (the kept graphs carry no drafting setting in their key: sv_cb_set_lookup and sv_debug_cb_set_lookup_drafts drop them)
    const bool draft = e->cb_K > 0;
    struct LookupOff { sv_engine* e; ~LookupOff() { e->lookup_on = false; } } lookup_off{e};
    e->lookup_on = draft;
    const auto one_step = [&]() {
        decode_forward(e, Bb, st);
        if (draft) {
            CbLookupArgs q;
            cb_lookup_args(e, q, nullptr, record, false);
            launch_cb_lookup_step(q, Bb / cb_k1(e), st);
            return;
        }
        CbStepArgs a;
        cb_step_args(e, a, nullptr, record);
        launch_cb_step(a, Bb, st);
    };
    if (graph_enabled()) {
        // one graph per (bucket, steps per launch), kept for the life of the engine: every argument is engine-owned.  The scheduler asks for the same
        // n_steps call after call, so the whole call is ONE graph of n_steps copies of the step (engine_generate.hip: the GPU idles 8.6 us between two
        // graph launches and not at all between two kernels of one graph); key = bucket + 1024 * copies (0: the one-step graph) + 2^24 when a slot
        // records log-probs (the recording kernel: a batch in which nobody asks replays the plain graphs).
        auto capture = [&](int copies, hipGraphExec_t* out) -> int {
            const int key = Bb + 1024 * (copies > 1 ? copies : 0) + (record ? 1 << 24 : 0);
            GraphSlot& slot = e->cb_graphs[key];         // (the map's key says everything: the slot's own stays empty)
            if (!slot.x) SVCHECK(slot.use("", st, copies, one_step));
            *out = slot.x;
            return 0;
        };
        if (n_steps >= 2 && n_steps <= graph_steps_cap()) {
            SVCHECK(capture(n_steps, &gexec));
            if (gexec) per_launch = n_steps;
        }
        if (!gexec) SVCHECK(capture(1, &gexec));
    }
    for (int i = 0; i < n_steps; i += per_launch) {
        if (gexec) HIPCHECK(hipGraphLaunch(gexec, st));
        else one_step();
    }
    // the live count and the give-up / non-finite flag in one round trip
    HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_CB_LIVE], e->cb_nlive, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(&e->h_flags[HF_BAD], e->d_bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *n_live_out = e->h_flags[HF_CB_LIVE];
    SVCHECK(report_bad_logits(e, st, "sv_cb_step", e->h_flags[HF_BAD]));
    e->timing_graph = gexec ? (double)per_launch : 0.0;
    return 0;
}

extern "C" int sv_cb_poll(sv_engine* e, int32_t* host_live, int32_t* host_steps, int32_t capacity) {
    if (!e || !host_live || !host_steps) return fail(SV_EINVAL, "sv_cb_poll: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (capacity < e->cfg.max_batch) return fail(SV_EINVAL, "sv_cb_poll: capacity %d < max_batch %d", capacity, e->cfg.max_batch);
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2) { host_live[s2] = 0; host_steps[s2] = 0; }
    if (!e->cb_active) return 0;
    HIPCHECK(hipSetDevice(e->cfg.device));
    std::vector<CbSlot> hs(e->cfg.max_batch);
    HIPCHECK(hipMemcpyAsync(hs.data(), e->cb_slots, hs.size() * sizeof(CbSlot), hipMemcpyDeviceToHost, e->gen_stream));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2)
        if (e->cb_used[s2]) { host_live[s2] = hs[s2].live; host_steps[s2] = hs[s2].step; }
    return 0;
}

extern "C" int sv_cb_read(sv_engine* e, int32_t slot, int32_t first, int32_t count, int64_t* host_tokens) {
    if (!e || !host_tokens) return fail(SV_EINVAL, "sv_cb_read: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->cb_active || slot < 0 || slot >= e->cfg.max_batch || !e->cb_used[slot]) return fail(SV_EINVAL, "sv_cb_read: slot %d is not in use", slot);
    if (first < 0 || count < 0 || first + count > e->out_ld) return fail(SV_EINVAL, "sv_cb_read: columns [%d, %d) out of range", first, first + count);
    if (count == 0) return 0;
    HIPCHECK(hipSetDevice(e->cfg.device));
    std::vector<int32_t> tmp(count);
    HIPCHECK(hipMemcpyAsync(tmp.data(), e->out_tok + (size_t)slot * e->out_ld + first, (size_t)count * sizeof(int32_t),
                            hipMemcpyDeviceToHost, e->gen_stream));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    for (int i = 0; i < count; ++i) host_tokens[i] = tmp[i];
    return 0;
}

// columns [first, first + count) of a recording slot's record; only what the slot has emitted (< its step) exists
extern "C" int sv_cb_read_logprobs(sv_engine* e, int32_t slot, int32_t first, int32_t count, float* host_logprob, int32_t* host_rank,
                                   int32_t* host_ids, float* host_lps) {
    if (!e) return fail(SV_EINVAL, "sv_cb_read_logprobs: null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->cb_active || slot < 0 || slot >= e->cfg.max_batch || !e->cb_used[slot]) return fail(SV_EINVAL, "sv_cb_read_logprobs: slot %d is not in use", slot);
    if (!e->cb_lp || !e->cb_lp_host[slot].enable)
        return fail(SV_EINVAL, "sv_cb_read_logprobs: slot %d records no log-probs (admit it through sv_cb_admit_logprobs with enable = 1)", slot);
    if (first < 0 || count < 0) return fail(SV_EINVAL, "sv_cb_read_logprobs: columns [%d, %d) out of range", first, first + count);
    HIPCHECK(hipSetDevice(e->cfg.device));
    hipStream_t st = e->gen_stream;
    int32_t steps = 0;
    HIPCHECK(hipMemcpyAsync(&steps, &e->cb_slots[slot].step, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if ((long long)first + count > steps)
        return fail(SV_EINVAL, "sv_cb_read_logprobs: columns [%d, %d) of slot %d: it has emitted %d tokens", first, first + count, slot, steps);
    if (count == 0) return 0;
    const CbLogprobs& h = e->cb_lp_host[slot];
    const size_t k = (size_t)h.k;
    if (host_logprob) HIPCHECK(hipMemcpyAsync(host_logprob, h.logprob + first, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, st));
    if (host_rank) HIPCHECK(hipMemcpyAsync(host_rank, h.rank + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_ids && k) HIPCHECK(hipMemcpyAsync(host_ids, h.ids + (size_t)first * k, (size_t)count * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (host_lps && k) HIPCHECK(hipMemcpyAsync(host_lps, h.lps + (size_t)first * k, (size_t)count * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    return 0;
}

static int cb_release_locked(sv_engine* e, int slot, hipStream_t st) {
    // a slot released while still generating is stopped first (live -> 0, live counter adjusted on the host's view)
    CbSlot h;
    HIPCHECK(hipMemcpyAsync(&h, e->cb_slots + slot, sizeof(CbSlot), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (h.live) add_i32(e->cb_nlive, -1, 1, st);
    HIPCHECK(hipMemsetAsync(e->cb_slots + slot, 0, sizeof(CbSlot), st));
    const int K1 = cb_k1(e);                             // the slot's decode rows (1 unless the batch drafts)
    HIPCHECK(hipMemsetAsync(e->positions + (size_t)slot * K1, 0, K1 * sizeof(int32_t), st));
    HIPCHECK(hipMemsetAsync(e->cur_tok + (size_t)slot * K1, 0, K1 * sizeof(int32_t), st));
    if (e->cb_K) HIPCHECK(hipMemsetAsync(e->cb_lk_state + slot, 0, sizeof(int32_t), st));      // no drafts in flight
    SVCHECK(cb_lp_set(e, slot, nullptr, st));            // a free slot records nothing: the next holder starts from enable = 0
    fill_i32(e->block_table + (size_t)slot * K1 * e->pages_per_seq, e->trash_page, K1 * e->pages_per_seq, st);
    for (int pg : e->cb_pages[slot]) {
        // a shared prompt page (sv_cb_admit_shared) goes back when its last holder lets go; a private page at once
        if (e->page_refs[pg] > 0 && --e->page_refs[pg] > 0) continue;
        if (e->pc_reg[pg]) { pc_lru_push(e, pg); continue; }      // a cached prompt page without a holder waits in the LRU list
        e->free_pages.push_back(pg);
    }
    e->cb_pages[slot].clear();
    e->cb_used[slot] = 0;
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int sv_cb_release(sv_engine* e, int32_t slot) {
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->cb_active || slot < 0 || slot >= e->cfg.max_batch || !e->cb_used[slot]) return fail(SV_EINVAL, "sv_cb_release: slot %d is not in use", slot);
    HIPCHECK(hipSetDevice(e->cfg.device));
    return cb_release_locked(e, slot, e->gen_stream);
}

extern "C" int sv_cb_reset(sv_engine* e) {
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->cb_active) return 0;
    HIPCHECK(hipSetDevice(e->cfg.device));
    for (int s2 = 0; s2 < e->cfg.max_batch; ++s2)
        if (e->cb_used[s2]) SVCHECK(cb_release_locked(e, s2, e->gen_stream));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    std::fill(e->page_refs.begin(), e->page_refs.end(), 0);
    pc_drop(e);
    e->cb_active = false;
    return 0;
}

// ---- drafting (sv_cb_set_lookup / sv_cb_lookup_counts) ----
namespace sveng {
int cb_check_lookup(const char* who, const sv_lookup* lookup, sv_lookup& lk) {
    lk = lookup ? *lookup : sv_lookup{0, 0, 0};
    if (lk.num_draft_tokens < 0 || lk.num_draft_tokens > SV_LOOKUP_MAX_DRAFT)
        return fail(SV_EINVAL, "%s: num_draft_tokens %d unsupported (0..%d)", who, lk.num_draft_tokens, SV_LOOKUP_MAX_DRAFT);
    if (lk.max_ngram < 0 || lk.max_ngram > SV_LOOKUP_MAX_NGRAM)
        return fail(SV_EINVAL, "%s: max_ngram %d unsupported (1..%d, 0 = 3)", who, lk.max_ngram, SV_LOOKUP_MAX_NGRAM);
    if (lk.max_ngram == 0) lk.max_ngram = 3;
    if (lk.min_ngram < 0 || lk.min_ngram > lk.max_ngram)
        return fail(SV_EINVAL, "%s: min_ngram %d must lie in 1..max_ngram %d (0 = 1)", who, lk.min_ngram, lk.max_ngram);
    if (lk.min_ngram == 0) lk.min_ngram = 1;
    return 0;
}
void cb_drop_graphs(sv_engine* e) { e->cb_graphs.clear(); }      // (GraphSlot's destructor destroys the handles)
}  // namespace sveng

extern "C" int sv_cb_set_lookup(sv_engine* e, const sv_lookup* lookup) {
    sv_lookup lk;
    SVCHECK(cb_check_lookup("sv_cb_set_lookup", lookup, lk));      // (the checks that need no engine come first)
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lock(e->mu);
    if (e->cb_active) return fail(SV_ESTATE, "sv_cb_set_lookup: a continuous batch is active (the setting changes before the first admit or after sv_cb_reset)");
    const int K = lk.num_draft_tokens;
    if (K > 0 && e->kv_dtype != SV_KV_BF16)
        return fail(SV_ENOTSUP, "sv_cb_set_lookup: prompt-lookup drafting is not built for the fp8_e4m3 KV cache (the drafts' K / V pre-write is bf16)");
    if (e->cfg.max_batch / (K + 1) < 1)
        return fail(SV_ENOTSUP, "sv_cb_set_lookup: num_draft_tokens %d + 1 rows per slot exceed engine max_batch %d", K, e->cfg.max_batch);
    if (K == e->cb_K && (K == 0 || (lk.max_ngram == e->cb_max_ngram && lk.min_ngram == e->cb_min_ngram))) return 0;
    HIPCHECK(hipSetDevice(e->cfg.device));
    if (K && !e->cb_lk_state) SVCHECK(dalloc(e, &e->cb_lk_state, (size_t)4 * e->cfg.max_batch + 3));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    cb_drop_graphs(e);                                   // captured with the other setting
    e->cb_K = K;
    if (K) { e->cb_max_ngram = lk.max_ngram; e->cb_min_ngram = lk.min_ngram; }
    return 0;
}

extern "C" int sv_cb_lookup_counts(sv_engine* e, int32_t slot, int32_t* host_counts3) {
    if (!e || !host_counts3) return fail(SV_EINVAL, "sv_cb_lookup_counts: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    host_counts3[0] = host_counts3[1] = host_counts3[2] = 0;
    if (slot < -1 || slot >= e->cfg.max_batch || (slot >= 0 && !(e->cb_active && e->cb_used[slot])))
        return fail(SV_EINVAL, "sv_cb_lookup_counts: slot %d is not in use (-1 = the batch's totals)", slot);
    if (!e->cb_active || !e->cb_K) return 0;
    HIPCHECK(hipSetDevice(e->cfg.device));
    const int mb = e->cfg.max_batch;
    const int32_t* src = e->cb_lk_state + mb + (slot < 0 ? 3 * mb : 3 * slot);
    HIPCHECK(hipMemcpyAsync(host_counts3, src, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, e->gen_stream));
    HIPCHECK(hipStreamSynchronize(e->gen_stream));
    return 0;
}

// ---- the prefix cache's switch and counters (sv_cb_set_prefix_cache / sv_cb_prefix_cache_info) ----
extern "C" int sv_cb_set_prefix_cache(sv_engine* e, int32_t enable) {
    if (!e) return fail(SV_EINVAL, "null engine");
    std::lock_guard<std::mutex> lock(e->mu);
    if (e->cb_active) return fail(SV_ESTATE, "sv_cb_set_prefix_cache: a continuous batch is active (the setting changes before the first admit or after sv_cb_reset)");
    if (!enable) { e->pc_on = false; return 0; }
    if (e->kv_dtype != SV_KV_BF16)
        return fail(SV_ENOTSUP, "sv_cb_set_prefix_cache: not built for the fp8_e4m3 KV cache (a prompt pass behind cached pages sees the dequantised cache, a "
                                "one-shot pass the unquantised rows: the tokens would not be those of the same request with the cache off)");
    if (e->exp & SV_EXP_BATCH_REMAINDER)
        return fail(SV_ENOTSUP, "sv_cb_set_prefix_cache: the A/B arm SV_EXP_BATCH_REMAINDER is selected (its remainder rows depend on the batch)");
    if (e->cfg.hidden % 8 != 0) return fail(SV_ENOTSUP, "sv_cb_set_prefix_cache: hidden %d is no multiple of 8 (the digest reads 16-byte pieces)", e->cfg.hidden);
    HIPCHECK(hipSetDevice(e->cfg.device));
    if (!e->pc_dig) SVCHECK(dalloc(e, &e->pc_dig, (size_t)e->cfg.max_batch * e->pages_per_seq * 2));
    if (!e->pc_desc) SVCHECK(dalloc(e, &e->pc_desc, (size_t)2 * e->cfg.max_batch));
    e->pc_on = true;
    return 0;
}

extern "C" int sv_cb_prefix_cache_info(sv_engine* e, int64_t* host_out5) {
    if (!e || !host_out5) return fail(SV_EINVAL, "sv_cb_prefix_cache_info: null argument");
    std::lock_guard<std::mutex> lock(e->mu);
    for (int i = 0; i < 5; ++i) host_out5[i] = 0;
    if (!e->pc_on || !e->cb_active) return 0;
    host_out5[0] = e->pc_lookups; host_out5[1] = e->pc_reused; host_out5[2] = (int64_t)e->pc_table.size(); host_out5[3] = (int64_t)e->pc_lru.size();
    host_out5[4] = e->pc_evictions;
    return 0;
}
