// One logits row of a continuous-batching slot: the selection, the log-prob record and the bookkeeping, shared by cb_step_kernel (sampling.hip:
// one row per slot and launch) and cb_lookup_step_kernel (cb_lookup/cb_lookup.hip: up to K + 1 rows per slot and launch, one after the
// other).  Everything here runs in an SP_THREADS block whose threads all work for slot s.  The slot's fields are read through the reference
// `sl` where they are used (uniform address), never from a by-value copy: in cb_step_kernel they travel as scalar loads.
#pragma once
#include "kernels.h"
#include "warp.h"
#include "sample_row.h"
#include "topk.h"

namespace sv {

__device__ __forceinline__ void argmax_pair(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// max-shifted sums of a row (sampling.hip, sv_generate_stats): m = max x, ls = log sum exp(x - m), ent = ls - sum exp(x - m) (x - m) / sum exp(x - m)
template <class F>
__device__ __forceinline__ void ts_row_sums(F x, int V, float* red, float& m, float& ls, float& ent) {
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < V; i += SP_THREADS) mx = fmaxf(mx, x(i));
    mx = wp_block_max(mx, red);
    float s = 0.f, u = 0.f;
    for (int i = tid; i < V; i += SP_THREADS) {
        const float d = x(i) - mx;
        const float ex = expf(d);
        s += ex;
        u += ex > 0.f ? ex * d : 0.f;                                // a term with e = 0 (x = -inf included) adds 0
    }
    s = wp_block_sum(s, red);
    u = wp_block_sum(u, red);
    m = mx;
    ls = logf(s);
    ent = ls - u / s;
}

// the list of one row (topk.h row_topk) to ids[0..k) / lps[0..k) and *rank: n slots found; a row without a comparable value reads -1 / NaN / 0
__device__ __forceinline__ void topk_store(int n, int k, float nolp, bool wr, int rk, int32_t* ids, float* lps, int32_t* rank) {
    const RowTopkSmem& sm = row_topk_smem();
    if ((int)threadIdx.x < k) {
        ids[threadIdx.x] = sm.id[threadIdx.x];
        lps[threadIdx.x] = n > 0 ? sm.lp[threadIdx.x] : nolp;
    }
    if (rank && threadIdx.x == 0) *rank = (wr && n > 0) ? rk : 0;
}

__device__ __forceinline__ void cb_vllm_process(const CbStepArgs& p, const CbSlot& sl, int s, float* row) {
    const int tid = threadIdx.x;
    if (tid < sl.n_bias) {                                          // 1. logit_bias (distinct ids: checked at admit)
        const CbBias& bb = p.bias[s];
        row[bb.id[tid]] += bb.val[tid];
    }
    __syncthreads();
    if (sl.step < sl.min_new) {                                     // 2. min_tokens: eos and every stop id -> -inf (after the bias)
        if (tid == 0 && sl.eos >= 0) row[sl.eos] = -INFINITY;
        if (tid >= 1 && tid <= sl.n_any) row[sl.any[tid - 1]] = -INFINITY;
    }
    __syncthreads();
    const float rp = sl.penalty, fp = sl.frequency, pp = sl.presence;
    if (rp == 1.0f && fp == 0.f && pp == 0.f) return;              // 3. penalties (-inf stays -inf through all three)
    const uint32_t* srow = p.seen + (size_t)s * p.seen_words;
    const uint16_t* crow = p.counts + (size_t)s * p.ld_counts;
    for (int i = tid * 4; i < p.V; i += SP_THREADS * 4) {          // ld and ld_counts are multiples of 4: aligned vector accesses
        float4 v = *reinterpret_cast<const float4*>(row + i);
        const ushort4 c = *reinterpret_cast<const ushort4*>(crow + i);
        const uint32_t bits = srow[i >> 5] >> (i & 31);
        float a[4] = {v.x, v.y, v.z, v.w};
        const float cn[4] = {(float)c.x, (float)c.y, (float)c.z, (float)c.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float l = a[e];
            if ((bits >> e) & 1u) l = l > 0.f ? l / rp : l * rp;   // vLLM: repetition over prompt ids and output ids
            l -= fp * cn[e];
            l -= cn[e] > 0.f ? pp : 0.f;
            a[e] = l;
        }
        v = make_float4(a[0], a[1], a[2], a[3]);
        if (i + 3 < p.V) {
            *reinterpret_cast<float4*>(row + i) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (i + e < p.V) row[i + e] = a[e];
        }
    }
    __syncthreads();
}

// rank of a column whose value is x_tok, without a list (k = 0): row_topk's count, 1 + #{ x(i) > x_tok }; 0 when x_tok is NaN or no column enters
template <class F>
__device__ __forceinline__ int cb_row_rank(F x, int V, float x_tok, float* red) {
    float above = 0.f, any = 0.f;
    for (int i = threadIdx.x; i < V; i += SP_THREADS) {
        const float v = x(i);
        above += v > x_tok ? 1.f : 0.f;
        any = v > -INFINITY ? 1.f : any;
    }
    above = wp_block_sum(above, red);                                // exact: counts < 2^24
    any = wp_block_max(any, red);
    return (x_tok == x_tok && any > 0.f) ? 1 + (int)above : 0;
}

// The log-prob record of one recording slot at its step (CbLogprobs, kernels.h), by every thread of the slot's block: `tok` is the token the
// selection took (block-uniform, inside the vocabulary), `row` the row as the selection saw it (a vLLM slot has rewritten it), srow / hold_eos the
// selection's own processors; the seen bitmap and the counts have not taken `tok` yet.  The functors, the sums and the log-prob expressions are
// token_topk_kernel's, so an HF slot's record equals its solo sv_generate_topk output bit for bit.  A vLLM slot is source 1 with the HF
// processors off: log_softmax over its rewritten row, for a sampling slot divided by T under the top-k / top-p / min_p kept set.
__device__ __forceinline__ void cb_record(const CbSlot& sl, const CbLogprobs& d, const float* row, int V, const uint32_t* srow, bool hold_eos,
                                          int tok, float* red) {
    const int k = d.k, t = sl.step;
    const float T = sl.do_sample ? sl.temperature : 1.0f;
    int32_t* ids = d.ids + (size_t)t * k;
    float* lps = d.lps + (size_t)t * k;
    const float qnan = __uint_as_float(0x7fc00000u);
    float m, ls, ent, lp_tok, nolp = qnan;
    int rk = 0, n = 0;
    if (d.source == 0) {
        ts_row_sums([&](int i) { return row[i] / T; }, V, red, m, ls, ent);
        auto key = [&](int i) { return row[i]; };
        lp_tok = (row[tok] / T - m) - ls;
        nolp = (row[0] / T - m) - ls;
        if (k > 0) n = row_topk(key, V, k, [&](float v) { return (v / T - m) - ls; }, red, true, row[tok], &rk);
        else rk = cb_row_rank(key, V, row[tok], red);
    } else {
        const int eos = sl.eos;
        const float pen = sl.penalty;
        auto base = [&](int i) { return (hold_eos && i == eos) ? -INFINITY : rep_penalty(row[i], i, srow, pen); };
        if (sl.do_sample) {
            const float invT = 1.0f / sl.temperature;
            WarpStats w = row_warp_stats<false, true>([&](int i) { return base(i) * invT; }, V, sl.top_k, sl.top_p, 1, red);
            w.mthr = wp_minp_thr(w.mx, sl.min_p > 0.f ? __logf(sl.min_p) : -INFINITY);
            auto kept = [&](int i) { const float s = base(i); return wp_keep(w, s * invT) ? s : -INFINITY; };      // the key: before the division by T
            ts_row_sums([&](int i) { const float s = base(i); return wp_keep(w, s * invT) ? s / T : -INFINITY; }, V, red, m, ls, ent);
            const float xt = kept(tok);
            lp_tok = (xt / T - m) - ls;
            if (k > 0) n = row_topk(kept, V, k, [&](float v) { return (v / T - m) - ls; }, red, true, xt, &rk);
            else rk = cb_row_rank(kept, V, xt, red);
        } else {
            ts_row_sums(base, V, red, m, ls, ent);
            const float xt = base(tok);
            lp_tok = (xt - m) - ls;
            if (k > 0) n = row_topk(base, V, k, [&](float v) { return (v - m) - ls; }, red, true, xt, &rk);
            else rk = cb_row_rank(base, V, xt, red);
        }
    }
    if (k > 0) topk_store(n, k, nolp, true, rk, ids, lps, d.rank + t);
    else if (threadIdx.x == 0) d.rank[t] = rk;
    if (threadIdx.x == 0) d.logprob[t] = lp_tok;
}

// the LDS of one selection: red [SP_THREADS / 64], scan [SP_THREADS], one int, and the per-wave arg-max pairs [SP_THREADS / 64] each
struct CbRowLds { float* red; float* scan; int* result; float* am_v; int* am_i; };

// Steps 1 of a row: slot s (live, block-uniform) selects from `row` against its CURRENT state -- the vLLM rewrite of the row in place, the
// repetition set, the min-length hold on sl.step, greedy arg-max (lowest id on ties) or sample_row with (seed, sl.step, 0) -- and, LP and the
// slot recording, writes the record at column sl.step.  Returns the token (block-uniform; the 0x7fffffff sentinel when the row has no finite
// logit: cb_row_commit turns it into id 0 and raises `bad`).  srow_out: the HF slot's repetition set, nullptr when it has none.
template <bool LP>
__device__ __forceinline__ int cb_row_select(const CbStepArgs& p, const CbSlot& sl, int s, const float* row, const CbRowLds& m, const uint32_t*& srow_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool vl = sl.vllm != 0;
    if (vl) cb_vllm_process(p, sl, s, const_cast<float*>(row));    // block-uniform; rewrites the row in place
    const uint32_t* srow = (!vl && p.seen && sl.penalty > 0.f && sl.penalty != 1.0f) ? p.seen + (size_t)s * p.seen_words : nullptr;
    const bool hold_eos = !vl && sl.step < sl.min_new;              // MinLengthLogitsProcessor
    int tok;
    if (sl.do_sample) {
        const float invT = 1.0f / sl.temperature;
        const float minp_log = sl.min_p > 0.f ? __logf(sl.min_p) : -INFINITY;
        auto lg = [&](int i) { return (hold_eos && i == sl.eos) ? -INFINITY : rep_penalty(row[i], i, srow, sl.penalty) * invT; };
        tok = sample_row(lg, p.V, sl.top_k, sl.top_p, minp_log, sl.seed, (uint32_t)sl.step, 0u, m.red, m.scan, m.result);
    } else {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid * 4; i < p.V; i += SP_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4*>(row + i);
            const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < p.V && !(hold_eos && i + e == sl.eos)) argmax_pair(best, bi, rep_penalty(a[e], i + e, srow, sl.penalty), i + e);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            argmax_pair(best, bi, ov, oi);
        }
        if (lane == 0) { m.am_v[wave] = best; m.am_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SP_THREADS / 64; ++w) argmax_pair(best, bi, m.am_v[w], m.am_i[w]);
            *m.result = bi;
        }
        __syncthreads();
        tok = *m.result;
    }
    if constexpr (LP) {
        const CbLogprobs& d = p.lp[s];
        if (d.enable) cb_record(sl, d, row, p.V, srow, hold_eos, (unsigned)tok >= (unsigned)p.V ? 0 : tok, m.red);       // block-uniform
    }
    srow_out = srow;
    return tok;
}

// Step 2 of a row, by ONE thread of the block: the token into the slot's history at column sl.step, the seen bit and the vLLM count, EOS /
// budget / stop_any / stop sequence, the step counter, and -- when the request ends here -- live, n_live and events.  The caller writes the
// slot's decode rows (cur_tok, positions): how many a slot owns is the caller's layout.  Returns the id emitted; fin = the request ended.
__device__ __forceinline__ int cb_row_commit(const CbStepArgs& p, const CbSlot& sl, int s, int tok, const uint32_t* srow, bool& fin_out) {
    if ((unsigned)tok >= (unsigned)p.V) {               // no finite logit: never index the embedding table with the sentinel
        tok = 0;
        if (p.bad) atomicCAS(p.bad, 0, 1);              // 0 -> 1 only (see finish_step_kernel)
    }
    const bool vl = sl.vllm != 0;
    const int t = sl.step;
    int32_t* out = p.out_tokens + (size_t)s * p.ld_out;
    out[t] = tok;
    if (srow) atomicOr(p.seen + (size_t)s * p.seen_words + (tok >> 5), 1u << (tok & 31));
    bool fin = tok == sl.eos || t + 1 >= sl.budget;
    if (vl) {                                                       // the slot's only writer: plain read-modify-write of its count
        uint16_t* c = p.counts + (size_t)s * p.ld_counts + tok;
        *c = (uint16_t)(*c + 1);
        atomicOr(p.seen + (size_t)s * p.seen_words + (tok >> 5), 1u << (tok & 31));
        for (int i = 0; i < sl.n_any; ++i)
            if (tok == p.slots[s].any[i]) fin = true;
    }
    if (!fin && sl.n_stop > 0 && t + 1 >= sl.n_stop) {
        fin = true;
        for (int i = 0; i < sl.n_stop; ++i)
            if (out[t + 1 - sl.n_stop + i] != p.slots[s].stop[i]) { fin = false; break; }      // from memory: indexing the register copy puts it on the stack
    }
    p.slots[s].step = t + 1;
    if (fin) {
        p.slots[s].live = 0;
        atomicSub(p.n_live, 1);
        atomicAdd(p.events, 1);
    }
    fin_out = fin;
    return tok;
}

}  // namespace sv
