// Token selection + generation bookkeeping on device (no per-step host sync).
//   argmax        : greedy (HF _sample with do_sample=False): argmax of the fp32 logits, lowest index on ties
//   sample_top_p  : TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (warp.h) -> softmax -> one
//                   multinomial draw (counter-based RNG; distributional parity with torch.multinomial)
//   finish_step   : pad-after-EOS, append, EOS bookkeeping, the reference's row-0 stop sequence
//                   (starvector_base.py:9-20), max-length budget -> device "done" flag
#include "kernels.h"
#include "warp.h"
#include "sample_row.h"
#include "topk.h"
#include "cb_row.h"

namespace sv {

// (SP_THREADS, rep_penalty, sample_row_topk and sample_row live in sample_row.h: lookup_sampled/lookup_sampled.hip draws with them too;
//  argmax_pair, ts_row_sums and the continuous batch's row body in cb_row.h: cb_lookup/cb_lookup.hip selects with them too)

// grid (B, AM_SPLIT): one CU streams ~25 GB/s, so a 196 KB logits row is scanned by AM_SPLIT blocks; each
// leaves (max, index) of its slice and finish_step_kernel merges them (lowest index wins ties)
#define AM_SPLIT 8
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int ld, int V,
                                                     float* __restrict__ pval, int32_t* __restrict__ pidx,
                                                     const uint32_t* __restrict__ seen, int seen_words, float penalty) {
    __shared__ float sv_[4];
    __shared__ int si_[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (size_t)blockIdx.x * ld;
    const uint32_t* srow = seen ? seen + (size_t)blockIdx.x * seen_words : nullptr;
    const int per = (((V + AM_SPLIT - 1) / AM_SPLIT) + 3) & ~3;
    const int beg = blockIdx.y * per, end = min(beg + per, V);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = beg + tid * 4; i < end; i += 256 * 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + i);
        const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < end) argmax_pair(best, bi, rep_penalty(a[e], i + e, srow, penalty), i + e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        argmax_pair(best, bi, ov, oi);
    }
    if (lane == 0) { sv_[wave] = best; si_[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) argmax_pair(best, bi, sv_[w], si_[w]);
        pval[blockIdx.x * AM_SPLIT + blockIdx.y] = best;
        pidx[blockIdx.x * AM_SPLIT + blockIdx.y] = bi;
    }
}
__global__ void argmax_merge_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                    int32_t* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int s = 0; s < AM_SPLIT; ++s) argmax_pair(best, bi, pval[b * AM_SPLIT + s], pidx[b * AM_SPLIT + s]);
    out[b] = bi;
}
void launch_argmax_partial(const float* logits, int ld, int V, float* pval, int32_t* pidx, int B, const uint32_t* seen,
                           int seen_words, float penalty, hipStream_t st) {
    argmax_kernel<<<dim3(B, AM_SPLIT), 256, 0, st>>>(logits, ld, V, pval, pidx, seen, seen_words, penalty);
}
void launch_argmax(const float* logits, int ld, int V, int32_t* out, float* pval, int32_t* pidx, int B, hipStream_t st) {
    launch_argmax_partial(logits, ld, V, pval, pidx, B, nullptr, 0, 1.f, st);
    argmax_merge_kernel<<<(B + 63) / 64, 64, 0, st>>>(pval, pidx, out, B);
}

__global__ __launch_bounds__(SP_THREADS) void sample_top_p_kernel(SampleArgs p) {
    __shared__ float red[SP_THREADS / 64];
    __shared__ float scan[SP_THREADS];
    __shared__ int result;
    const float* row = p.logits + (size_t)blockIdx.x * p.ld;
    const uint32_t* srow = p.seen ? p.seen + (size_t)blockIdx.x * p.seen_words : nullptr;
    const float invT = 1.0f / p.temperature;
    auto lg = [&](int i) { return rep_penalty(row[i], i, srow, p.penalty) * invT; };     // processors, then temperature
    const int tok = sample_row(lg, p.V, p.top_k, p.top_p, p.minp_log, p.seed, (uint32_t)p.step[0], (uint32_t)blockIdx.x, red, scan, &result);
    if (threadIdx.x == 0) p.out[blockIdx.x] = tok;
}
void launch_sample_top_p(const SampleArgs& a, hipStream_t st) {
    sample_top_p_kernel<<<a.B, SP_THREADS, 0, st>>>(a);
}

// ------------------------------------------------------------------------------------------------
// sv_generate_ex outputs (HF output_scores / output_logits): the raw row and the processed row of step t = *step, written by a
// wide grid of 16-byte stores (2 x rows x V fp32 per step).  Sampling first takes the row's TopK -> TopP thresholds with the sampler's
// score functor (one 1024-thread block per row, thresholds to p.warp) -- through row_warp_stats<false, true>, i.e. warp.h's
// row_warp_stats_select<49> / row_warp_stats_regs<49, ONCE> / row_warp_stats_global, NOT the forms the sampler draws through
// (sample_row_topk, or row_warp_stats<true, true> = regs<16> / regs<52> / global).  That a drawn token has a finite captured score therefore
// spans two forms: tests/test_gpu_warper_kept_set.py holds each to the float64 reference by exact set equality and
// test_drawn_support_captured_support_and_reference_are_one_set ties them together.
// ------------------------------------------------------------------------------------------------
#define CAP_QPB 1024                       // 16-byte quads per block of the write grid (4096 floats)

__global__ __launch_bounds__(SP_THREADS) void capture_warp_kernel(CaptureArgs p) {
    __shared__ float red[SP_THREADS / 64];
    if (*p.done) return;
    const int t = *p.step;
    if (t < 0 || t >= p.desc->max_new) return;
    const int b = blockIdx.x;
    const float* row = p.src + (size_t)b * p.ld_src;
    const uint32_t* srow = p.seen ? p.seen + (size_t)b * p.seen_words : nullptr;
    const float invT = 1.0f / p.temperature;
    const bool hold = t < p.min_new;
    const int eos = p.eos;
    auto lg = [&](int i) { return (hold && i == eos) ? -INFINITY : rep_penalty(row[i], i, srow, p.penalty) * invT; };
    const WarpStats w = row_warp_stats<false, true>(lg, p.V, p.top_k, p.top_p, 1, red);
    if (threadIdx.x == 0) {
        float* o = p.warp + (size_t)b * 8;
        o[0] = w.kth; o[1] = w.mx; o[2] = w.invZ; o[3] = w.v0; o[4] = w.smin; o[5] = wp_minp_thr(w.mx, p.minp_log);
    }
}

__global__ __launch_bounds__(256) void capture_write_kernel(CaptureArgs p) {
    if (*p.done) return;
    const CaptureDesc d = *p.desc;
    const int t = *p.step;
    const int b = blockIdx.x;
    if (t < 0 || t >= d.max_new || b >= d.rows) return;
    const float* row = p.src + (size_t)b * p.ld_src;
    const size_t off = ((size_t)t * d.rows + b) * (size_t)d.ld;
    const int q0 = blockIdx.y * CAP_QPB, q1 = q0 + CAP_QPB;
    const bool edges = blockIdx.y == 0;
    if (d.logits && (p.what & 1)) capture_store_row(d.logits + off, p.V, q0, q1, edges, [&](int j) { return row[j]; });
    if (!d.scores || !(p.what & 2)) return;
    const uint32_t* srow = p.seen ? p.seen + (size_t)b * p.seen_words : nullptr;
    const int eos = t < p.min_new ? p.eos : -1;                      // MinLength: the EOS id at -inf while held
    const float pen = p.penalty;
    if (p.do_sample) {
        const float* o = p.warp + (size_t)b * 8;
        WarpStats w;
        w.kth = o[0]; w.mx = o[1]; w.invZ = o[2]; w.v0 = o[3]; w.smin = o[4]; w.mthr = o[5];
        const float T = p.temperature, invT = 1.0f / T;
        // kept: the sampler's test on the sampler's value (s * invT); reported: HF's TemperatureLogitsWarper, s / T
        capture_store_row(d.scores + off, p.V, q0, q1, edges, [&](int j) {
            const float s = j == eos ? -INFINITY : rep_penalty(row[j], j, srow, pen);
            return wp_keep(w, s * invT) ? s / T : -INFINITY;
        });
    } else {
        capture_store_row(d.scores + off, p.V, q0, q1, edges,
                          [&](int j) { return j == eos ? -INFINITY : rep_penalty(row[j], j, srow, pen); });
    }
}
void launch_capture_rows(const CaptureArgs& a, hipStream_t st) {
    if (a.do_sample && a.warp && (a.what & 2)) capture_warp_kernel<<<a.B, SP_THREADS, 0, st>>>(a);
    capture_write_kernel<<<dim3(a.B, (a.V + 4 * CAP_QPB - 1) / (4 * CAP_QPB)), 256, 0, st>>>(a);
}

// ------------------------------------------------------------------------------------------------
// sv_generate_stats: log-prob, processed log-prob and entropy of the token each row emits (TokenStatsArgs, kernels.h).  One 1024-thread block per
// row, every reduction in fp32 and in a fixed order (a thread's columns ascending, xor butterfly inside a wave, waves in wave order).
//   max-shifted sums, as score.hip: m = max x, s = sum exp(x - m), u = sum exp(x - m) (x - m);  lse = m + log s, entropy = log s - u / s
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SP_THREADS) void token_stats_kernel(TokenStatsArgs p) {
    __shared__ float red[SP_THREADS / 64];
    if (*p.done) return;
    const TokenStatsDesc d = *p.desc;
    const int t = *p.step;
    const int b = blockIdx.x;
    if (t < 0 || t >= d.max_new || b >= d.rows) return;
    const bool live = p.unfinished[b] != 0;                          // block-uniform
    const float* row = p.src + (size_t)b * p.ld_src;
    float* raw = p.raw + (size_t)b * 4;
    const float T = p.do_sample ? p.temperature : 1.0f;
    const size_t o = (size_t)b * (size_t)d.ld + (size_t)t;
    if (!live) {                                                     // finished before this step: 0, what completion_logprobs returns at pads
        if ((p.what & 2) && threadIdx.x == 0) {
            if (d.logprob) d.logprob[o] = 0.f;
            if (d.processed) d.processed[o] = 0.f;
            if (d.entropy) d.entropy[o] = 0.f;
        }
        return;
    }
    float m, ls, ent;
    if (p.what & 1) {
        ts_row_sums([&](int i) { return row[i] / T; }, p.V, red, m, ls, ent);
        if (!(p.what & 2)) {
            if (threadIdx.x == 0) { raw[0] = m; raw[1] = ls; raw[2] = ent; }
            return;
        }
    } else {
        m = raw[0]; ls = raw[1]; ent = raw[2];
    }
    int tok;
    if (p.pval) {                                                    // greedy: the merge finish_step_kernel does
        float best = -INFINITY;
        tok = 0x7fffffff;
        for (int s = 0; s < AM_SPLIT; ++s) argmax_pair(best, tok, p.pval[b * AM_SPLIT + s], p.pidx[b * AM_SPLIT + s]);
    } else {
        tok = p.next[b];
    }
    if ((unsigned)tok >= (unsigned)p.V) tok = 0;                     // no finite logit: finish_step_row emits 0 and raises the call's flag
    // the emitted id is never a banned or held one: row[tok] is still its raw value after the in-place rewrites
    if (threadIdx.x == 0) {
        if (d.logprob) d.logprob[o] = (row[tok] / T - m) - ls;
        if (d.entropy) d.entropy[o] = ent;
    }
    if (!d.processed) return;
    const uint32_t* srow = p.seen ? p.seen + (size_t)b * p.seen_words : nullptr;
    const int eos = t < p.min_new ? p.eos : -1;                      // MinLength: the EOS id at -inf while held
    const float pen = p.penalty;
    auto base = [&](int i) { return i == eos ? -INFINITY : rep_penalty(row[i], i, srow, pen); };
    float pm, pls, pent, stok;
    if (p.do_sample) {
        // the capture's thresholds (capture_warp_kernel): the sampler's score functor through row_warp_stats; kept = the sampler's test on the
        // sampler's value (s * invT), the value that is normalised = HF's TemperatureLogitsWarper, s / T (capture_write_kernel)
        const float invT = 1.0f / p.temperature;
        WarpStats w = row_warp_stats<false, true>([&](int i) { return base(i) * invT; }, p.V, p.top_k, p.top_p, 1, red);
        w.mthr = wp_minp_thr(w.mx, p.minp_log);
        ts_row_sums([&](int i) { const float s = base(i); return wp_keep(w, s * invT) ? s / T : -INFINITY; }, p.V, red, pm, pls, pent);
        stok = base(tok) / T;
    } else {
        ts_row_sums(base, p.V, red, pm, pls, pent);
        stok = base(tok);
    }
    if (threadIdx.x == 0) d.processed[o] = (stok - pm) - pls;
}
void launch_token_stats(const TokenStatsArgs& a, hipStream_t st) {
    token_stats_kernel<<<a.B, SP_THREADS, 0, st>>>(a);
}

// ------------------------------------------------------------------------------------------------
// sv_generate_topk: the k best ids of the distribution behind the token each row emits, and the token's rank (TokenTopkArgs, kernels.h; the list is
// topk.h's row_topk).  The sums are ts_row_sums over the functors of token_stats_kernel and a slot's log-prob is that kernel's expression for its
// id: the slot of the emitted id equals dev_logprob / dev_logprob_processed bit for bit.  Every thread of the block calls these.
// ------------------------------------------------------------------------------------------------
// (topk_store, the list of one row to ids / lps / *rank, is cb_row.h's)
// source 0 on one fp32 row: log_softmax(row / T), keyed on row[i]; tok < 0: no rank.  A continuous-batching launch can call it as it is.
__device__ __forceinline__ void token_topk_raw_row(const float* row, int V, float T, int k, int tok, float* red, int32_t* ids, float* lps,
                                                   int32_t* rank) {
    float m, ls, ent;
    ts_row_sums([&](int i) { return row[i] / T; }, V, red, m, ls, ent);
    const bool wr = rank != nullptr && tok >= 0;
    int rk = 0;
    const int n = row_topk([&](int i) { return row[i]; }, V, k, [&](float v) { return (v / T - m) - ls; }, red, wr,
                           wr ? row[tok] : __uint_as_float(0x7fc00000u), &rk);
    topk_store(n, k, (row[0] / T - m) - ls, wr, rk, ids, lps, rank);       // (no comparable value: m = -inf or NaN, the NaN dev_logprob holds)
}

// SOURCE is a template argument: the raw form carries none of the warper's registers (row_warp_stats holds the row's 49 values per thread)
template <int SOURCE>
__global__ __launch_bounds__(SP_THREADS) void token_topk_kernel(TokenTopkArgs p) {
    __shared__ float red[SP_THREADS / 64];
    if (*p.done) return;
    const TokenTopkDesc d = *p.desc;
    const int t = *p.step;
    const int b = blockIdx.x;
    if (t < 0 || t >= d.max_new || b >= d.rows) return;
    const int k = p.k;
    const size_t o = (size_t)b * (size_t)d.ld + (size_t)t;
    int32_t* ids = d.ids + o * (size_t)k;
    float* lps = d.logprobs + o * (size_t)k;
    int32_t* rank = (p.want_rank && d.rank) ? d.rank + o : nullptr;
    if (!p.unfinished[b]) {                                          // finished before this step (block-uniform): what the statistics read there
        if ((int)threadIdx.x < k) { ids[threadIdx.x] = -1; lps[threadIdx.x] = 0.f; }
        if (rank && threadIdx.x == 0) *rank = 0;
        return;
    }
    const float* row = p.src + (size_t)b * p.ld_src;
    const float T = p.do_sample ? p.temperature : 1.0f;
    int tok = -1;
    if (rank) {                                                      // the token, as token_stats_kernel reads it
        if (p.pval) {
            float best = -INFINITY;
            tok = 0x7fffffff;
            for (int s = 0; s < AM_SPLIT; ++s) argmax_pair(best, tok, p.pval[b * AM_SPLIT + s], p.pidx[b * AM_SPLIT + s]);
        } else {
            tok = p.next[b];
        }
        if ((unsigned)tok >= (unsigned)p.V) tok = 0;
    }
    if constexpr (SOURCE == 0) {
        token_topk_raw_row(row, p.V, T, k, tok, red, ids, lps, rank);
        return;
    }
    // source 1: the processed row (token_stats_kernel's functors; greedy: T = 1 and x / 1 = x, the sums and the expression are that kernel's)
    const uint32_t* srow = p.seen ? p.seen + (size_t)b * p.seen_words : nullptr;
    const int eos = t < p.min_new ? p.eos : -1;
    const float pen = p.penalty;
    auto base = [&](int i) { return i == eos ? -INFINITY : rep_penalty(row[i], i, srow, pen); };
    const bool wr = rank != nullptr;
    const float qnan = __uint_as_float(0x7fc00000u);
    float pm, pls, pent;
    int rk = 0, n;
    if (p.do_sample) {
        const float invT = 1.0f / p.temperature;
        WarpStats w = row_warp_stats<false, true>([&](int i) { return base(i) * invT; }, p.V, p.top_k, p.top_p, 1, red);
        w.mthr = wp_minp_thr(w.mx, p.minp_log);
        auto kept = [&](int i) { const float s = base(i); return wp_keep(w, s * invT) ? s : -INFINITY; };      // the key: before the division by T
        ts_row_sums([&](int i) { const float s = base(i); return wp_keep(w, s * invT) ? s / T : -INFINITY; }, p.V, red, pm, pls, pent);
        n = row_topk(kept, p.V, k, [&](float v) { return (v / T - pm) - pls; }, red, wr, wr ? kept(tok) : qnan, &rk);
    } else {
        ts_row_sums(base, p.V, red, pm, pls, pent);
        n = row_topk(base, p.V, k, [&](float v) { return (v - pm) - pls; }, red, wr, wr ? base(tok) : qnan, &rk);
    }
    topk_store(n, k, qnan, wr, rk, ids, lps, rank);
}
void launch_token_topk(const TokenTopkArgs& a, hipStream_t st) {
    if (a.source == 0) token_topk_kernel<0><<<a.B, SP_THREADS, 0, st>>>(a);
    else token_topk_kernel<1><<<a.B, SP_THREADS, 0, st>>>(a);
}
__global__ __launch_bounds__(SP_THREADS) void token_topk_rows_kernel(TokenTopkRowsArgs p) {
    __shared__ float red[SP_THREADS / 64];
    const int b = blockIdx.x;
    int tok = p.tokens ? p.tokens[b] : -1;
    if (tok >= p.V) tok = -1;
    token_topk_raw_row(p.rows + (size_t)b * p.ld, p.V, p.temperature, p.k, tok, red, p.ids + (size_t)b * p.k, p.logprobs + (size_t)b * p.k,
                       p.rank ? p.rank + b : nullptr);
}
void launch_token_topk_rows(const TokenTopkRowsArgs& a, hipStream_t st) {
    token_topk_rows_kernel<<<a.B, SP_THREADS, 0, st>>>(a);
}

__global__ void finish_step_kernel(FinishArgs p) {
    __shared__ int any_unf;
    if (*p.done) return;
    const int b = threadIdx.x;
    const int t = *p.step;
    if (b == 0) any_unf = 0;
    __syncthreads();
    if (b < p.B) {
        int nxt;
        if (p.amax) {                       // greedy, selection folded into the lm_head launch: decode the row's key, re-arm the slot
            unsigned long long* slot = p.amax + (size_t)b * SV_AMAX_STRIDE;
            nxt = sv_amax_index(__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            __hip_atomic_store(slot, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (p.pval) {                // greedy: merge the AM_SPLIT slice winners of this row
            float best = -INFINITY;
            nxt = 0x7fffffff;
            for (int s = 0; s < AM_SPLIT; ++s) argmax_pair(best, nxt, p.pval[b * AM_SPLIT + s], p.pidx[b * AM_SPLIT + s]);
        } else {
            nxt = p.next[b];
        }
        if (finish_step_row(p, b, t, nxt)) atomicOr(&any_unf, 1);
    }
    __syncthreads();
    if (b == 0) finish_step_call(p, t, any_unf);
}
void launch_finish_step(const FinishArgs& a, hipStream_t st) {
    int threads = ((a.B + 63) / 64) * 64;
    finish_step_kernel<<<1, threads, 0, st>>>(a);
}

// ------------------------------------------------------------------------------------------------
// Continuous batching (the reference's worker admits 5 concurrent requests, serve/model_worker.py:
// 216-229, and runs them one HF generate each): every row ("slot") of the decode batch is an independent REQUEST with its
// own sampling parameters, budget, EOS and stop sequence.  One block per slot selects the token (greedy argmax, lowest
// index on ties; or temperature -> top-k -> top-p -> multinomial) and does the slot's bookkeeping -- everything is per row,
// so the reference's row-0 stop (starvector_base.py:9-20: right for ONE request per generate call) becomes each request's
// own stop.  The random stream of a slot depends on (its seed, its own step, row 0): a request produces the same tokens
// as when it runs alone through sv_generate.
// vLLM-mode slots (CbSlot::vllm, vLLM 0.5.5's sampler order) first rewrite their logits row in place -- logit_bias, the min_tokens
// hold of eos and the stop ids, repetition over prompt + output ids, frequency and presence over the output counts -- and then
// take the same selection as an HF slot (greedy argmax, or temperature -> top-k -> top-p -> min_p -> one draw) with the HF
// processors off.  The logits buffer is the engine's own and the next lm_head overwrites it, so the rewrite is safe.
// ------------------------------------------------------------------------------------------------
// LP = "some slot of this launch records log-probs" (CbStepArgs::lp): the record sits between the selection and the bookkeeping.  LP = false is
// the kernel of every batch in which nobody asks -- none of the record's registers, scratch or LDS.
// The row's body -- selection, record, bookkeeping -- is cb_row.h's, shared with cb_lookup_step_kernel (cb_lookup/cb_lookup.hip).
template <bool LP>
__global__ __launch_bounds__(SP_THREADS) void cb_step_kernel(CbStepArgs p) {
    __shared__ float red[SP_THREADS / 64];
    __shared__ float scan[SP_THREADS];
    __shared__ int result;
    __shared__ float am_v[SP_THREADS / 64];
    __shared__ int am_i[SP_THREADS / 64];
    const int b = blockIdx.x;
    // block-uniform by construction: say so, and the slot's fields travel as scalar loads into SGPRs instead of occupying ~30 VGPRs
    // across sample_row (round 3: a by-value copy of the slot, 224 B of scratch per lane; now 80 B, all of it inside the general
    // bisection path of sample_row, which holds 48 scores per thread under the 128-VGPR cap of a 1024-thread block)
    const int s = __builtin_amdgcn_readfirstlane(p.slot_map ? p.slot_map[b] : b);
    const CbSlot& sl = p.slots[s];                                  // a reference: the fields are read where they are used (uniform address)
    if (!sl.live) return;
    const CbRowLds lds = {red, scan, &result, am_v, am_i};
    const uint32_t* srow;
    int tok = cb_row_select<LP>(p, sl, s, p.logits + (size_t)b * p.ld, lds, srow);
    if (threadIdx.x != 0) return;
    bool fin;
    tok = cb_row_commit(p, sl, s, tok, srow, fin);
    p.cur_tok[s] = tok;                                             // the slot's one decode row
    p.positions[s] += 1;
}
void launch_cb_step(const CbStepArgs& a, int nblocks, hipStream_t st) {
    if (a.lp) cb_step_kernel<true><<<nblocks, SP_THREADS, 0, st>>>(a);
    else cb_step_kernel<false><<<nblocks, SP_THREADS, 0, st>>>(a);
}

}  // namespace sv
