// The k best columns of one row, ordered, and the rank of one of its columns: the list behind sv_generate_topk (sampling.hip, fp32 rows of the
// decode step) and sv_forward_topk (score.hip, bf16 rows of the scoring pass).  One 1024-thread block per row; a row's result depends on nothing
// but that row (fixed orders everywhere: the same row gives the same bits alone, among 64 rows, in any launch).
//
//   order   descending by x(i), equal values by ascending column: the rule of argmax_pair, slot 0 is what greedy selection picks.  The key is
//           x(i) itself -- the value BEFORE any division by the temperature -- so rounding after the division can never reorder or merge entries.
//           -0.0 and +0.0 are one value.  In code: a column's key is the pair (wp_key(x), column); no two columns have the same pair, so "the k
//           best" and their order are a property of the row, not of the order in which threads arrive anywhere.
//   enters  NaN never, -inf never (+inf does).  Fewer than k such columns: the tail slots hold id -1 and log-prob -inf.
//   rank    1 + #{ i : x(i) > x_tok }, NaN compares false (vLLM's definition); 0 when x_tok is NaN or the caller has no token.
//   values  slot j holds lp(x(id)) of its column -- the column's own value read again, not the value rebuilt from the key (-0.0 stays -0.0) --
//           `lp` being the caller's own expression for the log-prob of a column: the slot of the emitted / target column is then the caller's
//           log-prob bit for bit.
//
// Method (the sampler's, sampling.hip::sample_row_topk): thread t owns the columns t, t + 1024, ... (coalesced sweeps).
//   1. one sweep: every thread's largest value key m_t; the columns above x_tok are counted in the same sweep
//   2. T0 = the k-th largest of the 1024 m_t (8-bit MSB-first radix select): k threads hold a column >= T0, so the row's k-th best is >= T0
//   3. a second sweep compacts the columns with key >= T0 into LDS, thread order (block scan of the per-thread counts) -- ~k of them
//   4. candidate c's slot = #{ candidates that beat it } under the pair order; slots < k are written.  One read of n pairs per candidate.
// A row outside that scope -- more than TKR_CAP candidates (a plateau across T0 wider than the cap) or more than TKR_PER in one thread -- takes k
// rounds of block arg-max under the same pair order ("the largest pair below the previous one"): same list, one sweep per slot.
#pragma once
#include "kernels.h"
#include "warp.h"

namespace sv {

#define TKR_CAP 2048
#define TKR_PER 4

struct RowTopkSmem {
    uint32_t key[TKR_CAP];
    int idx[TKR_CAP];
    int hist[256];
    int wtot[WP_THREADS / 64];
    uint32_t wkey[WP_THREADS / 64];
    int widx[WP_THREADS / 64];
    uint32_t sel_key;
    int sel_need;
    int id[SV_TOPK_MAX_DEV];              // the result: column of slot j (-1: none) ...
    float lp[SV_TOPK_MAX_DEV];            // ... and its log-prob (-inf: none)
};
__device__ __forceinline__ RowTopkSmem& row_topk_smem() {
    __shared__ RowTopkSmem s;
    return s;
}

// 0 = "never enters" (NaN, -inf); every value that enters has a key > 0x007fffff.  x + 0.0f: -0.0 -> +0.0
__device__ __forceinline__ uint32_t tkr_key(float x) { return x > -INFINITY ? wp_key(x + 0.0f) : 0u; }
// pair order: does (ka, ia) come before (kb, ib) in the list?
__device__ __forceinline__ bool tkr_before(uint32_t ka, int ia, uint32_t kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// Called by every thread of a 1024-thread block (block-uniform arguments).  x(i): column i of the row, i in [0, V).  1 <= k <= SV_TOPK_MAX_DEV.
// lp(v): the log-prob of a column whose value is v.  want_rank: count the columns with x(i) > x_tok into *rank (0 when x_tok is NaN).
// Returns n_found = min(k, columns that enter); row_topk_smem().id / .lp hold the k slots (valid for every thread after the return: the function
// ends on a barrier).  red: >= 16 words of LDS.
template <class F, class L>
__device__ int row_topk(F x, int V, int k, L lp, float* red, bool want_rank, float x_tok, int* rank) {
    RowTopkSmem& sm = row_topk_smem();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int UNR = 8;
    __syncthreads();                                                  // a caller may loop over rows: the previous list has been read
    if (tid < SV_TOPK_MAX_DEV) { sm.id[tid] = -1; sm.lp[tid] = -INFINITY; }

    // ---- 1. thread maxima (value keys), the rank count ----
    uint32_t mkey = 0u;
    float above = 0.f;
    for (int i0 = tid; i0 < V; i0 += UNR * WP_THREADS) {
        float v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i = i0 + u * WP_THREADS;
            v[u] = i < V ? x(i) : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const uint32_t kk = tkr_key(v[u]);
            mkey = kk > mkey ? kk : mkey;
            above += v[u] > x_tok ? 1.f : 0.f;
        }
    }
    if (want_rank) {
        above = wp_block_sum(above, red);                             // exact: counts < 2^24
        if (rank) *rank = x_tok == x_tok ? 1 + (int)above : 0;
    }

    // ---- 2. T0 = the k-th largest thread maximum (0 when fewer than k threads hold a column that enters) ----
    uint32_t prefix = 0u;
    int need = k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) sm.hist[tid] = 0;
        __syncthreads();
        if (pass == 0 || (mkey >> (shift + 8)) == prefix) atomicAdd(&sm.hist[(mkey >> shift) & 255u], 1);      // (a histogram: counts, no order)
        __syncthreads();
        if (tid < 64) {                                               // lane l owns bins 255 - 4l .. 252 - 4l (descending keys)
            const int b0 = 255 - 4 * tid;
            const int h0 = sm.hist[b0], h1 = sm.hist[b0 - 1], h2 = sm.hist[b0 - 2], h3 = sm.hist[b0 - 3];
            const int sum4 = h0 + h1 + h2 + h3;
            int inc = sum4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (tid >= o) inc += t;
            }
            int ab = inc - sum4;                                      // keys in the bins above this lane's four
            if (ab < need && need <= inc) {
                int d = b0;
                if (need > ab + h0) {
                    ab += h0; d = b0 - 1;
                    if (need > ab + h1) {
                        ab += h1; d = b0 - 2;
                        if (need > ab + h2) { ab += h2; d = b0 - 3; }
                    }
                }
                sm.sel_key = (prefix << 8) | (uint32_t)d;
                sm.sel_need = need - ab;
            }
        }
        __syncthreads();
        prefix = sm.sel_key;                                          // (1024 keys, 1 <= need <= 1024: some lane always writes)
        need = sm.sel_need;
    }
    const uint32_t t0 = prefix > 1u ? prefix : 1u;                    // key 0 never enters

    // ---- 3. the columns with key >= T0 into LDS, thread order ----
    uint32_t ck[TKR_PER];
    int ci[TKR_PER];
    int cnt = 0;
    for (int i0 = tid; i0 < V; i0 += UNR * WP_THREADS) {
        uint32_t kk[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i = i0 + u * WP_THREADS;
            kk[u] = i < V ? tkr_key(x(i)) : 0u;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (kk[u] >= t0) {
#pragma unroll
                for (int q = 0; q < TKR_PER; ++q)
                    if (cnt == q) { ck[q] = kk[u]; ci[q] = i0 + u * WP_THREADS; }
                ++cnt;
            }
        }
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sm.wtot[wave] = inc;
    const float over = wp_block_max(cnt > TKR_PER ? 1.f : 0.f, red);  // (syncs inside: wtot and the cleared list are visible after it)
    int off = inc - cnt, n = 0;
#pragma unroll
    for (int w = 0; w < WP_THREADS / 64; ++w) {
        const int t = sm.wtot[w];
        off += w < wave ? t : 0;
        n += t;
    }

    if (over > 0.f || n > TKR_CAP) {                                  // block-uniform
        // ---- k rounds of block arg-max: slot j = the best pair that comes after slot j - 1 ----
        uint32_t pk = 0xffffffffu;
        int pi = -1;
        int found = 0;
        for (int j = 0; j < k; ++j) {
            uint32_t bk = 0u;
            int bi = 0x7fffffff;
            for (int i = tid; i < V; i += WP_THREADS) {
                const uint32_t kk = tkr_key(x(i));
                if (kk != 0u && tkr_before(pk, pi, kk, i) && tkr_before(kk, i, bk, bi)) { bk = kk; bi = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t ok = __shfl_xor(bk, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (tkr_before(ok, oi, bk, bi)) { bk = ok; bi = oi; }
            }
            __syncthreads();
            if (lane == 0) { sm.wkey[wave] = bk; sm.widx[wave] = bi; }
            __syncthreads();
            bk = sm.wkey[0]; bi = sm.widx[0];
#pragma unroll
            for (int w = 1; w < WP_THREADS / 64; ++w)
                if (tkr_before(sm.wkey[w], sm.widx[w], bk, bi)) { bk = sm.wkey[w]; bi = sm.widx[w]; }
            if (bk == 0u) break;                                      // block-uniform: nothing is left
            if (tid == 0) { sm.id[j] = bi; sm.lp[j] = lp(x(bi)); }
            pk = bk; pi = bi;
            ++found;
        }
        __syncthreads();
        return found;
    }

#pragma unroll
    for (int q = 0; q < TKR_PER; ++q)
        if (q < cnt) { sm.key[off + q] = ck[q]; sm.idx[off + q] = ci[q]; }
    __syncthreads();

    // ---- 4. slot of candidate c = the candidates in front of it ----
    for (int c = tid; c < n; c += WP_THREADS) {
        const uint32_t kc = sm.key[c];
        const int ic = sm.idx[c];
        int front = 0;
        for (int j = 0; j < n; ++j) front += tkr_before(sm.key[j], sm.idx[j], kc, ic) ? 1 : 0;
        if (front < k) { sm.id[front] = ic; sm.lp[front] = lp(x(ic)); }             // distinct pairs: one writer per slot
    }
    __syncthreads();
    return n < k ? n : k;
}

}  // namespace sv
