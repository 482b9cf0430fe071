// Prompt-lookup speculative decoding for greedy generate (sv_generate_lookup; DESIGN.md "Prompt-lookup decoding").
//   lookup_kv_write : per layer, between c_attn and the decode attention: every row's k_new | v_new into its page slot, so that the K + 1
//                     rows of a sequence -- which alias the same pages -- see their siblings' keys through the cache
//   lookup_hold_eos : the min-length hold per row (a row's column is n_emit + j, not the common step index)
//   lookup_begin    : after the prompt pass and the first token: the n_seq x (K + 1) row layout, the counters, the first drafts
//   lookup_step     : one block per sequence behind the lm_head and the slice argmax: accept, emit, EOS / stop / budget, draft the next step
// The arithmetic of lookup_kv_write is attn_decode_kernel's own (attention.hip), restated here because that kernel's text is pinned by hand;
// tests/test_gpu_lookup_ops.py holds the two to the same bits.
#include "../kernels.h"
#include "lk_draft.h"

namespace sv {

// the page layout of attention.hip (kv_k_offset / kv_v_offset)
__device__ __forceinline__ size_t lk_k_offset(int D, int t64, int d) {
    const int kg = t64 >> 4, key = t64 & 15, s = d >> 5, c = (d >> 3) & 3, e = d & 7;
    return ((size_t)((kg * (D >> 5) + s) * 64 + c * 16 + key)) * 16 + e * 2;
}
__device__ __forceinline__ size_t lk_v_offset(int D, int t64, int dv) {
    const int g = t64 >> 5, k32 = t64 & 31, u = k32 >> 4, c = (k32 >> 2) & 3, r = k32 & 3;
    const int e = 4 * u + r, t = dv >> 4, dl = dv & 15;
    return (size_t)64 * D * 2 + ((size_t)((g * (D >> 4) + t) * 64 + c * 16 + dl)) * 16 + e * 2;
}

// grid rows * n_kv, block 2 * head_dim: thread c owns column c of k_new [0, D) | v_new [D, 2 D) of one (row, KV head)
__global__ __launch_bounds__(256) void lookup_kv_write_kernel(LookupKvArgs p) {
    const int D = p.head_dim;
    const int b = blockIdx.x / p.n_kv, kvh = blockIdx.x % p.n_kv;
    const int kc = threadIdx.x;
    if (b >= p.rows || kc >= 2 * D) return;
    const int pos = p.positions[b];
    if (pos < 0 || (pos >> 6) >= p.max_pages) return;            // never index the block table past the row
    const unsigned slab = (unsigned)p.rows_ws * (unsigned)p.ldws;
    const bool is_k = kc < D;
    const int d = kc & (D - 1);
    const unsigned base = (unsigned)(p.H * D + kvh * D) + (is_k ? 0u : (unsigned)(p.n_kv * D));
    // slabs summed in slab order from zero, then the bias, then bf16: slab_sum() of the attention kernel
    auto column = [&](unsigned col) -> bf16_t {
        float a = 0.f;
        for (int sp = 0; sp < p.splitk; ++sp) a += p.ws[(size_t)sp * slab + (size_t)b * p.ldws + col];
        return f2bf(a + bf2f(p.bias[col]));
    };
    bf16_t out = column(base + d);
    if (is_k && p.rope_cos) {
        // rotate_half at `pos`; the products and the sum rounded to bf16 one by one, as the attention kernel rounds them
        const int h = d < D / 2 ? d : d - D / 2;
        const float x1 = bf2f(d < D / 2 ? out : column(base + h));
        const float x2 = bf2f(d < D / 2 ? column(base + h + D / 2) : out);
        const float cs = p.rope_cos[(size_t)pos * (D / 2) + h], sn = p.rope_sin[(size_t)pos * (D / 2) + h];
        out = d < D / 2 ? f2bf(bfround(x1 * cs) + bfround(-x2 * sn)) : f2bf(bfround(x2 * cs) + bfround(x1 * sn));
    }
    char* page = p.pool_layer + (size_t)kvh * p.kv_head_stride + (size_t)p.block_table[(size_t)b * p.max_pages + (pos >> 6)] * kv_page_bytes(D);
    const int t64 = pos & 63;
    *reinterpret_cast<bf16_t*>(page + (is_k ? lk_k_offset(D, t64, d) : lk_v_offset(D, t64, d))) = out;
}
void launch_lookup_kv_write(const LookupKvArgs& a, hipStream_t st) {
    lookup_kv_write_kernel<<<a.rows * a.n_kv, 2 * a.head_dim, 0, st>>>(a);
}

__global__ void lookup_hold_eos_kernel(float* logits, int ld, int eos, const int32_t* __restrict__ n_emit, int K1, int min_new, int rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    if (n_emit[r / K1] + r % K1 < min_new) logits[(size_t)r * ld + eos] = -INFINITY;
}
void launch_lookup_hold_eos(float* logits, int ld, int eos, const int32_t* n_emit, int K1, int min_new, int rows, hipStream_t st) {
    lookup_hold_eos_kernel<<<(rows + 63) / 64, 64, 0, st>>>(logits, ld, eos, n_emit, K1, min_new, rows);
}

#define LK_THREADS 256
#define LK_AM_SPLIT 8           // slices per row of launch_argmax_partial (sampling.hip AM_SPLIT)
// the rule of sampling.hip's argmax_pair: lowest index wins a tie, NaN never wins
__device__ __forceinline__ void lk_argmax_pair(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// The drafts of sequence s behind L generated ids (block-uniform result, the ids in sh_draft): the rule of lk_draft.h, at most K and never
// more than the call's budget leaves room to emit (a step emits its accepted drafts and one token more).
__device__ int lk_draft(const LookupArgs& p, int s, int L, int* sh_red, int* sh_draft) {
    return lk_draft_ids<LK_THREADS>(p.out_tok + (size_t)s * p.ld_out, L, min(p.K, p.max_new - L - 1), p.max_ngram, p.min_ngram,
                                    p.forced ? p.forced + (size_t)s * p.forced_ld : nullptr, p.forced_ld, sh_red, sh_draft);
}
// the next step's rows of sequence s: row 0 = the last emitted id at its position, rows 1 .. nd the drafts behind it, the rest exact copies of row 0
__device__ void lk_write_rows(const LookupArgs& p, int s, int last, int pos0, int nd, const int* sh_draft) {
    const int K1 = p.K + 1;
    for (int j = threadIdx.x; j < K1; j += LK_THREADS) {
        const bool live = j >= 1 && j <= nd;
        p.cur_tok[s * K1 + j] = live ? sh_draft[j - 1] : last;
        p.positions[s * K1 + j] = pos0 + (live ? j : 0);
    }
    if (threadIdx.x == 0) p.n_draft[s] = nd;
}
// row 0's stop sequence ends at column L - 1?  (finish_step_call's test)
__device__ __forceinline__ bool lk_stop_at(const LookupArgs& p, int L) {
    if (p.n_stop <= 0 || L < p.n_stop) return false;
    for (int i = 0; i < p.n_stop; ++i)
        if (p.out_tok[L - p.n_stop + i] != p.stop_ids[i]) return false;
    return true;
}
// A sequence that has finished in front of its budget: pad ids up to the budget (what the bookkeeping of the plain call writes step by step).  Row 0's
// stop sequence is looked for in those columns too -- the plain call tests row 0 at every step, finished or not.
__device__ void lk_finish_pad(const LookupArgs& p, int s, int L, bool stopped) {
    for (int c = L + (int)threadIdx.x; c < p.max_new; c += LK_THREADS) p.out_tok[(size_t)s * p.ld_out + c] = p.pad;
    if (s != 0 || p.n_stop <= 0 || stopped) return;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int c = L + 1; c <= p.max_new; ++c)
            if (lk_stop_at(p, c)) { atomicMin(p.limit, c); break; }
}

// one block: the rows the first token's bookkeeping left (row s = sequence s) -> the row layout; the sequences are read before any row is written
__global__ __launch_bounds__(LK_THREADS) void lookup_begin_kernel(LookupArgs p) {
    __shared__ int tk[64], ps[64], uf[64], sh_red[LK_THREADS / 64], sh_draft[LK_MAXK1];
    const int tid = threadIdx.x;
    if (tid < p.n_seq) { tk[tid] = p.cur_tok[tid]; ps[tid] = p.positions[tid]; uf[tid] = p.unfinished[tid]; }
    if (tid == 0) { p.counts[0] = 0; p.counts[1] = 0; p.counts[2] = 0; *p.limit = p.max_new; *p.ticket = 0u; }
    __syncthreads();
    for (int s = 0; s < p.n_seq; ++s) {
        const bool f = !uf[s] || p.max_new <= 1;
        if (tid == 0) { p.n_emit[s] = 1; p.fin[s] = f ? 1 : 0; p.base[s] = ps[s]; }
        if (f) lk_finish_pad(p, s, 1, false);
        const int nd = f ? 0 : lk_draft(p, s, 1, sh_red, sh_draft);
        lk_write_rows(p, s, tk[s], ps[s], nd, sh_draft);
        __syncthreads();
    }
}
void launch_lookup_begin(const LookupArgs& a, hipStream_t st) { lookup_begin_kernel<<<1, LK_THREADS, 0, st>>>(a); }

// grid n_seq.  Row j of the sequence chose t_j (the merge of its slice winners, as finish_step_kernel merges them).  Accepted: the longest
// prefix of the drafts with d_i == t_{i-1}; emitted: t_0 .. t_a at the sequence's own column, each through the EOS / budget / row-0 stop tests
// of the plain bookkeeping -- an EOS or a completed stop sequence inside the run ends it there.  The last block of the grid (an arrival
// ticket) takes the call's part: the step count, and the end of the call once every sequence has finished or reached the stop's column limit.
__global__ __launch_bounds__(LK_THREADS) void lookup_step_kernel(LookupArgs p) {
    __shared__ int t_sh[LK_MAXK1], sh_red[LK_THREADS / 64], sh_draft[LK_MAXK1], info[4];
    if (*p.done) return;                            // a finished call: the wasted steps of a polling chunk change nothing
    const int tid = threadIdx.x, s = blockIdx.x, K1 = p.K + 1;
    const int L0 = p.n_emit[s];
    // (row 0 counts as finished once its stop sequence has fired; the other sequences run on until they finish or the call ends, whatever the
    //  limit says meanwhile: no block reads what another block of the same launch writes, so the state is the same from run to run)
    const bool active = !p.fin[s];
    if (active) {
        if (tid < K1) {
            const int r = s * K1 + tid;
            float best = -INFINITY;
            int nxt = 0x7fffffff;
            for (int i = 0; i < LK_AM_SPLIT; ++i) lk_argmax_pair(best, nxt, p.pval[r * LK_AM_SPLIT + i], p.pidx[r * LK_AM_SPLIT + i]);
            if ((unsigned)nxt >= (unsigned)p.V) {   // no finite logit in this row: never index the embedding table with it
                nxt = 0;
                if (p.bad) atomicCAS(p.bad, 0, 1);
            }
            t_sh[tid] = nxt;
        }
        __syncthreads();
        if (tid == 0) {
            const int nd = p.n_draft[s];
            int a = 0;
            while (a < nd && p.cur_tok[s * K1 + a + 1] == t_sh[a]) ++a;
            int L = L0, f = 0, stopped = 0;
            for (int i = 0; i <= a && !f && !stopped; ++i) {
                const int tok = t_sh[i];
                p.out_tok[(size_t)s * p.ld_out + L] = tok;
                ++L;
                if (tok == p.eos || L >= p.max_new) f = 1;
                if (s == 0 && lk_stop_at(p, L)) { atomicMin(p.limit, L); stopped = 1; f = 1; }
            }
            p.n_emit[s] = L; p.fin[s] = f;
            atomicAdd(p.counts + 1, nd);
            atomicAdd(p.counts + 2, L - L0 - 1);
            info[0] = L; info[1] = f; info[2] = stopped; info[3] = p.out_tok[(size_t)s * p.ld_out + L - 1];
        }
        __syncthreads();
        const int L = info[0];
        const bool f = info[1] != 0, stopped = info[2] != 0;
        if (f) lk_finish_pad(p, s, L, stopped);
        const int nd = f ? 0 : lk_draft(p, s, L, sh_red, sh_draft);
        lk_write_rows(p, s, info[3], p.base[s] + L - 1, nd, sh_draft);
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const unsigned t = atomicAdd(p.ticket, 1u);
        if (t == (unsigned)p.n_seq - 1u) {          // every sequence's part is in memory
            __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();
            const int lim = __hip_atomic_load(p.limit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int all = 1, mx = 0;
            for (int q = 0; q < p.n_seq; ++q) {
                const int Lq = __hip_atomic_load(p.n_emit + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int fq = __hip_atomic_load(p.fin + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!(fq || Lq >= lim)) all = 0;
                mx = max(mx, Lq);
            }
            p.counts[0] += 1;
            if (all) { *p.n_emitted = min(lim, mx); *p.done = 1; }
        }
    }
}
void launch_lookup_step(const LookupArgs& a, hipStream_t st) { lookup_step_kernel<<<a.n_seq, LK_THREADS, 0, st>>>(a); }

}  // namespace sv
