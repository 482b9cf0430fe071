// Prompt-lookup decoding with the selection the call asks for (sv_generate_lookup_sampled; DESIGN.md "Prompt-lookup decoding"): sampling and
// the repetition penalty over the K + 1 rows of a verification step.
//   lookup_sample : every row draws its token with the plain sampler's own code (sample_row.h) and the (seed, step, row) triple the plain call
//                   uses at the row's column; the token goes to lookup_step_kernel as slice 0 of the row's slice winners
//   lookup_seen   : one bitmap of generated ids per sequence, and from it the bitmap of every row of the next step (the sequence's ids plus
//                   the drafts in front of the row), which the selection kernels index by row
// Neither kernel waits for another block: what one launch needs from another it reads behind the launch boundary.
#include "../sample_row.h"

namespace sv {

#define LS_AM_SPLIT 8           // slices per row that lookup_step_kernel merges (lookup.hip LK_AM_SPLIT, sampling.hip AM_SPLIT)
#define LS_SEEN_THREADS 256

// grid rows, block SP_THREADS
__global__ __launch_bounds__(SP_THREADS) void lookup_sample_kernel(LookupSampleArgs p) {
    __shared__ float red[SP_THREADS / 64];
    __shared__ float scan[SP_THREADS];
    __shared__ int result;
    if (p.done && *p.done) return;                                   // block-uniform: a finished call's steps change nothing
    const int r = blockIdx.x, s = r / p.K1, j = r % p.K1;
    const float* row = p.logits + (size_t)r * p.ld;
    const uint32_t* srow = p.seen ? p.seen + (size_t)r * p.seen_words : nullptr;
    const float invT = 1.0f / p.temperature;
    auto lg = [&](int i) { return rep_penalty(row[i], i, srow, p.penalty) * invT; };     // processors, then temperature (sample_top_p_kernel's functor)
    const int tok = sample_row(lg, p.V, p.top_k, p.top_p, -INFINITY, p.seed, (uint32_t)(p.n_emit[s] + j), (uint32_t)s, red, scan, &result);
    if (threadIdx.x < LS_AM_SPLIT) {
        const bool has = threadIdx.x == 0 && (unsigned)tok < (unsigned)p.V;
        p.pval[(size_t)r * LS_AM_SPLIT + threadIdx.x] = has ? 0.f : -INFINITY;
        p.pidx[(size_t)r * LS_AM_SPLIT + threadIdx.x] = has ? tok : 0x7fffffff;
    }
}
void launch_lookup_sample(const LookupSampleArgs& a, hipStream_t st) {
    lookup_sample_kernel<<<a.rows, SP_THREADS, 0, st>>>(a);
}

// grid n_seq, block LS_SEEN_THREADS, dynamic LDS words * 4 bytes: the sequence's bitmap, then row by row with one draft more
__global__ __launch_bounds__(LS_SEEN_THREADS) void lookup_seen_kernel(LookupSeenArgs p) {
    extern __shared__ uint32_t ls_bits[];
    if (p.done && *p.done) return;
    const int tid = threadIdx.x, s = blockIdx.x, W = p.words, K1 = p.K1;
    const unsigned nbits = (unsigned)W * 32u;
    const int L1 = p.n_emit[s], L0 = p.begin ? L1 : p.seq_cols[s];
    uint32_t* seq = p.seq_seen + (size_t)s * W;
    for (int w = tid; w < W; w += LS_SEEN_THREADS) ls_bits[w] = seq[w];
    __syncthreads();
    if (tid == 0)
        for (int c = L0; c < L1; ++c) {
            const int id = p.out_tok[(size_t)s * p.ld_out + c];
            if ((unsigned)id < nbits) ls_bits[id >> 5] |= 1u << (id & 31);
        }
    __syncthreads();
    const int nd = min(max(p.n_draft[s], 0), K1 - 1);
    for (int w = tid; w < W; w += LS_SEEN_THREADS) {
        const uint32_t v = ls_bits[w];
        seq[w] = v;
        p.row_seen[(size_t)(s * K1) * W + w] = v;
        for (int j = nd + 1; j < K1; ++j) p.row_seen[(size_t)(s * K1 + j) * W + w] = v;      // dead rows: row 0's set
    }
    if (tid == 0) p.seq_cols[s] = L1;
    for (int j = 1; j <= nd; ++j) {
        __syncthreads();                                             // row j - 1 has been read
        if (tid == 0) {
            const int id = p.cur_tok[s * K1 + j];
            if ((unsigned)id < nbits) ls_bits[id >> 5] |= 1u << (id & 31);
        }
        __syncthreads();
        for (int w = tid; w < W; w += LS_SEEN_THREADS) p.row_seen[(size_t)(s * K1 + j) * W + w] = ls_bits[w];
    }
}
void launch_lookup_seen(const LookupSeenArgs& a, hipStream_t st) {
    lookup_seen_kernel<<<a.n_seq, LS_SEEN_THREADS, (size_t)a.words * sizeof(uint32_t), st>>>(a);
}

}  // namespace sv
