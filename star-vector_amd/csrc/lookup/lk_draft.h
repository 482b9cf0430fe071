// The n-gram draft of prompt-lookup decoding, shared by lookup.hip (sv_generate_lookup: one block of LK_THREADS per sequence) and
// cb_lookup/cb_lookup.hip (the continuous batch: one block of SP_THREADS per slot).  NT = threads of the calling block, all of which call.
#pragma once
#include "../kernels.h"

namespace sv {

#define LK_MAXK1 16
// block-wide maximum of one int per thread (every thread gets it); sh holds NT / 64 ints
template <int NT>
__device__ __forceinline__ int lk_block_max_n(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    __syncthreads();                                             // sh may still be read from the round before
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
    for (int w = 1; w < NT / 64; ++w) v = max(v, sh[w]);
    return v;
}
// The drafts behind the L ids hist[0, L) (block-uniform result, the ids in sh_draft), at most K of them -- the caller has cut K to what its
// budget leaves room to emit (a step emits its accepted drafts and one token more).  For n = max_ngram .. min_ngram the LATEST earlier
// occurrence of the last n ids whose continuation is not empty -- the largest i with hist[i, i + n) == hist[L - n, L) and i + n < L --
// gives hist[i + n, ...), cut at L.  Threads stride over i; a block max-reduce picks the largest.
// forced != nullptr (the test surface): draft j is forced[L + j] instead, as far as forced_ld reaches.
template <int NT>
__device__ __forceinline__ int lk_draft_ids(const int32_t* hist, int L, int K, int max_ngram, int min_ngram, const int32_t* forced, int forced_ld,
                                            int* sh_red, int* sh_draft) {
    const int tid = threadIdx.x;
    if (K <= 0) return 0;
    if (forced) {
        const int nd = max(0, min(K, forced_ld - L));
        if (tid < nd) sh_draft[tid] = forced[L + tid];
        __syncthreads();
        return nd;
    }
    for (int n = max_ngram; n >= min_ngram; --n) {
        if (L <= n) continue;
        int best = -1;
        for (int i = tid; i + n < L; i += NT) {
            bool m = true;
            for (int k = 0; k < n; ++k) m = m && hist[i + k] == hist[L - n + k];
            if (m) best = i;
        }
        best = lk_block_max_n<NT>(best, sh_red);
        if (best >= 0) {
            const int start = best + n, nd = min(K, L - start);
            if (tid < nd) sh_draft[tid] = hist[start + tid];
            __syncthreads();
            return nd;
        }
    }
    return 0;
}

}  // namespace sv
