// HF logits processors that BAN tokens, on device (transformers 4.49 generation/logits_process.py):
//   NoRepeatNGramLogitsProcessor(n)   at step t the ids { g[j + n - 1] : 0 <= j <= t - n, g[j .. j + n - 2] == g[t - n + 1 .. t - 1] } -- every id that
//                                     would complete an n-gram the row has already generated; nothing while t < n - 1; n = 1: every earlier id
//   NoBadWordsLogitsProcessor         a sequence of one id: always; a sequence of L > 1 ids: its last id when t >= L and the row's last L - 1 ids
//                                     are the sequence's first L - 1 (HF skips a sequence that is "longer than the context", L > t: with exactly
//                                     L - 1 ids generated nothing is banned yet, whatever they are)
// g[0 .. t - 1] = the ids the row has generated so far (with inputs_embeds HF's input_ids start empty; a finished row keeps receiving pads, and
// they count).  The banned scores become -inf in the row's fp32 logits, in place: the launch sits between the lm_head and the selection
// (engine_generate.hip, sample_and_finish), so the selection, the score capture and every other processor see the banned row.
//
// One block per row.  The n - 1 ids every window is compared with and the step are block-uniform: they are read once and kept in scalar
// registers; the threads stride the history, one dword load per id.  Several threads may ban the same id: they store the same -inf with
// plain stores, in any order.  The history is at most max_seq_len ids per row -- a few microseconds next to a decode step's milliseconds --
// so the kernel is not tuned beyond that.
#include "kernels.h"

namespace sv {

#define BAN_THREADS 256

__global__ __launch_bounds__(BAN_THREADS) void ban_tokens_kernel(BanArgs p) {
    if (p.done && *p.done) return;
    const int b = blockIdx.x;
    const int t = __builtin_amdgcn_readfirstlane(p.hist_len ? p.hist_len[b] : *p.step);
    if (t < 0 || t > p.ld_hist) return;                              // never a history index outside the row
    const int tid = threadIdx.x;
    float* row = p.logits + (size_t)b * p.ld;
    const int32_t* g = p.hist + (size_t)b * p.ld_hist;
    const unsigned V = (unsigned)p.V;

    const int n = p.ngram;
    if (n >= 1 && n <= SV_BAN_MAXNGRAM && t >= n - 1) {
        int suf[SV_BAN_MAXNGRAM - 1];                                 // g[t - n + 1 .. t - 1], block-uniform
#pragma unroll
        for (int k = 0; k < SV_BAN_MAXNGRAM - 1; ++k) suf[k] = k < n - 1 ? __builtin_amdgcn_readfirstlane(g[t - (n - 1) + k]) : 0;
        for (int j = tid; j <= t - n; j += BAN_THREADS) {             // window g[j .. j + n - 2]; the id behind it: g[j + n - 1], j + n - 1 <= t - 1
            bool same = true;
#pragma unroll
            for (int k = 0; k < SV_BAN_MAXNGRAM - 1; ++k)
                if (k < n - 1) same = same && g[j + k] == suf[k];
            if (same) {
                const unsigned id = (unsigned)g[j + n - 1];
                if (id < V) row[id] = -INFINITY;
            }
        }
    }

    if (tid < p.n_words) {                                           // one thread per bad-word sequence (at most SV_BAN_MAXWORDS of them)
        const BanWord* w = p.words + tid;
        const int L = w->len;
        if (L >= 1 && L <= SV_BAN_MAXLEN && (L == 1 || t >= L)) {
            bool same = true;
            for (int k = 0; k < L - 1; ++k) same = same && g[t - (L - 1) + k] == w->id[k];
            const unsigned id = (unsigned)w->id[L - 1];
            if (same && id < V) row[id] = -INFINITY;
        }
    }
}

void launch_ban_tokens(const BanArgs& a, hipStream_t st) {
    ban_tokens_kernel<<<a.B, BAN_THREADS, 0, st>>>(a);
}

}  // namespace sv
