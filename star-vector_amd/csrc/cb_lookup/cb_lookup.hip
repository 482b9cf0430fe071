// Prompt-lookup drafting in the continuous batch (sv_cb_set_lookup; DESIGN.md "Prompt-lookup decoding", kernels.h CbLookupArgs).
//   cb_lookup_step : one block per slot behind the lm_head of a verification step (or behind the prompt pass: the `first` form).  The slot's
//                    K + 1 logits rows are verified one after the other with the plain step's own row body (cb_row.h) against the slot's
//                    CURRENT state; then the block drafts from the ids the slot has emitted (lookup/lk_draft.h) and writes the next step's rows.
// Exact by construction: row j is looked at only after rows 0 .. j - 1 have been committed and only if its draft is the token row j - 1
// emitted, so it is selected with the step counter, repetition set, counts, hold and sampler triple the plain batch has at that column.
// A block reads nothing another block of the launch writes; between a commit by thread 0 and the next row's block-wide reads: fence, barrier.
#include "../cb_row.h"
#include "../lookup/lk_draft.h"

namespace sv {

template <bool LP>
__global__ __launch_bounds__(SP_THREADS) void cb_lookup_step_kernel(CbLookupArgs q) {
    __shared__ float red[SP_THREADS / 64];
    __shared__ float scan[SP_THREADS];
    __shared__ int result;
    __shared__ float am_v[SP_THREADS / 64];
    __shared__ int am_i[SP_THREADS / 64];
    __shared__ int sh_red[SP_THREADS / 64], sh_draft[LK_MAXK1], info[3];
    const CbStepArgs& p = q.st;
    const int b = blockIdx.x, tid = threadIdx.x, K1 = q.K + 1;
    const int s = __builtin_amdgcn_readfirstlane(p.slot_map ? p.slot_map[b] : b);
    const CbSlot& sl = p.slots[s];
    if (!sl.live) return;                                           // a dead slot: its rows, history and counters stay as they are
    const CbRowLds lds = {red, scan, &result, am_v, am_i};
    const int nd = q.first ? 0 : max(0, min(q.n_draft[s], q.K));
    const int L0 = sl.step;
    int tok, L;
    bool fin;
    for (int j = 0;; ++j) {
        const float* row = p.logits + (size_t)(q.first ? b : s * K1 + j) * p.ld;
        const uint32_t* srow;
        const int sel = cb_row_select<LP>(p, sl, s, row, lds, srow);
        if (tid == 0) {
            bool f;
            info[0] = cb_row_commit(p, sl, s, sel, srow, f);
            info[1] = f ? 1 : 0;
            info[2] = L0 + j + 1;
        }
        __threadfence();
        __syncthreads();                                            // the commit is in memory before any thread reads the slot's state again
        tok = info[0]; fin = info[1] != 0; L = info[2];
        if (fin || j >= nd || p.cur_tok[s * K1 + j + 1] != tok) break;      // block-uniform
    }
    // the next step: drafts behind the L ids of the slot, never more than its own budget leaves room to emit
    int ndn = 0;
    if (!fin) {
        const bool forced = q.forced && s < q.forced_n;
        ndn = lk_draft_ids<SP_THREADS>(p.out_tokens + (size_t)s * p.ld_out, L, min(q.K, sl.budget - L - 1), q.max_ngram, q.min_ngram,
                                       forced ? q.forced + (size_t)s * q.forced_ld : nullptr, q.forced_ld, sh_red, sh_draft);
    }
    const int pos0 = sl.base + L - 1;
    if (tid < K1) {                                                 // lk_write_rows' layout
        const bool live = tid >= 1 && tid <= ndn;
        p.cur_tok[s * K1 + tid] = live ? sh_draft[tid - 1] : tok;
        p.positions[s * K1 + tid] = pos0 + (live ? tid : 0);
    }
    if (tid == 0) {
        q.n_draft[s] = ndn;
        int32_t* c = q.counts + 3 * s;
        if (q.first) {
            c[0] = 0; c[1] = 0; c[2] = 0;
        } else {
            c[0] += 1; c[1] += nd; c[2] += L - L0 - 1;
            atomicAdd(q.totals, 1);
            if (nd) atomicAdd(q.totals + 1, nd);
            if (L - L0 - 1) atomicAdd(q.totals + 2, L - L0 - 1);
        }
    }
}
void launch_cb_lookup_step(const CbLookupArgs& a, int nblocks, hipStream_t st) {
    if (a.st.lp) cb_lookup_step_kernel<true><<<nblocks, SP_THREADS, 0, st>>>(a);
    else cb_lookup_step_kernel<false><<<nblocks, SP_THREADS, 0, st>>>(a);
}

}  // namespace sv
