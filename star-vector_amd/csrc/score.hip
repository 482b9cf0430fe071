// Per-token log-probabilities of the scoring forward (GRPO's log-prob pass): what a trainer computes from the logits of
// StarVectorForCausalLM.forward -- log_softmax over the vocabulary gathered at the completion ids, the entropy, the arg-max --
// straight from the bf16 rows the lm_head GEMM leaves in its workspace, so that no [rows][vocab] tensor ever reaches the caller.
#include <math.h>
#include "kernels.h"
#include "topk.h"

namespace sv {

#define LP_THREADS 256
#define LP_WAVES (LP_THREADS / 64)

// lowest index wins a tie, NaN never wins (the rule of sampling.hip's argmax_pair)
__device__ __forceinline__ void lp_argmax_pair(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// the log-prob of a column whose bf16 logit is x: ONE expression for logprob_rows_kernel's target and for every slot of topk_rows_bf16_kernel
__device__ __forceinline__ float lp_value(float x, float it, float lse) { return x * it - lse; }

// One block per row, two passes over the row (196 KiB of fp32 would not fit a block's registers; 96 KiB of bf16 comes back out
// of L2 / the last-level cache the second time): (1) maximum + first maximal index, (2) sum exp(x - max) and sum exp(x - max) (x - max).
// 16-byte loads: ld is a multiple of 8 and rows start 16-byte aligned, so the vector that holds column V - 1 lies inside the row;
// its columns >= V are masked.  Every sum runs in a fixed order (a thread's columns ascending into four interleaved accumulators,
// xor butterfly inside a wave, waves in wave order): the same row gives the same bits in any launch, at any row count.
//   x_i = float(logit_i) * inv_t;  lse = max + log(sum exp(x_i - max));  logprob = x_target - lse
//   entropy = lse - sum p_i x_i = log(s) - (sum e_i (x_i - max)) / s     (differences to the maximum: no cancellation at |x| ~ 100;
//                                                                         a term with e_i = 0, x_i = -inf included, adds 0)
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(LogprobArgs p) {
    __shared__ float sh_v[LP_WAVES];
    __shared__ int sh_i[LP_WAVES];
    __shared__ float sh_s[LP_WAVES], sh_u[LP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, V = p.V;
    const bf16_t* row = p.logits + (size_t)r * p.ld;
    const float it = p.inv_t;

    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid * 8; i < V; i += LP_THREADS * 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(row + i);
        float f[8];
        unpack8(u, f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (i + e < V) lp_argmax_pair(best, bi, f[e], i + e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        lp_argmax_pair(best, bi, ov, oi);
    }
    if (lane == 0) { sh_v[wave] = best; sh_i[wave] = bi; }
    __syncthreads();
    best = sh_v[0]; bi = sh_i[0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) lp_argmax_pair(best, bi, sh_v[w], sh_i[w]);

    // no comparable value in the row (all NaN / all -inf): every output NaN, arg-max -1, flag code 2
    if (bi == 0x7fffffff || best == -INFINITY) {
        if (tid == 0) {
            const float qnan = __uint_as_float(0x7fc00000u);
            if (p.logprob) p.logprob[r] = qnan;
            if (p.lse) p.lse[r] = qnan;
            if (p.entropy) p.entropy[r] = qnan;
            if (p.argmax) p.argmax[r] = -1;
            if (p.bad) { atomicOr(p.bad, 2); atomicMin(p.bad + 1, p.row0 + r); }
        }
        return;
    }
    // inv_t > 0: the maximum of x is the maximum logit scaled (the product is monotone)
    const float m = best * it;
    float s4[4] = {0.f, 0.f, 0.f, 0.f}, u4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid * 8; i < V; i += LP_THREADS * 8) {
        const uint4 u = *reinterpret_cast<const uint4*>(row + i);
        float f[8];
        unpack8(u, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (i + e < V) {
                const float d = f[e] * it - m;
                const float ex = expf(d);
                s4[e & 3] += ex;
                u4[e & 3] += ex > 0.f ? ex * d : (ex == 0.f ? 0.f : ex);      // (NaN stays NaN)
            }
        }
    }
    float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    float uu = (u4[0] + u4[1]) + (u4[2] + u4[3]);
    s = wave_sum(s);
    uu = wave_sum(uu);
    if (lane == 0) { sh_s[wave] = s; sh_u[wave] = uu; }
    __syncthreads();
    if (tid != 0) return;
    s = sh_s[0]; uu = sh_u[0];
#pragma unroll
    for (int w = 1; w < LP_WAVES; ++w) { s += sh_s[w]; uu += sh_u[w]; }
    const float ls = logf(s);
    const float lse = m + ls;
    if (p.lse) p.lse[r] = lse;
    if (p.entropy) p.entropy[r] = ls - uu / s;
    if (p.argmax) p.argmax[r] = bi;
    if (p.logprob) {
        const int t = p.targets ? p.targets[r] : -100;
        float lp;
        if (t == -100) lp = 0.f;                                        // HF's ignore index
        else if (t >= 0 && t < V) lp = lp_value(bf2f(row[t]), it, lse);
        else {
            lp = __uint_as_float(0x7fc00000u);
            if (p.bad) { atomicOr(p.bad, 1); atomicMin(p.bad + 1, p.row0 + r); }
        }
        p.logprob[r] = lp;
    }
}

void launch_logprob_rows(const LogprobArgs& a, hipStream_t st) {
    if (a.R < 1) return;
    logprob_rows_kernel<<<dim3((unsigned)a.R), LP_THREADS, 0, st>>>(a);
}

// sv_forward_topk: the k best columns of a row and the rank of its target (TopkRowsArgs, kernels.h; topk.h's row_topk keyed on the bf16 logit itself,
// before the product with inv_t).  The row's lse is the one logprob_rows_kernel left: every slot is that kernel's log-prob of its column.
__global__ __launch_bounds__(WP_THREADS) void topk_rows_bf16_kernel(TopkRowsArgs p) {
    __shared__ float red[WP_THREADS / 64];
    const int r = blockIdx.x, V = p.V, k = p.k;
    const bf16_t* row = p.logits + (size_t)r * p.ld;
    const float it = p.inv_t, lse = p.lse[r];
    const int t = p.targets ? p.targets[r] : -100;
    const bool wr = p.rank != nullptr && t >= 0 && t < V;           // -100 / an id outside the vocabulary: rank 0
    int rk = 0;
    const int n = row_topk([&](int i) { return bf2f(row[i]); }, V, k, [&](float v) { return lp_value(v, it, lse); }, red, wr,
                           wr ? bf2f(row[t]) : __uint_as_float(0x7fc00000u), &rk);
    const RowTopkSmem& sm = row_topk_smem();
    if ((int)threadIdx.x < k) {
        p.ids[(size_t)r * k + threadIdx.x] = sm.id[threadIdx.x];
        p.logprobs[(size_t)r * k + threadIdx.x] = n > 0 ? sm.lp[threadIdx.x] : __uint_as_float(0x7fc00000u);
    }
    if (p.rank && threadIdx.x == 0) p.rank[r] = (wr && n > 0) ? rk : 0;
}
void launch_topk_rows_bf16(const TopkRowsArgs& a, hipStream_t st) {
    if (a.R < 1) return;
    topk_rows_bf16_kernel<<<dim3((unsigned)a.R), WP_THREADS, 0, st>>>(a);
}

}  // namespace sv
