// The MLP half of a decode layer as one launch: mlp_fused_kernel, its design note and launch_mlp_fused.  The stream
// helpers it shares with the two kernels it replaces (gemm.hip) are in skinny_dev.h.
#include <cstddef>
#include "skinny_dev.h"

namespace sv {

// ------------------------------------------------------------------------------------------------
// mlp_fused_kernel: the MLP half of a decode layer (gpt_bigcode/modeling_gpt_bigcode.py:645-660: c_fc -> GELU-tanh -> c_proj) as ONE
// launch of F/32 co-resident blocks (256 for StarVector-1B, one 8-wave block per CU), instead of gemm_skinny_kernel<8, true> (folded
// c_fc) and gemm_skinny_kernel<8, false> (down projection, split-K slabs) with a kernel boundary between them.  Round 4; on for an
// engine that owns its GPU (sv_config.exclusive_device), SV_EXP_MLP_FUSED_FORCE / SV_EXP_MLP_FUSED_OFF = forced on / off.  Measured in process on one MI355X,
// BASELINE config 2: 1079 vs 1111 us per decode step, tokens bit-identical (every version's A/B and wall-clock
// trace: profiles/mlp_fused_r04_ab.log).
//
//   Why it pays (MI355X_MICROARCH.md price list: boundary, prefetch-credit): both GEMMs are pure weight streams (2 x 33.5 MB) and the
//   WEIGHTS of the second one depend on nothing.  Two launches pay a boundary (1.7-1.9 us) plus the second kernel's cold start; here a
//   wave requests the first half of its share of the down projection's weights as soon as its c_fc loop has issued its last MFMA, so
//   HBM keeps streaming under the c_fc reduction, epilogue and publish.
//
//   Phase 1  block L = (xcd = L & 7, i = L >> 3): c_fc tile nt1 = split * (T1 / S) + (xcd / S) * (T1 / 8) + i with split = xcd % S --
//            the 32 GELU output columns of a tile are 2 KiB contiguous in fragment order; they go LDS -> 16-byte sc1 (write-through)
//            stores.  No flag, no counter, nothing to drain.
//   Phase 2  the same block owns (tile nt2 = (xcd / S) * (T1 / 8) + i, K slice `split`) of the down projection = exactly the
//            (tile, slice) the XCD-aware assignment of the slab kernel gives block L.  Wave w needs the c_fc columns of its 16 k-steps
//            = the tiles of 8 producer blocks; it reads them with sc1 loads (L1 bypass) and recognises "not written yet" by the data
//            itself: the launch in front fills the buffer with the bf16 pair 0xFFFF'FFFF (two NaNs -- never a finite GELU output), a
//            k-step that still shows the pattern is re-requested after an s_sleep, BOUNDED (a give-up code in *err, never a hang).
//   What the traces taught (all of it in profiles/mlp_fused_r04_ab.log):
//            * one arrival counter per K slice (64 arrivals + 64 pollers per word): 25.5 us per launch against 17.8 for two launches;
//              one flag word per producer: 17.7 us (the publish store drained behind 24 MB of weight prefetch); in-band pattern: 14.9;
//              + the first half of the weights requested before the reduction: 13.8 us -- this version.
//            * a CU's miss queue takes ~64 KiB: a wave that requests more BLOCKS AT ISSUE until the queue drains, and a wave's loads
//              return IN ORDER -- a poll queued behind 16 KiB of its own weight requests completes after them.  Requesting all 16 KiB
//              at once, moving the reduction to two "critical-path" waves, and the attention output projection as a phase 0 in front
//              (a residual-stream ping-pong, 4 launches per layer) were all built, bit-identical, and slower or equal: removed.
//              Round 5 BUILT the loader wave (a ninth wave per block streams the block's W2 share into LDS with global_load_lds, the
//              consumers request nothing but polls after the publish): bit-identical, +2.0 ... +2.5 us per layer for every start
//              trigger / depth tried -- polls issued at the publish find the pattern and every failed poll is a ~2 us round trip beside
//              the CU's own fill stream; this form's polls ride behind the second half of the weights and arrive when the data is there.
//              What is left over the 12.2 us that 67 MB + the phase-2 tail take is ~1 us.  profiles/mlp_fused_r05_loader_ab.log; removed.
//   Results  per-wave k ranges, MFMA order, cross-wave reduction order, fold statistics and epilogues are those of the two kernels it
//            replaces: bit-identical slabs (tests/test_gpu_e2e.py::test_fused_mlp_launch_equals_the_two_launches_bit_for_bit).
//   Safety   needs all F/32 blocks resident at once (one per CU): enabled only when #CUs >= F/32 AND the engine owns the device -- two
//            processes decoding on one GPU could each hold part of the CUs and wait for blocks that cannot be scheduled (then both
//            give up after the bounded spin and the call fails: never a hang, never wrong tokens).  The pattern is written by the
//            kernel in front (gemm_cols_resid_kernel, ColsArgs::poison), never by this launch; a NaN pair with the pattern (corrupted
//            inputs only: arithmetic NaNs are 0x7FC0) ends in the give-up code, i.e. an error from sv_generate.
// ------------------------------------------------------------------------------------------------
struct MlpFusedKernarg { const bf16_t* W1; const bf16_t* x1; const bf16_t* W2; int KS1; int KS2; int S; MlpFusedArgs p; };
// amdgpu_waves_per_eu(2, 2): one 8-wave block per CU is the design point (2 waves per SIMD, 256 VGPRs each); without it the
// scheduler trades registers for a third wave that can never exist and serialises phase 2's 16 activation loads 3 at a time
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mlp_fused_kernel(const bf16_t* W1_, const bf16_t* x1_, const bf16_t* W2_, int KS1_, int KS2_, int S_,
                                                        MlpFusedArgs p_unused) {
    constexpr int WAVES = 8, CH = 4, NB = 2, RPW = 2, KPW = 16;          // k-steps per wave in BOTH phases (host-checked)
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    float (*red)[16][64] = reinterpret_cast<float (*)[16][64]>(sk_smem);          // [WAVES][16][64]
    float2* fst_s = reinterpret_cast<float2*>(sk_smem + (size_t)WAVES * 16 * 64 * 4);      // [WAVES][32] partial row statistics
    bf16_t* tile_s = reinterpret_cast<bf16_t*>(sk_smem + (size_t)WAVES * 16 * 64 * 4 + (size_t)WAVES * 32 * 8);   // 2 KiB: the c_fc tile
    int* flag_s = reinterpret_cast<int*>(tile_s + 1024);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 31, half = lane >> 5;
    const int L = blockIdx.x, xcd = L & 7, ii = L >> 3;
    const int T1 = gridDim.x, tpg = T1 >> 3;
    const int split = xcd % S_, grp = xcd / S_;
    const int nt2 = grp * tpg + ii;
    const int nt1 = split * (T1 / S_) + nt2;
    const long long t_start = wall_clock64();             // 100 MHz; only stored when the trace buffer is on (tools/mlp_trace.py)

    // ---- phase 1: folded c_fc, tile nt1 over the whole K1 (gemm_skinny_kernel<8, true>, long-range path) ----
    const int ks0 = wave * KPW;
    const u32x4* wptr = reinterpret_cast<const u32x4*>(W1_) + ((size_t)nt1 * KS1_ + ks0) * 64 + lane;
    const u32x4* xptr = reinterpret_cast<const u32x4*>(x1_) + (size_t)ks0 * 64 + lane;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    SkChunk<CH> ck[NB];
    float fs1 = 0.f, fs2 = 0.f;
    auto fold_acc = [&](const u32x4& xv) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float a = __uint_as_float(xv[w] << 16), b = __uint_as_float(xv[w] & 0xffff0000u);
            fs1 += a + b;
            fs2 = fmaf(a, a, fmaf(b, b, fs2));
        }
    };
#pragma unroll
    for (int b = 0; b < NB; ++b) sk_load_full<CH>(ck[b], wptr, xptr, b * CH);
    const MlpFusedArgs p = sv_late_args<MlpFusedArgs>(offsetof(MlpFusedKernarg, p));
    float c2v[RPW], c1v[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wave * RPW + i;
        const int n = nt1 * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        c1v[i] = n < p.N1 ? p.fold_c1[n] : 0.f;
        c2v[i] = n < p.N1 ? p.fold_c2[n] : 0.f;
    }
    sk_settle<RPW>(c2v, c1v);
#pragma unroll
    for (int ks = 0; ks < KPW; ks += NB * CH) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag4(ck[b].w[u]), as_frag4(ck[b].x[u]), acc, 0, 0, 0);
                fold_acc(ck[b].x[u]);
            }
            if (ks + (b + NB) * CH < KPW) {
                __builtin_amdgcn_sched_barrier(0);
                sk_load_full<CH>(ck[b], wptr, xptr, ks + (b + NB) * CH);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const long long t_loop1 = wall_clock64();
    const int ks2 = split * (WAVES * KPW) + wave * KPW;
    const u32x4* w2ptr = reinterpret_cast<const u32x4*>(W2_) + ((size_t)nt2 * KS2_ + ks2) * 64 + lane;
    u32x4 w2[KPW];
    // The down projection's weights of this wave (tile nt2, k-steps split * 128 + wave * 16 .. + 16: 16 KiB) depend on nothing: the first
    // half is requested NOW, so that the HBM stream does not pause while the block reduces and publishes (third version: requested after
    // the publish -- HBM idle for 2.5 us); 8 KiB per wave in flight is what the steady state of the stand-alone kernels keeps (all
    // 16 KiB at once put 24 MB of reads in front of every tile store of the chip: second version, 6 us from loop end to publish).
    // (round 5 re-measured the alternative "reduce and publish with an empty queue, then the whole 16 KiB share": publish 0.9 us earlier, but the
    //  MFMAs then wait 2.7 us for the weights -- 1100 vs 1066 us per step; removed.)
#pragma unroll
    for (int u = 0; u < 8; ++u) w2[u] = __builtin_nontemporal_load(w2ptr + (size_t)u * 64);

    // K reduction across the waves (wave order) + LayerNorm fold epilogue: gemm_skinny_kernel<8, true>'s, value for value
    float v[RPW];
    fs1 += __shfl_xor(fs1, 32, 64);
    fs2 += __shfl_xor(fs2, 32, 64);
    if (half == 0) fst_s[wave * 32 + m] = make_float2(fs1, fs2);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wave * RPW + i;
        float t = red[0][r][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += red[w][r][lane];
        v[i] = t;
    }
    {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) { const float2 t = fst_s[q * 32 + m]; s1 += t.x; s2 += t.y; }
        const float invD = 1.0f / (float)p.fold_D;
        const float mean = s1 * invD;
        float var = s2 * invD - mean * mean;
        var = var > 0.f ? var : 0.f;
        const float rstd = rsqrtf(var + p.fold_eps);
        const int r = wave * RPW;
        const int nl = 8 * (r >> 2) + 4 * half + (r & 3);                 // local column of v[0] (v[1]: + 1)
        float o[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            float x = 0.f;
            if (nt1 * 32 + nl + i < p.N1) {
                x = bfround(rstd * (v[i] - mean * c1v[i]) + c2v[i]);
                if (p.act != ACT_NONE) x = sv_act(x, p.act);
            }
            o[i] = x;
        }
        // the tile in fragment order (the image xp_index addresses: [k-step nl >> 4][64 lanes][8])
        *reinterpret_cast<uint32_t*>(tile_s + (((nl >> 4) * 64 + ((nl >> 3) & 1) * 32 + m) * 8 + (nl & 7))) = pack2bf(o[0], o[1]);
    }
    __syncthreads();
    // ---- hand-off, third version: NO flag and NO counter.  The launch in front of this one (gemm_cols_resid_kernel) fills the whole
    // activation buffer with the bf16 pair 0xFFFF'FFFF (two NaNs: no finite GELU output has that pattern).  A producer only writes its
    // 2 KiB tile (write-through 16-byte stores, nothing to wait for); a consumer WAVE polls the 16 KiB it needs itself -- the tiles of
    // the 8 producers behind its 16 k-steps, not of all 64 producers of the slice -- and re-requests only the k-steps that still
    // carry the pattern.  History (profiles/mlp_fused_r04_ab.log): one ticket word per K slice: 25.5 us per launch (64 arrivals + 64
    // pollers per word); one flag word per producer polled by wave 0: 17.7 us = the two launches, with 6 us of "publish" (the store
    // drained behind 24 MB of weight prefetch) and 4 us of "wait" on the critical path.
    const __amdgpu_buffer_rsrc_t rs_act = __builtin_amdgcn_make_buffer_rsrc(p.out_xp, 0, (unsigned)((size_t)p.out_KS * 1024), 0x00020000);
    if (wave < 2) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(tile_s) + tid * 16);
        __builtin_amdgcn_raw_buffer_store_b128(q, rs_act, nt1 * 2048 + tid * 16, 0, 16);          // sc1: write-through
    }
    const long long t_pub = wall_clock64();
    // second half of the weights (the first half has landed during the reduction), then -- once half of THAT is in -- the activations:
    // their producers publish at about the same time as this block, and a request that finds the pattern costs a whole extra round trip
#pragma unroll
    for (int u = 8; u < 16; ++u) w2[u] = __builtin_nontemporal_load(w2ptr + (size_t)u * 64);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");

    // ---- phase 2: down projection (tile nt2, K slice `split`) -> fp32 slab, gemm_skinny_kernel<8, false>'s order ----
    // (round 5 tried rowln_cattn_kernel's lesson here -- hold the first poll until a fixed time after the block's start: 1007.1 us per step at 10.0 us
    //  against 1009.8 without, worse from 11 us on: the polls already sit where the data turns up; profiles/rowln_cattn_r05_ab.log)
    u32x4 x2[KPW];
#pragma unroll
    for (int u = 0; u < KPW; ++u) x2[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_act, (ks2 + u) * 1024 + lane * 16, 0, 16);   // sc1: L1 bypass
    unsigned pending = 0xffffu;                              // k-steps whose activations are not (known to be) complete: wave-uniform
    int gave_up = 1;
    // Bounded by WALL CLOCK, not by a poll count (65536 polls of ~2 us each per wave, per layer, per step turned a
    // co-residency failure into minutes before the host saw it): a wave gives up after spin_ticks (5 ms) -- and at once when another
    // wave or an earlier launch has already raised the flag (every later layer of a void step then falls through without waiting).
    for (int it = 0;; ++it) {
        unsigned still = 0u;
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
            if (pending & (1u << u)) {
                const bool bad = x2[u][0] == 0xffffffffu || x2[u][1] == 0xffffffffu || x2[u][2] == 0xffffffffu || x2[u][3] == 0xffffffffu;
                if (__any(bad)) still |= 1u << u;
            }
        }
        pending = still;
        if (!pending) { gave_up = 0; break; }
        if ((it & 7) == 7 && (wall_clock64() - t_pub > (long long)p.spin_ticks ||
                              __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
        __builtin_amdgcn_s_sleep(8);
#pragma unroll
        for (int u = 0; u < KPW; ++u)
            if (pending & (1u << u)) x2[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_act, (ks2 + u) * 1024 + lane * 16, 0, 16);
    }
    if (gave_up && lane == 0) atomicCAS(p.err, 0, 3);      // the step's result is void; the first code raised survives
    const long long t_go = wall_clock64();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int u = 0; u < KPW; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag4(w2[u]), as_frag4(x2[u]), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int r = wave * RPW + i;
        float t = red[0][r][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += red[w][r][lane];
        v[i] = t;
    }
    {
        const int r = wave * RPW;
        const int n0 = nt2 * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        *reinterpret_cast<float2*>(p.ws + ((size_t)split * p.rows_ws + m) * p.ldws + n0) = make_float2(v[0], v[1]);
    }
    if (p.trace && tid == 0) {                              // block L: start | c_fc loop done | tile published | slice complete | end  (wave 0's clock)
        long long* q = p.trace + (size_t)L * 8;
        q[0] = t_start; q[1] = t_loop1; q[2] = t_pub; q[3] = t_go; q[4] = wall_clock64(); { unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc)); q[5] = (long long)(xcc & 0xf); }
    }
}
static size_t mlp_fused_smem() { return (size_t)8 * 16 * 64 * 4 + (size_t)8 * 32 * 8 + 2048 + 64; }

// 0 = launched; -1 = the shapes are outside the kernel's scope (the caller runs the two launches)
int launch_mlp_fused(const MlpFusedArgs& a, hipStream_t st) {
    const int KS1 = a.K1 / 16, KS2 = a.K2 / 16, T1 = a.N1pad / 32, T2 = a.N2pad / 32;
    if (a.splitk < 1 || 8 % a.splitk || T1 % 8 || KS1 != 8 * 16 || KS2 != a.splitk * 8 * 16) return -1;      // 16 k-steps per wave in both phases
    if (T2 * a.splitk != T1 || a.K2 != a.N1pad || a.N1 != a.N1pad || a.N2 != a.N2pad) return -1;
    if (!a.err || !a.fold_c1 || !a.fold_c2) return -1;
    mlp_fused_kernel<<<T1, 512, mlp_fused_smem(), st>>>(a.W1, a.x1, a.W2, KS1, KS2, a.splitk, a);
    return 0;
}

}  // namespace sv
