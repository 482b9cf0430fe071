// Device helpers shared by the GEMM units (no kernel lives here):
//  * lds_dma16: the 16-byte-per-lane LDS-DMA of the prompt-side tile kernels and of the two-row-tile ring kernel (gemm.hip);
//  * the pieces every weight-streaming decode kernel is assembled from (gemm.hip, mlp_fused.hip): register chunks
//    of the stream, the early bias request, the shared epilogue, the fp8 -> bf16 widening and the kernarg layout.
#pragma once
#include <cstddef>
#include "kernels.h"

namespace sv {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ void lds_dma16(const void* g, char* lds_wave_base) {
    // 16 B per lane; LDS destination = wave-uniform base + lane*16 (hardware), source is per lane
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)lds_wave_base, 16, 0, 0);
}

// 8 e4m3 bytes (one lane's share of a k-step) -> the bf16 MFMA operand.  gfx950 converts two fp8 to a packed bf16 pair in ONE
// instruction (v_cvt_scalef32_pk_bf16_fp8, scale 1.0: exact, every e4m3 value is a bf16 value); round 2 went through float
// (v_cvt_pk_f32_fp8 + shift / and-or per pair: 12 VALU instructions per k-step against these 4, next to 2 MFMAs of 8 passes).
typedef __bf16 sv_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 fp8x8_to_bf16x8(uint32_t lo, uint32_t hi) {
    const sv_bf16x2 a0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), a1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const sv_bf16x2 a2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), a3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    union { sv_bf16x2 b; uint32_t u; } c0, c1, c2, c3;
    c0.b = a0; c1.b = a1; c2.b = a2; c3.b = a3;
    u32x4 wf = {c0.u, c1.u, c2.u, c3.u};
    return wf;
}

// one chunk of the weight / activation stream held in registers
template <int CH>
struct SkChunk {
    u32x4 w[CH];
    u32x4 x[CH];
};

template <int CH>
__device__ __forceinline__ void sk_load(SkChunk<CH>& c, const u32x4* wptr, const u32x4* xptr, int ks, int ks_end) {
#pragma unroll
    for (int u = 0; u < CH; ++u)
        if (ks + u < ks_end) c.w[u] = __builtin_nontemporal_load(wptr + (size_t)(ks + u) * 64);   // streamed once
#pragma unroll
    for (int u = 0; u < CH; ++u)
        if (ks + u < ks_end) c.x[u] = xptr[(size_t)(ks + u) * 64];                                 // wave-uniform guard
}

// the same without guards: the chunk lies inside the wave's k range.  The steady-state loops use this one on purpose: with the
// wave-uniform guards of sk_load every load sits behind a branch, the compiler's wait-count analysis merges "loaded" and "not
// loaded" paths and falls back to s_waitcnt vmcnt(0) in front of EVERY chunk's MFMAs -- the wave then waits for the loads it has
// just issued (two chunks "in flight" were one round trip per chunk pair; found in round 3 from the ISA).
template <int CH>
__device__ __forceinline__ void sk_load_full(SkChunk<CH>& c, const u32x4* wptr, const u32x4* xptr, int ks) {
#pragma unroll
    for (int u = 0; u < CH; ++u) c.w[u] = __builtin_nontemporal_load(wptr + (size_t)(ks + u) * 64);
#pragma unroll
    for (int u = 0; u < CH; ++u) c.x[u] = xptr[(size_t)(ks + u) * 64];
}

// the bias of this lane's RPW output columns, requested BEFORE the weight stream (the epilogue must not start with a round trip)
template <int RPW>
__device__ __forceinline__ void sk_bias(const SkinnyArgs& p, float* bias_d, int r0, int nt, int half, float* fc1 = nullptr) {
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        bias_d[i] = 0.f;
        if (fc1) fc1[i] = 0.f;
        const int r = r0 + i;
        const int n = nt * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        if (p.out_mode == SK_OUT_PACKED_ACT && n < p.N) {
            if (fc1 && p.fold_c1) { fc1[i] = p.fold_c1[n]; bias_d[i] = p.fold_c2[n]; }
            else if (p.bias) bias_d[i] = bf2f(p.bias[n]);
        }
    }
}
// The epilogue operands must have LANDED before the k loop starts: a load that stays pending across the loop makes the compiler's
// wait-count analysis give up on the loop (an unbounded distance to the oldest pending load) and put s_waitcnt vmcnt(0) at the
// top of every iteration.  An empty asm that "uses" the values forces the wait here, once, in the prologue.
template <int RPW>
__device__ __forceinline__ void sk_settle(float* a, float* b = nullptr) {
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        asm volatile("" : "+v"(a[i]));
        if (b) asm volatile("" : "+v"(b[i]));
    }
}
// shared tail of the skinny kernels: v[i] = the reduced accumulator row r0 + i of lane (m, half), i.e. output
// column n(r) = nt*32 + 8*(r >> 2) + 4*half + (r & 3) of row mt*32 + m; RPW consecutive rows r (RPW in {1, 2, 4, 8, 16})
// fold: LayerNorm applied algebraically (decode_cols.hip): x = rstd * (acc - mean * c1[n]) + c2[n]; fc1 / fc2 = this lane's RPW
// values of c1 / c2, (mean, rstd) = the statistics of row m
struct SkFold { bool on; float mean, rstd; };
template <int RPW>
__device__ __forceinline__ void sk_store(const SkinnyArgs& p, float* v, const float* bias_d, int r0, int nt, int mt, int split, int m,
                                         int half, const SkFold fold = SkFold{false, 0.f, 1.f}, const float* fc1 = nullptr) {
    constexpr int G = RPW >= 4 ? RPW / 4 : 1;          // groups of (up to) 4 consecutive columns
    constexpr int W = RPW >= 4 ? 4 : RPW;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int r = r0 + 4 * g;
        const int n0 = nt * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        float* vv = v + 4 * g;
        auto store_f32 = [&](float* dst) {
            if constexpr (W == 4) *reinterpret_cast<float4*>(dst) = make_float4(vv[0], vv[1], vv[2], vv[3]);
            else if constexpr (W == 2) *reinterpret_cast<float2*>(dst) = make_float2(vv[0], vv[1]);
            else dst[0] = vv[0];
        };
        // TWO separate stores on purpose: written as one store through `cond ? ws + .. : out_f32 + ..` (or an if / else that only
        // picks the pointer) hipcc 7.2 keeps the out_f32 base register for both arms and the slab store goes to a null pointer
        // (seen twice: the fp8 kernel in round 2, this helper in round 3 -- a GPU memory fault at 0x1000).
        if (p.out_mode == SK_OUT_PARTIAL) {
            store_f32(p.ws + ((size_t)split * p.MT * 32 + mt * 32 + m) * p.ldws + n0);
        } else if (p.out_mode == SK_OUT_F32) {
            if (p.round_bf16) {
#pragma unroll
                for (int i = 0; i < W; ++i) vv[i] = bfround(vv[i]);
            }
            store_f32(p.out_f32 + ((size_t)mt * 32 + m) * p.ldo + n0);
        } else {   // SK_OUT_PACKED_ACT
#pragma unroll
            for (int i = 0; i < W; ++i) {
                float x = 0.f;
                if (n0 + i < p.N) {
                    // (fold: bias_d carries c2 = sum_k beta_k W[n][k] + bias[n])
                    x = fold.on ? bfround(fold.rstd * (vv[i] - fold.mean * fc1[4 * g + i]) + bias_d[4 * g + i])
                                : bfround(vv[i] + bias_d[4 * g + i]);
                    if (p.act != ACT_NONE) x = sv_act(x, p.act);
                }
                vv[i] = x;
            }
            bf16_t* dst = p.out_xp + xp_index(mt, p.out_KS, m, n0);
            if constexpr (W == 4) {
                uint2 o; o.x = pack2bf(vv[0], vv[1]); o.y = pack2bf(vv[2], vv[3]);
                *reinterpret_cast<uint2*>(dst) = o;
            } else if constexpr (W == 2) {
                *reinterpret_cast<uint32_t*>(dst) = pack2bf(vv[0], vv[1]);
            } else {
                dst[0] = f2bf(vv[0]);
            }
        }
    }
}

// Leading scalar parameters = the few values the first address computation needs: they are PRELOADED into SGPRs by the command
// processor (build flag -amdgpu-kernarg-preload-count; only scalar / pointer parameters qualify, not a by-value struct), so the
// weight stream is requested without first waiting for a scalar load of the argument block (a cold K$ miss at every launch).
struct SkinnyKernarg { const void* W; const bf16_t* x; int KS; int ks_per_split; int flags; SkinnyArgs p; };      // the kernarg segment of the skinny kernels

}  // namespace sv
