// MXFP4 decoder weights (sv_config.weight_dtype = SV_WEIGHT_MXFP4; DESIGN.md "MXFP4 decoder weights"):
//   mxfp4_pack_kernel        : fp32 / bf16 rows -> e8m0 block exponents + e2m1 codes in the decode image, and the dequantised values as
//                              bf16 in the usual packed layout (kernels.h states the format and both layouts)
//   gemm_skinny_mxfp4_kernel : the decode GEMM over the 4-bit image: gemm_skinny_fp8_kernel's structure, the codes widened to the bf16
//                              MFMA operand with the block scale in one instruction per pair (v_cvt_scalef32_pk_bf16_fp4)
// A dequantised weight q * 2^E is exactly a bf16 number, so the widened operand is bit for bit what the bf16 image holds: the launch computes
// what the bf16 kernels compute over that image, except for the K-summation order.
#include "../skinny_dev.h"

namespace sv {

template <typename SrcT>
__device__ __forceinline__ float mx_ld_f32(const SrcT* p) {
    if constexpr (sizeof(SrcT) == 4) return (float)*p;
    else return bf2f((bf16_t)*p);
}
// block exponent E of a block maximum (see kernels.h): floor(log2(amax)) - 2 is the fp32 exponent field - 129
__device__ __forceinline__ int mx_block_exp(float amax) {
    if (!(amax > 0.f)) return 0;
    int E = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 129;
    return E < -125 ? -125 : E > 125 ? 125 : E;
}
// |v| / 2^E -> the e2m1 magnitude, round to nearest, ties to the even mantissa bit (rintf is ties-to-even on each of the three grids:
// steps of 0.5 below 2, of 1 below 4, of 2 above), saturating at 6
__device__ __forceinline__ float mx_round_e2m1(float a) {
    if (a < 2.f) return rintf(a * 2.f) * 0.5f;
    if (a < 4.f) return rintf(a);
    return fminf(rintf(a * 0.5f) * 2.f, 6.f);
}
__device__ __forceinline__ uint32_t mx_code(float r) {       // {0, .5, 1, 1.5, 2, 3, 4, 6} -> 0 .. 7
    const int r2 = (int)(r * 2.f);
    return (uint32_t)(r2 < 4 ? r2 : r2 < 8 ? 2 + (r2 >> 1) : 4 + (r2 >> 2));
}

// one thread = one lane's 16 bytes of one group (column tile, 64 consecutive k): four k-steps of 8 codes.  A lane holds half of each of the
// group's two MX blocks, lane ^ 32 the other half: the block maxima meet through one cross-lane exchange (whole waves run the loop: the
// total and the stride are multiples of 64).
template <typename SrcT>
__global__ __launch_bounds__(256) void mxfp4_pack_kernel(const SrcT* __restrict__ src, bf16_t* __restrict__ dst_bf16, uint8_t* __restrict__ dst_w4,
                                                         uint8_t* __restrict__ scale_plain, int N, int K, int Npad, int Kpad) {
    const int KS = Kpad >> 4, KG = Kpad >> 6;
    const size_t total = (size_t)(Npad >> 5) * KG * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63), m = lane & 31, half = lane >> 5;
        const size_t t = i >> 6;
        const int g = (int)(t % KG), nt = (int)(t / KG);
        const int n = nt * 32 + m;
        float f[4][8];
        float amax[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 64 * g + 16 * u + 8 * half + e;
                f[u][e] = (n < N && k < K) ? mx_ld_f32(src + (size_t)n * K + k) : 0.f;
                amax[u >> 1] = fmaxf(amax[u >> 1], fabsf(f[u][e]));
            }
        int E[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            amax[b] = fmaxf(amax[b], __shfl_xor(amax[b], 32));
            E[b] = mx_block_exp(amax[b]);
        }
        uint32_t words[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int Eb = E[u >> 1];
            const float inv = __uint_as_float((uint32_t)(127 - Eb) << 23), sc = __uint_as_float((uint32_t)(127 + Eb) << 23);
            uint32_t w = 0;
            float q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float r = mx_round_e2m1(fabsf(f[u][e]) * inv);
                const bool neg = f[u][e] < 0.f;
                w |= (mx_code(r) | (neg ? 8u : 0u)) << (4 * e);
                q[e] = neg ? -(r * sc) : r * sc;               // exact: at most two significant bits, 2^-126 <= |q| < 2^128
            }
            words[u] = w;
            *reinterpret_cast<uint4*>(dst_bf16 + (((size_t)nt * KS + 4 * g + u) * 64 + lane) * 8) = pack8(q);
        }
        uint8_t* grp = dst_w4 + ((size_t)nt * KG + g) * SV_MXFP4_GROUP;
        *reinterpret_cast<uint4*>(grp + lane * 16) = make_uint4(words[0], words[1], words[2], words[3]);
        if (half == 0) {
            const uint32_t b0 = (uint32_t)(E[0] + 127), b1 = (uint32_t)(E[1] + 127);
            *reinterpret_cast<uint16_t*>(grp + 1024 + m * 2) = (uint16_t)(b0 | (b1 << 8));
            if (scale_plain) {
                scale_plain[(size_t)n * (Kpad >> 5) + 2 * g] = (uint8_t)b0;
                scale_plain[(size_t)n * (Kpad >> 5) + 2 * g + 1] = (uint8_t)b1;
            }
        }
    }
}

void launch_pack_weight_mxfp4(const void* src, int src_is_f32, bf16_t* dst_bf16, uint8_t* dst_w4, uint8_t* scale_plain, int N, int K,
                              int Npad, int Kpad, hipStream_t st) {
    const size_t total = (size_t)(Npad / 32) * (Kpad / 64) * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    if (src_is_f32) mxfp4_pack_kernel<float><<<blocks, 256, 0, st>>>((const float*)src, dst_bf16, dst_w4, scale_plain, N, K, Npad, Kpad);
    else mxfp4_pack_kernel<bf16_t><<<blocks, 256, 0, st>>>((const bf16_t*)src, dst_bf16, dst_w4, scale_plain, N, K, Npad, Kpad);
}

// 8 e2m1 codes (one lane's share of a k-step) -> the bf16 MFMA operand, times the block scale: one instruction per pair.  The scale
// operand is an f32 whose exponent field is the e8m0 byte.
__device__ __forceinline__ u32x4 fp4x8_to_bf16x8(uint32_t w, float sc) {
    const sv_bf16x2 a0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), a1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
    const sv_bf16x2 a2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), a3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
    u32x4 wf = {__builtin_bit_cast(uint32_t, a0), __builtin_bit_cast(uint32_t, a1), __builtin_bit_cast(uint32_t, a2), __builtin_bit_cast(uint32_t, a3)};
    return wf;
}

// ------------------------------------------------------------------------------------------------
// skinny GEMM with MXFP4 weights: the decode step's weight stream at 4.25 bits per weight.  gemm_skinny_fp8_kernel's structure: K split
// over the waves of a block and over `splitk` blocks, non-temporal weight loads, the late argument block, the shared epilogue (fp32 slabs,
// packed activations with bias + activation, fp32 logits).  A lane's 16-byte load is a GROUP of four k-steps (two MX blocks of its row,
// whose two scale bytes ride in the same 1088-byte group); each k-step's 8 codes are widened with their block's scale and fed to the bf16
// MFMA in ascending k.  No accumulator scale.
// CT = column tiles per block (1, 2, 4): every activation fragment a wave loads feeds CT MFMAs (a block re-reads 4 / CT activation bytes
// out of L2 per weight byte).  The k order of an output is the same for every CT, so the bits are too.  Row tiles ride on grid.z.
// The 5th kernel parameter is the number of column tiles (the last block of a CT > 1 launch may hold fewer).
// ------------------------------------------------------------------------------------------------
template <int WAVES, int CT>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_mxfp4_kernel(const uint8_t* W4_, const bf16_t* xp_, int KS_, int ks_per_split_, int n_tiles_, SkinnyArgs p_unused) {
    constexpr int G = CT == 4 ? 1 : 2;                     // groups (of 4 k-steps) per register chunk
    extern __shared__ __attribute__((aligned(16))) char mx_smem[];
    float (*red)[16][64] = reinterpret_cast<float (*)[16][64]>(mx_smem);          // [WAVES][16][64]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt0 = blockIdx.x * CT, split = blockIdx.y, mt = blockIdx.z;
    const int KS = KS_, n_tiles = n_tiles_;
    const int ks_per_split = ks_per_split_;
    const int ks_per_wave = ks_per_split / WAVES;          // a multiple of 4 (launcher)
    const int gpw = ks_per_wave >> 2;                      // groups per wave
    const int ks0 = split * ks_per_split + wave * ks_per_wave;
    const int m = lane & 31, half = lane >> 5;

    // a column tile past the last one (CT > 1, the last block) streams the last tile again and stores nothing
    const uint8_t* wb[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int nt = nt0 + j < n_tiles ? nt0 + j : n_tiles - 1;
        wb[j] = W4_ + ((size_t)nt * (KS >> 2) + (ks0 >> 2)) * SV_MXFP4_GROUP;
    }
    const u32x4* xptr = reinterpret_cast<const u32x4*>(xp_) + ((size_t)mt * KS + ks0) * 64 + lane;

    f32x16 acc[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    constexpr int RPW = 16 / WAVES;                       // WAVES in {2, 4, 8}
    struct Chunk { u32x4 w[CT][G]; uint32_t s[CT][G]; u32x4 x[4 * G]; };
    Chunk ca, cb;
    auto load = [&](Chunk& c, int gi, auto full) {         // FULL: no guards (exact wait counts in the steady state, see sk_load_full)
        constexpr bool FULL = decltype(full)::value;
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int t = 0; t < G; ++t)
                if (FULL || gi + t < gpw) {
                    const uint8_t* grp = wb[j] + (size_t)(gi + t) * SV_MXFP4_GROUP;
                    c.w[j][t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(grp) + lane);
                    c.s[j][t] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(grp + 1024) + m);
                }
#pragma unroll
        for (int t = 0; t < G; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (FULL || gi + t < gpw) c.x[4 * t + u] = xptr[(size_t)((gi + t) * 4 + u) * 64];
    };
    auto compute = [&](Chunk& c, int gi, auto full) {
        constexpr bool FULL = decltype(full)::value;
#pragma unroll
        for (int t = 0; t < G; ++t) {
            if (FULL || gi + t < gpw) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < CT; ++j) {
                        const uint32_t sb = u < 2 ? (c.s[j][t] & 0xffu) : (c.s[j][t] >> 8);
                        const u32x4 wf = fp4x8_to_bf16x8(c.w[j][t][u], __uint_as_float(sb << 23));
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag4(wf), as_frag4(c.x[4 * t + u]), acc[j], 0, 0, 0);
                    }
            }
        }
    };
    SkinnyArgs p;
    float bias_d[CT][RPW];
    auto late = [&]() {     // the bias needs the argument block (a scalar load): requested after the stream is in flight
        p = sv_late_args<SkinnyArgs>(offsetof(SkinnyKernarg, p));
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            sk_bias<RPW>(p, bias_d[j], wave * RPW, nt0 + j, half);
            sk_settle<RPW>(bias_d[j]);
        }
    };
    auto guarded = [&](int gi) {
        for (; gi < gpw; gi += 2 * G) {
            compute(ca, gi, std::false_type{});
            if (gi + 2 * G < gpw) load(ca, gi + 2 * G, std::false_type{});
            if (gi + G < gpw) compute(cb, gi + G, std::false_type{});
            if (gi + 3 * G < gpw) load(cb, gi + 3 * G, std::false_type{});
        }
    };
    if (gpw >= 4 * G) {                                     // long ranges: branch-free steady state
        load(ca, 0, std::true_type{});
        load(cb, G, std::true_type{});
        late();
        int gi = 0;
        for (; gi + 4 * G <= gpw; gi += 2 * G) {
            compute(ca, gi, std::true_type{});
            __builtin_amdgcn_sched_barrier(0);
            load(ca, gi + 2 * G, std::true_type{});
            __builtin_amdgcn_sched_barrier(0);
            compute(cb, gi + G, std::true_type{});
            __builtin_amdgcn_sched_barrier(0);
            load(cb, gi + 3 * G, std::true_type{});
            __builtin_amdgcn_sched_barrier(0);
        }
        guarded(gi);
    } else {
        load(ca, 0, std::false_type{});
        if (G < gpw) load(cb, G, std::false_type{});
        late();
        guarded(0);
    }
    // the K reduction across waves, one column tile at a time through the same buffer
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        if (j) __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[j][r];
        __syncthreads();
        float v[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int r = wave * RPW + i;
            float t = red[0][r][lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) t += red[w][r][lane];
            v[i] = t;
        }
        if (nt0 + j < n_tiles) sk_store<RPW>(p, v, bias_d[j], wave * RPW, nt0 + j, mt, split, m, half);      // block-uniform
    }
}

// Waves per block = how K is cut inside a block = the order in which a row's partial sums are added: a function of (K, split-K) only,
// never of the rows.  A wave's range is whole groups of 4 k-steps.
int skinny_waves_mxfp4(int KS, int splitk) {
    if (splitk < 1 || KS % splitk) return 0;
    const int per_split = KS / splitk;
    if (per_split % 32 == 0) return 8;
    if (per_split % 16 == 0) return 4;
    if (per_split % 8 == 0) return 2;
    return 0;
}

template <int W, int CT>
static void launch_mx(const SkinnyArgs& a, hipStream_t st) {
    const int n_tiles = a.Npad / 32;
    const dim3 grid((n_tiles + CT - 1) / CT, a.splitk, a.MT);
    gemm_skinny_mxfp4_kernel<W, CT><<<grid, W * 64, (size_t)W * 16 * 64 * 4, st>>>(a.W4, a.xp, a.K / 16, (a.K / 16) / a.splitk, n_tiles, a);
}
template <int W>
static void launch_mx_ct(const SkinnyArgs& a, int ct, hipStream_t st) {
    if (ct >= 4) launch_mx<W, 4>(a, st);
    else if (ct >= 2) launch_mx<W, 2>(a, st);
    else launch_mx<W, 1>(a, st);
}

bool launch_gemm_skinny_mxfp4(const SkinnyArgs& a, hipStream_t st) {
    if (!a.W4 || a.K % 64 || a.MT < 1) return false;
    if (!(a.out_mode == SK_OUT_PARTIAL || ((a.out_mode == SK_OUT_PACKED_ACT || a.out_mode == SK_OUT_F32) && a.splitk == 1)))
        return false;
    if (a.fold_c1 || a.amax || a.poison) return false;      // the folded LayerNorm / selection / pattern stores belong to the bf16 kernels
    // engines pass their plan (pick_decode_plan); 0: the op-level entry points take sv_debug_set_col_tiles' value, else one tile
    const int ct = a.col_tiles ? a.col_tiles : g_op_col_tiles.load(std::memory_order_relaxed);
    switch (skinny_waves_mxfp4(a.K / 16, a.splitk)) {
        case 8: launch_mx_ct<8>(a, ct, st); return true;
        case 4: launch_mx_ct<4>(a, ct, st); return true;
        case 2: launch_mx_ct<2>(a, ct, st); return true;
        default: return false;
    }
}

}  // namespace sv
