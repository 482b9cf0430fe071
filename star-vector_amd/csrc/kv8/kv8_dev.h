// The e4m3 paged KV cache (SV_KV_FP8_E4M3): page layout, quantiser and dequantiser shared by attention.hip (decode attention, prompt
// rows -> pages) and kv8.hip (sv_debug_kv_read).  No kernel lives here.  The rule is stated in include/starvector_hip.h.
//
// One page = 64 tokens of one layer (one KV head), 64 * D * 2 + 128 bytes:
//   K codes  [2 halves of 32 keys][D/32 k-steps][64 lanes][2 key-groups of 16][8] : lane (key = l&15, c = l>>4) holds, for u = 0, 1,
//            K[32 half + 16 u + key][32 s + 8 c + e] -- the two 8-byte halves of ONE 16-byte load are the bf16 layout's fragments
//            (kg = 2 half + u, s) and become the A operands of S^T = K.Q^T once widened
//   V codes  [2 key-groups of 32][D/32 dv-tile pairs][64 lanes][2 dv-tiles][8] : lane (dv = l&15, c = l>>4) holds, for tl = 0, 1,
//            V[32 g + 16 (e>>2) + 4 c + (e&3)][16 (2 t2 + tl) + dv]
//   K scales [64] one byte E + 127 per token, then V scales [64]
// A wave-load is one contiguous 1 KiB, as in the bf16 layout; a 32-key group costs D/32 + D/32 of them instead of D/16 + D/16.
#pragma once
#include "../kernels.h"

namespace sv {

__device__ __forceinline__ size_t kv8_k_offset(int D, int t64, int d) {
    const int kg = t64 >> 4, key = t64 & 15, s = d >> 5, c = (d >> 3) & 3, e = d & 7;
    return ((size_t)((((kg >> 1) * (D >> 5) + s) * 64 + c * 16 + key) * 2 + (kg & 1))) * 8 + e;
}
__device__ __forceinline__ size_t kv8_v_offset(int D, int t64, int dv) {
    const int g = t64 >> 5, k32 = t64 & 31, u = k32 >> 4, c = (k32 >> 2) & 3, r = k32 & 3;
    const int e = 4 * u + r, t = dv >> 4, dl = dv & 15;
    return (size_t)64 * D + ((size_t)((((g * (D >> 5) + (t >> 1)) * 64 + c * 16 + dl) * 2 + (t & 1)))) * 8 + e;
}
__device__ __forceinline__ size_t kv8_kscale_offset(int D, int t64) { return (size_t)128 * D + t64; }
__device__ __forceinline__ size_t kv8_vscale_offset(int D, int t64) { return (size_t)128 * D + 64 + t64; }

// |x| of a bf16 as an ordered integer, 0 for a non-finite one: the maximum of these over a row is the row's amax (bf16 bits)
__device__ __forceinline__ uint32_t kv8_mag(uint32_t bf) {
    const uint32_t a = bf & 0x7fffu;
    return a < 0x7f80u ? a : 0u;
}
// the scale byte E + 127 of a row whose amax has the bf16 bits `amax_bits`: E = floor(log2 amax) - 7 in [-120, 120]; amax = 0: E = 0
// (a subnormal amax lies below 2^-126: the clamp)
__device__ __forceinline__ uint32_t kv8_scale_byte(uint32_t amax_bits) {
    if (amax_bits == 0u) return 127u;
    int E = (int)(amax_bits >> 7) - 127 - 7;
    E = E < -120 ? -120 : (E > 120 ? 120 : E);
    return (uint32_t)(E + 127);
}
// 2^(byte - 127) as a float, for ANY byte: what a page's last owner left behind a sequence's position may be read as a scale, and
// must never turn into an Inf or NaN factor (0 x Inf = NaN in the P.V product) -- so the exponent is clamped to the format's range again
__device__ __forceinline__ float kv8_scale_f32(uint32_t byte) {
    const uint32_t b = byte < 7u ? 7u : (byte > 247u ? 247u : byte);
    return __uint_as_float(b << 23);
}
// one code: e4m3_rne(x * 2^-E); the multiply is exact, |x * 2^-E| < 256 never saturates; a non-finite x becomes the NaN code
__device__ __forceinline__ uint32_t kv8_code(bf16_t x, uint32_t scale_byte) {
    if ((x & 0x7fffu) >= 0x7f80u) return 0x7fu;
    const float y = bf2f(x) * __uint_as_float((254u - scale_byte) << 23);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y, 0.f, 0, false) & 0xffu;
}
// 8 bf16 (one 16-byte piece of a row) -> 8 codes
__device__ __forceinline__ uint2 kv8_code8(const uint4& v, uint32_t scale_byte) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t c[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = kv8_code((bf16_t)(w[i] & 0xffffu), scale_byte);
        c[2 * i + 1] = kv8_code((bf16_t)(w[i] >> 16), scale_byte);
    }
    return make_uint2(c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24, c[4] | c[5] << 8 | c[6] << 16 | c[7] << 24);
}
// two codes -> two bf16 times the scale, one v_cvt_scalef32_pk_bf16_fp8 (exact: 2^E x e4m3 is a bf16 number)
__device__ __forceinline__ uint32_t kv8_widen2(uint32_t codes, float scale, bool hi) {
    typedef __bf16 kv8_bf16x2 __attribute__((ext_vector_type(2)));
    const kv8_bf16x2 a = hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes, scale, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes, scale, false);
    return __builtin_bit_cast(uint32_t, a);
}
// 8 codes of ONE key -> the bf16 fragment (K side: a lane's fragment is one key's)
__device__ __forceinline__ u32x4 kv8_widen8(uint32_t lo, uint32_t hi, float scale) {
    return u32x4{kv8_widen2(lo, scale, false), kv8_widen2(lo, scale, true), kv8_widen2(hi, scale, false), kv8_widen2(hi, scale, true)};
}
// one code of a row with scale byte `sb` as the attention sees it (the scalar form of the above, for the read-back)
__device__ __forceinline__ bf16_t kv8_deq1(uint32_t code, uint32_t sb) {
    return (bf16_t)(kv8_widen2(code & 0xffu, kv8_scale_f32(sb), false) & 0xffffu);
}

// the raw fragments of one 32-key group: the codes and the scale bytes this lane needs
//   ks[u]: key 16 u + (l & 15) (its K fragments);  vs[h]: the four keys 16 h + 4 c .. + 3 (elements 4 h .. 4 h + 3 of its V fragments)
template <int D>
struct Kv8Raw {
    u32x4 k[D / 32];
    u32x4 v[D / 32];
    uint32_t ks[2];
    uint32_t vs[2];
};

template <int D>
__device__ __forceinline__ void load_group(Kv8Raw<D>& f, const char* pool, int page_index, int page_bytes, int g, int lane) {
    constexpr int NK = D / 32;
    const char* page = pool + (size_t)page_index * page_bytes;
    const int half = g & 1;
#pragma unroll
    for (int s = 0; s < NK; ++s)
        f.k[s] = *reinterpret_cast<const u32x4*>(page + ((size_t)((half * NK + s) * 64 + lane)) * 16);
#pragma unroll
    for (int t = 0; t < NK; ++t)
        f.v[t] = *reinterpret_cast<const u32x4*>(page + (size_t)64 * D + ((size_t)((half * NK + t) * 64 + lane)) * 16);
    const unsigned char* sc = reinterpret_cast<const unsigned char*>(page + (size_t)128 * D);
    f.ks[0] = sc[32 * half + (lane & 15)];
    f.ks[1] = sc[32 * half + 16 + (lane & 15)];
    f.vs[0] = *reinterpret_cast<const uint32_t*>(sc + 64 + 32 * half + 4 * (lane >> 4));
    f.vs[1] = *reinterpret_cast<const uint32_t*>(sc + 64 + 32 * half + 16 + 4 * (lane >> 4));
}

// raw -> the bf16 fragments of the bf16 cache's KvFrags<D> (K part k[2][D/32], V part v[D/16]), holding deq(quant(.)) exactly
template <int D, typename Frags>
__device__ __forceinline__ void kv8_widen_group(const Kv8Raw<D>& r, Frags& f) {
    constexpr int NK = D / 32;
    const float k0 = kv8_scale_f32(r.ks[0]), k1 = kv8_scale_f32(r.ks[1]);
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        f.k[0][s] = kv8_widen8(r.k[s][0], r.k[s][1], k0);
        f.k[1][s] = kv8_widen8(r.k[s][2], r.k[s][3], k1);
    }
    // a V fragment holds 8 keys: elements (2 j, 2 j + 1) of the low word pair are keys 4 c + 2 j, + 1 of the group's first 16, the high
    // word pair the same keys of its second 16 -- a packed conversion takes ONE scale, so the pair is converted once per key and merged
    float sv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sv[e] = kv8_scale_f32((r.vs[e >> 2] >> (8 * (e & 3))) & 0xffu);
#pragma unroll
    for (int t = 0; t < 2 * NK; ++t) {
        const uint32_t lo = r.v[t >> 1][2 * (t & 1)], hi = r.v[t >> 1][2 * (t & 1) + 1];
        u32x4 o;
        o[0] = (kv8_widen2(lo, sv[0], false) & 0xffffu) | (kv8_widen2(lo, sv[1], false) & 0xffff0000u);
        o[1] = (kv8_widen2(lo, sv[2], true) & 0xffffu) | (kv8_widen2(lo, sv[3], true) & 0xffff0000u);
        o[2] = (kv8_widen2(hi, sv[4], false) & 0xffffu) | (kv8_widen2(hi, sv[5], false) & 0xffff0000u);
        o[3] = (kv8_widen2(hi, sv[6], true) & 0xffffu) | (kv8_widen2(hi, sv[7], true) & 0xffff0000u);
        f.v[t] = o;
    }
}

}  // namespace sv
