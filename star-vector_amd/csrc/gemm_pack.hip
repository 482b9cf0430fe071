// What turns a checkpoint's weights into the images the GEMMs read (gfx950):
//
//  * pack_weight_kernel / convert_bf16_kernel : fp32 / bf16 rows -> bf16 in MFMA fragment order (the linear, conflict-free
//                         LDS image of the big-M kernels and the 1 KiB wave loads of the decode kernels, gemm.hip), or plain bf16;
//  * fp8_row_scale_kernel / pack_weight_fp8_kernel : weight-only e4m3 quantisation, one scale per output row, the fp8 image
//                         for the decode stream and the same values as bf16 for the big-M kernels;
//  * cvt_bf16_hw_kernel : the hardware f32 -> bf16 convert on its own (test surface).
#include "kernels.h"

namespace sv {

// ------------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------------
template <typename SrcT>
__global__ void pack_weight_kernel(const SrcT* __restrict__ W, bf16_t* __restrict__ Wp, int N, int K,
                                   int Npad, int Kpad) {
    const int KS = Kpad >> 4;
    const size_t total = (size_t)(Npad >> 5) * KS * 64;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < total;
         c += (size_t)gridDim.x * blockDim.x) {
        int lane = (int)(c & 63);
        size_t t = c >> 6;
        int ks = (int)(t % KS);
        int nt = (int)(t / KS);
        int n = nt * 32 + (lane & 31);
        int k0 = ks * 16 + (lane >> 5) * 8;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int k = k0 + e;
            float v = 0.f;
            if (n < N && k < K) {
                if constexpr (sizeof(SrcT) == 4) v = (float)W[(size_t)n * K + k];
                else v = bf2f((bf16_t)W[(size_t)n * K + k]);
            }
            f[e] = v;
        }
        *reinterpret_cast<uint4*>(Wp + c * 8) = pack8(f);
    }
}

void launch_pack_weight(const void* src, int src_is_f32, bf16_t* dst, int N, int K, int Npad, int Kpad,
                        hipStream_t st) {
    size_t total = (size_t)(Npad / 32) * (Kpad / 16) * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    if (src_is_f32)
        pack_weight_kernel<float><<<blocks, 256, 0, st>>>((const float*)src, dst, N, K, Npad, Kpad);
    else
        pack_weight_kernel<bf16_t><<<blocks, 256, 0, st>>>((const bf16_t*)src, dst, N, K, Npad, Kpad);
}

template <typename SrcT>
__global__ void convert_bf16_kernel(const SrcT* __restrict__ s, bf16_t* __restrict__ d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if constexpr (sizeof(SrcT) == 4) d[i] = f2bf((float)s[i]);
        else d[i] = (bf16_t)s[i];
    }
}
void launch_convert_to_bf16(const void* src, int src_is_f32, bf16_t* dst, size_t n, hipStream_t st) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    if (src_is_f32) convert_bf16_kernel<float><<<blocks, 256, 0, st>>>((const float*)src, dst, n);
    else convert_bf16_kernel<bf16_t><<<blocks, 256, 0, st>>>((const bf16_t*)src, dst, n);
}

// ------------------------------------------------------------------------------------------------
// fp8 (OCP e4m3) weight-only quantisation at load time (BASELINE config 5: fp8 weights).  One scale per output row.
// ------------------------------------------------------------------------------------------------
template <typename SrcT>
__device__ __forceinline__ float ld_as_f32(const SrcT* p) {
    if constexpr (sizeof(SrcT) == 4) return (float)*p;
    else return bf2f((bf16_t)*p);
}
template <typename SrcT>
__global__ __launch_bounds__(256) void fp8_row_scale_kernel(const SrcT* __restrict__ src, float* __restrict__ scale, int N,
                                                            int K, int Npad) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    float m = 0.f;
    if (n < N)
        for (int k = tid; k < K; k += 256) m = fmaxf(m, fabsf(ld_as_f32(src + (size_t)n * K + k)));
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        scale[n] = m > 0.f ? m / 448.0f : 1.0f;             // e4m3 max normal = 448
    }
}
// one thread = one lane's 16 fp8 bytes (two k-steps) of one (n-tile, k-step pair)
template <typename SrcT>
__global__ void pack_weight_fp8_kernel(const SrcT* __restrict__ src, const float* __restrict__ scale, bf16_t* __restrict__ dst_bf16,
                                       uint8_t* __restrict__ dst_q, int N, int K, int Npad, int Kpad) {
    const int KS = Kpad >> 4, KS2 = KS >> 1;
    const size_t total = (size_t)(Npad >> 5) * KS2 * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const size_t t = i >> 6;
        const int ks2 = (int)(t % KS2), nt = (int)(t / KS2);
        const int n = nt * 32 + (lane & 31);
        const float sc = n < N ? scale[n] : 1.0f;
        uint32_t words[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ks = 2 * ks2 + h;
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 16 * ks + 8 * (lane >> 5) + e;
                f[e] = (n < N && k < K) ? ld_as_f32(src + (size_t)n * K + k) / sc : 0.f;
            }
            int w0 = 0, w1 = 0;
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
            words[2 * h] = (uint32_t)w0;
            words[2 * h + 1] = (uint32_t)w1;
            // the same values as bf16 (exact: 3 mantissa bits) for the big-M kernels
            float q[8];
            const f32x2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8(w0, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8(w0, true);
            const f32x2 a2 = __builtin_amdgcn_cvt_pk_f32_fp8(w1, false), a3 = __builtin_amdgcn_cvt_pk_f32_fp8(w1, true);
            q[0] = a0[0]; q[1] = a0[1]; q[2] = a1[0]; q[3] = a1[1]; q[4] = a2[0]; q[5] = a2[1]; q[6] = a3[0]; q[7] = a3[1];
            *reinterpret_cast<uint4*>(dst_bf16 + (((size_t)nt * KS + ks) * 64 + lane) * 8) = pack8(q);
        }
        *reinterpret_cast<uint4*>(dst_q + (((size_t)nt * KS2 + ks2) * 64 + lane) * 16) = make_uint4(words[0], words[1], words[2], words[3]);
    }
}
void launch_pack_weight_fp8(const void* src, int src_is_f32, bf16_t* dst_bf16, uint8_t* dst_q, float* scale, int N, int K,
                            int Npad, int Kpad, hipStream_t st) {
    const size_t total = (size_t)(Npad / 32) * (Kpad / 32) * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    if (src_is_f32) {
        fp8_row_scale_kernel<float><<<Npad, 256, 0, st>>>((const float*)src, scale, N, K, Npad);
        pack_weight_fp8_kernel<float><<<blocks, 256, 0, st>>>((const float*)src, scale, dst_bf16, dst_q, N, K, Npad, Kpad);
    } else {
        fp8_row_scale_kernel<bf16_t><<<Npad, 256, 0, st>>>((const bf16_t*)src, scale, N, K, Npad);
        pack_weight_fp8_kernel<bf16_t><<<blocks, 256, 0, st>>>((const bf16_t*)src, scale, dst_bf16, dst_q, N, K, Npad, Kpad);
    }
}

// f32 -> bf16 through the hardware convert every epilogue uses (common.h pack2bf: v_cvt_pk_bf16_f32; test surface)
__global__ void cvt_bf16_hw_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i + 1 < n) {
        *reinterpret_cast<uint32_t*>(y + i) = pack2bf(x[i], x[i + 1]);
    } else if (i < n) {
        y[i] = (bf16_t)(pack2bf(x[i], 0.f) & 0xffffu);
    }
}
void launch_cvt_bf16_hw(const float* x, bf16_t* y, size_t n, hipStream_t st) {
    cvt_bf16_hw_kernel<<<(unsigned)((n / 2 + 256) / 256), 256, 0, st>>>(x, y, n);
}

}  // namespace sv
