// The e4m3 paged KV cache: what carries a name of its own.  The format's layout, quantiser and dequantiser are kv8_dev.h; the kernels that
// write and read it on the hot path are the KVF = 1 forms of attention.hip's kv_write_prefill_kernel and attn_decode_kernel.
//   kv_read_kernel : sv_debug_kv_read -- tokens of one block-table row back as bf16 rows, as the decode attention sees them, from a pool of
//                    either format (the bf16 pool: the stored bits; the e4m3 pool: the widening of kv8_dev.h, the attention's own)
#include "kv8_dev.h"

namespace sv {

// the bf16 page layout of attention.hip (kv_k_offset / kv_v_offset)
__device__ __forceinline__ size_t kvr_k_offset(int D, int t64, int d) {
    const int kg = t64 >> 4, key = t64 & 15, s = d >> 5, c = (d >> 3) & 3, e = d & 7;
    return ((size_t)((kg * (D >> 5) + s) * 64 + c * 16 + key)) * 16 + e * 2;
}
__device__ __forceinline__ size_t kvr_v_offset(int D, int t64, int dv) {
    const int g = t64 >> 5, k32 = t64 & 31, u = k32 >> 4, c = (k32 >> 2) & 3, r = k32 & 3;
    const int e = 4 * u + r, t = dv >> 4, dl = dv & 15;
    return (size_t)64 * D * 2 + ((size_t)((g * (D >> 4) + t) * 64 + c * 16 + dl)) * 16 + e * 2;
}

// grid (count, n_kv), block 2 * head_dim: thread c owns column c of k [0, D) | v [D, 2 D) of one (token, KV head)
__global__ __launch_bounds__(256) void kv_read_kernel(KvReadArgs p) {
    const int D = p.head_dim;
    const int i = blockIdx.x, kvh = blockIdx.y, kc = threadIdx.x;
    if (i >= p.count || kc >= 2 * D) return;
    const int tok = p.first + i, t64 = tok & 63;
    const bool is_k = kc < D;
    const int d = kc & (D - 1);
    const char* page = p.pool_layer + (size_t)kvh * p.kv_head_stride + (size_t)p.table_row[tok >> 6] * (p.kv_fmt ? kv8_page_bytes(D) : kv_page_bytes(D));
    bf16_t out;
    if (p.kv_fmt) {
        const uint32_t code = *reinterpret_cast<const unsigned char*>(page + (is_k ? kv8_k_offset(D, t64, d) : kv8_v_offset(D, t64, d)));
        const uint32_t sb = *reinterpret_cast<const unsigned char*>(page + (is_k ? kv8_kscale_offset(D, t64) : kv8_vscale_offset(D, t64)));
        out = kv8_deq1(code, sb);
    } else {
        out = *reinterpret_cast<const bf16_t*>(page + (is_k ? kvr_k_offset(D, t64, d) : kvr_v_offset(D, t64, d)));
    }
    p.out[(size_t)i * 2 * p.n_kv * D + (is_k ? 0 : p.n_kv * D) + kvh * D + d] = out;
}
void launch_kv_read(const KvReadArgs& a, hipStream_t st) {
    if (a.count < 1) return;
    kv_read_kernel<<<dim3(a.count, a.n_kv), 2 * a.head_dim, 0, st>>>(a);
}

}  // namespace sv
