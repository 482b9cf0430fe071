// The fork launch of a shared prompt pass (kernels.h, ForkArgs): one prompt was prefilled once, its samples continue as rows of their own.
// Two bandwidth-trivial kernels, run once per call between the prompt pass and the first selection.
#include "kernels.h"

namespace sv {

// grid (prompt, layer * KV heads + KV head, FK_Z page slices).  A thread loads a 16-byte piece of the prompt's tail page, then stores it into
// the same place of every other row's tail page: the source is read once however many samples there are.  Source and destinations are different
// pages (the page plan gives every row its own pages from the tail page on), so there is nothing to order between threads.
#define FK_Z 4
__global__ __launch_bounds__(256) void fork_tail_copy_kernel(ForkArgs a) {
    const int32_t* p = a.prompts + 4 * blockIdx.x;
    const int src_row = p[0], len = p[1], d0 = p[2], nd = p[3];
    if (len % SV_PAGE_TOKENS == 0 || nd == 0) return;          // no partially filled page, or nobody to hand it to
    const int pi = len / SV_PAGE_TOKENS;
    const int layer = blockIdx.y / a.n_kv, kvh = blockIdx.y % a.n_kv;
    char* pool = a.kv_pool + (size_t)layer * a.layer_stride + (size_t)kvh * a.kv_head_stride;
    const uint4* src = reinterpret_cast<const uint4*>(pool + (size_t)a.block_table[(size_t)src_row * a.max_pages + pi] * a.page_bytes);
    const int n16 = a.page_bytes / 16, per = (n16 + FK_Z - 1) / FK_Z;
    const int beg = blockIdx.z * per, end = min(beg + per, n16);
    for (int i = beg + threadIdx.x; i < end; i += 256) {
        const uint4 v = src[i];
        for (int d = 0; d < nd; ++d) {
            const int row = a.dst_rows[d0 + d];
            reinterpret_cast<uint4*>(pool + (size_t)a.block_table[(size_t)row * a.max_pages + pi] * a.page_bytes)[i] = v;
        }
    }
}

// one thread per 16-byte column piece of the logits rows, rows walked downwards: row i <- row lsrc[i].  With lsrc[i] <= i a row is read before any
// row above it is written, and no two threads share a column piece: in place, no staging buffer.
__global__ __launch_bounds__(256) void fork_logits_kernel(ForkArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.ld / 4) return;
    for (int i = a.n_rows - 1; i >= 0; --i) {
        const int s = a.lsrc[i];
        if (s == i) continue;
        reinterpret_cast<float4*>(a.logits + (size_t)i * a.ld)[c] = reinterpret_cast<const float4*>(a.logits + (size_t)s * a.ld)[c];
    }
}

void launch_fork_prompt(const ForkArgs& a, hipStream_t st) {
    fork_tail_copy_kernel<<<dim3(a.n_prompts, a.n_layer * a.n_kv, FK_Z), 256, 0, st>>>(a);
    fork_logits_kernel<<<(a.ld / 4 + 255) / 256, 256, 0, st>>>(a);
}

}  // namespace sv
