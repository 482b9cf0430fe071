// The extension pass (sv_prefill_extend, chunked prefill), the parts that are its own: the pages -> rows gather, the page writer that starts at a
// position other than 0, the host plan and its probe.  The layer loop is engine_forward.hip::extend_forward.
//
// Sequence b has ctx_b tokens in its pages and gets len_b own rows at positions ctx_b + j.  It stands for the solo sequence of T_b = ctx_b + len_b rows,
// and every own row must come out with the bits of a one-shot pass over a sequence of total_b >= T_b rows:
//   * LayerNorm, the ascending-k GEMM kernels, GELU, the embedding and RoPE are per row; a row's position is its solo index (launch_prefix_row_pos);
//   * the split-K remainder kernel takes the rows it takes in the solo pass of total_b rows: the last seq_peel_rows(total_b) of them where
//     gemm_seq_form(total_b, N, K, act) holds (extend_plan lists those that are own rows of this pass);
//   * the attention is the prefixed form of attn_prefill_kernel, one launch per sequence with a context: tiles, masks and the window are counted from
//     solo index 0, and solo index s is read at row s of the sequence's K | V buffer -- rows [0, ctx_b) gathered from the pages by kv_gather_kernel
//     (bf16 pages: the stored bits; e4m3 pages: what attn_decode_kernel sees), rows [ctx_b, T_b) the UNQUANTISED own rows, copied there by the writer.
//     The query tile that straddles ctx_b reads the up to q_tile - 1 Q rows in front of the sequence's first own row: the rows of the sequence packed in
//     front of it, or the zeroed pad in front of the buffer -- defined values; query rows are independent and "output rows with s < Pl are not stored";
//   * the pages: kv_write_extend_kernel writes the own tokens by the one-shot writer's rule (kv_write_prefill_kernel) and leaves every byte of a cached
//     token as it is, codes and scale bytes: a V piece that holds cached tokens is read, merged and written back by the one block that owns its group.
#include <algorithm>
#include "../engine_internal.h"
#include "../kv8/kv8_dev.h"

namespace sv {

// the bf16 page layout of attention.hip (kv_k_offset / kv_v_offset)
__device__ __forceinline__ size_t ext_k_offset(int D, int t64, int d) {
    const int kg = t64 >> 4, key = t64 & 15, s = d >> 5, c = (d >> 3) & 3, e = d & 7;
    return ((size_t)((kg * (D >> 5) + s) * 64 + c * 16 + key)) * 16 + e * 2;
}

// descriptor of one sequence of the pass: {block-table row, first packed own row, ctx, len, first row of its region of the K | V buffer or -1, 0};
// the region holds the solo rows [0, ctx + len)
#define XS 6

// Pages -> rows.  One block per (listed {sequence, 32-token group}, KV head): every wave-load is one contiguous 1 KiB piece of the page (a K fragment
// (key-group, k-step) or a V fragment (dv-tile)), every store 16 bytes of one token-major row.  K leaves from the registers it arrived in (a lane holds
// 8 consecutive dims of ONE key); V goes through LDS (a lane holds one dim of 8 keys).  Tokens >= ctx of the last group are not stored: those rows of
// the region are the own rows.
template <int KVF>
__global__ __launch_bounds__(256) void kv_gather_kernel(ExtKvArgs p) {
    extern __shared__ __attribute__((aligned(16))) char ext_smem[];
    bf16_t* Vs = reinterpret_cast<bf16_t*>(ext_smem);                 // [32][D + 8]
    const int D = p.head_dim, VST = D + 8, NK = D >> 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kvh = blockIdx.y;
    const int32_t* xs = p.xseq + XS * p.blocks[2 * blockIdx.x];
    const int g = p.blocks[2 * blockIdx.x + 1], tok0 = 32 * g, half = g & 1;
    const int b = xs[0], ctx = xs[2];
    const long long G = xs[4];
    const char* page = p.pool_layer + (size_t)kvh * p.kv_head_stride +
                       (size_t)p.table[(size_t)b * p.max_pages + (tok0 >> 6)] * (KVF ? kv8_page_bytes(D) : kv_page_bytes(D));
    bf16_t* kout = p.gkv + (size_t)(G + tok0) * p.gkv_stride + kvh * D;
    bf16_t* vout = kout + p.n_kv * D;
    const int key = lane & 15, c = lane >> 4;
    if constexpr (KVF != 0) {
        const unsigned char* sc = reinterpret_cast<const unsigned char*>(page + (size_t)128 * D);
        for (int s = wave; s < NK; s += 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(page + ((size_t)((half * NK + s) * 64 + lane)) * 16);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = 16 * u + key;
                if (tok0 + r < ctx)
                    *reinterpret_cast<u32x4*>(kout + (size_t)r * p.gkv_stride + 32 * s + 8 * c) =
                        kv8_widen8(v[2 * u], v[2 * u + 1], kv8_scale_f32(sc[32 * half + r]));
            }
        }
        for (int t2 = wave; t2 < NK; t2 += 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(page + (size_t)64 * D + ((size_t)((half * NK + t2) * 64 + lane)) * 16);
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ka = 16 * h + 4 * c + r;
                        Vs[ka * VST + 16 * (2 * t2 + tl) + key] = kv8_deq1(v[2 * tl + h] >> (8 * r), sc[64 + 32 * half + ka]);
                    }
        }
    } else {
        for (int w = wave; w < 2 * NK; w += 4) {
            const int kgl = w / NK, s = w - kgl * NK, r = 16 * kgl + key;
            const u32x4 v = *reinterpret_cast<const u32x4*>(page + ((size_t)(((2 * half + kgl) * NK + s) * 64 + lane)) * 16);
            if (tok0 + r < ctx) *reinterpret_cast<u32x4*>(kout + (size_t)r * p.gkv_stride + 32 * s + 8 * c) = v;
        }
        for (int t = wave; t < (D >> 4); t += 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(page + (size_t)64 * D * 2 + ((size_t)((half * (D >> 4) + t) * 64 + lane)) * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ka = 16 * (e >> 2) + 4 * c + (e & 3);
                Vs[ka * VST + 16 * t + key] = (bf16_t)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            }
        }
    }
    __syncthreads();
    const int NC = D >> 3;
    for (int i = tid; i < 32 * NC; i += 256) {
        const int r = i / NC, ch = i - r * NC;
        if (tok0 + r < ctx)
            *reinterpret_cast<uint4*>(vout + (size_t)r * p.gkv_stride + ch * 8) = *reinterpret_cast<const uint4*>(Vs + r * VST + ch * 8);
    }
}

// Own rows -> pages, from position ctx on.  One block per (listed {sequence, 32-token group}, KV head), groups ctx / 32 .. (ctx + len - 1) / 32.  A token
// of the group is cached (< ctx: every byte of it stays), own (written by kv_write_prefill_kernel's rule) or behind the new end (V = 0 / code 0 and
// scale byte 127, as that kernel leaves it).  The own rows' K | V also go, unquantised, to rows ctx + j of the sequence's region of the K | V buffer.
template <int KVF>
__global__ __launch_bounds__(256) void kv_write_extend_kernel(ExtKvArgs p) {
    extern __shared__ __attribute__((aligned(16))) char ext_smem[];
    bf16_t* Vs = reinterpret_cast<bf16_t*>(ext_smem);                 // bf16: V rows [32][D + 8]; e4m3: K rows, then V rows [64][D + 8], then [64] scale words
    const int D = p.head_dim, VST = D + 8, NC = D >> 3;
    const int tid = threadIdx.x, kvh = blockIdx.y;
    const int32_t* xs = p.xseq + XS * p.blocks[2 * blockIdx.x];
    const int g = p.blocks[2 * blockIdx.x + 1], tok0 = 32 * g, half = g & 1;
    const int b = xs[0], R = xs[1], ctx = xs[2], end = xs[2] + xs[3];
    const long long G = xs[4];
    char* page = p.pool_layer + (size_t)kvh * p.kv_head_stride +
                 (size_t)p.table[(size_t)b * p.max_pages + (tok0 >> 6)] * (KVF ? kv8_page_bytes(D) : kv_page_bytes(D));
    const int k_off = p.k_off + kvh * D, v_off = p.v_off + kvh * D;
    for (int i = tid; i < 32 * NC; i += 256) {
        const int r = i / NC, ch = i - r * NC, tok = tok0 + r;
        uint4 kq = make_uint4(0u, 0u, 0u, 0u), vq = kq;
        if (tok >= ctx && tok < end) {
            const bf16_t* src = p.qkv + (size_t)(R + tok - ctx) * p.row_stride;
            kq = *reinterpret_cast<const uint4*>(src + k_off + ch * 8);
            vq = *reinterpret_cast<const uint4*>(src + v_off + ch * 8);
            if (G >= 0) {
                bf16_t* dst = p.gkv + (size_t)(G + tok) * p.gkv_stride + kvh * D + ch * 8;
                *reinterpret_cast<uint4*>(dst) = kq;
                *reinterpret_cast<uint4*>(dst + p.n_kv * D) = vq;
            }
            if constexpr (KVF == 0) *reinterpret_cast<uint4*>(page + ext_k_offset(D, tok & 63, ch * 8)) = kq;
        }
        if constexpr (KVF != 0) {
            *reinterpret_cast<uint4*>(Vs + r * VST + ch * 8) = kq;
            *reinterpret_cast<uint4*>(Vs + (32 + r) * VST + ch * 8) = vq;
        } else {
            *reinterpret_cast<uint4*>(Vs + r * VST + ch * 8) = vq;
        }
    }
    __syncthreads();
    const bool mixed = tok0 < ctx;                                    // the group holds cached tokens: their part of every V piece is kept
    if constexpr (KVF != 0) {
        uint32_t* sb = reinterpret_cast<uint32_t*>(Vs + 64 * VST);
        {
            const int row = tid >> 2, q = tid & 3;                    // 64 rows x 4 threads
            uint32_t m = 0u;
            for (int d = q * (D >> 2); d < (q + 1) * (D >> 2); ++d) {
                const uint32_t a = kv8_mag(Vs[row * VST + d]);
                m = a > m ? a : m;
            }
            uint32_t o = __shfl_xor(m, 1, 64);
            m = o > m ? o : m;
            o = __shfl_xor(m, 2, 64);
            m = o > m ? o : m;
            if (q == 0) {
                const uint32_t byte = kv8_scale_byte(m);              // (a token behind the end is a row of zeros: 127)
                const int tok = tok0 + (row & 31), t64 = tok & 63;
                sb[row] = byte;
                if (tok >= ctx)
                    *reinterpret_cast<unsigned char*>(page + (row < 32 ? kv8_kscale_offset(D, t64) : kv8_vscale_offset(D, t64))) = (unsigned char)byte;
            }
        }
        __syncthreads();
        for (int i = tid; i < 32 * NC; i += 256) {
            const int r = i / NC, ch = i - r * NC;
            if (tok0 + r < ctx) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(Vs + r * VST + ch * 8);
            *reinterpret_cast<uint2*>(page + kv8_k_offset(D, (tok0 + r) & 63, ch * 8)) = kv8_code8(v, sb[r]);
        }
        for (int i = tid; i < (D >> 5) * 64; i += 256) {
            const int t2 = i >> 6, l = i & 63, dl = l & 15, c = l >> 4;
            uint4* piece = reinterpret_cast<uint4*>(page + (size_t)64 * D + ((size_t)((half * (D >> 5) + t2) * 64 + l)) * 16);
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (mixed) { const uint4 o = *piece; w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = o.w; }
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    uint32_t word = w[2 * tl + h];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ka = 16 * h + 4 * c + r;                   // element e = 4 h + r of the fragment
                        if (tok0 + ka < ctx) continue;
                        const uint32_t code = kv8_code(Vs[(32 + ka) * VST + 16 * (2 * t2 + tl) + dl], sb[32 + ka]);
                        word = (word & ~(0xffu << (8 * r))) | (code << (8 * r));
                    }
                    w[2 * tl + h] = word;
                }
            *piece = make_uint4(w[0], w[1], w[2], w[3]);
        }
        return;
    }
    for (int i = tid; i < (D >> 4) * 64; i += 256) {
        const int t = i >> 6, l = i & 63, dl = l & 15, c = l >> 4;
        uint4* piece = reinterpret_cast<uint4*>(page + (size_t)64 * D * 2 + ((size_t)((half * (D >> 4) + t) * 64 + l)) * 16);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (mixed) { const uint4 o = *piece; w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = o.w; }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ka = 16 * (e >> 2) + 4 * c + (e & 3);
            if (tok0 + ka < ctx) continue;
            const uint32_t sh = 16 * (e & 1);
            w[e >> 1] = (w[e >> 1] & ~(0xffffu << sh)) | ((uint32_t)Vs[ka * VST + 16 * t + dl] << sh);
        }
        *piece = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

void launch_kv_gather(const ExtKvArgs& a, hipStream_t st) {
    if (a.n_blocks < 1) return;
    const size_t smem = (size_t)32 * (a.head_dim + 8) * 2;
    if (a.kv_fmt) kv_gather_kernel<1><<<dim3(a.n_blocks, a.n_kv), 256, smem, st>>>(a);
    else kv_gather_kernel<0><<<dim3(a.n_blocks, a.n_kv), 256, smem, st>>>(a);
}
void launch_kv_write_extend(const ExtKvArgs& a, hipStream_t st) {
    if (a.n_blocks < 1) return;
    if (a.kv_fmt) kv_write_extend_kernel<1><<<dim3(a.n_blocks, a.n_kv), 256, (size_t)64 * (a.head_dim + 8) * 2 + 64 * 4, st>>>(a);
    else kv_write_extend_kernel<0><<<dim3(a.n_blocks, a.n_kv), 256, (size_t)32 * (a.head_dim + 8) * 2, st>>>(a);
}
}  // namespace sv

// ------------------------------------------------------------------------------------------------
// host plan
// ------------------------------------------------------------------------------------------------
// the passes of a call under a row budget (0: one pass): sequences walked in order, each takes what the budget leaves; take[pass][b] rows
void sveng::extend_schedule(const int32_t* lens, int B, int budget, std::vector<std::vector<int32_t>>& take) {
    take.clear();
    std::vector<int32_t> left(lens, lens + B);
    for (int b = 0; b < B;) {
        std::vector<int32_t> t((size_t)B, 0);
        int room = budget > 0 ? budget : INT32_MAX;
        while (b < B && room > 0) {
            const int n = std::min(left[b], room);
            t[b] = n; left[b] -= n; room -= n;
            if (left[b] == 0) ++b; else break;
        }
        while (b < B && left[b] == 0) ++b;      // (sequences of length 0: nothing to take)
        take.push_back(std::move(t));
    }
}

void sveng::extend_plan(const ExtendSeq* seqs, int B, int q_tile, const PlanProj* proj, int n_proj, ExtendPass& out) {
    out = ExtendPass();
    out.B = B;
    int R = 0;
    long long G = 0;
    for (int b = 0; b < B; ++b) {
        const int ctx = seqs[b].ctx, len = seqs[b].len, total = seqs[b].total, T = ctx + len;
        if (len < 1) continue;
        const int x = (int)out.list[XL_XSEQ].size() / 6;
        const bool fin = T == total;
        const int32_t xs[6] = {b, R, ctx, len, ctx > 0 ? (int32_t)G : -1, 0};
        out.list[XL_XSEQ].insert(out.list[XL_XSEQ].end(), xs, xs + 6);
        const int32_t seg[3] = {R, len, ctx};
        out.list[XL_SEG].insert(out.list[XL_SEG].end(), seg, seg + 3);
        for (int g = ctx / 32; g <= (T - 1) / 32; ++g) { out.list[XL_WRITE].push_back(x); out.list[XL_WRITE].push_back(g); }
        const int n_tiles = (T + q_tile - 1) / q_tile;
        if (ctx > 0) {
            for (int g = 0; g < (ctx + 31) / 32; ++g) { out.list[XL_GATHER].push_back(x); out.list[XL_GATHER].push_back(g); }
            ExtendPass::CtxSeq cs;
            cs.b = b; cs.region = G; cs.index_row0 = R - ctx; cs.fin = fin;
            cs.seq_off = (int)out.list[XL_CTX_SEQ].size(); cs.blocks_off = (int)out.list[XL_CTX_BLOCKS].size();
            const int32_t d[4] = {R, T, R - ctx, ctx};
            out.list[XL_CTX_SEQ].insert(out.list[XL_CTX_SEQ].end(), d, d + 4);
            // query tiles counted from solo index 0; the first listed tile is the one that holds row ctx (it may straddle the context's end);
            // every launch sees its own sequence as sequence 0
            for (int t = ctx / q_tile; t < n_tiles; ++t) { out.list[XL_CTX_BLOCKS].push_back(0); out.list[XL_CTX_BLOCKS].push_back(t); }
            cs.n_blocks = n_tiles - ctx / q_tile;
            out.ctx_seqs.push_back(cs);
            G += T;
        } else {
            const int ps = (int)out.list[XL_PLAIN_SEQ].size() / 2;
            out.list[XL_PLAIN_SEQ].push_back(R); out.list[XL_PLAIN_SEQ].push_back(len);
            for (int t = 0; t < n_tiles; ++t) { out.list[XL_PLAIN_BLOCKS].push_back(ps); out.list[XL_PLAIN_BLOCKS].push_back(t); }
            if (fin) { out.list[XL_PLAIN_LAST].push_back(ps); out.list[XL_PLAIN_LAST].push_back(n_tiles - 1); }
        }
        const int fi = (int)out.fin.size();
        if (fin) { out.fin.push_back(b); out.list[XL_FIN].push_back(R); out.list[XL_FIN].push_back(len); }
        // the remainder rows of the solo pass of `total` rows that are own rows of this pass
        const int r = seq_peel_rows(total);
        for (int i = 0; i < n_proj && r > 0; ++i) {
            if (!gemm_seq_form(total, proj[i].N, proj[i].K, proj[i].act)) continue;
            for (int s = std::max(total - r, ctx); s < std::min(total, T); ++s) out.rows(i).push_back(R + s - ctx);
            if (fin) out.last(i).push_back(fi);
        }
        R += len;
    }
    out.M = R;
    out.gkv_rows = G;
}

// What an extension call decides, for ONE projection (N, K, act): the call's passes under `budget` (0: one pass) and per pass its sequences, remainder
// rows, attention tiles and page groups.  out (int32, `capacity` of them; *out_n = how many were written, or are needed when SV_EINVAL says capacity):
//   n_passes, then per pass:  n_seq, {b, ctx, len, first packed row} x n_seq | n_rows, packed row x n_rows | n_tiles, {b, tile} x n_tiles |
//                             n_groups, {b, 32-token group} x n_groups | n_fin, b x n_fin
extern "C" int sv_debug_extend_plan(const int32_t* ctx, const int32_t* lens, const int32_t* totals, int32_t B, int32_t budget, int32_t N, int32_t K,
                                    int32_t act, int32_t q_tile, int32_t* out, int32_t capacity, int32_t* out_n) {
    const char* who = "sv_debug_extend_plan";
    if (!ctx || !lens || !out || !out_n) return fail(SV_EINVAL, "%s: null argument", who);
    if (B < 1 || budget < 0 || N < 1 || K < 1 || (q_tile != 32 && q_tile != 128))
        return fail(SV_EINVAL, "%s: bad argument (B %d, budget %d, N %d, K %d, q_tile %d)", who, B, budget, N, K, q_tile);
    long long rows = 0;
    for (int b = 0; b < B; ++b) {
        if (ctx[b] < 0 || lens[b] < 0) return fail(SV_EINVAL, "%s: context %d / length %d of sequence %d", who, ctx[b], lens[b], b);
        if (totals && totals[b] < ctx[b] + lens[b]) return fail(SV_EINVAL, "%s: total %d of sequence %d < context %d + length %d", who, totals[b], b, ctx[b], lens[b]);
        rows += (long long)ctx[b] + lens[b];
    }
    if (rows > (1 << 24)) return fail(SV_EINVAL, "%s: %lld rows: more than this test surface takes", who, rows);
    std::vector<std::vector<int32_t>> take;
    extend_schedule(lens, B, budget, take);
    std::vector<int32_t> o;
    o.push_back((int32_t)take.size());
    std::vector<int32_t> at(ctx, ctx + B);
    const PlanProj pj{N, K, act};
    for (const std::vector<int32_t>& t : take) {
        std::vector<ExtendSeq> seqs((size_t)B);
        for (int b = 0; b < B; ++b) seqs[b] = {at[b], t[b], totals ? totals[b] : ctx[b] + lens[b]};
        ExtendPass p;
        extend_plan(seqs.data(), B, q_tile, &pj, 1, p);
        const std::vector<int32_t>& xs = p.list[XL_XSEQ];
        const auto seq_b = [&](int x) { return xs[6 * x]; };
        o.push_back((int32_t)xs.size() / 6);
        for (size_t x = 0; x < xs.size() / 6; ++x) { o.push_back(xs[6 * x]); o.push_back(xs[6 * x + 2]); o.push_back(xs[6 * x + 3]); o.push_back(xs[6 * x + 1]); }
        o.push_back((int32_t)p.rows(0).size());
        o.insert(o.end(), p.rows(0).begin(), p.rows(0).end());
        std::vector<int32_t> tiles, plain_b;      // plain_b: the call's sequence behind every entry of XL_PLAIN_SEQ
        for (size_t x = 0; x < xs.size() / 6; ++x) if (xs[6 * x + 2] == 0) plain_b.push_back(seq_b((int)x));
        for (size_t i = 0; i + 1 < p.list[XL_PLAIN_BLOCKS].size(); i += 2) {
            tiles.push_back(plain_b[p.list[XL_PLAIN_BLOCKS][i]]); tiles.push_back(p.list[XL_PLAIN_BLOCKS][i + 1]);
        }
        for (const ExtendPass::CtxSeq& cs : p.ctx_seqs)
            for (int i = 0; i < cs.n_blocks; ++i) { tiles.push_back(cs.b); tiles.push_back(p.list[XL_CTX_BLOCKS][cs.blocks_off + 2 * i + 1]); }
        o.push_back((int32_t)tiles.size() / 2);
        o.insert(o.end(), tiles.begin(), tiles.end());
        o.push_back((int32_t)p.list[XL_WRITE].size() / 2);
        for (size_t i = 0; i + 1 < p.list[XL_WRITE].size(); i += 2) { o.push_back(seq_b(p.list[XL_WRITE][i])); o.push_back(p.list[XL_WRITE][i + 1]); }
        o.push_back((int32_t)p.fin.size());
        o.insert(o.end(), p.fin.begin(), p.fin.end());
        for (int b = 0; b < B; ++b) at[b] += t[b];
    }
    *out_n = (int32_t)o.size();
    if ((size_t)(capacity < 0 ? 0 : capacity) < o.size()) return fail(SV_EINVAL, "%s: capacity %d < %zu", who, capacity, o.size());
    std::copy(o.begin(), o.end(), out);
    return 0;
}

// tokens [0, count) of decode row `row` of `layer` through kv_gather_kernel -- the launch an extension pass makes -- into dev_out_bf16
// [count][2 * n_kv * head_dim] (k heads | v heads): bit for bit what sv_debug_kv_read returns for them
extern "C" int sv_debug_kv_gather(sv_engine* e, int32_t layer, int32_t row, int32_t count, void* dev_out_bf16, sv_stream stream) {
    if (!e || !dev_out_bf16) return fail(SV_EINVAL, "sv_debug_kv_gather: null argument");
    const sv_config& c = e->cfg;
    if (layer < 0 || layer >= c.n_layer || row < 0 || row >= c.max_batch || count < 1 || count > c.max_seq_len)
        return fail(SV_EINVAL, "sv_debug_kv_gather: bad layer %d / row %d / count %d (max_batch %d, max_seq_len %d)", layer, row, count, c.max_batch, c.max_seq_len);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHECK(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> img = {row, 0, count, 0, 0, 0};
    for (int g = 0; g < (count + 31) / 32; ++g) { img.push_back(0); img.push_back(g); }
    int32_t* d = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d), img.size() * sizeof(int32_t)));
    int rc = 0;
    if (hipMemcpy(d, img.data(), img.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) rc = fail(SV_EHIP, "sv_debug_kv_gather: upload failed");
    if (!rc) {
        ExtKvArgs a = extend_kv_args(e, layer, e->block_table, d, d + 6, (count + 31) / 32, (bf16_t*)dev_out_bf16);
        launch_kv_gather(a, st);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = fail(SV_EHIP, "sv_debug_kv_gather: launch failed");
    }
    (void)hipFree(d);
    return rc;
}
