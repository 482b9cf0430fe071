// The shared-prefix scoring pass (sv_forward_logprobs_prefixed), the parts that are its own: the host plan and the row-position builder.
//
// P prefixes (the visual rows of P images) and the own rows of B sequences (G completions per image) travel through the decoder in ONE packed
// buffer, prefixes first.  Sequence b stands for the solo sequence concat(prefix[prefix_of[b]], own rows of b) of T_b = Pl + len_b rows, and every
// kept row must come out with the bits of that solo run.  A prefix row is computed once, so it must have ONE value whoever shares it:
//   * LayerNorm, the ascending-k GEMM kernels, GELU and the embedding are per row;
//   * a row's position (wpe / RoPE) is its solo index: j in a prefix, Pl + j in own rows (prefix_row_pos_kernel);
//   * the attention reads a solo index through one indirection (attn_prefill_kernel<.., PFX>), tiles counted from solo index 0;
//   * the split-K remainder kernel (its own K order) computes the last seq_peel_rows(T_b) rows of a solo run wherever gemm_seq_form(T_b, N, K, act)
//     holds: those are listed among the OWN rows only.  If they would reach below Pl the prefix row would need different bits for different
//     sharers: the call is refused (PackedPlan::refused).  A prefix is never listed by its own length (a 257-row prefix has no peel row here).
#include <algorithm>
#include "../engine_internal.h"

namespace sv {
__global__ void prefix_row_pos_kernel(const int32_t* __restrict__ seg, int32_t* __restrict__ row_pos) {
    const int r0 = seg[3 * blockIdx.x], len = seg[3 * blockIdx.x + 1], pos0 = seg[3 * blockIdx.x + 2];
    for (int j = threadIdx.x; j < len; j += blockDim.x) row_pos[r0 + j] = pos0 + j;
}
void launch_prefix_row_pos(const int32_t* seg, int n_seg, int32_t* row_pos, hipStream_t st) {
    if (n_seg < 1) return;
    prefix_row_pos_kernel<<<n_seg, 256, 0, st>>>(seg, row_pos);
}
}  // namespace sv

int sveng::prefix_check(const char* who, const int32_t* prefix_lens, int P, const int32_t* lens, const int32_t* prefix_of, int B, const int32_t* keep) {
    if (P < 1 || B < P) return fail(SV_EINVAL, "%s: bad P=%d / B=%d (1 <= P <= B)", who, P, B);
    for (int u = 0; u < P; ++u)
        if (prefix_lens[u] < 1) return fail(SV_EINVAL, "%s: length %d of prefix %d (must be >= 1)", who, prefix_lens[u], u);
    std::vector<char> used((size_t)P, 0);
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) return fail(SV_EINVAL, "%s: length %d of sequence %d (must be >= 1)", who, lens[b], b);
        if (prefix_of[b] < 0 || prefix_of[b] >= P) return fail(SV_EINVAL, "%s: prefix_of %d of sequence %d outside 0..%d", who, prefix_of[b], b, P - 1);
        if (keep && (keep[b] < 1 || keep[b] > lens[b] + 1))
            return fail(SV_EINVAL, "%s: keep %d of sequence %d must be in 1..its length + 1 (%d)", who, keep[b], b, lens[b] + 1);
        used[prefix_of[b]] = 1;
    }
    for (int u = 0; u < P; ++u)
        if (!used[u]) return fail(SV_EINVAL, "%s: prefix %d is used by no sequence", who, u);
    return 0;
}

// The prefixes travel as ordinary ragged sequences (PL_SEQ0 = {first packed row, Pl}) through the first attention launch, the sequences through the
// second one in the prefixed form; no K / V page is written and no layer is pruned.
void sveng::prefix_plan(const int32_t* prefix_lens, int P, const int32_t* lens, const int32_t* prefix_of, int B, int q_tile, const PlanProj* proj,
                        int n_proj, const int32_t* keep, PackedPlan& out) {
    out = PackedPlan();
    out.B = B; out.n_seg = P + B; out.n_attn = 2; out.tail = PackedPlan::SCORE_LISTED_ROWS;
    std::vector<int32_t>&seg = out.list[PL_DESC], &pseq = out.list[PL_SEQ0], &sseq = out.list[PL_SEQ1], &sblocks = out.list[PL_BLOCKS1],
                        &kept = out.list[PL_KEPT];
    std::vector<int32_t> prow0((size_t)P);
    int r0 = 0;
    for (int u = 0; u < P; ++u) {
        prow0[u] = r0;
        const int32_t s[3] = {r0, prefix_lens[u], 0};
        seg.insert(seg.end(), s, s + 3);
        pseq.push_back(r0); pseq.push_back(prefix_lens[u]);
        r0 += prefix_lens[u];
    }
    out.src_rows[0] = r0;
    ragged_blocks(prefix_lens, P, q_tile, false, out.list[PL_BLOCKS0]);
    for (int b = 0; b < B; ++b) {
        const int p0 = prow0[prefix_of[b]], pl = prefix_lens[prefix_of[b]], T = pl + lens[b];
        const int32_t s[3] = {r0, lens[b], pl};
        seg.insert(seg.end(), s, s + 3);
        const int32_t d[4] = {r0, T, p0, pl};
        sseq.insert(sseq.end(), d, d + 4);
        // query tiles counted from solo index 0; the first listed tile is the one that holds row Pl (it may straddle the prefix's end)
        for (int t = pl / q_tile, n = (T + q_tile - 1) / q_tile; t < n; ++t) { sblocks.push_back(b); sblocks.push_back(t); }
        const int r = seq_peel_rows(T);
        for (int i = 0; i < n_proj && r > 0; ++i) {
            if (!gemm_seq_form(T, proj[i].N, proj[i].K, proj[i].act)) continue;
            if (lens[b] < r) {
                if (out.refused < 0) { out.refused = b; out.refused_proj = i; }
                continue;
            }
            for (int j = lens[b] - r; j < lens[b]; ++j) out.rows(i).push_back(r0 + j);
        }
        for (int s = keep ? T - keep[b] : T; s < T; ++s) kept.push_back(s < pl ? p0 + s : r0 + s - pl);
        r0 += lens[b];
    }
    out.M = r0; out.src_rows[1] = r0 - out.src_rows[0];
    out.kept = (int)kept.size();
}

// the plan for ONE projection (N, K, act): row_pos_out [capacity] the solo index of every packed row, rows_out [capacity] its remainder rows,
// blocks_out [capacity] the {sequence, query tile} pairs of the prefixed attention launch; out4 = {remainder rows, blocks, refused sequence or -1,
// packed rows}.  capacity >= max(packed rows, 3 B, 2 x blocks): SV_EINVAL naming the need otherwise.
extern "C" int sv_debug_prefix_plan(const int32_t* prefix_lens, int32_t P, const int32_t* lens, const int32_t* prefix_of, int32_t B, int32_t N,
                                    int32_t K, int32_t act, int32_t q_tile, int32_t* row_pos_out, int32_t* rows_out, int32_t* blocks_out,
                                    int32_t capacity, int32_t* out4) {
    const char* who = "sv_debug_prefix_plan";
    if (!prefix_lens || !lens || !prefix_of || !row_pos_out || !rows_out || !blocks_out || !out4) return fail(SV_EINVAL, "%s: null argument", who);
    if (N < 1 || K < 1 || (q_tile != 32 && q_tile != 128)) return fail(SV_EINVAL, "%s: bad argument (N %d, K %d, q_tile %d)", who, N, K, q_tile);
    SVCHECK(prefix_check(who, prefix_lens, P, lens, prefix_of, B, nullptr));
    long long total = 0;
    for (int u = 0; u < P; ++u) total += prefix_lens[u];
    for (int b = 0; b < B; ++b) total += lens[b];
    if (total > (1 << 24)) return fail(SV_EINVAL, "%s: %lld rows: more than this test surface takes", who, total);
    PackedPlan pp;
    const PlanProj pj{N, K, act};
    prefix_plan(prefix_lens, P, lens, prefix_of, B, q_tile, &pj, 1, nullptr, pp);
    const std::vector<int32_t>&seg = pp.list[PL_DESC], &rows = pp.rows(0), &sblocks = pp.list[PL_BLOCKS1];
    const size_t need = std::max<size_t>(std::max<size_t>((size_t)pp.M, (size_t)3 * B), sblocks.size());
    if ((size_t)(capacity < 0 ? 0 : capacity) < need) return fail(SV_EINVAL, "%s: capacity %d < %zu", who, capacity, need);
    for (size_t i = 0; i + 2 < seg.size(); i += 3)
        for (int j = 0; j < seg[i + 1]; ++j) row_pos_out[seg[i] + j] = seg[i + 2] + j;
    std::copy(rows.begin(), rows.end(), rows_out);
    std::copy(sblocks.begin(), sblocks.end(), blocks_out);
    out4[0] = (int32_t)rows.size(); out4[1] = (int32_t)sblocks.size() / 2; out4[2] = pp.refused; out4[3] = pp.M;
    return 0;
}
