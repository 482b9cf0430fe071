// The prefix cache of the continuous batch (sv_cb_set_prefix_cache), the parts that are its own: the page digests on the device, the host arithmetic
// of the keys, and their probes.  The table, the holder counts, the LRU list and the admit path are engine_cb.hip's.
//
// Prompts reach the engine as embedding rows, so the key of a KV page comes from the rows themselves.
//
// Digest.  A full page of a prompt is 64 consecutive packed rows of `hidden` bf16 = 16 * hidden little-endian 64-bit words w_0 .. w_{n-1} (word i =
// elements 4 i .. 4 i + 3 of the page, element 0 in the low 16 bits).  With
//     mix64(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31        (splitmix64's finaliser)
//     C1 = 0x9E3779B97F4A7C15, C2 = 0xC2B2AE3D27D4EB4F, C3 = 0x165667B19E3779F9                                        (all arithmetic mod 2^64)
// the digest is the pair
//     a = SUM_i mix64(w_i + (i + 1) * C1)            b = XOR_i mix64((w_i ^ C3) + (i + 1) * C2)
// Every bit of every word enters through a bijection that also takes the word's index, so flipping a bit, or swapping two rows or two elements,
// changes the digest (up to a 2^-128 accident); SUM and XOR are commutative, so the result does not depend on how the launch splits the words among
// lanes, waves or blocks.  The digest depends on the page's own bytes alone: not on where the prompt lies in the packed buffer, not on its neighbours.
//
// Chaining (host).  key_k = chain(key_{k-1}, digest_k):  key_k.a = mix64((key_{k-1}.a ^ d.a) + C1),  key_k.b = mix64((key_{k-1}.b + d.b) ^ key_k.a),
// key_{-1} = (0x5356505243414348, 0x7061676564696731).  key_k stands for "these exact rows at positions 64 k .. 64 k + 63 behind exactly this prefix".
//
// Collisions.  A hit is NOT verified against the rows: two different prefixes with the same 128-bit key would share pages.  (vLLM's prefix cache
// trusts its block hashes the same way.)  tests/prefix_key_ref.py restates all of the above in numpy.
#include "../engine_internal.h"

namespace sv {

#define PC_C1 0x9E3779B97F4A7C15ull
#define PC_C2 0xC2B2AE3D27D4EB4Full
#define PC_C3 0x165667B19E3779F9ull

__host__ __device__ __forceinline__ uint64_t pc_mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

struct PageDigestArgs {
    const uint4* embeds;       // packed rows, hidden / 8 16-byte pieces each
    const int32_t* desc;       // {first packed row, len} per prompt; nullptr: prompt u = rows [u * S0, (u + 1) * S0)
    int S0, pieces_per_row, max_pages;
    uint64_t* out;             // [prompts][max_pages][2]
};

__device__ __forceinline__ uint64_t pc_shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// One block per (page k, prompt u); blocks with k >= len_u / 64 leave at once (the partial tail page has no digest).  A page is one contiguous
// piece of the packed buffer: every lane walks it in 16-byte loads, each row read once, and keeps its own (sum, xor); the block's 256 pairs
// are folded through shuffles and 4 LDS slots, lane 0 stores the pair with one 16-byte store.
__global__ __launch_bounds__(256) void page_digest_kernel(PageDigestArgs p) {
    __shared__ uint64_t part[4][2];
    const int u = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
    const long long row0 = p.desc ? p.desc[2 * u] : (long long)u * p.S0;
    const int len = p.desc ? p.desc[2 * u + 1] : p.S0;
    if (k >= len / SV_PAGE_TOKENS) return;
    const uint4* src = p.embeds + (size_t)(row0 + (long long)SV_PAGE_TOKENS * k) * p.pieces_per_row;
    const int nq = SV_PAGE_TOKENS * p.pieces_per_row;
    uint64_t a = 0, b = 0;
#pragma unroll 4
    for (int q = tid; q < nq; q += 256) {
        const uint4 v = src[q];
        const uint64_t w0 = ((uint64_t)v.y << 32) | v.x, w1 = ((uint64_t)v.w << 32) | v.z;
        const uint64_t i0 = 2ull * q + 1, i1 = i0 + 1;
        a += pc_mix64(w0 + i0 * PC_C1) + pc_mix64(w1 + i1 * PC_C1);
        b ^= pc_mix64((w0 ^ PC_C3) + i0 * PC_C2) ^ pc_mix64((w1 ^ PC_C3) + i1 * PC_C2);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { a += pc_shfl_xor64(a, m); b ^= pc_shfl_xor64(b, m); }
    if ((tid & 63) == 0) { part[tid >> 6][0] = a; part[tid >> 6][1] = b; }
    __syncthreads();
    if (tid == 0) {
        a = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        b = part[0][1] ^ part[1][1] ^ part[2][1] ^ part[3][1];
        *reinterpret_cast<uint4*>(p.out + 2 * ((size_t)u * p.max_pages + k)) =
            make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
}
}  // namespace sv

int sveng::pc_launch_digests(const bf16_t* embeds, int n, const int32_t* dev_desc, int S0, int hidden, int max_pages, uint64_t* dev_out, hipStream_t st) {
    if (n < 1 || max_pages < 1) return 0;
    PageDigestArgs a;
    a.embeds = reinterpret_cast<const uint4*>(embeds); a.desc = dev_desc; a.S0 = S0; a.pieces_per_row = hidden / 8; a.max_pages = max_pages; a.out = dev_out;
    page_digest_kernel<<<dim3(max_pages, n), 256, 0, st>>>(a);
    HIPCHECK(hipGetLastError());
    return 0;
}

PcKey sveng::pc_key0() { return PcKey{0x5356505243414348ull, 0x7061676564696731ull}; }
PcKey sveng::pc_chain(const PcKey& prev, const PcKey& d) {
    PcKey k;
    k.a = pc_mix64((prev.a ^ d.a) + PC_C1);
    k.b = pc_mix64((prev.b + d.b) ^ k.a);
    return k;
}

// ------------------------------------------------------------------------------------------------
// probes (include/starvector_hip_debug.h)
// ------------------------------------------------------------------------------------------------
// the digest launch on its own, no engine: host_out [n][max_pages][2], entry (u, k) = the digest of page k of prompt u, zeros for k >= len_u / 64
extern "C" int sv_debug_page_digests(const void* dev_embeds_packed, int32_t n, const int32_t* host_lens, int32_t S0, int32_t hidden, int32_t max_pages,
                                     uint64_t* host_out, sv_stream stream) {
    const char* who = "sv_debug_page_digests";
    if (!dev_embeds_packed || !host_out) return fail(SV_EINVAL, "%s: null argument", who);
    if (n < 1 || n > 4096 || hidden < 8 || hidden % 8 != 0 || max_pages < 1)
        return fail(SV_EINVAL, "%s: bad argument (n %d in 1..4096, hidden %d a multiple of 8, max_pages %d >= 1)", who, n, hidden, max_pages);
    if (((uintptr_t)dev_embeds_packed & 15) != 0) return fail(SV_EINVAL, "%s: the packed rows must be 16-byte aligned", who);
    if (!host_lens && S0 < 1) return fail(SV_EINVAL, "%s: bad prompt length %d", who, S0);
    std::vector<int32_t> desc;
    long long row = 0;
    for (int u = 0; u < n; ++u) {
        const int len = host_lens ? host_lens[u] : S0;
        if (len < 1) return fail(SV_EINVAL, "%s: prompt %d: bad prompt length %d", who, u, len);
        if (len / SV_PAGE_TOKENS > max_pages) return fail(SV_EINVAL, "%s: prompt %d: %d full pages exceed max_pages %d", who, u, len / SV_PAGE_TOKENS, max_pages);
        desc.push_back((int32_t)row); desc.push_back(len);
        row += len;
        if (row > INT32_MAX) return fail(SV_EINVAL, "%s: more than 2^31 packed rows", who);
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t words = (size_t)n * max_pages * 2;
    uint64_t* d_out = nullptr;
    int32_t* d_desc = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_out), words * sizeof(uint64_t)));
    int rc = 0;
    if (hipMalloc(reinterpret_cast<void**>(&d_desc), desc.size() * sizeof(int32_t)) != hipSuccess) rc = fail(SV_EHIP, "%s: allocation failed", who);
    if (!rc && (hipMemsetAsync(d_out, 0, words * sizeof(uint64_t), st) != hipSuccess ||
                hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess))
        rc = fail(SV_EHIP, "%s: upload failed", who);
    if (!rc) rc = pc_launch_digests((const bf16_t*)dev_embeds_packed, n, host_lens ? d_desc : nullptr, S0, hidden, max_pages, d_out, st);
    if (!rc && (hipMemcpyAsync(host_out, d_out, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
        rc = fail(SV_EHIP, "%s: launch failed: %s", who, hipGetErrorString(hipGetLastError()));
    (void)hipFree(d_out);
    if (d_desc) (void)hipFree(d_desc);
    return rc;
}

// Host arithmetic, no device: the keys of a prompt of L rows from its L / 64 page digests, and the pages an admit would reuse against a table that
// holds `n_table` keys: h = min(leading keys found in the table, (L - 1) / 64).  host_keys_out [L / 64][2] may be NULL.
extern "C" int sv_debug_prefix_hit(const uint64_t* host_digests, int32_t n_pages, int32_t L, const uint64_t* host_table_keys, int32_t n_table,
                                   uint64_t* host_keys_out, int32_t* h_out) {
    const char* who = "sv_debug_prefix_hit";
    if (!h_out || (n_pages > 0 && !host_digests) || (n_table > 0 && !host_table_keys)) return fail(SV_EINVAL, "%s: null argument", who);
    if (L < 1 || n_pages != L / SV_PAGE_TOKENS || n_table < 0)
        return fail(SV_EINVAL, "%s: a prompt of %d rows has %d full pages (%d digests given; n_table %d)", who, L, L < 1 ? 0 : L / SV_PAGE_TOKENS, n_pages, n_table);
    PcKey key = pc_key0();
    int matched = 0;
    bool run = true;
    for (int k = 0; k < n_pages; ++k) {
        key = pc_chain(key, PcKey{host_digests[2 * k], host_digests[2 * k + 1]});
        if (host_keys_out) { host_keys_out[2 * k] = key.a; host_keys_out[2 * k + 1] = key.b; }
        bool found = false;
        for (int t = 0; run && t < n_table && !found; ++t) found = host_table_keys[2 * t] == key.a && host_table_keys[2 * t + 1] == key.b;
        if (run && found) ++matched; else run = false;
    }
    *h_out = pc_hit_pages(matched, L);
    return 0;
}
