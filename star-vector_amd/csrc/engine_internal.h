// Internal header of the host driver (engine_*.hip): engine state, error plumbing and the functions the translation units
// share.  Not part of the C ABI (include/starvector_hip.h is); nothing here is exported by name to callers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/starvector_hip.h"
#include "../../include/starvector_hip_debug.h"
#include "kernels.h"
#include "beam.h"

using namespace sv;

// ------------------------------------------------------------------------------------------------
// errors (engine_core.hip owns the thread-local message)
// ------------------------------------------------------------------------------------------------
namespace sveng {
std::string& last_error();
int fail(int code, const char* fmt, ...);
}  // namespace sveng
using sveng::fail;
#define g_err (sveng::last_error())
#define HIPCHECK(x)                                                                              \
    do {                                                                                         \
        hipError_t _e = (x);                                                                     \
        if (_e != hipSuccess)                                                                    \
            return fail(SV_EHIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define SVCHECK(x)          \
    do {                    \
        int _r = (x);       \
        if (_r) return _r;  \
    } while (0)

// ------------------------------------------------------------------------------------------------
// engine state
// ------------------------------------------------------------------------------------------------
struct Linear {
    bf16_t* Wp = nullptr;
    bf16_t* bias = nullptr;
    int wfmt = SV_WFMT_BF16;   // weight format (kernels.h SV_WFMT_*): decoder weights quantised at load when sv_config.weight_dtype != 0
    uint8_t* Wq = nullptr;     //   fp8: decode image (launch_pack_weight_fp8); Wp then holds the SAME q values as bf16
    float* wscale = nullptr;   //   fp8: per-output-row scale [Npad]
    uint8_t* W4 = nullptr;     //   mxfp4: decode image (launch_pack_weight_mxfp4); Wp then holds the dequantised values (no scale)
    int N = 0, K = 0, Npad = 0, Kpad = 0;
    int splitk = 1;       // decode-path split-K factor (fp32 slabs summed by the consumer)
    int col_tiles = 1;    // column tiles per block of the two-row-tile decode kernel (33..64 rows; pick_decode_plan)
    int cpb = 8;          // output columns per block of the slab-free output projection (decode_cols.hip)
    bf16_t* Wf = nullptr; // LayerNorm-folded image W' = bf16(W * gamma) (decode_cols.hip; c_fc only), with
    float* c1 = nullptr;  //   c1[n] = sum_k W'[n][k]
    float* c2 = nullptr;  //   c2[n] = sum_k beta[k] W[n][k] + bias[n]
};
struct LNp { bf16_t* g = nullptr; bf16_t* b = nullptr; };
struct VitLayer { LNp ln1, ln2; Linear in_proj, out_proj, c_fc, c_proj; };
struct DecLayer { LNp ln1, ln2; Linear c_attn, c_proj, c_fc, c_proj2; };

enum SlotKind { SLOT_LINEAR_W, SLOT_RAW, SLOT_WTE };
struct Slot {
    SlotKind kind;
    Linear* lin = nullptr;
    bf16_t** raw = nullptr;
    size_t numel = 0;
    bool loaded = false;
    bool required = true;
    int row_off = 0;          // fused projections (q|k|v): first output row of this part inside the Linear
    int part_rows = 0;        // rows of this part (0 = the whole tensor)
};

// An owned captured decode step: the hipGraph, its instantiation and what it was captured for.  Move-only; the handles go with the slot.
struct GraphSlot {
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;      // nullptr: nothing kept (the caller runs plain launches of the same kernels)
    std::string key;
    GraphSlot() = default;
    GraphSlot(GraphSlot&& o) noexcept : g(o.g), x(o.x), key(std::move(o.key)) { o.g = nullptr; o.x = nullptr; }
    ~GraphSlot() { drop(); }
    void drop() {
        if (x) (void)hipGraphExecDestroy(x);
        if (g) (void)hipGraphDestroy(g);
        g = nullptr; x = nullptr; key.clear();
    }
    bool holds(const std::string& k) const { return x && key == k; }
    // the kept graph if it was captured for `k`; otherwise what the slot holds is dropped and `copies` calls of one_step are captured in its place
    // (capture_steps, below: a failure that is no error leaves the slot empty).  engine_core.hip
    int use(const std::string& k, hipStream_t st, int copies, const std::function<void()>& one_step, bool required = true);
};

// sv_engine::h_flags, the pinned words the device's flags are copied into: the done flag, the emitted count, the continuous batch's live count, the
// bad-logits code; HF_BLOCK + BLK_* = a snapshot of the device block {step, done, n_emitted, bad}, HF_LOOKUP + 0..3 = lk_state's {steps, drafted,
// accepted, n_emit[0]}
enum { HF_DONE = 0, HF_NEMIT = 1, HF_CB_LIVE = 3, HF_BAD = 4, HF_BLOCK = 8, HF_LOOKUP = 12, BLK_STEP = 0, BLK_DONE = 1, BLK_NEMIT = 2, BLK_BAD = 3 };
// a prefix-cache key / page digest: two 64-bit lanes (prefix_cache/prefix_cache.hip)
struct PcKey {
    uint64_t a, b;
    bool operator==(const PcKey& o) const { return a == o.a && b == o.b; }
};
struct PcKeyHash { size_t operator()(const PcKey& k) const { return (size_t)(k.a ^ (k.b * 0x9E3779B97F4A7C15ull)); } };
struct sv_engine {
    sv_config cfg;
    std::mutex mu;
    int T = 0, NP = 0, dh = 0, vdh = 0;
    int nkv = 1, QKV = 0, vit_F = 0;      // KV heads, width of the fused q|k|v projection, ViT MLP width
    bool v2 = false;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    size_t kv_head_stride = 0;
    int conv_K = 0;

    // weights
    Linear conv1;
    bf16_t *cls = nullptr, *pos = nullptr;
    LNp ln_pre, ln_vision;
    std::vector<VitLayer> vit;
    Linear ad_fc, ad_proj;
    bf16_t *ad_w = nullptr, *ad_b = nullptr, *ad_rm = nullptr, *ad_rv = nullptr;
    bf16_t *wte = nullptr, *wpe = nullptr;
    Linear lm_head;
    bool lm_head_explicit = false;
    LNp ln_f;
    std::vector<DecLayer> dec;
    std::unordered_map<std::string, Slot> slots;
    std::vector<void*> allocs;

    // vision workspaces (rows = max_batch * T)
    bf16_t *patches = nullptr, *patch_out = nullptr, *vx = nullptr, *vln = nullptr, *vqkv = nullptr,
           *vattn = nullptr, *vmlp = nullptr, *a1 = nullptr, *a2 = nullptr;
    // prefill workspaces (lazily grown)
    size_t pf_rows = 0;
    bf16_t *ph = nullptr, *pln = nullptr, *pqkv = nullptr, *pattn = nullptr, *pmlp = nullptr;
    // decode workspaces
    int MT = 0, ldws = 0, Vpad = 0;
    bf16_t *h_dec = nullptr, *hl = nullptr, *xp_a = nullptr, *xp_attn = nullptr, *xp_mlp = nullptr;
    bf16_t* h_xp = nullptr;         // residual stream of the decode step in fragment order (6-launch layer)
    // sv_config.exclusive_device == 2 ("optimistic"): the fused launches are on until one of them gives up (another tenant holds CUs); then they are off for the
    // rest of the engine's life and the failed sv_generate call is run again without them (engine_generate.hip)
    bool fused_off = false;
    int last_giveup = 0;            // code (3 / 4) of the give-up the last report_bad_logits saw, 0: none
    int stream_skip = 0;            // columns the failed attempt of an optimistic call already handed to the streaming callback
    bool fold6 = false;             // 6 launches per layer: slab-free attention output projection + ln_2 folded into c_fc
    bool fold_ready = false;
    bf16_t* xp_f = nullptr;         // ln_f output of the last row update (the lm_head's operand) when xp_a belongs to the fused row-update + c_attn launch
    long long* rc_dbg = nullptr;    //   [8] what the first GEMM wave to give up saw
    hipStream_t tenant_stream = nullptr;       // sv_debug_occupy_cus (safety tests): the stream the foreign tenant's kernel runs on
    int rc_delay = 390;             //   narrow rows: its GEMM blocks' first poll, 10-ns ticks after block start (3.9 us: measured optimum); wide rows: their
                                    //   hold-back in front of the weight requests (0); SV_RC_DELAY at sv_create
    int step_nodes = 0; bool step_rc = false, step_sel = false, step_mlp = false;      // sv_debug_step_plan: the last captured / launched decode step
    bool xpa_armed = false;         // xp_a carries the "not written yet" pattern, put there by a write-through fill of the lm_head launch in front (layer 0 of the next fused step polls it)
    bool rc_fused_ok = false;       // row update + c_attn as one launch (rowops.hip rowln_cattn_kernel) fits this engine: shapes + all blocks resident
    bool mlp_fused_ok = false;      // the MLP half as one launch (mlp_fused.hip mlp_fused_kernel) fits this engine: shapes + one block per CU
    long long* attn_trace = nullptr;// SV_ATTN_TRACE=1: wall-clock stamps of the decode attention of the middle layer, [rows * kv heads * splits][16]
    long long* mlp_trace = nullptr; // SV_MLP_TRACE=1: wall-clock stamps of the LAST fused MLP launch, [F / 32][8] (sv_debug_mlp_trace)
    bool only_skinny = false;       // profiling: enqueue only the weight-streaming GEMMs of a step
    bool skip_skinny = false;       // profiling: enqueue everything BUT the weight-streaming GEMMs
    int exp = 0;                    // A/B switches: a mask of sv_exp_bits (include/starvector_hip_debug.h), from SV_EXP at sv_create or sv_debug_set_exp
    float *ws = nullptr, *ws2 = nullptr, *logits = nullptr, *sample_scratch = nullptr, *attn_part = nullptr;
    unsigned* attn_cnt = nullptr;
    float* am_val = nullptr; int32_t* am_idx = nullptr;
    // the step's bookkeeping folded into the lm_head launch (SkinnyArgs::finish): set by sv_generate for the decode steps of a call whose selection is folded
    // (greedy_fused), read by decode_forward; fin_folded = the lm_head launch just issued took the bookkeeping (sample_and_finish launches no finish_step_kernel)
    FinishArgs fin_args; bool fin_fold = false, fin_folded = false; unsigned* fin_cnt = nullptr;
    float* tail_ws = nullptr; unsigned* tail_cnt = nullptr;      // SkinnyArgs::tail_ws / ::tail_cnt (gemm_skinny_tailsplit_kernel): partials + zeroed arrival tickets
    unsigned long long* amax = nullptr;   // greedy selection folded into the lm_head launch: one 64-bit key per row, [64 * SV_AMAX_STRIDE]
    bool greedy_fused = false;            //   on for the decode steps of the current sv_generate call (set and cleared by it)
    uint32_t* seen = nullptr; int seen_words = 0;      // repetition-penalty bitmap [rows][Vpad/32]
    int32_t *cur_tok = nullptr, *next_tok = nullptr, *unfinished = nullptr, *positions = nullptr,
            *out_tok = nullptr, *d_step = nullptr, *d_done = nullptr, *d_nemit = nullptr, *d_stop = nullptr, *d_bad = nullptr;
    int out_ld = 0;
    int32_t* h_flags = nullptr;   // pinned, indexed by HF_* (above)
    int32_t* h_table = nullptr;   // pinned host image of block_table (assign_pages); table_ev = its last upload
    hipEvent_t table_ev = nullptr;
    bool table_pending = false;
    // packed prompt passes (PackedPlan below): the lists of the call's plan, concatenated into a pinned host image and uploaded without a stream
    // synchronise like the block table (engine_forward.hip::rag_upload_plan); grown on demand
    int32_t *h_rag = nullptr, *d_rag = nullptr;
    size_t rag_cap = 0;                           // int32 elements either holds
    hipEvent_t rag_ev = nullptr;
    bool rag_pending = false;
    int32_t* rag_row_pos = nullptr; size_t rag_pos_rows = 0;      // [packed rows] position of a row inside its sequence
    bf16_t* rag_rsave = nullptr;                  // [3 * max_batch][hidden] residual rows of a GEMM's remainder launch (launch_gemm_ragged)
    long long prompt_passes = 0;                  // prompt passes run so far, rectangular and packed (sv_debug_prompt_passes)
    // KV pool
    char* kv_pool = nullptr;
    size_t layer_stride = 0;
    int pages_per_seq = 0, num_pages = 0, page_bytes = 0;
    int kv_dtype = 0;               // SV_KV_BF16 / SV_KV_FP8_E4M3 (sv_create_kv): the format of kv_pool's pages, page_bytes follows from it
    int32_t* block_table = nullptr;
    std::vector<int> free_pages;
    // shared prompt pass (sv_generate_shared / sv_cb_admit_shared): pinned image of the prompt-pass table + the fork launch's descriptors, their
    // device copy ([6 * max_batch]: prompts | other rows | logits source rows), both allocated on first use; holders of every SHARED page of a
    // continuous batch (0: the page is private to one slot, or free)
    int32_t* h_fork = nullptr;
    int32_t* fork_desc = nullptr;
    std::vector<int> page_refs;
    // beam search (num_beams > 1): device scorer
    BeamScorer beam;
    bf16_t* score_ws = nullptr;      // scoring forward: kept hidden rows, their ln_f, bf16 logits [rows][Vpad]
    size_t score_elems = 0;
    // sv_forward_logprobs: the lm_head runs over the kept rows in chunks of score_chunk_rows rows into this workspace ([chunk][Vpad] bf16 + the kernel's
    // int32[2] flag behind it), logprob_rows reads the chunk back; allocated on first use, a function of the chunk size alone -- never of B x n_keep
    bf16_t* score_chunk_ws = nullptr;
    int score_chunk_alloc = 0;       // rows the workspace holds
    int score_chunk_rows = 0;        // sv_debug_set_score_chunk_rows; 0 = SV_SCORE_CHUNK_ROWS
    float* score_lse_ws = nullptr;   // sv_forward_topk without a caller's logsumexp: [score_lse_alloc] fp32, the chunk's lse between the two kernels
    int score_lse_alloc = 0;
    int cached_B = 0;
    // extension passes (sv_prefill_open / sv_prefill_extend, chunked prefill; extend/extend.hip).  ctx_known: ctx_len[b] / ctx_cap[b] are the tokens
    // cached for row b and the tokens its pages hold -- set by sv_prefill, sv_prefill_ragged, sv_debug_kv_load and the two calls, +1 per
    // sv_decode_step, void after anything else that assigns pages or runs a prompt pass.  prefill_chunk: the row budget of sv_set_prefill_chunk (0: off).
    // gkv: the K | V rows of the sequences with a context, [gkv_rows][2 * n_kv * head_dim]; logit_stash: [max_batch][Vpad] last-row logits of the
    // sequences a chunked call finished in an earlier pass
    bool ctx_known = false;
    std::vector<int> ctx_len, ctx_cap;
    int prefill_chunk = 0;
    bf16_t* gkv = nullptr; size_t gkv_rows = 0;
    float* logit_stash = nullptr;
    int dbg_pos_hi = 0;            // sv_debug_kv_load / sv_debug_attn_decode: upper bound of positions[] (host side), kept below max_seq_len
    int num_cus = 256;
    double timing[3] = {0, 0, 0};
    double timing_graph = 0;
    // generation runs on an engine-owned non-blocking stream (the caller's stream may be the legacy
    // null stream, which cannot be captured into a hipGraph); ordered after the caller's stream by an event
    hipStream_t gen_stream = nullptr;
    hipEvent_t gen_event = nullptr;
    // continuous batching: one request per row ("slot")
    bool cb_active = false;
    std::vector<char> cb_used;                    // slot in use (admitted, not yet released)
    std::vector<std::vector<int>> cb_pages;       // pages held by each slot
    CbSlot* cb_slots = nullptr;                   // device [max_batch]
    CbBias* cb_bias = nullptr;                    // device [max_batch]: logit bias of vLLM-mode slots
    uint16_t* cb_counts = nullptr;                // device [max_batch][Vpad]: output-token counts of vLLM-mode slots
    int32_t *cb_map = nullptr, *cb_nlive = nullptr, *cb_events = nullptr, *cb_table_pf = nullptr;
    // sv_cb_admit_logprobs: the per-slot record descriptors (device [max_batch]) and their host image (enable = 0 for every slot that is free or
    // did not ask), over four engine-owned buffers of max_batch x max_seq_len columns (log-prob, rank: 4 B each; ids, log-probs: SV_TOPK_MAX x 4 B
    // each).  All of it is allocated by the first admit that asks: cb_lp == nullptr on an engine that never did.
    CbLogprobs* cb_lp = nullptr;
    std::vector<CbLogprobs> cb_lp_host;
    // sv_cb_set_lookup: cb_K > 0 = the batch drafts, a slot owns cb_K + 1 decode rows (kernels.h CbLookupArgs).  cb_lk_state (device, allocated
    // by the first such setting): n_draft [max_batch] | counts [max_batch][3] | totals [3].  cb_lk_forced (sv_debug_cb_set_lookup_drafts):
    // [cb_lk_forced_n][cb_lk_forced_ld] on the device (allocated once, [max_batch][max_seq_len]); n = 0: the lookup
    int cb_K = 0, cb_max_ngram = 3, cb_min_ngram = 1;
    int32_t* cb_lk_state = nullptr;
    int32_t* cb_lk_forced = nullptr;
    int cb_lk_forced_n = 0, cb_lk_forced_ld = 0;
    int trash_page = 0;                       // what the block-table rows of free slots point at
    // sv_cb_set_prefix_cache (prefix_cache/prefix_cache.hip; the table: engine_cb.hip).  pc_on stays across sv_cb_reset; everything else lives from
    // cb_begin to sv_cb_reset.  pc_table: chained key -> page.  A registered page's page_refs entry is its exact holder count; one without a holder
    // sits in pc_lru (front = least recently released) instead of the free list.  pc_dig [max_batch][pages_per_seq] digests and pc_desc
    // [2 * max_batch] descriptors are device memory of the engine (allocated by the first enable), pc_ws the compacted own rows of an admit with hits
    bool pc_on = false;
    std::unordered_map<PcKey, int, PcKeyHash> pc_table;
    std::vector<PcKey> pc_key_of;                 // [num_pages + 1] the key a registered page stands under
    std::vector<char> pc_reg;                     // [num_pages + 1] page is in pc_table
    std::list<int> pc_lru;
    std::vector<std::list<int>::iterator> pc_lru_it;
    std::vector<char> pc_in_lru;
    long long pc_lookups = 0, pc_reused = 0, pc_evictions = 0;
    uint64_t* pc_dig = nullptr;
    int32_t* pc_desc = nullptr;
    bf16_t* pc_ws = nullptr; size_t pc_ws_rows = 0;
    std::unordered_map<int, GraphSlot> cb_graphs;      // one captured step per row bucket (cleared by cb_drop_graphs alone)
    // sv_generate: the captured decode step is kept while the next call has the same shape and sampling parameters
    GraphSlot gen_step;
    // the same step SV_GRAPH_STEPS times in ONE graph (engine_generate.hip: a hipGraphLaunch-to-hipGraphLaunch boundary costs 8.6 us of idle GPU per step,
    // a kernel-to-kernel boundary inside a graph nothing measurable -- profiles/step_gaps_r06.log); built for calls long enough to pay for its instantiation
    GraphSlot gen_multi;             // key = the step count
    // sv_generate_ex outputs: the device descriptor of the caller's slabs (rewritten for every call, never baked into a graph), its host image,
    // per-row warper thresholds of the sampling capture; cap_on = the current call captures (set and cleared by sv_generate_ex)
    CaptureDesc* cap_desc = nullptr;
    CaptureDesc cap_host = {};
    float* cap_warp = nullptr;
    bool cap_on = false;
    // sv_generate_stats: the device descriptor of the caller's three [rows][ld] buffers (rewritten for every call, like cap_desc), its host image, the
    // raw row's {max, log-sum, entropy} per row; ts_on = the current call asks for statistics (set and cleared by it)
    TokenStatsDesc* ts_desc = nullptr;
    TokenStatsDesc ts_host = {};
    float* ts_raw = nullptr;
    bool ts_on = false;
    // sv_generate_topk: the device descriptor of the caller's top-k buffers (rewritten for every call), its host image, and the request the step is
    // keyed on; tk_on = the current call asks for the lists (set and cleared by it)
    TokenTopkDesc* tk_desc = nullptr;
    TokenTopkDesc tk_host = {};
    int tk_k = 0, tk_source = 0;
    bool tk_rank = false, tk_on = false;
    // sv_generate_processed: the HF logits processors of the current call (set and cleared by it).  A ban (no_repeat_ngram_size, bad words) adds
    // one launch between the lm_head and the selection (processors.hip); min_p rides in the sampler's arguments.  The bad-word table is device
    // memory of the engine, uploaded once per call (ban_host = its host image, kept alive for the upload)
    int ban_ngram = 0, ban_nwords = 0;
    float minp_log = -INFINITY;
    BanWord* ban_words = nullptr;
    std::vector<BanWord> ban_host;
    // sv_generate_lookup (engine_generate.hip): lookup_on = decode_forward runs the K/V pre-write in front of every attention launch (set and
    // cleared by the call).  lk_state (device, allocated by the first such call): counts[3] | n_emit | fin | base | n_draft [max_batch each] |
    // limit | ticket.  The captured verification step has a cache slot of its own: a plain call after a lookup call replays the graph it kept.
    // lk_forced (sv_debug_set_lookup_drafts): [lk_forced_B][lk_forced_ld] forced drafts on the device (allocated once, [max_batch][max_seq_len]);
    // lk_forced_B = 0: the lookup.
    bool lookup_on = false;
    int32_t* lk_state = nullptr;
    int32_t* lk_forced = nullptr;
    int lk_forced_B = 0, lk_forced_ld = 0;
    // sv_generate_lookup_sampled with a repetition penalty (lookup_seen_kernel): one bitmap of generated ids per SEQUENCE [64][seen_words] and
    // the columns it covers [64]; e->seen then holds one bitmap per ROW of the step in flight (allocated by the first such call)
    uint32_t* lk_seen = nullptr;
    int32_t* lk_seen_cols = nullptr;
    GraphSlot lk_step;
    // optional per-kernel HIP-event profiling of the decode step (bench.py roofline leg)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_kind;
    size_t prof_used = 0;
};

enum { PK_SKINNY = 0, PK_ATTN = 1, PK_ROWLN = 2, PK_SAMPLE = 3, PK_COUNT = 4,
       // stages of the time to first token (sv_profile_ttft): never marked by decode_forward
       PK_VIT_GEMM = 4, PK_VIT_ATTN, PK_VIT_ROWS, PK_AD_GEMM, PK_AD_NORM, PK_PF_GEMM, PK_GEMM_TAIL, PK_PF_ATTN, PK_PF_ROWS, PK_PF_LMHEAD,
       PK_FIRST_SAMPLE, PK_END, PK_TTFT_FIRST = PK_VIT_GEMM, PK_TTFT_COUNT = PK_END - PK_VIT_GEMM };

namespace sveng {
// engine_core.hip: small utility kernels behind host wrappers, allocation, decode planning
void fill_i32(int32_t* p, int32_t v, int n, hipStream_t st);
void gen_state_init(int32_t* positions, int32_t pos0, int32_t* unfinished, int B, int32_t* state3, unsigned long long* amax, int n_amax, hipStream_t st);
void add_i32(int32_t* p, int32_t v, int n, hipStream_t st);
void suppress_token(float* logits, int ld, int token, const int32_t* step, int min_new, int B, hipStream_t st);
void tokens_to_i64(const int32_t* src, int ld, int64_t* dst, int B, int ncols, int dst_ld, hipStream_t st);
void fill_random_bf16(bf16_t* p, size_t n, unsigned seed, int blocks, hipStream_t st);
void pack_rows(const bf16_t* x, int ldx, bf16_t* xp, int M, int K, hipStream_t st);
void unpack_rows(const bf16_t* xp, bf16_t* x, int ldx, int M, int K, hipStream_t st);
void reduce_partials(const float* ws, int splitk, int rows_ws, int ldws, const bf16_t* bias, float* y, int M, int N, hipStream_t st);
int dev_alloc(sv_engine* e, void** p, size_t bytes, bool zero = true);
template <typename T>
inline int dalloc(sv_engine* e, T** p, size_t count, bool zero = true) {
    return dev_alloc(e, reinterpret_cast<void**>(p), count * sizeof(T), zero);
}
void pick_decode_plan(const Linear& l, int MT, int num_cus, int wfmt, bool whole_k, int* splitk, int* col_tiles);
int check_exp_mask(int mask, const char* who);      // SV_EINVAL (naming the bits) unless mask is a subset of SV_EXP_KNOWN
// hipGraph capture of decode steps, shared by sv_generate (greedy, lookup and beam) and sv_cb_step through GraphSlot::use.  capture_steps: relaxed capture of `copies` calls of
// one_step on `st` -> *g, instantiated -> *ge.  On failure the sticky HIP error is cleared, both handles are destroyed and nulled, and the
// result is SV_EHIP if `required` and SV_REQUIRE_GRAPH is set, else 0 with *ge == nullptr: the caller runs plain launches of the same kernels.
bool graph_enabled();       // SV_NO_GRAPH unset (read per call: the tests switch it inside one process)
int graph_steps_cap();      // SV_GRAPH_STEPS (read once per process), 32 by default: most steps in one graph
int capture_steps(hipStream_t st, int copies, const std::function<void()>& one_step, hipGraph_t* g, hipGraphExec_t* ge, bool required = true);
// engine_forward.hip: the op graphs
void prof_mark(sv_engine* e, int kind, hipStream_t st);
int attn_max_splits_of(int max_batch, int nkv, int num_cus);
int attn_groups_per_block_of(int max_batch, int nkv, int num_cus);
void reset_free_pages(sv_engine* e);      // every page of the pool is free again, lowest page handed out first
int assign_pages(sv_engine* e, int B, int total_len, hipStream_t st);      // assign_pages_ragged without lengths: total_len tokens per sequence
// rows per lm_head chunk of sv_forward_logprobs: a multiple of 256 (the big-M tile height: a chunk boundary never cuts a tile); 4096 rows x Vpad ~ 49.2 k
// bf16 = 403 MB at StarVector's vocabulary -- the fastest of 512 / 1024 / 2048 / 4096 measured (profiles/score_logprobs.md; DESIGN.md "Scoring without logits")
#define SV_SCORE_CHUNK_ROWS 4096
// what sv_forward_logprobs asks of the scoring pass instead of the logits: [B][n_keep] each, any output may be nullptr
// (sv_forward_topk: k > 0 adds [B][n_keep][k] ids and log-probs and the [B][n_keep] rank of the target, rank may be nullptr)
struct ScoreLogprobs { const int32_t* targets; float inv_t; float* logprob; float* lse; float* entropy; int32_t* argmax;
                       int k = 0; int32_t* topk_ids = nullptr; float* topk_logprobs = nullptr; int32_t* rank = nullptr; };
int prefill_forward(sv_engine* e, const bf16_t* embeds, int B, int S0, hipStream_t st, int n_keep = 0,
                    bf16_t* dev_scores = nullptr, const int32_t* table = nullptr, const ScoreLogprobs* lp = nullptr);
void decode_forward(sv_engine* e, int B, hipStream_t st);
void attn_decode_args(sv_engine* e, int layer, int B, const float* ws, int splitk, const bf16_t* bias, bf16_t* out_xp, AttnDecodeArgs& ad);
LookupKvArgs lookup_kv_args(const AttnDecodeArgs& ad);      // the pre-write of a verification step in front of the attention launch `ad`
int check_ready(sv_engine* e);
// continuous batching (engine_cb.hip): validation of one request (SV_EINVAL + message) and its device state -- the slot, its
// logit bias, its repetition bitmap row (seen_words words: the prompt ids in vLLM mode, cleared otherwise)
int cb_check_request(const sv_cb_request& r, int V, int i, const char* who);
void cb_fill_slot(const sv_cb_request& r, CbSlot& h, CbBias& bias, std::vector<uint32_t>& seen_row, int seen_words);
// the log-prob requests of n requests (lps may be nullptr: nobody asks): SV_EINVAL + message for an entry with enable != 0 and k outside
// 0..SV_TOPK_MAX, a source outside {0, 1}, or source 0 on a vLLM-semantics request -- host arithmetic, no device
int cb_check_logprobs(const sv_cb_request* reqs, const sv_cb_logprobs* lps, int n, const char* who);
// group admit (sv_cb_admit_shared): validation of (lens, group) and the page plan -- host arithmetic, stated by sv_debug_shared_plan for the CPU tests
int shared_check_group(const char* who, const int32_t* lens, int n_prompts, const int32_t* group, int n);
long long shared_page_plan(const int32_t* lens, int n_prompts, const int32_t* group, const int32_t* budgets, int n, int32_t* shared, int32_t* private_);
int cb_guard(sv_engine* e, const char* who);
// sv_cb_set_lookup's range checks and defaults (host arithmetic): lk <- the values in force
int cb_check_lookup(const char* who, const sv_lookup* lookup, sv_lookup& lk);
void cb_drop_graphs(sv_engine* e);          // the kept step graphs name the drafting setting and the forced-draft buffer: gone when either changes
int prefill_locked(sv_engine* e, const void* dev_embeds, int B, int S0, int total_len, hipStream_t st, bool set_positions = true);
// The packed prompt passes (engine_forward.hip::prefill_forward_packed): sequences of different lengths, embeddings packed back to back, no padding row.
// Two forms share the one layer loop and differ only in the data of a PackedPlan:
//   ragged    B sequences of lengths lens[0..B) (sv_prefill_ragged, sv_generate_ragged, the CB admit paths, sv_forward_logprobs_ragged)
//   prefixed  P prefixes and the own rows of B sequences in ONE packed buffer, prefixes first; sequence b stands for the solo sequence
//             concat(prefix[prefix_of[b]], own rows of b) of T_b = Pl + len_b rows (sv_forward_logprobs_prefixed; why the bits hold: prefix/prefix.hip)
// Everything a plan decides is host arithmetic: ragged_plan and prefix_plan need no engine (sv_debug_ragged_plan / sv_debug_prefix_plan state them for
// the CPU tests).  The lists of a plan, in the order they lie in the plan image (sv_engine::h_rag / d_rag):
enum {
    PL_DESC,            // ragged: descriptors {first packed row, length} x B | prefixed: segments {first packed row, length, position of its first row} x (P + B)
    PL_SEQ0, PL_BLOCKS0,   // first attention launch: its sequences (EMPTY: the ragged descriptors) | {sequence, query tile}, every tile
    PL_SEQ1, PL_BLOCKS1,   // second attention launch (prefixed form): {first own packed row, T, first prefix packed row, Pl} | tiles whose last row >= Pl
    PL_LAST_TILES,      // {sequence, its last query tile}: the pruned last layer (ragged generation)
    PL_KV_BLOCKS,       // {sequence, 32-row tile} of the KV write; EMPTY: no page is written (prefixed)
    PL_ROWS,            // + 2 i: the packed rows projection i sends through the split-K remainder kernel -- the last seq_peel_rows(T) rows of every
                        //   solo sequence of T rows with gemm_seq_form(T, N, K, act); + 2 i + 1: the sequences whose LAST row is one of them (the pruned
                        //   last layer's compact rows; ragged only)
    PL_KEPT = PL_ROWS + 8,   // scoring: ragged {first packed row, length, keep, first output row} x B | prefixed: the kept packed rows, in output order
    PL_COUNT
};
constexpr int pl_rows(int i) { return PL_ROWS + 2 * i; }
constexpr int pl_last(int i) { return PL_ROWS + 2 * i + 1; }
// The ragged form's descriptors are the FIRST list: they lie at offset 0 of d_rag and stay valid until the next packed pass -- ragged_positions,
// the generate drivers (kv.rag_seq = e->d_rag) and the CB admit paths read them there after the pass has returned.
struct PackedPlan {
    enum Tail { GENERATE,             // last layer pruned to every sequence's last row, then last-row logits
                SCORE_TAIL_ROWS,      // gather_tail_rows over PL_KEPT -> ln_f -> chunked lm_head + logprob_rows, then last-row logits
                SCORE_LISTED_ROWS };  // gather_listed_rows over PL_KEPT -> the same; no last-row logits
    int M = 0, B = 0;                      // packed rows | sequences
    const bf16_t* src[2] = {nullptr, nullptr};   // embedding sources, laid back to back in the pass's hidden buffer (set by the caller of the builder)
    int src_rows[2] = {0, 0};              //   and their rows (ragged: M, 0 | prefixed: prefix rows, own rows)
    int n_seg = 0;                         // 0: row positions from the ragged descriptors | P + B segments of the prefixed form
    int n_attn = 1;                        // attention launches per layer; the second one is the prefixed form
    Tail tail = GENERATE;
    int kept = 0;                          // kept rows of a scoring tail
    int refused = -1, refused_proj = -1;   // prefixed: first sequence whose remainder rows would reach into its prefix (and the projection that says so)
    std::vector<int32_t> list[PL_COUNT];
    std::vector<int32_t>& rows(int i) { return list[pl_rows(i)]; }
    std::vector<int32_t>& last(int i) { return list[pl_last(i)]; }
};
struct PlanProj { int N, K, act; };        // a projection as the remainder-row rule sees it
// {sequence, tile} pairs of `tile` rows counted from each sequence's first row (last_only: each sequence's last tile alone)
void ragged_blocks(const int32_t* lens, int B, int tile, bool last_only, std::vector<int32_t>& out);
// the ragged form's plan.  keep == nullptr: generation; otherwise scoring -- the last keep[b] (1..lens[b]) rows of every sequence, outputs packed
// [sum(keep)] in sequence order, no layer pruned.  n_proj = 0: no per-sequence remainder anywhere (SV_EXP_BATCH_REMAINDER)
void ragged_plan(const int32_t* lens, int B, int q_tile, const PlanProj* proj, int n_proj, const int32_t* keep, PackedPlan& out);
int ragged_check_lens(const sv_engine* e, const int32_t* lens, int B, const char* who, int* max_len, long long* total);
int assign_pages_ragged(sv_engine* e, int B, const int32_t* lens, int extra, hipStream_t st);
int prefill_forward_packed(sv_engine* e, const PackedPlan& p, const int32_t* table, const ScoreLogprobs* lp, hipStream_t st);
// ragged_plan over (lens, keep) for this engine, then the pass; keep + lp: both (scoring) or neither (generation)
int prefill_forward_ragged(sv_engine* e, const bf16_t* embeds, int B, const int32_t* lens, hipStream_t st, const int32_t* table = nullptr,
                           const int32_t* keep = nullptr, const ScoreLogprobs* lp = nullptr);
// positions[i] = lens[i / rep] + delta for i < B * rep, from the descriptors the last ragged pass uploaded
void ragged_positions(sv_engine* e, int B, int rep, int delta, hipStream_t st);
// the launch behind it: positions[i] = rag_seq[2 * (i / rep) + 1] + delta for i < n, descriptors {first packed row, length}
void launch_ragged_positions(int32_t* positions, const int32_t* rag_seq, int n, int rep, int delta, hipStream_t st);
// SV_EINVAL + message (who: ...) for P / B out of order (1 <= P <= B), a length < 1, a prefix_of outside 0..P-1, a prefix no sequence uses, and
// -- keep != nullptr -- a keep outside 1..len + 1
int prefix_check(const char* who, const int32_t* prefix_lens, int P, const int32_t* lens, const int32_t* prefix_of, int B, const int32_t* keep);
// the prefixed form's plan (prefix/prefix.hip).  keep != nullptr: PL_KEPT = the last keep[b] solo rows of every sequence (keep = len + 1 starts at its
// prefix's last row)
void prefix_plan(const int32_t* prefix_lens, int P, const int32_t* lens, const int32_t* prefix_of, int B, int q_tile, const PlanProj* proj, int n_proj,
                 const int32_t* keep, PackedPlan& out);
// The extension pass (extend/extend.hip; the layer loop is engine_forward.hip::extend_forward): sequence b has ctx tokens in its pages, gets len own
// rows in this pass and is routed as a sequence of total >= ctx + len rows; len == 0: the sequence takes no part in the pass.
struct ExtendSeq { int ctx, len, total; };
enum {
    XL_DESC,            // what the CALLER wants at offset 0 of d_rag behind the pass (a chunked ragged pass: {first packed row, length} x B of the whole call)
    XL_XSEQ,            // {block-table row, first packed own row, ctx, len, first row of its K | V region or -1, 0} per sequence of the pass (kernels.h ExtKvArgs)
    XL_SEG,             // {first packed row, len, ctx}: the row positions (launch_prefix_row_pos)
    XL_WRITE, XL_GATHER,   // {sequence of the pass, 32-token group}: the page writer's groups | the gather's
    XL_PLAIN_SEQ, XL_PLAIN_BLOCKS, XL_PLAIN_LAST,   // sequences without a context: ragged descriptors {first packed row, len} | their tiles | the last tile of those that finish
    XL_CTX_SEQ, XL_CTX_BLOCKS,   // sequences with one: {first own packed row, T, R - ctx, ctx} | {0, tile} from the straddling tile on -- one launch each (ExtendPass::CtxSeq)
    XL_FIN,             // {first packed row, len} of the sequences that reach their total in this pass: the pruned last layer's compact rows
    XL_POS,             // caller: positions[] behind the pass (sv_prefill_extend)
    XL_ROWS,            // + 2 i: remainder rows of projection i | + 2 i + 1: the compact rows (indices into XL_FIN) whose last row is one
    XL_COUNT = XL_ROWS + 8
};
struct ExtendPass {
    struct CtxSeq { int b; long long region; int index_row0; bool fin; int seq_off, blocks_off, n_blocks; };
    int M = 0, B = 0;
    long long gkv_rows = 0;
    std::vector<int32_t> list[XL_COUNT];
    std::vector<CtxSeq> ctx_seqs;
    std::vector<int32_t> fin;              // the call's sequence behind every compact row
    std::vector<int32_t>& rows(int i) { return list[XL_ROWS + 2 * i]; }
    std::vector<int32_t>& last(int i) { return list[XL_ROWS + 2 * i + 1]; }
    const std::vector<int32_t>& rows(int i) const { return list[XL_ROWS + 2 * i]; }
    const std::vector<int32_t>& last(int i) const { return list[XL_ROWS + 2 * i + 1]; }
};
void extend_schedule(const int32_t* lens, int B, int budget, std::vector<std::vector<int32_t>>& take);
void extend_plan(const ExtendSeq* seqs, int B, int q_tile, const PlanProj* proj, int n_proj, ExtendPass& out);
ExtKvArgs extend_kv_args(sv_engine* e, int layer, const int32_t* table, const int32_t* xseq, const int32_t* blocks, int n_blocks, bf16_t* gkv);
// one pass over p.M packed own rows `embeds`; p.list[XL_DESC] / [XL_POS] are the caller's.  Last-row logits of compact row i (sequence p.fin[i]) -> row i of e->logits
int extend_forward(sv_engine* e, ExtendPass& p, const bf16_t* embeds, const int32_t* table, hipStream_t st);
// a generate-tail prompt pass over B sequences of lens[] rows as passes of at most e->prefill_chunk own rows (one pass when the budget does not
// apply); leaves e->logits and d_rag as the one-shot pass does.  ctx0 != nullptr: sequence b already has ctx0[b] < lens[b] tokens in its pages (the
// prefix cache's reused pages) and `embeds` packs only the lens[b] - ctx0[b] own rows of every sequence; the budget counts own rows
int prefill_chunked(sv_engine* e, const bf16_t* embeds, int B, const int32_t* lens, const int32_t* table, hipStream_t st, const int32_t* ctx0 = nullptr);
// prefix_cache/prefix_cache.hip: the page digests of an admit and the host arithmetic of the keys
//   digests: one launch over n packed prompts (lens == nullptr: n x S0 rows) -> dev_out [n][max_pages] digests, entry (u, k) written for k < len_u / 64;
//            dev_desc: room for 2 * n int32 (the {first packed row, len} descriptors, uploaded from host_desc -- which must outlive the copy)
int pc_launch_digests(const bf16_t* embeds, int n, const int32_t* dev_desc, int S0, int hidden, int max_pages, uint64_t* dev_out, hipStream_t st);
PcKey pc_chain(const PcKey& prev, const PcKey& digest);      // key_k = mix(key_{k-1}, digest_k)
PcKey pc_key0();                                             // key_{-1}
inline int pc_hit_pages(int matched, int L) { return std::min(matched, (L - 1) / SV_PAGE_TOKENS); }      // at least one own row is always computed
void pc_drop(sv_engine* e);      // engine_cb.hip: the table is empty again; cached pages nobody holds go back to the free list
// engine_generate.hip
void fork_args(sv_engine* e, int n_prompts, int n_rows, ForkArgs& f);      // the fork launch over e->fork_desc, the engine's block table, pool and logits
// validation of a processor set against a vocabulary of V ids (V <= 0: the ids are only checked for >= 0) -- host arithmetic, no device -- and
// the bad-word table it describes
int check_logits_processors(const sv_logits_processors* lp, int V, const char* who);
void ban_word_table(const sv_logits_processors& lp, std::vector<BanWord>& out);
int check_finite_logits(sv_engine* e, hipStream_t st, const char* who);
int report_bad_logits(sv_engine* e, hipStream_t st, const char* who, int what);      // what = the d_bad code already read (0: fine)
}  // namespace sveng
using namespace sveng;
