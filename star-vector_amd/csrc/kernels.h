// Internal host-side launchers for the gfx950 kernels (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include "common.h"

namespace sv {

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
// An A/B switch of the environment, read per call (A/B inside one process; a captured graph keeps its choice): unset = dflt
inline int env_switch(const char* name, int dflt) {
    const char* ev = getenv(name);
    return ev ? atoi(ev) : dflt;
}

// ---- weights -----------------------------------------------------------------------------------
// src: [N][K] row-major (bf16 if src_is_f32==0 else float).  dst: packed [Npad/32][Kpad/16][64][8].
void launch_pack_weight(const void* src, int src_is_f32, bf16_t* dst, int N, int K, int Npad, int Kpad,
                        hipStream_t st);
void launch_convert_to_bf16(const void* src, int src_is_f32, bf16_t* dst, size_t n, hipStream_t st);
// fp8 (OCP e4m3) weight-only quantisation, one scale per output row: scale[n] = max_k |W[n][k]| / 448,
// q = fp8_rne(W / scale).  Writes the decode image Wq [Npad/32][Kpad/32][64 lanes][16 B] (a lane's two consecutive
// k-steps of 8 fp8 each), the bf16 image of the SAME q values in the usual packed layout (prefill / big-M kernels, which
// apply the scale in their epilogue like the decode kernel does), and scale[Npad] (1 for padding rows).
void launch_pack_weight_fp8(const void* src, int src_is_f32, bf16_t* dst_bf16, uint8_t* dst_q, float* scale, int N, int K,
                            int Npad, int Kpad, hipStream_t st);
// weight formats of a Linear (sv_config.weight_dtype; skinny_plan / pick_decode_plan take them where they took `fp8`)
enum { SV_WFMT_BF16 = 0, SV_WFMT_FP8 = 1, SV_WFMT_MXFP4 = 2 };
// MXFP4 (OCP MX: e2m1 codes, one e8m0 scale byte per 32 consecutive k of an output row) weight-only quantisation (mxfp4/mxfp4.hip).
// Per block: amax = max |W|; amax == 0: E = 0, codes 0; else E = floor(log2(amax)) - 2 clamped to [-125, 125], scale byte = E + 127;
// code = W / 2^E rounded to {0, .5, 1, 1.5, 2, 3, 4, 6} with its sign, ties to the even mantissa bit, magnitudes above 6 saturate.
// Writes
//  * the decode image W4: groups [Npad/32][Kpad/64] of SV_MXFP4_GROUP = 1088 bytes, a group = one column tile's 64 consecutive k:
//      bytes [0, 1024)    [64 lanes][16 B], lane = 32 * ((k / 8) & 1) + n % 32 (the bf16 image's lane), a lane's 16 bytes = four k-steps
//                         (word (k / 16) & 3) of 8 codes each: code k % 8 is nibble k % 8 of the word (byte (k % 8) / 2, low nibble = even k);
//      bytes [1024, 1088) [32 rows][2] scale bytes: row n % 32, byte (k / 32) & 1 (the two MX blocks of the group);
//    4.25 bits per weight, scales included;
//  * the bf16 image of the dequantised values q * 2^E (each exactly a bf16 number) in the usual packed layout, for the big-M kernels
//    with no column scale;
//  * scale_plain (optional, test surface): the scale bytes as [Npad][Kpad/32].
// Kpad % 64 == 0.  Padding rows / columns quantise as zeros (scale byte 127).
#define SV_MXFP4_GROUP 1088
inline size_t mxfp4_image_bytes(int Npad, int Kpad) { return (size_t)(Npad / 32) * (Kpad / 64) * SV_MXFP4_GROUP; }
void launch_pack_weight_mxfp4(const void* src, int src_is_f32, bf16_t* dst_bf16, uint8_t* dst_w4, uint8_t* scale_plain, int N, int K,
                              int Npad, int Kpad, hipStream_t st);

// ---- big-M MFMA GEMM:  C[M][N] = epi( A[M][K] . W^T + bias ) (+ residual) ----------------------
struct GemmArgs {
    const bf16_t* A; int lda;        // activations, row-major bf16, K-contiguous
    const bf16_t* Wp;                // packed weight
    const bf16_t* bias;              // [N] or nullptr
    const bf16_t* R; int ldr;        // residual [M][N] or nullptr (added after the activation)
    void* C; int ldc;                // bf16 (out_f32==0) or float
    int M, N, K;                     // K = padded K (multiple of 64) shared by A and Wp
    int act; int out_f32;
    const float* cscale = nullptr;   // fp8 weights: per-output-column scale applied to the accumulator (or nullptr)
    long long* trace = nullptr;      // optional [blocks][8] wall-clock stamps of the 256^2 kernel (tools/gemm_trace.py); nullptr in production
    void (*tail_mark)(void* ctx, hipStream_t st) = nullptr;   // profiling hook: called right before the remainder-row launch of a peeled GEMM
    void* tail_ctx = nullptr;        //   (sv_profile_ttft prices the tails apart from the tile launches); nullptr in production
    // Sequence structure of the rows (round 6, gemm.hip "rows a sequence leaves over"): the M rows are M / seq_rows sequences of seq_rows
    // rows each.  Where gemm_seq_form(seq_rows, N, K, act) holds, the first seq_rows - r rows of EVERY sequence go through the tile
    // kernels (a tile never straddles two sequences) and the last r = seq_rows % 256 rows of every sequence through the split-K
    // remainder kernel -- which kernel computes a row depends on the row's position in its sequence and on the projection, never on
    // the batch around it.  0 = plain row-major problem.
    int seq_rows = 0;
    int seq_tail = 0;                // set by the launcher for the remainder launch: row i -> (i / seq_tail) * seq_rows + seq_rows - seq_tail + i % seq_tail
    int splitk_rows = 0;             // 1: the M rows (compact, contiguous) are LAST rows of sequences of seq_rows rows (the pruned last prompt layer): they take
                                     //    the kernel the same rows take inside the full problem (split-K remainder kernel where gemm_seq_form holds)
    // Ragged prompt pass (launch_gemm_ragged): the remainder launch takes an EXPLICIT row list instead of the arithmetic map -- element i of the launch
    // reads row row_list[i] of A and writes row row_list[i] of C; r_compact = 1: its residual row is row i of R (saved aside before the first pass
    // added the residual in place)
    const int32_t* row_list = nullptr;
    int r_compact = 0;
    int tune_in_place = 0;           // 1 (and no residual operand): the tuner's timing runs write C itself instead of a scratch output of M x ldc elements
                                     //    (the chunked lm_head of the scoring forward: its footprint must not grow with rows x vocab; C is overwritten anyway)
};
// r = rows a sequence of S rows leaves over its 256-row tiles when that is a handful (32 sequences leave at most 96 rows) and a full tile exists; else 0
inline int seq_peel_rows(int S) { const int r = S % 256; return (S > 256 && r >= 1 && r <= 3) ? r : 0; }
// Does the projection (N, K, act) take the per-sequence form for sequences of S rows?  A function of the sequence length and the projection ONLY
// (never of the batch): where the dispatch's cost model peels the row remainder of a 32-sequence batch (gemm.hip gemm_plan).
bool gemm_seq_form(int S, int N, int K, int act);
void launch_gemm(const GemmArgs& a, hipStream_t st);
// Rows of sequences of DIFFERENT lengths, packed back to back (the ragged prompt pass).  Which kernel computes a row stays a function of the row's
// position in its own sequence: rows[0..n_rows) (device int32, built on the host from the lengths: the last seq_peel_rows(len) rows of every sequence
// for which gemm_seq_form(len, N, K, act) holds) go through the split-K remainder kernel, every other row through an ascending-k kernel (any of them:
// they agree bitwise, so tiles may straddle sequences).  In-place residual (R == C): the listed rows' residual is saved to r_save [n_rows][N] first,
// so the remainder launch adds the ORIGINAL residual and every row ends up written with the value of its solo run.
void launch_gemm_ragged(const GemmArgs& a, const int32_t* rows, int n_rows, bf16_t* r_save, hipStream_t st);
// one fixed configuration (kernel256: 0 = 128^2 tiles, 1 = 256^2; peel: the row remainder over a multiple of 256 in its own launch), no tuning
void launch_gemm_fixed(const GemmArgs& a, int kernel256, int peel, hipStream_t st);
int get_mt2x();
void set_mt2x(int on);                // (sv_debug_set_skinny_form / sv_debug_skinny_form) 33..64-row decode GEMMs: 1 = activations through a wave-private LDS ring (gemm_skinny_mt2x_kernel, default), 0 = both operands in registers
long long tailsplit_launches();        // host-side count of gemm_skinny_tailsplit_kernel launches since load (sv_debug_tailsplit_launches)
void set_gemm_form(int form);         // -1: tuned (default); 0 / 1: every big-M launch takes that form, rows not peeled; 2: 256^2 + the remainder peeled; 3: every row through the one-wave-per-tile kernel
// what launch_gemm decides for a shape (host arithmetic only; tail_on: 0 never peel, 1 cost model, 2 always)
struct GemmPlan { int peel, tail_rows, tail_by_tiles, main_256; double est_us; };
GemmPlan gemm_plan(int M, int N, int K, int act, int tail_on);

// ---- skinny (M<=32 per tile) weight-streaming GEMM --------------------------------------------
enum { SK_OUT_PARTIAL = 0, SK_OUT_PACKED_ACT = 1, SK_OUT_F32 = 2 };
struct SkinnyArgs {
    const bf16_t* xp;                // packed activations [MT][K/16][64][8]
    const bf16_t* Wp;                // packed weight [Npad/32][K/16][64][8]
    const uint8_t* Wq;               // fp8 image of the same weight (launch_pack_weight_fp8) or nullptr: then the fp8 kernel runs
    const float* wscale;             //   with its per-column scales [Npad]
    const bf16_t* bias;              // [N] or nullptr (PACKED_ACT only)
    int MT;                          // number of 32-row tiles
    int Npad, K;                     // Npad multiple of 32, K multiple of 16
    int splitk;                      // >=1; (K/16) must be divisible by splitk*waves
    int out_mode; int act;
    int N;                           // valid columns (<= Npad)
    float* ws; int ldws;             // PARTIAL: fp32 slabs ws[split][MT*32][ldws], summed in slab order by the consumer
    bf16_t* out_xp; int out_KS;      // PACKED_ACT: fragment-order buffer with out_KS = Npad/16 k-steps
    float* out_f32; int ldo;         // F32: [MT*32][ldo]; rounded to bf16 values if round_bf16
    int round_bf16;
    int col_tiles;                   // two-row-tile kernel (33..64 rows): column tiles per block, 1..3; 0 = the launcher's default
    int xcd_remap;                   // 1: XCD-aware (tile, K slice) assignment of a split-K launch (needs splitk | 8, (Npad/32 * splitk) % 8 == 0)
    // LayerNorm fold (decode_cols.hip; split-K 1): xp is the RAW residual stream, Wp the folded image W' = bf16(W * gamma);
    // epilogue x = rstd[m] * (acc - mean[m] * c1[n]) + c2[n], the row statistics accumulated from the activation stream in the kernel
    const float* fold_c1; const float* fold_c2;            // [Npad] (nullptr: off)
    int fold_D; float fold_eps;                            // LayerNorm width (= K) and epsilon
    // Greedy selection folded into the lm_head epilogue (F32 mode, one row tile, bf16 weights): every block leaves the best
    // (value, lowest index) of its 32 columns per row in amax[row * SV_AMAX_STRIDE] through an atomic max on a 64-bit key
    // (sv_amax_key); finish_step_kernel decodes and re-arms it.  nullptr: off.
    unsigned long long* amax; int amax_rows;               // rows < amax_rows take part
    // F32 mode (lm_head), one-row-tile bf16 kernel only: a buffer the launch fills with the 0xFFFF'FFFF pattern through write-through
    // stores, 16 bytes per thread (the LayerNorm output buffer of the fused row-update + c_attn launch of the NEXT decode step)
    void* poison; unsigned poison_bytes;
    // PACKED_ACT, one row tile, whole K (StarVector-8B's c_fc: 576 column tiles on 512 block slots): the tiles beyond the first round of blocks go to a second
    // launch that runs the one-tile kernel's 8 K ranges on 4 blocks per tile; every range leaves its raw fp32 accumulator here and a last arriver elected
    // through `tail_cnt` sums them in range order (gemm_skinny_tailsplit_kernel).
    // Per-engine scratch: [SV_TAIL_TILES][8][16][64] floats + [SV_TAIL_TILES] zeroed counters; nullptr: off.
    float* tail_ws; unsigned* tail_cnt;
    // The step's bookkeeping (finish_step_kernel) folded into the lm_head launch of a greedy step whose selection is folded already (`amax`; persistent-block
    // kernel only): every block drains its key atomics and draws a ticket from `fin_cnt` (zeroed, re-armed by the last arriver); the last block's first wave
    // decodes the keys and runs the bookkeeping.  `finish` is a HOST pointer read by the launcher (the struct rides behind SkinnyArgs in that kernel's
    // arguments); nullptr: off.  skinny_head_folds_finish(a) tells the caller whether the launch takes the bookkeeping with it.
    const struct FinishArgs* finish; unsigned* fin_cnt;
    // MXFP4 image of the same weight (launch_pack_weight_mxfp4) or nullptr: then gemm_skinny_mxfp4_kernel runs (Wp holds the dequantised values);
    // col_tiles = column tiles per block there (1, 2, 4; 0 = the launcher's default)
    const uint8_t* W4;
};
bool skinny_head_folds_finish(const SkinnyArgs& a);
#define SV_TAIL_TILES 128
#define SV_AMAX_STRIDE 16          // one 128-byte line per row: the rows' atomics do not share an L2 line
// key = (order-preserving image of the float) << 32 | (0xFFFFFFFF - column): larger value wins, equal values -> LOWER column wins
// (torch.argmax / HF _sample's tie-break, sampling.hip argmax_pair); 0 = "no finite-or-infinite score seen" (NaN never wins).
__host__ __device__ inline unsigned long long sv_amax_key(float v, unsigned col) {
    if (v != v) return 0ull;
    if (v == 0.f) v = 0.f;                                 // -0.0 == +0.0 for the comparison the argmax kernel makes
    union { float f; unsigned u; } c; c.f = v;
    const unsigned o = (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - col);
}
__host__ __device__ inline int sv_amax_index(unsigned long long key) { return key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)) : 0x7fffffff; }
void launch_gemm_skinny(const SkinnyArgs& a, hipStream_t st);
// host arithmetic of the launch: waves per block (how K is cut inside a block = the summation order of a row) and whether a
// block carries two row tiles; a function of the GEMM only for the former (sv_debug_skinny_plan, CPU tests)
// (wfmt: SV_WFMT_*)
void skinny_plan(int Npad, int K, int splitk, int wfmt, int MT, int* waves, int* two_row_tiles);
// the MXFP4 decode GEMM (mxfp4/mxfp4.hip): waves per block for (k-steps, split-K), a function of those two only (0: no K cut fits -- a wave's
// range is whole groups of 4 k-steps); the launcher returns false when the shape / mode is outside the kernel's scope
int skinny_waves_mxfp4(int KS, int splitk);
bool launch_gemm_skinny_mxfp4(const SkinnyArgs& a, hipStream_t st);
extern std::atomic<int> g_op_col_tiles;       // sv_debug_set_col_tiles: what SkinnyArgs.col_tiles == 0 means (0 = the launcher's default)

int init_gemm_kernels();        // hipFuncSetAttribute for the large-LDS variants (0 = ok)

void launch_cvt_bf16_hw(const float* x, bf16_t* y, size_t n, hipStream_t st);

// ---- the MLP half of a decode layer as one launch (mlp_fused.hip: mlp_fused_kernel; round-4 experiment, SV_EXP_MLP_FUSED_FORCE) ----
struct MlpFusedArgs {
    const bf16_t* W1; const bf16_t* x1;      // folded c_fc image W' [N1pad/32][K1/16][64][8], raw residual stream in fragment order
    int N1, N1pad, K1;
    const float* fold_c1; const float* fold_c2; int fold_D; float fold_eps; int act;
    bf16_t* out_xp; int out_KS;              // the GELU output in fragment order (N1pad = 16 * out_KS columns): phase 2's operand;
                                             // filled with 0xFFFF'FFFF by the launch in front (ColsArgs::poison)
    const bf16_t* W2; int N2, N2pad, K2;     // down projection, K2 == N1pad
    int splitk;                              // K slices of the down projection = fp32 slabs
    float* ws; int ldws; int rows_ws;        // slabs [splitk][rows_ws][ldws]
    int* err;                                // set to 3 when a block gives up waiting (never a hang)
    int spin_ticks;                          // wall-clock budget of a wave's wait in 100 MHz ticks (s_memrealtime): on expiry -- or when
                                             // *err is already set by another wave / launch -- the wave gives up (code 3)
    long long* trace;                        // optional [N1pad / 32][8] wall-clock stamps per block (tools/mlp_trace.py); nullptr in production
};
int launch_mlp_fused(const MlpFusedArgs& a, hipStream_t st);

// ---- attention output projection without slabs + LayerNorm fold (decode_cols.hip) ------------------
struct ColsArgs {
    const bf16_t* xp;                // packed activations [MT][K/16][64][8]
    const bf16_t* Wp;                // packed weight [Npad/32][K/16][64][8] (the image the 32-column kernels read)
    const bf16_t* bias;              // [N] or nullptr
    int MT, N, K;                    // K multiple of 32
    int M;                           // live rows when MT == 1 (0: not known = all 32); rows beyond it need not be written.  The row-half form
                                     // (one row tile, K <= 2048, N / 16 a multiple of 8: 16 rows x 16 columns per block) launches ceil(M / 16) halves
    int cpb;                         // output columns per block (<= 32) of the 32-row form: cols_pick_cpb(N, K)
    bf16_t* h_xp; int out_KS;        // residual stream in fragment order, N = 16 * out_KS columns: h = bf(h + bf(x W^T + b)), in place
    void* poison; unsigned poison_bytes; // optional: a buffer the blocks fill with 0xFF bytes (the fused MLP launch behind this one
                                     // recognises unwritten activations by that pattern); a multiple of 16 bytes
    void* poison2; unsigned poison2_bytes;   // optional: the NEXT layer's LayerNorm output buffer (the polled buffer of rowln_cattn_kernel), armed here with
                                     // write-through stores when the attention launch's grid is too small to carry the pattern (batches below 10 rows)
};
int cols_pick_cpb(int N, int K);
int launch_gemm_cols(const ColsArgs& a, hipStream_t st);        // 0 = ok, -1 = unsupported shape
void cols_rowhalf_launches(long long* launches, long long* halves);      // host-side counts since load: row-half launches and the row halves they ran
int init_cols_kernels();
void launch_fold_prepare(const bf16_t* Wp, const bf16_t* gamma, const bf16_t* beta, const bf16_t* bias, bf16_t* Wf, float* c1, float* c2,
                         int N, int Npad, int K, hipStream_t st);

// ---- row kernels ---------------------------------------------------------------------------------
void launch_layernorm_rows(const bf16_t* x, int ldx, const bf16_t* g, const bf16_t* b, bf16_t* y, int ldy,
                           int M, int D, float eps, hipStream_t st);
// y_packed (xp layout) variant for the decode path
void launch_layernorm_rows_packed(const bf16_t* x, int ldx, const bf16_t* g, const bf16_t* b, bf16_t* yp,
                                  int M, int D, float eps, hipStream_t st);

// decode row update: v = sum_s ws[s][m][:] + bias ; h = bf(h + bf(v)) (in place) ; xp = LN(h)
struct RowUpdateArgs {
    const float* ws; int splitk; int ldws; int rows_ws;   // partials [splitk][rows_ws][ldws] (or nullptr)
    const bf16_t* bias;
    bf16_t* h; int ldh;                                    // residual stream [M][D] (in/out); ldh == 0: fragment order (xp layout)
    const bf16_t* wte; const bf16_t* wpe;                  // embedding mode (ws == nullptr)
    const int32_t* tokens; const int32_t* positions;       // [M]
    const bf16_t* g; const bf16_t* b; float eps;           // LayerNorm applied to the updated row
    bf16_t* xp_out;                                        // packed LN output
    int M, D;
};
void launch_row_update_ln(const RowUpdateArgs& a, hipStream_t st);
// the row update and the split-K projection that consumes its LayerNorm output (c_attn) as ONE launch (rowops.hip, rowln_cattn_kernel):
// late arguments of the launch; the leading scalars (slabs, bias, residual stream, weights, shapes) travel as kernel parameters
struct RowCattnArgs {
    const bf16_t* g; const bf16_t* b; float eps; int D;
    const bf16_t* wte; const bf16_t* wpe; const int32_t* tokens; const int32_t* positions;      // embedding mode (slabs == nullptr)
    bf16_t* xp_out;                                          // LayerNorm output in fragment order = the projection's operand; pre-filled with
                                                             // the 0xFFFF'FFFF pattern by an earlier launch of the step
    float* ws_out; int ldws_out;                             // the projection's fp32 slabs [splitk][32][ldws]
    int* err; int spin_ticks;                                // give-up code 4 after spin_ticks x 10 ns of waiting (never a hang)
    int delay;                                               // GEMM blocks: 10-ns ticks between block start and the first poll
    int first_round;                                         //   ... for the blocks below this index (the ones resident when the launch starts)
    int ldh;                                                 // WIDE row role: residual row stride (0 = fragment order)
    long long* dbg; int layer;                               // optional [8]: what the first wave to give up saw (reported with the failure)
};
// 0 = launched; -1 = outside the kernel's scope (the caller runs the two launches).  sk.xp must be ru.xp_out.
int launch_rowln_cattn(const RowUpdateArgs& ru, const SkinnyArgs& sk, int* err, int spin_ticks, hipStream_t st, int delay = 390, long long* dbg = nullptr, int layer = 0,
                       int num_cus = 256);
bool rowln_cattn_fits(int D, int Npad, int K, int splitk, int splitk_ru, int num_cus);
int rowln_cattn_blocks_per_cu(bool wide);       // hipOccupancyMaxActiveBlocksPerMultiprocessor of the form on the current device
bool rowln_cattn_resident(bool wide);           // >= 2 (narrow) / 3 (wide) of them: what the launch's waits assume (logs when not)

// ---- embeddings ---------------------------------------------------------------------------------
void launch_im2col(const bf16_t* img, bf16_t* out, int B, int img_size, int patch, int Kpad, hipStream_t st);
void launch_vit_embed_lnpre(const bf16_t* patch_out, int ldp, const bf16_t* cls, const bf16_t* pos,
                            const bf16_t* g, const bf16_t* b, bf16_t* x, int B, int NP, int Dv, float eps,
                            hipStream_t st);
// row_pos (ragged prompt pass, B * S0 = packed rows): the position of every row inside its own sequence; nullptr: row % S0
void launch_dec_embed(const bf16_t* emb, const bf16_t* wpe, bf16_t* h, int B, int S0, int D, hipStream_t st, const int32_t* row_pos = nullptr);
// per_seq > 0: row r goes to out + (r / per_seq) * seq_stride + (r % per_seq) * D (token rows written behind the visual rows of a prefill buffer)
void launch_gather_rows(const bf16_t* table, const int64_t* ids, bf16_t* out, int n, int D, hipStream_t st, int per_seq = 0, size_t seq_stride = 0);
// rag_seq (ragged prompt pass): per-sequence descriptors {first packed row, length}; nullptr: sequences of S0 rows
void launch_gather_last_rows(const bf16_t* h, bf16_t* out, int B, int S0, int D, hipStream_t st, const int32_t* rag_seq = nullptr);
// out[i][:] = x[rows[i]][:] (D % 8 == 0)
void launch_gather_listed_rows(const bf16_t* x, int ldx, const int32_t* rows, int n, bf16_t* out, int D, hipStream_t st);
// ragged prompt pass: row_pos[first row of b + j] = j for j < len[b], from the descriptors {first packed row, length} [B]
void launch_ragged_row_pos(const int32_t* rag_seq, int B, int32_t* row_pos, hipStream_t st);
// shared-prefix scoring pass (prefix/prefix.hip): row_pos[first row of segment i + j] = pos0 of segment i + j for j < its length, from the
// segment descriptors {first packed row, length, pos0} [n_seg] -- a prefix starts at 0, a sequence's own rows at its prefix's length
void launch_prefix_row_pos(const int32_t* seg, int n_seg, int32_t* row_pos, hipStream_t st);
// rag_keep (ragged scoring pass): per-sequence descriptors {first packed row, length, keep, first output row}, rag_rows = sum(keep) output rows;
// nullptr: the last n_keep rows of B sequences of S0 rows
void launch_gather_tail_rows(const bf16_t* h, bf16_t* out, int B, int S0, int n_keep, int D, hipStream_t st, const int32_t* rag_keep = nullptr,
                             int rag_rows = 0);

// ---- adapter norm -------------------------------------------------------------------------------
// y_batch_stride (elements, 0 = planes back to back): the planes may be written straight into a [B][S0][D] prefill buffer
void launch_plane_layernorm(const bf16_t* x, const bf16_t* g, const bf16_t* b, bf16_t* y, int B, int QD,
                            float eps, hipStream_t st, size_t y_batch_stride = 0);
void launch_token_batchnorm(const bf16_t* x, const bf16_t* w, const bf16_t* b, const bf16_t* rm,
                            const bf16_t* rv, bf16_t* y, int B, int Q, int D, float eps, hipStream_t st, size_t y_batch_stride = 0);

// ---- attention ----------------------------------------------------------------------------------
struct AttnPrefillArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v;   // token-major buffers
    int q_row_stride, kv_row_stride;                      // elements between consecutive tokens
    int q_head_stride, kv_head_stride;                    // elements between heads (kv: 0 for MQA)
    bf16_t* o; int o_row_stride;                          // [B*S][H*D]
    int B, S, H, head_dim, kv_group;                      // kv head = head / kv_group
    int causal; float scale;
    int window = 0;                                       // causal only: query q sees keys q - window < k <= q (StarCoder2); 0 = all
    int last_rows = 0;                                    // > 0: only the query tiles holding the last `last_rows` rows of every sequence are launched
    int q_tile0 = 0;                                      //   (set by the launcher: first query tile of the grid)
    // Ragged form (causal prompt pass over packed sequences of different lengths): rag_seq [n_seq] = {first packed row, length}, rag_blocks
    // [rag_nblocks] = {sequence, query tile} -- one block per entry (x heads), query tiles counted from the sequence's first row and key tiles from
    // its key 0, exactly as in the sequence's solo launch; a block never covers rows of two sequences.  B / S / last_rows are unused then (the
    // pruned last layer passes the list of every sequence's last query tile).
    const int32_t* rag_seq = nullptr;
    const int32_t* rag_blocks = nullptr;
    int rag_nblocks = 0;
    // Prefixed form of the ragged form (the shared-prefix scoring pass): rag_seq [n_seq] = {first OWN packed row, T, first PREFIX packed row, Pl}.
    // The sequence is the solo sequence concat(prefix, own rows) of T = Pl + len rows: tiles, masks and the window are counted from solo index 0
    // as above, only the ADDRESS of solo index s changes (s < Pl: prefix row s, else own row s - Pl), and output rows with s < Pl are not stored
    // (the prefix's own launch writes them).  The caller lists only the query tiles whose last row is >= Pl.
    int rag_prefixed = 0;
};
inline int attn_prefill_q_tile(int n_head, int n_kv_head) { const int g = n_head / (n_kv_head > 0 ? n_kv_head : 1); return (g % 4 == 0 && n_head % 4 == 0) ? 32 : 128; }
void launch_attn_prefill(const AttnPrefillArgs& a, hipStream_t st);

// paged KV cache geometry (one layer):  page = 64 tokens, K|V in MFMA-fragment order, 32 KiB
#define SV_PAGE_TOKENS 64
struct KvLayout { int head_dim; int page_bytes; };
__host__ __device__ inline int kv_page_bytes(int head_dim) { return SV_PAGE_TOKENS * head_dim * 2 * 2; }
// the e4m3 cache (kv_fmt 1 = SV_KV_FP8_E4M3; csrc/kv8/kv8_dev.h): one code per element, one scale byte per token for K and for V
__host__ __device__ inline int kv8_page_bytes(int head_dim) { return SV_PAGE_TOKENS * head_dim * 2 + 2 * SV_PAGE_TOKENS; }
inline int kv_page_bytes_of(int kv_fmt, int head_dim) { return kv_fmt ? kv8_page_bytes(head_dim) : kv_page_bytes(head_dim); }

// scatter prefill K/V rows (from the c_attn output) into the paged cache
void launch_kv_write_prefill(const bf16_t* qkv, int row_stride, int k_off, int v_off, char* pool_layer,
                             const int32_t* block_table, int max_pages, int B, int S0, int head_dim,
                             hipStream_t st, int kv_fmt = 0);
// ragged form: rag_blocks [n_blocks] = {sequence, 32-token group of that sequence}; page and slot from the row's own sequence and position
void launch_kv_write_prefill_ragged(const bf16_t* qkv, int row_stride, int k_off, int v_off, char* pool_layer,
                                    const int32_t* block_table, int max_pages, const int32_t* rag_seq, const int32_t* rag_blocks,
                                    int n_blocks, int head_dim, hipStream_t st, int kv_fmt = 0);

struct AttnDecodeArgs {
    const float* ws; int splitk; int ldws; int rows_ws;   // c_attn output as fp32 split-K slabs [splitk][rows][ldws], summed here in slab order
    const bf16_t* bias;                                    //   + c_attn bias [H*D + 2*n_kv*D]
    char* pool_layer;                                      // this layer's page pool
    const int32_t* block_table; int max_pages;
    const int32_t* positions;                              // [B] index of the new token (= tokens already cached)
    bf16_t* out_xp; int out_KS;                            // packed [MT][H*D/16][64][8]
    int B, H, head_dim; float scale;
    float* part;                                           // [B][splits][32 + 16*D] partial (m, l, O)
    unsigned* counters;                                    // [B * n_kv] arrival tickets, zero between launches
    int max_splits;                                        // cap on active context splits (#CUs / (B*n_kv), <= 16)
    int n_kv;                                              // key/value heads (1 = MQA); grid.x = B * n_kv
    size_t kv_head_stride;                                 // bytes between the page pools of consecutive KV heads
    const float* rope_cos; const float* rope_sin;          // [positions][D/2] rotary tables (nullptr: no RoPE)
    int window;                                            // sliding window: keys pos - window < j <= pos (0 = all)
    int groups_per_block;                                  // 32-key groups a block takes before another context split joins (0 = 4)
    long long* trace;                                      // optional [B * n_kv * max_splits][16] wall-clock stamps (tools/attn_trace.py); nullptr in production
    void* poison2; unsigned poison2_bytes;                 // a second buffer filled the same way, by the threads behind those of the first (the next layer's
                                                           // LayerNorm output buffer: rowln_cattn_kernel)
    void* poison; unsigned poison_bytes;                   // optional: a buffer the launch fills with 0xFF bytes, 16 per thread, before anything else (the
                                                           // "not written yet" pattern of the fused MLP launch later in the layer): this kernel is bound by
                                                           // latencies, a store per thread costs it nothing -- in gemm_cols_resid_kernel it cost 0.5 us
    int kv_fmt;                                            // the pool's format (host side only: picks the instantiation): 0 bf16, 1 e4m3 + per-key scales
};
// in-place rotary embedding of the q and k heads of a prefill c_attn output (rotate_half convention)
void launch_rope_prefill(bf16_t* qkv, int row_stride, int rows, int S0, int n_heads, int head_dim,
                         const float* cos_t, const float* sin_t, hipStream_t st, const int32_t* row_pos = nullptr);
void launch_attn_decode(const AttnDecodeArgs& a, hipStream_t st);
// XCC_ID of every block of a 1-D launch of `blocks` 8-wave blocks (heavy = 1: with the decode attention's LDS footprint and 10 us of residence)
int launch_xcc_probe(int32_t* out, int blocks, int heavy, hipStream_t st);
int launch_occupy(int blocks, int lds_bytes, int ticks, hipStream_t st);     // test tenant: pins LDS of `blocks` CUs for ticks x 10 ns
size_t attn_decode_part_floats(int head_dim);            // floats of `part` per sequence
int init_attention_kernels();   // returns a hipError_t value (0 = ok)
// tokens [first, first + count) of one block-table row as the decode attention sees them: out bf16 [count][2 * n_kv * head_dim] (k heads | v heads),
// either pool format (csrc/kv8/kv8.hip)
struct KvReadArgs { const char* pool_layer; size_t kv_head_stride; const int32_t* table_row; int n_kv, head_dim, first, count, kv_fmt; bf16_t* out; };
void launch_kv_read(const KvReadArgs& a, hipStream_t st);
// The extension pass's two page kernels (csrc/extend/extend.hip), one layer, grid (n_blocks, n_kv).  xseq: one descriptor per sequence of the pass,
// {block-table row, first packed own row, ctx, len, first row of its region of gkv or -1, 0}; blocks: {descriptor, 32-token group} x n_blocks.
//   launch_kv_gather        tokens [0, ctx) of every listed group, pages of either format -> rows region + token of gkv (bf16 [..][gkv_stride]:
//                           k heads | v heads), as the decode attention sees them
//   launch_kv_write_extend  the own rows (packed rows of qkv, K at column k_off + head * head_dim, V at v_off + ...) -> pages at positions ctx + j, every
//                           cached token's bytes kept; and, unquantised, -> rows region + ctx + j of gkv (region -1: no copy)
struct ExtKvArgs {
    const bf16_t* qkv; int row_stride, k_off, v_off;
    char* pool_layer; size_t kv_head_stride; const int32_t* table; int max_pages;
    const int32_t* xseq; const int32_t* blocks; int n_blocks;
    int head_dim, n_kv, kv_fmt;
    bf16_t* gkv; int gkv_stride;
};
void launch_kv_gather(const ExtKvArgs& a, hipStream_t st);
void launch_kv_write_extend(const ExtKvArgs& a, hipStream_t st);

// ---- sampling -----------------------------------------------------------------------------------
// greedy selection: per-slice winners (pval/pidx: [B][8]) then a merge (standalone, or inside finish_step)
// seen / penalty: HF RepetitionPenaltyLogitsProcessor (bitmap of generated ids per row, [B][seen_words]); nullptr = off
void launch_argmax_partial(const float* logits, int ld, int V, float* pval, int32_t* pidx, int B, const uint32_t* seen,
                           int seen_words, float penalty, hipStream_t st);
void launch_argmax(const float* logits, int ld, int V, int32_t* out, float* pval, int32_t* pidx, int B, hipStream_t st);
struct SampleArgs {
    const float* logits; int ld; int V; int B;
    float temperature, top_p; int top_k;                             // top_k <= 0: off
    uint64_t seed; const int32_t* step;                              // device step counter
    int32_t* out; float* scratch;                                    // scratch >= B*4 floats
    const uint32_t* seen; int seen_words; float penalty;             // repetition penalty (nullptr = off)
    float minp_log = -INFINITY;                                      // HF MinPLogitsWarper after top-p: log(min_p), -inf = off
};
void launch_sample_top_p(const SampleArgs& a, hipStream_t st);

struct FinishArgs {
    const int32_t* next;          // [B] raw sampled ids (sampling path)
    const float* pval; const int32_t* pidx;   // greedy path: [B][8] slice winners merged here (or nullptr)
    unsigned long long* amax;     // greedy path, selection folded into the lm_head launch: keys [B * SV_AMAX_STRIDE] (SkinnyArgs::amax),
                                  // decoded and re-armed (zeroed) here; nullptr: off
    int32_t* cur_tok;             // [B] token fed to the next step
    int32_t* unfinished;          // [B]
    int32_t* positions;           // [B] (+1 each step)
    int32_t* out_tokens; int ld_out;   // [B][max_new]
    int32_t* step;                // device scalar: number of tokens emitted so far
    int32_t* done;                // device scalar: 1 once generation has ended
    int32_t* n_emitted;           // device scalar: final column count
    const int32_t* stop_ids; int n_stop;
    int eos, pad, B, max_new;
    uint32_t* seen; int seen_words;   // repetition-penalty bitmap to update with the emitted ids (nullptr = off)
    int V; int32_t* bad;          // vocabulary size; device flag raised when a row has no valid token (all logits NaN): the id
                                  // fed to the next step is then 0, never an out-of-range row of the embedding table
};
void launch_finish_step(const FinishArgs& a, hipStream_t st);

// ---- per-step outputs of sv_generate_ex (HF output_scores / output_logits) ------------------------------------------
// Device-resident descriptor of the caller's slabs, rewritten by the host for every call: a captured decode graph keeps only
// the descriptor's address, so two calls with different output tensors replay the same graph correctly.
struct CaptureDesc {
    float* scores;                 // [max_new][rows][ld] processed row (nullptr: not requested)
    float* logits;                 // [max_new][rows][ld] raw row (nullptr: not requested)
    long long ld;                  // >= V
    int rows, max_new;
};
// greedy / sampling: row b of `src` at the device step t = *step (nothing once *done or t >= max_new).  The processed row is what the
// selection ranks: RepetitionPenalty over the seen bitmap, the min-length EOS hold, and (do_sample) temperature as s / T with the
// tokens outside TopK -> TopP at -inf.  Runs BEFORE suppress_token rewrites the EOS logit in place.
struct CaptureArgs {
    const CaptureDesc* desc;
    const float* src; int ld_src; int V; int B;
    const int32_t* step; const int32_t* done;
    const uint32_t* seen; int seen_words; float penalty;             // seen = nullptr: penalty off
    int eos, min_new;                                                // min_new <= 0: hold off
    int do_sample; float temperature, top_p; int top_k;
    float* warp;                                                     // [B][8] per-row warper thresholds (do_sample)
    float minp_log = -INFINITY;                                      // do_sample: min_p after top-p (log(min_p), -inf = off)
    int what = 3;                                                    // 1 = the raw row, 2 = the processed row, 3 = both (a call with token bans
                                                                     //   takes them apart: raw row -> ban_tokens_kernel -> processed row)
};
void launch_capture_rows(const CaptureArgs& a, hipStream_t st);

// ---- per-token statistics of sv_generate_stats: for the token row b emits at the device step t = *step, three fp32 values at [b][t] of the
// caller's [rows][ld] buffers (reached through a device-resident descriptor, like CaptureDesc: a kept graph writes each call's own buffers)
//   logprob   = log_softmax(x / T)[tok], x the raw lm_head row, T = temperature when do_sample, else 1
//   entropy   = entropy of softmax(x / T)                                   (score.hip's definition)
//   processed = log_softmax(s)[tok], s the row the selection ranks -- bans, repetition penalty, min-length hold, and (do_sample) s / T with the
//               ids outside TopK -> TopP -> min_p at -inf.  The kept set is the CAPTURE's (capture_warp_kernel: the sampler's score functor through
//               row_warp_stats and wp_keep), so the value is log_softmax of the dev_scores row bit for bit in its inputs; with 0 < top_k <= 256 the
//               sampler itself draws through sample_row_topk, whose top-p test has no round-off slack -- its kept set lies inside this one
// A row that had finished before step t gets 0 in all three.  The launch sits BETWEEN the selection and finish_step_kernel: the token is known
// (next, or the AM_SPLIT slice winners of the greedy path), while *step, *done, unfinished[] and the seen bitmap still describe step t.
struct TokenStatsDesc {
    float* logprob; float* processed; float* entropy;    // [rows][ld] each, nullptr: not requested
    long long ld;                                        // >= max_new
    int rows, max_new;
};
struct TokenStatsArgs {
    const TokenStatsDesc* desc;
    const float* src; int ld_src; int V; int B;
    const int32_t* step; const int32_t* done; const int32_t* unfinished;
    const int32_t* next;                                             // sampling: [B] drawn ids
    const float* pval; const int32_t* pidx;                          // greedy: [B][8] slice winners (nullptr when sampling)
    const uint32_t* seen; int seen_words; float penalty;             // seen = nullptr: penalty off
    int eos, min_new;                                                // min_new <= 0: hold off
    int do_sample; float temperature, top_p; int top_k;
    float minp_log = -INFINITY;
    float* raw;                                                      // [B][4] {max, log sum exp(x - max), entropy} of the raw row
    int what = 3;                                                    // 1 = the raw row's statistics into `raw` (a call whose step rewrites the row in place -- a
                                                                     //   ban, the min-length hold -- takes them in front of the rewrite), 2 = the outputs, from
                                                                     //   `raw` and the row as the selection saw it, 3 = both in one launch
};
void launch_token_stats(const TokenStatsArgs& a, hipStream_t st);

// ---- the k best ids of the distribution behind each generated token, and the token's rank (sv_generate_topk; topk.h row_topk).  For the device step
// t = *step, row b writes k ids and k log-probs at [b][t][0..k) and its rank at [b][t] of the caller's buffers (device descriptor, as above).
//   source 0  the distribution of TokenStatsDesc::logprob: log_softmax(x / T) over the raw row.  When the step rewrites the raw row in place (a ban,
//             the min-length hold) the launch sits in front of the rewrite, where the token is not known yet: no rank then (want_rank = 0)
//   source 1  the distribution of TokenStatsDesc::processed: the processed row with the capture's kept set, removed ids at -inf (they never enter)
// Descending by value, equal values by ascending id; a slot's log-prob is the expression token_stats_kernel writes for that id, bit for bit.  Fewer
// than k ids that enter: the tail holds (-1, -inf).  A row that had finished before step t: ids -1, log-probs 0, rank 0.  A row without a
// comparable value: ids -1, rank 0, log-probs NaN.  k, source and want_rank are launch arguments (the captured step is keyed on them).
#define SV_TOPK_MAX_DEV 32                                   // == SV_TOPK_MAX (include/starvector_hip.h; static_assert in engine_generate.hip)
struct TokenTopkDesc {
    int32_t* ids; float* logprobs;                       // [rows][ld][k]
    int32_t* rank;                                       // [rows][ld], nullptr: not requested
    long long ld;                                        // >= max_new
    int rows, max_new;
};
struct TokenTopkArgs {
    const TokenTopkDesc* desc;
    const float* src; int ld_src; int V; int B;
    const int32_t* step; const int32_t* done; const int32_t* unfinished;
    const int32_t* next;                                             // sampling: [B] drawn ids
    const float* pval; const int32_t* pidx;                          // greedy: [B][8] slice winners (nullptr when sampling)
    const uint32_t* seen; int seen_words; float penalty;             // seen = nullptr: penalty off
    int eos, min_new;                                                // min_new <= 0: hold off
    int do_sample; float temperature, top_p; int top_k;
    float minp_log = -INFINITY;
    int k, source, want_rank;
};
void launch_token_topk(const TokenTopkArgs& a, hipStream_t st);
// the source-0 row function on caller-given rows (sv_op_token_topk): rows [B][ld] fp32, tokens [B] or nullptr (no rank), outputs [B][k] / [B]
struct TokenTopkRowsArgs {
    const float* rows; int ld; int V; int B; float temperature;
    const int32_t* tokens; int k;
    int32_t* ids; float* logprobs; int32_t* rank;
};
void launch_token_topk_rows(const TokenTopkRowsArgs& a, hipStream_t st);
#ifdef __HIPCC__
// one thread block's share of a captured row: out[j] = f(j) for j in [0, V), with 16-byte stores wherever `out` allows (the slab
// rows are ld floats apart, ld need not be a multiple of 4); the block takes quads [q0, q1) of the aligned body, block 0 the
// unaligned head and the tail (< 4 elements each)
template <class F>
__device__ __forceinline__ void capture_store_row(float* out, int V, int q0, int q1, bool edges, F f) {
    const int head = min((int)((4u - (unsigned)(((uintptr_t)out >> 2) & 3u)) & 3u), V);
    const int nq = (V - head) >> 2;
    const int tail0 = head + 4 * nq;
    q1 = min(q1, nq);
    for (int q = q0 + (int)threadIdx.x; q < q1; q += (int)blockDim.x) {
        const int j = head + 4 * q;
        *reinterpret_cast<float4*>(out + j) = make_float4(f(j), f(j + 1), f(j + 2), f(j + 3));
    }
    if (edges) {
        const int i = (int)threadIdx.x;
        if (i < head) out[i] = f(i);
        if (tail0 + i < V && i < 4) out[tail0 + i] = f(tail0 + i);
    }
}
#endif
#ifdef __HIPCC__
// the per-row part of the bookkeeping (row b takes token `nxt` at step t): returns whether the row is still generating
__device__ __forceinline__ int finish_step_row(const FinishArgs& p, int b, int t, int nxt) {
    const int unf = p.unfinished[b];
    if (unf && (unsigned)nxt >= (unsigned)p.V) {     // no finite logit in this row: never index the embedding table with it
        nxt = 0;
        if (p.bad) atomicCAS(p.bad, 0, 1);          // 0 -> 1 only: a code already there (3 = the fused MLP launch gave up) survives
    }
    const int tok = unf ? nxt : p.pad;
    p.out_tokens[(size_t)b * p.ld_out + t] = tok;
    p.cur_tok[b] = tok;
    if (p.seen && tok >= 0) atomicOr(p.seen + (size_t)b * p.seen_words + (tok >> 5), 1u << (tok & 31));
    const int still = unf && tok != p.eos;
    p.unfinished[b] = still;
    p.positions[b] += 1;
    return still;
}
// the call's part (one thread, after every row's): stop sequence on row 0, step counter, end of generation
__device__ __forceinline__ void finish_step_call(const FinishArgs& p, int t, int any_unf) {
    bool fired = false;
    if (p.n_stop > 0 && t + 1 >= p.n_stop) {
        fired = true;
        for (int i = 0; i < p.n_stop; ++i)
            if (p.out_tokens[t + 1 - p.n_stop + i] != p.stop_ids[i]) { fired = false; break; }
    }
    *p.step = t + 1;
    if (fired || !any_unf || t + 1 >= p.max_new) {
        *p.done = 1;
        *p.n_emitted = t + 1;
    }
}
#endif

// ---- HF logits processors that ban tokens (processors.hip): NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor over a row's
// generated ids.  One block per row writes -inf at the banned ids of the row's fp32 logits, in place, between the lm_head and the selection.
#define SV_BAN_MAXNGRAM 8
#define SV_BAN_MAXWORDS 64
#define SV_BAN_MAXLEN 8
struct BanWord { int32_t len; int32_t id[SV_BAN_MAXLEN]; };          // device-resident table entry: one bad-word sequence
struct BanArgs {
    float* logits; int ld; int V; int B;                             // [B][ld] fp32 rows, V valid columns
    const int32_t* hist; int ld_hist;                                // [B][ld_hist] generated ids of every row (the engine's out_tok)
    const int32_t* step;                                             // device scalar: ids generated so far, the same for every row ...
    const int32_t* hist_len;                                         //   ... or [B] lengths, one per row (the operator's test surface); nullptr: *step
    const int32_t* done;                                             // device scalar or nullptr: nothing is written once it is set
    int ngram;                                                       // no_repeat_ngram_size: 0 = off, 1 .. SV_BAN_MAXNGRAM
    const BanWord* words; int n_words;                               // bad-word table, 0 .. SV_BAN_MAXWORDS entries
};
void launch_ban_tokens(const BanArgs& a, hipStream_t st);

// ---- continuous batching: one request per row ("slot"), everything per row (sampling.hip) ---------------------------
#define SV_CB_MAXSTOP 16
#define SV_CB_MAXANY 8
#define SV_CB_MAXBIAS 128
struct CbSlot {                  // device-resident, one per slot
    int32_t live;                // 1 = generating
    int32_t step;                // tokens emitted so far
    int32_t budget;              // new-token budget of the request
    int32_t do_sample; float temperature, top_p; int32_t top_k;
    int32_t eos, pad, min_new; float penalty;
    int32_t n_stop; int32_t stop[SV_CB_MAXSTOP];
    int32_t base;                // prompt length: the slot's column c sits at position base + c (set and read by the drafting batch only)
    uint64_t seed;
    // vLLM 0.5.5 sampler semantics (vllm = 1): before the selection the slot's block rewrites its logits row in place with
    // logit_bias (CbBias), the min_tokens hold (eos and every `any` id -> -inf), repetition over the seen bitmap (prompt ids
    // seeded at admit, output ids added per step), frequency and presence over the output counts; min_p after top-p
    int32_t vllm;
    float presence, frequency, min_p;            // min_p 0 = off
    int32_t n_bias, n_any;
    int32_t any[SV_CB_MAXANY];                   // stop_token_ids: any one of them ends the request (not a sequence)
};
struct CbBias { int32_t id[SV_CB_MAXBIAS]; float val[SV_CB_MAXBIAS]; };     // device-resident, one per slot
// Per-slot log-prob record (device-resident, one per slot; the buffers are the engine's, allocated at the first admit that asks): at its step t a
// recording slot writes the emitted token's log-prob and rank at [t] and the k best ids / log-probs of the step's distribution at [t][0..k), all
// inside the selection's own block -- after the token is known, before the seen bitmap and the counts take it.  The definitions are those of
// sv_generate_topk (TokenTopkArgs above): source 0 = log_softmax(raw / T) (HF slots only: a vLLM slot has rewritten its row by then), source 1 =
// the row the selection saw with the sampler's kept set, removed ids at -inf.  The step graph holds the address of this array, never a buffer's.
struct CbLogprobs {
    int32_t enable;              // 0: the slot records nothing (and runs none of the code)
    int32_t k;                   // 0..SV_TOPK_MAX_DEV list entries per step
    int32_t source;              // 0 raw, 1 processed
    int32_t pad_;
    float* logprob; int32_t* rank;       // [budget]
    int32_t* ids; float* lps;            // [budget][k]
};
struct CbStepArgs {
    const float* logits; int ld; int V;
    CbSlot* slots; const int32_t* slot_map;      // block b works for slot slot_map[b] (nullptr: b) on logits row b
    int32_t* cur_tok; int32_t* positions; int32_t* out_tokens; int ld_out;
    uint32_t* seen; int seen_words;
    int32_t* n_live; int32_t* events;           // device counters: live slots, finished-slot events
    int32_t* bad;                               // raised when a slot has no valid token (all logits NaN); the id becomes 0
    // vLLM-mode slots only: output-token counts [slot][ld_counts] (uint16: any budget below 65 536 tokens, checked at admit)
    // and the logit bias entries per slot.  The logits rows are rewritten in place for those slots.
    uint16_t* counts; int ld_counts;
    const CbBias* bias;
    // per-slot log-prob records (sv_cb_admit_logprobs): nullptr = nobody records, the plain kernel runs -- the launch of every batch without them
    const CbLogprobs* lp = nullptr;
};
void launch_cb_step(const CbStepArgs& a, int nblocks, hipStream_t st);

// ---- prompt-lookup drafting in the continuous batch (cb_lookup/cb_lookup.hip; sv_cb_set_lookup).  A slot owns K1 = K + 1 decode rows:
// rows s * K1 + j of cur_tok / positions / the block table and of the step's logits.  Row 0 carries the slot's last emitted id at its position,
// rows 1 .. n_draft[s] the drafts behind it, the rest are copies of row 0 (lk_write_rows' layout).  One block per slot verifies the rows ONE
// AFTER THE OTHER with the plain step's own row body (cb_row.h): after every committed token the slot's state is the plain batch's at that
// column, so the next row is selected exactly as the plain batch would select it -- and it is looked at only if its draft was the token just
// emitted.  Then the block drafts from the slot's history (lk_draft.h) and writes the rows of the next step.
// first != 0: the first token of a new request.  Block b works for slot slot_map[b] on logits row b (the prompt pass's), there are no drafts.
struct CbLookupArgs {
    CbStepArgs st;                               // as the plain step's; slots, out_tokens, seen, counts, bias, lp indexed by slot
    int K, max_ngram, min_ngram, first;
    int32_t* n_draft;                            // [slots] live drafts of the step in flight
    int32_t* counts;                             // [slots][3] {verification steps, drafts verified, drafts accepted} since the slot's admit
    int32_t* totals;                             // [3] the same over every slot since the batch began (steps: one per slot and step)
    const int32_t* forced; int forced_n, forced_ld;      // sv_debug_cb_set_lookup_drafts: draft j of slot s < forced_n is forced[s][step_s + j]
};
void launch_cb_lookup_step(const CbLookupArgs& a, int nblocks, hipStream_t st);

// ---- shared prompt pass (fork.hip): one prompt, several samples.  Between the prompt pass and the first selection, on the engine stream:
//   (a) the partially filled tail page of prompt u (len % 64 != 0) fans out from the row that took the prompt pass to the other rows of the prompt,
//       for every layer and KV head (the full prompt pages are shared through the block table and never copied);
//   (b) logits row i becomes logits row lsrc[i] (in place): every sample selects its first token from its prompt's prefill logits.
// Descriptors (device int32): prompts [n_prompts][4] = {row holding the prompt, prompt length, first entry in dst_rows, entries}; dst_rows = the
// other rows of each prompt; lsrc [n_rows] with lsrc[i] <= i (the in-place fan-out walks the rows downwards: a row is read before any row
// above it is written).  Rows index block_table ([rows][max_pages]): decode rows of sv_generate_shared, slots of sv_cb_admit_shared.
struct ForkArgs {
    const int32_t* prompts; const int32_t* dst_rows; int n_prompts;
    const int32_t* block_table; int max_pages;
    char* kv_pool; size_t layer_stride, kv_head_stride; int n_layer, n_kv; int page_bytes;
    float* logits; int ld; const int32_t* lsrc; int n_rows;
};
void launch_fork_prompt(const ForkArgs& a, hipStream_t st);

// ---- per-token log-probabilities of the scoring forward (score.hip): one block per row of bf16 logits, fp32 arithmetic over
// x_i = float(logit_i) * inv_t.  logits rows start 16-byte aligned and ld % 8 == 0.  Every output may be nullptr.
struct LogprobArgs {
    const bf16_t* logits; int ld; int V; int R;     // [R][ld], V valid columns
    const int32_t* targets;                         // [R]; -100 = ignore (logprob 0); nullptr = every row ignored
    float inv_t;                                    // 1 / temperature, > 0
    float* logprob; float* lse; float* entropy; int32_t* argmax;      // [R]: x_target - lse | lse | entropy | first maximal index
    int32_t* bad;                                   // device int32[2] or nullptr: [0] |= 1 (a target outside [0, V) and not -100: logprob NaN) / 2 (a row
    int row0;                                       //   without a finite logit: all outputs NaN, argmax -1); [1] = min(row0 + row) over such rows
};
void launch_logprob_rows(const LogprobArgs& a, hipStream_t st);
// the k best columns of the same rows and the rank of the target (sv_forward_topk; topk.h row_topk): one 1024-thread block per row, after
// launch_logprob_rows has left the row's lse.  Slot j holds float(logit) * inv_t - lse of its column -- logprob_rows' own expression: the slot of the
// target equals LogprobArgs::logprob bit for bit; slot 0's id is LogprobArgs::argmax.  Target -100 (or outside the vocabulary): rank 0.  A row whose
// lse is NaN because it has no comparable value: ids -1, log-probs NaN, rank 0.
struct TopkRowsArgs {
    const bf16_t* logits; int ld; int V; int R;     // [R][ld], V valid columns
    const int32_t* targets;                         // [R] or nullptr
    float inv_t;
    const float* lse;                               // [R], from launch_logprob_rows over the same rows and inv_t
    int k;                                          // 1 .. 32
    int32_t* ids; float* logprobs;                  // [R][k]
    int32_t* rank;                                  // [R] or nullptr
};
void launch_topk_rows_bf16(const TopkRowsArgs& a, hipStream_t st);

// ---- image pre-processing (preprocess.hip): uint8 HWC (3 or 4 channels) -> float32 [3][S][S], returns a hipError_t value
int preprocess_image(const uint8_t* dev_pixels, int width, int height, int channels, int out_size, int recipe,
                     const float* mean3, const float* std3, float* dev_out, hipStream_t st);
// batched + stateless: n images (any sizes) -> [n][3][S][S]; the caller owns the workspace (preprocess_workspace_bytes);
// nothing is copied from the host or synchronised inside.  Returns a hipError_t value, or -1 if the workspace is too small.
size_t preprocess_workspace_bytes(const int32_t* widths, const int32_t* heights, int n, int out_size, int recipe);
int preprocess_images(const uint8_t* const* dev_pixels, const int32_t* widths, const int32_t* heights, const int32_t* channels,
                      int n, int out_size, int recipe, const float* mean3, const float* std3, float* dev_out, void* workspace,
                      size_t workspace_bytes, hipStream_t st);

// ---- prompt-lookup speculative decoding (lookup/lookup.hip; DESIGN.md "Prompt-lookup decoding").  One verification step is a decode step over
// n_seq x (K + 1) rows: row s * (K + 1) + j carries sequence s's last accepted token (j = 0) or its j-th draft, at position ctx_s + j, and its
// block-table row is a copy of sequence s's -- all K + 1 rows alias the same pages.
// The pre-write, per layer, between c_attn and the decode attention: EVERY row's k_new | v_new goes into its page slot with the arithmetic of
// attn_decode_kernel (slabs summed in slab order, + bias, bf16; RoPE at the row's position with the same one-by-one bf16 roundings), so that
// the unmodified attention kernel reads from the cache, for the siblings in front of a row, the bits a sequential decode would have left there.
struct LookupKvArgs {
    const float* ws; int splitk; int ldws; int rows_ws; const bf16_t* bias;      // the c_attn slabs, as AttnDecodeArgs has them
    char* pool_layer; const int32_t* block_table; int max_pages; const int32_t* positions;
    int rows, H, head_dim, n_kv; size_t kv_head_stride;
    const float* rope_cos; const float* rope_sin;                                // nullptr: no rotary embedding
};
void launch_lookup_kv_write(const LookupKvArgs& a, hipStream_t st);
// The call's state on the device.  Per sequence: tokens emitted, finished, prompt length, live drafts of the step in flight.  Per call: counts =
// {verification steps, drafts verified, drafts accepted}; limit = the column count row 0's stop sequence allows (max_new until it fires);
// ticket = arrivals of lookup_step_kernel's blocks (zero between launches).
struct LookupArgs {
    int32_t *n_emit, *fin, *base, *n_draft, *counts, *limit; unsigned* ticket;
    int n_seq, K, max_ngram, min_ngram;
    int32_t* cur_tok; int32_t* positions;           // [n_seq * (K + 1)] the next step's input rows
    const int32_t* unfinished;                      // lookup_begin: [n_seq] as the first token's bookkeeping left it
    int32_t* out_tok; int ld_out;                   // [n_seq][ld_out] every sequence's generated ids, at its own column
    const float* pval; const int32_t* pidx;         // [rows][8] slice winners of launch_argmax_partial
    int32_t *done, *n_emitted, *bad;                // the call's device scalars (FinishArgs)
    const int32_t* stop_ids; int n_stop; int eos, pad, max_new, V;
    const int32_t* forced; int forced_ld;           // sv_debug_set_lookup_drafts: draft j of sequence s is forced[s][n_emit_s + j]; nullptr: the lookup
};
void launch_lookup_begin(const LookupArgs& a, hipStream_t st);       // after the first token: rows 0 .. n_seq of cur_tok / positions -> the row layout
void launch_lookup_step(const LookupArgs& a, hipStream_t st);        // accept, emit, stop / EOS / budget, draft the next step
// the min-length hold of a verification step: logits[row][eos] = -inf while n_emit[row / K1] + row % K1 < min_new (in front of the argmax)
void launch_lookup_hold_eos(float* logits, int ld, int eos, const int32_t* n_emit, int K1, int min_new, int rows, hipStream_t st);

// ---- the sampled / penalised selection of a verification step (lookup_sampled/lookup_sampled.hip; sv_generate_lookup_sampled).
// Row r = s * K1 + j draws one token from its row of `logits` with the plain sampler's own code (sample_row.h) and the triple the plain call
// uses at that column: (seed, step = n_emit[s] + j, row = s).  The token is handed to lookup_step_kernel in the form it merges: slice 0 of the
// row's pval / pidx = (0, token), the other slices (-inf, 0x7fffffff); a row without a finite score holds the sentinel in every slice.
struct LookupSampleArgs {
    const float* logits; int ld; int V; int rows; int K1;
    const int32_t* n_emit;                                           // [rows / K1]
    const int32_t* done;                                             // device scalar or nullptr: nothing is drawn once it is set
    float temperature, top_p; int top_k; uint64_t seed;
    const uint32_t* seen; int seen_words; float penalty;             // [rows][seen_words] per ROW (lookup_seen_kernel); nullptr = off
    float* pval; int32_t* pidx;                                      // [rows][8]
};
void launch_lookup_sample(const LookupSampleArgs& a, hipStream_t st);
// The repetition penalty's seen sets of a verification step, one block per sequence behind lookup_step_kernel:
//   seq_seen[s] |= { out_tok[s][c] : seq_cols[s] <= c < n_emit[s] }, seq_cols[s] = n_emit[s]          (the ids the step emitted)
//   row_seen[s * K1 + j] = seq_seen[s] | { cur_tok[s * K1 + 1 .. j] } for j <= n_draft[s], = seq_seen[s] for the dead rows behind
// begin != 0 (the launch behind lookup_begin_kernel): seq_seen holds the sets the first token's bookkeeping left, nothing is emitted.
struct LookupSeenArgs {
    uint32_t* seq_seen; int32_t* seq_cols;                           // [n_seq][words], [n_seq]
    uint32_t* row_seen;                                              // [n_seq * K1][words]
    int words, n_seq, K1, begin;
    const int32_t *n_emit, *n_draft, *cur_tok;                       // as lookup_step_kernel left them
    const int32_t* out_tok; int ld_out;
    const int32_t* done;                                             // device scalar or nullptr
};
void launch_lookup_seen(const LookupSeenArgs& a, hipStream_t st);

}  // namespace sv
