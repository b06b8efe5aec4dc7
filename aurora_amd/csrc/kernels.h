// Internal kernel-launcher interface (C++ side, not part of the C ABI).
#pragma once
#include "common.h"

enum { EPI_ROW = 0, EPI_QKV = 1 };
enum { ACT_NONE = 0, ACT_QUICK_GELU = 1, ACT_GELU = 2, ACT_SILU_MUL = 3, ACT_SILU = 4, ACT_RELU = 5, ACT_GELU_TANH = 6 };   // 1, 2, 4, 5, 6 = AUR_ACT_*

struct GemmArgs {
    const half_t* A;        // [M, K] row-major activations
    int lda;
    const half_t* W;        // FRAG-packed weights [Npad/16][K/32][512]
    const float* bias;      // [Npad] fp32 or nullptr
    int M, Npad, K;         // Npad % 128 == 0, K % 64 == 0
    // ---- EPI_ROW
    half_t* C;              // row-major output
    int ldc;
    const half_t* resid;    // optional residual [M, ldr] (may alias C)
    int ldr;
    const int32_t* out_rows;   // optional output row map (m -> row of C, <0 = drop)
    int act;
    int n_real;             // columns actually stored (ACT_SILU_MUL stores n_real/2)
    // ---- EPI_QKV
    int rows_per_seq;       // rows of A per sequence / frame (multiple of 32)
    int q_cols, k_cols;     // padded column counts of the Q and K regions (multiples of 64)
    int hd;                 // true head dim (V region head width; rope table row = hd/2)
    half_t* Qf;             // Q fragments [seq][head][tok16][kblk][FRAG]
    KvLayout kv;            // K fragments / V^T fragments destination
    const float2* rope;     // [pos][hd/2] (cos, sin) or nullptr
    int pos0;               // position of row 0 of each sequence (multiple of 32); > 0: a tail (pruned last layer) or an extend pass
    int seq0;               // first sequence's row in the page table
    const int32_t* tail_lens;  // non-null (the pruned last layer of a variable-length prefill): sequence i's rows are the rows_per_seq rows that
    int tail_cap;              // end at round_up(len_i, 32), so its first row's position is `pos0` (the position of the pass's row 0: 0, or an
                               // extend's pos0) + var_row0(var_len(tail_lens, i, tail_cap), rows_per_seq)
    // ---- per-ctx tuning knobs (aur_set_option; filled by the engine at every launch - nothing is process-global)
    int gemm_mode;          // 0: 128x128 kernel only, 1: auto, 2: force 256x256 when Npad % 256 == 0
    int max_wgs;            // 256x256 kernel: > 0 = at most this many persistent workgroups (= CUs); 0 = one per CU
    int tail_split;         // 1 = a mostly idle last round of the 256x256 kernel is replaced by a 128x128 launch over the bottom rows
    int nt_out;             // 1 = the output of this launch is larger than the L2s together: written with non-temporal stores (ctx_gemm)
    int tag;                // GT_*: which projection of the path this is.  No effect on the arithmetic: the 256x256 kernel is
                            // instantiated once per tag so that profiler traces (rocprofv3 groups by kernel NAME; the persistent
                            // grid is the same for every shape) separate the shapes - profiles/*_kernel_stats.txt, *_pmc.json
};
enum { GT_OTHER = 0, GT_VIT_QKV, GT_VIT_OUT, GT_VIT_FC1, GT_VIT_FC2, GT_LLM_QKV, GT_LLM_O, GT_LLM_GATEUP, GT_LLM_DOWN, GT_COUNT };

hipError_t gemm_init();
hipError_t attn_init();
hipError_t tome_init();
hipError_t skinny_init();
hipError_t launch_gemm(const GemmArgs& a, int epi, hipStream_t s);
// gemm256.hip: 256x256x64 staggered two-group kernel for large shapes (auto-selected by launch_gemm)
hipError_t gemm256_init();
bool gemm256_eligible(const GemmArgs& a);
int gemm256_grid_cap();           // persistent workgroups of the 256x256 kernel when max_wgs == 0
hipError_t launch_gemm256(const GemmArgs& a, int epi, hipStream_t s);
hipError_t launch_pack_weight(const half_t* w, int n_src, int k_src, int ld_src, const int32_t* row_map, int npad,
                              int kpad, half_t* out, hipStream_t s);

// ---- norm.hip
hipError_t launch_layernorm(const half_t* x, int ldx, const float* w, const float* b, float eps, int rows, int d,
                            half_t* y, int ldy, hipStream_t s);
hipError_t launch_rmsnorm(const half_t* x, int ldx, const float* w, float eps, int rows, int d, half_t* y, int ldy,
                          hipStream_t s);

// ---- attn.hip (prefill / ViT flash attention over fragments)
struct AttnArgs {
    const half_t* Qf;       // [seq][head][tok16][kblk][FRAG]
    KvLayout kv;
    int seq0;               // page-table row of sequence 0
    int nseq, heads;
    int rows_per_seq;       // padded query rows per sequence (multiple of 32)
    int t;                  // valid keys / queries per sequence
    int causal;
    float scale;            // softmax scale (hd^-0.5)
    half_t* O;              // [nseq*rows_per_seq, ldo] row-major, head h at columns h*hd
    int ldo;
    int hd;
    int nqb;                // filled by launch_attention: query blocks of 128 rows per sequence
    int q_pos0;             // position of query row 0 of every sequence among its keys (causal mask): 0 = the Q buffer starts at the
                            // sequence's first token; > 0 = it holds only a tail of the sequence (the pruned last prefill layer)
    const int32_t* seq_lens;   // non-null: valid keys / queries of sequence i = var_len(seq_lens, i, len_cap) instead of `t` (device memory);
    int len_cap;               // query rows at or beyond a sequence's length are stored as zeros
    int q_tail;                // with seq_lens: 1 = q_pos0 of sequence i is len_pos0 + var_row0(len_i, rows_per_seq) (the pruned last layer)
    int len_pos0;              // with seq_lens: positions the sequence held before this pass (aur_llm_extend_*; 0 = a prefill) - the lengths count
                               // the rows of the pass, so valid keys = len_pos0 + len_i, and q_pos0 of an untailed pass is len_pos0 (set by the caller)
};
hipError_t launch_attention(const AttnArgs& a, hipStream_t s);

// ---- tome.hip
struct TomeArgs {
    int frames, t, t_pad, r, c;      // c = metric channels (head_dim); r already clamped, > 0
    int d;                           // hidden size
    const float* metric;             // [frames][t][c] fp32
    const half_t* x;                 // [frames][t_pad][d]
    const float* size;               // [frames][t_pad] (nullptr = ones)
    int t_out_pad;                   // padded rows per frame of the output
    half_t* x_out;                   // [frames][t_out_pad][d]
    float* size_out;                 // [frames][t_out_pad]
    // scratch / optional parity outputs (device): node_max [frames][ta], node_idx [frames][ta],
    // unm [frames][ta - r], src [frames][r], dst [frames][r]
    float* node_max;
    int32_t* node_idx;
    int32_t* unm;
    int32_t* src;
    int32_t* dst;
    float* mhat;                     // scratch: the normalised metric as fp32 MFMA operand blocks, tome_mfrag_floats(t, c) per frame
    const KvLayout* kv;              // non-null: metric = mean over heads of these K fragments (aurora.py:639), `metric` unused
    float* metric_out;               // with kv: optional copy of the un-normalised metric [frames][t][c]
    // optional LayerNorm of the merged rows (aurora.py:750), written beside x_out from the merge launch: y = LN(x_out) as
    // norm_kernel<false> computes it (bitwise), all frames * t_out_pad rows.  ln_out == nullptr: none.  Needs d % 8 == 0.
    const float* ln_w;
    const float* ln_b;
    float ln_eps;
    half_t* ln_out;                  // [frames][t_out_pad][d]
};
hipError_t launch_tome_step(const TomeArgs& a, hipStream_t s);
int64_t tome_mfrag_floats(int t, int c);          // floats of TomeArgs.mhat per frame
// metric[f][tok][d] = mean over heads of K (read back from PAIRED K fragments of the ViT "pages")
hipError_t launch_tome_metric(const KvLayout& kv, int frames, int t, int hd, float* metric, hipStream_t s);
// the merge map (aurora_amd/merge_map.py): rows [frames][n] rewritten in place through one step's row table (r clamped, > 0; t <= 8192)
hipError_t launch_tome_map(int32_t* rows, int frames, int n, int t, int r, const int32_t* unm, const int32_t* src, const int32_t* dst,
                           hipStream_t s);
hipError_t launch_tome_map_init(int32_t* map, int frames, int n, hipStream_t s);                     // map[f][p] = 1 + p
// map -= 1; size_out [frames][n_kept] (may be null) = size[f][1 + k] of the padded size vector, ones when size is null
hipError_t launch_tome_map_finish(int32_t* map, int frames, int n, const float* size, int t_pad, int n_kept, float* size_out, hipStream_t s);
hipError_t launch_unmerge_rows(const half_t* tokens, const int32_t* map, int frames, int n, int n_kept, int d, half_t* out, hipStream_t s);

// ---- vit.hip
hipError_t launch_im2col(const half_t* pixels, int frames, int chans, int height, int width, int patch, int kpad, half_t* out,
                         hipStream_t s);
hipError_t launch_vit_assemble(const half_t* patches, const half_t* cls, const half_t* pos, const float* ln_w,
                               const float* ln_b, float eps, int frames, int npatch, int d, int t_pad, half_t* x,
                               hipStream_t s);
hipError_t launch_strip_cls(const half_t* x, int frames, int t, int t_pad, int d, half_t* out, hipStream_t s);
hipError_t launch_pad_rows(const half_t* src, const float* size_src, int frames, int t, int t_pad, int d, half_t* dst,
                           float* size_dst, hipStream_t s);
hipError_t launch_pos_interp(const half_t* pos, int n, int gh, int gw, int d, half_t* out, hipStream_t s);
hipError_t launch_unpad_rows(const half_t* src, const float* size_src, int frames, int t, int t_pad, int d, half_t* dst,
                             float* size_dst, hipStream_t s);
hipError_t launch_gather_rows(const half_t* src, int ld_src, const int32_t* rows, int nrows, int d, half_t* dst,
                              int ld_dst, hipStream_t s);
hipError_t launch_embed_rows(const half_t* table, int d, const int32_t* ids, const int32_t* dst_rows, int n,
                             half_t* dst, int ld_dst, hipStream_t s);      // dst_rows[i] < 0: entry i is skipped
// variable-length prefill: rows [len_i, stride) of every sequence = 0
hipError_t launch_clear_tail_rows(half_t* x, int d, int nseq, int stride, const int32_t* lens, hipStream_t s);
// pruned last layer of a variable-length prefill: the block of `lb` rows that ends at round_up(len_i, 32) of every sequence, strided <-> compact.
// gather: ca[i] = a[i][row0_i ..], cb[i] = b[i][row0_i ..]; scatter (gather == 0): b[i][row0_i ..] = cb[i]
hipError_t launch_tail_rows(half_t* a, half_t* b, half_t* ca, half_t* cb, int d, int nseq, int stride, int lb, const int32_t* lens,
                            int gather, hipStream_t s);

// ---- decode.hip
struct SkinnyArgs {
    const half_t* xf;       // activations in x-fragment form [ceil(B/16)][K/32][64][8], lane = g*16 + (b % 16)
    const half_t* W;        // FRAG-packed [Npad/16][K/32][512]
    int B, Npad, K, n_real;
    int mode;               // SK_ROW, SK_LOGITS, SK_SILU_MUL, SK_QKV
    int b_lo, b_hi;         // only batch columns b_lo <= b < b_hi are stored
    half_t* xres;           // SK_ROW: residual stream in x-fragment form (K32 = n_real/32), updated in place: x += y
    unsigned long long* ssq_out;        // SK_ROW: sum(x_new^2) per row [AUR_SSQ_SLOTS][AUR_MAX_BATCH], 2^-28 fixed point, integer atomics
    const unsigned long long* ssq_in;   // folded RMSNorm: sum(x^2) of the input rows -> acc *= rsqrt(ssq/K + eps); nullptr = none
    unsigned long long* ssq_zero;       // accumulator (all slots) to reset for a later kernel; nullptr = none
    float norm_eps;
    half_t* out_f;          // SK_SILU_MUL: x-fragment form with K32 = out_k32 (input of the down projection)
    int out_k32;
    float* out32;           // SK_LOGITS: [B, n_real] fp32
    // SK_QKV
    int q_cols, k_cols, hd;
    half_t* qbuf;           // [B][heads][kblk][4][8]   (PAIRED-d pieces)
    KvLayout kv;
    const float2* rope;
    const int32_t* pos;     // [B] device: position of the new token (= tokens already cached)
    const int32_t* seq_ids; // [B] page-table rows (nullptr = identity)
    // structure: 0 = x fragments per wave from L2 (engines of <= 32 decode slots), 1 = x through LDS once per workgroup
    // (decode.hip "skinny GEMM, x through LDS").  Chosen per ENGINE (capacity), never per live batch: batch invariance.
    int variant;
    float* part;            // variant 1, SK_ROW: split-K partials [4][Npad/16][ceil(B/16)][64][4] fp32 (nullptr: keep structure 0)
    int* row_cnt;           // variant 1, SK_ROW: arrival counters [Npad/16], zero between launches: the workgroup that completes a tile's 4
                            // partials sums them (fixed order) and runs the residual epilogue IN the projection kernel.  nullptr = a second
                            // launch does it (skinny_row_reduce_kernel; bitwise the same result)
    int gu_ks;              // variant 1, SK_SILU_MUL: k phases per tile, 2 (default) or 1 (engines of > 64 slots: the half grid needs it).
                            // A constant of the ENGINE: it fixes the summation order
    int half_grid;          // variant 1, > 64 rows, SK_QKV / SK_SILU_MUL: 1 = half as many workgroups with twice the tiles each, for
                            // launches into a stream that owns half of the CUs (bitwise the full-grid result)
};
enum { SK_ROW = 0, SK_LOGITS = 1, SK_SILU_MUL = 2, SK_QKV = 3 };
hipError_t launch_skinny(const SkinnyArgs& a, hipStream_t s);
// xf[b0 + row] = RMSNorm(x[row]) (w != nullptr) or x[row], in x-fragment form; x rows are ldx halves apart
hipError_t launch_xfrag_norm(const half_t* x, int64_t ldx, const float* w, float eps, int rows, int d, int b0, half_t* xf,
                             unsigned long long* ssq_out, hipStream_t s, int waves = 16, const int32_t* lens = nullptr, int len_cap = 0);
// lens != nullptr: row i is x[i * ldx + (var_len(lens, i, len_cap) - 1) * d ..] (the last prompt row of sequence i of a variable-length prefill)
hipError_t launch_xfrag_pack(const half_t* x, int64_t ldx, int rows, int d, half_t* xf, hipStream_t s);

struct DecAttnArgs {
    const half_t* qbuf;     // [B][heads][kblk][4][8]
    KvLayout kv;
    const int32_t* pos;     // [B]: keys valid = pos[b] + 1 (the new token's K/V is already written)
    const int32_t* seq_ids;
    int B, heads, hd;
    int nsplit, pages_per_split;
    float scale;
    float* part_o;          // [B][heads][nsplit][hd]
    float* part_ml;         // [B][heads][nsplit][2]
    half_t* out_f;          // [B, heads*hd] in x-fragment form (K32 = out_k32 = heads*hd/32)
    int out_k32;
    int local_splits;       // > 1 (== nsplit, 2 or 4): the splits of a (sequence, head) are the waves of ONE workgroup, joined through LDS (no combine launch)
};
hipError_t launch_decode_attention(const DecAttnArgs& a, hipStream_t s);            // main + combine
hipError_t launch_decode_attention_main(const DecAttnArgs& a, hipStream_t s);
hipError_t launch_decode_attention_combine(const DecAttnArgs& a, hipStream_t s);

// ---- attn_map.hip: the decode step's attention over a prefix window of the keys, mean over heads (and over the layers that launch it)
#define AUR_ATTN_MAP_MAX_HEADS 128
struct AttnMapArgs {
    const half_t* qbuf;     // [B][heads][kblk][4][8]: the roped queries the step's QKV projection wrote
    KvLayout kv;
    const int32_t* pos;     // [B]: keys valid = pos[b] + 1
    int B, heads;
    float scale;
    int window;             // W: keys [0, W) are recorded, a multiple of 64
    float* score;           // scratch [B][heads][W]: scale log2(e) q . k_j
    float* page_ml;         // scratch [B][heads][kv.max_pages][2]: (max, sum of exp2(score - max)) of every 64-token page
    const int32_t *s_len, *s_fin;     // decode step: slot b writes row s_len[b] unless finished / s_len outside [1, max_new); nullptr: every row b writes row 0
    int max_new;            // rows per slot of `out` (1 with s_len == nullptr)
    float* out;             // [B][max_new][W]
    float weight;           // 1 / (heads x selected layers)
    int first;              // 1: the first selected layer stores the row; 0: adds to it
};
hipError_t launch_attn_map(const AttnMapArgs& a, hipStream_t s);

hipError_t launch_argmax_advance(const float* logits, int b0, int nb, int vocab, const half_t* embed, int d, int eos_id,
                                 int max_new, int32_t* out_ids, int32_t* out_len, int32_t* finished, int32_t* pos,
                                 half_t* xf, unsigned long long* ssq, int advance_pos, int set_pos, hipStream_t s,
                                 const int32_t* set_pos_lens = nullptr, int len_cap = 0);      // non-null: pos[b0 + i] = var_len(set_pos_lens, i, len_cap)

// ---- sample.hip: the sampled pick (temperature / top-k / top-p, counter-based draw); per-slot parameters in device memory
struct aur_sampling;
hipError_t sample_init();
// stage: 1 = the row is staged in LDS when it fits, 0 = re-read from global memory on every pass (same token either way)
hipError_t launch_sample_advance(const float* logits, int b0, int nb, int vocab, const aur_sampling* params, const half_t* embed, int d,
                                 int eos_id, int max_new, int32_t* out_ids, int32_t* out_len, int32_t* finished, int32_t* pos, half_t* xf,
                                 unsigned long long* ssq, int advance_pos, int set_pos, hipStream_t s, const int32_t* set_pos_lens,
                                 int len_cap, int stage);
hipError_t launch_sample_rows(const float* logits, int rows, int vocab, const aur_sampling* params, const int32_t* n_dev,
                              int32_t* tokens_out, int32_t* kept_out, hipStream_t s, int stage);

// ---- logit_rules.hip: repetition penalty / no-repeat n-gram / min-new-tokens on the logits rows of slots [b0, b0 + nb) ahead of the
// pick, and the originals back behind it.  ids [.., ids_stride] / lens: the slots' generated tokens; save: logit_rules_save_bytes(slots,
// ids_stride) bytes (ids_stride + 1 entries per slot), save_cnt int32 [slots]
struct aur_logit_rules;
int64_t logit_rules_save_bytes(int rows, int ids_stride);
hipError_t launch_logit_rules_apply(float* logits, int b0, int nb, int vocab, const aur_logit_rules* rules, const int32_t* ids, int ids_stride,
                                    const int32_t* lens, int eos_id, void* save, int32_t* save_cnt, hipStream_t s);
hipError_t launch_logit_rules_restore(float* logits, int b0, int nb, int vocab, int ids_stride, const void* save, const int32_t* save_cnt,
                                      hipStream_t s);

// ---- stop.hip: stop ids / stop strings / per-request budget behind the pick, on slots [b0, b0 + nb): sets finished[b] of an unfinished
// slot whose newest token stops it, nothing else.  ids [.., ids_stride] / lens: the slots' generated tokens; offsets int32 [vocab + 1] /
// bytes uint8 [nbytes]: the bytes every token decodes to (nullptr: no string matches)
struct aur_stop_rules;
hipError_t launch_stop_check(int b0, int nb, const aur_stop_rules* rules, const int32_t* ids, int ids_stride, const int32_t* lens,
                             int batch_max_new, int32_t* finished, const int32_t* offsets, const uint8_t* bytes, int vocab, int64_t nbytes,
                             hipStream_t s);

// ---- guidance.hip: classifier-free guidance around the pick of slots [b0, b0 + nb).  recs [max_batch]: a leader's record names its
// partner (clamped into [0, max_batch)); save fp32 [max_batch][vocab]: the leaders' model rows between apply and restore.  follow: the
// partner takes the leader's newest token, out_len, finished and next input.  clear: records [s0, s0 + n) and their leaders' -> neutral
struct aur_guidance;
hipError_t launch_guidance_apply(float* logits, int b0, int nb, int vocab, int max_batch, const aur_guidance* recs, float* save, hipStream_t s);
hipError_t launch_guidance_restore(float* logits, int b0, int nb, int vocab, const aur_guidance* recs, const float* save, hipStream_t s);
hipError_t launch_guidance_follow(int b0, int nb, int vocab, int max_batch, const aur_guidance* recs, const half_t* embed, int d, int max_new,
                                  int32_t* out_ids, int32_t* out_len, int32_t* finished, half_t* xf, unsigned long long* ssq, hipStream_t s);
hipError_t launch_guidance_clear(aur_guidance* recs, int max_batch, int s0, int n, hipStream_t s);

// ---- score.hip: log-probability of a target token under a logits row (+ the row's first argmax), and the row-list gather that feeds
// any rows of a prefill pass to the pick path's lm_head (aur_llm_score_var)
hipError_t launch_score_rows(const float* logits, int rows, int vocab, const int32_t* targets, float* logprob_out, int32_t* argmax_out,
                             hipStream_t s);
// log-probabilities of generated tokens (top_n <= 8 alternatives each).  launch_token_logprob runs BEHIND the pick over slots
// [b0, b0 + nb): a slot whose out_len differs from lp_len gets the record of its newest token at index out_len - 1 of lp [.., max_new],
// top_id / top_lp [.., max_new, top_n], and lp_len = out_len.  _rows: the same evaluation on caller rows, one token per row.  _clear:
// slots [b0, b0 + nb) hold no record (lp_len 0, lp 0, ranks (-1, 0.0)).
hipError_t launch_token_logprob(const float* logits, int b0, int nb, int vocab, const int32_t* out_ids, const int32_t* out_len, int max_new,
                                int top_n, int32_t* lp_len, float* lp, int32_t* top_id, float* top_lp, hipStream_t s);
hipError_t launch_token_logprob_rows(const float* logits, int rows, int vocab, const int32_t* tokens, int top_n, float* lp, int32_t* top_id,
                                     float* top_lp, hipStream_t s);
hipError_t launch_token_logprob_clear(int b0, int nb, int max_new, int top_n, int32_t* lp_len, float* lp, int32_t* top_id, float* top_lp,
                                      hipStream_t s);
// column b < n of xf = flat row rows[b] of x (sequence rows[b] / stride, row rows[b] % stride) + its sum(x^2); entries that are negative,
// outside nseq * stride or at / beyond their sequence's clamped length - and columns [n, ncols) - are zero rows; eff_targets[b] =
// targets[b] for a live entry, -1 otherwise
hipError_t launch_score_gather(const half_t* x, int d, const int32_t* rows, const int32_t* targets, int n, int ncols, int nseq, int stride,
                               const int32_t* lens, half_t* xf, unsigned long long* ssq_out, int32_t* eff_targets, hipStream_t s);
