/* aurora_hip.h - C ABI of the MI355X-native AuroraCap inference hot path (libaurora_hip.so).
 *
 * The reference (rese1f/aurora @ 2025-06-14) is 100 % Python and has NO FFI: this ABI is the seam a
 * maintainer binds with ctypes to replace the eager-PyTorch calls listed per entry
 * point.  Conventions:
 *   - extern "C", plain C types, every call returns int status: 0 = ok, negative = error code;
 *     no C++ exception crosses the boundary; aur_last_error(ctx) returns the message.
 *   - The CALLER owns every buffer (weights, workspace, KV pool, inputs, outputs) and the stream.
 *     The library owns only its ctx; hot calls never allocate device memory.
 *   - All device pointers are raw HIP device pointers (torch: tensor.data_ptr()); `stream` is a
 *     hipStream_t passed as void* (torch: torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it, nothing synchronises unless documented.
 *   - One ctx per device / process; calls on one ctx are not re-entrant.
 *   - Compute dtype: fp16 storage, fp32 accumulation (the reference runs torch.float16, inference.py:50,54).
 */
#ifndef AURORA_HIP_H
#define AURORA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUR_OK 0
#define AUR_ERR_ARG -1      /* invalid argument / shape (cf. ValueError at aurora.py:649-652) */
#define AUR_ERR_STATE -2    /* missing weight / workspace / call order */
#define AUR_ERR_HIP -3      /* HIP runtime error */
#define AUR_ERR_UNSUPPORTED -4 /* e.g. num_beams > 1 (cf. NotImplementedError at aurora.py:269-270) */

#define AUR_ACT_QUICK_GELU 1    /* x * sigmoid(1.702 x) */
#define AUR_ACT_GELU 2          /* exact erf GELU (ACT2FN["gelu"]) */
#define AUR_ACT_SILU 4          /* x * sigmoid(x) (ACT2FN["silu"] / ["swish"]) */
#define AUR_ACT_RELU 5
#define AUR_ACT_GELU_TANH 6     /* 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) (ACT2FN["gelu_new"] / ["gelu_pytorch_tanh"]) */

typedef struct aur_ctx aur_ctx;

/* Model + capacity description.  Values come from the checkpoint's config.json files at load time
 * (never hard-coded). */
typedef struct aur_config {
    /* vision tower: AuroraEncoder / HF CLIPVisionConfig (aurora.py:869-904) */
    int32_t vit_hidden, vit_heads, vit_layers, vit_mlp, vit_patch, vit_image, vit_channels;
    int32_t vit_act;            /* AUR_ACT_* from config.hidden_act */
    float vit_ln_eps;           /* config.layer_norm_eps (pre_layrnorm); encoder layers use 1e-5 (aurora.py:709) */
    /* projector (modeling_projector.py:20-33, configuration_projector.py:9-22): Linear(vit_hidden, llm_hidden), then (act, Linear(llm_hidden,
     * llm_hidden)) x (depth - 1); depth / hidden_act come from projector/config.json through proj_depth / proj_act at the end of this struct */
    /* language model: HF LlamaConfig */
    int32_t llm_hidden, llm_heads, llm_layers, llm_mlp, llm_vocab;
    float llm_rms_eps, rope_theta, rope_factor;   /* linear RoPE scaling factor (vicuna-16k: 4.0) */
    /* capacity */
    int32_t max_frames;         /* frames per aur_vit_encode call */
    int32_t max_batch;          /* decode slots (batch rows of the decode step), <= 128 */
    int32_t max_ctx;            /* tokens per sequence (prompt + generated) */
    int32_t max_new_tokens;     /* output buffer width per slot */
    int32_t page_tokens;        /* KV page size in tokens: must be 64 (the decode attention's page pipeline is written for 64-token pages;
                                 * aur_create rejects anything else - kept as a field so the KV layout stays self-describing) */
    int32_t use_graph;          /* 1: capture the decode step into a hipGraph */
    int32_t num_banks;          /* 1 or 2 generation banks (2: KV pool and per-batch state doubled, see aur_select_bank) */
    int32_t vit_native_image;   /* side of the square input the checkpoint's position table was trained for (config.image_size);
                                 * 0 = vit_image.  vit_image is then the CAPACITY: the largest input side aur_vit_encode_hw accepts */
    int32_t spare_slots;        /* extra KV sequences per bank beyond max_batch (ids max_batch .. max_batch + spare_slots - 1): targets of
                                 * aur_llm_prefill_stage while every decode slot is still generating.  0 = none */
    int32_t proj_depth;         /* ProjectorConfig.depth: number of Linear layers, 1 .. 8; 0 = 2 (the AuroraCap checkpoints) */
    int32_t proj_act;           /* AUR_ACT_* of ProjectorConfig.hidden_act between the Linear layers; 0 = AUR_ACT_GELU */
} aur_config;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int aur_create(const aur_config* cfg, aur_ctx** out);
void aur_destroy(aur_ctx* ctx);
const char* aur_last_error(const aur_ctx* ctx);   /* ctx may be NULL: returns the last create() error */
const char* aur_version(void);

/* Named device tensors (weights in kernel layout).  Replaces the three from_pretrained loads at
 * inference.py:46-57.  Names and layouts: aurora_amd/engine.py::_load_vit / _load_llm / _load_projector
 * (e.g. "vit.3.qkv.w", "llm.7.down.w", "proj.0.w" / "proj.0.b" .. "proj.<depth-1>.b"; a bias-free projector passes zeros). */
int aur_set_tensor(aur_ctx* ctx, const char* name, const void* dev_ptr, int64_t nbytes);
/* Caller-owned scratch; sizes from the two queries (depend only on cfg). */
int64_t aur_workspace_bytes(const aur_ctx* ctx);
int64_t aur_kv_pool_bytes(const aur_ctx* ctx);
int aur_set_workspace(aur_ctx* ctx, void* dev_ptr, int64_t nbytes);
int aur_set_kv_pool(aur_ctx* ctx, void* dev_ptr, int64_t nbytes);
/* Checks that every tensor the config needs was provided; builds the RoPE table and the static page table. */
int aur_finalize(aur_ctx* ctx, void* stream);

/* Weight re-layout helper (device -> device): row-major fp16 W[n_src, k_src] (leading dim ld_src) ->
 * MFMA fragment tiles [npad/16][kpad/32][64][8].  row_map (device int32[npad] or NULL) selects the source row
 * of each packed row (-1 = zero row): QKV concatenation, head padding, RoPE pairing, gate/up interleave. */
int aur_pack_linear(aur_ctx* ctx, const void* w, int32_t n_src, int32_t k_src, int32_t ld_src,
                    const int32_t* row_map, int32_t npad, int32_t kpad, void* out, void* stream);

/* ---- the token schedule (aurora.py:895, tome.py:45) -------------------------------------------- */
/* r = int(W*H / patch^2 * (1 - ratio) / layers) evaluated in doubles in exactly that order. */
int32_t aur_tome_r(int32_t height, int32_t width, int32_t patch, double token_kept_ratio, int32_t layers);
/* tokens per frame entering layer `layer` (0..layers), t0 = tokens at layer 0 incl. CLS. */
int32_t aur_tokens_at_layer(int32_t t0, int32_t r, int32_t layer);

/* ---- hot path ---------------------------------------------------------------------------------- */
/* ViT + per-layer ToMe: replaces visual_encoder(pixel_values, output_hidden_states=True)
 * .hidden_states[-2][:, 1:]  (aurora.py:249-253; AuroraEncoder.forward aurora.py:883-904).
 * pixels: fp16 [frames, channels, image, image] (already normalised, inference.py:71-75).
 * out_tokens: fp16 [frames * n_kept, vit_hidden].  *n_kept_out (host) = kept tokens per frame. */
int aur_vit_encode(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t r, void* out_tokens,
                   int32_t* n_kept_out, void* stream);
/* Same for inputs that are not vit_image x vit_image (AuroraEncoder.interpolate_pos_encoding,
 * aurora.py:909-951): pixels fp16 [frames, channels, height, width]; the patch grid is (height / patch) x (width / patch)
 * and must fit the ctx ((h/p)*(w/p) + 1 <= (vit_image/patch)^2 + 1; make vit_image larger than vit_native_image to admit bigger inputs).  pos_emb: fp16 [1 + (h/p)*(w/p), vit_hidden], the
 * position table of this grid (aur_vit_pos_interp; the engine caches one per input size); NULL is allowed only
 * for the native grid.  r is computed by the caller from height and width (aur_tome_r). */
/* AuroraEncoder.interpolate_pos_encoding (aurora.py:909-951) for an input of height x width pixels: the n x n patch rows of the
 * checkpoint's table ("vit.pos") resampled bicubically to (height / patch) x (width / patch) with the reference's scale factors
 * (g + 0.1) / n - ATen's upsample_bicubic2d arithmetic (align_corners = False, A = -0.75), fp32 on the stored fp16 table - class row kept.
 * pos_out: fp16 [1 + (height / patch) * (width / patch), vit_hidden], the table aur_vit_encode_hw takes.  Valid for the native grid
 * too (it then reproduces the table up to the resampling's rounding; callers pass NULL to aur_vit_encode_hw instead). */
int aur_vit_pos_interp(aur_ctx* ctx, int32_t height, int32_t width, void* pos_out, void* stream);

int aur_vit_encode_hw(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t height, int32_t width,
                      const void* pos_emb, int32_t r, void* out_tokens, int32_t* n_kept_out, void* stream);
/* aur_vit_encode_hw with the merge map (aurora_amd/merge_map.py; the reference's merge_source, tome.py:222-232, carried through every
 * layer): which kept token every patch was merged into.  Two more outputs in device memory:
 *   map_out  int32 [frames, (height / patch) * (width / patch)], patches row-major: map_out[f][p] in [0, n_kept) is the row of
 *            out_tokens' frame f that patch p ended in;
 *   size_out fp32 [frames, n_kept] or NULL: patches per kept token - the size vector of merge_wavg (tome.py:207-219) without its class
 *            entry; bincount(map_out[f]) == size_out[f], exactly.
 * The map is built in map_out itself - set to 1 + p, rewritten through the layer's row table by one launch of its own behind the ToMe
 * step of every merging layer (on the same stream, before the next layer reuses the step's index buffers), the class row taken off at
 * the end - so aur_workspace_bytes does not grow, nothing is allocated, and the call is enqueue-only and recordable with
 * aur_graph_begin like aur_vit_encode_hw.  r = 0, or a schedule that never merges: the identity and ones.  out_tokens are bitwise those of
 * aur_vit_encode_hw, which IS this call with map_out = size_out = NULL and launches exactly the kernels it launched before. */
int aur_vit_encode_map(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t height, int32_t width,
                       const void* pos_emb, int32_t r, void* out_tokens, int32_t* map_out, float* size_out,
                       int32_t* n_kept_out, void* stream);

/* projector + prefix splice: replaces self.projector(...) (aurora.py:254-256) and
 * prepare_inputs_labels_for_multimodal (model/utils.py:138-295) for one sequence.
 * vis: fp16 [nvis, vit_hidden]; vis_rows / text_rows: device int32 destination rows in `embeds`
 * (row order of the spliced sequence, computed on the host from input_ids); text_ids: device int32.
 * embeds: fp16 [rows_pad, llm_hidden] with rows_pad = round_up(seq_len, 32) (pad rows zeroed here).
 * STREAM RULE: the projector's intermediates live in the ctx's front-end scratch (the prefill layers' normalised-input and MLP
 * buffers: a projector of depth >= 3 ping-pongs through both), so a splice must be ordered against every aur_llm_prefill* /
 * aur_llm_prefill_stage call of the same ctx - enqueue them on ONE stream (as aurora_amd.engine does) or order the streams
 * with events; a splice on another stream beside a running prefill corrupts that prefill silently. */
int aur_project_splice(aur_ctx* ctx, const void* vis, int32_t nvis, const int32_t* vis_rows,
                       const int32_t* text_ids, const int32_t* text_rows, int32_t ntext,
                       int32_t seq_len, void* embeds, void* stream);
/* The same for one sequence of a variable-length prefill: text_ids / text_rows hold ntext_cap entries of which those with
 * text_rows[j] < 0 are unused and skipped (a prompt shorter than the capacity pads with -1), so the call needs no length and a captured
 * graph serves every prompt that fits the capacity.  embeds: the sequence's `stride` rows (stride as in aur_llm_prefill_batch_var);
 * rows that no entry names are left as they are - the variable-length prefill clears [len, stride) itself.  Same STREAM RULE. */
int aur_project_splice_var(aur_ctx* ctx, const void* vis, int32_t nvis, const int32_t* vis_rows,
                           const int32_t* text_ids, const int32_t* text_rows, int32_t ntext_cap,
                           int32_t stride, void* embeds, void* stream);

/* Greedy generation state: replaces llm.generate(inputs_embeds=..., do_sample=False, max_new_tokens=N)
 * (inference.py:89-96).  eos_id < 0 disables the EOS stop (benchmark: fixed-length outputs). */
int aur_begin_batch(aur_ctx* ctx, int32_t batch, int32_t max_new_tokens, int32_t eos_id, void* stream);
/* Generation banks (num_banks = 2): each bank has its own max_batch KV slots, residual stream, outputs and captured
 * graph.  All generation calls (begin_batch / prefill / decode / get_outputs / ...) act on the selected bank, so batch
 * i can decode on one stream while batch i+1 is prefetched into the other bank on a second stream (decode is HBM-bound,
 * ViT + prefill are MFMA-bound).  The caller orders the streams with its own events.  The current bank is part of what a
 * caller-captured graph freezes (aur_graph_begin): AUR_ERR_STATE inside a capture. */
int aur_select_bank(aur_ctx* ctx, int32_t bank);
/* Prefill `slot` with embeds [round_up(seq_len,32), llm_hidden] (clobbered), write its KV pages, produce the
 * first token (argmax of the last position's logits). */
int aur_llm_prefill(aur_ctx* ctx, int32_t slot, void* embeds, int32_t seq_len, void* stream);
/* Same for `nseq` sequences of EQUAL length in slots [slot0, slot0 + nseq): embeds is
 * [nseq * round_up(seq_len,32), llm_hidden]; one pass of M = nseq * round_up(seq_len,32) rows through every GEMM. */
int aur_llm_prefill_batch(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t seq_len, void* stream);
/* The same prefill in two halves, for a front end that runs on its OWN stream (e.g. a CU-masked one) next to the decode
 * stream while all slots are still generating (the reference harness has no such overlap: it runs one clip at a time,
 * lmms_eval/models/auroracap.py:344-525):
 *   stage : the layer stack only - writes the KV pages of KV sequences [seq0, seq0 + nseq) (any ids below
 *           max_batch + spare_slots; normally the spare ones) and leaves the final hidden states in `embeds`.  Touches no
 *           decode state, so it may run concurrently with aur_llm_decode on another stream.
 *   commit: on the DECODE stream, between two aur_llm_decode calls and after `stage` has completed (caller's event):
 *           exchanges the page-table rows of slots [slot0 ..) with those of sequences [seq0 ..) - the slots now own the
 *           freshly written pages, the spare sequences own the pages the slots used before -, resets the slots, and
 *           produces their first tokens from the last prompt rows of `embeds`.  seq0 == slot0: no exchange. */
int aur_llm_prefill_stage(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t seq_len, void* stream);
int aur_llm_prefill_commit(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t seq_len, void* stream);
/* Variable-length forms of the three calls above: prompts of DIFFERENT lengths in one pass, the lengths in device memory.
 * embeds is fp16 [nseq * stride, llm_hidden], stride a multiple of 32 and at most the positions of a sequence's KV pages
 * (ceil(max_ctx / page_tokens) * page_tokens); sequence i occupies rows [i * stride, i * stride + len_i), len_i = seq_lens_dev[i]:
 * int32 in DEVICE memory, caller-owned, read by the kernels when the work runs - it must stay valid (and unchanged) until then.  The
 * host never reads the lengths: no synchronisation, no allocation, the calls are enqueue-only and may be recorded with aur_graph_begin.
 * A capture freezes stride, nseq, the slot / sequence ids and the pointers - NOT the lengths: refill the lengths buffer (and embeds)
 * before each replay.  Because the host cannot check them, every kernel clamps len_i into [1, stride]; that len_i + max_new_tokens <=
 * max_ctx is the CALLER'S promise (aurora_amd.engine checks it where the lengths are known).
 * Rows [len_i, stride) of embeds are don't-care on input - stale states of an earlier, longer prompt, Inf / NaN patterns -: the prefill
 * clears them itself before the first layer, they stay zero in every layer, and the K / V written for positions [len_i, stride) are
 * zeros until decode steps overwrite them.  For sequence i the first token, the logits row, every K / V value at positions < len_i and
 * the decode position are BITWISE those of aur_llm_prefill(slot, embeds_i, len_i).  aur_llm_prefill_commit_var reads only row
 * len_i - 1 of each sequence and takes the same (stride, seq_lens_dev) its stage was given. */
int aur_llm_prefill_batch_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t stride, const int32_t* seq_lens_dev, void* stream);
int aur_llm_prefill_stage_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t stride, const int32_t* seq_lens_dev, void* stream);
int aur_llm_prefill_commit_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t stride, const int32_t* seq_lens_dev, void* stream);
/* Shared prefixes: several prompts about one clip agree on every row up to and including the last visual token, so
 * a sibling request takes those positions from the first request's KV sequence and prefills only the rows that differ.
 *
 * aur_kv_copy_prefix copies the K and V of positions [0, tokens) of KV sequence src_seq into sequences [dst_seq0, dst_seq0 + ndst) of
 * the selected bank, for every layer (kv_copy_prefix_kernel: each 16-byte piece of a source page is loaded once and stored ndst times).
 * The page ids are read from the page table ON THE DEVICE when the work runs: the call is enqueue-only, recordable with aur_graph_begin,
 * and correct behind earlier aur_llm_prefill_commit row exchanges queued on the same stream.  tokens: a positive multiple of page_tokens
 * (64), at most the positions of a sequence's pages; every id below max_batch + spare_slots; src_seq outside the destination range;
 * anything else returns AUR_ERR_ARG and leaves the ctx usable.  Pages are COPIED, not shared: the static page table, the commit's row
 * exchange and every decode kernel stay as they are - no reference counts, no copy-on-write.  The source may be a live, decoding slot
 * (its pages below `tokens` are only read by its own decode steps).
 *
 * aur_llm_extend_*_var: the _prefill_*_var calls for sequences that already hold valid K / V for positions [0, pos0).  embeds is fp16
 * [nseq * stride, llm_hidden]; its rows [i * stride, i * stride + len_i) are the input embeddings of positions [pos0, pos0 + len_i),
 * len_i = new_lens_dev[i] (int32, device memory, clamped into [1, stride] by every kernel).  pos0: a positive multiple of page_tokens;
 * stride: a multiple of 32; pos0 + stride at most the positions of a sequence's pages - anything else AUR_ERR_ARG.  pos0 + len_i +
 * max_new_tokens <= max_ctx is the CALLER'S promise (aurora_amd.engine checks it where the lengths are known).  Inside it is the layer
 * stack of the prefill over the new rows alone: RoPE and the page write at pos0 + row, queries at pos0 + row over keys [0, pos0 + len_i),
 * padding rows cleared and kept zero, the pruned last layer (when the stride is long enough to prune) with its row0 relative to the new
 * rows, the first token from row len_i - 1 - greedy, or sampled with the slot's record at token index 0 -, decode position pos0 + len_i.
 * CONTRACT: for sequence i the first token, the logits row, every K / V value at positions [pos0, pos0 + len_i) and the decode position
 * are BITWISE those of aur_llm_prefill(slot, full_embeds_i, pos0 + len_i), provided positions [0, pos0) hold what that prefill writes (a
 * GEMM element's k order does not depend on M; attention is row-independent and walks the key blocks in order).  Recordable like their
 * _prefill_ counterparts; a capture freezes pos0, stride, nseq, the ids and the pointers, not the lengths. */
int aur_kv_copy_prefix(aur_ctx* ctx, int32_t src_seq, int32_t dst_seq0, int32_t ndst, int32_t tokens, void* stream);
int aur_llm_extend_batch_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride, const int32_t* new_lens_dev, void* stream);
int aur_llm_extend_stage_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride, const int32_t* new_lens_dev, void* stream);
int aur_llm_extend_commit_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t pos0, int32_t stride, const int32_t* new_lens_dev, void* stream);
/* Sampled generation: with option "sampling" = 1 (aur_set_option) the token pick of every prefill / commit /
 * decode step draws from the slot's temperature / top-k / top-p distribution instead of taking the first maximum.  The draw for
 * (seed, stream, token index) is word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (token index, stream, 0, 0): a pure
 * function of those and of the logits row, whatever the batch, slot, bank or launch form.  temperature == 0 on a slot = greedy. */
typedef struct aur_sampling { float temperature, top_p; int32_t top_k; uint32_t stream; uint64_t seed; } aur_sampling;
/* per-slot parameters of the selected bank, copied device-to-device from caller-owned DEVICE memory when the work runs (like
 * seq_lens_dev): enqueue-only, recordable with aur_graph_begin; a capture freezes the pointer, not the values.  They hold until
 * overwritten; aur_begin_batch sets every slot to greedy (temperature 0).  Must be ordered before the prefill / commit that
 * produces the slot's first token.  temperature < 0 (-> 0), top_p outside (0, 1] (<= 0: the maximum alone; > 1: off), top_k < 0
 * (-> off) are clamped by the kernel (the host cannot see them); the Python layer validates where the values are known. */
int aur_slot_sampling(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_sampling* params_dev, void* stream);
/* Logit rules ahead of the pick: with option "logit_rules" = 1 (aur_set_option) every prefill / commit / decode
 * step rewrites the slot's fp32 logits row before the token is picked - greedy or sampled - and puts the model's values back behind the
 * pick, so aur_copy_logits and the log-probability records keep seeing the unmodified row.  The rules are transformers'
 * RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor over the history h = the n tokens
 * the slot has GENERATED so far (not the prompt: generate(inputs_embeds=...) starts input_ids empty):
 *   repetition_penalty p (1 = off; <= 0 or NaN -> 1): every distinct token t of h, once: l[t] = l[t] < 0 ? l[t] * p : l[t] / p in fp32,
 *     the divide correctly rounded;
 *   no_repeat_ngram g (0 = off; < 0 -> 0): if n + 1 >= g, l[h[i + g - 1]] = -inf for every i in [0, n - g + 1) with
 *     h[i .. i + g - 1) == h[n - g + 1 .. n); g = 1 bans every generated token;
 *   min_new_tokens m (0 = off; < 0 -> 0): while n < m, l[eos] = -inf; nothing when the batch has no EOS (eos_id < 0).
 * A ban wins over a penalty on the same index; the result does not depend on the order of the rules.  aurora_amd/logit_rules.py is
 * the definition in numpy.  reserved: 0. */
typedef struct aur_logit_rules { float repetition_penalty; int32_t no_repeat_ngram; int32_t min_new_tokens; int32_t reserved; } aur_logit_rules;
/* per-slot records of the selected bank: aur_slot_sampling's contract - device-to-device from caller-owned DEVICE memory, enqueue-only,
 * recordable; a capture freezes the pointer, not the values; ordered before the prefill / commit that picks the slot's first token.
 * aur_begin_batch and aur_slot_reset set the slots they clear to neutral (the all-zero record: a penalty <= 0 counts as 1, like
 * (1, 0, 0)): such a slot's row is never touched.  A commit keeps a slot's record. */
int aur_slot_logit_rules(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_logit_rules* rules_dev, void* stream);
/* Classifier-free guidance: with option "guidance" = 1 (aur_set_option) a guided request is a PAIR of slots that
 * decode in lock-step.  The leader's record names its partner, whose sequence is the negative prompt; the partner's own record stays
 * neutral.  Ahead of every prefill's / commit's / decode step's pick - and ahead of the logit rules - the leader's fp32 row c becomes
 *   out_i = scale * (lc_i - lu_i) + lu_i,  lc = log_softmax(c), lu = log_softmax(u), u = the partner's row
 * (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor; aurora_amd/guidance.py is the definition in numpy), and behind the
 * pick the model's row is back, so aur_copy_logits and the log-probability records keep seeing the unmodified conditional row.  Behind
 * the stop check the partner takes the leader's newest token, out_len, finished flag and next input: both sequences hold the same
 * generated ids and stop together.  A first pick needs the partner's row: prefill the partner before its leader.
 * scale: finite, positive and not 1 asks for guidance; anything else - the all-zero record among them - is neutral: the slot is not
 * touched.  partner: a slot of the bank, clamped into [0, max_batch) by the kernels. */
typedef struct aur_guidance { float scale; int32_t partner; } aur_guidance;
/* per-slot records of the selected bank: aur_slot_sampling's contract - device-to-device from caller-owned DEVICE memory, enqueue-only,
 * recordable; a capture freezes the pointer, not the values; ordered before the prefill / commit that picks the slot's first token.
 * aur_begin_batch and aur_slot_reset set the slots they clear to neutral, and a leader whose partner they clear as well; a commit keeps
 * a slot's record.  The records and the save buffer (max_batch * llm_vocab * 4 bytes per bank) live in memory the first "guidance" 1
 * allocates (aur_workspace_bytes does not grow): AUR_ERR_STATE before that. */
int aur_slot_guidance(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_guidance* recs_dev, void* stream);
/* Stop conditions behind the pick: with option "stop_rules" = 1 (aur_set_option) stop_check_kernel runs behind
 * every prefill's / commit's / decode step's pick, greedy or sampled, eager or captured, and sets finished[b] of an unfinished slot whose
 * newest token t = h[n - 1] (h = the n tokens the slot has GENERATED, never the prompt) fulfils one of
 *   stop_token: t is one of token_ids[0 .. n_token_ids);
 *   stop_string: in the concatenation of the bytes the tokens of h decode to (the table of aur_stop_vocab), an occurrence of one of
 *     strings[i][0 .. string_len[i]) ends inside t's bytes or at their end (it may begin in earlier tokens, t may go on behind it); a
 *     token of zero bytes completes nothing, an id outside the table has no bytes and breaks the text;
 *   length: n >= max_new_tokens (<= 0: the batch's limit alone, which advance_tail enforces in the engine).
 * Nothing else is written: t stays in the output, and pos, the next-token embedding and out_len are what an EOS leaves, so a stopped slot
 * behaves in later steps exactly like one that saw the EOS.  The kernel clamps n_token_ids / n_strings into [0, 8] and string_len into
 * [0, 64] (a string of length 0 matches nothing); the all-zero record is neutral.  aurora_amd/stopping.py is the definition. */
#define AUR_STOP_MAX_IDS 8
#define AUR_STOP_MAX_STRINGS 8
#define AUR_STOP_MAX_STRING_BYTES 64
#define AUR_STOP_MAX_TOKEN_BYTES 255
typedef struct aur_stop_rules {
    int32_t max_new_tokens, n_token_ids, n_strings, reserved;
    int32_t token_ids[AUR_STOP_MAX_IDS];
    int32_t string_len[AUR_STOP_MAX_STRINGS];
    uint8_t strings[AUR_STOP_MAX_STRINGS][AUR_STOP_MAX_STRING_BYTES];
} aur_stop_rules;
/* The bytes each vocabulary entry decodes to: offsets_dev int32 [vocab + 1] (entry t is bytes_dev[offsets[t] .. offsets[t + 1])), bytes_dev
 * uint8 [nbytes]; caller-owned DEVICE memory that must outlive its use, handed over once (NULL, NULL, 0, 0 takes it back: string stops then
 * match nothing).  The kernel never reads outside [0, vocab] / [0, nbytes) whatever the offsets hold, and a token counts at most 255 bytes.
 * The pointers are frozen inside captured graphs: the decode graphs are dropped; AUR_ERR_STATE inside a capture. */
int aur_stop_vocab(aur_ctx* ctx, const int32_t* offsets_dev, const uint8_t* bytes_dev, int32_t vocab, int64_t nbytes);
/* per-slot records of the selected bank: aur_slot_sampling's contract - device-to-device from caller-owned DEVICE memory, enqueue-only,
 * recordable; a capture freezes the pointer, not the values; ordered before the prefill / commit that picks the slot's first token.
 * aur_begin_batch and aur_slot_reset set the slots they clear to neutral; a commit keeps a slot's record.  The records live in memory the
 * first "stop_rules" 1 allocates (aur_workspace_bytes does not grow): AUR_ERR_STATE before that. */
int aur_slot_stop(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_stop_rules* rules_dev, void* stream);
/* Run `steps` decode steps for slots [0, batch): one new token per unfinished slot per step. */
int aur_llm_decode(aur_ctx* ctx, int32_t steps, void* stream);
/* Synchronises the stream and copies results to host: ids [batch * max_new_tokens], lens [batch]. */
int aur_get_outputs(aur_ctx* ctx, int32_t* ids_host, int32_t* lens_host, void* stream);
/* Synchronises; number of slots still generating (EOS not seen, length < max_new_tokens). */
int aur_unfinished(aur_ctx* ctx, int32_t* count_host, void* stream);
/* Continuous batching: the slots of the active batch are independent sequences.  A slot is
 * finished after EOS or max_new_tokens; a finished slot stops advancing (it never leaves its KV pages however many more
 * steps the batch decodes).  aur_slot_reset makes a slot empty and active again - follow it with aur_llm_prefill into
 * that slot while the other slots keep their state; aur_slot_retire parks a slot (finished, nothing to collect);
 * aur_slot_state copies the per-slot generated lengths / finished flags to the host (synchronises the stream). */
int aur_slot_reset(aur_ctx* ctx, int32_t slot, void* stream);
int aur_slot_retire(aur_ctx* ctx, int32_t slot, void* stream);
int aur_slot_state(aur_ctx* ctx, int32_t* lens_host, int32_t* finished_host, void* stream);
/* Asynchronous (no host synchronisation) device-to-device copy of the results of slots [slot0, slot0 + nslots): ids_dev int32
 * [nslots, max_new_tokens], lens_dev int32 [nslots] - lets a serving loop collect finished captions and re-fill their slots
 * without ever draining the stream (bench.py's steady-state latency point). */
int aur_slot_collect(aur_ctx* ctx, int32_t slot0, int32_t nslots, int32_t* ids_dev, int32_t* lens_dev, void* stream);

/* ---- captured front ends (the reference tree's serving engine captures one graph per shape bucket and copies the inputs into the
 * graph's static buffers before every replay: src/sglang/python/sglang/srt/model_executor/cuda_graph_runner.py:163-279) ------------
 * aur_graph_begin opens a hipGraph capture on `stream` (thread-local mode); every enqueue-only call of this ctx that follows on that
 * stream from the same thread - aur_vit_encode(_hw), aur_project_splice(_var), aur_llm_prefill / _batch / _stage / _commit (and their _var forms),
 * aur_kv_copy_prefix, aur_llm_extend_*_var, aur_llm_score_var, aur_slot_reset /
 * _retire / _collect, the kernel-level entry points - is recorded instead of run; aur_graph_end instantiates the recording and returns
 * a handle (>= 1) that aur_graph_launch replays with one call.  Pointers, shapes, KV sequence ids, the ctx's gemm_* knobs and the
 * current bank (whose page table the prefill writes through) are frozen at capture time: a serving loop keeps one graph per (bank,
 * frames, input size, r, prompt structure, target sequences) bucket and copies each clip's pixels / ids into the bucket's staging
 * buffers before the replay (aurora_amd/engine.py FrontEndGraph).  Calls that synchronise or re-capture (aur_get_outputs,
 * aur_unfinished, aur_slot_state, aur_microbench, aur_decode_stamps_read, aur_begin_batch, aur_set_option, aur_logprob_enable,
 * aur_get_logprobs, aur_finalize,
 * aur_profile_enable), aur_select_bank (it would split the capture between two banks) and aur_llm_decode (it replays its own graph)
 * return AUR_ERR_STATE inside a capture without touching the runtime: the capture stays valid, and aur_graph_end - which must be called
 * in any case - closes it.  A synchronising HIP call of the CALLER's own inside the capture invalidates it: aur_graph_end then returns
 * AUR_ERR_HIP.  One capture at a time per ctx.  aur_graph_destroy: the caller guarantees no replay is still queued. */
int aur_graph_begin(aur_ctx* ctx, void* stream);
int aur_graph_end(aur_ctx* ctx, void* stream, int32_t* graph_out, int64_t* nodes_out);
int aur_graph_launch(aur_ctx* ctx, int32_t graph, void* stream);
int aur_graph_destroy(aur_ctx* ctx, int32_t graph);

/* With option "decode_stamp_layer" = l (aur_set_option; -1 = off, the default) every decode step brackets layer l's attention launch
 * with two one-thread launches that store the device's constant-rate clock: the kernel's duration in the loop the caller really runs
 * (replayed from the graph, on whatever stream, beside whatever else) plus two kernel boundaries (~3 us).  Copies the intervals of the
 * last min(cap, steps stamped, 4096) steps to us_out (microseconds, oldest first), their number to *n_out and the total number of
 * stamped steps to *steps_total_out (may be NULL).  Synchronises the stream. */
int aur_decode_stamps_read(aur_ctx* ctx, double* us_out, int32_t cap, int64_t* steps_total_out, int32_t* n_out, void* stream);

/* ---- kernel-level entry points (parity tests, reuse by other callers) --------------------------- */
/* One ToMe step on caller data: replaces bipartite_soft_matching + merge_wavg (tome.py:18-98,207-219;
 * call site aurora.py:746-747).  metric fp32 [frames, t, c]; x fp16 [frames, t, d]; size fp32 [frames, t]
 * or NULL (= ones); x_out fp16 [frames, t-r', d]; size_out fp32 [frames, t-r'] with r' = min(r, (t-1)/2).
 * Optional index outputs (device int32, may be NULL): node_idx [frames, ceil(t/2)], unm_idx
 * [frames, ceil(t/2)-r'], src_idx [frames, r'], dst_idx [frames, r'].  r' <= 0: copies x/size.
 * Limits: c <= 128 metric channels (the similarity runs on v_mfma_f32_16x16x4_f32 over operand blocks of 16 channels), ceil(t/2) <= 4096,
 * d <= 2048 and a multiple of 8; anything else returns AUR_ERR_ARG. */
int aur_tome_step(aur_ctx* ctx, const float* metric, const void* x, const float* size, int32_t frames,
                  int32_t t, int32_t c, int32_t d, int32_t r, void* x_out, float* size_out,
                  int32_t* node_idx, int32_t* unm_idx, int32_t* src_idx, int32_t* dst_idx, void* stream);

/* The merge-map step alone on caller data (tome.hip tome_map_kernel; aurora_amd/merge_map.py step_rows): rows_dev int32 [frames, n], in
 * and out, entry e of frame f becomes the new row of old row e under ONE ToMe step over t rows - odd rows 2 i + 1 go to
 * ceil(t / 2) - r + i, even rows 2 unm[k] to k, even rows 2 src[k] to ceil(t / 2) - r + dst[k].  unm [frames, ceil(t / 2) - r], src and dst
 * [frames, r]: device int32, the shapes aur_tome_step returns.  0 <= r <= (t - 1) / 2 (the caller clamps); r = 0 is a no-op.  t <= 8192,
 * the limit of aur_tome_step (a workgroup holds one frame's row table in LDS).  Anything else returns AUR_ERR_ARG and leaves the ctx
 * usable.  The host never sees the values: entries are clamped into [0, t) and indices into their ranges before they address anything.
 * Enqueue-only. */
int aur_tome_map_rows(aur_ctx* ctx, int32_t* rows_dev, int32_t frames, int32_t n, int32_t t, int32_t r, const int32_t* unm,
                      const int32_t* src, const int32_t* dst, void* stream);
/* out[f][p][:] = tokens[f][map[f][p]][:]: the reference's unmerge closures (tome.py:83-98) applied from the last layer back to the first,
 * as one gather.  tokens fp16 [frames, n_kept, d]; map device int32 [frames, n], entries clamped into [0, n_kept); out fp16
 * [frames, n, d].  A pure copy in 16-byte pieces: a d that is not a multiple of 8, or a tokens / out that is not 16-byte aligned, returns
 * AUR_ERR_ARG.  Enqueue-only. */
int aur_unmerge_rows(aur_ctx* ctx, const void* tokens, const int32_t* map, int32_t frames, int32_t n, int32_t n_kept, int32_t d,
                     void* out, void* stream);

/* C[M, n] = act(A[M, K] W^T + bias) (+ resid): replaces F.linear.  w_packed from aur_pack_linear
 * (npad % 128 == 0, K % 64 == 0, K >= 64, n % 4 == 0, 4 <= n <= npad: the rules of aur_gemm_rows at lda = K, ldc = ldr = n); bias fp32
 * [npad] or NULL; act 0 / AUR_ACT_GELU / AUR_ACT_QUICK_GELU (any other value: none); resid fp16 [M, n] or NULL. */
int aur_linear(aur_ctx* ctx, const void* a, int32_t m, int32_t k, const void* w_packed, int32_t npad,
               int32_t n, const float* bias, int32_t act, const void* resid, void* c, void* stream);
/* One row-major tile GEMM alone on caller buffers (tests/test_gpu_gemm_modes.py): a single EPI_ROW launch through the ctx's own
 * dispatch, so "gemm_mode", "gemm_max_wgs", "gemm_tail_split" and "gemm_nt_out" apply exactly as they do to a prefill, ViT or projector
 * GEMM, with every argument aur_linear fixes exposed:
 *   a fp16, rows lda halves apart (a column window of a wider buffer when lda > k); w_packed [npad, k] from aur_pack_linear;
 *   bias fp32 [npad] (ALL npad entries are read: the 256x256 kernel's wide epilogue loads a tile's 64 bias columns unconditionally) or NULL;
 *   act 0, an AUR_ACT_*, or AUR_GEMM_SILU_MUL: columns (2j, 2j + 1) of the product are (gate_j, up_j) - the weight packed with the
 *     loader's interleaving row map - and silu(gate_j) * up_j is stored at column j: n is the interleaved width, n / 2 columns are stored;
 *   tag AUR_GEMM_TAG_*: which projection's instantiation of the 256x256 kernel runs (its activation is a compile-time constant; a tag
 *     whose activation is not `act` runs AUR_GEMM_TAG_OTHER); no effect on the result;
 *   resid fp16, rows ldr halves apart, or NULL: added after the activation; may be c itself (then ldr == ldc and no row map);
 *   out_rows_dev int32 [m] in device memory or NULL: row i of the product is stored at row out_rows_dev[i] of c, a negative entry drops
 *     the row (the caller's promise that the rows exist and differ: the host never reads the array);
 *   c fp16, rows ldc halves apart: only the stored columns of the stored rows are written.
 * Refused with AUR_ERR_ARG before anything is launched (the ctx stays usable) - each rule is an access width of the kernels:
 *   k % 64 == 0, k >= 64         a K-tile is 64 columns, and both kernels stage K-tile 0 unconditionally (gemm.hip, gemm256.hip prologue)
 *   npad % 128 == 0              whole 128-column tiles of packed weight fragments (the 256x256 kernel needs npad % 256 == 0: else the 128 one runs)
 *   n % 4 == 0, 4 <= n <= npad   a lane owns 4 consecutive columns: 8-byte h4 stores, and the residual load's column clamp is n - 4 (gemm_epilogue.h)
 *   lda >= k, lda % 8 == 0       A rows are staged by 16-byte LDS-DMA pieces; a, w_packed 16-byte aligned for the same reason
 *   ldc >= stored columns, ldc % 4 == 0 (% 2 with AUR_GEMM_SILU_MUL)     h4 (h2) stores of the direct epilogue; ldc % 8 == 0 (% 4) selects the
 *                                256x256 kernel's wide epilogue with its 16-byte (8-byte) stores, hence c 16-byte aligned
 *   ldr >= n, ldr % 4 == 0       h4 residual loads (16-byte ones in the wide epilogue when ldr % 8 == 0: resid 16-byte aligned)
 *   no residual with AUR_GEMM_SILU_MUL (the epilogues ignore it, the wide one after loading n columns of it)
 *   resid == c with ldr != ldc or a row map (a lane must read exactly the elements it later writes)
 *   a tag outside the list below (the QKV tags belong to the other epilogue), an act outside the list. */
#define AUR_GEMM_SILU_MUL 3
#define AUR_GEMM_TAG_OTHER 0
#define AUR_GEMM_TAG_VIT_OUT 2
#define AUR_GEMM_TAG_VIT_FC1 3
#define AUR_GEMM_TAG_VIT_FC2 4
#define AUR_GEMM_TAG_LLM_O 6
#define AUR_GEMM_TAG_LLM_GATEUP 7
#define AUR_GEMM_TAG_LLM_DOWN 8
int aur_gemm_rows(aur_ctx* ctx, const void* a, int32_t m, int32_t k, int32_t lda, const void* w_packed, int32_t npad, int32_t n,
                  const float* bias, int32_t act, int32_t tag, const void* resid, int32_t ldr, const int32_t* out_rows_dev, void* c,
                  int32_t ldc, void* stream);
/* Same contraction through the decode weight-streaming kernel (m <= 128, k % 128 == 0, any n <= npad); out fp32 [m, n]. */
int aur_linear_skinny(aur_ctx* ctx, const void* a, int32_t m, int32_t k, const void* w_packed, int32_t npad,
                      int32_t n, float* out, void* stream);
int aur_layernorm(aur_ctx* ctx, const void* x, int32_t rows, int32_t d, const float* w, const float* b,
                  float eps, void* y, void* stream);
int aur_rmsnorm(aur_ctx* ctx, const void* x, int32_t rows, int32_t d, const float* w, float eps, void* y,
                void* stream);

/* One full ViT encoder layer from caller state (teacher-forced parity): replaces
 * AuroraCLIPEncoderLayer.forward (aurora.py:713-759).  x fp16 [frames, t, D]; size fp32 [frames, t] or NULL.
 * Outputs: x_out fp16 [frames, t', D], size_out fp32 [frames, t'], metric_out fp32 [frames, t, head_dim]
 * (may be NULL), index arrays as in aur_tome_step (may be NULL).  Uses the ctx workspace. */
int aur_vit_layer(aur_ctx* ctx, int32_t layer, const void* x, const float* size, int32_t frames, int32_t t,
                  int32_t r, void* x_out, float* size_out, float* metric_out, int32_t* node_idx,
                  int32_t* unm_idx, int32_t* src_idx, int32_t* dst_idx, void* stream);

/* The attention kernels alone on caller rows (tests/test_gpu_attention.py): the layer's own fragment writer, then its attention launch.
 * aur_attn_rows: launch_gemm(EPI_QKV) + launch_attention (attn_kernel: ViT and causal prefill).  x fp16 [nseq * rows, kx] (kx % 64 == 0),
 * w_packed [npad, kx] from aur_pack_linear with the loader's QKV row map (npad = the model's packed QKV width), bias fp32 [npad] or NULL.
 * With x = [q | k | v] and the identity as weight the fragments hold exactly the caller's q, k, v.  layout AUR_ATTN_VIT: one page per
 * sequence in the workspace, the ctx's ViT head geometry, seq0 = rope = 0, nseq <= max_frames, rows <= the padded token capacity;
 * AUR_ATTN_LLM: layer 0 of the KV pool through the selected bank's page table, KV sequences [seq0, seq0 + nseq), positions [0, rows),
 * RoPE on (rope = 1) or off.  rows: a multiple of 32, >= round_up(t, 32).  Valid keys / queries per sequence: t by value (lens_dev ==
 * NULL), or lens_dev int32 [nseq] in device memory, clamped into [1, rows] (the AttnArgs seq_lens path: output rows at or beyond a
 * sequence's length are zeros).  out fp16 [nseq * rows, heads * head_dim] row-major.  K / V of all `rows` positions stay in the pages
 * (they feed aur_attn_decode_rows); no decode state is touched.  Bad arguments: AUR_ERR_ARG, the ctx stays usable.
 * aur_attn_decode_rows: launch_xfrag_pack + launch_skinny(SK_QKV) + launch_decode_attention (decode_attn_dot_kernel, decode_attn_combine_kernel)
 * with the split geometry of the decode step ("dec_attn_pps", "dec_attn_local").  x fp16 [rows, kx] (rows <= max_batch, kx % 128 == 0);
 * pos_dev int32 [rows] in device memory: tokens already cached for KV sequence b of the selected bank - the step writes its K / V at
 * position pos[b] (< the positions of a sequence's pages: the CALLER'S promise, the host never reads it) and attends to keys [0, pos[b]].
 * out fp16 [rows, hidden] row-major.  scratch: aur_attn_decode_scratch_bytes(ctx, kx) bytes, 256-byte aligned.  Uses the decode step's
 * query / partial / output scratch of the workspace: not beside a running aur_llm_decode. */
#define AUR_ATTN_VIT 0
#define AUR_ATTN_LLM 1
int aur_attn_rows(aur_ctx* ctx, int32_t layout, const void* x, int32_t nseq, int32_t rows, int32_t kx, const void* w_packed, int32_t npad,
                  const float* bias, int32_t seq0, int32_t rope, int32_t t, const int32_t* lens_dev, int32_t causal, void* out, void* stream);
int64_t aur_attn_decode_scratch_bytes(const aur_ctx* ctx, int32_t kx);
int aur_attn_decode_rows(aur_ctx* ctx, const void* x, int32_t rows, int32_t kx, const void* w_packed, int32_t npad, const int32_t* pos_dev,
                         int32_t rope, void* scratch, int64_t scratch_bytes, void* out, void* stream);

/* One decode projection alone on caller rows (tests/test_gpu_skinny_modes.py): the producer of x fragments, then launch_skinny in the
 * structure the decode step of THIS engine picks (capacity, "skinny_row_split_min_k", "decode_fused_reduce", "decode_half_grid"): the
 * arguments come from the builders the step itself calls, and the rule is stated once, in mk_skinny (aurora_amd/csrc/engine.hip).
 * x fp16 [rows, k] lands at batch rows [b0, b0 + rows) (b0 + rows <= max_batch; k % 128 == 0); every other batch row of the x fragments,
 * up to rp = round_up(max_batch, 16), holds `fill`.  fold = 1: the producer is the prefill hand-over's (x fragments + sum(x^2) into
 * ssq_in), the projection scales by rsqrt(sum / k + eps) and must clear ssq_zero, which the entry fills with a non-zero pattern first;
 * fold = 0: plain fragments.  w_packed [npad, k] from aur_pack_linear (npad % 256 == 0; AUR_PROJ_SILU_MUL: gate / up rows interleaved).
 * mode AUR_PROJ_ROW      (no fold, n % 32 == 0): out fp16 [rp, n] is the residual, in and out; ssq_out u64 [16][128] in and out (the
 *                        projection adds); row_cnt_out int32 [npad / 16] or NULL: the fused reduce's arrival counters after the launch.
 *      AUR_PROJ_SILU_MUL (n % 64 == 0): out fp16 [rp, n / 2], in (the caller's sentinel) and out.
 *      AUR_PROJ_LOGITS   (any n): out fp32 [rp, n] plus at least 4 floats of guard, written in place (16-byte aligned).
 * out_bytes: size of out.  ssq_in / ssq_zero: u64 [16][128] device arrays (fold only).  scratch: 256-byte aligned, at least
 * aur_decode_proj_scratch_bytes bytes; no workspace buffer is used.  Bad arguments: AUR_ERR_ARG, the ctx stays usable. */
#define AUR_PROJ_ROW 0
#define AUR_PROJ_LOGITS 1
#define AUR_PROJ_SILU_MUL 2
int64_t aur_decode_proj_scratch_bytes(const aur_ctx* ctx, int32_t k, int32_t npad);
int aur_decode_proj_rows(aur_ctx* ctx, int32_t mode, const void* x, int32_t rows, int32_t b0, int32_t k, const void* w_packed, int32_t npad,
                         int32_t n, int32_t fold, float eps, float fill, void* out, int64_t out_bytes, unsigned long long* ssq_out,
                         unsigned long long* ssq_in, unsigned long long* ssq_zero, int32_t* row_cnt_out, void* scratch,
                         int64_t scratch_bytes, void* stream);

/* Copy the last-position logits of the most recent prefill / decode step into dst_dev: fp32 [batch, vocab]. */
int aur_copy_logits(aur_ctx* ctx, float* dst_dev, void* stream);

/* The sampled pick alone on caller rows (parity tests).  logits fp32 [rows, vocab] device (16-byte aligned); params_dev [rows];
 * n_dev int32 [rows] (the token index that goes into the counter); tokens_out int32 [rows]; kept_out int32 [rows] or NULL (the size
 * of the kept set). */
int aur_sample_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const aur_sampling* params_dev,
                    const int32_t* n_dev, int32_t* tokens_out, int32_t* kept_out, void* stream);
/* The logit-rule kernels alone on caller rows (parity tests).  logits fp32 [rows, vocab] device, rewritten in place; ids_dev int32
 * [rows, ids_stride] and lens_dev int32 [rows]: row i's history is ids_dev[i][0 .. min(lens_dev[i], ids_stride)); rules_dev [rows];
 * eos_id as aur_begin_batch takes it.  restore = 0: the processed rows stay; restore = 1: apply, then restore - every row is bitwise
 * its input again.  Allocates its side list, synchronises the stream and frees it: not recordable. */
int aur_logit_rules_rows(aur_ctx* ctx, float* logits, int32_t rows, int32_t vocab, const int32_t* ids_dev, int32_t ids_stride,
                         const int32_t* lens_dev, const aur_logit_rules* rules_dev, int32_t eos_id, int32_t restore, void* stream);
/* The guidance kernels alone on a caller's buffer (parity tests): logits fp32 [rows, vocab], read and written; recs_dev [rows], whose
 * partners are rows of the same buffer (clamped into [0, rows)); save fp32 [rows, vocab].  mode 0: guidance_apply_kernel - a leader's
 * row goes into its save row and the guided row stands in its place; every other row, and every other save row, is not touched.
 * mode 1: guidance_restore_kernel - the leaders' save rows back.  Enqueue-only. */
int aur_guidance_rows(aur_ctx* ctx, float* logits, int32_t rows, int32_t vocab, const aur_guidance* recs_dev, float* save, int32_t mode,
                      void* stream);
/* stop_check_kernel alone on caller rows (parity tests).  ids_dev int32 [rows, ids_stride] and lens_dev int32 [rows]: row i's generated
 * tokens are ids_dev[i][0 .. min(lens_dev[i], ids_stride)); rules_dev [rows] (8-byte aligned); finished_dev int32 [rows], read and written:
 * a row whose flag is set is skipped, a row that stops gets 1; batch_max_new: the limit a record with max_new_tokens <= 0 stands for
 * and that ends a row on its own, as advance_tail does in the engine.  The byte table as aur_stop_vocab takes it (NULL: no string
 * matches).  Enqueue-only. */
int aur_stop_rows(aur_ctx* ctx, int32_t rows, const int32_t* ids_dev, int32_t ids_stride, const int32_t* lens_dev, const aur_stop_rules* rules_dev,
                  int32_t* finished_dev, int32_t batch_max_new, const int32_t* offsets_dev, const uint8_t* bytes_dev, int32_t vocab, int64_t nbytes, void* stream);

/* ---- scoring given continuations (lmms-eval's `loglikelihood` request) ---------------------------------------
 * aur_score_rows: the kernel alone on caller rows.  logits fp32 [rows, vocab] device; targets_dev int32 [rows].  Per row, with a =
 * the first index of the maximum m: logprob_out = (l[target] - m) - log(sum exp(l[i] - m)) in fp32 and argmax_out = a - a pure function
 * of the row's values (the same bits at any row index, row count or alignment).  A target outside [0, vocab) marks an unused entry:
 * logprob 0, argmax -1, the row is not read.  aurora_amd/scoring.py is the definition in numpy.
 * aur_llm_score_var: the layer stack of aur_llm_prefill_stage_var (pos0 == 0) or aur_llm_extend_stage_var (pos0 a positive multiple of
 * the 64-token page) over KV sequences [seq0, seq0 + nseq) - same argument checks, same clearing of the padding rows, the K / V of
 * every position written, no decode state touched (on spare sequences it may sit between two aur_llm_decode calls) - except that the
 * last layer always runs unpruned; then nscore_cap entries are scored, in chunks of max_batch, through the pick path's lm_head (folded
 * final norm) and the kernel above, on the caller's scratch (aur_score_scratch_bytes, 256-byte aligned; a function of the config
 * alone).  Entry j names flat row score_rows_dev[j] = i * stride + r of embeds - the hidden state at position pos0 + r of sequence i -
 * and the target score_targets_dev[j] it is scored against.  A row < 0, outside nseq * stride or at / beyond its sequence's clamped
 * length, or a target outside [0, vocab), marks an unused entry (logprob 0, argmax -1).  logits_out: fp32 [nscore_cap, vocab] or
 * NULL (tests; rows of unused entries are unspecified).  The host reads none of the device arrays: enqueue-only, recordable with
 * aur_graph_begin; a capture freezes the capacity and the pointers, not the values.
 * CONTRACT: for an entry naming row r of sequence i the logits row is BITWISE what aur_copy_logits returns after
 * aur_llm_prefill(slot, embeds_i[0 .. pos0 + r], pos0 + r + 1) on the same ctx, argmax_out is that prefill's greedy first token, and
 * logprob_out / argmax_out are bitwise what aur_score_rows gives on that row. */
int64_t aur_score_scratch_bytes(const aur_ctx* ctx);
int aur_llm_score_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride, const int32_t* lens_dev,
                      const int32_t* score_rows_dev, const int32_t* score_targets_dev, int32_t nscore_cap, void* scratch,
                      int64_t scratch_bytes, float* logprob_out, int32_t* argmax_out, float* logits_out, void* stream);
int aur_score_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const int32_t* targets_dev, float* logprob_out,
                   int32_t* argmax_out, void* stream);

/* ---- log-probabilities of GENERATED tokens, with top-n alternatives (the reference tree's serving engine offers
 * it per request as return_logprob / top_logprobs_num, from log_softmax of the raw last-position logits:
 * sglang/srt/layers/logits_processor.py:187-218).  aurora_amd/scoring.py token_logprobs is the definition in numpy.
 * For the fp32 logits row l a token t was picked from - by the greedy or the sampled pick; temperature, top-k and top-p do not enter -:
 * lp(t) = (l[t] - m) - log(sum exp(l[i] - m)), bitwise what aur_score_rows says about that row; and the first top_n (0 .. 8) entries
 * of the row in the order (value descending, index ascending), each with its lp: rank 0 is aur_score_rows' argmax, ties go to the
 * lower index, ranks at or beyond vocab are (-1, 0.0).
 * The state of one bank lives in a CALLER-OWNED device buffer of aur_logprob_bytes bytes (16-byte aligned; the layout is the library's
 * business): nothing is allocated here, aur_workspace_bytes does not grow, and a process that never asks launches exactly what it did.
 * aur_logprob_enable acts on the CURRENT bank: resets the buffer on the stream (no slot holds a record) and, from then on, every
 * prefill's first token, every commit and every decode step - captured or eager - is followed by one more launch that records the
 * newest token of each slot that appended one.  buf_dev == NULL turns it off again.  Call it before aur_begin_batch.  The choice is
 * frozen in the bank's captured decode graphs, which the call drops (as option "sampling" does), and in a CALLER's capture that holds a
 * prefill / commit / aur_slot_reset, which the caller re-captures; AUR_ERR_STATE inside aur_graph_begin / aur_graph_end.
 * aur_begin_batch, aur_slot_reset and the commits clear the records of the slots whose lengths they clear.
 * aur_get_logprobs (synchronises, like aur_get_outputs): lp_host fp32 [batch * max_new_tokens], top_ids_host int32 / top_lp_host fp32
 * [batch * max_new_tokens * top_n] (NULL to skip), lens_host [batch] = tokens recorded per slot (= the slot's generated length); entries
 * at or beyond a slot's length are 0 / (-1, 0.0).  max_new_tokens: the batch's, as for aur_get_outputs.
 * aur_slot_collect_logprobs: the same for slots [slot0, slot0 + nslots) device-to-device, enqueue-only and recordable like
 * aur_slot_collect.
 * aur_token_logprob_rows: the kernel alone on caller rows.  logits fp32 [rows, vocab] device; tokens_dev int32 [rows]; lp_out fp32
 * [rows]; top_ids_out int32 / top_lp_out fp32 [rows, top_n] (NULL allowed for top_n == 0).  A pure function of the row's values: the
 * same bits at any row index, row count or alignment.  A token outside [0, vocab) marks an unused entry: lp 0, every rank (-1, 0.0),
 * the row is not read. */
int64_t aur_logprob_bytes(const aur_ctx* ctx, int32_t top_n);      /* -1: top_n outside [0, 8] */
int aur_logprob_enable(aur_ctx* ctx, int32_t top_n, void* buf_dev, int64_t nbytes, void* stream);
int aur_get_logprobs(aur_ctx* ctx, float* lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* lens_host, void* stream);
int aur_slot_collect_logprobs(aur_ctx* ctx, int32_t slot0, int32_t nslots, float* lp_dev, int32_t* top_ids_dev, float* top_lp_dev,
                              int32_t* lens_dev, void* stream);
int aur_token_logprob_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const int32_t* tokens_dev, int32_t top_n,
                           float* lp_out, int32_t* top_ids_out, float* top_lp_out, void* stream);

/* ---- attention of every GENERATED token over a prefix window of its context (transformers'
 * generate(output_attentions=True), averaged).  aurora_amd/attn_map.py is the definition in numpy.
 * The decode step that picks generated token i >= 1 of a slot (token 0 is the prefill's and has no record) attends, in every layer l and
 * head h, with the roped fp16 query it wrote to keys [0, npos = pos + 1) of the slot's pages - the one it has just written included:
 * P[l, h, j] = softmax_j(scale q . k_j), the distribution the decode attention itself uses, evaluated in fp32.  The record is
 * A[i, j] = mean over the selected layers and all heads of P[l, h, j] for j < min(window, npos), and exactly 0.0 for the other j < window.
 * Row 0 of a slot and every row at or beyond its generated length are zeros; with window >= npos a recorded row sums to 1.
 * window: a multiple of 64 in [64, max_ctx rounded up to 64].  layer_mask: bit l = layer l (at most 64 layers), 0 = all.
 * The state of one bank lives in a CALLER-OWNED device buffer of aur_attn_map_bytes bytes (256-byte aligned: records fp32
 * [max_batch][max_new_tokens][window], then the recorder's scratch): nothing is allocated here, aur_workspace_bytes does not grow, and a
 * process that never asks launches exactly what it did.  aur_attn_map_enable acts on the CURRENT bank: clears the records on the stream
 * and, from then on, every decode step - captured or eager - launches the recorder (attn_map.hip: two kernels, one more pass over K)
 * behind the QKV projection of each selected layer.  Slots that are finished or full write nothing.  The record is a function of the
 * slot's own q and K alone: bitwise the same at any batch, slot, bank, split geometry ("dec_attn_pps", "dec_attn_local") or launch
 * form.  buf_dev == NULL turns it off again.  The choice is frozen in the bank's captured decode graphs, which the call drops;
 * AUR_ERR_STATE inside aur_graph_begin / aur_graph_end.  aur_begin_batch, aur_slot_reset and the commits clear the rows of the slots
 * whose lengths they clear (a caller's capture that holds one of them is re-captured by the caller).
 * aur_get_attn_map (synchronises, like aur_get_logprobs): map_host fp32 [batch * max_new_tokens * window], max_new_tokens the batch's.
 * aur_slot_collect_attn_map: the same for slots [slot0, slot0 + nslots) device-to-device, enqueue-only and recordable.
 * aur_attn_map_rows: the kernels alone on caller rows, beside aur_attn_decode_rows and with its arguments: one layer, all heads, row b of
 * out fp32 [rows, window] is the record of row b at position pos_dev[b].  scratch: aur_attn_map_rows_scratch_bytes(ctx, kx, window). */
int64_t aur_attn_map_bytes(const aur_ctx* ctx, int32_t window);      /* -1: a bad window */
int aur_attn_map_enable(aur_ctx* ctx, int32_t window, uint64_t layer_mask, void* buf_dev, int64_t nbytes, void* stream);
int aur_get_attn_map(aur_ctx* ctx, float* map_host, void* stream);
int aur_slot_collect_attn_map(aur_ctx* ctx, int32_t slot0, int32_t nslots, float* out_dev, void* stream);
int64_t aur_attn_map_rows_scratch_bytes(const aur_ctx* ctx, int32_t kx, int32_t window);
int aur_attn_map_rows(aur_ctx* ctx, const void* x, int32_t rows, int32_t kx, const void* w_packed, int32_t npad, const int32_t* pos_dev,
                      int32_t rope, void* scratch, int64_t scratch_bytes, int32_t window, float* out, void* stream);

/* Tuning knobs.  Invalidate the captured decode graphs (of every bank): "decode_fused_reduce" 0 (default: the split-K residual projections are followed
 * by a reduce launch) / 1 (the last-arriving split reduces inside the kernel; bitwise the same), "dec_attn_local" 1 (default: on engines
 * of 8-15 slots x 32 heads the splits of a (sequence, head) are the waves of one attention workgroup, joined through LDS) / 0
 * (decode_attn_combine_kernel joins them; bitwise the same), "dec_attn_pps" pages per decode-attention split, "skinny_row_split_min_k"
 * (K from which the residual projections of an engine of <= 64 slots take the split-K structure), "decode_stamp_layer" (see
 * aur_decode_stamps_read), "sampling" 0 (default: the pick is argmax_advance_kernel) / 1 (sample_advance_kernel with the slots'
 * aur_sampling records; the kernel choice is frozen inside captured graphs - the decode step's, which this call drops, and a CALLER's
 * capture that holds a prefill / commit, which the caller re-captures), "sample_stage" 1 (default: the sampler stages its logits
 * row in LDS when it fits) / 0 (re-reads it from L2; same tokens), "logit_rules" 0 (default: the launches are exactly those of a ctx
 * that never heard of them) / 1 (logit_rules_apply_kernel ahead of every pick and logit_rules_restore_kernel behind it, with the slots'
 * aur_logit_rules records; frozen inside captured graphs exactly like "sampling"; the first 1 allocates the banks' side lists -
 * max_batch * (max_new_tokens + 1) entries of 8 bytes each - which live as long as the ctx), "guidance" 0 (default: the launches are exactly those of a ctx that never heard of it) / 1 (guidance_apply_kernel ahead of the logit rules,
 * guidance_restore_kernel behind the pick and guidance_follow_kernel behind the stop check, with the slots' aur_guidance records; frozen inside captured graphs exactly like
 * "sampling"; the first 1 allocates the banks' records and save buffers - max_batch * llm_vocab * 4 bytes each - which live as long as the ctx), "stop_rules" 0 (default: the launches are exactly those of a ctx that never
 * heard of it) / 1 (stop_check_kernel behind every pick, with the slots' aur_stop_rules records; frozen inside captured graphs exactly like
 * "sampling"; the first 1 allocates the banks' records - max_batch * sizeof(aur_stop_rules) each - which live as long as the ctx).  Keep the graphs: "tome_fused_ln" 1 (default: LayerNorm 2 of a merging ViT layer comes out of the ToMe merge
 * launch) / 0 (its own launch; bitwise the same); "prefill_prune_last" 1 (default) / 0: the last layer of a prefill computes K / V for
 * every position and the rest for each sequence's last 128 rows only - nothing else is read after it; bitwise the same logits and K / V;
 * "decode_half_grid" 1 / 0 (one graph is kept per setting): the next aur_llm_decode calls go to a stream that owns half of the CUs, so
 * the QKV / gate-up projections launch half as many workgroups with twice the tiles each - bitwise the same tokens; the GEMM knobs (no
 * GEMM is part of the captured decode step): "gemm_mode" 0 (128x128) / 1 (auto) / 2 (force 256x256), "gemm_nt_out" -1 (default: GEMM
 * outputs larger than the eight L2s together, 32 MiB, are written with non-temporal stores) / 0 (never) / 1 (always), "gemm_max_wgs"
 * n > 0: the 256x256 GEMM runs persistently on at most n workgroups (= CUs; 0 = one workgroup per tile), "gemm_tail_split" 1 (a mostly
 * idle last round of the 256x256 kernel goes to the 128x128 kernel over the bottom rows) / 0, "microbench_prefill_nseq" sequences per
 * pass for the pre_* microbenchmarks.  Every knob is state of THIS ctx.  The gemm_* knobs, tome_fused_ln, prefill_prune_last,
 * dec_attn_local, decode_fused_reduce and decode_half_grid are bit-neutral; dec_attn_pps / skinny_row_split_min_k change how fp32
 * partial sums are partitioned (same tolerance, not bit-comparable across settings).  Knobs whose losing arm was measured twice are
 * gone (rounds 5-6): the decode structure is a function of the engine's capacity alone (x fragments per wave up to 32 slots, x through
 * LDS above; mk_skinny in aurora_amd/csrc/engine.hip is the one place that picks it, for the step, aur_microbench and the parity entries), the 256x256 GEMM always takes the LDS-transposed epilogue and the compact tile order, residual projections run 8 waves. */
int aur_set_option(aur_ctx* ctx, const char* name, int64_t value);
/* Time one kernel of the LLM path in isolation on the current generation state (after aur_llm_prefill):
 * kernel in {dec_norm, dec_qkv, dec_attn, dec_o, dec_gateup, dec_down, dec_lm_head, dec_pick (the token pick of the current "sampling" mode), dec_rules (the logit-rule apply + restore pair; option "logit_rules" 1), dec_guid (guidance's apply + restore + follow; option "guidance" 1), dec_stop (stop_check_kernel; option "stop_rules" 1), pre_norm, pre_qkv, pre_attn,
 * pre_o, pre_gateup, pre_down}; mean microseconds per launch over `iters` launches cycling through the layers. */
int aur_microbench(aur_ctx* ctx, const char* kernel, int32_t iters, double* us_out, void* stream);

/* Per-stage kernel-time accounting (HIP events on the caller's stream): enable, run, read back
 * milliseconds for "vit", "project", "prefill", "decode" - and the dominant decode GEMM kernel. */
int aur_profile_enable(aur_ctx* ctx, int32_t on);
int aur_profile_read(aur_ctx* ctx, const char* stage, double* ms_out, int64_t* launches_out);

/* ---- input stage (stateless, no ctx) --------------------------------- */
/* Replaces CLIPImageProcessor(size=378, crop_size=378)(frames)["pixel_values"].to(float16) at inference.py:58-63,
 * 71-75 (Pillow 8-bit BICUBIC resize of the shortest edge to `image`, centre crop, rescale, normalise) for decoded
 * rgb24 frames that are already on the device.  Bit-exact against the reference processor.
 *
 * aur_preprocess_plan: HOST-only; fills `plan_host` (aur_preprocess_plan_len int32 words: geometry header, per output
 * column / row the first input index, tap count and int32 taps with 22 fractional bits) for one input size.  The
 * caller copies it to the device once per input size and reuses it.
 * aur_preprocess_frames: frames_dev uint8 [frames, in_h, in_w, 3]; lut_dev fp16 bits [3][256] =
 * ((v * rescale) - mean[c]) / std[c] computed by the caller from preprocessor_config.json; tmp_dev
 * aur_preprocess_tmp_bytes; out_pixels fp16 [frames, 3, image, image] (the layout aur_vit_encode takes). */
int64_t aur_preprocess_plan_len(int32_t in_h, int32_t in_w, int32_t image);
int aur_preprocess_plan(int32_t in_h, int32_t in_w, int32_t image, int32_t* plan_host, int64_t len);
int64_t aur_preprocess_tmp_bytes(int32_t frames, int32_t in_h, int32_t in_w, int32_t image);
int aur_preprocess_frames(const uint8_t* frames_dev, int32_t frames, int32_t in_h, int32_t in_w, int32_t image,
                          const int32_t* plan_dev, const uint16_t* lut_dev, uint8_t* tmp_dev, void* out_pixels,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AURORA_HIP_H */
