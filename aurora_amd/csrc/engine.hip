// libaurora_hip.so - context, workspace carving, pipelines and the extern "C" boundary (include/aurora_hip.h).
//
// Pipelines restate the reference's call sequence for the AuroraCap inference path with one enqueue per
// kernel on the caller's stream:
//   aur_vit_encode      <- AuroraEncoder.forward + AuroraCLIPEncoder loop   (aurora.py:883-904, 772-860, 713-759)
//   aur_vit_encode_map  <- the same with merge_source carried through the layers (tome.py:222-232)
//   aur_project_splice  <- projector + prepare_inputs_labels_for_multimodal (aurora.py:254-258, utils.py:138-295)
//   aur_llm_prefill / aur_llm_decode <- LlamaForCausalLM.generate greedy    (inference.py:89-96)
#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/aurora_hip.h"
#include "kernels.h"
#include "advance.h"      // xfrag_piece

struct Tensor {
    const void* p;
    int64_t bytes;
};

struct VitLayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_b, *out_b, *fc1_b, *fc2_b;
    const half_t *qkv_w, *out_w, *fc1_w, *fc2_w;
};
struct LlmLayerW {
    const float *ln1_w, *ln2_w;
    const half_t *qkv_w, *o_w, *gateup_w, *down_w;
};

struct StageTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0;
    int64_t launches = 0;
    bool open = false;
    uint64_t range_id = 0;       // roctx range of the stage (AURORA_ROCTX=1)
    bool range_open = false;
};

struct aur_ctx {
    aur_config cfg;
    std::string err;
    std::unordered_map<std::string, Tensor> tensors;
    char* ws = nullptr;
    int64_t ws_bytes = 0;
    char* kvpool = nullptr;
    int64_t kv_bytes = 0;
    bool finalized = false;
    // derived: vision
    int v_hd, v_hd_pad, v_kblk, v_vd16, v_qcols, v_qkv_npad, v_dpad, v_mlp_pad, v_npatch, v_t0, v_t0pad, v_kpad, v_native_npatch;
    // derived: llm
    int l_hd, l_kblk, l_vd16, l_qkv_npad, l_gu_npad, l_dpad, l_vocab_pad, l_max_pages, l_ctx_pad;
    int64_t l_page_halves, l_layer_halves;
    int kv_seqs = 0;                 // KV sequences per bank (max_batch decode slots + cfg.spare_slots)
    // weights
    std::vector<VitLayerW> vl;
    std::vector<LlmLayerW> ll;
    const half_t *v_patch_w, *v_cls, *v_pos, *l_embed, *l_head_w;
    const float *v_preln_w, *v_preln_b, *l_norm_w;
    std::vector<const half_t*> p_w;      // projector Linear layers (modeling_projector.py:20-33): [proj_depth] packed weights
    std::vector<const float*> p_b;       //                                                        and biases (zeros for bias = False)
    int p_depth = 2, p_act = ACT_GELU;
    // workspace regions (vision)
    half_t *w_col, *w_patch, *w_xa, *w_xb, *w_xn, *w_qf, *w_kv, *w_attn, *w_h;
    float *w_metric, *w_mhat, *w_nmax, *w_sza, *w_szb;
    int32_t *w_nidx, *w_unm, *w_src, *w_dst;
    // workspace regions (llm)
    half_t *l_xn, *l_qf, *l_attn, *l_h, *l_p1, *d_q, *d_attn, *d_h, *d_scr;
    float *d_part_o, *d_part_ml;
    float2* l_rope;
    int32_t* s_ptab;                 // page tables of both banks
    int nsplit = 1, pps = 1;
    int last_prefill_len = 0, mb_nseq = 1;                         // tuning knobs (aur_set_option)
    int decode_half = 0;             // 1: the next aur_llm_decode calls target a stream that owns half of the CUs (own hipGraph)
    int gemm_mode = 1, gemm_max_wgs = 0, gemm_tail_split = 1, prune_last = 1, gemm_nt_out = -1;                           // GEMM knobs: per ctx, copied into GemmArgs at every launch
    int skinny_variant = 0, row_split_min_k = 8192;                             // decode projections: x through LDS (engines of > 32 slots)
    int skinny_variant_wide = 0;                                                // the two WIDE projections (QKV, gate/up): x through LDS at every capacity
    float* d_part_row = nullptr;                                                // split-K partials of the SK_ROW projection
    int* d_row_cnt = nullptr;                                                   // its arrival counters (zero between launches)
    int attn_local = 1;                                                         // 1: workgroup-local join of the decode attention's splits where it applies (mk_dec_attn); 0 = always decode_attn_combine_kernel (A/B and test)
    int tome_fused_ln = 1;                                                      // 1: LayerNorm 2 of a merging ViT layer comes out of the ToMe merge launch (bitwise norm_kernel's result; 0 = its own launch, A/B and test only)
    int sampling = 0, sample_stage = 1;                                         // the token pick: 0 argmax_advance_kernel, 1 sample_advance_kernel (row staged in LDS / re-read from L2)
    int logit_rules = 0;                                                        // 1: logit_rules_apply_kernel ahead of every pick, logit_rules_restore_kernel behind it (the slots' aur_logit_rules records)
    int stop_rules = 0;                                                         // 1: stop_check_kernel behind every pick (the slots' aur_stop_rules records)
    const int32_t* stop_off = nullptr;                                          // aur_stop_vocab: the caller's token byte table (device memory)
    const uint8_t* stop_bytes = nullptr;
    int stop_vocab = 0;
    int64_t stop_nbytes = 0;
    int guidance = 0;                                                           // 1: guidance_apply_kernel ahead of the logit rules, guidance_restore_kernel behind the pick, guidance_follow_kernel behind the stop check (the slots' aur_guidance records)
    int fused_reduce = 0;                                                       // 1: the split-K reduce runs inside the projection kernel
    // Generation banks: double-buffered per-batch state (KV slots, residual stream, sum(x^2), logits, outputs, graphs) so
    // that one batch can decode on one stream while the next batch's ViT + prefill run on another.  Every generation call
    // acts on the CURRENT bank (aur_select_bank), reached through bank() only.
    struct Bank {
        half_t* d_x;
        unsigned long long *s_ssq_mlp, *s_ssq_attn;
        float* d_logits;
        int32_t *s_pos, *s_ids, *s_len, *s_fin;
        aur_sampling* s_samp;                                // per-slot sampling parameters (aur_slot_sampling); temperature 0 = greedy
        aur_logit_rules* s_rules;                            // per-slot logit rules (aur_slot_logit_rules); all zero = neutral
        int32_t* lr_cnt;                                     // entries of each slot's side list written by the last apply
        void* lr_save = nullptr;                             // side lists [max_batch][max_new_tokens + 1] of (index, original logit): allocated by option "logit_rules" 1
        aur_stop_rules* s_stop = nullptr;                    // per-slot stop records (aur_slot_stop) [max_batch]; all zero = neutral: allocated by option "stop_rules" 1
        aur_guidance* s_guid = nullptr;                      // per-slot guidance records (aur_slot_guidance); all zero = neutral: allocated by option "guidance" 1
        float* gd_save = nullptr;                            // the leaders' model rows while their guided rows stand in d_logits [max_batch][vocab]: allocated with the records
        int32_t* ptab;                                       // page-table rows of the bank's kv_seqs sequences
        // log-probabilities of generated tokens (aur_logprob_enable): the caller's buffer, nullptr = off.  lp_len [max_batch]: tokens of
        // slot b recorded so far; lp [b][max_new], lp_top_id / lp_top_lp [b][max_new][lp_top_n]: rows max_new apart, like s_ids
        int32_t *lp_len = nullptr, *lp_top_id = nullptr;
        float *lp = nullptr, *lp_top_lp = nullptr;
        int lp_top_n = 0;
        // attention over the prompt during decode (aur_attn_map_enable): the caller's buffer, nullptr = off.  am [b][max_new][am_window]:
        // rows max_new apart, like s_ids; am_score / am_ml: the recorder's scratch (attn_map.hip); am_mask bit l = layer l records
        float *am = nullptr, *am_score = nullptr, *am_ml = nullptr;
        int am_window = 0, am_nlayers = 0;
        uint64_t am_mask = 0;
        int batch = 0, max_new = 0, eos = -1;
        hipGraphExec_t graph = nullptr, graph_h = nullptr;   // decode step: full grid / half grid (decode_half)
        int graph_batch = 0;
    } banks[2];
    int nbanks = 1, cur_bank = 0;
    Bank& bank() { return banks[cur_bank]; }
    const Bank& bank() const { return banks[cur_bank]; }
    // caller-captured hipGraphs (aur_graph_begin / aur_graph_end / aur_graph_launch): a front end per shape bucket
    struct UserGraph {
        hipGraphExec_t exec = nullptr;
        int64_t nodes = 0;
    };
    std::vector<UserGraph> ugraphs;                      // handle = index + 1; destroyed slots keep exec == nullptr
    bool capturing = false;
    hipStream_t cap_stream = nullptr;
    // in-loop timing of the dominant decode kernel: option "decode_stamp_layer" brackets that layer's attention launch with two
    // one-thread launches that store the device's constant-rate clock (part of the captured step, so the timed loop itself is measured)
    int stamp_layer = -1;
    unsigned long long* d_stamp = nullptr;               // [0] steps stamped so far, [8 + 2 * (step % AUR_STAMP_RING) + {0, 1}] begin / end
    // profiling
    bool prof = false;
    std::unordered_map<std::string, StageTimer> timers;
    struct KernelEvents {                                // HIP-event pairs around every launch of one decode kernel
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
        size_t used = 0;
        double ms = 0;
        int64_t n = 0;
    } kev[4];                                            // 0: decode attention (main kernel), 1: gate/up GEMV, 2: ToMe step (3 launches), 3: lm_head + argmax
};

static std::string g_create_err;

static int aur_fail(aur_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_err = buf;
    return code;
}
#define CK(expr)                                                                                       \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return aur_fail(ctx, AUR_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Entry points that synchronise (or destroy graphs) refuse to run inside aur_graph_begin / aur_graph_end BEFORE touching the runtime:
// a synchronising HIP call on a capturing stream invalidates the capture and (ROCm 7.2) leaves the stream refusing later launches
#define NO_CAPTURE(who)                                                                                                     \
    do {                                                                                                                    \
        if (ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "%s inside aur_graph_begin / aur_graph_end: it synchronises", who); \
    } while (0)

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }
static inline int64_t rup64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// every GEMM of a ctx goes through here: the ctx's tuning knobs travel in the argument block (no process-global state)
static hipError_t ctx_gemm(const aur_ctx* ctx, GemmArgs a, int epi, hipStream_t s) {
    a.gemm_mode = ctx->gemm_mode;
    a.max_wgs = ctx->gemm_max_wgs;
    a.tail_split = ctx->gemm_tail_split;
    // Output policy.  A round of 256x256 tiles writes 256 x 128 KiB in one burst (every CU reaches its epilogue together) - the capacity
    // of the eight L2s; with the default policy that burst evicts the operand panels the next tiles share through L2.  Outputs the L2s
    // could not hold for the consumer anyway go out non-temporal (round 4: ViT fc1 +8 %, prefill gate/up +3 %, QKV +2-3 %); a single
    // clip's prefill (17-50 MB per projection, read back at once by the next launch) keeps the default (+1 % on its layer stack).
    const int64_t out_cols = epi == EPI_QKV ? (int64_t)a.q_cols + 2 * a.k_cols : (a.act == ACT_SILU_MUL ? a.n_real / 2 : a.n_real);
    a.nt_out = ctx->gemm_nt_out >= 0 ? ctx->gemm_nt_out : ((int64_t)a.M * out_cols * 2 > ((int64_t)32 << 20));
    return launch_gemm(a, epi, s);
}

// ------------------------------------------------------------------------------------------ schedule
extern "C" int32_t aur_tome_r(int32_t height, int32_t width, int32_t patch, double ratio, int32_t layers) {
    // aurora.py:895 - same operation order in doubles: W*H / patch**2 * (1 - ratio) / L, then int()
    const double v = (double)width * (double)height / (double)(patch * patch) * (1.0 - ratio) / (double)layers;
    return (int32_t)v;
}
extern "C" int32_t aur_tokens_at_layer(int32_t t0, int32_t r, int32_t layer) {
    int t = t0;
    for (int l = 0; l < layer; ++l) {
        int rl = r < (t - 1) / 2 ? r : (t - 1) / 2;      // tome.py:45
        if (rl > 0) t -= rl;
    }
    return t;
}
extern "C" const char* aur_version(void) { return "aurora_hip 0.1 (gfx950)"; }
extern "C" const char* aur_last_error(const aur_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// ------------------------------------------------------------------------------------------ layout
struct Carver {
    int64_t off = 0;
    char* base;
    explicit Carver(char* b) : base(b) {}
    template <typename T>
    T* take(int64_t n) {
        T* p = base ? (T*)(base + off) : nullptr;
        off = rup64(off + n * (int64_t)sizeof(T), 256);
        return p;
    }
};

static void derive(aur_ctx* c) {
    const aur_config& g = c->cfg;
    c->v_hd = g.vit_hidden / g.vit_heads;
    c->v_hd_pad = rup(c->v_hd, 32);
    c->v_kblk = c->v_hd_pad / 32;
    c->v_vd16 = c->v_hd / 16;
    c->v_qcols = rup(g.vit_heads * c->v_hd_pad, 64);
    c->v_qkv_npad = rup(2 * c->v_qcols + g.vit_heads * c->v_hd, 256);
    c->v_dpad = rup(g.vit_hidden, 256);
    c->v_mlp_pad = rup(g.vit_mlp, 256);
    const int gw = g.vit_image / g.vit_patch;
    c->v_npatch = gw * gw;
    c->v_t0 = c->v_npatch + 1;
    c->v_t0pad = rup(c->v_t0, 32);
    const int gn = (g.vit_native_image > 0 ? g.vit_native_image : g.vit_image) / g.vit_patch;    // grid of the checkpoint's position table
    c->v_native_npatch = gn * gn;
    c->v_kpad = rup(g.vit_channels * g.vit_patch * g.vit_patch, 64);
    c->l_hd = g.llm_hidden / g.llm_heads;
    c->l_kblk = c->l_hd / 32;
    c->l_vd16 = c->l_hd / 16;
    c->l_qkv_npad = rup(3 * g.llm_hidden, 256);
    c->l_gu_npad = rup(2 * g.llm_mlp, 256);
    c->l_dpad = rup(g.llm_hidden, 256);
    c->l_vocab_pad = rup(g.llm_vocab, 256);
    c->l_max_pages = (g.max_ctx + g.page_tokens - 1) / g.page_tokens;
    c->l_ctx_pad = c->l_max_pages * g.page_tokens;
    c->l_page_halves = (int64_t)2 * g.llm_heads * g.page_tokens * c->l_hd;
    c->nbanks = g.num_banks == 2 ? 2 : 1;
    c->skinny_variant = g.max_batch > 32 ? 1 : 0;        // a function of the engine's capacity, never of the live batch
    // QKV and gate/up (N = 12288 / 22016: several tiles per CU share x) gain from x-through-LDS at EVERY capacity - 22.3-22.9 -> 20.4-20.8 us
    // and 33.3-33.8 -> 31.6-31.9 us at 1, 4 and 8 rows (round 4, tools/microbench.py --batch 1 / 4 / 8) - while o / down do not (9.1 /
    // 19.0-19.5 us either way or worse).  configs[3]'s per-GPU engine (8 slots): 5.80 -> 6.01 captions/s with this and the GEMM changes.
    c->skinny_variant_wide = 1;
    c->kv_seqs = g.max_batch + (g.spare_slots > 0 ? g.spare_slots : 0);     // KV sequences per bank: decode slots + spare prefill targets
    c->l_layer_halves = c->l_page_halves * c->l_max_pages * c->kv_seqs * c->nbanks;
    // decode attention: one wave per (sequence, head, split).  Enough splits to put ~512 waves on the GPU for small batches,
    // as few as possible (1) once the batch supplies them - every extra split re-reads q, writes a partial and lengthens
    // the combine (measured at a 2.2k context: B=64 344 us with 2 splits vs 362 with 10; B=1 15.1 us with 13 vs 24.8 with 38).
    // A function of the engine's capacity only, never of the live batch: results stay batch-invariant per engine.
    int want = (512 + g.llm_heads * g.max_batch - 1) / (g.llm_heads * g.max_batch);
    want = want < 1 ? 1 : (want > 16 ? 16 : want);          // 1 split (>= 512 sequence-heads): 333.6 us vs 333.4 us with 2 at 64 x 32, and no combine
    c->pps = (c->l_max_pages + want - 1) / want;
    if (c->pps < 1) c->pps = 1;
    c->nsplit = (c->l_max_pages + c->pps - 1) / c->pps;
}

static int64_t vit_page_halves(const aur_ctx* c, int t_pad) { return (int64_t)c->cfg.vit_heads * t_pad * (c->v_hd_pad + c->v_hd); }

static int64_t carve(aur_ctx* c, char* base) {
    const aur_config& g = c->cfg;
    Carver k(base);
    const int64_t F = g.max_frames, TP = c->v_t0pad, D = g.vit_hidden;
    c->w_col = k.take<half_t>(F * c->v_npatch * c->v_kpad);
    c->w_patch = k.take<half_t>(F * c->v_npatch * D);
    c->w_xa = k.take<half_t>(F * TP * D);
    c->w_xb = k.take<half_t>(F * TP * D);
    c->w_xn = k.take<half_t>(F * TP * D);
    c->w_qf = k.take<half_t>(F * g.vit_heads * TP * c->v_hd_pad);
    c->w_kv = k.take<half_t>(F * vit_page_halves(c, (int)TP));
    c->w_attn = k.take<half_t>(F * TP * D);
    c->w_h = k.take<half_t>(F * TP * g.vit_mlp);
    c->w_metric = k.take<float>(F * c->v_t0 * c->v_hd);
    c->w_mhat = k.take<float>(F * tome_mfrag_floats(c->v_t0, c->v_hd));          // fp32 MFMA operand blocks (tome.hip)
    const int64_t ta = (c->v_t0 + 1) / 2;
    c->w_nmax = k.take<float>(F * ta);
    c->w_nidx = k.take<int32_t>(F * ta);
    c->w_unm = k.take<int32_t>(F * ta);
    c->w_src = k.take<int32_t>(F * ta);
    c->w_dst = k.take<int32_t>(F * ta);
    c->w_sza = k.take<float>(F * TP);
    c->w_szb = k.take<float>(F * TP);
    // llm
    const int64_t B = g.max_batch, d = g.llm_hidden;
    const int64_t LP = (int64_t)c->l_ctx_pad * B;          // batched prefill: up to max_batch sequences in one pass
    c->l_xn = k.take<half_t>(LP * d);
    c->l_qf = k.take<half_t>(LP * d);
    c->l_attn = k.take<half_t>(LP * d);
    c->l_h = k.take<half_t>(LP * g.llm_mlp);
    c->l_p1 = k.take<half_t>(LP * d);
    c->l_rope = k.take<float2>((int64_t)c->l_ctx_pad * (c->l_hd / 2));
    const int64_t Bp = rup((int)B, 16);                    // x-fragment buffers hold whole groups of 16 rows
    for (int bk = 0; bk < 2; ++bk) {
        aur_ctx::Bank& K = c->banks[bk];
        K.d_x = k.take<half_t>(Bp * d);                    // residual stream    (x-fragment form)
        K.s_ssq_mlp = k.take<unsigned long long>(AUR_SSQ_SLOTS * AUR_MAX_BATCH);      // sum(x^2) per row after the MLP / embedding (2^-28 fixed point)
        K.s_ssq_attn = k.take<unsigned long long>(AUR_SSQ_SLOTS * AUR_MAX_BATCH);     // sum(x^2) per row after the attention residual
        K.d_logits = k.take<float>(B * g.llm_vocab);
        K.s_pos = k.take<int32_t>(B);
        K.s_ids = k.take<int32_t>(B * g.max_new_tokens);
        K.s_len = k.take<int32_t>(B);
        K.s_fin = k.take<int32_t>(B);
        K.s_samp = k.take<aur_sampling>(B);
        K.s_rules = k.take<aur_logit_rules>(B);
        K.lr_cnt = k.take<int32_t>(B);
    }
    c->d_q = k.take<half_t>(B * d);
    c->d_attn = k.take<half_t>(Bp * d);                    // attention output  (x-fragment form)
    c->d_h = k.take<half_t>(Bp * g.llm_mlp);               // SiLU(gate)*up     (x-fragment form)
    c->d_scr = k.take<half_t>(AUR_MAX_BATCH * 16384);                 // scratch x-fragments for aur_linear_skinny
    c->d_part_row = k.take<float>((int64_t)4 * (c->l_dpad / 16) * (Bp / 16) * 256);          // [4 k splits][tiles][column groups][64 lanes][4]
    c->d_row_cnt = k.take<int>(c->l_dpad / 16);
    c->d_stamp = k.take<unsigned long long>(8 + 2 * AUR_STAMP_RING);
    c->d_part_o = k.take<float>(B * g.llm_heads * c->l_max_pages * c->l_hd);     // room for pages_per_split = 1
    c->d_part_ml = k.take<float>(B * g.llm_heads * c->l_max_pages * 2);
    c->s_ptab = k.take<int32_t>(2 * (int64_t)c->kv_seqs * c->l_max_pages);
    for (int bk = 0; bk < 2; ++bk) c->banks[bk].ptab = c->s_ptab ? c->s_ptab + (int64_t)bk * c->kv_seqs * c->l_max_pages : nullptr;
    return k.off;
}

// ------------------------------------------------------------------------------------------ lifecycle
extern "C" int aur_create(const aur_config* cfg, aur_ctx** out) {
    if (!cfg || !out) return aur_fail(nullptr, AUR_ERR_ARG, "aur_create: null argument");
    const aur_config& g = *cfg;
    if (g.vit_hidden % 64 || g.vit_mlp % 64 || g.vit_hidden % g.vit_heads || (g.vit_hidden / g.vit_heads) % 16)
        return aur_fail(nullptr, AUR_ERR_ARG, "vit dims: hidden/mlp must be multiples of 64, head_dim a multiple of 16");
    if (g.llm_hidden % 128 || g.llm_mlp % 128 || g.llm_hidden % g.llm_heads || (g.llm_hidden / g.llm_heads) % 32)
        return aur_fail(nullptr, AUR_ERR_ARG, "llm dims: hidden/mlp must be multiples of 128, head_dim a multiple of 32");
    if (g.max_batch < 1 || g.max_batch > AUR_MAX_BATCH) return aur_fail(nullptr, AUR_ERR_ARG, "max_batch must be in [1, %d]", AUR_MAX_BATCH);
    if (g.page_tokens != 64) return aur_fail(nullptr, AUR_ERR_ARG, "page_tokens must be 64 (the decode attention's page pipeline is written for 64-token pages)");
    if (g.vit_image % g.vit_patch) return aur_fail(nullptr, AUR_ERR_ARG, "image size must be a multiple of the patch size");
    {   // the ToMe step's limits (tome.hip launch_tome_step), checked here so that an out-of-range ViT fails at create time, not at the first encode
        const int64_t t0 = (int64_t)(g.vit_image / g.vit_patch) * (g.vit_image / g.vit_patch) + 1;
        if (g.vit_hidden > 2048) return aur_fail(nullptr, AUR_ERR_ARG, "vit_hidden %d exceeds 2048 (token-merge kernel: one row of at most 2048 features per wave)", g.vit_hidden);
        if (g.vit_hidden / g.vit_heads > 128) return aur_fail(nullptr, AUR_ERR_ARG, "vit head_dim %d exceeds 128 (token-merge metric: at most 128 channels)", g.vit_hidden / g.vit_heads);
        if ((t0 + 1) / 2 > 4096) return aur_fail(nullptr, AUR_ERR_ARG, "vit_image %d / patch %d gives %lld tokens per frame; the token-merge select kernel ranks at most 4096 = ceil(t / 2) of them", g.vit_image, g.vit_patch, (long long)t0);
    }
    if (g.vit_native_image < 0 || g.vit_native_image > g.vit_image || g.vit_native_image % g.vit_patch)
        return aur_fail(nullptr, AUR_ERR_ARG, "vit_native_image must be 0 or a multiple of the patch size <= vit_image");
    {
        hipError_t e;
        if ((e = gemm_init()) != hipSuccess || (e = attn_init()) != hipSuccess || (e = tome_init()) != hipSuccess ||
            (e = skinny_init()) != hipSuccess || (e = gemm256_init()) != hipSuccess || (e = sample_init()) != hipSuccess)
            return aur_fail(nullptr, AUR_ERR_HIP, "kernel attribute init failed (is a gfx950 GPU visible?): %s", hipGetErrorString(e));
    }
    if (g.proj_depth < 0 || g.proj_depth > 8) return aur_fail(nullptr, AUR_ERR_ARG, "proj_depth must be 0 (= 2) or 1 .. 8");
    if (g.proj_act != 0 && g.proj_act != AUR_ACT_QUICK_GELU && g.proj_act != AUR_ACT_GELU && g.proj_act != AUR_ACT_SILU && g.proj_act != AUR_ACT_RELU &&
        g.proj_act != AUR_ACT_GELU_TANH)
        return aur_fail(nullptr, AUR_ERR_UNSUPPORTED, "proj_act %d is not one of AUR_ACT_*", g.proj_act);
    aur_ctx* c = new aur_ctx();
    c->cfg = g;
    c->p_depth = g.proj_depth > 0 ? g.proj_depth : 2;
    c->p_act = g.proj_act > 0 ? g.proj_act : ACT_GELU;
    derive(c);
    *out = c;
    return AUR_OK;
}

static void drop_graphs(aur_ctx::Bank& K) {
    if (K.graph) (void)hipGraphExecDestroy(K.graph);
    if (K.graph_h) (void)hipGraphExecDestroy(K.graph_h);
    K.graph = K.graph_h = nullptr;
}

extern "C" void aur_destroy(aur_ctx* ctx) {
    if (!ctx) return;
    for (auto& K : ctx->banks) {
        drop_graphs(K);
        if (K.lr_save) (void)hipFree(K.lr_save);
        if (K.s_guid) (void)hipFree(K.s_guid);
        if (K.gd_save) (void)hipFree(K.gd_save);
        if (K.s_stop) (void)hipFree(K.s_stop);
    }
    for (auto& ug : ctx->ugraphs)
        if (ug.exec) (void)hipGraphExecDestroy(ug.exec);
    for (auto& kv : ctx->timers) {
        if (kv.second.e0) (void)hipEventDestroy(kv.second.e0);
        if (kv.second.e1) (void)hipEventDestroy(kv.second.e1);
    }
    for (auto& kv : ctx->kev)
        for (auto& p : kv.ev) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    delete ctx;
}

extern "C" int aur_set_tensor(aur_ctx* ctx, const char* name, const void* dev_ptr, int64_t nbytes) {
    if (!ctx || !name || !dev_ptr) return aur_fail(ctx, AUR_ERR_ARG, "aur_set_tensor: null argument");
    ctx->tensors[name] = Tensor{dev_ptr, nbytes};
    ctx->finalized = false;
    return AUR_OK;
}
extern "C" int64_t aur_workspace_bytes(const aur_ctx* ctx) {
    aur_ctx tmp = *ctx;
    return carve(&tmp, nullptr);
}
extern "C" int64_t aur_kv_pool_bytes(const aur_ctx* ctx) { return ctx->l_layer_halves * ctx->cfg.llm_layers * 2; }
extern "C" int aur_set_workspace(aur_ctx* ctx, void* p, int64_t n) {
    if (n < aur_workspace_bytes(ctx)) return aur_fail(ctx, AUR_ERR_ARG, "workspace too small: %lld < %lld", (long long)n, (long long)aur_workspace_bytes(ctx));
    ctx->ws = (char*)p;
    ctx->ws_bytes = n;
    carve(ctx, ctx->ws);
    ctx->finalized = false;
    if (ctx->d_row_cnt) CK(hipMemset(ctx->d_row_cnt, 0, (size_t)(ctx->l_dpad / 16) * 4));     // split-K arrival counters, likewise
    if (ctx->d_stamp) CK(hipMemset(ctx->d_stamp, 0, (size_t)(8 + 2 * AUR_STAMP_RING) * 8));
    return AUR_OK;
}
extern "C" int aur_set_kv_pool(aur_ctx* ctx, void* p, int64_t n) {
    if (n < aur_kv_pool_bytes(ctx)) return aur_fail(ctx, AUR_ERR_ARG, "kv pool too small");
    ctx->kvpool = (char*)p;
    ctx->kv_bytes = n;
    return AUR_OK;
}

template <typename T>
static bool get(aur_ctx* c, const std::string& name, const T** out, int64_t min_bytes, bool required = true) {
    auto it = c->tensors.find(name);
    if (it == c->tensors.end()) {
        if (required) aur_fail(c, AUR_ERR_STATE, "missing tensor '%s'", name.c_str());
        *out = nullptr;
        return !required;
    }
    if (it->second.bytes < min_bytes) {
        aur_fail(c, AUR_ERR_STATE, "tensor '%s' has %lld bytes, need %lld", name.c_str(), (long long)it->second.bytes, (long long)min_bytes);
        return false;
    }
    *out = (const T*)it->second.p;
    return true;
}

extern "C" int aur_finalize(aur_ctx* ctx, void* stream) {
    NO_CAPTURE("aur_finalize");
    if (!ctx->ws) return aur_fail(ctx, AUR_ERR_STATE, "aur_finalize: workspace not set");
    const aur_config& g = ctx->cfg;
    hipStream_t s = (hipStream_t)stream;
    const bool have_vit = ctx->tensors.count("vit.patch.w") > 0;
    const bool have_llm = ctx->tensors.count("llm.embed") > 0;
    if (have_vit) {
        const int64_t D = g.vit_hidden;
        bool ok = get(ctx, "vit.patch.w", &ctx->v_patch_w, (int64_t)ctx->v_dpad * ctx->v_kpad * 2) &&
                  get(ctx, "vit.cls", &ctx->v_cls, D * 2) && get(ctx, "vit.pos", &ctx->v_pos, (int64_t)(ctx->v_native_npatch + 1) * D * 2) &&
                  get(ctx, "vit.preln.w", &ctx->v_preln_w, D * 4) && get(ctx, "vit.preln.b", &ctx->v_preln_b, D * 4);
        if (!ok) return AUR_ERR_STATE;
        // hidden_states[-2] needs layers 0 .. L-2 only: the last layer's weights are optional
        const int nl = g.vit_layers - 1;
        ctx->vl.assign(nl > 0 ? nl : 0, VitLayerW{});
        for (int l = 0; l < nl; ++l) {
            const std::string p = "vit." + std::to_string(l) + ".";
            VitLayerW& w = ctx->vl[l];
            ok = get(ctx, p + "ln1.w", &w.ln1_w, D * 4) && get(ctx, p + "ln1.b", &w.ln1_b, D * 4) &&
                 get(ctx, p + "ln2.w", &w.ln2_w, D * 4) && get(ctx, p + "ln2.b", &w.ln2_b, D * 4) &&
                 get(ctx, p + "qkv.w", &w.qkv_w, (int64_t)ctx->v_qkv_npad * D * 2) && get(ctx, p + "qkv.b", &w.qkv_b, (int64_t)ctx->v_qkv_npad * 4) &&
                 get(ctx, p + "out.w", &w.out_w, (int64_t)ctx->v_dpad * D * 2) && get(ctx, p + "out.b", &w.out_b, (int64_t)ctx->v_dpad * 4) &&
                 get(ctx, p + "fc1.w", &w.fc1_w, (int64_t)ctx->v_mlp_pad * D * 2) && get(ctx, p + "fc1.b", &w.fc1_b, (int64_t)ctx->v_mlp_pad * 4) &&
                 get(ctx, p + "fc2.w", &w.fc2_w, (int64_t)ctx->v_dpad * g.vit_mlp * 2) && get(ctx, p + "fc2.b", &w.fc2_b, (int64_t)ctx->v_dpad * 4);
            if (!ok) return AUR_ERR_STATE;
        }
    }
    if (have_llm) {
        if (!ctx->kvpool) return aur_fail(ctx, AUR_ERR_STATE, "aur_finalize: kv pool not set");
        const int64_t d = g.llm_hidden;
        bool ok = get(ctx, "llm.embed", &ctx->l_embed, (int64_t)g.llm_vocab * d * 2) &&
                  get(ctx, "llm.lm_head.w", &ctx->l_head_w, (int64_t)ctx->l_vocab_pad * d * 2);
        if (!ok) return AUR_ERR_STATE;
        ctx->ll.assign(g.llm_layers, LlmLayerW{});
        for (int l = 0; l < g.llm_layers; ++l) {
            const std::string p = "llm." + std::to_string(l) + ".";
            LlmLayerW& w = ctx->ll[l];
            ok = get(ctx, p + "qkv.w", &w.qkv_w, (int64_t)ctx->l_qkv_npad * d * 2) && get(ctx, p + "o.w", &w.o_w, (int64_t)ctx->l_dpad * d * 2) &&
                 get(ctx, p + "gateup.w", &w.gateup_w, (int64_t)ctx->l_gu_npad * d * 2) &&
                 get(ctx, p + "down.w", &w.down_w, (int64_t)ctx->l_dpad * g.llm_mlp * 2);
            if (!ok) return AUR_ERR_STATE;
        }
        // projector is part of the language-side prefix path
        ctx->p_w.clear();
        ctx->p_b.clear();
        if (ctx->tensors.count("proj.0.w")) {
            for (int i = 0; i < ctx->p_depth; ++i) {
                const half_t* pw;
                const float* pb;
                const std::string p = "proj." + std::to_string(i) + ".";
                ok = get(ctx, p + "w", &pw, (int64_t)ctx->l_dpad * (i == 0 ? g.vit_hidden : d) * 2) && get(ctx, p + "b", &pb, (int64_t)ctx->l_dpad * 4);
                if (!ok) return AUR_ERR_STATE;
                ctx->p_w.push_back(pw);
                ctx->p_b.push_back(pb);
            }
        }
        // RoPE table (HF linear scaling: position / factor), cos/sin in fp32 like HF
        const int half = ctx->l_hd / 2;
        std::vector<float2> tab((size_t)ctx->l_ctx_pad * half);
        for (int p = 0; p < ctx->l_ctx_pad; ++p)
            for (int i = 0; i < half; ++i) {
                const float inv = 1.0f / powf(g.rope_theta, (float)(2 * i) / (float)ctx->l_hd);
                const float ang = ((float)p / g.rope_factor) * inv;
                tab[(size_t)p * half + i] = make_float2(cosf(ang), sinf(ang));
            }
        CK(hipMemcpyAsync(ctx->l_rope, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice, s));
        std::vector<int32_t> pt((size_t)2 * ctx->kv_seqs * ctx->l_max_pages);
        for (size_t i = 0; i < pt.size(); ++i) pt[i] = (int32_t)i;      // initial allocation: sequence q owns pages [q*max_pages, ...)
        CK(hipMemcpyAsync(ctx->s_ptab, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, s));
        // decode scratch in x-fragment form: lanes of unused batch rows must hold finite values forever
        CK(hipMemsetAsync(ctx->d_attn, 0, (size_t)rup(g.max_batch, 16) * g.llm_hidden * 2, s));
        CK(hipMemsetAsync(ctx->d_h, 0, (size_t)rup(g.max_batch, 16) * g.llm_mlp * 2, s));
        // KV pool: attention reads whole 64-token pages and weights the not-yet-written tail of the last page with p = 0;
        // 0 x (stale bits that decode as NaN / Inf) would poison the output, so the pool starts all-zero and from then on
        // only finite K / V values are ever stored into it.
        CK(hipMemsetAsync(ctx->kvpool, 0, (size_t)ctx->kv_bytes, s));
        CK(hipStreamSynchronize(s));
    }
    if (!have_vit && !have_llm) return aur_fail(ctx, AUR_ERR_STATE, "aur_finalize: no weights were provided");
    ctx->finalized = true;
    return AUR_OK;
}

extern "C" int aur_pack_linear(aur_ctx* ctx, const void* w, int32_t n_src, int32_t k_src, int32_t ld_src,
                               const int32_t* row_map, int32_t npad, int32_t kpad, void* out, void* stream) {
    if (npad % 16 || kpad % 32 || !w || !out) return aur_fail(ctx, AUR_ERR_ARG, "aur_pack_linear: npad %% 16, kpad %% 32 required");
    CK(launch_pack_weight((const half_t*)w, n_src, k_src, ld_src, row_map, npad, kpad, (half_t*)out, (hipStream_t)stream));
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ profiling
// roctx ranges per stage (tracing): `rocprofv3 --marker-trace --kernel-trace` then groups the launches of a stage under
// its name instead of by kernel name only.  The marker library is looked up at run time (librocprofiler-sdk-roctx.so, else libroctx64.so)
// when AURORA_ROCTX=1 is set - the product library has no link-time dependency on a profiler, and without the variable a range costs one
// predictable branch.  Ranges bracket the host-side ENQUEUE of a stage (what roctx measures); the device time is in the kernel trace.
// A ctx is driven by ONE host thread at a time (include/aurora_hip.h: "calls on one ctx are not re-entrant"): the open range of a stage name is state of the ctx,
// keyed by (name, stream), so the same stage enqueued on two streams by that thread (a front end beside the decode) keeps two ranges apart.
// Ranges are START / STOP ranges with ids (not the push / pop stack): an entry point that fails between stage_begin and stage_end
// (every CK() is an early return) leaves ONE unclosed range, which the next stage_begin of that name closes - the nesting of later
// stages cannot be skewed.
struct Roctx {
    uint64_t (*start)(const char*) = nullptr;
    void (*stop)(uint64_t) = nullptr;
    Roctx() {
        const char* on = getenv("AURORA_ROCTX");
        if (!on || on[0] != '1') return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        start = (uint64_t (*)(const char*))dlsym(h, "roctxRangeStartA");
        stop = (void (*)(uint64_t))dlsym(h, "roctxRangeStop");
        if (!start || !stop) start = nullptr, stop = nullptr;
    }
};
static const Roctx& roctx() {
    static Roctx r;          // read-only after its thread-safe initialisation
    return r;
}
static std::string range_key(const char* name, hipStream_t s) {
    char buf[96];
    snprintf(buf, sizeof buf, "%s@%p", name, (void*)s);
    return buf;
}
static void stage_begin(aur_ctx* c, const char* name, hipStream_t s) {
    if (roctx().start) {
        StageTimer& tr = c->timers[range_key(name, s)];
        if (tr.range_open) roctx().stop(tr.range_id);       // left open by a call that failed mid-stage
        tr.range_id = roctx().start(name);
        tr.range_open = true;
    }
    if (!c->prof || c->capturing) return;
    StageTimer& t = c->timers[name];
    if (!t.e0) {
        (void)hipEventCreate(&t.e0);
        (void)hipEventCreate(&t.e1);
    }
    if (t.open) {      // fold the previous interval
        (void)hipEventSynchronize(t.e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, t.e0, t.e1);
        t.ms += ms;
        t.open = false;
    }
    (void)hipEventRecord(t.e0, s);
}
static void stage_end(aur_ctx* c, const char* name, hipStream_t s) {
    if (roctx().stop) {
        StageTimer& tr = c->timers[range_key(name, s)];
        if (tr.range_open) roctx().stop(tr.range_id);
        tr.range_open = false;
    }
    if (!c->prof || c->capturing) return;
    StageTimer& t = c->timers[name];
    (void)hipEventRecord(t.e1, s);
    t.open = true;
    t.launches++;
}
extern "C" int aur_profile_enable(aur_ctx* ctx, int32_t on) {
    NO_CAPTURE("aur_profile_enable");
    ctx->prof = on != 0;
    for (auto& kv : ctx->timers) {
        kv.second.ms = 0;
        kv.second.launches = 0;
        kv.second.open = false;
    }
    for (auto& kv : ctx->kev) {
        kv.used = 0;
        kv.ms = 0;
        kv.n = 0;
    }
    return AUR_OK;
}
static void kev_fold(aur_ctx::KernelEvents& k) {
    for (size_t i = 0; i < k.used; ++i) {
        (void)hipEventSynchronize(k.ev[i].second);
        float ms = 0;
        if (hipEventElapsedTime(&ms, k.ev[i].first, k.ev[i].second) == hipSuccess) {
            k.ms += ms;
            k.n++;
        }
    }
    k.used = 0;
}
static void kev_begin(aur_ctx::KernelEvents& k, hipStream_t s) {
    if (k.used == k.ev.size()) {
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        k.ev.push_back({a, b});
    }
    (void)hipEventRecord(k.ev[k.used].first, s);
}
static void kev_end(aur_ctx::KernelEvents& k, hipStream_t s) {
    (void)hipEventRecord(k.ev[k.used].second, s);
    k.used++;
    if (k.used >= 4096) kev_fold(k);
}
extern "C" int aur_profile_read(aur_ctx* ctx, const char* stage, double* ms_out, int64_t* launches_out) {
    const int which = !strcmp(stage, "decode_attn") ? 0 : !strcmp(stage, "decode_gemm_gateup") ? 1 : !strcmp(stage, "vit_tome") ? 2 : !strcmp(stage, "first_token") ? 3 : -1;
    if (which >= 0) {
        kev_fold(ctx->kev[which]);
        if (ms_out) *ms_out = ctx->kev[which].ms;
        if (launches_out) *launches_out = ctx->kev[which].n;
        return AUR_OK;
    }
    auto it = ctx->timers.find(stage);
    if (it == ctx->timers.end()) {
        if (ms_out) *ms_out = 0;
        if (launches_out) *launches_out = 0;
        return AUR_OK;
    }
    StageTimer& t = it->second;
    if (t.open) {
        (void)hipEventSynchronize(t.e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, t.e0, t.e1);
        t.ms += ms;
        t.open = false;
    }
    if (ms_out) *ms_out = t.ms;
    if (launches_out) *launches_out = t.launches;
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ vision
static KvLayout vit_kv(const aur_ctx* c, int t_pad) {
    KvLayout L;
    L.base = c->w_kv;
    L.page_table = nullptr;
    L.max_pages = 0;
    L.page_tokens = t_pad;
    L.heads = c->cfg.vit_heads;
    L.kblk = c->v_kblk;
    L.vd16 = c->v_vd16;
    L.page_halves = vit_page_halves(c, t_pad);
    L.v_off = (int64_t)c->cfg.vit_heads * t_pad * c->v_hd_pad;
    return L;
}

// One encoder layer on padded state x [F][t_pad][D] (in place for r == 0; x_out otherwise).  Returns via
// *t_out the new token count; result lives in *x_res / *size_res (one of the two ping-pong buffers).
static int vit_layer_run(aur_ctx* ctx, int l, int F, int t, int r, half_t* x, const float* size, half_t* x_alt, float* size_alt,
                         half_t** x_res, const float** size_res, int* t_out, hipStream_t s, bool want_metric = false,
                         int32_t* map = nullptr, int map_n = 0) {
    const aur_config& g = ctx->cfg;
    const VitLayerW& w = ctx->vl[l];
    const int D = g.vit_hidden, t_pad = rup(t, 32), M = F * t_pad;
    CK(launch_layernorm(x, D, w.ln1_w, w.ln1_b, 1e-5f, M, D, ctx->w_xn, D, s));          // aurora.py:735 (eps: :709)
    GemmArgs q{};
    q.A = ctx->w_xn; q.lda = D; q.W = w.qkv_w; q.bias = w.qkv_b; q.M = M; q.Npad = ctx->v_qkv_npad; q.K = D;
    q.rows_per_seq = t_pad; q.q_cols = ctx->v_qcols; q.k_cols = ctx->v_qcols; q.hd = ctx->v_hd; q.Qf = ctx->w_qf;
    q.kv = vit_kv(ctx, t_pad); q.rope = nullptr; q.pos0 = 0; q.seq0 = 0; q.tag = GT_VIT_QKV;
    CK(ctx_gemm(ctx, q, EPI_QKV, s));                                                        // aurora.py:634-636
    AttnArgs at{};
    at.Qf = ctx->w_qf; at.kv = q.kv; at.seq0 = 0; at.nseq = F; at.heads = g.vit_heads; at.rows_per_seq = t_pad; at.t = t;
    at.causal = 0; at.scale = 1.0f / sqrtf((float)ctx->v_hd); at.O = ctx->w_attn; at.ldo = D; at.hd = ctx->v_hd;
    CK(launch_attention(at, s));                                                           // aurora.py:647-697
    GemmArgs o{};
    o.A = ctx->w_attn; o.lda = D; o.W = w.out_w; o.bias = w.out_b; o.M = M; o.Npad = ctx->v_dpad; o.K = D;
    o.C = x; o.ldc = D; o.resid = x; o.ldr = D; o.n_real = D; o.act = ACT_NONE; o.tag = GT_VIT_OUT;
    CK(ctx_gemm(ctx, o, EPI_ROW, s));                                                        // aurora.py:699, 743
    int rl = r < (t - 1) / 2 ? r : (t - 1) / 2;                                            // tome.py:45
    half_t* xc = x;
    const float* sc = size;
    int t2 = t;
    bool ln2_done = false;
    if (rl > 0) {
        TomeArgs ta{};
        t2 = t - rl;
        ta.frames = F; ta.t = t; ta.t_pad = t_pad; ta.r = rl; ta.c = ctx->v_hd; ta.d = D;
        ta.kv = &q.kv; ta.metric_out = want_metric ? ctx->w_metric : nullptr;             // metric = mean_h K, aurora.py:639
        ta.x = x; ta.size = size; ta.t_out_pad = rup(t2, 32); ta.x_out = x_alt; ta.size_out = size_alt;
        ta.node_max = ctx->w_nmax; ta.node_idx = ctx->w_nidx; ta.unm = ctx->w_unm; ta.src = ctx->w_src; ta.dst = ctx->w_dst;
        ta.mhat = ctx->w_mhat;
        // LayerNorm 2 (aurora.py:750, eps :711) of the merged rows comes out of the merge launch (tome.hip: bitwise norm_kernel<false>)
        ln2_done = ctx->tome_fused_ln && (D & 7) == 0;
        if (ln2_done) { ta.ln_w = w.ln2_w; ta.ln_b = w.ln2_b; ta.ln_eps = 1e-5f; ta.ln_out = ctx->w_xn; }
        if (ctx->prof) kev_begin(ctx->kev[2], s);
        CK(launch_tome_step(ta, s));                                                       // aurora.py:746-747
        if (ctx->prof) kev_end(ctx->kev[2], s);
        // the merge map follows the step in a launch of its own: w_unm / w_src / w_dst are the next layer's too (merge_map.py)
        if (map) CK(launch_tome_map(map, F, map_n, t, rl, ctx->w_unm, ctx->w_src, ctx->w_dst, s));
        xc = x_alt;
        sc = size_alt;
    }
    const int t2_pad = rup(t2, 32), M2 = F * t2_pad;
    if (!ln2_done) CK(launch_layernorm(xc, D, w.ln2_w, w.ln2_b, 1e-5f, M2, D, ctx->w_xn, D, s));         // aurora.py:750
    GemmArgs f1{};
    f1.A = ctx->w_xn; f1.lda = D; f1.W = w.fc1_w; f1.bias = w.fc1_b; f1.M = M2; f1.Npad = ctx->v_mlp_pad; f1.K = D;
    f1.C = ctx->w_h; f1.ldc = g.vit_mlp; f1.n_real = g.vit_mlp; f1.act = g.vit_act == AUR_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU; f1.tag = GT_VIT_FC1;
    CK(ctx_gemm(ctx, f1, EPI_ROW, s));
    GemmArgs f2{};
    f2.A = ctx->w_h; f2.lda = g.vit_mlp; f2.W = w.fc2_w; f2.bias = w.fc2_b; f2.M = M2; f2.Npad = ctx->v_dpad; f2.K = g.vit_mlp;
    f2.C = xc; f2.ldc = D; f2.resid = xc; f2.ldr = D; f2.n_real = D; f2.act = ACT_NONE; f2.tag = GT_VIT_FC2;
    CK(ctx_gemm(ctx, f2, EPI_ROW, s));                                                       // aurora.py:751-752
    *x_res = xc;
    *size_res = sc;
    *t_out = t2;
    return AUR_OK;
}

extern "C" int aur_vit_pos_interp(aur_ctx* ctx, int32_t height, int32_t width, void* pos_out, void* stream) {
    if (!ctx->finalized || ctx->vl.empty()) return aur_fail(ctx, AUR_ERR_STATE, "aur_vit_pos_interp: vision weights not finalized");
    const aur_config& g = ctx->cfg;
    const int gh = height / g.vit_patch, gw = width / g.vit_patch;
    if (gh < 1 || gw < 1 || !pos_out) return aur_fail(ctx, AUR_ERR_ARG, "aur_vit_pos_interp: input %dx%d, patch %d", height, width, g.vit_patch);
    int n = 1;
    while ((n + 1) * (n + 1) <= ctx->v_native_npatch) ++n;          // aurora.py:929-931: the native grid is square
    if (n * n != ctx->v_native_npatch) return aur_fail(ctx, AUR_ERR_STATE, "aur_vit_pos_interp: the native table holds %d patch rows, not a square", ctx->v_native_npatch);
    CK(launch_pos_interp(ctx->v_pos, n, gh, gw, g.vit_hidden, (half_t*)pos_out, (hipStream_t)stream));
    return AUR_OK;
}

extern "C" int aur_vit_encode_map(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t height, int32_t width,
                                  const void* pos_emb, int32_t r, void* out_tokens, int32_t* map_out, float* size_out,
                                  int32_t* n_kept_out, void* stream) {
    if (!ctx->finalized || ctx->vl.empty()) return aur_fail(ctx, AUR_ERR_STATE, "aur_vit_encode: vision weights not finalized");
    const aur_config& g = ctx->cfg;
    if (frames < 1 || frames > g.max_frames) return aur_fail(ctx, AUR_ERR_ARG, "frames %d outside [1, %d]", frames, g.max_frames);
    if (r < 0) return aur_fail(ctx, AUR_ERR_ARG, "r must be >= 0");
    const int gh = height / g.vit_patch, gw = width / g.vit_patch, npatch = gh * gw, t0 = npatch + 1;
    if (gh < 1 || gw < 1 || t0 > ctx->v_t0)
        return aur_fail(ctx, AUR_ERR_ARG, "input %dx%d gives %d tokens per frame; this ctx holds up to %d (vit_image %d)", height, width,
                        t0, ctx->v_t0, g.vit_image);
    const bool native = gh == gw && npatch == ctx->v_native_npatch;
    if (!pos_emb && !native) return aur_fail(ctx, AUR_ERR_ARG, "a %dx%d patch grid needs an interpolated position table (pos_emb)", gh, gw);
    hipStream_t s = (hipStream_t)stream;
    stage_begin(ctx, "vit", s);
    const int D = g.vit_hidden;
    CK(launch_im2col((const half_t*)pixels, frames, g.vit_channels, height, width, g.vit_patch, ctx->v_kpad, ctx->w_col, s));
    GemmArgs pe{};
    pe.A = ctx->w_col; pe.lda = ctx->v_kpad; pe.W = ctx->v_patch_w; pe.bias = nullptr; pe.M = frames * npatch;
    pe.Npad = ctx->v_dpad; pe.K = ctx->v_kpad; pe.C = ctx->w_patch; pe.ldc = D; pe.n_real = D; pe.act = ACT_NONE;
    CK(ctx_gemm(ctx, pe, EPI_ROW, s));
    CK(launch_vit_assemble(ctx->w_patch, ctx->v_cls, pos_emb ? (const half_t*)pos_emb : ctx->v_pos, ctx->v_preln_w, ctx->v_preln_b,
                           g.vit_ln_eps, frames, npatch, D, rup(t0, 32), ctx->w_xa, s));
    half_t* x = ctx->w_xa;
    half_t* x_alt = ctx->w_xb;
    const float* size = nullptr;          // aurora.py:811: size = None at layer 0
    float* size_alt = ctx->w_sza;
    int t = t0;
    // the merge map is built in map_out itself: 1 + p, one rewrite behind every merging layer, the class row taken off at the end
    if (map_out) CK(launch_tome_map_init(map_out, frames, npatch, s));
    for (int l = 0; l < g.vit_layers - 1; ++l) {
        half_t* xr;
        const float* sr;
        int t2;
        int rc = vit_layer_run(ctx, l, frames, t, r, x, size, x_alt, size_alt, &xr, &sr, &t2, s, false, map_out, npatch);
        if (rc) return rc;
        if (xr != x) {           // merged into the alternate buffer: swap ping-pong roles
            x_alt = x;
            x = xr;
            size_alt = (sr == ctx->w_sza) ? ctx->w_szb : ctx->w_sza;
            size = sr;
        }
        t = t2;
    }
    CK(launch_strip_cls(x, frames, t, rup(t, 32), D, (half_t*)out_tokens, s));           // aurora.py:253
    // size stays null when no layer merged (r = 0): the sizes are then written as ones
    if (map_out || size_out) CK(launch_tome_map_finish(map_out, frames, npatch, size, rup(t, 32), t - 1, size_out, s));
    if (n_kept_out) *n_kept_out = t - 1;
    stage_end(ctx, "vit", s);
    return AUR_OK;
}

extern "C" int aur_vit_encode_hw(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t height, int32_t width,
                                 const void* pos_emb, int32_t r, void* out_tokens, int32_t* n_kept_out, void* stream) {
    return aur_vit_encode_map(ctx, pixels, frames, height, width, pos_emb, r, out_tokens, nullptr, nullptr, n_kept_out, stream);
}

extern "C" int aur_vit_encode(aur_ctx* ctx, const void* pixels, int32_t frames, int32_t r, void* out_tokens,
                              int32_t* n_kept_out, void* stream) {
    const int nat = ctx->cfg.vit_native_image > 0 ? ctx->cfg.vit_native_image : ctx->cfg.vit_image;
    return aur_vit_encode_hw(ctx, pixels, frames, nat, nat, nullptr, r, out_tokens, n_kept_out, stream);
}

extern "C" int aur_vit_layer(aur_ctx* ctx, int32_t layer, const void* x, const float* size, int32_t frames, int32_t t,
                             int32_t r, void* x_out, float* size_out, float* metric_out, int32_t* node_idx,
                             int32_t* unm_idx, int32_t* src_idx, int32_t* dst_idx, void* stream) {
    if (!ctx->finalized || layer < 0 || layer >= (int)ctx->vl.size()) return aur_fail(ctx, AUR_ERR_ARG, "aur_vit_layer: bad layer / not finalized");
    if (frames < 1 || frames > ctx->cfg.max_frames || t < 2 || t > ctx->v_t0) return aur_fail(ctx, AUR_ERR_ARG, "aur_vit_layer: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int D = ctx->cfg.vit_hidden, t_pad = rup(t, 32);
    CK(launch_pad_rows((const half_t*)x, size, frames, t, t_pad, D, ctx->w_xa, size ? ctx->w_sza : nullptr, s));
    half_t* xr;
    const float* sr;
    int t2;
    int rc = vit_layer_run(ctx, layer, frames, t, r, ctx->w_xa, size ? ctx->w_sza : nullptr, ctx->w_xb, ctx->w_szb, &xr, &sr, &t2, s, metric_out != nullptr);
    if (rc) return rc;
    CK(launch_unpad_rows(xr, sr, frames, t2, rup(t2, 32), D, (half_t*)x_out, size_out, s));
    const int rl = r < (t - 1) / 2 ? r : (t - 1) / 2;
    if (rl > 0) {
        const int ta = (t + 1) / 2;
        if (metric_out) CK(hipMemcpyAsync(metric_out, ctx->w_metric, (size_t)frames * t * ctx->v_hd * 4, hipMemcpyDeviceToDevice, s));
        if (node_idx) CK(hipMemcpyAsync(node_idx, ctx->w_nidx, (size_t)frames * ta * 4, hipMemcpyDeviceToDevice, s));
        if (unm_idx) CK(hipMemcpyAsync(unm_idx, ctx->w_unm, (size_t)frames * (ta - rl) * 4, hipMemcpyDeviceToDevice, s));
        if (src_idx) CK(hipMemcpyAsync(src_idx, ctx->w_src, (size_t)frames * rl * 4, hipMemcpyDeviceToDevice, s));
        if (dst_idx) CK(hipMemcpyAsync(dst_idx, ctx->w_dst, (size_t)frames * rl * 4, hipMemcpyDeviceToDevice, s));
    } else if (metric_out) {
        KvLayout kv = vit_kv(ctx, t_pad);
        CK(launch_tome_metric(kv, frames, t, ctx->v_hd, metric_out, s));
    }
    return AUR_OK;
}

extern "C" int aur_tome_step(aur_ctx* ctx, const float* metric, const void* x, const float* size, int32_t frames, int32_t t,
                             int32_t c, int32_t d, int32_t r, void* x_out, float* size_out, int32_t* node_idx,
                             int32_t* unm_idx, int32_t* src_idx, int32_t* dst_idx, void* stream) {
    if (!ctx->ws) return aur_fail(ctx, AUR_ERR_STATE, "aur_tome_step: workspace not set");
    if (frames < 1 || t < 1 || c < 1 || (d & 7)) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_step: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int rl = r < (t - 1) / 2 ? r : (t - 1) / 2;
    if (rl <= 0) {      // tome.py:47-48 do_nothing; merge_wavg still materialises size (tome.py:212-213)
        CK(hipMemcpyAsync(x_out, x, (size_t)frames * t * d * 2, hipMemcpyDeviceToDevice, s));
        CK(launch_unpad_rows((const half_t*)x, size, frames, t, t, d, (half_t*)x_out, size_out, s));
        return AUR_OK;
    }
    const int64_t ta = (t + 1) / 2;
    // scratch must fit the ctx workspace regions sized for the configured ViT
    if (c > 128) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_step: at most 128 metric channels (got %d)", c);
    if (ta > 4096) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_step: ceil(t / 2) = %lld exceeds 4096 (the select kernel ranks one frame's A tokens in one workgroup)", (long long)ta);
    if (d > 2048) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_step: d = %d exceeds 2048 (a merge workgroup holds one row of at most 2048 features per wave)", d);
    if ((int64_t)frames * tome_mfrag_floats(t, c) > (int64_t)ctx->cfg.max_frames * tome_mfrag_floats(ctx->v_t0, ctx->v_hd) || (int64_t)frames * ta > (int64_t)ctx->cfg.max_frames * ((ctx->v_t0 + 1) / 2) ||
        (int64_t)frames * rup(t, 32) * d > (int64_t)ctx->cfg.max_frames * ctx->v_t0pad * ctx->cfg.vit_hidden)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_step: problem larger than the workspace configured at aur_create");
    const int t_pad = rup(t, 32), t2 = t - rl, t2_pad = rup(t2, 32);
    CK(launch_pad_rows((const half_t*)x, size, frames, t, t_pad, d, ctx->w_xa, ctx->w_sza, s));
    TomeArgs a{};
    a.frames = frames; a.t = t; a.t_pad = t_pad; a.r = rl; a.c = c; a.d = d; a.metric = metric; a.x = ctx->w_xa;
    a.size = size ? ctx->w_sza : nullptr; a.t_out_pad = t2_pad; a.x_out = ctx->w_xb; a.size_out = ctx->w_szb;
    a.node_max = ctx->w_nmax; a.node_idx = ctx->w_nidx; a.unm = ctx->w_unm; a.src = ctx->w_src; a.dst = ctx->w_dst; a.mhat = ctx->w_mhat;
    CK(launch_tome_step(a, s));
    CK(launch_unpad_rows(ctx->w_xb, ctx->w_szb, frames, t2, t2_pad, d, (half_t*)x_out, size_out, s));
    if (node_idx) CK(hipMemcpyAsync(node_idx, ctx->w_nidx, (size_t)frames * ta * 4, hipMemcpyDeviceToDevice, s));
    if (unm_idx) CK(hipMemcpyAsync(unm_idx, ctx->w_unm, (size_t)frames * (ta - rl) * 4, hipMemcpyDeviceToDevice, s));
    if (src_idx) CK(hipMemcpyAsync(src_idx, ctx->w_src, (size_t)frames * rl * 4, hipMemcpyDeviceToDevice, s));
    if (dst_idx) CK(hipMemcpyAsync(dst_idx, ctx->w_dst, (size_t)frames * rl * 4, hipMemcpyDeviceToDevice, s));
    return AUR_OK;
}

extern "C" int aur_tome_map_rows(aur_ctx* ctx, int32_t* rows_dev, int32_t frames, int32_t n, int32_t t, int32_t r, const int32_t* unm,
                                 const int32_t* src, const int32_t* dst, void* stream) {
    if (!rows_dev || frames < 1 || n < 1 || t < 1) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_map_rows: bad shape (frames %d, n %d, t %d)", frames, n, t);
    if (t > 8192) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_map_rows: t = %d exceeds 8192 (a workgroup holds one frame's row table in LDS)", t);
    if (r < 0 || r > (t - 1) / 2) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_map_rows: r = %d outside [0, (t - 1) / 2 = %d]", r, (t - 1) / 2);
    if (r == 0) return AUR_OK;
    if (!unm || !src || !dst) return aur_fail(ctx, AUR_ERR_ARG, "aur_tome_map_rows: unm / src / dst missing");
    CK(launch_tome_map(rows_dev, frames, n, t, r, unm, src, dst, (hipStream_t)stream));
    return AUR_OK;
}

extern "C" int aur_unmerge_rows(aur_ctx* ctx, const void* tokens, const int32_t* map, int32_t frames, int32_t n, int32_t n_kept, int32_t d,
                                void* out, void* stream) {
    if (!tokens || !map || !out || frames < 1 || n < 1 || n_kept < 1 || d < 8)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_unmerge_rows: bad shape (frames %d, n %d, n_kept %d, d %d)", frames, n, n_kept, d);
    if (d & 7) return aur_fail(ctx, AUR_ERR_ARG, "aur_unmerge_rows: d = %d is not a multiple of 8 (rows move as 16-byte pieces)", d);
    if (((uintptr_t)tokens | (uintptr_t)out) & 15) return aur_fail(ctx, AUR_ERR_ARG, "aur_unmerge_rows: tokens and out must be 16-byte aligned");
    if (((int64_t)frames * n * (d >> 3) + 255) / 256 > 0x7fffffffll) return aur_fail(ctx, AUR_ERR_ARG, "aur_unmerge_rows: too many rows for one launch");
    CK(launch_unmerge_rows((const half_t*)tokens, map, frames, n, n_kept, d, (half_t*)out, (hipStream_t)stream));
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ skinny-GEMM launches
// THE structure rule: which skinny-GEMM structure (kernels.h SkinnyArgs: variant, part, row_cnt, gu_ks, half_grid) a launch of `mode`
// gets on THIS engine - a function of the engine's capacity and its knobs, never of the live batch.  Every SkinnyArgs of the library is
// built here: the decode step's projections (mk_sk_qkv / _row / _gateup under mk_dec_*), the lm_head (mk_lm_head), aur_microbench and
// the parity entries (aur_linear_skinny, aur_decode_proj_rows, aur_attn_decode_rows), which differ only in the buffers they pass.
// tests/skinny_ref.py structure() is the tests' independent statement of the rule.
// ssq_in != nullptr: the RMSNorm folded into W, 1/rms from the rows' sum(x^2).  part / row_cnt: the split-K partials and arrival
// counters an SK_ROW launch may take (ignored by the other modes).
static SkinnyArgs mk_skinny(const aur_ctx* ctx, int mode, const half_t* xf, const half_t* W, int B, int b_lo, int b_hi, int K, int Npad, int n_real,
                            const unsigned long long* ssq_in, unsigned long long* ssq_zero, float* part, int* row_cnt) {
    SkinnyArgs a{};
    a.xf = xf; a.W = W; a.B = B; a.b_lo = b_lo; a.b_hi = b_hi; a.K = K; a.Npad = Npad; a.n_real = n_real; a.mode = mode;
    a.ssq_in = ssq_in; a.norm_eps = ssq_in ? ctx->cfg.llm_rms_eps : 0.f; a.ssq_zero = ssq_zero;
    const bool wide = mode == SK_QKV || mode == SK_SILU_MUL;        // N of several tiles per CU: x through LDS at every capacity (derive)
    a.variant = wide ? ctx->skinny_variant_wide : ctx->skinny_variant;
    if (mode == SK_LOGITS) return a;                                // the lm_head runs outside the step's half grid
    a.half_grid = ctx->decode_half;
    if (mode == SK_ROW) {
        a.part = (K >= ctx->row_split_min_k || ctx->cfg.max_batch > 64) ? part : nullptr;
        a.row_cnt = ctx->fused_reduce ? row_cnt : nullptr;
    }
    if (mode == SK_SILU_MUL) a.gu_ks = ctx->cfg.max_batch > 64 ? 1 : 2;
    return a;
}

// ------------------------------------------------------------------------------------------ generic ops
static_assert(AUR_GEMM_SILU_MUL == ACT_SILU_MUL && AUR_ACT_SILU == ACT_SILU && AUR_ACT_RELU == ACT_RELU && AUR_ACT_GELU_TANH == ACT_GELU_TANH, "public activation codes");
static_assert(AUR_GEMM_TAG_OTHER == GT_OTHER && AUR_GEMM_TAG_VIT_OUT == GT_VIT_OUT && AUR_GEMM_TAG_VIT_FC1 == GT_VIT_FC1 && AUR_GEMM_TAG_VIT_FC2 == GT_VIT_FC2 &&
              AUR_GEMM_TAG_LLM_O == GT_LLM_O && AUR_GEMM_TAG_LLM_GATEUP == GT_LLM_GATEUP && AUR_GEMM_TAG_LLM_DOWN == GT_LLM_DOWN, "public GEMM tags");
// One EPI_ROW launch on caller buffers: every rule the two tile kernels and their epilogues assume is checked HERE, before anything is
// launched (aur_gemm_rows in include/aurora_hip.h says where each one comes from); aur_linear is the same launch with lda = k,
// ldc = ldr = n, no tag and no row map.
static int gemm_rows(aur_ctx* ctx, const char* who, const void* a, int m, int k, int lda, const void* w_packed, int npad, int n, const float* bias,
                     int act, int tag, const void* resid, int ldr, const int32_t* out_rows, void* c, int ldc, hipStream_t s) {
    if (!ctx) return AUR_ERR_ARG;
    if (!a || !w_packed || !c) return aur_fail(ctx, AUR_ERR_ARG, "%s: null argument", who);
    if (m < 1 || k < 64 || (k & 63) || npad < 128 || (npad & 127) || n < 4 || n > npad || (n & 3))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: need m >= 1, k a positive multiple of 64, npad a positive multiple of 128, n %% 4 == 0, 4 <= n <= npad (got %d, %d, %d, %d)", who, m, k, npad, n);
    if (act != ACT_NONE && act != ACT_QUICK_GELU && act != ACT_GELU && act != ACT_SILU_MUL && act != ACT_SILU && act != ACT_RELU && act != ACT_GELU_TANH)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: act %d is neither 0, an AUR_ACT_* nor AUR_GEMM_SILU_MUL", who, act);
    if (tag != GT_OTHER && tag != GT_VIT_OUT && tag != GT_VIT_FC1 && tag != GT_VIT_FC2 && tag != GT_LLM_O && tag != GT_LLM_GATEUP && tag != GT_LLM_DOWN)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: tag %d is not an AUR_GEMM_TAG_* of a row-major projection", who, tag);
    if (lda < k || (lda & 7) || ((uintptr_t)a & 15) || ((uintptr_t)w_packed & 15))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: need lda >= k, lda %% 8 == 0, a and w_packed 16-byte aligned (lda %d, k %d)", who, lda, k);
    const bool mul = act == ACT_SILU_MUL;
    const int stored = mul ? n / 2 : n;
    if (ldc < stored || (ldc & (mul ? 1 : 3)) || ((uintptr_t)c & 15))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: need ldc >= %d stored columns, ldc %% %d == 0, c 16-byte aligned (ldc %d)", who, stored, mul ? 2 : 4, ldc);
    if (resid) {
        if (mul) return aur_fail(ctx, AUR_ERR_ARG, "%s: the gate-times-up mode takes no residual", who);
        if (ldr < n || (ldr & 3) || ((uintptr_t)resid & 15)) return aur_fail(ctx, AUR_ERR_ARG, "%s: need ldr >= n, ldr %% 4 == 0, resid 16-byte aligned (ldr %d, n %d)", who, ldr, n);
        if (resid == c && (ldr != ldc || out_rows)) return aur_fail(ctx, AUR_ERR_ARG, "%s: a residual read in place needs ldr == ldc and no row map", who);
    }
    GemmArgs g{};
    g.A = (const half_t*)a; g.lda = lda; g.W = (const half_t*)w_packed; g.bias = bias; g.M = m; g.Npad = npad; g.K = k;
    g.C = (half_t*)c; g.ldc = ldc; g.resid = (const half_t*)resid; g.ldr = ldr; g.n_real = n; g.out_rows = out_rows;
    g.act = act; g.tag = tag;
    CK(ctx_gemm(ctx, g, EPI_ROW, s));
    return AUR_OK;
}
extern "C" int aur_linear(aur_ctx* ctx, const void* a, int32_t m, int32_t k, const void* w_packed, int32_t npad, int32_t n,
                          const float* bias, int32_t act, const void* resid, void* c, void* stream) {
    const int ga = act == AUR_ACT_GELU ? ACT_GELU : act == AUR_ACT_QUICK_GELU ? ACT_QUICK_GELU : ACT_NONE;
    return gemm_rows(ctx, "aur_linear", a, m, k, k, w_packed, npad, n, bias, ga, GT_OTHER, resid, n, nullptr, c, n, (hipStream_t)stream);
}
extern "C" int aur_gemm_rows(aur_ctx* ctx, const void* a, int32_t m, int32_t k, int32_t lda, const void* w_packed, int32_t npad, int32_t n,
                             const float* bias, int32_t act, int32_t tag, const void* resid, int32_t ldr, const int32_t* out_rows_dev, void* c,
                             int32_t ldc, void* stream) {
    return gemm_rows(ctx, "aur_gemm_rows", a, m, k, lda, w_packed, npad, n, bias, act, tag, resid, ldr, out_rows_dev, c, ldc, (hipStream_t)stream);
}
extern "C" int aur_linear_skinny(aur_ctx* ctx, const void* a, int32_t m, int32_t k, const void* w_packed, int32_t npad,
                                 int32_t n, float* out, void* stream) {
    if (m < 1 || m > AUR_MAX_BATCH || (k & 127) || k > 16384 || (npad & 31) || n < 1 || n > npad)       // any n: a ragged row end is stored column by column
        return aur_fail(ctx, AUR_ERR_ARG, "aur_linear_skinny: need m <= %d, k %% 128 == 0, k <= 16384, 1 <= n <= npad", AUR_MAX_BATCH);
    if (!ctx->ws) return aur_fail(ctx, AUR_ERR_STATE, "aur_linear_skinny: workspace not set");
    hipStream_t st = (hipStream_t)stream;
    CK(hipMemsetAsync(ctx->d_scr, 0, (size_t)AUR_MAX_BATCH * 16384 * 2, st));
    CK(launch_xfrag_pack((const half_t*)a, k, m, k, ctx->d_scr, st));
    SkinnyArgs s = mk_skinny(ctx, SK_LOGITS, ctx->d_scr, (const half_t*)w_packed, m, 0, m, k, npad, n, nullptr, nullptr, nullptr, nullptr);
    s.out32 = out;
    CK(launch_skinny(s, st));
    return AUR_OK;
}
extern "C" int aur_layernorm(aur_ctx* ctx, const void* x, int32_t rows, int32_t d, const float* w, const float* b, float eps,
                             void* y, void* stream) {
    CK(launch_layernorm((const half_t*)x, d, w, b, eps, rows, d, (half_t*)y, d, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_rmsnorm(aur_ctx* ctx, const void* x, int32_t rows, int32_t d, const float* w, float eps, void* y, void* stream) {
    CK(launch_rmsnorm((const half_t*)x, d, w, eps, rows, d, (half_t*)y, d, (hipStream_t)stream));
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ projector + splice
// seq_len < 0: the strided form (aur_project_splice_var) - `ntext` is the capacity of the text arrays, entries with text_rows < 0 are
// skipped, and no padding row is cleared here (the variable-length prefill clears rows [len, stride) itself).
static int project_splice(aur_ctx* ctx, const void* vis, int32_t nvis, const int32_t* vis_rows, const int32_t* text_ids,
                          const int32_t* text_rows, int32_t ntext, int32_t seq_len, void* embeds, void* stream) {
    const aur_config& g = ctx->cfg;
    hipStream_t s = (hipStream_t)stream;
    stage_begin(ctx, "project", s);
    const int d = g.llm_hidden, lp = rup(seq_len, 32);
    if (seq_len > 0 && lp > seq_len) CK(hipMemsetAsync((half_t*)embeds + (int64_t)seq_len * d, 0, (size_t)(lp - seq_len) * d * 2, s));
    if (nvis > 0) {
        // modeling_projector.py:20-33: Linear, then (act, Linear) x (depth - 1); the activation rides in the producing GEMM's epilogue and
        // the LAST Linear writes straight into the spliced rows.  Intermediates ping-pong between l_p1 and l_xn (front-end scratch, free
        // until the prefill that follows on this stream).
        const half_t* in = (const half_t*)vis;
        int K = g.vit_hidden;
        for (int i = 0; i < ctx->p_depth; ++i) {
            const bool last = i == ctx->p_depth - 1;
            half_t* out = last ? (half_t*)embeds : ((i & 1) ? ctx->l_xn : ctx->l_p1);
            GemmArgs a{};
            a.A = in; a.lda = K; a.W = ctx->p_w[i]; a.bias = ctx->p_b[i]; a.M = nvis; a.Npad = ctx->l_dpad; a.K = K;
            a.C = out; a.ldc = d; a.n_real = d; a.act = last ? ACT_NONE : ctx->p_act; a.out_rows = last ? vis_rows : nullptr;
            CK(ctx_gemm(ctx, a, EPI_ROW, s));
            in = out;
            K = d;
        }
    }
    CK(launch_embed_rows(ctx->l_embed, d, text_ids, text_rows, ntext, (half_t*)embeds, d, s));   // utils.py:214-216
    stage_end(ctx, "project", s);
    return AUR_OK;
}
extern "C" int aur_project_splice(aur_ctx* ctx, const void* vis, int32_t nvis, const int32_t* vis_rows, const int32_t* text_ids,
                                  const int32_t* text_rows, int32_t ntext, int32_t seq_len, void* embeds, void* stream) {
    if (!ctx->finalized || ctx->p_w.empty()) return aur_fail(ctx, AUR_ERR_STATE, "aur_project_splice: projector weights not finalized");
    const aur_config& g = ctx->cfg;
    if (seq_len < 1 || seq_len > g.max_ctx || nvis + ntext != seq_len) return aur_fail(ctx, AUR_ERR_ARG, "aur_project_splice: seq_len %d (nvis %d + ntext %d), max_ctx %d", seq_len, nvis, ntext, g.max_ctx);
    return project_splice(ctx, vis, nvis, vis_rows, text_ids, text_rows, ntext, seq_len, embeds, stream);
}
extern "C" int aur_project_splice_var(aur_ctx* ctx, const void* vis, int32_t nvis, const int32_t* vis_rows, const int32_t* text_ids,
                                      const int32_t* text_rows, int32_t ntext_cap, int32_t stride, void* embeds, void* stream) {
    if (!ctx->finalized || ctx->p_w.empty()) return aur_fail(ctx, AUR_ERR_STATE, "aur_project_splice_var: projector weights not finalized");
    if (stride < 32 || stride % 32 || stride > ctx->l_ctx_pad)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_project_splice_var: stride %d is not a multiple of 32 within the %d positions of a sequence's KV pages", stride, ctx->l_ctx_pad);
    if (nvis < 0 || ntext_cap < 0 || nvis > stride || ntext_cap > stride || !embeds || (nvis > 0 && (!vis || !vis_rows)) || (ntext_cap > 0 && (!text_ids || !text_rows)))
        return aur_fail(ctx, AUR_ERR_ARG, "aur_project_splice_var: nvis %d / ntext_cap %d outside [0, stride %d], or a null array", nvis, ntext_cap, stride);
    return project_splice(ctx, vis, nvis, vis_rows, text_ids, text_rows, ntext_cap, -1, embeds, stream);
}

// ------------------------------------------------------------------------------------------ language model
static KvLayout llm_kv(const aur_ctx* c, int layer) {
    KvLayout L;
    L.base = (half_t*)c->kvpool + (int64_t)layer * c->l_layer_halves;
    L.page_table = c->bank().ptab;
    L.max_pages = c->l_max_pages;
    L.page_tokens = c->cfg.page_tokens;
    L.heads = c->cfg.llm_heads;
    L.kblk = c->l_kblk;
    L.vd16 = c->l_vd16;
    L.page_halves = c->l_page_halves;
    L.v_off = c->l_page_halves / 2;
    return L;
}

// ---- one builder per decode launch: the caller passes the buffers that differ, the structure comes from mk_skinny.  The decode step
// (mk_dec_*, also timed by aur_microbench) passes the bank's buffers, the parity entries the caller's scratch.
static SkinnyArgs mk_sk_qkv(const aur_ctx* ctx, int l, const half_t* xf, const half_t* W, int B, int K, const float2* rope, const int32_t* pos,
                            const unsigned long long* ssq_in, unsigned long long* ssq_zero) {
    const int d = ctx->cfg.llm_hidden;
    SkinnyArgs q = mk_skinny(ctx, SK_QKV, xf, W, B, 0, B, K, ctx->l_qkv_npad, 3 * d, ssq_in, ssq_zero, nullptr, nullptr);
    q.q_cols = d; q.k_cols = d; q.hd = ctx->l_hd; q.qbuf = ctx->d_q; q.kv = llm_kv(ctx, l); q.rope = rope; q.pos = pos; q.seq_ids = nullptr;
    return q;
}
// residual projection (o, down): xres += W x, sum(xres^2) added to ssq_out
static SkinnyArgs mk_sk_row(const aur_ctx* ctx, const half_t* xf, const half_t* W, half_t* xres, unsigned long long* ssq_out, float* part, int* row_cnt,
                            int B, int b_lo, int b_hi, int K, int Npad, int n_real) {
    SkinnyArgs a = mk_skinny(ctx, SK_ROW, xf, W, B, b_lo, b_hi, K, Npad, n_real, nullptr, nullptr, part, row_cnt);
    a.xres = xres; a.ssq_out = ssq_out;
    return a;
}
// gate/up: out_f = SiLU(gate) * up, n_real / 2 columns in x-fragment form
static SkinnyArgs mk_sk_gateup(const aur_ctx* ctx, const half_t* xf, const half_t* W, half_t* out_f, int B, int b_lo, int b_hi, int K, int Npad,
                               int n_real, const unsigned long long* ssq_in, unsigned long long* ssq_zero) {
    SkinnyArgs a = mk_skinny(ctx, SK_SILU_MUL, xf, W, B, b_lo, b_hi, K, Npad, n_real, ssq_in, ssq_zero, nullptr, nullptr);
    a.out_f = out_f; a.out_k32 = n_real / 64;
    return a;
}
// the lm_head on batch columns [b_lo, b_hi) of B: the final RMSNorm is folded into its weight, 1/rms from ssq_in
static SkinnyArgs mk_lm_head(const aur_ctx* ctx, const half_t* xf, const unsigned long long* ssq_in, float* out32, int B, int b_lo, int b_hi) {
    SkinnyArgs h = mk_skinny(ctx, SK_LOGITS, xf, ctx->l_head_w, B, b_lo, b_hi, ctx->cfg.llm_hidden, ctx->l_vocab_pad, ctx->cfg.llm_vocab, ssq_in, nullptr,
                             nullptr, nullptr);
    h.out32 = out32;
    return h;
}

static SkinnyArgs mk_dec_qkv(aur_ctx* ctx, int l) {
    const aur_ctx::Bank& K = ctx->bank();
    return mk_sk_qkv(ctx, l, K.d_x, ctx->ll[l].qkv_w, K.batch, ctx->cfg.llm_hidden, ctx->l_rope, K.s_pos, K.s_ssq_mlp, K.s_ssq_attn);
}
static DecAttnArgs mk_dec_attn(aur_ctx* ctx, int l) {
    const aur_config& g = ctx->cfg;
    DecAttnArgs at{};
    at.qbuf = ctx->d_q; at.kv = llm_kv(ctx, l); at.pos = ctx->bank().s_pos; at.seq_ids = nullptr; at.B = ctx->bank().batch; at.heads = g.llm_heads;
    at.hd = ctx->l_hd; at.nsplit = ctx->nsplit; at.pages_per_split = ctx->pps; at.scale = 1.0f / sqrtf((float)ctx->l_hd);
    at.part_o = ctx->d_part_o; at.part_ml = ctx->d_part_ml; at.out_f = ctx->d_attn; at.out_k32 = g.llm_hidden / 32;
    // engines whose capacity alone gives one attention workgroup per CU and still split the context (8-15 slots of 32 heads): the splits of a
    // (sequence, head) are the waves of one workgroup and meet in LDS - bitwise the two-launch result, one launch per layer less
    at.local_splits = (g.max_batch * g.llm_heads >= gemm256_grid_cap() /* one attention workgroup per CU */ && (ctx->nsplit == 2 || ctx->nsplit == 4) && ctx->l_hd == 128 && ctx->attn_local) ? ctx->nsplit : 0;
    return at;
}
static SkinnyArgs mk_dec_o(aur_ctx* ctx, int l) {
    const aur_ctx::Bank& K = ctx->bank();
    const int d = ctx->cfg.llm_hidden;
    return mk_sk_row(ctx, ctx->d_attn, ctx->ll[l].o_w, K.d_x, K.s_ssq_attn, ctx->d_part_row, ctx->d_row_cnt, K.batch, 0, K.batch, d, ctx->l_dpad, d);
}
static SkinnyArgs mk_dec_gateup(aur_ctx* ctx, int l) {
    const aur_ctx::Bank& K = ctx->bank();
    return mk_sk_gateup(ctx, K.d_x, ctx->ll[l].gateup_w, ctx->d_h, K.batch, 0, K.batch, ctx->cfg.llm_hidden, ctx->l_gu_npad, 2 * ctx->cfg.llm_mlp,
                        K.s_ssq_attn, K.s_ssq_mlp);
}
static SkinnyArgs mk_dec_down(aur_ctx* ctx, int l) {
    const aur_ctx::Bank& K = ctx->bank();
    return mk_sk_row(ctx, ctx->d_h, ctx->ll[l].down_w, K.d_x, K.s_ssq_mlp, ctx->d_part_row, ctx->d_row_cnt, K.batch, 0, K.batch, ctx->cfg.llm_mlp,
                     ctx->l_dpad, ctx->cfg.llm_hidden);
}

// ---- attention over the prompt during decode: the recorder's launch for layer l of the decode step
static bool attn_map_layer(const aur_ctx::Bank& K, int l) { return l < 64 && ((K.am_mask >> l) & 1); }
static AttnMapArgs mk_attn_map(const aur_ctx* ctx, int l, const int32_t* pos, int B, int window, float* score, float* ml, float* out) {
    AttnMapArgs a{};
    a.qbuf = ctx->d_q; a.kv = llm_kv(ctx, l); a.pos = pos; a.B = B; a.heads = ctx->cfg.llm_heads; a.scale = 1.0f / sqrtf((float)ctx->l_hd);
    a.window = window; a.score = score; a.page_ml = ml; a.s_len = nullptr; a.s_fin = nullptr; a.max_new = 1; a.out = out;
    a.weight = 1.0f / (float)ctx->cfg.llm_heads; a.first = 1;
    return a;
}
static AttnMapArgs mk_dec_attn_map(const aur_ctx* ctx, int l) {
    const aur_ctx::Bank& K = ctx->bank();
    AttnMapArgs a = mk_attn_map(ctx, l, K.s_pos, K.batch, K.am_window, K.am_score, K.am_ml, K.am);
    a.s_len = K.s_len; a.s_fin = K.s_fin; a.max_new = K.max_new;
    a.weight = 1.0f / (float)(ctx->cfg.llm_heads * K.am_nlayers);
    a.first = (K.am_mask & ((1ull << l) - 1)) == 0;
    return a;
}

// slots [b0, b0 + nb) of bank K hold no log-probability record and no attention record: wherever their s_len is zeroed
static int slot_records_clear(aur_ctx* ctx, const aur_ctx::Bank& K, int b0, int nb, hipStream_t s) {
    if (K.lp_len) CK(launch_token_logprob_clear(b0, nb, K.max_new, K.lp_top_n, K.lp_len, K.lp, K.lp_top_id, K.lp_top_lp, s));
    // and no attention record (aur_attn_map_enable): their rows are zeros, a fill node like the s_len memsets beside every call of this
    if (K.am) CK(hipMemsetAsync(K.am + (int64_t)b0 * K.max_new * K.am_window, 0, (size_t)nb * K.max_new * K.am_window * 4, s));
    return AUR_OK;
}

extern "C" int aur_begin_batch(aur_ctx* ctx, int32_t batch, int32_t max_new_tokens, int32_t eos_id, void* stream) {
    NO_CAPTURE("aur_begin_batch");
    if (!ctx->finalized || ctx->ll.empty()) return aur_fail(ctx, AUR_ERR_STATE, "aur_begin_batch: language weights not finalized");
    const aur_config& g = ctx->cfg;
    if (batch < 1 || batch > g.max_batch) return aur_fail(ctx, AUR_ERR_ARG, "batch %d outside [1, %d]", batch, g.max_batch);
    if (max_new_tokens < 1 || max_new_tokens > g.max_new_tokens) return aur_fail(ctx, AUR_ERR_ARG, "max_new_tokens %d outside [1, %d]", max_new_tokens, g.max_new_tokens);
    hipStream_t s = (hipStream_t)stream;
    aur_ctx::Bank& K = ctx->bank();
    if ((K.graph || K.graph_h) && (K.max_new != max_new_tokens || K.eos != eos_id || K.graph_batch != batch)) {
        // eos / max_new / batch are by-value kernel arguments frozen inside the captured graph
        CK(hipStreamSynchronize(s));
        drop_graphs(K);
    }
    K.batch = batch; K.max_new = max_new_tokens; K.eos = eos_id;
    CK(hipMemsetAsync(K.s_len, 0, (size_t)g.max_batch * 4, s));
    CK(hipMemsetAsync(K.s_fin, 0, (size_t)g.max_batch * 4, s));
    CK(hipMemsetAsync(K.s_pos, 0, (size_t)g.max_batch * 4, s));
    CK(hipMemsetAsync(K.s_samp, 0, (size_t)g.max_batch * sizeof(aur_sampling), s));      // every slot greedy until aur_slot_sampling says otherwise
    CK(hipMemsetAsync(K.s_rules, 0, (size_t)g.max_batch * sizeof(aur_logit_rules), s));  // every slot neutral until aur_slot_logit_rules says otherwise
    if (K.s_stop) CK(hipMemsetAsync(K.s_stop, 0, (size_t)g.max_batch * sizeof(aur_stop_rules), s));   // every slot without a stop request until aur_slot_stop says otherwise
    if (K.s_guid) CK(hipMemsetAsync(K.s_guid, 0, (size_t)g.max_batch * sizeof(aur_guidance), s));     // every slot unguided until aur_slot_guidance says otherwise
    CK(hipMemsetAsync(K.s_ids, 0, (size_t)g.max_batch * g.max_new_tokens * 4, s));
    const size_t bp = (size_t)rup(g.max_batch, 16);       // unused fragment lanes must hold finite values
    CK(hipMemsetAsync(K.d_x, 0, bp * g.llm_hidden * 2, s));          // bank-owned buffers only: the other bank may be decoding
    CK(hipMemsetAsync(K.s_ssq_mlp, 0, AUR_SSQ_SLOTS * AUR_MAX_BATCH * 8, s));
    CK(hipMemsetAsync(K.s_ssq_attn, 0, AUR_SSQ_SLOTS * AUR_MAX_BATCH * 8, s));
    return slot_records_clear(ctx, K, 0, g.max_batch, s);
}

// logits for batch columns [b0, b0 + nb) from the residual rows in d_x (x-fragment form; final RMSNorm folded into the
// lm_head weights, 1/rms from s_ssq_mlp), then greedy bookkeeping + next-token embedding
static int lm_head_and_advance(aur_ctx* ctx, int b0, int nb, int advance, int set_pos, hipStream_t s, const int32_t* set_pos_lens = nullptr,
                               int len_cap = 0) {
    const aur_config& g = ctx->cfg;
    const aur_ctx::Bank& K = ctx->bank();
    CK(launch_skinny(mk_lm_head(ctx, K.d_x, K.s_ssq_mlp, K.d_logits, K.batch, b0, b0 + nb), s));
    // guidance: a leader's row becomes the contrast of its own and its partner's for the pick alone, ahead of the logit rules (transformers' order)
    if (ctx->guidance) CK(launch_guidance_apply(K.d_logits, b0, nb, g.llm_vocab, g.max_batch, K.s_guid, K.gd_save, s));
    // logit rules: the affected entries of the rows are rewritten for the pick alone; behind it the rows are the model's again
    if (ctx->logit_rules)
        CK(launch_logit_rules_apply(K.d_logits, b0, nb, g.llm_vocab, K.s_rules, K.s_ids, K.max_new, K.s_len, K.eos, K.lr_save, K.lr_cnt, s));
    if (ctx->sampling)
        CK(launch_sample_advance(K.d_logits, b0, nb, g.llm_vocab, K.s_samp, ctx->l_embed, g.llm_hidden, K.eos, K.max_new, K.s_ids, K.s_len,
                                 K.s_fin, K.s_pos, K.d_x, K.s_ssq_mlp, advance, set_pos, s, set_pos_lens, len_cap, ctx->sample_stage));
    else
        CK(launch_argmax_advance(K.d_logits, b0, nb, g.llm_vocab, ctx->l_embed, g.llm_hidden, K.eos, K.max_new, K.s_ids, K.s_len,
                                 K.s_fin, K.s_pos, K.d_x, K.s_ssq_mlp, advance, set_pos, s, set_pos_lens, len_cap));
    if (ctx->logit_rules) CK(launch_logit_rules_restore(K.d_logits, b0, nb, g.llm_vocab, K.max_new, K.lr_save, K.lr_cnt, s));
    if (ctx->guidance) CK(launch_guidance_restore(K.d_logits, b0, nb, g.llm_vocab, K.s_guid, K.gd_save, s));
    // the log-probability of what was just picked, under the row it was picked from: a launch of its own behind the pick, which stays as it is
    if (K.lp_len)
        CK(launch_token_logprob(K.d_logits, b0, nb, g.llm_vocab, K.s_ids, K.s_len, K.max_new, K.lp_top_n, K.lp_len, K.lp, K.lp_top_id,
                                K.lp_top_lp, s));
    // stop ids / stop strings / budget on the token just appended: sets `finished` of a slot that stops, as the pick does for an EOS
    if (ctx->stop_rules)
        CK(launch_stop_check(b0, nb, K.s_stop, K.s_ids, K.max_new, K.s_len, K.max_new, K.s_fin, ctx->stop_off, ctx->stop_bytes, ctx->stop_vocab,
                             ctx->stop_nbytes, s));
    // guidance: the partner of every leader in the range takes the leader's token, length, finished flag and next input
    if (ctx->guidance)
        CK(launch_guidance_follow(b0, nb, g.llm_vocab, g.max_batch, K.s_guid, ctx->l_embed, g.llm_hidden, K.max_new, K.s_ids, K.s_len, K.s_fin,
                                  K.d_x, K.s_ssq_mlp, s));
    return AUR_OK;
}

// ---- one description of a prefill pass: nseq sequences into KV sequences [seq0, seq0 + nseq), rows in x [nseq * rows_per_seq(), d].
// Three forms, told apart by check_pass and by nothing else:
//   fixed length (aur_llm_prefill*):      lens == nullptr, pos0 == 0 - every sequence holds t rows, rup(t, 32) rows apart.
//   variable (aur_llm_prefill_*_var):     lens != nullptr, pos0 == 0 - t is the row stride, a multiple of 32, and sequence i holds lens[i] rows
//       (device memory, never read on the host: enqueue-only, capturable); the attention kernel reads the lengths, the other kernels of a
//       layer work row by row and need none.
//   extend (aur_llm_extend_*_var):        lens != nullptr, pos0 > 0 - the rows are positions [pos0, pos0 + lens[i]) of sequences whose pages
//       already hold [0, pos0): RoPE and the page write at pos0 + row, queries at pos0 + row over keys [0, pos0 + lens[i]); everything else
//       is the same launch.
struct PrefillPass {
    int seq0, nseq;
    half_t* x;
    int t;                       // seq_len, or the stride
    const int32_t* lens;
    int pos0;
    bool prune_ok;               // false (aur_llm_score_var): the last layer runs over every row - rows in front of the last 128 are read after it
    int rows_per_seq() const { return rup(t, 32); }
    // first element in x of sequence 0's last prompt row: t - 1 by value, or found per sequence from the device lengths (launch_xfrag_norm)
    int64_t last_row(int d) const { return lens ? 0 : (int64_t)(t - 1) * d; }
    // decode position behind the pass, as lm_head_and_advance's (set_pos, lens, len_cap = rows_per_seq()): t, or pos0 + lens[i] on the device
    int set_pos() const { return lens ? pos0 : t; }
    // RoPE position of the first row of the pruned last layer's 128-row tail block: row0 by value, or pos0 + the row0 the query GEMM derives
    // per sequence from the device lengths (GemmArgs.tail_lens)
    int tail_rope_pos0(int row0) const { return lens ? pos0 : pos0 + row0; }
};

// ---- the four GEMMs of a prefill layer on M rows of A (all rows of a pass, or the compact 128-row tails of its last layer)
enum { QKV_Q = 1, QKV_KV = 2, QKV_ALL = 3 };     // column blocks of the packed QKV weight: the Q third's tiles come first
static GemmArgs mk_pre_qkv(const aur_ctx* ctx, int l, const half_t* A, int M, int rows_per_seq, int seq0, int pos0, int cols, int tag) {
    const int d = ctx->cfg.llm_hidden;
    GemmArgs q{};
    q.A = A; q.lda = d; q.W = ctx->ll[l].qkv_w + ((cols & QKV_Q) ? 0 : (int64_t)(d / 16) * (d / 32) * AUR_FRAG_HALVES); q.M = M; q.K = d;
    q.Npad = cols == QKV_ALL ? ctx->l_qkv_npad : cols == QKV_Q ? d : ctx->l_qkv_npad - d;
    q.rows_per_seq = rows_per_seq; q.q_cols = (cols & QKV_Q) ? d : 0; q.k_cols = (cols & QKV_KV) ? d : 0; q.hd = ctx->l_hd; q.Qf = ctx->l_qf;
    q.kv = llm_kv(ctx, l); q.rope = ctx->l_rope; q.pos0 = pos0; q.seq0 = seq0; q.tag = tag;
    return q;
}
static GemmArgs mk_pre_o(const aur_ctx* ctx, int l, const half_t* A, int M, half_t* x, int tag) {
    const int d = ctx->cfg.llm_hidden;
    GemmArgs o{};
    o.A = A; o.lda = d; o.W = ctx->ll[l].o_w; o.M = M; o.Npad = ctx->l_dpad; o.K = d; o.C = x; o.ldc = d; o.resid = x; o.ldr = d;
    o.n_real = d; o.act = ACT_NONE; o.tag = tag;
    return o;
}
static GemmArgs mk_pre_gateup(const aur_ctx* ctx, int l, const half_t* A, int M, half_t* h, int tag) {
    const int d = ctx->cfg.llm_hidden, mlp = ctx->cfg.llm_mlp;
    GemmArgs gu{};
    gu.A = A; gu.lda = d; gu.W = ctx->ll[l].gateup_w; gu.M = M; gu.Npad = ctx->l_gu_npad; gu.K = d; gu.C = h; gu.ldc = mlp;
    gu.n_real = 2 * mlp; gu.act = ACT_SILU_MUL; gu.tag = tag;
    return gu;
}
static GemmArgs mk_pre_down(const aur_ctx* ctx, int l, const half_t* A, int M, half_t* x, int tag) {
    const int d = ctx->cfg.llm_hidden, mlp = ctx->cfg.llm_mlp;
    GemmArgs dn{};
    dn.A = A; dn.lda = mlp; dn.W = ctx->ll[l].down_w; dn.M = M; dn.Npad = ctx->l_dpad; dn.K = mlp; dn.C = x; dn.ldc = d;
    dn.resid = x; dn.ldr = d; dn.n_real = d; dn.act = ACT_NONE; dn.tag = tag;
    return dn;
}
// causal attention of a pass over query rows `rows_per_seq` apart (all rows, or the tail blocks) into O
static AttnArgs mk_pre_attn(const aur_ctx* ctx, int l, const PrefillPass& p, int rows_per_seq, half_t* O) {
    AttnArgs at{};
    at.Qf = ctx->l_qf; at.kv = llm_kv(ctx, l); at.seq0 = p.seq0; at.nseq = p.nseq; at.heads = ctx->cfg.llm_heads; at.rows_per_seq = rows_per_seq;
    at.t = p.t; at.causal = 1; at.scale = 1.0f / sqrtf((float)ctx->l_hd); at.O = O; at.ldo = ctx->cfg.llm_hidden; at.hd = ctx->l_hd;
    at.seq_lens = p.lens; at.len_cap = p.rows_per_seq(); at.q_pos0 = p.pos0; at.len_pos0 = p.pos0;
    return at;
}

// One prefill layer; `which` selects the kernels (bit 0 norm1, 1 qkv, 2 attention, 3 o_proj, 4 norm2, 5 gate/up, 6 down)
// so that aur_microbench can time each of them in isolation.
static int prefill_layer(aur_ctx* ctx, int l, int which, const PrefillPass& p, hipStream_t s) {
    const aur_config& g = ctx->cfg;
    const int d = g.llm_hidden, Mseq = p.rows_per_seq(), M = p.nseq * Mseq;
    if (which & 1) CK(launch_rmsnorm(p.x, d, nullptr, g.llm_rms_eps, M, d, ctx->l_xn, d, s));      // weight folded into qkv.w
    if (which & 2) CK(ctx_gemm(ctx, mk_pre_qkv(ctx, l, ctx->l_xn, M, Mseq, p.seq0, p.pos0, QKV_ALL, GT_LLM_QKV), EPI_QKV, s));
    if (which & 4) CK(launch_attention(mk_pre_attn(ctx, l, p, Mseq, ctx->l_attn), s));
    if (which & 8) CK(ctx_gemm(ctx, mk_pre_o(ctx, l, ctx->l_attn, M, p.x, GT_LLM_O), EPI_ROW, s));
    if (which & 16) CK(launch_rmsnorm(p.x, d, nullptr, g.llm_rms_eps, M, d, ctx->l_xn, d, s));     // weight folded into gateup.w
    if (which & 32) CK(ctx_gemm(ctx, mk_pre_gateup(ctx, l, ctx->l_xn, M, ctx->l_h, GT_LLM_GATEUP), EPI_ROW, s));
    if (which & 64) CK(ctx_gemm(ctx, mk_pre_down(ctx, l, ctx->l_h, M, p.x, GT_LLM_DOWN), EPI_ROW, s));
    return AUR_OK;
}

// The LAST layer of a prefill pass.  After it only each sequence's last hidden state is read (final norm + lm_head for the first token),
// while every later decode step needs the layer's K and V of ALL positions.  So: K / V projection (+ RoPE + page write) over all rows as
// in any layer, and the query projection, attention, o projection, residual and the whole MLP on the LAST 128 ROWS of every sequence only
// (the attention kernel's query block; it holds position seq_len - 1 because rows are padded to a multiple of 32).  HF computes all rows
// and throws them away; every value that is kept is bit-identical here - a GEMM's per-element k order does not depend on M, the tile
// kernels agree bitwise (tests), and the query block sees the same keys.  Saves 83 % of one layer of 32: ~2.5 % of a prefill.
// Scratch: the compact [nseq * 128] activations live in l_h (free until this layer's gate/up), the compact Q fragments in l_qf.
// p.lens != nullptr: the block of sequence i is the 128 rows that end at rup(lens[i], 32) - row0 is per sequence, so the gathers and the
// scatter are one small kernel that reads the lengths, and the query GEMM's RoPE position and the attention's q_pos0 derive from them
// on the device (GemmArgs.tail_lens, AttnArgs.q_tail).  A sequence of <= 128 rows has row0 = 0: its block is the unpruned computation.
// p.pos0 > 0: row0 stays relative to the rows of this pass; positions are pos0 + row as in prefill_layer.
static int prefill_last_layer(aur_ctx* ctx, int l, const PrefillPass& p, hipStream_t s) {
    const aur_config& g = ctx->cfg;
    const int d = g.llm_hidden, nseq = p.nseq, Mseq = p.rows_per_seq(), M = nseq * Mseq, LB = 128, Mc = nseq * LB, row0 = Mseq - LB;
    half_t* const x = p.x;
    half_t* xn_c = ctx->l_h;
    half_t* attn_c = xn_c + (int64_t)Mc * d;
    half_t* x_c = attn_c + (int64_t)Mc * d;
    half_t* h_c = x_c + (int64_t)Mc * d;
    const size_t rowb = (size_t)d * 2;
    CK(launch_rmsnorm(x, d, nullptr, g.llm_rms_eps, M, d, ctx->l_xn, d, s));
    CK(ctx_gemm(ctx, mk_pre_qkv(ctx, l, ctx->l_xn, M, Mseq, p.seq0, p.pos0, QKV_KV, GT_LLM_QKV), EPI_QKV, s));      // K and V of every position
    if (p.lens) CK(launch_tail_rows(ctx->l_xn, x, xn_c, x_c, d, nseq, Mseq, LB, p.lens, 1, s));
    else {
        CK(hipMemcpy2DAsync(xn_c, LB * rowb, ctx->l_xn + (int64_t)row0 * d, Mseq * rowb, LB * rowb, nseq, hipMemcpyDeviceToDevice, s));
        CK(hipMemcpy2DAsync(x_c, LB * rowb, x + (int64_t)row0 * d, Mseq * rowb, LB * rowb, nseq, hipMemcpyDeviceToDevice, s));
    }
    GemmArgs a = mk_pre_qkv(ctx, l, xn_c, Mc, LB, p.seq0, p.tail_rope_pos0(row0), QKV_Q, GT_OTHER);                               // queries of the last block
    a.tail_lens = p.lens; a.tail_cap = Mseq;
    CK(ctx_gemm(ctx, a, EPI_QKV, s));
    AttnArgs at = mk_pre_attn(ctx, l, p, LB, attn_c);
    at.q_pos0 = p.pos0 + row0; at.q_tail = 1;
    CK(launch_attention(at, s));
    CK(ctx_gemm(ctx, mk_pre_o(ctx, l, attn_c, Mc, x_c, GT_OTHER), EPI_ROW, s));
    CK(launch_rmsnorm(x_c, d, nullptr, g.llm_rms_eps, Mc, d, xn_c, d, s));
    CK(ctx_gemm(ctx, mk_pre_gateup(ctx, l, xn_c, Mc, h_c, GT_OTHER), EPI_ROW, s));
    CK(ctx_gemm(ctx, mk_pre_down(ctx, l, h_c, Mc, x_c, GT_OTHER), EPI_ROW, s));
    if (p.lens) CK(launch_tail_rows(nullptr, x, nullptr, x_c, d, nseq, Mseq, LB, p.lens, 0, s));
    else CK(hipMemcpy2DAsync(x + (int64_t)row0 * d, Mseq * rowb, x_c, LB * rowb, LB * rowb, nseq, hipMemcpyDeviceToDevice, s));
    return AUR_OK;
}

// The layer stack of a pass: KV pages and front-end scratch only - no decode state.  Opens the "prefill" stage; the tail closes it.
// p.lens != nullptr: the rows [lens[i], stride) of every sequence are cleared first: whatever the caller left there, they are zeros in
// every layer (an all-zero row stays zero through norm, projections, RoPE and the MLP, and the attention kernel stores zeros for it), and
// so are the K / V written for them.
static int prefill_layers(aur_ctx* ctx, const PrefillPass& p, hipStream_t s) {
    const aur_config& g = ctx->cfg;
    stage_begin(ctx, "prefill", s);
    ctx->last_prefill_len = p.t;
    const int Mseq = p.rows_per_seq();
    if (p.lens) CK(launch_clear_tail_rows(p.x, g.llm_hidden, p.nseq, Mseq, p.lens, s));
    for (int l = 0; l < g.llm_layers; ++l) {
        // the compact scratch of the pruned last layer must fit l_h: nseq * 128 * (3 d + mlp) <= nseq * Mseq * mlp (and LB < Mseq)
        const bool prune = p.prune_ok && ctx->prune_last && l == g.llm_layers - 1 && (int64_t)128 * (3 * g.llm_hidden + g.llm_mlp) <= (int64_t)Mseq * g.llm_mlp && Mseq > 128;
        if (int rc = prune ? prefill_last_layer(ctx, l, p, s) : prefill_layer(ctx, l, 0x7f, p, s)) return rc;
    }
    return AUR_OK;
}
// First tokens of slots [slot0, slot0 + p.nseq) from the last prompt rows of p.x (the final hidden states `prefill_layers` left
// there): residual fragments + sum(x^2) - the lm_head applies the (folded) final RMSNorm itself -, logits, the pick, bookkeeping.
static int prefill_first_tokens(aur_ctx* ctx, int slot0, const PrefillPass& p, const char* stage, hipStream_t s) {
    const aur_config& g = ctx->cfg;
    const int d = g.llm_hidden, Mseq = p.rows_per_seq();
    if (ctx->prof) kev_begin(ctx->kev[3], s);
    CK(launch_xfrag_norm(p.x + p.last_row(d), (int64_t)Mseq * d, nullptr, g.llm_rms_eps, p.nseq, d, slot0, ctx->bank().d_x, ctx->bank().s_ssq_mlp, s, 16,
                         p.lens, Mseq));
    int rc = lm_head_and_advance(ctx, slot0, p.nseq, 0, p.set_pos(), s, p.lens, Mseq);
    if (ctx->prof) kev_end(ctx->kev[3], s);       // closed on the error path too: the event ring and the roctx nesting stay balanced
    stage_end(ctx, stage, s);
    return rc;
}

// page-table rows of sequences [a0, a0 + n) <-> [b0, b0 + n)
__global__ void ptab_swap_kernel(int32_t* __restrict__ pt, int a0, int b0, int n, int max_pages) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * max_pages) return;
    const int j = i / max_pages, p = i - j * max_pages;
    int32_t* pa = pt + (int64_t)(a0 + j) * max_pages + p;
    int32_t* pb = pt + (int64_t)(b0 + j) * max_pages + p;
    const int32_t t = *pa;
    *pa = *pb;
    *pb = t;
}

// ---- the argument checks of every prefill / extend / score entry point, in ONE order: state (finalized, language weights, active batch),
// range (SLOTS: slots [slot0 ..) inside the active batch; SEQS: sequences [seq0 ..) inside the bank's KV sequences; both for a commit,
// whose staged sequences are the slots' own or apart from them), then what the form can see of its rows on the host - FIXED: embeds,
// seq_len >= 1 and seq_len + max_new <= max_ctx; VAR: embeds, lengths, stride; EXTEND: VAR's, then pos0.  The lengths stay on the device.
enum { SLOTS = 1, SEQS = 2 };
enum { FIXED, VAR, EXTEND };
static int check_pass(aur_ctx* ctx, const char* who, int target, int form, int slot0, int seq0, int nseq, const void* embeds, int t, const int32_t* lens,
                      int pos0) {
    const aur_config& g = ctx->cfg;
    const aur_ctx::Bank& K = ctx->bank();
    if (!ctx->finalized || ctx->ll.empty()) return aur_fail(ctx, AUR_ERR_STATE, "%s: language weights not finalized", who);
    if (K.batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "%s: no active batch (aur_begin_batch)", who);
    if ((target & SLOTS) && (nseq < 1 || slot0 < 0 || slot0 + nseq > K.batch))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: slots [%d, %d) outside the batch of %d (aur_begin_batch)", who, slot0, slot0 + nseq, K.batch);
    if ((target & SEQS) && (nseq < 1 || seq0 < 0 || seq0 + nseq > ctx->kv_seqs))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: KV sequences [%d, %d) outside [0, %d) (max_batch + spare_slots)", who, seq0, seq0 + nseq, ctx->kv_seqs);
    if (target == (SLOTS | SEQS) && seq0 != slot0 && seq0 < slot0 + nseq && slot0 < seq0 + nseq)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: slot and sequence ranges overlap", who);
    if (form == FIXED) {
        if (!embeds) return aur_fail(ctx, AUR_ERR_ARG, "%s: null embeds", who);
        if (t < 1 || t + K.max_new > g.max_ctx) return aur_fail(ctx, AUR_ERR_ARG, "%s: seq_len %d + max_new %d exceeds max_ctx %d", who, t, K.max_new, g.max_ctx);
        return AUR_OK;
    }
    // sequences `t` = stride rows apart
    if (!embeds || !lens) return aur_fail(ctx, AUR_ERR_ARG, "%s: null %s", who, !embeds ? "embeds" : "seq_lens_dev");
    if (t < 32 || t % 32) return aur_fail(ctx, AUR_ERR_ARG, "%s: stride %d is not a positive multiple of 32", who, t);
    if (t > ctx->l_ctx_pad) return aur_fail(ctx, AUR_ERR_ARG, "%s: stride %d exceeds the %d positions of a sequence's KV pages", who, t, ctx->l_ctx_pad);
    if (nseq > g.max_batch) return aur_fail(ctx, AUR_ERR_ARG, "%s: %d sequences exceed the front-end scratch of max_batch %d", who, nseq, g.max_batch);
    if (form == VAR) return AUR_OK;
    // the host checks what it can see of a pass that starts behind [0, pos0)
    if (pos0 < g.page_tokens || pos0 % g.page_tokens)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: pos0 %d is not a positive multiple of the %d-token page", who, pos0, g.page_tokens);
    if ((int64_t)pos0 + t > ctx->l_ctx_pad)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: pos0 %d + stride %d exceeds the %d positions of a sequence's KV pages", who, pos0, t, ctx->l_ctx_pad);
    return AUR_OK;
}

// ---- the three tails of a pass.  BATCH: layers + first tokens of slots [slot0 ..) = the pass's sequences.  STAGE: layers only, into any
// KV sequences (normally the spare ones): its own "prefill" timer interval, opened and closed on THIS stream.  COMMIT (decode stream,
// possibly several stages later; timed as "prefill_commit"): slots [slot0 ..) exchange page-table rows with the staged sequences
// [p.seq0 ..), are reset and receive their first tokens from the staged pass's last rows.
enum { BATCH, STAGE, COMMIT };
static int run_pass(aur_ctx* ctx, int kind, const PrefillPass& p, int slot0, hipStream_t s) {
    if (kind != COMMIT) {
        if (int rc = prefill_layers(ctx, p, s)) return rc;
        if (kind == BATCH) return prefill_first_tokens(ctx, slot0, p, "prefill", s);
        stage_end(ctx, "prefill", s);
        return AUR_OK;
    }
    const aur_ctx::Bank& K = ctx->bank();
    const int nseq = p.nseq, seq0 = p.seq0;
    stage_begin(ctx, "prefill_commit", s);
    if (seq0 != slot0) {
        const int n = nseq * ctx->l_max_pages;
        hipLaunchKernelGGL(ptab_swap_kernel, dim3((n + 255) / 256), dim3(256), 0, s, K.ptab, slot0, seq0, nseq, ctx->l_max_pages);
        CK(hipGetLastError());
    }
    CK(hipMemsetAsync(K.s_len + slot0, 0, (size_t)nseq * 4, s));
    CK(hipMemsetAsync(K.s_fin + slot0, 0, (size_t)nseq * 4, s));
    CK(hipMemsetAsync(K.s_pos + slot0, 0, (size_t)nseq * 4, s));
    CK(hipMemsetAsync(K.s_ids + (int64_t)slot0 * K.max_new, 0, (size_t)nseq * K.max_new * 4, s));
    if (int rc = slot_records_clear(ctx, K, slot0, nseq, s)) return rc;
    return prefill_first_tokens(ctx, slot0, p, "prefill_commit", s);
}
// an entry point = its name, its tail, its form: slots [slot0 ..) for BATCH / COMMIT, KV sequences [seq0 ..) for the rows (BATCH: seq0 == slot0)
static int prefill_entry(aur_ctx* ctx, const char* who, int kind, int form, int slot0, int seq0, int nseq, void* embeds, int t, const int32_t* lens,
                         int pos0, void* stream) {
    const int target = kind == BATCH ? SLOTS : kind == STAGE ? SEQS : SLOTS | SEQS;
    if (int rc = check_pass(ctx, who, target, form, slot0, seq0, nseq, embeds, t, lens, pos0)) return rc;
    return run_pass(ctx, kind, PrefillPass{seq0, nseq, (half_t*)embeds, t, lens, pos0, true}, slot0, (hipStream_t)stream);
}

extern "C" int aur_llm_prefill(aur_ctx* ctx, int32_t slot, void* embeds, int32_t seq_len, void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill", BATCH, FIXED, slot, slot, 1, embeds, seq_len, nullptr, 0, stream);
}
extern "C" int aur_llm_prefill_batch(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t seq_len, void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_batch", BATCH, FIXED, slot0, slot0, nseq, embeds, seq_len, nullptr, 0, stream);
}
extern "C" int aur_llm_prefill_stage(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t seq_len, void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_stage", STAGE, FIXED, 0, seq0, nseq, embeds, seq_len, nullptr, 0, stream);
}
extern "C" int aur_llm_prefill_commit(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t seq_len, void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_commit", COMMIT, FIXED, slot0, seq0, nseq, embeds, seq_len, nullptr, 0, stream);
}
extern "C" int aur_llm_prefill_batch_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t stride, const int32_t* seq_lens_dev,
                                         void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_batch_var", BATCH, VAR, slot0, slot0, nseq, embeds, stride, seq_lens_dev, 0, stream);
}
extern "C" int aur_llm_prefill_stage_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t stride, const int32_t* seq_lens_dev,
                                         void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_stage_var", STAGE, VAR, 0, seq0, nseq, embeds, stride, seq_lens_dev, 0, stream);
}
extern "C" int aur_llm_prefill_commit_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t stride,
                                          const int32_t* seq_lens_dev, void* stream) {
    return prefill_entry(ctx, "aur_llm_prefill_commit_var", COMMIT, VAR, slot0, seq0, nseq, embeds, stride, seq_lens_dev, 0, stream);
}
// prefill that starts at a position > 0: the pages already hold [0, pos0) (an earlier prefill, or aur_kv_copy_prefix from a sequence with
// the same leading rows).  The layer stack is the one above with pos0 added to every position.
extern "C" int aur_llm_extend_batch_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride,
                                        const int32_t* new_lens_dev, void* stream) {
    return prefill_entry(ctx, "aur_llm_extend_batch_var", BATCH, EXTEND, slot0, slot0, nseq, embeds, stride, new_lens_dev, pos0, stream);
}
extern "C" int aur_llm_extend_stage_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride,
                                        const int32_t* new_lens_dev, void* stream) {
    return prefill_entry(ctx, "aur_llm_extend_stage_var", STAGE, EXTEND, 0, seq0, nseq, embeds, stride, new_lens_dev, pos0, stream);
}
extern "C" int aur_llm_extend_commit_var(aur_ctx* ctx, int32_t slot0, int32_t nseq, int32_t seq0, void* embeds, int32_t pos0, int32_t stride,
                                         const int32_t* new_lens_dev, void* stream) {
    return prefill_entry(ctx, "aur_llm_extend_commit_var", COMMIT, EXTEND, slot0, seq0, nseq, embeds, stride, new_lens_dev, pos0, stream);
}

// ---- scoring given continuations: the layer stack of a _stage_var pass, then ANY of its rows through the pick path's lm_head and
// score_rows_kernel.  Scratch (the caller's; a function of cfg alone): x fragments of round_up(max_batch, 16) columns | sum(x^2) stripes |
// fp32 logits [max_batch, vocab] | int32 effective targets [max_batch], each region 256-byte aligned.
static int64_t score_xf_bytes(const aur_ctx* c) { return rup64((int64_t)rup(c->cfg.max_batch, 16) * c->cfg.llm_hidden * 2, 256); }
static int64_t score_ssq_bytes() { return (int64_t)AUR_SSQ_SLOTS * AUR_MAX_BATCH * 8; }
static int64_t score_logits_bytes(const aur_ctx* c) { return rup64((int64_t)c->cfg.max_batch * c->cfg.llm_vocab * 4, 256); }
extern "C" int64_t aur_score_scratch_bytes(const aur_ctx* ctx) {
    return score_xf_bytes(ctx) + score_ssq_bytes() + score_logits_bytes(ctx) + rup64((int64_t)ctx->cfg.max_batch * 4, 256);
}

extern "C" int aur_llm_score_var(aur_ctx* ctx, int32_t seq0, int32_t nseq, void* embeds, int32_t pos0, int32_t stride, const int32_t* lens_dev,
                                 const int32_t* score_rows_dev, const int32_t* score_targets_dev, int32_t nscore_cap, void* scratch,
                                 int64_t scratch_bytes, float* logprob_out, int32_t* argmax_out, float* logits_out, void* stream) {
    const char* who = "aur_llm_score_var";
    if (int rc = check_pass(ctx, who, SEQS, pos0 ? EXTEND : VAR, 0, seq0, nseq, embeds, stride, lens_dev, pos0)) return rc;
    if (!score_rows_dev || !score_targets_dev || !logprob_out || !argmax_out || nscore_cap < 1)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: null entry / output array or nscore_cap %d < 1", who, nscore_cap);
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < aur_score_scratch_bytes(ctx))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: scratch must be 256-byte aligned and hold aur_score_scratch_bytes = %lld bytes (got %lld)", who,
                        (long long)aur_score_scratch_bytes(ctx), (long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = run_pass(ctx, STAGE, PrefillPass{seq0, nseq, (half_t*)embeds, stride, lens_dev, pos0, false}, 0, s)) return rc;
    const aur_config& g = ctx->cfg;
    const int B = g.max_batch;
    half_t* xf = (half_t*)scratch;
    unsigned long long* ssq = (unsigned long long*)((char*)scratch + score_xf_bytes(ctx));
    float* lg = (float*)((char*)ssq + score_ssq_bytes());
    int32_t* tgt = (int32_t*)((char*)lg + score_logits_bytes(ctx));
    stage_begin(ctx, "score", s);
    for (int j0 = 0; j0 < nscore_cap; j0 += B) {
        const int n = nscore_cap - j0 < B ? nscore_cap - j0 : B;
        CK(launch_score_gather((const half_t*)embeds, g.llm_hidden, score_rows_dev + j0, score_targets_dev + j0, n, B, nseq, stride, lens_dev, xf,
                               ssq, tgt, s));
        CK(launch_skinny(mk_lm_head(ctx, xf, ssq, lg, B, 0, n), s));       // the pick path's launch, on the caller's scratch and at the engine's capacity
        CK(launch_score_rows(lg, n, g.llm_vocab, tgt, logprob_out + j0, argmax_out + j0, s));
        if (logits_out) CK(hipMemcpyAsync(logits_out + (int64_t)j0 * g.llm_vocab, lg, (size_t)n * g.llm_vocab * 4, hipMemcpyDeviceToDevice, s));
    }
    stage_end(ctx, "score", s);
    return AUR_OK;
}

extern "C" int aur_score_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const int32_t* targets_dev, float* logprob_out,
                              int32_t* argmax_out, void* stream) {
    if (!ctx || !logits || !targets_dev || !logprob_out || !argmax_out) return aur_fail(ctx, AUR_ERR_ARG, "aur_score_rows: null argument");
    if (rows < 1 || vocab < 1) return aur_fail(ctx, AUR_ERR_ARG, "aur_score_rows: rows %d or vocab %d < 1", rows, vocab);
    CK(launch_score_rows(logits, rows, vocab, targets_dev, logprob_out, argmax_out, (hipStream_t)stream));
    return AUR_OK;
}

// K and V of positions [0, tokens) of KV sequence src_seq -> sequences [dst_seq0, dst_seq0 + ndst) of the selected bank, every layer.
// One workgroup per (chunk, page, layer): the page ids come from the page table when the kernel runs (whatever row exchanges earlier
// commits queued on the stream), each 16-byte piece of the source page is loaded once and stored ndst times.  The pages stream through
// (33 pages x 32 layers x 1 MiB per child at 7B, several times the L2s): non-temporal stores, as for the large GEMM outputs.
#define KVC_THREADS 256
#define KVC_PIECES 4                                         /* 16-byte pieces per thread: 16 KiB per workgroup */
__global__ __launch_bounds__(KVC_THREADS) void kv_copy_prefix_kernel(half_t* __restrict__ pool, int64_t layer_halves, int64_t page_halves,
                                                                      const int32_t* __restrict__ ptab, int max_pages, int src_seq, int dst_seq0,
                                                                      int ndst) {
    const int page = blockIdx.y, layer = blockIdx.z;
    const int64_t pieces = page_halves >> 3;                 // a page is whole 1 KiB fragments
    const int64_t p0 = (int64_t)blockIdx.x * (KVC_THREADS * KVC_PIECES) + threadIdx.x;
    half_t* const lbase = pool + (int64_t)layer * layer_halves;
    const h8* src = (const h8*)(lbase + (int64_t)ptab[(int64_t)src_seq * max_pages + page] * page_halves);
    h8 v[KVC_PIECES];
#pragma unroll
    for (int i = 0; i < KVC_PIECES; ++i) {
        const int64_t p = p0 + i * KVC_THREADS;
        if (p < pieces) v[i] = src[p];
    }
    for (int j = 0; j < ndst; ++j) {
        h8* dst = (h8*)(lbase + (int64_t)ptab[(int64_t)(dst_seq0 + j) * max_pages + page] * page_halves);
#pragma unroll
        for (int i = 0; i < KVC_PIECES; ++i) {
            const int64_t p = p0 + i * KVC_THREADS;
            if (p < pieces) __builtin_nontemporal_store(v[i], dst + p);
        }
    }
}
extern "C" int aur_kv_copy_prefix(aur_ctx* ctx, int32_t src_seq, int32_t dst_seq0, int32_t ndst, int32_t tokens, void* stream) {
    if (!ctx->finalized || ctx->ll.empty() || !ctx->kvpool) return aur_fail(ctx, AUR_ERR_STATE, "aur_kv_copy_prefix: language weights not finalized");
    const int pt = ctx->cfg.page_tokens;
    if (tokens < pt || tokens % pt || tokens > ctx->l_ctx_pad)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_kv_copy_prefix: tokens %d is not a positive multiple of the %d-token page within the %d positions of a sequence", tokens, pt, ctx->l_ctx_pad);
    if (src_seq < 0 || src_seq >= ctx->kv_seqs || ndst < 1 || dst_seq0 < 0 || (int64_t)dst_seq0 + ndst > ctx->kv_seqs)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_kv_copy_prefix: source %d or destinations [%d, %d) outside [0, %d) (max_batch + spare_slots)", src_seq, dst_seq0, dst_seq0 + ndst, ctx->kv_seqs);
    if (src_seq >= dst_seq0 && src_seq < dst_seq0 + ndst)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_kv_copy_prefix: source %d inside the destinations [%d, %d)", src_seq, dst_seq0, dst_seq0 + ndst);
    const int64_t pieces = ctx->l_page_halves >> 3;
    const dim3 grid((unsigned)((pieces + KVC_THREADS * KVC_PIECES - 1) / (KVC_THREADS * KVC_PIECES)), tokens / pt, ctx->cfg.llm_layers);
    hipLaunchKernelGGL(kv_copy_prefix_kernel, grid, dim3(KVC_THREADS), 0, (hipStream_t)stream, (half_t*)ctx->kvpool, ctx->l_layer_halves,
                       ctx->l_page_halves, ctx->bank().ptab, ctx->l_max_pages, src_seq, dst_seq0, ndst);
    CK(hipGetLastError());
    return AUR_OK;
}

// ---- the attention kernels alone on caller rows (parity tests): the production fragment writer - the QKV epilogue of the layer - then the
// production attention launch, nothing else.  With x = [q | k | v] and the identity as weight (packed with the loader's row map) the
// fragments hold exactly the caller's q, k, v: fp16 x 1.0 accumulated in fp32 is exact.
extern "C" int aur_attn_rows(aur_ctx* ctx, int32_t layout, const void* x, int32_t nseq, int32_t rows, int32_t kx, const void* w_packed,
                             int32_t npad, const float* bias, int32_t seq0, int32_t rope, int32_t t, const int32_t* lens_dev, int32_t causal,
                             void* out, void* stream) {
    const char* who = "aur_attn_rows";
    if (!ctx || !x || !w_packed || !out) return aur_fail(ctx, AUR_ERR_ARG, "%s: null argument", who);
    if (layout != AUR_ATTN_VIT && layout != AUR_ATTN_LLM) return aur_fail(ctx, AUR_ERR_ARG, "%s: layout %d is neither AUR_ATTN_VIT nor AUR_ATTN_LLM", who, layout);
    if (!ctx->ws) return aur_fail(ctx, AUR_ERR_STATE, "%s: workspace not set", who);
    if (nseq < 1 || rows < 32 || (rows & 31) || kx < 64 || (kx & 63))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: need nseq >= 1, rows a positive multiple of 32, kx a positive multiple of 64 (got %d, %d, %d)", who, nseq, rows, kx);
    if (!lens_dev && (t < 1 || t > rows)) return aur_fail(ctx, AUR_ERR_ARG, "%s: t %d outside [1, rows %d]", who, t, rows);
    const aur_config& g = ctx->cfg;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs q{};
    q.A = (const half_t*)x; q.lda = kx; q.W = (const half_t*)w_packed; q.bias = bias; q.M = nseq * rows; q.Npad = npad; q.K = kx;
    q.rows_per_seq = rows; q.pos0 = 0;
    AttnArgs at{};
    at.nseq = nseq; at.rows_per_seq = rows; at.t = lens_dev ? rows : t; at.causal = causal ? 1 : 0; at.O = (half_t*)out;
    at.seq_lens = lens_dev; at.len_cap = rows;
    if (layout == AUR_ATTN_VIT) {
        if (seq0 != 0 || rope) return aur_fail(ctx, AUR_ERR_ARG, "%s: the ViT layout has no page table and no RoPE (seq0 %d, rope %d)", who, seq0, rope);
        if (nseq > g.max_frames || rows > ctx->v_t0pad) return aur_fail(ctx, AUR_ERR_ARG, "%s: %d sequences of %d rows exceed the workspace (%d frames of %d rows)", who, nseq, rows, g.max_frames, ctx->v_t0pad);
        if (npad != ctx->v_qkv_npad) return aur_fail(ctx, AUR_ERR_ARG, "%s: npad %d is not the ViT's packed QKV width %d", who, npad, ctx->v_qkv_npad);
        q.q_cols = ctx->v_qcols; q.k_cols = ctx->v_qcols; q.hd = ctx->v_hd; q.Qf = ctx->w_qf; q.kv = vit_kv(ctx, rows); q.rope = nullptr; q.seq0 = 0;
        q.tag = GT_VIT_QKV;
        at.heads = g.vit_heads; at.hd = ctx->v_hd;
    } else {
        if (!ctx->finalized || ctx->ll.empty() || !ctx->kvpool) return aur_fail(ctx, AUR_ERR_STATE, "%s: language weights not finalized", who);
        if (seq0 < 0 || seq0 + nseq > ctx->kv_seqs) return aur_fail(ctx, AUR_ERR_ARG, "%s: KV sequences [%d, %d) outside [0, %d)", who, seq0, seq0 + nseq, ctx->kv_seqs);
        if (rows > ctx->l_ctx_pad || (int64_t)nseq * rows > (int64_t)ctx->l_ctx_pad * g.max_batch)
            return aur_fail(ctx, AUR_ERR_ARG, "%s: %d sequences of %d rows exceed the workspace (%d sequences of %d positions)", who, nseq, rows, g.max_batch, ctx->l_ctx_pad);
        if (npad != ctx->l_qkv_npad) return aur_fail(ctx, AUR_ERR_ARG, "%s: npad %d is not the language model's packed QKV width %d", who, npad, ctx->l_qkv_npad);
        q.q_cols = g.llm_hidden; q.k_cols = g.llm_hidden; q.hd = ctx->l_hd; q.Qf = ctx->l_qf; q.kv = llm_kv(ctx, 0);
        q.rope = rope ? ctx->l_rope : nullptr; q.seq0 = seq0; q.tag = GT_LLM_QKV;
        at.heads = g.llm_heads; at.hd = ctx->l_hd;
    }
    at.Qf = q.Qf; at.kv = q.kv; at.seq0 = q.seq0; at.scale = 1.0f / sqrtf((float)at.hd); at.ldo = at.heads * at.hd;
    CK(ctx_gemm(ctx, q, EPI_QKV, s));
    CK(launch_attention(at, s));
    return AUR_OK;
}

// The decode step's attention alone: x fragments of the caller's rows, the step's QKV projection (RoPE, K / V written at pos[b] into layer
// 0 of the selected bank's pages of sequence b), then the decode attention exactly as mk_dec_attn sets it up.  Scratch (the caller's):
// x fragments of round_up(max_batch, 16) rows of kx columns | a (cos, sin) = (1, 0) table for rope == 0 (x * 1 - y * 0 is exact).
__global__ void rope_identity_kernel(float2* __restrict__ tab, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab[i] = make_float2(1.f, 0.f);
}
__global__ void xfrag_unpack_kernel(const half_t* __restrict__ xf, int rows, int d, half_t* __restrict__ out) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x, nchunk = d >> 3;
    if (id >= rows * nchunk) return;
    const int b = id / nchunk, k = (id % nchunk) * 8;
    *(h8*)(out + (int64_t)b * d + k) = *(const h8*)(xf + xfrag_piece(b, k, d >> 5));
}
static int64_t attn_dec_xf_bytes(const aur_ctx* c, int kx) { return rup64((int64_t)rup(c->cfg.max_batch, 16) * kx * 2, 256); }
extern "C" int64_t aur_attn_decode_scratch_bytes(const aur_ctx* ctx, int32_t kx) {
    if (!ctx || kx < 1) return 0;
    return attn_dec_xf_bytes(ctx, kx) + rup64((int64_t)ctx->l_ctx_pad * (ctx->l_hd / 2) * (int64_t)sizeof(float2), 256);
}
extern "C" int aur_attn_decode_rows(aur_ctx* ctx, const void* x, int32_t rows, int32_t kx, const void* w_packed, int32_t npad,
                                    const int32_t* pos_dev, int32_t rope, void* scratch, int64_t scratch_bytes, void* out, void* stream) {
    const char* who = "aur_attn_decode_rows";
    if (!ctx || !x || !w_packed || !pos_dev || !out) return aur_fail(ctx, AUR_ERR_ARG, "%s: null argument", who);
    if (!ctx->finalized || ctx->ll.empty() || !ctx->kvpool) return aur_fail(ctx, AUR_ERR_STATE, "%s: language weights not finalized", who);
    const aur_config& g = ctx->cfg;
    if (rows < 1 || rows > g.max_batch || kx < 128 || (kx & 127)) return aur_fail(ctx, AUR_ERR_ARG, "%s: need 1 <= rows <= max_batch %d and kx a positive multiple of 128 (got %d, %d)", who, g.max_batch, rows, kx);
    if (npad != ctx->l_qkv_npad) return aur_fail(ctx, AUR_ERR_ARG, "%s: npad %d is not the language model's packed QKV width %d", who, npad, ctx->l_qkv_npad);
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < aur_attn_decode_scratch_bytes(ctx, kx))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: scratch must be 256-byte aligned and hold aur_attn_decode_scratch_bytes = %lld bytes (got %lld)", who,
                        (long long)aur_attn_decode_scratch_bytes(ctx, kx), (long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int d = g.llm_hidden;
    half_t* xf = (half_t*)scratch;
    float2* ident = (float2*)((char*)scratch + attn_dec_xf_bytes(ctx, kx));
    CK(hipMemsetAsync(xf, 0, (size_t)rup(rows, 16) * kx * 2, s));          // lanes of unused rows of the last group hold finite values
    CK(launch_xfrag_pack((const half_t*)x, kx, rows, kx, xf, s));
    if (!rope) {
        const int n = ctx->l_ctx_pad * (ctx->l_hd / 2);
        hipLaunchKernelGGL(rope_identity_kernel, dim3((n + 255) / 256), dim3(256), 0, s, ident, n);
        CK(hipGetLastError());
    }
    // mk_dec_qkv's launch without the folded norm, on the caller's rows and positions
    CK(launch_skinny(mk_sk_qkv(ctx, 0, xf, (const half_t*)w_packed, rows, kx, rope ? ctx->l_rope : ident, pos_dev, nullptr, nullptr), s));
    DecAttnArgs at = mk_dec_attn(ctx, 0);
    at.pos = pos_dev; at.B = rows;
    CK(launch_decode_attention(at, s));
    hipLaunchKernelGGL(xfrag_unpack_kernel, dim3((rows * (d >> 3) + 255) / 256), dim3(256), 0, s, ctx->d_attn, rows, d, (half_t*)out);
    CK(hipGetLastError());
    return AUR_OK;
}

// The attention-map kernels alone on caller rows, beside aur_attn_decode_rows: the same QKV launch writes the caller's q into d_q and
// its k at pos_b into the pages, then the recorder runs for one layer and all heads.  Scratch: aur_attn_decode_rows' | scores | page sums.
static int64_t attn_map_score_bytes(const aur_ctx* c, int window) { return rup64((int64_t)c->cfg.max_batch * c->cfg.llm_heads * window * 4, 256); }
static int64_t attn_map_ml_bytes(const aur_ctx* c) { return rup64((int64_t)c->cfg.max_batch * c->cfg.llm_heads * c->l_max_pages * 2 * 4, 256); }
static bool attn_map_window_ok(const aur_ctx* c, int window) {
    return window >= 64 && window % 64 == 0 && window <= c->l_ctx_pad && c->cfg.llm_heads <= AUR_ATTN_MAP_MAX_HEADS;
}
extern "C" int64_t aur_attn_map_rows_scratch_bytes(const aur_ctx* ctx, int32_t kx, int32_t window) {
    if (!ctx || kx < 1 || !attn_map_window_ok(ctx, window)) return 0;
    return aur_attn_decode_scratch_bytes(ctx, kx) + attn_map_score_bytes(ctx, window) + attn_map_ml_bytes(ctx);
}
extern "C" int aur_attn_map_rows(aur_ctx* ctx, const void* x, int32_t rows, int32_t kx, const void* w_packed, int32_t npad, const int32_t* pos_dev,
                                 int32_t rope, void* scratch, int64_t scratch_bytes, int32_t window, float* out, void* stream) {
    const char* who = "aur_attn_map_rows";
    if (!ctx || !x || !w_packed || !pos_dev || !out) return aur_fail(ctx, AUR_ERR_ARG, "%s: null argument", who);
    if (!ctx->finalized || ctx->ll.empty() || !ctx->kvpool) return aur_fail(ctx, AUR_ERR_STATE, "%s: language weights not finalized", who);
    const aur_config& g = ctx->cfg;
    if (rows < 1 || rows > g.max_batch || kx < 128 || (kx & 127)) return aur_fail(ctx, AUR_ERR_ARG, "%s: need 1 <= rows <= max_batch %d and kx a positive multiple of 128 (got %d, %d)", who, g.max_batch, rows, kx);
    if (npad != ctx->l_qkv_npad) return aur_fail(ctx, AUR_ERR_ARG, "%s: npad %d is not the language model's packed QKV width %d", who, npad, ctx->l_qkv_npad);
    if (!attn_map_window_ok(ctx, window)) return aur_fail(ctx, AUR_ERR_ARG, "%s: window %d is not a multiple of 64 in [64, %d] (or more than %d heads)", who, window, ctx->l_ctx_pad, AUR_ATTN_MAP_MAX_HEADS);
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < aur_attn_map_rows_scratch_bytes(ctx, kx, window))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: scratch must be 256-byte aligned and hold aur_attn_map_rows_scratch_bytes = %lld bytes (got %lld)", who,
                        (long long)aur_attn_map_rows_scratch_bytes(ctx, kx, window), (long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    half_t* xf = (half_t*)scratch;
    float2* ident = (float2*)((char*)scratch + attn_dec_xf_bytes(ctx, kx));
    float* score = (float*)((char*)scratch + aur_attn_decode_scratch_bytes(ctx, kx));
    float* ml = (float*)((char*)score + attn_map_score_bytes(ctx, window));
    CK(hipMemsetAsync(xf, 0, (size_t)rup(rows, 16) * kx * 2, s));
    CK(launch_xfrag_pack((const half_t*)x, kx, rows, kx, xf, s));
    if (!rope) {
        const int n = ctx->l_ctx_pad * (ctx->l_hd / 2);
        hipLaunchKernelGGL(rope_identity_kernel, dim3((n + 255) / 256), dim3(256), 0, s, ident, n);
        CK(hipGetLastError());
    }
    CK(launch_skinny(mk_sk_qkv(ctx, 0, xf, (const half_t*)w_packed, rows, kx, rope ? ctx->l_rope : ident, pos_dev, nullptr, nullptr), s));
    CK(launch_attn_map(mk_attn_map(ctx, 0, pos_dev, rows, window, score, ml, out), s));
    return AUR_OK;
}

// One decode projection alone on caller rows (parity tests): the production producer of x fragments (and sum(x^2)) at batch rows
// [b0, b0 + rows), then launch_skinny with arguments from the builders the decode step itself uses (mk_sk_row / mk_sk_gateup / mk_lm_head):
// the structure - variant, split-K partials, fused reduce, k phases of gate/up, half grid - is mk_skinny's, stated nowhere else.  Everything else is
// copies between the caller's row-major buffers and the fragment forms.  Scratch (the caller's): x fragments of round_up(max_batch, 16)
// rows | residual / SiLU*up fragments | split-K partials | arrival counters.
static int64_t proj_rows_pad(const aur_ctx* c) { return rup(c->cfg.max_batch, 16); }
static int64_t proj_xf_bytes(const aur_ctx* c, int k) { return rup64(proj_rows_pad(c) * k * 2, 256); }
static int64_t proj_frag_bytes(const aur_ctx* c, int npad) { return rup64(proj_rows_pad(c) * npad * 2, 256); }
static int64_t proj_part_bytes(const aur_ctx* c, int npad) { return rup64((int64_t)4 * (npad / 16) * (proj_rows_pad(c) / 16) * 1024, 256); }
extern "C" int64_t aur_decode_proj_scratch_bytes(const aur_ctx* ctx, int32_t k, int32_t npad) {
    if (!ctx || k < 1 || npad < 16) return 0;
    return proj_xf_bytes(ctx, k) + proj_frag_bytes(ctx, npad) + proj_part_bytes(ctx, npad) + rup64((int64_t)(npad / 16) * 4, 256);
}
extern "C" int aur_decode_proj_rows(aur_ctx* ctx, int32_t mode, const void* x, int32_t rows, int32_t b0, int32_t k, const void* w_packed,
                                    int32_t npad, int32_t n, int32_t fold, float eps, float fill, void* out, int64_t out_bytes,
                                    unsigned long long* ssq_out, unsigned long long* ssq_in, unsigned long long* ssq_zero, int32_t* row_cnt_out,
                                    void* scratch, int64_t scratch_bytes, void* stream) {
    const char* who = "aur_decode_proj_rows";
    if (!ctx || !x || !w_packed || !out) return aur_fail(ctx, AUR_ERR_ARG, "%s: null argument", who);
    if (mode != AUR_PROJ_ROW && mode != AUR_PROJ_LOGITS && mode != AUR_PROJ_SILU_MUL)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: mode %d is not AUR_PROJ_ROW, AUR_PROJ_LOGITS or AUR_PROJ_SILU_MUL", who, mode);
    const aur_config& g = ctx->cfg;
    if (rows < 1 || b0 < 0 || b0 + rows > g.max_batch) return aur_fail(ctx, AUR_ERR_ARG, "%s: batch rows [%d, %d) outside [0, max_batch %d)", who, b0, b0 + rows, g.max_batch);
    if (k < 128 || (k & 127) || k > 16384 || npad < 256 || (npad & 255) || n < 1 || n > npad)
        return aur_fail(ctx, AUR_ERR_ARG, "%s: need k a multiple of 128 in [128, 16384], npad a positive multiple of 256, 1 <= n <= npad (got %d, %d, %d)", who, k, npad, n);
    if (mode == AUR_PROJ_ROW && ((n & 31) || !ssq_out || fold))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: a residual projection needs n %% 32 == 0 (got %d), ssq_out, and folds no norm", who, n);
    if (mode == AUR_PROJ_SILU_MUL && (n & 63)) return aur_fail(ctx, AUR_ERR_ARG, "%s: gate/up needs n %% 64 == 0 (got %d)", who, n);
    if (fold && (!ssq_in || !ssq_zero)) return aur_fail(ctx, AUR_ERR_ARG, "%s: fold needs ssq_in and ssq_zero", who);
    const int64_t rp = proj_rows_pad(ctx);
    // out: SK_ROW the residual fp16 [rp, n]; SK_SILU_MUL fp16 [rp, n / 2]; SK_LOGITS fp32 [rp, n] + at least 4 floats of guard
    const int64_t need = mode == AUR_PROJ_ROW ? rp * n * 2 : mode == AUR_PROJ_SILU_MUL ? rp * (n / 2) * 2 : (rp * n + 4) * 4;
    if (out_bytes < need || ((uintptr_t)out & 15)) return aur_fail(ctx, AUR_ERR_ARG, "%s: out must be 16-byte aligned and hold %lld bytes (got %lld)", who, (long long)need, (long long)out_bytes);
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < aur_decode_proj_scratch_bytes(ctx, k, npad))
        return aur_fail(ctx, AUR_ERR_ARG, "%s: scratch must be 256-byte aligned and hold aur_decode_proj_scratch_bytes = %lld bytes (got %lld)", who,
                        (long long)aur_decode_proj_scratch_bytes(ctx, k, npad), (long long)scratch_bytes);
    hipStream_t s = (hipStream_t)stream;
    half_t* xf = (half_t*)scratch;
    half_t* frag = (half_t*)((char*)scratch + proj_xf_bytes(ctx, k));
    float* part = (float*)((char*)frag + proj_frag_bytes(ctx, npad));
    int* cnt = (int*)((char*)part + proj_part_bytes(ctx, npad));
    // 1. producer: every batch row holds the fill, then the caller's rows land at [b0, b0 + rows)
    const half_t fh = (half_t)fill;
    unsigned short fbits;
    memcpy(&fbits, &fh, 2);
    CK(hipMemsetD16Async((hipDeviceptr_t)xf, fbits, (size_t)rp * k, s));
    if (fold) {
        CK(hipMemsetAsync(ssq_zero, 0x5a, (size_t)AUR_SSQ_SLOTS * AUR_MAX_BATCH * 8, s));       // the projection must clear all of it
        CK(launch_xfrag_norm((const half_t*)x, k, nullptr, eps, rows, k, b0, xf, ssq_in, s));   // the prefill hand-over's call
    } else if (b0 == 0) CK(launch_xfrag_pack((const half_t*)x, k, rows, k, xf, s));
    else CK(launch_xfrag_norm((const half_t*)x, k, nullptr, eps, rows, k, b0, xf, nullptr, s));  // the same rows at an offset: a plain copy
    // 2. projection
    const half_t* W = (const half_t*)w_packed;
    const int B = b0 + rows;
    if (!fold) ssq_in = ssq_zero = nullptr;
    SkinnyArgs a;
    if (mode == AUR_PROJ_ROW) {
        CK(launch_xfrag_pack((const half_t*)out, n, (int)rp, n, frag, s));
        CK(hipMemsetAsync(cnt, 0, (size_t)(npad / 16) * 4, s));
        a = mk_sk_row(ctx, xf, W, frag, ssq_out, part, cnt, B, b0, B, k, npad, n);
    } else if (mode == AUR_PROJ_SILU_MUL) {
        CK(launch_xfrag_pack((const half_t*)out, n / 2, (int)rp, n / 2, frag, s));
        a = mk_sk_gateup(ctx, xf, W, frag, B, b0, B, k, npad, n, ssq_in, ssq_zero);
    } else {      // the production lm_head launch on the caller's weight and dimensions (and, unlike it, with an accumulator to clear)
        a = mk_lm_head(ctx, xf, ssq_in, (float*)out, B, b0, B);
        a.W = W; a.Npad = npad; a.K = k; a.n_real = n; a.ssq_zero = ssq_zero;
    }
    if (fold) a.norm_eps = eps;
    CK(launch_skinny(a, s));
    // 3. results back in the caller's row-major form, all round_up(max_batch, 16) batch rows
    if (a.mode != SK_LOGITS) {
        const int d = a.mode == SK_ROW ? n : n / 2;
        hipLaunchKernelGGL(xfrag_unpack_kernel, dim3((unsigned)((rp * (d >> 3) + 255) / 256)), dim3(256), 0, s, frag, (int)rp, d, (half_t*)out);
        CK(hipGetLastError());
    }
    if (a.mode == SK_ROW && row_cnt_out) CK(hipMemcpyAsync(row_cnt_out, cnt, (size_t)(npad / 16) * 4, hipMemcpyDeviceToDevice, s));
    return AUR_OK;
}

// One thread stores the device's constant-rate clock (wall_clock64: hipDeviceAttributeWallClockRate kHz) for step `n` = ring[0];
// the closing stamp advances the step count.  Two of these bracket ONE layer's attention launch inside the captured decode step when
// option "decode_stamp_layer" is set: the interval they give is that kernel's duration in the loop the caller actually runs (beside a
// front end, on a CU-masked stream, replayed from the graph) plus two kernel boundaries (~3 us).
__global__ void stamp_kernel(unsigned long long* __restrict__ ring, int which) {
    const unsigned long long n = ring[0];
    ring[8 + 2 * (n % AUR_STAMP_RING) + which] = (unsigned long long)wall_clock64();
    if (which) ring[0] = n + 1;
}

static int enqueue_decode_step(aur_ctx* ctx, hipStream_t s, bool instrument) {
    const aur_config& g = ctx->cfg;
    const int B = ctx->bank().batch;
    for (int l = 0; l < g.llm_layers; ++l) {
        CK(launch_skinny(mk_dec_qkv(ctx, l), s));
        if (ctx->bank().am && attn_map_layer(ctx->bank(), l)) CK(launch_attn_map(mk_dec_attn_map(ctx, l), s));       // the layer's roped q is in d_q, its newest key in the pages
        {
            const DecAttnArgs at = mk_dec_attn(ctx, l);
            const bool stamp = l == ctx->stamp_layer && ctx->d_stamp && !instrument;
            if (instrument) kev_begin(ctx->kev[0], s);
            if (stamp) { hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, s, ctx->d_stamp, 0); CK(hipGetLastError()); }
            CK(launch_decode_attention_main(at, s));
            if (stamp) { hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, s, ctx->d_stamp, 1); CK(hipGetLastError()); }
            if (instrument) kev_end(ctx->kev[0], s);
            CK(launch_decode_attention_combine(at, s));
        }
        CK(launch_skinny(mk_dec_o(ctx, l), s));
        SkinnyArgs gu = mk_dec_gateup(ctx, l);
        if (instrument) kev_begin(ctx->kev[1], s);
        CK(launch_skinny(gu, s));
        if (instrument) kev_end(ctx->kev[1], s);
        CK(launch_skinny(mk_dec_down(ctx, l), s));
    }
    return lm_head_and_advance(ctx, 0, B, 1, -1, s);
}

extern "C" int aur_llm_decode(aur_ctx* ctx, int32_t steps, void* stream) {
    aur_ctx::Bank& K = ctx->bank();
    if (!ctx->finalized || ctx->ll.empty() || K.batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "aur_llm_decode: call aur_begin_batch / aur_llm_prefill first");
    hipStream_t s = (hipStream_t)stream;
    if (steps <= 0) return AUR_OK;
    if (ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "aur_llm_decode inside aur_graph_begin / aur_graph_end: the decode step replays its own graph");
    stage_begin(ctx, "decode", s);
    const bool use_graph = ctx->cfg.use_graph && !ctx->prof;
    if (use_graph) {
        if (K.graph_batch != K.batch) drop_graphs(K);
        hipGraphExec_t& gx = ctx->decode_half ? K.graph_h : K.graph;
        if (!gx) {
            hipGraph_t gr;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            int rc = enqueue_decode_step(ctx, s, false);
            hipError_t e = hipStreamEndCapture(s, &gr);
            if (rc) return rc;
            if (e != hipSuccess) return aur_fail(ctx, AUR_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
            CK(hipGraphInstantiate(&gx, gr, nullptr, nullptr, 0));
            (void)hipGraphDestroy(gr);
            K.graph_batch = K.batch;
        }
        for (int i = 0; i < steps; ++i) CK(hipGraphLaunch(gx, s));
    } else {
        for (int i = 0; i < steps; ++i) {
            int rc = enqueue_decode_step(ctx, s, ctx->prof);
            if (rc) return rc;
        }
    }
    stage_end(ctx, "decode", s);
    return AUR_OK;
}

// In-loop intervals of the stamped attention launch (option "decode_stamp_layer"): the last min(cap, steps stamped, AUR_STAMP_RING)
// steps, oldest first, in microseconds.  Synchronises the stream.
extern "C" int aur_decode_stamps_read(aur_ctx* ctx, double* us_out, int32_t cap, int64_t* steps_total_out, int32_t* n_out, void* stream) {
    NO_CAPTURE("aur_decode_stamps_read");
    if (!ctx->d_stamp || !us_out || cap < 1 || !n_out) return aur_fail(ctx, AUR_ERR_ARG, "aur_decode_stamps_read: workspace not set or null argument");
    hipStream_t s = (hipStream_t)stream;
    std::vector<unsigned long long> h(8 + 2 * AUR_STAMP_RING);
    CK(hipMemcpyAsync(h.data(), ctx->d_stamp, h.size() * 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    int dev = 0, khz = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
    if (khz <= 0) return aur_fail(ctx, AUR_ERR_HIP, "hipDeviceAttributeWallClockRate = %d", khz);
    const unsigned long long total = h[0];
    int64_t n = (int64_t)(total < (unsigned long long)AUR_STAMP_RING ? total : AUR_STAMP_RING);
    if (n > cap) n = cap;
    for (int64_t i = 0; i < n; ++i) {
        const unsigned long long step = total - (unsigned long long)n + (unsigned long long)i;
        const unsigned long long t0 = h[8 + 2 * (step % AUR_STAMP_RING)], t1 = h[8 + 2 * (step % AUR_STAMP_RING) + 1];
        us_out[i] = (double)(t1 - t0) * 1e3 / (double)khz;
    }
    if (steps_total_out) *steps_total_out = (int64_t)total;
    *n_out = (int32_t)n;
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ caller-captured graphs
// The front end of a clip (or of a group of equal-shape clips) is ~600 launches whose arguments depend only on the shape bucket
// (frames, input size, r, prompt structure, target KV sequences) once the inputs sit in fixed staging buffers.  A serving loop captures
// that call sequence once per bucket and replays it with one call - the design the reference tree's serving engine uses for its decode
// step (src/sglang/python/sglang/srt/model_executor/cuda_graph_runner.py:163-279: one captured graph per shape bucket, inputs copied
// into the graph's static buffers before each replay).  Everything between begin and end must be enqueue-only calls of THIS ctx on
// THIS stream from THIS thread (aur_vit_encode*, aur_project_splice, aur_llm_prefill_batch / _stage / _commit, aur_slot_reset /
// _retire / _collect, the kernel-level entry points); calls that synchronise (aur_get_outputs, aur_unfinished, aur_slot_state,
// aur_microbench, aur_decode_stamps_read, aur_set_option on a dec_* knob) and aur_llm_decode (it replays its own graph) are rejected by
// the runtime and fail the capture.  Kernel arguments, including the ctx's gemm_* knobs and the current bank, are frozen at capture
// time: aur_select_bank is refused inside a capture.
extern "C" int aur_graph_begin(aur_ctx* ctx, void* stream) {
    if (!ctx->finalized) return aur_fail(ctx, AUR_ERR_STATE, "aur_graph_begin: weights not finalized");
    if (ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "aur_graph_begin: a capture is already open on this ctx");
    if (ctx->prof) return aur_fail(ctx, AUR_ERR_STATE, "aur_graph_begin: per-stage profiling is on (aur_profile_enable): its events cannot be captured");
    CK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    ctx->cap_stream = (hipStream_t)stream;
    return AUR_OK;
}
// Ends the capture opened by aur_graph_begin (always - also after a failed call in between) and instantiates the graph.
// *graph_out: handle >= 1 for aur_graph_launch; *nodes_out (may be NULL): number of graph nodes.
extern "C" int aur_graph_end(aur_ctx* ctx, void* stream, int32_t* graph_out, int64_t* nodes_out) {
    if (!ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "aur_graph_end: no capture is open");
    if ((hipStream_t)stream != ctx->cap_stream) return aur_fail(ctx, AUR_ERR_ARG, "aur_graph_end: not the stream aur_graph_begin was given");
    ctx->capturing = false;
    hipGraph_t gr = nullptr;
    hipError_t e = hipStreamEndCapture((hipStream_t)stream, &gr);
    if (e != hipSuccess || !gr) {
        // a call of the CALLER's inside the capture synchronised: make sure the stream has really left capture mode and drop the sticky error
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
            hipGraph_t g2 = nullptr;
            (void)hipStreamEndCapture((hipStream_t)stream, &g2);
            if (g2) (void)hipGraphDestroy(g2);
        }
        (void)hipGetLastError();
        return aur_fail(ctx, AUR_ERR_HIP, "hipStreamEndCapture: %s (a call inside the capture synchronised or failed)", hipGetErrorString(e));
    }
    if (!graph_out) {
        (void)hipGraphDestroy(gr);
        return aur_fail(ctx, AUR_ERR_ARG, "aur_graph_end: graph_out is NULL");
    }
    size_t n = 0;
    (void)hipGraphGetNodes(gr, nullptr, &n);
    aur_ctx::UserGraph ug;
    e = hipGraphInstantiate(&ug.exec, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    if (e != hipSuccess) return aur_fail(ctx, AUR_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    ug.nodes = (int64_t)n;
    size_t slot = 0;
    while (slot < ctx->ugraphs.size() && ctx->ugraphs[slot].exec) ++slot;
    if (slot == ctx->ugraphs.size()) ctx->ugraphs.push_back(ug);
    else ctx->ugraphs[slot] = ug;
    *graph_out = (int32_t)slot + 1;
    if (nodes_out) *nodes_out = ug.nodes;
    return AUR_OK;
}
extern "C" int aur_graph_launch(aur_ctx* ctx, int32_t graph, void* stream) {
    if (graph < 1 || graph > (int32_t)ctx->ugraphs.size() || !ctx->ugraphs[graph - 1].exec) return aur_fail(ctx, AUR_ERR_ARG, "aur_graph_launch: unknown graph %d", graph);
    if (ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "aur_graph_launch: a capture is open on this ctx");
    CK(hipGraphLaunch(ctx->ugraphs[graph - 1].exec, (hipStream_t)stream));
    return AUR_OK;
}
// The caller guarantees that no launch of the graph is still queued or running (its own event / stream synchronisation).
extern "C" int aur_graph_destroy(aur_ctx* ctx, int32_t graph) {
    if (graph < 1 || graph > (int32_t)ctx->ugraphs.size() || !ctx->ugraphs[graph - 1].exec) return aur_fail(ctx, AUR_ERR_ARG, "aur_graph_destroy: unknown graph %d", graph);
    (void)hipGraphExecDestroy(ctx->ugraphs[graph - 1].exec);
    ctx->ugraphs[graph - 1] = aur_ctx::UserGraph{};
    return AUR_OK;
}

extern "C" int aur_get_outputs(aur_ctx* ctx, int32_t* ids_host, int32_t* lens_host, void* stream) {
    NO_CAPTURE("aur_get_outputs");
    hipStream_t s = (hipStream_t)stream;
    const aur_ctx::Bank& K = ctx->bank();
    if (ids_host) CK(hipMemcpyAsync(ids_host, K.s_ids, (size_t)K.batch * K.max_new * 4, hipMemcpyDeviceToHost, s));
    if (lens_host) CK(hipMemcpyAsync(lens_host, K.s_len, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return AUR_OK;
}
extern "C" int aur_unfinished(aur_ctx* ctx, int32_t* count_host, void* stream) {
    NO_CAPTURE("aur_unfinished");
    hipStream_t s = (hipStream_t)stream;
    const aur_ctx::Bank& K = ctx->bank();
    std::vector<int32_t> fin(K.batch), len(K.batch);
    CK(hipMemcpyAsync(fin.data(), K.s_fin, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(len.data(), K.s_len, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    int n = 0;
    for (int b = 0; b < K.batch; ++b) n += (!fin[b] && len[b] < K.max_new) ? 1 : 0;
    *count_host = n;
    return AUR_OK;
}
// ---- per-slot control for continuous batching: slots of the active batch are independent sequences
static int slot_check(aur_ctx* ctx, int32_t slot, const char* who) {
    const int batch = ctx->bank().batch;
    if (batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "%s: no active batch (aur_begin_batch)", who);
    if (slot < 0 || slot >= batch) return aur_fail(ctx, AUR_ERR_ARG, "%s: slot %d outside the batch of %d", who, slot, batch);
    return AUR_OK;
}
extern "C" int aur_slot_reset(aur_ctx* ctx, int32_t slot, void* stream) {
    if (int rc = slot_check(ctx, slot, "aur_slot_reset")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const aur_ctx::Bank& K = ctx->bank();
    CK(hipMemsetAsync(K.s_len + slot, 0, 4, s));
    CK(hipMemsetAsync(K.s_fin + slot, 0, 4, s));
    CK(hipMemsetAsync(K.s_pos + slot, 0, 4, s));
    CK(hipMemsetAsync(K.s_ids + (int64_t)slot * K.max_new, 0, (size_t)K.max_new * 4, s));
    CK(hipMemsetAsync(K.s_rules + slot, 0, sizeof(aur_logit_rules), s));
    if (K.s_stop) CK(hipMemsetAsync(K.s_stop + slot, 0, sizeof(aur_stop_rules), s));
    if (K.s_guid) CK(launch_guidance_clear(K.s_guid, ctx->cfg.max_batch, slot, 1, s));       // the slot's record, and a leader's whose partner it was
    return slot_records_clear(ctx, K, slot, 1, s);
}
extern "C" int aur_slot_retire(aur_ctx* ctx, int32_t slot, void* stream) {
    if (int rc = slot_check(ctx, slot, "aur_slot_retire")) return rc;
    CK(hipMemsetD32Async((hipDeviceptr_t)(ctx->bank().s_fin + slot), 1, 1, (hipStream_t)stream));      // a fill node: no host source, no synchronisation
    return AUR_OK;
}
extern "C" int aur_slot_state(aur_ctx* ctx, int32_t* lens_host, int32_t* finished_host, void* stream) {
    NO_CAPTURE("aur_slot_state");
    const aur_ctx::Bank& K = ctx->bank();
    if (K.batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "aur_slot_state: no active batch");
    hipStream_t s = (hipStream_t)stream;
    if (lens_host) CK(hipMemcpyAsync(lens_host, K.s_len, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    if (finished_host) CK(hipMemcpyAsync(finished_host, K.s_fin, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return AUR_OK;
}
extern "C" int aur_slot_collect(aur_ctx* ctx, int32_t slot0, int32_t nslots, int32_t* ids_dev, int32_t* lens_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_collect")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (nslots < 1 || slot0 + nslots > K.batch || !ids_dev || !lens_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_collect: slots [%d, %d) outside the batch of %d", slot0, slot0 + nslots, K.batch);
    hipStream_t s = (hipStream_t)stream;
    CK(hipMemcpyAsync(ids_dev, K.s_ids + (int64_t)slot0 * K.max_new, (size_t)nslots * K.max_new * 4, hipMemcpyDeviceToDevice, s));
    CK(hipMemcpyAsync(lens_dev, K.s_len + slot0, (size_t)nslots * 4, hipMemcpyDeviceToDevice, s));
    return AUR_OK;
}
// ---- log-probabilities of generated tokens
static int64_t logprob_entries(const aur_config& g) { return (int64_t)g.max_batch * g.max_new_tokens; }
extern "C" int64_t aur_logprob_bytes(const aur_ctx* ctx, int32_t top_n) {
    if (!ctx || top_n < 0 || top_n > 8) return -1;
    return 4 * ((int64_t)ctx->cfg.max_batch + logprob_entries(ctx->cfg) * (1 + 2 * (int64_t)top_n));
}
extern "C" int aur_logprob_enable(aur_ctx* ctx, int32_t top_n, void* buf_dev, int64_t nbytes, void* stream) {
    NO_CAPTURE("aur_logprob_enable");
    aur_ctx::Bank& K = ctx->bank();
    if (buf_dev) {
        if (top_n < 0 || top_n > 8) return aur_fail(ctx, AUR_ERR_ARG, "aur_logprob_enable: top_n %d outside [0, 8]", top_n);
        if (((uintptr_t)buf_dev & 15) || nbytes < aur_logprob_bytes(ctx, top_n))
            return aur_fail(ctx, AUR_ERR_ARG, "aur_logprob_enable: buffer of %lld bytes (need %lld, 16-byte aligned)", (long long)nbytes,
                            (long long)aur_logprob_bytes(ctx, top_n));
    }
    // whether the step launches token_logprob_kernel, and with which pointers, is frozen inside this bank's captured decode graphs
    if (K.graph || K.graph_h) {
        (void)hipDeviceSynchronize();
        drop_graphs(K);
    }
    K.lp_len = nullptr;
    if (!buf_dev) return AUR_OK;
    const aur_config& g = ctx->cfg;
    const int64_t n = logprob_entries(g);
    int32_t* len = (int32_t*)buf_dev;
    float* lp = (float*)(len + g.max_batch);
    int32_t* tid = (int32_t*)(lp + n);
    float* tlp = (float*)(tid + n * top_n);
    // every slot without a record, at the widest row distance: that is every entry of the buffer, whatever max_new a batch runs with
    CK(launch_token_logprob_clear(0, g.max_batch, g.max_new_tokens, top_n, len, lp, tid, tlp, (hipStream_t)stream));
    K.lp_len = len; K.lp = lp; K.lp_top_id = tid; K.lp_top_lp = tlp; K.lp_top_n = top_n;
    return AUR_OK;
}
// counterpart of aur_get_outputs: synchronises.  lp_host [batch * max_new_tokens], top_ids_host / top_lp_host [batch * max_new_tokens * top_n]
// (may be NULL), lens_host [batch]: tokens recorded per slot.
extern "C" int aur_get_logprobs(aur_ctx* ctx, float* lp_host, int32_t* top_ids_host, float* top_lp_host, int32_t* lens_host, void* stream) {
    NO_CAPTURE("aur_get_logprobs");
    hipStream_t s = (hipStream_t)stream;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.lp_len || K.batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "aur_get_logprobs: not enabled on this bank (aur_logprob_enable), or no active batch");
    const size_t n = (size_t)K.batch * K.max_new;
    if (lp_host) CK(hipMemcpyAsync(lp_host, K.lp, n * 4, hipMemcpyDeviceToHost, s));
    if (top_ids_host && K.lp_top_n) CK(hipMemcpyAsync(top_ids_host, K.lp_top_id, n * K.lp_top_n * 4, hipMemcpyDeviceToHost, s));
    if (top_lp_host && K.lp_top_n) CK(hipMemcpyAsync(top_lp_host, K.lp_top_lp, n * K.lp_top_n * 4, hipMemcpyDeviceToHost, s));
    if (lens_host) CK(hipMemcpyAsync(lens_host, K.lp_len, (size_t)K.batch * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return AUR_OK;
}
// counterpart of aur_slot_collect: device-to-device, enqueue-only, recordable
extern "C" int aur_slot_collect_logprobs(aur_ctx* ctx, int32_t slot0, int32_t nslots, float* lp_dev, int32_t* top_ids_dev, float* top_lp_dev,
                                         int32_t* lens_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_collect_logprobs")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.lp_len) return aur_fail(ctx, AUR_ERR_STATE, "aur_slot_collect_logprobs: not enabled on this bank (aur_logprob_enable)");
    if (nslots < 1 || slot0 + nslots > K.batch || !lp_dev || !lens_dev || (K.lp_top_n && (!top_ids_dev || !top_lp_dev)))
        return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_collect_logprobs: slots [%d, %d) outside the batch of %d, or a null output", slot0, slot0 + nslots, K.batch);
    hipStream_t s = (hipStream_t)stream;
    const int64_t e0 = (int64_t)slot0 * K.max_new;
    const size_t n = (size_t)nslots * K.max_new;
    CK(hipMemcpyAsync(lp_dev, K.lp + e0, n * 4, hipMemcpyDeviceToDevice, s));
    if (K.lp_top_n) {
        CK(hipMemcpyAsync(top_ids_dev, K.lp_top_id + e0 * K.lp_top_n, n * K.lp_top_n * 4, hipMemcpyDeviceToDevice, s));
        CK(hipMemcpyAsync(top_lp_dev, K.lp_top_lp + e0 * K.lp_top_n, n * K.lp_top_n * 4, hipMemcpyDeviceToDevice, s));
    }
    CK(hipMemcpyAsync(lens_dev, K.lp_len + slot0, (size_t)nslots * 4, hipMemcpyDeviceToDevice, s));
    return AUR_OK;
}
extern "C" int aur_token_logprob_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const int32_t* tokens_dev, int32_t top_n,
                                      float* lp_out, int32_t* top_ids_out, float* top_lp_out, void* stream) {
    if (!ctx || !logits || !tokens_dev || !lp_out) return aur_fail(ctx, AUR_ERR_ARG, "aur_token_logprob_rows: null argument");
    if (rows < 1 || vocab < 1) return aur_fail(ctx, AUR_ERR_ARG, "aur_token_logprob_rows: rows %d or vocab %d < 1", rows, vocab);
    if (top_n < 0 || top_n > 8 || (top_n && (!top_ids_out || !top_lp_out)))
        return aur_fail(ctx, AUR_ERR_ARG, "aur_token_logprob_rows: top_n %d outside [0, 8], or null outputs for it", top_n);
    CK(launch_token_logprob_rows(logits, rows, vocab, tokens_dev, top_n, lp_out, top_ids_out, top_lp_out, (hipStream_t)stream));
    return AUR_OK;
}
// ---- attention over the prompt during decode.  Buffer: records fp32 [max_batch][max_new_tokens][window] | scores | page sums
static int64_t attn_map_rec_bytes(const aur_ctx* c, int window) { return rup64((int64_t)c->cfg.max_batch * c->cfg.max_new_tokens * window * 4, 256); }
extern "C" int64_t aur_attn_map_bytes(const aur_ctx* ctx, int32_t window) {
    if (!ctx || !attn_map_window_ok(ctx, window)) return -1;
    return attn_map_rec_bytes(ctx, window) + attn_map_score_bytes(ctx, window) + attn_map_ml_bytes(ctx);
}
extern "C" int aur_attn_map_enable(aur_ctx* ctx, int32_t window, uint64_t layer_mask, void* buf_dev, int64_t nbytes, void* stream) {
    NO_CAPTURE("aur_attn_map_enable");
    aur_ctx::Bank& K = ctx->bank();
    const aur_config& g = ctx->cfg;
    uint64_t mask = 0;
    if (buf_dev) {
        if (!attn_map_window_ok(ctx, window))
            return aur_fail(ctx, AUR_ERR_ARG, "aur_attn_map_enable: window %d is not a multiple of 64 in [64, %d] (or more than %d heads)", window, ctx->l_ctx_pad, AUR_ATTN_MAP_MAX_HEADS);
        const uint64_t all = g.llm_layers >= 64 ? ~0ull : ((1ull << g.llm_layers) - 1);
        mask = layer_mask ? layer_mask : all;
        if (g.llm_layers > 64 || (mask & ~all)) return aur_fail(ctx, AUR_ERR_ARG, "aur_attn_map_enable: layer mask 0x%llx names a layer outside [0, %d) (at most 64 layers)", (unsigned long long)layer_mask, g.llm_layers);
        if (((uintptr_t)buf_dev & 255) || nbytes < aur_attn_map_bytes(ctx, window))
            return aur_fail(ctx, AUR_ERR_ARG, "aur_attn_map_enable: buffer of %lld bytes (need %lld, 256-byte aligned)", (long long)nbytes, (long long)aur_attn_map_bytes(ctx, window));
    }
    // whether the step launches the recorder, for which layers and with which pointers, is frozen inside this bank's captured decode graphs
    if (K.graph || K.graph_h) {
        (void)hipDeviceSynchronize();
        drop_graphs(K);
    }
    K.am = nullptr;
    if (!buf_dev) return AUR_OK;
    CK(hipMemsetAsync(buf_dev, 0, (size_t)attn_map_rec_bytes(ctx, window), (hipStream_t)stream));
    K.am = (float*)buf_dev;
    K.am_score = (float*)((char*)buf_dev + attn_map_rec_bytes(ctx, window));
    K.am_ml = (float*)((char*)K.am_score + attn_map_score_bytes(ctx, window));
    K.am_window = window; K.am_mask = mask; K.am_nlayers = __builtin_popcountll(mask);
    return AUR_OK;
}
// counterpart of aur_get_logprobs: synchronises.  map_host fp32 [batch * max_new_tokens of the batch * window]
extern "C" int aur_get_attn_map(aur_ctx* ctx, float* map_host, void* stream) {
    NO_CAPTURE("aur_get_attn_map");
    hipStream_t s = (hipStream_t)stream;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.am || K.batch < 1) return aur_fail(ctx, AUR_ERR_STATE, "aur_get_attn_map: not enabled on this bank (aur_attn_map_enable), or no active batch");
    if (!map_host) return aur_fail(ctx, AUR_ERR_ARG, "aur_get_attn_map: null output");
    CK(hipMemcpyAsync(map_host, K.am, (size_t)K.batch * K.max_new * K.am_window * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return AUR_OK;
}
// counterpart of aur_slot_collect_logprobs: device-to-device, enqueue-only, recordable.  out_dev fp32 [nslots][max_new_tokens of the batch][window]
extern "C" int aur_slot_collect_attn_map(aur_ctx* ctx, int32_t slot0, int32_t nslots, float* out_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_collect_attn_map")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.am) return aur_fail(ctx, AUR_ERR_STATE, "aur_slot_collect_attn_map: not enabled on this bank (aur_attn_map_enable)");
    if (nslots < 1 || slot0 + nslots > K.batch || !out_dev)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_collect_attn_map: slots [%d, %d) outside the batch of %d, or a null output", slot0, slot0 + nslots, K.batch);
    const int64_t per = (int64_t)K.max_new * K.am_window;
    CK(hipMemcpyAsync(out_dev, K.am + slot0 * per, (size_t)nslots * per * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_slot_sampling(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_sampling* params_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_sampling")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (nslots < 1 || slot0 + nslots > K.batch || !params_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_sampling: slots [%d, %d) outside the batch of %d, or null parameters", slot0, slot0 + nslots, K.batch);
    CK(hipMemcpyAsync(K.s_samp + slot0, params_dev, (size_t)nslots * sizeof(aur_sampling), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_sample_rows(aur_ctx* ctx, const float* logits, int32_t rows, int32_t vocab, const aur_sampling* params_dev,
                               const int32_t* n_dev, int32_t* tokens_out, int32_t* kept_out, void* stream) {
    if (!ctx || !logits || !params_dev || !n_dev || !tokens_out) return aur_fail(ctx, AUR_ERR_ARG, "aur_sample_rows: null argument");
    if (rows < 1 || rows > 65535 || vocab < 1) return aur_fail(ctx, AUR_ERR_ARG, "aur_sample_rows: rows %d outside [1, 65535] or vocab %d < 1", rows, vocab);
    if ((uintptr_t)logits & 15) return aur_fail(ctx, AUR_ERR_ARG, "aur_sample_rows: logits must be 16-byte aligned");
    CK(launch_sample_rows(logits, rows, vocab, params_dev, n_dev, tokens_out, kept_out, (hipStream_t)stream, ctx->sample_stage));
    return AUR_OK;
}
extern "C" int aur_slot_logit_rules(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_logit_rules* rules_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_logit_rules")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (nslots < 1 || slot0 + nslots > K.batch || !rules_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_logit_rules: slots [%d, %d) outside the batch of %d, or null rules", slot0, slot0 + nslots, K.batch);
    CK(hipMemcpyAsync(K.s_rules + slot0, rules_dev, (size_t)nslots * sizeof(aur_logit_rules), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_slot_guidance(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_guidance* recs_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_guidance")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.s_guid) return aur_fail(ctx, AUR_ERR_STATE, "aur_slot_guidance: set option \"guidance\" to 1 first");
    if (nslots < 1 || slot0 + nslots > K.batch || !recs_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_guidance: slots [%d, %d) outside the batch of %d, or null records", slot0, slot0 + nslots, K.batch);
    CK(hipMemcpyAsync(K.s_guid + slot0, recs_dev, (size_t)nslots * sizeof(aur_guidance), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_guidance_rows(aur_ctx* ctx, float* logits, int32_t rows, int32_t vocab, const aur_guidance* recs_dev, float* save, int32_t mode,
                                 void* stream) {
    if (!ctx || !logits || !recs_dev || !save) return aur_fail(ctx, AUR_ERR_ARG, "aur_guidance_rows: null argument");
    if (rows < 1 || rows > 65535 || vocab < 1 || mode < 0 || mode > 1)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_guidance_rows: rows %d outside [1, 65535], vocab %d < 1 or mode %d outside [0, 1]", rows, vocab, mode);
    if (mode == 0) CK(launch_guidance_apply(logits, 0, rows, vocab, rows, recs_dev, save, (hipStream_t)stream));
    else CK(launch_guidance_restore(logits, 0, rows, vocab, recs_dev, save, (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_logit_rules_rows(aur_ctx* ctx, float* logits, int32_t rows, int32_t vocab, const int32_t* ids_dev, int32_t ids_stride,
                                    const int32_t* lens_dev, const aur_logit_rules* rules_dev, int32_t eos_id, int32_t restore, void* stream) {
    if (!ctx || !logits || !ids_dev || !lens_dev || !rules_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_logit_rules_rows: null argument");
    NO_CAPTURE("aur_logit_rules_rows");
    if (rows < 1 || rows > 65535 || vocab < 1 || ids_stride < 1)
        return aur_fail(ctx, AUR_ERR_ARG, "aur_logit_rules_rows: rows %d outside [1, 65535], vocab %d < 1 or ids_stride %d < 1", rows, vocab, ids_stride);
    hipStream_t s = (hipStream_t)stream;
    char* side = nullptr;
    const int64_t list = logit_rules_save_bytes(rows, ids_stride);                     // the side lists, then the counts
    CK(hipMalloc((void**)&side, (size_t)list + (size_t)rows * 4));
    hipError_t e = launch_logit_rules_apply(logits, 0, rows, vocab, rules_dev, ids_dev, ids_stride, lens_dev, eos_id, side, (int32_t*)(side + list), s);
    if (e == hipSuccess && restore) e = launch_logit_rules_restore(logits, 0, rows, vocab, ids_stride, side, (const int32_t*)(side + list), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(side);
    CK(e);
    return AUR_OK;
}
extern "C" int aur_slot_stop(aur_ctx* ctx, int32_t slot0, int32_t nslots, const aur_stop_rules* rules_dev, void* stream) {
    if (int rc = slot_check(ctx, slot0, "aur_slot_stop")) return rc;
    const aur_ctx::Bank& K = ctx->bank();
    if (!K.s_stop) return aur_fail(ctx, AUR_ERR_STATE, "aur_slot_stop: needs option \"stop_rules\" 1 (it allocates the records)");
    if (nslots < 1 || slot0 + nslots > K.batch || !rules_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_slot_stop: slots [%d, %d) outside the batch of %d, or null rules", slot0, slot0 + nslots, K.batch);
    CK(hipMemcpyAsync(K.s_stop + slot0, rules_dev, (size_t)nslots * sizeof(aur_stop_rules), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}
static bool stop_table_ok(const int32_t* off, const uint8_t* bytes, int32_t vocab, int64_t nbytes) {
    if (!off && !bytes && vocab == 0 && nbytes == 0) return true;                      // no table: no string matches
    return off && bytes && vocab >= 1 && nbytes >= 1 && nbytes <= 0x7fffffff && !((uintptr_t)off & 3);
}
extern "C" int aur_stop_vocab(aur_ctx* ctx, const int32_t* offsets_dev, const uint8_t* bytes_dev, int32_t vocab, int64_t nbytes) {
    NO_CAPTURE("aur_stop_vocab");
    if (!stop_table_ok(offsets_dev, bytes_dev, vocab, nbytes))
        return aur_fail(ctx, AUR_ERR_ARG, "aur_stop_vocab: offsets [vocab + 1] and bytes [nbytes] with vocab >= 1 and 1 <= nbytes < 2^31, or all of them 0");
    // the pointers are by-value kernel arguments frozen inside the captured decode graphs of every bank
    if (ctx->stop_rules) {
        if (ctx->banks[0].graph || ctx->banks[0].graph_h || ctx->banks[1].graph || ctx->banks[1].graph_h) (void)hipDeviceSynchronize();
        for (auto& K : ctx->banks) drop_graphs(K);
    }
    ctx->stop_off = offsets_dev; ctx->stop_bytes = bytes_dev; ctx->stop_vocab = vocab; ctx->stop_nbytes = nbytes;
    return AUR_OK;
}
extern "C" int aur_stop_rows(aur_ctx* ctx, int32_t rows, const int32_t* ids_dev, int32_t ids_stride, const int32_t* lens_dev,
                             const aur_stop_rules* rules_dev, int32_t* finished_dev, int32_t batch_max_new, const int32_t* offsets_dev,
                             const uint8_t* bytes_dev, int32_t vocab, int64_t nbytes, void* stream) {
    if (!ctx || !ids_dev || !lens_dev || !rules_dev || !finished_dev) return aur_fail(ctx, AUR_ERR_ARG, "aur_stop_rows: null argument");
    if (rows < 1 || ids_stride < 1 || ((uintptr_t)rules_dev & 7))
        return aur_fail(ctx, AUR_ERR_ARG, "aur_stop_rows: rows %d < 1, ids_stride %d < 1 or records not 8-byte aligned", rows, ids_stride);
    if (!stop_table_ok(offsets_dev, bytes_dev, vocab, nbytes)) return aur_fail(ctx, AUR_ERR_ARG, "aur_stop_rows: byte table (see aur_stop_vocab)");
    CK(launch_stop_check(0, rows, rules_dev, ids_dev, ids_stride, lens_dev, batch_max_new, finished_dev, offsets_dev, bytes_dev, vocab, nbytes,
                         (hipStream_t)stream));
    return AUR_OK;
}
extern "C" int aur_copy_logits(aur_ctx* ctx, float* dst_dev, void* stream) {
    const aur_ctx::Bank& K = ctx->bank();
    if (K.batch < 1 || !dst_dev) return aur_fail(ctx, AUR_ERR_STATE, "aur_copy_logits: no active batch");
    CK(hipMemcpyAsync(dst_dev, K.d_logits, (size_t)K.batch * ctx->cfg.llm_vocab * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AUR_OK;
}

// ------------------------------------------------------------------------------------------ tuning / microbench
extern "C" int aur_set_option(aur_ctx* ctx, const char* name, int64_t value) {
    NO_CAPTURE("aur_set_option");
    if (!strcmp(name, "prefill_prune_last")) {          // 1 (default): the last prefill layer computes Q / attention / MLP for each sequence's last 128 rows only
        ctx->prune_last = value ? 1 : 0;
        return AUR_OK;
    }
    if (!strcmp(name, "tome_fused_ln")) {
        ctx->tome_fused_ln = value ? 1 : 0;
        return AUR_OK;
    }
    if (!strcmp(name, "dec_attn_local")) ctx->attn_local = value ? 1 : 0;
    else if (!strcmp(name, "skinny_row_split_min_k")) ctx->row_split_min_k = (int)value;
    else if (!strncmp(name, "gemm_", 5) || !strcmp(name, "microbench_prefill_nseq")) {
        // GEMM knobs: no GEMM is part of the captured decode step (its projections are the skinny kernels), so the graphs stay
        // valid - the serving schedule changes gemm_max_wgs around every front end (caption_stream) while decode launches are queued
        if (!strcmp(name, "gemm_mode")) ctx->gemm_mode = (int)value;
        else if (!strcmp(name, "gemm_max_wgs")) ctx->gemm_max_wgs = (int)value;
        else if (!strcmp(name, "gemm_nt_out")) ctx->gemm_nt_out = value < 0 ? -1 : (value ? 1 : 0);
        else if (!strcmp(name, "gemm_tail_split")) ctx->gemm_tail_split = value ? 1 : 0;
        else if (!strcmp(name, "microbench_prefill_nseq")) ctx->mb_nseq = (value >= 1 && value <= ctx->cfg.max_batch) ? (int)value : 1;
        else return aur_fail(ctx, AUR_ERR_ARG, "unknown option '%s'", name);
        return AUR_OK;
    }
    else if (!strcmp(name, "dec_attn_pps")) {
        if (value < 1) return aur_fail(ctx, AUR_ERR_ARG, "dec_attn_pps must be >= 1");
        ctx->pps = (int)value;
        ctx->nsplit = (ctx->l_max_pages + (int)value - 1) / (int)value;
    } else if (!strcmp(name, "decode_fused_reduce")) {
        // 1: the split-K residual projections (o, down) sum their partials in the projection kernel (the last-arriving split reduces;
        // decode.hip "split-K with the reduce IN the kernel"); 0: a second launch does (skinny_row_reduce_kernel).  Bitwise the same tokens.
        if (value < 0 || value > 1) return aur_fail(ctx, AUR_ERR_ARG, "decode_fused_reduce must be 0 or 1");
        ctx->fused_reduce = (int)value;
    } else if (!strcmp(name, "decode_stamp_layer")) {
        // value >= 0: two one-thread stamp launches bracket that layer's attention launch in every decode step (aur_decode_stamps_read);
        // -1 (default): none.  The step's graphs are re-captured.
        if (value < -1 || value >= ctx->cfg.llm_layers) return aur_fail(ctx, AUR_ERR_ARG, "decode_stamp_layer must be -1 or a layer index");
        ctx->stamp_layer = (int)value;
    } else if (!strcmp(name, "sampling") || !strcmp(name, "sample_stage")) {
        // which kernel picks the token (and how it reads its row) is frozen inside the captured decode graphs: they are re-captured
        if (value < 0 || value > 1) return aur_fail(ctx, AUR_ERR_ARG, "%s must be 0 or 1", name);
        (!strcmp(name, "sampling") ? ctx->sampling : ctx->sample_stage) = (int)value;
    } else if (!strcmp(name, "logit_rules")) {
        // whether the two launches bracket the pick is frozen inside the captured decode graphs, like "sampling": they are re-captured.
        // The side lists are allocated here, once, outside any capture; they live as long as the ctx
        if (value < 0 || value > 1) return aur_fail(ctx, AUR_ERR_ARG, "%s must be 0 or 1", name);
        if (value)
            for (int bk = 0; bk < 2; ++bk)
                if (!ctx->banks[bk].lr_save)
                    CK(hipMalloc(&ctx->banks[bk].lr_save, (size_t)logit_rules_save_bytes(ctx->cfg.max_batch, ctx->cfg.max_new_tokens)));
        ctx->logit_rules = (int)value;
    } else if (!strcmp(name, "guidance")) {
        // whether the three launches stand around the pick is frozen inside the captured decode graphs, like "sampling": they are
        // re-captured.  The records (neutral) and the save buffer are allocated here, once, outside any capture; they live as long as the ctx
        if (value < 0 || value > 1) return aur_fail(ctx, AUR_ERR_ARG, "%s must be 0 or 1", name);
        if (value)
            for (int bk = 0; bk < 2; ++bk) {
                aur_ctx::Bank& K = ctx->banks[bk];
                if (!K.s_guid) {
                    CK(hipMalloc((void**)&K.s_guid, (size_t)ctx->cfg.max_batch * sizeof(aur_guidance)));
                    CK(hipMemset(K.s_guid, 0, (size_t)ctx->cfg.max_batch * sizeof(aur_guidance)));
                }
                if (!K.gd_save) CK(hipMalloc((void**)&K.gd_save, (size_t)ctx->cfg.max_batch * ctx->cfg.llm_vocab * sizeof(float)));
            }
        ctx->guidance = (int)value;
    } else if (!strcmp(name, "stop_rules")) {
        // whether stop_check_kernel follows the pick is frozen inside the captured decode graphs, like "sampling": they are re-captured.
        // The records are allocated here, once, outside any capture, neutral; they live as long as the ctx
        if (value < 0 || value > 1) return aur_fail(ctx, AUR_ERR_ARG, "%s must be 0 or 1", name);
        if (value)
            for (int bk = 0; bk < 2; ++bk)
                if (!ctx->banks[bk].s_stop) {
                    CK(hipMalloc((void**)&ctx->banks[bk].s_stop, (size_t)ctx->cfg.max_batch * sizeof(aur_stop_rules)));
                    CK(hipMemset(ctx->banks[bk].s_stop, 0, (size_t)ctx->cfg.max_batch * sizeof(aur_stop_rules)));
                }
        ctx->stop_rules = (int)value;
    } else if (!strcmp(name, "decode_half_grid")) {
        // the following aur_llm_decode calls go to a stream that owns half of the CUs: QKV / gate-up launch half as many workgroups
        // with twice the tiles (decode.hip launch_skx_nb); bitwise the same tokens.  Keeps both captured graphs.
        ctx->decode_half = value ? 1 : 0;
        return AUR_OK;
    } else return aur_fail(ctx, AUR_ERR_ARG, "unknown option '%s'", name);
    // kernel arguments are frozen in the captured graphs of EVERY bank.  A graph may still be queued on a stream this call does not
    // know: wait for the device before destroying it (tuning path only - nothing in the serving schedules changes these knobs)
    if (ctx->banks[0].graph || ctx->banks[0].graph_h || ctx->banks[1].graph || ctx->banks[1].graph_h) (void)hipDeviceSynchronize();
    for (auto& K : ctx->banks) drop_graphs(K);
    return AUR_OK;
}

// Time ONE kernel of the path in isolation on the current generation state (after aur_llm_prefill): `iters`
// back-to-back launches cycling through the layers (so weights stream from HBM, not from the 256 MiB MALL),
// bracketed by HIP events on `stream`.  Synchronises.  us_out = mean microseconds per launch.
extern "C" int aur_microbench(aur_ctx* ctx, const char* kernel, int32_t iters, double* us_out, void* stream) {
    NO_CAPTURE("aur_microbench");
    const aur_ctx::Bank& K = ctx->bank();
    if (!ctx->finalized || ctx->ll.empty() || K.batch < 1 || ctx->last_prefill_len < 1)
        return aur_fail(ctx, AUR_ERR_STATE, "aur_microbench: prefill a batch first");
    hipStream_t s = (hipStream_t)stream;
    const aur_config& g = ctx->cfg;
    const int nl = g.llm_layers, d = g.llm_hidden;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto run = [&](int i) -> int {
        const int l = i % nl;
        if (!strcmp(kernel, "dec_qkv")) { CK(launch_skinny(mk_dec_qkv(ctx, l), s)); }
        else if (!strcmp(kernel, "dec_attn")) { CK(launch_decode_attention(mk_dec_attn(ctx, l), s)); }
        else if (!strcmp(kernel, "dec_o")) { CK(launch_skinny(mk_dec_o(ctx, l), s)); }
        else if (!strcmp(kernel, "dec_gateup")) { CK(launch_skinny(mk_dec_gateup(ctx, l), s)); }
        else if (!strcmp(kernel, "dec_down")) { CK(launch_skinny(mk_dec_down(ctx, l), s)); }
        else if (!strcmp(kernel, "dec_lm_head")) { CK(launch_skinny(mk_lm_head(ctx, K.d_x, K.s_ssq_mlp, K.d_logits, K.batch, 0, K.batch), s)); }
        else if (!strcmp(kernel, "dec_pick")) {              // the token pick alone, on the logits of the last step: whichever kernel the "sampling" mode selects
            if (ctx->sampling)
                CK(launch_sample_advance(K.d_logits, 0, K.batch, g.llm_vocab, K.s_samp, ctx->l_embed, d, K.eos, K.max_new, K.s_ids, K.s_len, K.s_fin,
                                         K.s_pos, K.d_x, K.s_ssq_mlp, 1, -1, s, nullptr, 0, ctx->sample_stage));
            else
                CK(launch_argmax_advance(K.d_logits, 0, K.batch, g.llm_vocab, ctx->l_embed, d, K.eos, K.max_new, K.s_ids, K.s_len, K.s_fin, K.s_pos,
                                         K.d_x, K.s_ssq_mlp, 1, -1, s));
        } else if (!strcmp(kernel, "dec_rules")) {             // the logit rules' two launches, on the logits and the history of the last step
            if (!ctx->logit_rules) return aur_fail(ctx, AUR_ERR_STATE, "aur_microbench: dec_rules needs option \"logit_rules\" 1");
            CK(launch_logit_rules_apply(K.d_logits, 0, K.batch, g.llm_vocab, K.s_rules, K.s_ids, K.max_new, K.s_len, K.eos, K.lr_save, K.lr_cnt, s));
            CK(launch_logit_rules_restore(K.d_logits, 0, K.batch, g.llm_vocab, K.max_new, K.lr_save, K.lr_cnt, s));
        } else if (!strcmp(kernel, "dec_guid")) {              // guidance's three launches, on the logits and the records of the last step
            if (!ctx->guidance) return aur_fail(ctx, AUR_ERR_STATE, "aur_microbench: dec_guid needs option \"guidance\" 1");
            CK(launch_guidance_apply(K.d_logits, 0, K.batch, g.llm_vocab, g.max_batch, K.s_guid, K.gd_save, s));
            CK(launch_guidance_restore(K.d_logits, 0, K.batch, g.llm_vocab, K.s_guid, K.gd_save, s));
            CK(launch_guidance_follow(0, K.batch, g.llm_vocab, g.max_batch, K.s_guid, ctx->l_embed, d, K.max_new, K.s_ids, K.s_len, K.s_fin, K.d_x,
                                      K.s_ssq_mlp, s));
        } else if (!strcmp(kernel, "dec_stop")) {              // the stop check alone, on the history and the records of the last step
            if (!ctx->stop_rules) return aur_fail(ctx, AUR_ERR_STATE, "aur_microbench: dec_stop needs option \"stop_rules\" 1");
            CK(launch_stop_check(0, K.batch, K.s_stop, K.s_ids, K.max_new, K.s_len, K.max_new, K.s_fin, ctx->stop_off, ctx->stop_bytes,
                                 ctx->stop_vocab, ctx->stop_nbytes, s));
        } else {
            int bit = !strcmp(kernel, "pre_norm") ? 1 : !strcmp(kernel, "pre_qkv") ? 2 : !strcmp(kernel, "pre_attn") ? 4 : !strcmp(kernel, "pre_o") ? 8
                      : !strcmp(kernel, "pre_gateup") ? 32 : !strcmp(kernel, "pre_down") ? 64 : 0;
            if (!bit) return aur_fail(ctx, AUR_ERR_ARG, "unknown kernel '%s'", kernel);
            // scratch residual stream: l_p1 (projector scratch) is free after the splice
            return prefill_layer(ctx, l, bit, PrefillPass{0, ctx->mb_nseq, ctx->l_p1, ctx->last_prefill_len, nullptr, 0, true}, s);
        }
        return AUR_OK;
    };
    for (int i = 0; i < 3; ++i) { int rc = run(i); if (rc) return rc; }
    CK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) { int rc = run(i + 3); if (rc) return rc; }
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *us_out = 1e3 * ms / iters;
    return AUR_OK;
}

extern "C" int aur_select_bank(aur_ctx* ctx, int32_t bank) {
    if (bank < 0 || bank >= ctx->nbanks) return aur_fail(ctx, AUR_ERR_ARG, "bank %d outside [0, %d) (aur_config.num_banks)", bank, ctx->nbanks);
    if (!ctx->ws) return aur_fail(ctx, AUR_ERR_STATE, "aur_select_bank: workspace not set");
    if (ctx->capturing) return aur_fail(ctx, AUR_ERR_STATE, "aur_select_bank inside aur_graph_begin / aur_graph_end: the captured calls belong to bank %d", ctx->cur_bank);
    ctx->cur_bank = bank;
    return AUR_OK;
}
