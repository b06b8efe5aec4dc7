// Logit rules ahead of the token pick: repetition penalty, no-repeat n-gram and min-new-tokens as transformers'
// RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor / MinNewTokensLengthLogitsProcessor define them, over the history
// h = out_ids[b][0 .. n), n = out_len[b]: the tokens GENERATED so far, not the prompt.  aurora_amd/logit_rules.py is the definition.
//
// logit_rules_apply_kernel rewrites the affected entries of a slot's fp32 logits row in place, logit_rules_restore_kernel puts the
// originals back behind the pick: between two steps the row is the model's, bit for bit (aur_copy_logits and token_logprob_kernel
// read it).  One workgroup per slot, the grid of the pick kernels.  Every affected index is a token of the history or the EOS id, so
// the side list of a slot has one entry per history position plus one: entry j < n = (h[j], l[h[j]]), entry n = (eos, l[eos]) while
// the EOS is banned; an index of -1 is an entry that holds nothing.  No atomics, no compaction.
//
// A token that occurs k times in h is held by k threads.  Three phases, a workgroup barrier between them, make their writes agree:
//   1. gather: every entry's original value goes into the side list; nothing is written to the row;
//   2. penalty: l[t] = o < 0 ? o * p : o / p from the GATHERED original o - duplicate writers store the same bits, once or k times;
//   3. bans: -inf at h[j] for every position j that ends a repeat of the last g - 1 tokens, and at the EOS while n < m - the same
//      bits from every writer, and behind the penalty: a ban wins, as -inf * p = -inf / p = -inf says it must.
// The history may be longer than the workgroup: every phase strides over it.
#include "../../include/aurora_hip.h"
#include "advance.h"

#define LR_THREADS ARGMAX_THREADS

struct LrEntry {
    int32_t idx;
    float val;
};

__global__ __launch_bounds__(LR_THREADS) void logit_rules_apply_kernel(float* __restrict__ logits, int b0, int vocab,
                                                                       const aur_logit_rules* __restrict__ rules,
                                                                       const int32_t* __restrict__ ids, int ids_stride,
                                                                       const int32_t* __restrict__ lens, int eos_id,
                                                                       LrEntry* __restrict__ save, int32_t* __restrict__ save_cnt) {
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    const aur_logit_rules r = rules[b];
    const float p = r.repetition_penalty > 0.f ? r.repetition_penalty : 1.f;          // <= 0 / NaN: off
    const int g = r.no_repeat_ngram > 0 ? r.no_repeat_ngram : 0, m = r.min_new_tokens > 0 ? r.min_new_tokens : 0;
    if (p == 1.f && g == 0 && m == 0) {                                               // neutral: the row is not touched
        if (tid == 0) save_cnt[b] = 0;
        return;
    }
    int n = lens[b];
    n = n < 0 ? 0 : (n > ids_stride ? ids_stride : n);
    float* lg = logits + (int64_t)b * vocab;
    const int32_t* h = ids + (int64_t)b * ids_stride;
    LrEntry* sv = save + (int64_t)b * (ids_stride + 1);
    const bool ban_eos = n < m && eos_id >= 0 && eos_id < vocab;
    // 1. gather
    for (int j = tid; j < n; j += LR_THREADS) {
        const int t = h[j];
        LrEntry e;
        e.idx = (t >= 0 && t < vocab) ? t : -1;
        e.val = e.idx >= 0 ? lg[t] : 0.f;
        sv[j] = e;
    }
    if (tid == 0) {
        LrEntry e;
        e.idx = ban_eos ? eos_id : -1;
        e.val = ban_eos ? lg[eos_id] : 0.f;
        sv[n] = e;
        save_cnt[b] = n + 1;
    }
    __syncthreads();
    // 2. penalty, from the gathered originals
    if (p != 1.f)
        for (int j = tid; j < n; j += LR_THREADS) {
            const LrEntry e = sv[j];
            if (e.idx >= 0) lg[e.idx] = e.val < 0.f ? e.val * p : __fdiv_rn(e.val, p);
        }
    __syncthreads();
    // 3. bans: position j ends the g-gram h[j - g + 1 .. j]; its first g - 1 tokens against the last g - 1 of the history
    if (g > 0 && n + 1 >= g)
        for (int j = g - 1 + tid; j < n; j += LR_THREADS) {
            bool same = true;
            for (int q = 1; q < g && same; ++q) same = h[j - q] == h[n - q];
            const int t = h[j];
            if (same && t >= 0 && t < vocab) lg[t] = -INFINITY;
        }
    if (tid == 0 && ban_eos) lg[eos_id] = -INFINITY;
}

__global__ __launch_bounds__(LR_THREADS) void logit_rules_restore_kernel(float* __restrict__ logits, int b0, int vocab, int cap,
                                                                         const LrEntry* __restrict__ save,
                                                                         const int32_t* __restrict__ save_cnt) {
    const int b = b0 + blockIdx.x;
    int n = save_cnt[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    float* lg = logits + (int64_t)b * vocab;
    const LrEntry* sv = save + (int64_t)b * cap;
    for (int j = threadIdx.x; j < n; j += LR_THREADS) {
        const LrEntry e = sv[j];
        if (e.idx >= 0 && e.idx < vocab) lg[e.idx] = e.val;                           // duplicates carry the same original
    }
}

int64_t logit_rules_save_bytes(int rows, int ids_stride) { return (int64_t)rows * (ids_stride + 1) * (int64_t)sizeof(LrEntry); }

hipError_t launch_logit_rules_apply(float* logits, int b0, int nb, int vocab, const aur_logit_rules* rules, const int32_t* ids, int ids_stride,
                                    const int32_t* lens, int eos_id, void* save, int32_t* save_cnt, hipStream_t s) {
    hipLaunchKernelGGL(logit_rules_apply_kernel, dim3(nb), dim3(LR_THREADS), 0, s, logits, b0, vocab, rules, ids, ids_stride, lens, eos_id,
                       (LrEntry*)save, save_cnt);
    return hipGetLastError();
}

hipError_t launch_logit_rules_restore(float* logits, int b0, int nb, int vocab, int ids_stride, const void* save, const int32_t* save_cnt,
                                      hipStream_t s) {
    hipLaunchKernelGGL(logit_rules_restore_kernel, dim3(nb), dim3(LR_THREADS), 0, s, logits, b0, vocab, ids_stride + 1, (const LrEntry*)save,
                       save_cnt);
    return hipGetLastError();
}
