// The token pick's shared halves (decode.hip argmax_advance_kernel, sample.hip sample_advance_kernel): the first-argmax scan of a
// logits row and the step bookkeeping that follows whichever pick ran.  One copy, so that a sampled slot and a greedy slot that
// pick the same token leave the same bits behind (next-token embedding, its sum(x^2), pos, out_ids).
#pragma once
#include "kernels.h"

// address (halves) of the 16-byte piece holding x[b][k .. k+8) (k % 8 == 0) in x-fragment form
__device__ __forceinline__ int64_t xfrag_piece(int b, int k, int K32) {
    return ((((int64_t)(b >> 4) * K32 + (k >> 5)) * 64) + ((k >> 3) & 3) * 16 + (b & 15)) * 8;
}

#define SSQ_SCALE 268435456.0f      /* 2^28 */
__device__ __forceinline__ void ssq_set(unsigned long long* ssq, int b, unsigned long long v) {        // one writer per row
    ssq[b] = v;
#pragma unroll
    for (int sl = 1; sl < AUR_SSQ_SLOTS; ++sl) ssq[sl * AUR_MAX_BATCH + b] = 0ull;
}

#define ARGMAX_THREADS 1024
__device__ __forceinline__ void argmax_take(float& best, int& bi, float v, int i) {
    if (v > best || (v == best && i < bi)) {
        best = v;
        bi = i;
    }
}

// First maximum of lg[0 .. vocab) by all ARGMAX_THREADS threads of the workgroup (value, then index: whatever the scan order);
// sv / si: 256 entries of LDS each.  Every thread returns the token; the row's maximum is left in sv[0].  Ends behind a barrier.
__device__ __forceinline__ int row_first_argmax(const float* __restrict__ lg, int vocab, float* sv, int* si) {
    const int tid = threadIdx.x;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if ((vocab & 3) == 0) {                        // rows stay 16-byte aligned
        const int n4 = vocab >> 2;
#pragma unroll 4
        for (int i = tid; i < n4; i += ARGMAX_THREADS) {
            const f4 v = *(const f4*)(lg + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) argmax_take(best, bi, v[j], 4 * i + j);
        }
    } else {
        for (int i = tid; i < vocab; i += ARGMAX_THREADS) argmax_take(best, bi, lg[i], i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_take(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
    if ((tid & 63) == 0) {
        sv[tid >> 6] = best;
        si[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ARGMAX_THREADS / 64; ++w) argmax_take(best, bi, sv[w], si[w]);
        si[0] = bi;
        sv[0] = best;
    }
    __syncthreads();
    int tok = si[0];
    if (tok == 0x7fffffff) tok = 0;
    return tok;
}

// The next input of slot b: x[b] = embed[tok] in x-fragment form, with its sum(x^2) (2^-28 fixed point).  By every thread of a workgroup
// of at least 256 threads; sv: 256 floats of LDS.  The 256-thread loop and tree of rounds 1-3: same additions in the same order, same
// bits, whoever calls (advance_tail for the slot that picked, guidance.hip guidance_follow_kernel for the partner that follows).
__device__ __forceinline__ void embed_next_input(int b, int tok, const half_t* __restrict__ embed, int d, half_t* __restrict__ xf,
                                                 unsigned long long* __restrict__ ssq, float* sv) {
    const int tid = threadIdx.x;
    float ss = 0.f;
    if (tid < 256) {
        for (int cidx = tid; cidx < (d >> 3); cidx += 256) {
            const h8 v = *(const h8*)(embed + (int64_t)tok * d + cidx * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += (float)v[j] * (float)v[j];
            *(h8*)(xf + xfrag_piece(b, cidx * 8, d >> 5)) = v;
        }
        sv[tid] = ss;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {            // fixed-order tree: deterministic
        if (tid < o) sv[tid] += sv[tid + o];
        __syncthreads();
    }
    if (tid == 0) ssq_set(ssq, b, (unsigned long long)__float2ll_rn(sv[0] * SSQ_SCALE));
}

// Step bookkeeping for slot b once its token is known (every thread holds `tok`; called behind a barrier that protects sv): append
// to out_ids unless the sequence already finished; EOS marks it finished; the next input x[b] = embed[token] is written in
// x-fragment form together with sum(x^2) (2^-28 fixed point) for the first folded RMSNorm of the next step; pos[b] += advance_pos.
// The embedding copy and its sum(x^2) are embed_next_input above.
__device__ __forceinline__ void advance_tail(int b, int row, int tok, const half_t* __restrict__ embed, int d, int eos_id, int max_new,
                                             int32_t* __restrict__ out_ids, int32_t* __restrict__ out_len, int32_t* __restrict__ finished,
                                             int32_t* __restrict__ pos, half_t* __restrict__ xf, unsigned long long* __restrict__ ssq,
                                             int advance_pos, int set_pos, const int32_t* __restrict__ set_pos_lens, int len_cap, float* sv) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        const bool was_finished = finished[b] != 0;
        if (!was_finished) {
            const int n = out_len[b];
            if (n < max_new) {
                out_ids[(int64_t)b * max_new + n] = tok;
                out_len[b] = n + 1;
            }
            if (tok == eos_id || n + 1 >= max_new) finished[b] = 1;     // EOS, or the output row is full
        }
        // a variable-length prefill: each slot's own length, behind the set_pos positions it already held (0, or an extend's pos0)
        if (set_pos_lens) pos[b] = set_pos + var_len(set_pos_lens, row, len_cap);
        else if (set_pos >= 0) pos[b] = set_pos;
        // a finished (or idle) slot stops advancing: it keeps recomputing one position inside its own pages, so extra
        // decode steps (other slots still running, continuous batching) can never walk it past its KV allocation
        if (advance_pos && !was_finished) pos[b] += 1;
    }
    embed_next_input(b, tok, embed, d, xf, ssq, sv);
}
