// The evaluation of one logits row that scoring (score.hip score_rows_kernel) and the log-probabilities of generated tokens (score.hip
// token_logprob_kernel) share: first argmax a of the maximum m, S = sum exp(l_i - m), both in a fixed element-to-thread map and two
// fixed butterflies.  One copy, so that a generated token's log-probability is bitwise what aur_score_rows says about the same row.
#pragma once
#include "advance.h"

#define SCORE_THREADS ARGMAX_THREADS

__device__ __forceinline__ f4 score_quad(const float* __restrict__ lg, int q, int vocab, bool vec) {
    if (vec) return *(const f4*)(lg + 4 * q);
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 4 * q + j < vocab ? lg[4 * q + j] : -INFINITY;
    return v;
}

// By all SCORE_THREADS threads of the workgroup.  Element e = 4 q + j belongs to thread q % SCORE_THREADS, which takes its elements in
// increasing e; the 64 partial results of a wave join in a butterfly (32, 16, .., 1), the 16 wave results in a second one (8, 4, 2, 1).
// The map is the same whether the quads are read with one 16-byte load (row 16-byte aligned and vocab % 4 == 0) or element by element.
// sv / si: SCORE_THREADS / 64 entries of LDS each (left in use: the caller's later LDS traffic goes elsewhere or behind a barrier).
// Every thread gets m and a (a row without a maximum - all NaN -: m = -inf, a = 0, as the greedy pick says); S is complete on THREAD 0 only.
__device__ __forceinline__ void score_row_stats(const float* __restrict__ lg, int vocab, bool vec, float* sv, int* si, float& m, int& a,
                                                float& s_out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nq = (vocab + 3) >> 2;
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll 4
    for (int q = tid; q < nq; q += SCORE_THREADS) {
        const f4 v = score_quad(lg, q, vocab, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < vocab) argmax_take(best, bi, v[j], 4 * q + j);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_take(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
    if (lane == 0) {
        sv[wv] = best;
        si[wv] = bi;
    }
    __syncthreads();
    best = sv[0];
    bi = si[0];
    for (int w = 1; w < SCORE_THREADS / 64; ++w) argmax_take(best, bi, sv[w], si[w]);      // every thread: the same 16 pairs
    m = best;
    a = bi == 0x7fffffff ? 0 : bi;
    __syncthreads();                                        // sv is reused below
    float s = 0.f;
#pragma unroll 4
    for (int q = tid; q < nq; q += SCORE_THREADS) {
        const f4 v = score_quad(lg, q, vocab, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < vocab) s += expf(v[j] - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sv[wv] = s;
    __syncthreads();
    if (wv == 0) {
        s = lane < SCORE_THREADS / 64 ? sv[lane] : 0.f;
#pragma unroll
        for (int o = SCORE_THREADS / 128; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    s_out = s;
}
