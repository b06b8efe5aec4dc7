// Scoring given continuations (aur_llm_score_var, aur_score_rows): the log-probability of a target token under a logits row, and the
// gather that feeds ANY rows of a prefill pass - not only each sequence's last - to the pick path's lm_head.
// aurora_amd/scoring.py is the definition in numpy.
#include "score_row.h"

// ------------------------------------------------------------------------------------ score_rows_kernel
// One workgroup per row: a = first index of the maximum m (argmax_take: a (value, index) pair, so the scan order does not matter),
// S = sum exp(l_i - m) in fp32, lp = (l_t - m) - log S.  The evaluation is score_row_stats (score_row.h): element e = 4 q + j belongs to
// thread q % SCORE_THREADS, which adds its elements in increasing e; the 64 partial sums of a wave join in a butterfly (32, 16, .., 1),
// the 16 wave sums in a second one (8, 4, 2, 1).  That map is the same whether the quads are read with one 16-byte load (row 16-byte
// aligned and vocab % 4 == 0) or element by element, so the result is a pure function of the row's values: the same bits at any row
// index, row count or alignment.
// Additions per element: ceil(vocab / 4096) * 4 + 6 + 4.  The second pass re-reads the row (128 KB at 32000: it comes from L2).
// An entry whose target lies outside [0, vocab) is unused: lp = 0, a = -1, the row is not read.
__global__ __launch_bounds__(SCORE_THREADS) void score_rows_kernel(const float* __restrict__ logits, int vocab,
                                                                   const int32_t* __restrict__ targets, float* __restrict__ logprob_out,
                                                                   int32_t* __restrict__ argmax_out) {
    __shared__ float sv[SCORE_THREADS / 64];
    __shared__ int si[SCORE_THREADS / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int t = targets[row];
    if (t < 0 || t >= vocab) {                              // the whole workgroup takes this branch
        if (tid == 0) {
            logprob_out[row] = 0.f;
            argmax_out[row] = -1;
        }
        return;
    }
    const float* lg = logits + (int64_t)row * vocab;
    const bool vec = (vocab & 3) == 0 && ((uintptr_t)lg & 15) == 0;
    float m, s;
    int a;
    score_row_stats(lg, vocab, vec, sv, si, m, a, s);
    if (tid == 0) {
        logprob_out[row] = (lg[t] - m) - logf(s);
        argmax_out[row] = a;
    }
}

hipError_t launch_score_rows(const float* logits, int rows, int vocab, const int32_t* targets, float* logprob_out, int32_t* argmax_out,
                             hipStream_t s) {
    if (rows < 1 || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_rows_kernel, dim3(rows), dim3(SCORE_THREADS), 0, s, logits, vocab, targets, logprob_out, argmax_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ token_logprob_kernel
// Log-probability of a PICKED token under the row it was picked from, and the first top_n entries of the row in the order (value
// descending, index ascending) with theirs.  aurora_amd/scoring.py token_logprobs is the definition in numpy.
//   lp(t)  = (l_t - m) - logf(S): score_row_stats and the two fp32 operations of score_rows_kernel - bitwise aur_score_rows' value;
//   rank 0 = score_row_stats' first argmax a; rank r = the first entry strictly behind rank r - 1 in the order, found by the same
//            (value, index) reduction as the argmax over the entries that qualify - a pure function of the row, whatever the scan
//            order: no sort.  Its lp is the same two operations, (v - m) - logf(S).  Ranks the row has no entry for (r >= vocab; every
//            rank behind 0 of a row without a maximum) are (-1, 0.0).
// Every round re-reads the row (128 KB at 32000: from L2).  A token outside [0, vocab) is unused: lp = 0, every rank (-1, 0.0), the
// row is not read.  LOGPROB_MAX_TOP bounds top_n.
#define LOGPROB_MAX_TOP 8

__device__ __forceinline__ bool behind(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }

// by all SCORE_THREADS threads; ends with thread 0 having written lp_out[0], ids_out[0 .. top_n) and lps_out[0 .. top_n)
__device__ __forceinline__ void token_logprob_row(const float* __restrict__ lg, int vocab, int t, int top_n, float* __restrict__ lp_out,
                                                  int32_t* __restrict__ ids_out, float* __restrict__ lps_out) {
    __shared__ float sv[SCORE_THREADS / 64];
    __shared__ int si[SCORE_THREADS / 64];
    __shared__ float rv[2][SCORE_THREADS / 64];             // the rounds alternate between two slabs: one barrier per round
    __shared__ int ri[2][SCORE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (t < 0 || t >= vocab) {                              // the whole workgroup takes this branch
        if (tid == 0) {
            lp_out[0] = 0.f;
            for (int r = 0; r < top_n; ++r) {
                ids_out[r] = -1;
                lps_out[r] = 0.f;
            }
        }
        return;
    }
    const bool vec = (vocab & 3) == 0 && ((uintptr_t)lg & 15) == 0;
    const int nq = (vocab + 3) >> 2;
    float m, s;
    int a;
    score_row_stats(lg, vocab, vec, sv, si, m, a, s);
    float log_s = 0.f;
    if (tid == 0) {
        log_s = logf(s);
        lp_out[0] = (lg[t] - m) - log_s;
    }
    float pv = m;
    int pi = a;
    for (int r = 0; r < top_n; ++r) {
        if (r > 0) {
            float best = -INFINITY;
            int bi = 0x7fffffff;
            if (pi >= 0) {                                  // uniform: every thread holds the same (pv, pi).  Behind rank 0 of an all-NaN row
                                                            // (m = -inf, a = 0) nothing qualifies: no comparison with a NaN holds
#pragma unroll 2
                for (int q = tid; q < nq; q += SCORE_THREADS) {
                    const f4 v = score_quad(lg, q, vocab, vec);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (4 * q + j < vocab && behind(v[j], 4 * q + j, pv, pi)) argmax_take(best, bi, v[j], 4 * q + j);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) argmax_take(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
                if (lane == 0) {
                    rv[r & 1][wv] = best;
                    ri[r & 1][wv] = bi;
                }
                __syncthreads();
                best = rv[r & 1][0];
                bi = ri[r & 1][0];
                for (int w = 1; w < SCORE_THREADS / 64; ++w) argmax_take(best, bi, rv[r & 1][w], ri[r & 1][w]);
            }
            pv = best;
            pi = bi == 0x7fffffff ? -1 : bi;
        }
        if (tid == 0) {
            ids_out[r] = pi;
            lps_out[r] = pi < 0 ? 0.f : (pv - m) - log_s;
        }
    }
}

// The decode path's form, launched BEHIND the pick for slots [b0, b0 + gridDim.x): slot b appended a token in this step exactly when
// out_len[b] != lp_len[b]; then t = out_ids[b][n - 1] was picked from logits row b, and its record goes to index n - 1.  A slot that
// appended nothing (finished or idle: its row belongs to no token) returns without reading the row.
__global__ __launch_bounds__(SCORE_THREADS) void token_logprob_kernel(const float* __restrict__ logits, int b0, int vocab,
                                                                      const int32_t* __restrict__ out_ids, const int32_t* __restrict__ out_len,
                                                                      int max_new, int top_n, int32_t* __restrict__ lp_len, float* __restrict__ lp,
                                                                      int32_t* __restrict__ top_id, float* __restrict__ top_lp) {
    const int b = b0 + blockIdx.x;
    const int n = out_len[b], rec = lp_len[b];
    __syncthreads();                                        // every thread has read lp_len before thread 0 writes it
    if (n == rec || n < 1 || n > max_new) return;           // the whole workgroup
    const int64_t e = (int64_t)b * max_new + (n - 1);
    token_logprob_row(logits + (int64_t)b * vocab, vocab, out_ids[e], top_n, lp + e, top_id + e * top_n, top_lp + e * top_n);
    if (threadIdx.x == 0) lp_len[b] = n;
}

__global__ __launch_bounds__(SCORE_THREADS) void token_logprob_rows_kernel(const float* __restrict__ logits, int vocab,
                                                                           const int32_t* __restrict__ tokens, int top_n, float* __restrict__ lp,
                                                                           int32_t* __restrict__ top_id, float* __restrict__ top_lp) {
    const int64_t row = blockIdx.x;
    token_logprob_row(logits + row * vocab, vocab, tokens[row], top_n, lp + row, top_id + row * top_n, top_lp + row * top_n);
}

// state of slots [b0, b0 + nb): no record (lp_len = 0, lp = 0, every rank (-1, 0.0)); one workgroup per slot
__global__ __launch_bounds__(256) void token_logprob_clear_kernel(int b0, int max_new, int top_n, int32_t* __restrict__ lp_len,
                                                                  float* __restrict__ lp, int32_t* __restrict__ top_id,
                                                                  float* __restrict__ top_lp) {
    const int b = b0 + blockIdx.x;
    if (threadIdx.x == 0) lp_len[b] = 0;
    for (int i = threadIdx.x; i < max_new; i += 256) lp[(int64_t)b * max_new + i] = 0.f;
    for (int i = threadIdx.x; i < max_new * top_n; i += 256) {
        top_id[(int64_t)b * max_new * top_n + i] = -1;
        top_lp[(int64_t)b * max_new * top_n + i] = 0.f;
    }
}

hipError_t launch_token_logprob(const float* logits, int b0, int nb, int vocab, const int32_t* out_ids, const int32_t* out_len, int max_new,
                                int top_n, int32_t* lp_len, float* lp, int32_t* top_id, float* top_lp, hipStream_t s) {
    if (nb < 1 || vocab < 1 || max_new < 1 || top_n < 0 || top_n > LOGPROB_MAX_TOP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_logprob_kernel, dim3(nb), dim3(SCORE_THREADS), 0, s, logits, b0, vocab, out_ids, out_len, max_new, top_n, lp_len,
                       lp, top_id, top_lp);
    return hipGetLastError();
}

hipError_t launch_token_logprob_rows(const float* logits, int rows, int vocab, const int32_t* tokens, int top_n, float* lp, int32_t* top_id,
                                     float* top_lp, hipStream_t s) {
    if (rows < 1 || vocab < 1 || top_n < 0 || top_n > LOGPROB_MAX_TOP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_logprob_rows_kernel, dim3(rows), dim3(SCORE_THREADS), 0, s, logits, vocab, tokens, top_n, lp, top_id, top_lp);
    return hipGetLastError();
}

hipError_t launch_token_logprob_clear(int b0, int nb, int max_new, int top_n, int32_t* lp_len, float* lp, int32_t* top_id, float* top_lp,
                                      hipStream_t s) {
    if (nb < 1 || max_new < 1 || top_n < 0 || top_n > LOGPROB_MAX_TOP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_logprob_clear_kernel, dim3(nb), dim3(256), 0, s, b0, max_new, top_n, lp_len, lp, top_id, top_lp);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ row-list x-fragment gather
// The row-list form of xfrag_norm_kernel (decode.hip) without a norm weight: column b < n of the x-fragment buffer = flat row
// rows[b] of x (rows of d halves; flat row i * stride + r = row r of sequence i of the pass), sum(x^2) of it into the 2^-28
// fixed-point stripes - the same loop and butterfly as xfrag_norm_kernel's phase 1, so a row gets the bits the first-token path gives it.
// An entry is live when 0 <= rows[b] < nseq * stride and r < var_len(lens, i, stride); every other column of the buffer, up to the
// ncols it holds, is a zero row with ssq = 0.  eff_targets[b] = the entry's target when it is live, else -1: score_rows_kernel then
// treats it as unused.  One 1024-thread workgroup per group of 16 columns, one wave per column in phase 1.
__global__ __launch_bounds__(1024) void score_gather_kernel(const half_t* __restrict__ x, int d, const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ targets, int n, int ncols, int nseq, int stride,
                                                            const int32_t* __restrict__ lens, half_t* __restrict__ xf,
                                                            unsigned long long* __restrict__ ssq_out, int32_t* __restrict__ eff_targets) {
    __shared__ int64_t src[16];                             // flat row of each column of the group, -1 = a zero row
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int grp = blockIdx.x, K32 = d >> 5;
    {
        const int b = grp * 16 + wv;                        // phase 1: wave wv <-> column wv of the group
        int64_t row = -1;
        if (b < n) {
            const int fr = rows[b];
            if (fr >= 0 && fr < nseq * stride) {
                const int i = fr / stride, r = fr - i * stride;
                if (r < var_len(lens, i, stride)) row = fr;
            }
        }
        float ss = 0.f;
        if (row >= 0) {
            const half_t* xr = x + row * d;
            const int nchunk = d >> 3;
            for (int c0 = 0; c0 < nchunk; c0 += 512) {          // batches of 8 independent 16-byte loads per lane
                h8 t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int cch = c0 + lane + i * 64;
                    if (cch < nchunk) t[i] = *(const h8*)(xr + cch * 8);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int cch = c0 + lane + i * 64;
                    if (cch < nchunk) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) ss += (float)t[i][j] * (float)t[i][j];
                    }
                }
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) {
            src[wv] = row;
            if (b < ncols) {
                ssq_set(ssq_out, b, (unsigned long long)__float2ll_rn(ss * SSQ_SCALE));
                eff_targets[b] = row >= 0 ? targets[b] : -1;
            }
        }
    }
    __syncthreads();
    const int r = lane & 15, g = lane >> 4;
    const int64_t row = src[r];
    const half_t* xr = x + (row >= 0 ? row : 0) * d + g * 8;
    half_t* dst = xf + ((int64_t)grp * K32 * 64 + lane) * 8;
    for (int k0 = 0; k0 < K32; k0 += 8 * 16) {                 // batches of 8 tiles per wave: loads first, then the stores
        h8 t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k32 = k0 + wv + i * 16;
            t[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (row >= 0 && k32 < K32) t[i] = *(const h8*)(xr + k32 * 32);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k32 = k0 + wv + i * 16;
            if (k32 < K32) *(h8*)(dst + (int64_t)k32 * AUR_FRAG_HALVES) = t[i];
        }
    }
}

// rows / targets: the n entries of this chunk (device); ncols: columns of the x-fragment buffer (the engine's max_batch), n <= ncols <= AUR_MAX_BATCH
hipError_t launch_score_gather(const half_t* x, int d, const int32_t* rows, const int32_t* targets, int n, int ncols, int nseq, int stride,
                               const int32_t* lens, half_t* xf, unsigned long long* ssq_out, int32_t* eff_targets, hipStream_t s) {
    if ((d & 31) || n < 1 || n > ncols || ncols > AUR_MAX_BATCH || nseq < 1 || stride < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_gather_kernel, dim3((ncols + 15) >> 4), dim3(1024), 0, s, x, d, rows, targets, n, ncols, nseq, stride, lens, xf,
                       ssq_out, eff_targets);
    return hipGetLastError();
}
