// Classifier-free guidance ahead of the token pick: a guided request is a PAIR of slots that decode in lock-step
// inside the ordinary step.  The leader's row c is conditioned on the prompt, its partner's row u on the negative prompt; with
//   lc_i = (c_i - max c) - log sum_j exp(c_j - max c),  lu_i likewise from u,
//   out_i = g * (lc_i - lu_i) + lu_i
// (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor; aurora_amd/guidance.py is the definition) `out` replaces the leader's
// row for the pick alone, ahead of the logit rules.  Three kernels, one workgroup per slot of the range, the grid of the pick kernels:
//   guidance_apply_kernel    leader: stores c into the save buffer and writes out in place; a neutral slot returns at once;
//   guidance_restore_kernel  leader: the saved row back - between two steps d_logits holds the model's rows, bit for bit;
//   guidance_follow_kernel   behind the stop check: the partner takes the leader's newest token, out_len, finished and next input.
// m and S of a row are score_row_stats' (score_row.h), so lc is the two fp32 operations of a token's log-probability.  out is three
// explicitly rounded operations, no contraction: a pure function of the two rows and g.  Element e = 4 q + j belongs to thread
// q % GD_THREADS whether the quad moves as 16 bytes or element by element.  No atomics; plain loads and vector stores.
#include "../../include/aurora_hip.h"
#include "score_row.h"

#define GD_THREADS SCORE_THREADS
#define GD_FOLLOW_THREADS 256

// a record asks for guidance: scale finite, positive and not 1 (the all-zero record, and a NaN, are neutral)
__device__ __forceinline__ bool gd_active(const aur_guidance r) { return r.scale > 0.f && r.scale < INFINITY && r.scale != 1.f; }
// the partner index comes from device memory: into [0, max_batch) before it addresses anything
__device__ __forceinline__ int gd_partner(const aur_guidance r, int max_batch) {
    return r.partner < 0 ? 0 : (r.partner >= max_batch ? max_batch - 1 : r.partner);
}

__global__ __launch_bounds__(GD_THREADS) void guidance_apply_kernel(float* __restrict__ logits, int b0, int vocab, int max_batch,
                                                                    const aur_guidance* __restrict__ recs, float* __restrict__ save) {
    __shared__ float sv[GD_THREADS / 64];
    __shared__ int si[GD_THREADS / 64];
    __shared__ float s_log[2];
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    const aur_guidance r = recs[b];
    if (!gd_active(r)) return;                                                        // neutral: nothing is read or written
    const float g = r.scale;
    float* c = logits + (int64_t)b * vocab;
    const float* u = logits + (int64_t)gd_partner(r, max_batch) * vocab;
    float* sav = save + (int64_t)b * vocab;
    const bool al4 = (vocab & 3) == 0;
    const bool vc = al4 && ((uintptr_t)c & 15) == 0, vu = al4 && ((uintptr_t)u & 15) == 0;
    float mc, mu, s;
    int a;
    score_row_stats(c, vocab, vc, sv, si, mc, a, s);
    if (tid == 0) s_log[0] = logf(s);
    __syncthreads();                                                                  // sv / si are reused
    score_row_stats(u, vocab, vu, sv, si, mu, a, s);
    if (tid == 0) s_log[1] = logf(s);
    __syncthreads();
    const float log_sc = s_log[0], log_su = s_log[1];
    const bool vec = vc && vu && ((uintptr_t)sav & 15) == 0;
    const int nq = (vocab + 3) >> 2;
#pragma unroll 2
    for (int q = tid; q < nq; q += GD_THREADS) {
        if (vec) {
            const f4 cv = *(const f4*)(c + 4 * q), uv = *(const f4*)(u + 4 * q);
            f4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float lc = __fsub_rn(__fsub_rn(cv[j], mc), log_sc), lu = __fsub_rn(__fsub_rn(uv[j], mu), log_su);
                o[j] = __fadd_rn(__fmul_rn(g, __fsub_rn(lc, lu)), lu);
            }
            *(f4*)(sav + 4 * q) = cv;
            *(f4*)(c + 4 * q) = o;
        } else {
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                if (e >= vocab) break;
                const float cv = c[e], uv = u[e];
                const float lc = __fsub_rn(__fsub_rn(cv, mc), log_sc), lu = __fsub_rn(__fsub_rn(uv, mu), log_su);
                sav[e] = cv;
                c[e] = __fadd_rn(__fmul_rn(g, __fsub_rn(lc, lu)), lu);
            }
        }
    }
}

__global__ __launch_bounds__(GD_THREADS) void guidance_restore_kernel(float* __restrict__ logits, int b0, int vocab,
                                                                      const aur_guidance* __restrict__ recs, const float* __restrict__ save) {
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    if (!gd_active(recs[b])) return;
    float* c = logits + (int64_t)b * vocab;
    const float* sav = save + (int64_t)b * vocab;
    const bool vec = (vocab & 3) == 0 && ((uintptr_t)c & 15) == 0 && ((uintptr_t)sav & 15) == 0;
    const int nq = (vocab + 3) >> 2;
    for (int q = tid; q < nq; q += GD_THREADS) {
        if (vec) *(f4*)(c + 4 * q) = *(const f4*)(sav + 4 * q);
        else
            for (int e = 4 * q; e < 4 * q + 4 && e < vocab; ++e) c[e] = sav[e];
    }
}

// For every leader of [b0, b0 + nb): its partner takes the leader's newest token, out_len and finished, and the next input
// x[partner] = embed[token] with its sum(x^2) (embed_next_input: advance_tail's loop and tree).  pos is not written: both slots were
// unfinished or finished together before the step, so each has advanced its own position, or not, already.  Idempotent.
__global__ __launch_bounds__(GD_FOLLOW_THREADS) void guidance_follow_kernel(int b0, int vocab, int max_batch,
                                                                            const aur_guidance* __restrict__ recs,
                                                                            const half_t* __restrict__ embed, int d, int max_new,
                                                                            int32_t* __restrict__ out_ids, int32_t* __restrict__ out_len,
                                                                            int32_t* __restrict__ finished, half_t* __restrict__ xf,
                                                                            unsigned long long* __restrict__ ssq) {
    __shared__ float sv[256];
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    const aur_guidance r = recs[b];
    if (!gd_active(r)) return;
    const int p = gd_partner(r, max_batch);
    if (p == b) return;
    int n = out_len[b];
    n = n < 0 ? 0 : (n > max_new ? max_new : n);
    if (n < 1) return;                                                                // nothing picked yet
    int tok = out_ids[(int64_t)b * max_new + n - 1];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    if (tid == 0) {
        out_ids[(int64_t)p * max_new + n - 1] = tok;
        out_len[p] = n;
        finished[p] = finished[b];
    }
    embed_next_input(p, tok, embed, d, xf, ssq, sv);
}

// records of slots [s0, s0 + n) become neutral, and so does a leader whose partner is one of them
__global__ void guidance_clear_kernel(aur_guidance* __restrict__ recs, int max_batch, int s0, int n) {
    for (int b = threadIdx.x; b < max_batch; b += blockDim.x) {
        const aur_guidance r = recs[b];
        const int p = gd_partner(r, max_batch);
        if ((b >= s0 && b < s0 + n) || (gd_active(r) && p >= s0 && p < s0 + n)) {
            aur_guidance z;
            z.scale = 0.f;
            z.partner = 0;
            recs[b] = z;
        }
    }
}

hipError_t launch_guidance_apply(float* logits, int b0, int nb, int vocab, int max_batch, const aur_guidance* recs, float* save, hipStream_t s) {
    hipLaunchKernelGGL(guidance_apply_kernel, dim3(nb), dim3(GD_THREADS), 0, s, logits, b0, vocab, max_batch, recs, save);
    return hipGetLastError();
}

hipError_t launch_guidance_restore(float* logits, int b0, int nb, int vocab, const aur_guidance* recs, const float* save, hipStream_t s) {
    hipLaunchKernelGGL(guidance_restore_kernel, dim3(nb), dim3(GD_THREADS), 0, s, logits, b0, vocab, recs, save);
    return hipGetLastError();
}

hipError_t launch_guidance_follow(int b0, int nb, int vocab, int max_batch, const aur_guidance* recs, const half_t* embed, int d, int max_new,
                                  int32_t* out_ids, int32_t* out_len, int32_t* finished, half_t* xf, unsigned long long* ssq, hipStream_t s) {
    hipLaunchKernelGGL(guidance_follow_kernel, dim3(nb), dim3(GD_FOLLOW_THREADS), 0, s, b0, vocab, max_batch, recs, embed, d, max_new, out_ids,
                       out_len, finished, xf, ssq);
    return hipGetLastError();
}

hipError_t launch_guidance_clear(aur_guidance* recs, int max_batch, int s0, int n, hipStream_t s) {
    hipLaunchKernelGGL(guidance_clear_kernel, dim3(1), dim3(256), 0, s, recs, max_batch, s0, n);
    return hipGetLastError();
}
