// Seeded sampling (temperature, top-k, top-p) for the token pick: sample_advance_kernel has argmax_advance_kernel's contract - one
// workgroup per slot, the shared bookkeeping tail of advance.h - but the token comes from DESIGN section 5's definition with the slot's
// parameters (aur_sampling) read from device memory.
//
// Arithmetic that does not depend on the scan order, so the token is a pure function of (row, parameters, seed, stream, n):
//   - a value's weight is the INTEGER w_i = rint(exp((l_i - max l) / T) * 2^40) (the maximum weighs exactly 2^40, so no kept set has
//     mass 0); every mass is a sum of these integers in 64 bits (exact up to 2^23 tokens) - LDS integer atomics, any order, same bits;
//   - thresholds are found by SELECTION, not by sorting, on the order-preserving integer image of the fp32 logit (sm_key; the order
//     of l_i / T is the order of l_i): a histogram of 256 bins carries per bin a count, a mass and the smallest / largest key seen;
//     a walk from the top bin (a 256-thread prefix scan) finds the bin that holds the k-th largest value (count walk) or the last
//     value whose heavier neighbours weigh less than p * Z_k (mass walk); the next level splits that bin's [smallest, largest] key
//     interval in 256 again, until the interval is one key.  The first level bins by VALUE, linearly between the row's minimum and
//     maximum (a monotone map, so a valid digit): the top bits of an fp32 put a whole octave of a Gaussian row into one bin, and
//     same-address LDS atomics serialise.  A typical row is done after two levels per threshold;
//   - the draw is one masked prefix sum in index order over the integer weights: the first index whose inclusive sum exceeds
//     u * Z_K, compared exactly (u = m * 2^-24: floor(m * Z_K / 2^24) from the 128-bit product).  It always exists, so the
//     definition's "largest index in K" fallback is unreachable here; it is kept for the letter of it.
// The row (vocab * 4 bytes: 125 KiB at 32000) is staged in LDS once when it fits next to the 8 KiB of bins (dynamic LDS, above 64 KiB:
// sample_init asks for it once, outside any capture) and re-read from global memory (L2) otherwise; option "sample_stage" selects.
#include "../../include/aurora_hip.h"
#include "advance.h"

#define SM_THREADS ARGMAX_THREADS
#define SM_WSCALE 1099511627776.0f          /* 2^40 */
#define SM_STAGE_MAX_BYTES (148 * 1024)     /* + sizeof(SmShared) stays inside the CU's 160 KiB */

struct SmShared {
    unsigned long long mass[256];
    unsigned int cnt[256], kmin[256], kmax[256];
    unsigned long long wa[16], wb[16];       // per-wave totals of the block scans
    unsigned long long r_mass_excl, r_mass_bin, r_cnt_excl, r_cnt_bin, r_need;
    unsigned int r_lo, r_hi;
    int r_ok, r_tok, r_last;
    float sv[256];
    int si[256];
};

__device__ __forceinline__ float sm_clean(float v) { return v == v ? v + 0.0f : -INFINITY; }      // NaN -> -inf, -0 -> +0
__device__ __forceinline__ unsigned sm_key(float v) {                                              // v < w  <=>  key(v) < key(w)
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long sm_weight(float v, float lmax, float T) {
    return __float2ull_rn(expf((v - lmax) / T) * SM_WSCALE);
}

// word 0 of Philox4x32-10, key (seed lo, seed hi), counter (c0, c1, 0, 0)
__device__ __forceinline__ unsigned sm_philox_x0(unsigned long long seed, unsigned c0, unsigned c1) {
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), x0 = c0, x1 = c1, x2 = 0u, x3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, x0), l0 = 0xD2511F53u * x0, h1 = __umulhi(0xCD9E8D57u, x2), l1 = 0xCD9E8D57u * x2;
        x0 = h1 ^ x1 ^ k0;
        x1 = l1;
        x2 = h0 ^ x3 ^ k1;
        x3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return x0;
}

__device__ __forceinline__ unsigned long long sm_wave_scan(unsigned long long v) {        // inclusive, over the wave's 64 lanes
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// f(i, l_i) for every element of the row, strided over the workgroup; 16-byte loads where the row allows them
template <bool STAGED, typename F>
__device__ __forceinline__ void sm_foreach(const float* __restrict__ lg, const float* st, int vocab, F f) {
    const int tid = threadIdx.x;
    if ((vocab & 3) == 0) {
        const int n4 = vocab >> 2;
        for (int i = tid; i < n4; i += SM_THREADS) {
            const f4 v = STAGED ? *(const f4*)(st + 4 * i) : *(const f4*)(lg + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(4 * i + j, STAGED ? v[j] : sm_clean(v[j]));
        }
    } else {
        for (int i = tid; i < vocab; i += SM_THREADS) f(i, STAGED ? st[i] : sm_clean(lg[i]));
    }
}

// Selection.  BY_MASS false: tau = the need-th largest key (1 <= need <= vocab).  BY_MASS true: tau = the smallest key whose strictly
// larger keys weigh less than P = ceil(p * Z), Z = zk or, zk == 0, the row's whole mass.  cnt_ge / mass_ge: count and mass of keys >= tau.
template <bool STAGED, bool BY_MASS>
__device__ __forceinline__ void sm_select(SmShared& S, const float* __restrict__ lg, const float* st, int vocab, float lmax, float scale,
                                          float T, unsigned long long need, float p, unsigned long long zk, unsigned& tau,
                                          unsigned long long& cnt_ge, unsigned long long& mass_ge) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned lo = 0u, hi = 0xffffffffu;
    int sh = 24;
    unsigned long long acc_c = 0ull, acc_m = 0ull;
    tau = 0u; cnt_ge = (unsigned long long)vocab; mass_ge = 0ull;
    for (int level = 0; level < 8; ++level) {
        if (tid < 256) {
            S.mass[tid] = 0ull; S.cnt[tid] = 0u; S.kmin[tid] = 0xffffffffu; S.kmax[tid] = 0u;
        }
        if (tid == 0) S.r_ok = 0;
        __syncthreads();
        sm_foreach<STAGED>(lg, st, vocab, [&](int, float v) {
            const unsigned key = sm_key(v);
            int bin;
            if (level == 0) {
                bin = 255 - (int)fminf((lmax - v) * scale, 255.f);          // monotone in v; NaN (inf * 0) -> 255 -> bin 0
            } else {
                if (key < lo || key > hi) return;
                bin = (int)((key - lo) >> sh);
            }
            const unsigned long long w = sm_weight(v, lmax, T);
            atomicAdd(&S.cnt[bin], 1u);
            if (w) atomicAdd(&S.mass[bin], w);
            atomicMin(&S.kmin[bin], key);
            atomicMax(&S.kmax[bin], key);
        });
        __syncthreads();
        // walk from the top bin: thread t < 256 owns bin 255 - t
        const int bin = 255 - tid;
        unsigned long long c = 0ull, m = 0ull;
        if (tid < 256) { c = S.cnt[bin]; m = S.mass[bin]; }
        unsigned long long ci = 0ull, mi = 0ull;
        if (wave < 4) {
            ci = sm_wave_scan(c);
            mi = sm_wave_scan(m);
            if (lane == 63) { S.wa[wave] = ci; S.wb[wave] = mi; }
        }
        __syncthreads();
        if (BY_MASS && level == 0) {
            const unsigned long long z = zk ? zk : S.wb[0] + S.wb[1] + S.wb[2] + S.wb[3];
            need = (unsigned long long)ceil((double)p * (double)z);
            need = need < 1ull ? 1ull : (need > z ? z : need);
        }
        if (tid < 256) {
            for (int w = 0; w < wave; ++w) { ci += S.wa[w]; mi += S.wb[w]; }
            const unsigned long long incl = BY_MASS ? mi : ci, own = BY_MASS ? m : c;
            if (incl >= need && incl - own < need) {
                S.r_cnt_excl = ci - c; S.r_cnt_bin = c; S.r_mass_excl = mi - m; S.r_mass_bin = m;
                S.r_need = need - (incl - own);
                S.r_lo = S.kmin[bin]; S.r_hi = S.kmax[bin];
                S.r_ok = 1;
            }
        }
        __syncthreads();
        const int ok = S.r_ok;
        const unsigned long long ce = S.r_cnt_excl, cb = S.r_cnt_bin, me = S.r_mass_excl, mb = S.r_mass_bin, nd = S.r_need;
        const unsigned nlo = S.r_lo, nhi = S.r_hi;
        __syncthreads();
        if (!ok) return;                                   // unreachable (need <= the total): every key is kept
        acc_c += ce; acc_m += me; need = nd; lo = nlo; hi = nhi;
        if (lo == hi) {
            tau = lo; cnt_ge = acc_c + cb; mass_ge = acc_m + mb;
            return;
        }
        const unsigned span = hi - lo;
        sh = span > 255u ? (32 - __clz(span)) - 8 : 0;
    }
}

// the draw: smallest index i with key_i >= tau whose inclusive weight sum exceeds u * Z_K, u = m24 * 2^-24
template <bool STAGED>
__device__ __forceinline__ int sm_draw(SmShared& S, const float* __restrict__ lg, const float* st, int vocab, float lmax, float T,
                                       unsigned tau, unsigned m24) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src = STAGED ? st : lg;
    const bool vec = (vocab & 3) == 0;
    const int chunk = (((vocab + SM_THREADS - 1) / SM_THREADS) + 3) & ~3;       // contiguous indices per thread, a multiple of 4
    const int i0 = tid * chunk, i1 = min(vocab, i0 + chunk);
    unsigned long long sum = 0ull;
    auto elem = [&](int i) -> unsigned long long {
        const float v = STAGED ? src[i] : sm_clean(src[i]);
        return sm_key(v) >= tau ? sm_weight(v, lmax, T) : 0ull;
    };
    if (vec) {
        for (int i = i0; i < i1; i += 4) {
            const f4 v4 = *(const f4*)(src + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = STAGED ? v4[j] : sm_clean(v4[j]);
                if (sm_key(v) >= tau) sum += sm_weight(v, lmax, T);
            }
        }
    } else {
        for (int i = i0; i < i1; ++i) sum += elem(i);
    }
    unsigned long long incl = sm_wave_scan(sum);
    if (lane == 63) S.wa[wave] = incl;
    if (tid == 0) { S.r_tok = -1; S.r_last = -1; }
    __syncthreads();
    unsigned long long total = 0ull;
    for (int w = 0; w < SM_THREADS / 64; ++w) {
        if (w < wave) incl += S.wa[w];
        total += S.wa[w];
    }
    // floor(m24 * total / 2^24) + 1 <= total: m24 < 2^24 and total >= 2^40 (the maximum is always kept)
    const unsigned long long thr = ((__umul64hi((unsigned long long)m24, total) << 40) | (((unsigned long long)m24 * total) >> 24)) + 1ull;
    if (incl >= thr && incl - sum < thr) {
        unsigned long long run = incl - sum;
        int tok = -1;
        for (int i = i0; i < i1 && tok < 0; ++i) {
            run += elem(i);
            if (run >= thr) tok = i;
        }
        S.r_tok = tok;
    }
    __syncthreads();
    if (S.r_tok < 0) {                                     // the definition's fallback: the largest kept index
        int last = -1;
        for (int i = i0; i < i1; ++i) {
            const float v = STAGED ? src[i] : sm_clean(src[i]);
            if (sm_key(v) >= tau) last = i;
        }
        if (last >= 0) atomicMax(&S.r_last, last);
        __syncthreads();
        return S.r_last < 0 ? 0 : S.r_last;
    }
    return S.r_tok;
}

// The pick for one row by the whole workgroup.  Every thread returns the token; *kept = |K|.  Ends behind a barrier.
template <bool STAGED>
__device__ __forceinline__ int sm_pick(SmShared& S, const float* __restrict__ lg, float* st, int vocab, const aur_sampling& prm, unsigned n,
                                       int* kept) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float T = prm.temperature;
    if (!(T > 0.f)) {                                      // temperature 0 (negative / NaN clamp to it): greedy, the first maximum
        *kept = 1;
        return row_first_argmax(lg, vocab, S.sv, S.si);
    }
    // pass 0: the row's maximum and smallest finite value; the staged copy
    float mx = -INFINITY, mn = INFINITY;
    auto take = [&](float v) {
        mx = fmaxf(mx, v);
        mn = fminf(mn, v == -INFINITY ? INFINITY : v);
    };
    if ((vocab & 3) == 0) {
        const int n4 = vocab >> 2;
        for (int i = tid; i < n4; i += SM_THREADS) {
            f4 v = *(const f4*)(lg + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = sm_clean(v[j]);
                take(v[j]);
            }
            if (STAGED) *(f4*)(st + 4 * i) = v;
        }
    } else {
        for (int i = tid; i < vocab; i += SM_THREADS) {
            const float v = sm_clean(lg[i]);
            take(v);
            if (STAGED) st[i] = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        mn = fminf(mn, __shfl_xor(mn, o));
    }
    if (lane == 0) { S.sv[wave] = mx; S.sv[16 + wave] = mn; }
    __syncthreads();
    for (int w = 0; w < SM_THREADS / 64; ++w) {
        mx = fmaxf(mx, S.sv[w]);
        mn = fminf(mn, S.sv[16 + w]);
    }
    __syncthreads();
    if (!(mx > -INFINITY && mx < INFINITY)) {              // no finite maximum: nothing to weigh, the greedy rule decides
        *kept = 1;
        return row_first_argmax(lg, vocab, S.sv, S.si);
    }
    const float range = mx - mn;
    const float scale = (range > 0.f && range < INFINITY) ? 255.0f / range : 0.f;
    const int k = prm.top_k < 0 ? 0 : prm.top_k;
    float p = prm.top_p;
    p = !(p <= 1.f) ? 1.f : (p > 0.f ? p : 1e-30f);        // p > 1 / NaN: off; p <= 0 keeps the maximum alone
    const bool k_on = k > 0 && k < vocab, p_on = p < 1.f;
    unsigned tau = 0u;
    unsigned long long cnt = (unsigned long long)vocab, zk = 0ull;
    if (k_on) sm_select<STAGED, false>(S, lg, st, vocab, mx, scale, T, (unsigned long long)k, 1.f, 0ull, tau, cnt, zk);
    if (p_on) {
        unsigned tp;
        unsigned long long cp, mp;
        sm_select<STAGED, true>(S, lg, st, vocab, mx, scale, T, 0ull, p, zk, tp, cp, mp);
        if (tp >= tau) { tau = tp; cnt = cp; }
    }
    *kept = (int)cnt;
    const unsigned m24 = sm_philox_x0(prm.seed, n, prm.stream) >> 8;
    const int tok = sm_draw<STAGED>(S, lg, st, vocab, mx, T, tau, m24);
    __syncthreads();
    return tok;
}

extern __shared__ __attribute__((aligned(16))) float sm_stage[];

template <bool STAGED>
__global__ __launch_bounds__(SM_THREADS) void sample_advance_kernel(const float* __restrict__ logits, int b0, int vocab,
                                                                    const aur_sampling* __restrict__ params,
                                                                    const half_t* __restrict__ embed, int d, int eos_id, int max_new,
                                                                    int32_t* __restrict__ out_ids, int32_t* __restrict__ out_len,
                                                                    int32_t* __restrict__ finished, int32_t* __restrict__ pos,
                                                                    half_t* __restrict__ xf, unsigned long long* __restrict__ ssq,
                                                                    int advance_pos, int set_pos, const int32_t* __restrict__ set_pos_lens,
                                                                    int len_cap) {
    __shared__ SmShared S;
    const int b = b0 + blockIdx.x;
    const aur_sampling prm = params[b];
    const unsigned n = (unsigned)out_len[b];               // index of the token being generated
    int kept;
    const int tok = sm_pick<STAGED>(S, logits + (int64_t)b * vocab, sm_stage, vocab, prm, n, &kept);
    __syncthreads();
    advance_tail(b, blockIdx.x, tok, embed, d, eos_id, max_new, out_ids, out_len, finished, pos, xf, ssq, advance_pos, set_pos, set_pos_lens,
                 len_cap, S.sv);
}

template <bool STAGED>
__global__ __launch_bounds__(SM_THREADS) void sample_rows_kernel(const float* __restrict__ logits, int vocab,
                                                                 const aur_sampling* __restrict__ params, const int32_t* __restrict__ n_dev,
                                                                 int32_t* __restrict__ tokens_out, int32_t* __restrict__ kept_out) {
    __shared__ SmShared S;
    const int b = blockIdx.x;
    const aur_sampling prm = params[b];
    int kept;
    const int tok = sm_pick<STAGED>(S, logits + (int64_t)b * vocab, sm_stage, vocab, prm, (unsigned)n_dev[b], &kept);
    if (threadIdx.x == 0) {
        tokens_out[b] = tok;
        if (kept_out) kept_out[b] = kept;
    }
}

hipError_t sample_init() {
    hipError_t e = hipFuncSetAttribute((const void*)sample_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_STAGE_MAX_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)sample_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_STAGE_MAX_BYTES);
}
static bool sm_staged(int vocab, int stage) { return stage && (int64_t)vocab * 4 <= SM_STAGE_MAX_BYTES; }

hipError_t launch_sample_advance(const float* logits, int b0, int nb, int vocab, const aur_sampling* params, const half_t* embed, int d,
                                 int eos_id, int max_new, int32_t* out_ids, int32_t* out_len, int32_t* finished, int32_t* pos, half_t* xf,
                                 unsigned long long* ssq, int advance_pos, int set_pos, hipStream_t s, const int32_t* set_pos_lens,
                                 int len_cap, int stage) {
    if (sm_staged(vocab, stage))
        hipLaunchKernelGGL(sample_advance_kernel<true>, dim3(nb), dim3(SM_THREADS), (size_t)vocab * 4, s, logits, b0, vocab, params, embed, d,
                           eos_id, max_new, out_ids, out_len, finished, pos, xf, ssq, advance_pos, set_pos, set_pos_lens, len_cap);
    else
        hipLaunchKernelGGL(sample_advance_kernel<false>, dim3(nb), dim3(SM_THREADS), 0, s, logits, b0, vocab, params, embed, d, eos_id,
                           max_new, out_ids, out_len, finished, pos, xf, ssq, advance_pos, set_pos, set_pos_lens, len_cap);
    return hipGetLastError();
}

hipError_t launch_sample_rows(const float* logits, int rows, int vocab, const aur_sampling* params, const int32_t* n_dev,
                              int32_t* tokens_out, int32_t* kept_out, hipStream_t s, int stage) {
    if (sm_staged(vocab, stage))
        hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(rows), dim3(SM_THREADS), (size_t)vocab * 4, s, logits, vocab, params, n_dev,
                           tokens_out, kept_out);
    else
        hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(rows), dim3(SM_THREADS), 0, s, logits, vocab, params, n_dev, tokens_out, kept_out);
    return hipGetLastError();
}
