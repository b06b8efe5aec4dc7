// Stop conditions behind the token pick: stop token ids, stop strings and a per-request budget, tested on the
// device because the decode step is a captured graph and the host looks at a slot only every check_every steps.  aurora_amd/stopping.py
// is the definition; the record and the byte table are described at aur_stop_rules / aur_stop_vocab (include/aurora_hip.h).
//
// stop_check_kernel: one wave per slot, behind whichever pick ran.  A slot whose `finished` flag is set - it finished earlier, or the pick
// just saw the EOS or filled the output row - is skipped: nothing of it is read or written.  For an unfinished slot with n >= 1
// generated tokens, t = h[n - 1]:
//   1. budget and stop ids on t;
//   2. the text window into LDS: t's bytes at s_txt[FRONT ..), and in front of them the last (longest string - 1) bytes of the tokens
//      before t - no earlier byte can belong to an occurrence that ends inside t.  The walk back through out_ids takes 64 tokens at a
//      time, one per lane (ids, then spans, then bytes: three dependent loads per 64 tokens, not per token); a wave scan of the token
//      lengths places each lane's bytes; an id outside the table ends the text there;
//   3. every (string, end offset inside t) pair, one pair per lane and round.
// A hit sets finished[b] = 1 and nothing else: pos, the next-token embedding and out_len are already what advance_tail leaves for an
// EOS.  Plain loads and vector stores; no atomics.  Everything the host cannot see is clamped: counts into [0, 8], string lengths
// into [0, 64], token spans into the byte table, a token to 255 bytes.
#include "../../include/aurora_hip.h"
#include "kernels.h"

#define STOP_THREADS 64
#define STOP_FRONT (AUR_STOP_MAX_STRING_BYTES - 1)

__device__ __forceinline__ int stop_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bytes [start, start + len) of token `tok`; false: an id outside the table (no bytes, and the text breaks there)
__device__ __forceinline__ bool stop_span(int tok, const int32_t* __restrict__ off, int vocab, int nbytes, int& start, int& len) {
    start = 0;
    len = 0;
    if (!off || tok < 0 || tok >= vocab) return false;
    const int a = stop_clamp(off[tok], 0, nbytes), e = stop_clamp(off[tok + 1], a, nbytes);
    start = a;
    len = e - a > AUR_STOP_MAX_TOKEN_BYTES ? AUR_STOP_MAX_TOKEN_BYTES : e - a;
    return true;
}

__global__ __launch_bounds__(STOP_THREADS) void stop_check_kernel(int b0, const aur_stop_rules* __restrict__ rules,
                                                                  const int32_t* __restrict__ ids, int ids_stride,
                                                                  const int32_t* __restrict__ lens, int batch_max_new,
                                                                  int32_t* __restrict__ finished, const int32_t* __restrict__ off,
                                                                  const uint8_t* __restrict__ bytes, int vocab, int nbytes) {
    __shared__ __align__(8) uint8_t s_str[AUR_STOP_MAX_STRINGS * AUR_STOP_MAX_STRING_BYTES];
    __shared__ uint8_t s_txt[STOP_FRONT + AUR_STOP_MAX_TOKEN_BYTES + 2];
    const int b = b0 + blockIdx.x, lane = threadIdx.x;
    if (finished[b] != 0) return;
    const int n = stop_clamp(lens[b], 0, ids_stride);
    if (n < 1) return;
    const aur_stop_rules* r = rules + b;
    const int32_t* h = ids + (int64_t)b * ids_stride;
    const int t = h[n - 1];
    // 1. budget (<= 0: the batch's) and stop ids
    const int budget = r->max_new_tokens > 0 ? r->max_new_tokens : batch_max_new;
    bool hit = n >= budget || n >= batch_max_new;
    const int nid = stop_clamp(r->n_token_ids, 0, AUR_STOP_MAX_IDS), nstr = stop_clamp(r->n_strings, 0, AUR_STOP_MAX_STRINGS);
    if (lane < nid) hit = hit || r->token_ids[lane] == t;
    int maxlen = 0;
    for (int i = 0; i < nstr; ++i) {
        const int L = stop_clamp(r->string_len[i], 0, AUR_STOP_MAX_STRING_BYTES);
        maxlen = L > maxlen ? L : maxlen;
    }
    int ts, Lt;
    const bool t_ok = stop_span(t, off, vocab, nbytes, ts, Lt);
    if (maxlen > 0 && t_ok && Lt > 0) {                                      // uniform: a token of zero bytes completes nothing
        // 2. the window: the strings (8 bytes per lane), t's bytes, then the bytes in front of t
        ((uint2*)s_str)[lane] = ((const uint2*)&r->strings[0][0])[lane];
        for (int i = lane; i < Lt; i += STOP_THREADS) s_txt[STOP_FRONT + i] = bytes[ts + i];
        const int need = maxlen - 1;                                         // <= STOP_FRONT
        int front = 0;
        for (int j = n - 2; front < need && j >= 0; j -= STOP_THREADS) {     // uniform: lane i holds token j - i
            const int jj = j - lane;
            int s0 = 0, len = 0;
            const bool ok = jj >= 0 && stop_span(h[jj], off, vocab, nbytes, s0, len);
            const unsigned long long brk = __ballot(!ok);                    // the history's start ends the text like an unknown id does
            if (brk && lane >= __ffsll((long long)brk) - 1) len = 0;
            int inc = len;
#pragma unroll
            for (int o = 1; o < STOP_THREADS; o <<= 1) {
                const int v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            const int excl = inc - len, total = __shfl(inc, STOP_THREADS - 1);
            const int room = need - front - excl, take = len < room ? len : room;
            const int end = STOP_FRONT - front - excl;                       // end - take >= STOP_FRONT - need >= 0
            for (int k = 0; k < take; ++k) s_txt[end - take + k] = bytes[s0 + len - take + k];
            front += total < need - front ? total : need - front;
            if (brk) break;
        }
        __syncthreads();
        // 3. string si ending e bytes into t: it must begin inside the gathered text
        const int lo = STOP_FRONT - front;
        for (int p = lane; p < nstr * Lt && !hit; p += STOP_THREADS) {
            const int si = p / Lt, e = p % Lt + 1;
            const int L = stop_clamp(r->string_len[si], 0, AUR_STOP_MAX_STRING_BYTES), st = STOP_FRONT + e - L;
            if (L < 1 || st < lo) continue;
            bool same = true;
            for (int k = 0; k < L && same; ++k) same = s_txt[st + k] == s_str[si * AUR_STOP_MAX_STRING_BYTES + k];
            hit = same;
        }
    }
    if (__ballot(hit) && lane == 0) finished[b] = 1;
}

hipError_t launch_stop_check(int b0, int nb, const aur_stop_rules* rules, const int32_t* ids, int ids_stride, const int32_t* lens,
                             int batch_max_new, int32_t* finished, const int32_t* offsets, const uint8_t* bytes, int vocab, int64_t nbytes,
                             hipStream_t s) {
    const int nby = nbytes < 0 ? 0 : (nbytes > 0x7fffffff ? 0x7fffffff : (int)nbytes);        // int32 offsets cannot name more
    hipLaunchKernelGGL(stop_check_kernel, dim3(nb), dim3(STOP_THREADS), 0, s, b0, rules, ids, ids_stride, lens, batch_max_new, finished,
                       (offsets && bytes && vocab > 0) ? offsets : nullptr, bytes, vocab, nby);
    return hipGetLastError();
}
