// Per-token attention over a prefix window of the context, recorded inside the decode step (aur_attn_map_enable; definition:
// aurora_amd/attn_map.py).  For the decode step that picks generated token i >= 1 of a slot:
//   A[i, j] = mean over the selected layers l and all heads h of softmax_j(scale q_lh . k_j) over keys [0, npos = pos + 1), j < min(W, npos)
// and exactly 0.0 for min(W, npos) <= j < W.  decode_attn_dot_kernel never holds a probability and sits at its register limit, so the record
// has kernels of its own: one more pass over K per recorded layer (V is never read), launched behind the layer's QKV projection.
//
//   attn_map_score_kernel   one wave per (slot, head, 64-token page), the K fragments read with decode_attn_dot_kernel's lane layout: lane
//                           (g, r) holds token kt * 16 + r x the 8 PAIRED dims of group g, 4 v_dot2 per fragment into one fp32 per (lane, kt),
//                           the 4 dim groups of a token meet by the xor 16 / xor 32 row exchanges, lane l owns token l of the page.  Writes
//                           the scaled log2-domain score of every key of a page inside the window (4 B per (head, key): a second pass over
//                           K instead would re-read 256 B per (head, key) at hd 128) and the page's (max, sum of exp2(score - max)).
//   attn_map_join_kernel    one lane per (slot, key of the window): per head, the pages joined in the fixed order p = 0, 1, .. (maximum, then
//                           fused multiply-adds of exp2(m_p - M) l_p), p = exp2(score - M) / sum, the heads added in the order h = 0, 1, ..,
//                           times 1 / (heads x layers).  The first selected layer stores the row, later layers add to it in stream order,
//                           and the lane that owns an element is the only one that touches it.
// The unit of the partial sums is the PAGE, not the decode attention's split: the record does not depend on dec_attn_pps / dec_attn_local,
// on the batch, the slot, the bank or the launch form - no atomics, no order that scheduling decides.  A page at or beyond
// ceil(npos / 64) is never dereferenced (its page-table entry may be stale); the window may be longer than the context.
#include "kernels.h"

template <int KBLK>
__global__ __launch_bounds__(64) void attn_map_score_kernel(AttnMapArgs a) {
    const int lane = threadIdx.x;
    const int g = lane >> 4, r = lane & 15;
    const int p = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    if (a.s_len) {                                       // decode step: a slot that takes no token records nothing
        const int len = a.s_len[b];
        if (a.s_fin[b] || len < 1 || len >= a.max_new) return;
    }
    const int npos = a.pos[b] + 1;
    if (p >= ((npos + 63) >> 6)) return;                 // wave-uniform: pages behind the context are never looked up
    const KvLayout& kv = a.kv;
    const int64_t bh = (int64_t)b * a.heads + head;
    h8 qf[KBLK];
#pragma unroll
    for (int blk = 0; blk < KBLK; ++blk) qf[blk] = *(const h8*)(a.qbuf + ((bh * KBLK + blk) * 4 + g) * 8);
    const half_t* page = kv_page(kv, b, p * 64) + kfrag_off(kv, head, 0, 0) + lane * 8;
    h8 kf[4 * KBLK];
#pragma unroll
    for (int i = 0; i < 4 * KBLK; ++i) kf[i] = *(const h8*)(page + i * AUR_FRAG_HALVES);
    const float sc = a.scale * 1.4426950408889634f;
    float s[4];
    float mx = -INFINITY, mine = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        float v = 0.f;
#pragma unroll
        for (int blk = 0; blk < KBLK; ++blk) {
            const h8 k8 = kf[kt * KBLK + blk], q8 = qf[blk];
            v = __builtin_amdgcn_fdot2(h2{k8[0], k8[1]}, h2{q8[0], q8[1]}, v, false);
            v = __builtin_amdgcn_fdot2(h2{k8[2], k8[3]}, h2{q8[2], q8[3]}, v, false);
            v = __builtin_amdgcn_fdot2(h2{k8[4], k8[5]}, h2{q8[4], q8[5]}, v, false);
            v = __builtin_amdgcn_fdot2(h2{k8[6], k8[7]}, h2{q8[6], q8[7]}, v, false);
        }
        v = xor16_sum(v);                                // the 4 dim groups of token kt * 16 + r: all 4 lanes get the same bits
        v = xor32_sum(v);
        v = (p * 64 + kt * 16 + r) < npos ? v * sc : -INFINITY;
        s[kt] = v;
        mx = fmaxf(mx, v);
        mine = kt == g ? v : mine;                       // lane l = g * 16 + r publishes token l of the page
    }
    mx = row16_max(mx);                                  // finite: key p * 64 is inside the context
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) l += __builtin_amdgcn_exp2f(s[kt] - mx);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) l += __shfl_xor(l, o, 64);      // over the 16 token lanes; the 4 groups hold the same sum
    if (p * 64 < a.window) a.score[bh * a.window + p * 64 + lane] = mine;
    if (lane == 0) {
        float* ml = a.page_ml + (bh * kv.max_pages + p) * 2;
        ml[0] = mx;
        ml[1] = l;
    }
}

__global__ __launch_bounds__(64) void attn_map_join_kernel(AttnMapArgs a) {
    __shared__ float sM[AUR_ATTN_MAP_MAX_HEADS], sL[AUR_ATTN_MAP_MAX_HEADS];
    const int lane = threadIdx.x, b = blockIdx.y, j = blockIdx.x * 64 + lane;
    int row = 0;
    if (a.s_len) {
        row = a.s_len[b];
        if (a.s_fin[b] || row < 1 || row >= a.max_new) return;       // block-uniform
    }
    const int npos = a.pos[b] + 1;
    float* dst = a.out + ((int64_t)b * a.max_new + row) * a.window + j;
    if (blockIdx.x * 64 >= npos) {                       // a whole block behind the context
        if (a.first) *dst = 0.f;
        return;
    }
    int npages = (npos + 63) >> 6;
    npages = npages < a.kv.max_pages ? npages : a.kv.max_pages;      // the score kernel's grid: pages a sequence can hold
    for (int h = lane; h < a.heads; h += 64) {
        const float* ml = a.page_ml + ((int64_t)b * a.heads + h) * a.kv.max_pages * 2;
        float M = -INFINITY, den = 0.f;
        for (int p = 0; p < npages; ++p) M = fmaxf(M, ml[p * 2]);
        for (int p = 0; p < npages; ++p) den = __builtin_fmaf(__builtin_amdgcn_exp2f(ml[p * 2] - M), ml[p * 2 + 1], den);
        sM[h] = M;
        sL[h] = den;
    }
    __syncthreads();
    float acc = 0.f;
    if (j < npos) {
        const float* sc = a.score + (int64_t)b * a.heads * a.window + j;
        for (int h = 0; h < a.heads; ++h) acc += __builtin_amdgcn_exp2f(sc[(int64_t)h * a.window] - sM[h]) / sL[h];
        acc *= a.weight;
    }
    if (a.first) *dst = acc;
    else if (j < npos) *dst += acc;
}

hipError_t launch_attn_map(const AttnMapArgs& a, hipStream_t s) {
    if (a.kv.page_tokens != 64 || a.window < 64 || (a.window & 63) || a.heads < 1 || a.heads > AUR_ATTN_MAP_MAX_HEADS || a.B < 1)
        return hipErrorInvalidValue;
    const dim3 grid(a.kv.max_pages, a.heads, a.B);
    if (a.kv.kblk == 4) hipLaunchKernelGGL((attn_map_score_kernel<4>), grid, dim3(64), 0, s, a);
    else if (a.kv.kblk == 2) hipLaunchKernelGGL((attn_map_score_kernel<2>), grid, dim3(64), 0, s, a);
    else if (a.kv.kblk == 1) hipLaunchKernelGGL((attn_map_score_kernel<1>), grid, dim3(64), 0, s, a);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(attn_map_join_kernel, dim3(a.window / 64, a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}
