"""Reference side of the attention-map tests (helpers, not collected): the fp64 definition of the record (aurora_amd/attn_map.py restated
in torch), an elementwise error bound derived from the kernels' stated arithmetic (csrc/attn_map.hip), and a plain fp32 emulator of that
arithmetic with mutation switches.  CPU torch only; nothing here imports the product package.  tests/attn_ref.py supplies the cases.

One record row: q [L, H, hd] (the step's queries of the L selected layers), k [L, H, nk, hd] (the keys of the sequence's pages, rows at
or beyond npos poison), npos visible keys, a window of W keys -> A [W]."""
import math
from collections import namedtuple

import torch

from tests.attn_ref import LOG2E

PAGE = 64
MUTATIONS = ("window", "tail", "newest", "last_page", "first_norm", "empty_join", "heads_sum", "layers_sum", "no_scale")

MapRef = namedtuple("MapRef", "a p max_arg a_max n_keys")


def definition_fp64(q, k, npos, window, scale=None):
    """MapRef(a [W] = mean over (l, h) of softmax_j(scale q . k_j) over keys [0, npos), columns at or beyond min(W, npos) zero;
    p [L, H, npos]; max_arg [L, H] = the largest |score scale log2(e)| over the visible keys; a_max [L, H] = the largest
    scale log2(e) sum_d |q_d k_jd| over them; n_keys = npos)"""
    q, k = q.double(), k.double()[..., :npos, :]
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = torch.einsum("lhd,lhjd->lhj", q, k) * scale
    p = torch.softmax(s, -1)
    a = torch.zeros(window, dtype=torch.float64)
    n = min(window, npos)
    a[:n] = p.mean((0, 1))[:n]
    a_max = (torch.einsum("lhd,lhjd->lhj", q.abs(), k.abs()) * scale * LOG2E).amax(-1)
    return MapRef(a, p, (s.abs() * LOG2E).amax(-1), a_max, npos)


def derived_bound(ref, window, hd, nsplit, delta=0.0, c32_scale=1.0):
    """Elementwise bound [W] on |kernel record - ref.a|, the sum of what the kernels' arithmetic allows.  Per key j, head h, layer l:

      c32 2^-23 p        c32 = n_keys + 2 max|arg| + 16 + 2 nsplit in units of 2^-24 relative, doubled because p's numerator and its
                         normaliser err independently: n_keys for the sums over the keys; max|arg| twice for the two exp2 arguments
                         s - M and m_p - M, whose terms are rounded to fp32 (an absolute error of |arg| 2^-24 in the exponent is that
                         relative error, times ln 2 < 1); 16 for the fixed number of other roundings (exp2 itself, the scale factor,
                         the division, the lane reductions); 2 nsplit for the join's exp2 weights and fused multiply-adds - the unit
                         joined is the 64-key page, so nsplit = ceil(n_keys / 64)
      2 hd 2^-24 A p     the score is accumulated in fp32 over hd products: its exponent moves by at most hd 2^-24 sum_d |q_d k_jd|
                         scale log2(e) <= hd 2^-24 A, A the largest such sum over the visible keys - once for the key, once for the
                         normaliser
      2 Delta p          RoPE on: the roped q and k are rounded to fp16 before they are stored (tests/attn_ref.py rope_delta)

    and on the mean: (H + 1 + L) 2^-24 mean p for the H - 1 additions over the heads, the L - 1 over the layers, the rounded weight
    1 / (H L) and the multiplication by it; 2^-120 absolute for a p that underflows fp32 (exp2 flushes below 2^-126).  c32_scale
    scales the c32 term alone: the CPU test also runs the emulator against c32_scale = 0.5."""
    L, H, npos = ref.p.shape
    c32 = ref.n_keys + 2 * ref.max_arg + 16 + 2 * nsplit
    rel = c32_scale * c32 * 2.0 ** -23 + 2 * hd * 2.0 ** -24 * ref.a_max + 2 * delta           # [L, H]
    per = (rel[..., None] * ref.p).mean((0, 1)) + (H + 1 + L) * 2.0 ** -24 * ref.p.mean((0, 1))
    b = torch.full((window,), 2.0 ** -120, dtype=torch.float64)
    n = min(window, npos)
    b[:n] += per[:n]
    return b


def worst_ratio(got, ref_a, bound):
    """max |got - ref| / bound; a non-finite record counts as infinitely wrong"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref_a).abs() / bound).max())


def emulate(q, k, npos, window, max_pages=None, scale=None, mut=()):
    """The arithmetic attn_map.hip states, restated plainly in fp32: scores accumulated in fp32 and scaled by the fp32 product
    scale x log2(e); per 64-key page the maximum and the sum of exp2(score - maximum) over its visible keys; per head the pages joined
    in the order 0, 1, .. (maximum, then fused multiply-adds of exp2(m_p - M) l_p); p = exp2(score - M) / sum; the heads added in
    order, times the fp32 weight 1 / (H L); the first layer stores, later layers add.

    mut: the errors the tests must catch - "window" (the last recorded column is lost: j < min(W, npos) - 1), "tail" (one key too many:
    j < npos + 1), "newest" (key npos - 1 is missing), "last_page" (the page that holds the newest key is ignored: a stale page count),
    "first_norm" (the normaliser of the first page only), "empty_join" (pages behind the context join as m = 0, l = 0 instead of being
    skipped; needs max_pages), "heads_sum" (heads summed instead of averaged), "layers_sum" (layers summed instead of averaged),
    "no_scale" (the 1 / sqrt(hd) is missing)."""
    assert set(mut) <= set(MUTATIONS)
    L, H, hd = q.shape
    nk = k.shape[-2]
    scale = hd ** -0.5 if scale is None else scale
    sc = torch.tensor(1.0 if "no_scale" in mut else scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    j = torch.arange(nk)
    ok = j < npos + (1 if "tail" in mut else 0)
    if "newest" in mut:
        ok = ok & (j != npos - 1)
    if "last_page" in mut:
        ok = ok & (j < (npos - 1) // PAGE * PAGE)
    n_vis = int(ok.nonzero().max()) + 1 if bool(ok.any()) else 0
    npages = (n_vis + PAGE - 1) // PAGE
    weight = torch.tensor(1.0 / ((1 if "heads_sum" in mut else H) * (1 if "layers_sum" in mut else L)), dtype=torch.float32)
    n_rec = min(window, npos) - (1 if "window" in mut else 0)
    out = torch.zeros(window, dtype=torch.float32)
    for l in range(L):
        s = (torch.einsum("hd,hjd->hj", q[l].float(), k[l].float()) * sc).masked_fill(~ok, -math.inf)      # [H, nk]
        ms, ls = [], []
        for p in range(npages):
            sp = s[:, p * PAGE:(p + 1) * PAGE]
            m = sp.amax(-1)
            ms.append(m)
            ls.append(torch.exp2(sp - m[:, None]).sum(-1))
        if "empty_join" in mut and max_pages is not None:
            for p in range(npages, max_pages):
                ms.append(torch.zeros(H))
                ls.append(torch.zeros(H))
        if not ms:
            return torch.full((window,), math.nan)
        M = torch.stack(ms).amax(0)
        den = torch.zeros(H)
        for m, lsum in zip(ms, ls):
            den = torch.exp2(m - M) * lsum + den
            if "first_norm" in mut:
                break
        acc = torch.zeros(nk)
        for h in range(H):
            acc = acc + torch.exp2(s[h] - M[h]) / den[h]
        acc = acc * weight
        n = max(min(n_rec, nk), 0)
        out[:n] = out[:n] + acc[:n]
    return out


# ---------------------------------------------------------------------------------------------------------------- a small Llama
def llama_qk(x, w, cfg, dtype=torch.float64, quant=None):
    """A plain restatement of the Llama decoder (HF modeling_llama: RMSNorm, rotate_half RoPE at position / rope_factor, causal
    softmax attention, SiLU MLP) over the rows x [T, d] of ONE sequence at positions 0 .. T - 1, evaluated in `dtype`.  quant: applied
    to every tensor the engine holds in fp16 (normed rows, roped q / k, v, the attention output, both residual sums, SiLU(gate) * up) -
    None for the definition, `lambda t: t.half().to(t.dtype)` for an fp16 forward.  Returns the roped (q, k), each [layers, H, T, hd]."""
    qz = quant or (lambda t: t)
    F = torch.nn.functional
    x = x.to(dtype)
    T, d = x.shape
    H = cfg["num_attention_heads"]
    hd = d // H
    eps = cfg["rms_norm_eps"]
    inv = 1.0 / (cfg["rope_theta"] ** (torch.arange(0, hd, 2, dtype=dtype) / hd))
    ang = (torch.arange(T, dtype=dtype) / cfg.get("rope_factor", 1.0))[:, None] * inv[None, :]
    cos, sin = torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()
    rot = lambda t: torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1)
    norm = lambda t, g: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * g.to(dtype)
    causal = torch.arange(T)[None, :] > torch.arange(T)[:, None]
    qs, ks = [], []
    for l in w["layers"]:
        W = {n: t.to(dtype) for n, t in l.items()}
        h = qz(norm(x, W["input_layernorm.weight"]))
        heads = lambda name: F.linear(h, W[name + ".weight"]).view(T, H, hd).transpose(0, 1)
        qq, kk, vv = heads("q_proj"), heads("k_proj"), qz(heads("v_proj"))
        qq, kk = qz(qq * cos + rot(qq) * sin), qz(kk * cos + rot(kk) * sin)
        qs.append(qq)
        ks.append(kk)
        s = (qq @ kk.transpose(-1, -2)) / math.sqrt(hd)
        o = (torch.softmax(s.masked_fill(causal[None], -math.inf), -1) @ vv).transpose(0, 1).reshape(T, d)
        x = qz(x + F.linear(qz(o), W["o_proj.weight"]))
        h = qz(norm(x, W["post_attention_layernorm.weight"]))
        x = qz(x + F.linear(qz(F.silu(F.linear(h, W["gate_proj.weight"])) * F.linear(h, W["up_proj.weight"])), W["down_proj.weight"]))
    return torch.stack(qs), torch.stack(ks)


def teacher_forced_maps(emb, ids, w, cfg, window, layers=None, quant=None):
    """The records of a caption whose prompt rows are emb [Lp, d] and whose generated ids are `ids`, from `llama_qk` in fp64 over the
    prompt followed by the embeddings of ids[:-1]: row i >= 1 belongs to the step at position Lp + i - 1 (the input is token i - 1),
    which sees Lp + i keys; row 0 is zeros.  layers: the selected layers (None = all).
    Returns (maps float64 [n, W], bounds float64 [n, W] - `derived_bound` of every row with its RoPE term)."""
    n, Lp = len(ids), emb.shape[0]
    full = torch.cat([emb.double(), w["embed_tokens.weight"][torch.tensor(ids[:-1], dtype=torch.long)].double()], 0) if n > 1 else emb.double()
    q, k = llama_qk(full, w, cfg, torch.float64, quant)
    sel = list(range(q.shape[0])) if layers is None else list(layers)
    q, k = q[sel], k[sel]
    hd = q.shape[-1]
    maps, bounds = torch.zeros(n, window, dtype=torch.float64), torch.full((n, window), 2.0 ** -120, dtype=torch.float64)
    for i in range(1, n):
        pos = Lp + i - 1
        ref = definition_fp64(q[:, :, pos], k, pos + 1, window)
        delta = 2.0 ** -10 * hd ** -0.5 * float(torch.einsum("lhd,lhjd->lhj", q[:, :, pos].abs(), k[:, :, :pos + 1].abs()).max())
        maps[i] = ref.a
        bounds[i] = derived_bound(ref, window, hd, (pos + 64) // 64, delta)
    return maps, bounds
