"""Reference side of the attention kernel tests (helpers, not collected): the fp64 definition of masked softmax attention, an
elementwise error bound derived from the kernels' stated arithmetic, a plain fp32 / fp16 emulator of that arithmetic with mutation
switches, and the case builders.  CPU torch only; nothing here imports the product package.

One (sequence, head) is a triple q [nq, hd], k [nk, hd], v [nk, hd]; leading dimensions broadcast.  Key j is visible to query i when
j < n_valid and, under a causal mask, j <= q_pos0 + i."""
import math
from collections import namedtuple

import torch

LOG2E = 1.4426950408889634
POISON_V = 1000.0
# each side of the 16-key tile, the 32-row wave, the 64-key block and the 128-row workgroup of attn_kernel
T_LIST = (1, 15, 16, 17, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)
# tokens already cached when the decode step runs: each side of the 16-token fragment row and of the 64-token page, up to five pages
DEC_POS = (0, 1, 15, 16, 62, 63, 64, 65, 127, 128, 129, 191, 255, 256, 300, 319)
FLASH_CASES = ("rand", "sharp", "ascending", "descending", "peak", "sink", "future")
DEC_CASES = ("rand", "sharp", "ascending", "descending", "peak", "sink", "newest")
MUTATIONS = ("causal", "tail", "newest", "last_page", "empty_join", "never_rescale")


def rup(x, m):
    return (x + m - 1) // m * m


def flash_shapes():
    """(n_valid, rows): rows = round_up(n_valid, 32), and n_valid + 32 where n_valid is a multiple of 32, so that a poison key sits
    exactly at the first slot of a 32-row tile / a 64-key block"""
    out = []
    for t in T_LIST:
        out.append((t, rup(t, 32)))
        if t % 32 == 0:
            out.append((t, t + 32))
    return out


def visible(nq, nk, causal, n_valid, q_pos0=0):
    j = torch.arange(nk)[None, :]
    ok = (j < n_valid).expand(nq, nk)
    if causal:
        ok = ok & (j <= torch.arange(nq)[:, None] + q_pos0)
    return ok


# ---------------------------------------------------------------------------------------------------------------- RoPE
def rope_angles(pos, hd, theta, factor, dtype=torch.float64):
    """the table formula of aur_finalize: angle[p, i] = (p / rope_factor) * theta^(-2 i / hd), i < hd / 2"""
    i = torch.arange(hd // 2, dtype=dtype)
    inv = 1.0 / torch.pow(torch.tensor(theta, dtype=dtype), 2 * i / hd)
    return (torch.as_tensor(pos, dtype=dtype)[:, None] / factor) * inv[None, :]


def rope_apply(x, pos, theta, factor, dtype=torch.float64):
    """HF rotate_half on x [..., n, hd] at positions pos [n]: (x1, x2) -> (x1 cos - x2 sin, x2 cos + x1 sin), evaluated in `dtype`"""
    hd = x.shape[-1]
    ang = rope_angles(pos, hd, theta, factor, dtype)
    c, s = torch.cos(ang), torch.sin(ang)
    x = x.to(dtype)
    x1, x2 = x[..., : hd // 2], x[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def rope_delta(q, k, scale, ok):
    """Delta = 2^-10 * scale * max over visible (i, j) of sum_d |q_id k_jd|: what rounding the roped q and the roped k to fp16 (2^-11
    relative each) can move a score by, in nats"""
    a = q.abs().double() @ k.abs().double().transpose(-1, -2)
    return 2.0 ** -10 * scale * float(a.masked_fill(~ok, 0.0).max())


# ---------------------------------------------------------------------------------------------------------------- the definition
Ref = namedtuple("Ref", "o pv_abs max_arg p n_keys v_max")


def attention_fp64(q, k, v, scale, causal, n_valid, q_pos0=0):
    """softmax(scale q k^T + mask) v in fp64.  Returns Ref(o [.., nq, hd], pv_abs = sum_j p_j |v_jd| [.., nq, hd], max_arg = the largest
    |s scale log2(e)| over the visible scores of each query [.., nq], p [.., nq, nk], n_keys = visible keys per query [nq], v_max =
    max over j < n_valid of |v_jd| [.., 1, hd])"""
    q, k, v = q.double(), k.double(), v.double()
    nq, nk = q.shape[-2], k.shape[-2]
    ok = visible(nq, nk, causal, n_valid, q_pos0)
    s = (q @ k.transpose(-1, -2)) * scale
    max_arg = (s.abs() * LOG2E).masked_fill(~ok, 0.0).amax(-1)
    p = torch.softmax(s.masked_fill(~ok, -math.inf), -1)
    return Ref(p @ v, p @ v.abs(), max_arg, p, ok.sum(-1).double(), v[..., :n_valid, :].abs().amax(-2, keepdim=True))


def derived_bound(ref, nsplit=1, delta=0.0, c32_scale=1.0):
    """Elementwise bound on |kernel output - ref.o| [.., nq, hd], the sum of what the kernels' arithmetic allows (attn.hip attn_kernel;
    decode.hip decode_attn_dot_kernel + decode_attn_combine_kernel).  P|V| = ref.pv_abs.

      2^-11 |o| (+ 2^-25 where |o| < 2^-14)   the output is rounded to fp16 once; below 2^-14 fp16 is subnormal, spacing 2^-24
      2^-11 P|V|                              p is rounded to fp16 once before the P V product in both kernels (`pf` / `p16`): a relative
                                              error of 2^-11 per key, weighted by |v|; the normalising sum takes the unrounded p
      n_keys 2^-25 max_j |v_jd|               p below 2^-14 is an fp16 subnormal or zero: up to 2^-25 absolute per key instead.  The
                                              normaliser is >= 1 (the maximal key contributes p = 1), so this is not magnified
      c32 2^-23 P|V|                          everything done in fp32, c32 = n_keys + max|arg| + 16 + 2 nsplit counted in units of
                                              2^-24 relative and doubled because numerator and normaliser err independently: n_keys
                                              for the running sums over the keys (numerator and denominator each add one term per key),
                                              max|arg| for the exp2 argument (s scale log2e and m scale log2e are rounded to fp32: an
                                              absolute error of |arg| 2^-24 in the exponent is that relative error in p, times ln 2 < 1),
                                              16 for the fixed number of other roundings (exp2 itself, alpha per block amortised by the
                                              geometric decay of old blocks, the reciprocal, the lane reductions), 2 nsplit for the
                                              combine's exp2 weights and fused multiply-adds
      2 Delta P|V|                            RoPE on: the roped q and k are rounded to fp16 before they are stored; Delta = rope_delta()
                                              bounds the score movement in nats, p moves by e^Delta - 1 ~ Delta relative and so does the
                                              normaliser.  (The table itself is fp32: its angle, up to 80 rad here, carries ~1e-5 of
                                              absolute error against the 4.9e-4 relative of an fp16 rounding - about 2 % of this term,
                                              inside what the worst case over d leaves unused; not counted.)

    The fp32 accumulation of a score over hd <= 128 products moves the exp2 argument by at most hd 2^-24 sum_d |q_d k_d| scale log2(e);
    at the keys that carry weight that sum is of the order of |arg| itself in every case here, so it sits under max|arg| and the 16.
    The emulator accumulates its scores in fp32 too and stays inside.  c32_scale scales the c32 term alone: the CPU test also runs the
    emulator against c32_scale = 0.5, to show that this coefficient is not what keeps it inside."""
    o = ref.o.abs()
    pv = ref.pv_abs
    b = 2.0 ** -11 * o + (o < 2.0 ** -14) * 2.0 ** -25
    b = b + 2.0 ** -11 * pv
    b = b + ref.n_keys[..., None] * 2.0 ** -25 * ref.v_max
    c32 = ref.n_keys + ref.max_arg + 16 + 2 * nsplit
    b = b + c32_scale * c32[..., None] * 2.0 ** -23 * pv
    return b + 2.0 * delta * pv


def worst_ratio(got, ref_o, bound):
    """max |got - ref| / bound; a non-finite output counts as infinitely wrong"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref_o).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------------- the emulator
def emulate(q, k, v, scale, causal, n_valid, q_pos0=0, ranges=None, mut=()):
    """The arithmetic both kernels state, restated plainly: fp32 scores, online softmax over blocks of 64 keys with the running maximum
    and sum in fp32, p rounded to fp16 for the P V product, fp32 accumulation, fp16 output.  ranges = [(k0, k1), ..] splits the keys into
    page ranges that are reduced independently and joined in fp32 like decode_attn_combine_kernel (an empty range is skipped).

    mut: the errors the GPU test must catch - "causal" (key <= query + 1), "tail" (key < n_valid + 1), "newest" (the newest key,
    n_valid - 1, is missing), "last_page" (the 64-key page that holds the newest key is ignored), "empty_join" (an empty range joins
    as m = 0, l = 0 instead of being skipped), "never_rescale" (the running sums are not rescaled when the maximum moves)."""
    assert set(mut) <= set(MUTATIONS)
    qf, kf, vf = q.float(), k.float(), v.float()
    nq, nk = qf.shape[-2], kf.shape[-2]
    j = torch.arange(nk)[None, :]
    ok = (j < n_valid + (1 if "tail" in mut else 0)).expand(nq, nk)
    if causal:
        ok = ok & (j <= torch.arange(nq)[:, None] + q_pos0 + (1 if "causal" in mut else 0))
    if "newest" in mut:
        ok = ok & (j != n_valid - 1)
    if "last_page" in mut:
        ok = ok & (j < (n_valid - 1) // 64 * 64)
    s = (qf @ kf.transpose(-1, -2)).masked_fill(~ok, -math.inf)
    sc = torch.tensor(scale * LOG2E, dtype=torch.float32)
    parts = []
    for k0, k1 in (ranges or [(0, nk)]):
        m = torch.full(s.shape[:-1], -math.inf)
        l = torch.zeros(s.shape[:-1])
        acc = torch.zeros(*s.shape[:-1], vf.shape[-1])
        for b0 in range(k0, min(k1, nk), 64):
            b1 = min(b0 + 64, k1, nk)
            sb = s[..., b0:b1]
            m_new = torch.maximum(m, sb.amax(-1))
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            p = torch.exp2(sb * sc - (m_use * sc)[..., None])
            alpha = torch.ones_like(m) if "never_rescale" in mut else torch.exp2((m - m_use) * sc)
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + p.half().float() @ vf[..., b0:b1, :]
            m = m_new
        parts.append((m * sc, l, acc))
    if len(parts) == 1:
        return (parts[0][2] / parts[0][1][..., None]).half()
    ms = torch.stack([p[0] for p in parts])
    if "empty_join" in mut:
        ms = torch.where(torch.isinf(ms), torch.zeros_like(ms), ms)
    w = torch.exp2(ms - ms.amax(0))                         # exp2(-inf) = 0: an empty range adds nothing
    num = sum(w[i][..., None] * parts[i][2] for i in range(len(parts)))
    den = sum(w[i] * parts[i][1] for i in range(len(parts)))
    return (num / den[..., None]).half()


def split_ranges(max_pages, pps):
    """the key ranges of the decode attention's splits: `pps` pages of 64 tokens each, ceil(max_pages / pps) of them"""
    return [(p * 64, min(p + pps, max_pages) * 64) for p in range(0, max_pages, pps)]


# ---------------------------------------------------------------------------------------------------------------- cases
def _h16(t):
    return t.half().float()


def build_case(name, hd, n_valid, rows, seed, rope_safe=False):
    """q, k, v [rows, hd], every value fp16-representable.  b = sqrt(hd) / log2(e) is the raw score worth one bit of the exp2 argument.

      rand        N(0, 1)
      sharp       q x 4, k x 2: peaked rows, the running maximum moves often
      ascending   score = j bits (dimension 0; the rest N(0, 1/16)): the maximum moves in every block, the last visible key wins
      descending  score = -(j + 160) bits: the maximum never moves after the first block; every score is far below zero, so joining an
                  empty split as m = 0 underflows every weight
      peak        score = -|j - c| bits, c = min(n_valid - 1, 96): the maximum moves by tens of bits from the first 64-key page to the second
                  and the keys behind it still carry the row - a decode split of two or more pages that does not rescale its sums is
                  caught even when later splits exist (ascending puts all weight in the LAST split, descending never moves the maximum)
      sink        key 0 is 40 bits above the rest and V[0] is small (x 2^-6): the other keys' p underflows fp16
      future      q_i = (i / 16, 1, ..), k_j = (-c, c j / 16, ..): score = c (j - i) / 16 grows with key - query.  c is the power of two with
                  c / 16 at least 8 bits (so every value is exact in fp16; a step is 8 .. 16 bits).  Causal only: the diagonal key wins,
                  the output is about V[i], and any leaked future key takes the row
      newest      key n_valid - 1 is 16 bits above the rest: a decode step whose own K / V is missing or late loses the row

    Dimension hd - 1 is the poison dimension: q = 1 on every row, k = 0 on valid rows.  Rows at or beyond n_valid are poison: k = 200
    sqrt(hd) in that dimension - 200 nats (288 bits) above zero for every query, above every visible score of every case - and v = 1000.
    Finite values only.  rope_safe: q and the valid k are scaled so that |q_i| |k_j| scale <= 2 (the poison keeps 200 f nats, f ~ 0.4)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(rows, hd, generator=g) for _ in range(3))
    b = math.sqrt(hd) / LOG2E
    j = torch.arange(rows, dtype=torch.float32)
    if name == "sharp":
        q, k = q * 4, k * 2
    elif name in ("ascending", "descending"):
        q, k = q * 0.25, k * 0.25
        q[:, 0] = 1.0
        k[:, 0] = j * b if name == "ascending" else -(j + 160) * b
    elif name == "peak":
        q, k = q * 0.25, k * 0.25
        q[:, 0] = 1.0
        k[:, 0] = -(j - min(n_valid - 1, 96)).abs() * b
    elif name == "sink":
        q, k = q * 0.5, k * 0.5
        q[:, 0], k[:, 0] = 1.0, 0.0
        k[0, 0] = 40 * b
        v[0] *= 2.0 ** -6
    elif name == "future":
        c = 2.0 ** math.ceil(math.log2(128 * b))
        q, k = q * 0.25, k * 0.25
        q[:, 0], q[:, 1] = j / 16, 1.0
        k[:, 0], k[:, 1] = -c, c * j / 16
    elif name == "newest":
        q, k = q * 0.5, k * 0.5
        q[:, 0], k[:, 0] = 1.0, 0.0
        k[n_valid - 1, 0] = 16 * b
    else:
        assert name == "rand", name
    q[:, hd - 1], k[:, hd - 1] = 1.0, 0.0
    if rope_safe:
        q, k = _h16(q), _h16(k)
        f = 0.98 * math.sqrt(2.0 * math.sqrt(hd) / float(q.norm(dim=-1).max() * k[:n_valid].norm(dim=-1).max()))
        q, k = q * f, k * f
    k[n_valid:] = 0.0
    k[n_valid:, hd - 1] = 200.0 * math.sqrt(hd)
    v[n_valid:] = POISON_V
    return _h16(q), _h16(k), _h16(v)
